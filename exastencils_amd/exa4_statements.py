"""Loop-body assignments of the ExaSlang-4 interpreter (mixin of exa4.Exa4Program): ONE recogniser says which kernel-layer call an
assignment stands for (`_recognise_assign` -> LoopStmt: a kind and the resolved operands), ONE launcher issues it (`_launch`; under a
multi-colouring `_launch_coloured`).  Everyone who needs to know what a statement is switches on the record -- the loop executors of
exa4.py, the smoother peepholes (exa4_peepholes.py: `_match_smoother`) and the pending loops of the cross-statement fusions
(exa4_fusion.py: `_try_defer`, `_consume_residual`; a pending loop IS its record and is flushed through `_launch`).  System rows,
point-wise set-up statements and semilinear operators are recognised in their mixins (exa4_systems.py, exa4_blocksys.py, exa4_nonlinear.py), which hand
back a record and launch nothing.  Recognition raises before anything is counted; `launches` is the launcher's.  Whole-loop forms
(reductions, stencil-field initialisation, rand / compare / check loops, `solve locally`) are not assignments of this kind and keep
their own code.  tests/test_exa4_calls.py pins the calls that come out of all this."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

from .exa4_common import APPLY, RESIDUAL, SMOOTH, _Frame
from .exa4_parser import Exa4Unsupported, _contains, _has_coord, _walk
from .field import Field, Stencil


@dataclass(frozen=True)
class LoopStmt:
    """What one assignment in a loop body launches.  kind: set | fill_fn | fill_expr | fill_expr_cell | copy | axpby | add_scalar |
    residual | apply | smooth | restrict | restrict_cell | prolong_add | prolong_add_cell | sys_row | pointwise_mul | pointwise_sub |
    bsys_row | nl_op | nl_smooth | axis_residual | axis_apply | axis_smooth | flux_step | reduce_expr | bc_face | v_set | v_axpby | v_op |
    v_smooth | v_restrict_cell | v_prolong_add_cell | v_components."""
    kind: str
    D: Field                        # the field assigned to
    ds: int
    U: Optional[Field] = None       # the field the loop reads: u of a stencil loop, x of axpby, the other level's field of a transfer
    us: int = 0
    F: Optional[Field] = None       # the right-hand side of a stencil loop; the second factor / the subtrahend of a point-wise statement
    fs: int = 0
    A: Optional[Stencil] = None
    s: float = 0.0                  # value of set / add_scalar, alpha of axpby, smoother weight, restriction scale, sign of pointwise_mul
    t: float = 0.0                  # beta of axpby
    prog: object = None             # compiled programs, function ids, system tables: whatever else the kind's call takes


class SmootherRefused(Exa4Unsupported):
    """The statement IS a damped-residual update, its weight is in no form the kernels evaluate: the one refusal that those who only
    ask what a statement is (`_recognise_or_none`) let through."""


class Statements:
    # pattern helpers ---------------------------------------------------------------------------------------------------
    def _is_scalar(self, e) -> bool:
        return not _contains(e, ("fld", "sten", "sentry")) and not self._over_position(e)

    def _over_position(self, e) -> bool:
        """Does the expression depend on the point: a coordinate, or -- on a non-uniform grid -- a width or the volume of its cell?"""
        return _has_coord(e, self.functions) or (self.grid is not None and self._reads_grid(e))

    def _same_access(self, a, b, fr: _Frame) -> bool:
        if a[0] != "fld" or b[0] != "fld":
            return False
        fa, sa = self._field(a, fr)
        fb, sb = self._field(b, fr)
        return fa is fb and sa == sb

    def _sten_times_field(self, e, fr: _Frame):
        """(scale, kind, stencil-or-name, stencil level, field expr) for `[s *] S * F`."""
        if e[0] != "bin" or e[1] != "*" or e[3][0] != "fld":
            return None
        s, scale = e[2], 1.0
        if s[0] == "bin" and s[1] == "*" and s[3][0] == "sten" and self._is_scalar(s[2]):
            scale, s = float(self._eval(s[2], fr)), s[3]
        if s[0] != "sten":
            return None
        if s[1] in self.transfer:
            factor = self.transfer_factor.get(s[1], 1.0)
            return (scale if factor == 1.0 else scale * factor), self.transfer[s[1]], s[1], None, e[3]
        return scale, "stencil", self.stencil(s[1], self._level_of(s[2], fr)), None, e[3]

    def _residual_form(self, e, fr: _Frame):
        """(F, A, U) for `F - A * U`."""
        if e[0] != "bin" or e[1] != "-" or e[2][0] != "fld":
            return None
        m = self._sten_times_field(e[3], fr)
        if m is None or m[1] != "stencil" or m[0] != 1.0:
            return None
        return e[2], m[2], m[4]

    def _smoother_weight(self, w, A: Stencil, fr: _Frame):
        """(omega, stencil as the kernel needs it): a stencil field carries the FORM of the weight -- the kernels evaluate per point
        what the statement says, `(1.0 / diag(A)) * omega` (Testing/SISC/3D_VarCoeff.exa4:145) or `omega / diag(A)`
        (Testing/PolyExpl/RBGS3Dvc.exa4:52); the two round differently."""
        axis = getattr(A, "is_axis", False)
        if A.cfield is None and not axis:
            return float(self._eval(w, fr)), A
        if (w[0] == "bin" and w[1] == "*" and w[2][0] == "bin" and w[2][1] == "/" and w[2][2] == ("num", 1.0)
                and w[2][3][0] == "call" and w[2][3][1] == "diag" and self._is_scalar(w[3])):
            return float(self._eval(w[3], fr)), A
        if w[0] == "bin" and w[1] == "/" and w[3][0] == "call" and w[3][1] == "diag" and self._is_scalar(w[2]):
            import dataclasses

            return float(self._eval(w[2], fr)), (A.with_wform(1) if axis else dataclasses.replace(A, wform=1))
        raise Exa4Unsupported("smoother weight on a stencil %s must read ((1.0 / diag(A)) * omega) or (omega / diag(A))"
                              % ("over the grid's virtual fields" if axis else "field"))

    # -- the recogniser -------------------------------------------------------------------------------------------------
    def _recognise_assign(self, st, fr: _Frame, colour=None) -> LoopStmt:
        """_recognise_plain, and the one thing that holds for every form: a stencil over the virtual fields of a non-uniform grid
        (grid.AxisStencil) stands in the three stencil loops only, which become kinds of their own -- no peephole, no fusion, no
        one-kernel solver and no coloured or lexicographic sweep asks for them; each runs as one examg_axis_op."""
        import dataclasses

        if self.grid is not None:
            for n in _walk(st[3]):
                sd = self._stencil_decls.get(n[1]) if n and n[0] == "sten" else None
                if sd is not None and any(self._reads_grid(e) and _contains(e, ("fld",)) for _, e in sd.entries):
                    raise Exa4Unsupported("stencil %s: a field in an entry of a stencil over the grid's virtual fields" % n[1])
        k = self._recognise_plain(st, fr, colour)
        if getattr(k.A, "has_complex_entries", False) and not k.kind.startswith("c_"):      # (flagged where the stencil is built: exa4.py)
            raise Exa4Unsupported("a stencil with complex entries on real field %s: real and complex mixed in one loop body" % k.D.name)
        if k.A is not None and getattr(k.A, "is_axis", False):
            if k.kind not in ("residual", "apply", "smooth"):
                raise Exa4Unsupported("a stencil over the grid's virtual fields in a %s statement" % k.kind)
            for X in (k.D, k.U, k.F):
                if X is not None and (X.layout.is_cell or X.layout.transform):
                    raise Exa4Unsupported("a stencil over the grid's virtual fields on the %s field %s"
                                          % ("cell" if X.layout.is_cell else "colour-split", X.name))
            return dataclasses.replace(k, kind="axis_" + k.kind)
        return k

    def _recognise_plain(self, st, fr: _Frame, colour=None) -> LoopStmt:
        """The record of the assignment `st` of a loop body, or the refusal that names why it is none of the kernels.  Scalars are
        evaluated here; nothing is launched or counted.  `colour`: the red-black colour of the loop, for the forms whose refusals
        depend on it (system rows, semilinear operators); what a smoother needs of it is checked where it is launched."""
        op, lhs, rhs = st[1], st[2], st[3]
        if self._has_vector and self._touches_vector(st):      # vector-valued cell fields: the kinds v_* (exa4_vector.py)
            return self._recognise_vector(st, fr, colour)
        if lhs[0] != "fld":
            raise Exa4Unsupported("loop body assigns to %s" % lhs[0])
        D, ds = self._field(lhs, fr)
        if D.layout.is_complex or self._reads_complex(rhs):      # complex fields: the kinds c_* (exa4_complex.py)
            if self._names_coef_expr(rhs):
                raise Exa4Unsupported("semilinear operator (coefficient-expression stencil) on complex field %s" % D.name)
            return self._recognise_complex(op, lhs, rhs, D, ds, fr)
        if self._names_coef_expr(rhs):
            return self._recognise_nonlinear(op, lhs, rhs, D, ds, colour, fr)
        if op == "=":
            if not _contains(rhs, ("fld", "sten", "sentry")):        # a scalar, or an expression over the position
                if not self._over_position(rhs):
                    return LoopStmt("set", D, ds, s=float(self._eval(rhs, fr)))
                if D.layout.is_cell:
                    return LoopStmt("fill_expr_cell", D, ds, prog=self._cell_program(rhs, D.level))
                fn, par = self._analytic(rhs, D.level)
                return LoopStmt("fill_fn", D, ds, prog=(fn, par)) if isinstance(fn, int) else LoopStmt("fill_expr", D, ds, prog=fn)
            if rhs[0] == "fld":
                return LoopStmt("copy", D, ds, *self._field(rhs, fr), s=1.0, t=0.0)
            k = (self._recognise_system_row(D, ds, rhs, colour, fr) or self._recognise_block_row(D, ds, rhs, colour, fr)
                 or (colour is None and self._recognise_pointwise(D, ds, rhs, fr)))
            if k:
                return k
            r = self._residual_form(rhs, fr)
            if r is not None:
                return LoopStmt("residual", D, ds, *self._field(r[2], fr), *self._field(r[0], fr), A=r[1])
            m = self._sten_times_field(rhs, fr)
            if m is not None:
                X, xs = self._field(m[4], fr)
                if m[1] in ("restriction", "cell_restriction"):
                    return self._transfer_stmt(m, +1, D, ds, X, xs)
                if m[1] == "stencil" and m[0] == 1.0:
                    return LoopStmt("apply", D, ds, X, xs, A=m[2])
            if rhs[0] == "bin" and rhs[1] == "+" and rhs[2][0] == "fld":
                # U_src + w * (F - A * U_src)   |   G + beta * D
                t = rhs[3]
                if t[0] == "bin" and t[1] == "*":
                    r = self._residual_form(t[3], fr)
                    if r is not None and self._same_access(rhs[2], r[2], fr):
                        return self._smoother_stmt(D, ds, rhs[2], t[2], r, fr)
                    if t[3][0] == "fld" and self._same_access(lhs, t[3], fr) and self._is_scalar(t[2]):
                        return LoopStmt("axpby", D, ds, *self._field(rhs[2], fr), s=1.0, t=float(self._eval(t[2], fr)))
        elif op in ("+=", "-="):
            sign = 1.0 if op == "+=" else -1.0
            if rhs[0] == "fld":          # x += y | x -= y  (y + (-1.0) * x is exactly y - x)
                return LoopStmt("axpby", D, ds, *self._field(rhs, fr), s=sign, t=1.0)
            if rhs[0] == "bin" and rhs[1] == "*":
                if rhs[3][0] == "fld" and self._is_scalar(rhs[2]):
                    return LoopStmt("axpby", D, ds, *self._field(rhs[3], fr), s=sign * float(self._eval(rhs[2], fr)), t=1.0)
                r = self._residual_form(rhs[3], fr)
                if r is not None and op == "+=" and self._same_access(lhs, r[2], fr):
                    return self._smoother_stmt(D, ds, lhs, rhs[2], r, fr)
                m = self._sten_times_field(rhs, fr)
                if m is not None and m[1] in ("prolongation", "cell_prolongation") and op == "+=" and m[0] == 1.0:
                    return self._transfer_stmt(m, -1, D, ds, *self._field(m[4], fr))
            # F += s | F -= s  (x + (-s) is exactly x - s).  Asked last, as it walks the whole expression: every form above names a field,
            # so a scalar matches none of them, and they evaluate nothing before they have seen theirs
            if self._is_scalar(rhs):
                return LoopStmt("add_scalar", D, ds, s=sign * float(self._eval(rhs, fr)))
        raise Exa4Unsupported("loop body statement is none of the recognised kernels: %s %s ..." % (lhs[1], op))

    def _recognise_or_none(self, st, fr: _Frame) -> Optional[LoopStmt]:
        """For those who ask what an assignment is without running it where it stands (peepholes, pending loops, the coloured loops):
        its record, None where the recogniser refuses it -- the plain path then meets the same statement and names the refusal."""
        try:
            return self._recognise_assign(st, fr)
        except SmootherRefused:
            raise
        except Exa4Unsupported:
            return None

    def _smoother_stmt(self, D: Field, ds: int, src, w, r, fr: _Frame) -> LoopStmt:
        U, us = self._field(src, fr)
        F, fs = self._field(r[0], fr)
        try:
            wv, A = self._smoother_weight(w, r[1], fr)
        except Exa4Unsupported as ex:
            raise SmootherRefused(str(ex)) from None
        return LoopStmt("smooth", D, ds, U, us, F, fs, A, wv)

    @staticmethod
    def _transfer_stmt(m, up: int, D: Field, ds: int, X: Field, xs: int) -> LoopStmt:
        """Restriction (`up` = +1: X is one level finer than D) or prolongation (-1) between two node fields or two cell fields."""
        cell = m[1].startswith("cell_")
        between = ("cell" if cell else "node", m[2], X.layout.localization, D.layout.localization)
        if cell != (X.layout.is_cell and D.layout.is_cell):
            raise Exa4Unsupported("%s restriction %s between %s and %s fields" % between) if up > 0 else \
                Exa4Unsupported("%s prolongation %s between %s and %s fields" % between)
        if X.level != D.level + up:
            raise Exa4Unsupported("restriction between levels %d and %d" % (X.level, D.level)) if up > 0 else \
                Exa4Unsupported("prolongation between levels %d and %d" % (X.level, D.level))
        return LoopStmt(("restrict" if up > 0 else "prolong_add") + ("_cell" if cell else ""), D, ds, X, xs, s=m[0])

    # -- the loop without a colouring ---------------------------------------------------------------------------------------
    def _is_lexicographic(self, k: LoopStmt, colour) -> bool:
        """An in-place smoother update with no colour on a kernel layer that has the lexicographic sweep (a layer without it keeps
        the launcher's refusal)."""
        return k.kind == "smooth" and colour is None and k.D is k.U and k.ds == k.us and hasattr(self.ops, "gs_sweep")

    def _check_lexicographic(self, k: LoopStmt, only, where, fr: _Frame):
        """What the lexicographic sweep cannot be, by name.  Its result depends on the order of the points of ONE fragment: the reference
        sweeps every fragment on its own, so merged fragments, several blocks or a periodic axis would compute another iteration."""
        what = "lexicographic Gauss-Seidel (in-place smoother update without colouring)"
        if only is not None or where is not None:
            raise Exa4Unsupported("%s in a loop with `only` or `where`" % what)
        if fr.contract is not None:
            raise Exa4Unsupported("%s under contraction" % what)
        if self._fragments != 1:
            raise Exa4Unsupported("%s: the knowledge file describes %d fragments, and every fragment sweeps on its own -- one merged "
                                  "block would compute another iteration" % (what, self._fragments))
        if self.domain.world_size != 1:
            raise Exa4Unsupported("%s on %d blocks (world_size must be 1)" % (what, self.domain.world_size))
        if any(self.domain.periodic):
            raise Exa4Unsupported("%s on a periodic domain" % what)
        for X in (k.D, k.F):
            if X.layout.is_cell:
                raise Exa4Unsupported("%s over cell field %s" % (what, X.name))
            if X.layout.transform:
                raise Exa4Unsupported("%s over colour-split field %s" % (what, X.name))
        if k.A.cfield is not None and k.A.ctransform:
            raise Exa4Unsupported("%s with an entry-fastest coefficient field" % what)

    # -- the launcher ---------------------------------------------------------------------------------------------------
    def _launch(self, k: LoopStmt, b, e, colour):
        """Issue the loop `k` stands for on the box [b, e): the only kernel-layer calls of loop-body assignments, and their count."""
        ops, kind = self.ops, k.kind
        D, U, F = k.D, k.U, k.F
        if kind.startswith("c_"):             # (exa4_complex.py) a loop over complex fields
            return self._launch_complex(k, b, e, colour)
        if kind.startswith("v_"):             # (exa4_vector.py) a loop over vector-valued cell fields: one launch over all components
            return self._launch_vector(k, b, e, colour)
        if kind == "bc_face":                 # (exa4_conservation.py) one face of a boundary function; no face: the block has a neighbour there
            return self._launch_bc_faces([k])
        if kind == "reduce_expr":             # the device scalar goes back to the reduction loop, which reads it
            self.launches += 1
            return ops.reduce_expr_cell(int(k.s), D.lc, [X.data(s) for X, s in k.prog[0]], k.prog[1], b, e)
        if kind == "bsys_row":              # (exa4_blocksys.py) the rows of a block system that stand together in a loop body
            self.launches += 1
            return self._launch_block_rows(k, b, e)
        if kind == "flux_step":
            ins, outs, spec = k.prog
            self.launches += 1
            return ops.flux_step(ins[0][0].lc, [X.data(s) for X, s in ins], D.lc, [X.data(s) for X, s in outs], spec, b, e)
        d = D.data(k.ds)
        u = None if U is None else U.data(k.us)
        lf, f = (None, None) if F is None else (F.lc, F.data(k.fs))
        if kind == "smooth":
            in_place = D is U and k.ds == k.us
            if in_place and colour is None:
                if not hasattr(ops, "gs_sweep"):
                    raise Exa4Unsupported("in-place smoother update without colouring (lexicographic Gauss-Seidel)")
                self.launches += 1
                ops.gs_sweep(U.lc, u, lf, f, k.A, k.s, b, e)       # the sequential nest's values (examg_gs_sweep); checked by _check_lexicographic
                return
            if not in_place and colour is not None:
                raise Exa4Unsupported("coloured update into another slot")
        if kind == "axis_smooth":
            in_place = D is U and k.ds == k.us
            if in_place != (colour is not None):
                raise Exa4Unsupported("a smoother over the grid's virtual fields runs out of place, or in place under the red-black colouring")
        self.launches += 1
        if kind == "set":
            ops.set(D.lc, d, k.s, b, e)
        elif kind in ("axis_residual", "axis_apply", "axis_smooth"):
            mode = {"axis_residual": RESIDUAL, "axis_apply": APPLY, "axis_smooth": SMOOTH}[kind]
            ops.axis_op(mode, U.lc, u, lf, f, D.lc, d, k.A, k.s, colour if kind == "axis_smooth" and colour is not None else -1, b, e)
        elif kind == "fill_expr_cell":
            ops.fill_expr_cell(D.lc, d, self.domain.geom(D.level), k.prog, b, e)
        elif kind == "fill_fn":
            ops.fill_fn(D.lc, d, self.domain.geom(D.level), k.prog[0], k.prog[1], b, e)
        elif kind == "fill_expr":
            if self.grid is not None:
                ops.fill_expr_grid(D.lc, d, self.grid.device(ops, D.level), k.prog, b, e)
            else:
                ops.fill_expr(D.lc, d, self.domain.geom(D.level), k.prog, b, e)
        elif kind in ("copy", "axpby"):
            ops.axpby(U.lc, u, D.lc, d, k.s, k.t, b, e)
        elif kind == "add_scalar":
            ops.add_scalar(D.lc, d, k.s, b, e)
        elif kind in ("residual", "apply", "smooth"):
            mode = {"residual": RESIDUAL, "apply": APPLY, "smooth": SMOOTH}[kind]
            ops.stencil_op(mode, U.lc, u, lf, f, D.lc, d, k.A, k.s, colour if kind == "smooth" and colour is not None else -1, b, e)
        elif kind == "restrict":
            ops.restrict(U.lc, u, D.lc, d, k.s, b, e)
        elif kind == "restrict_cell":
            ops.restrict_cell(U.lc, u, D.lc, d, k.s, b, e)
        elif kind == "prolong_add":
            ops.prolong_add(U.lc, u, D.lc, d, b, e)
        elif kind == "prolong_add_cell":
            ops.prolong_add_cell(U.lc, u, D.lc, d, b, e)
        elif kind == "sys_row":
            mode, us, G0, g, c = k.prog       # (exa4_systems.py: _recognise_system_row) one row of the system: a one-row mask
            fv, dst = [None] * len(us), [None] * len(us)
            fv[c], dst[c] = f, d
            ops.sys_op(mode, us[0][0].lc, [X.data(s) for X, s in us], lf or us[0][0].lc, fv, G0.lc,
                       [[x and x[0].data(x[1]) for x in row] for row in g], D.lc, dst, k.A, 1 << c, b, e)
        elif kind == "pointwise_mul":
            ops.pointwise_mul(U.lc, u, lf, f, D.lc, d, k.s, b, e)
        elif kind == "pointwise_sub":         # a copy and examg_axpby: x + (-1.0 * y) is bitwise x - y
            if not (U is D and k.us == k.ds):
                ops.axpby(U.lc, u, D.lc, d, 1.0, 0.0, b, e)
                self.launches += 1
            ops.axpby(lf, f, D.lc, d, -1.0, 1.0, b, e)
        elif kind == "nl_op":
            mode, Q, qs, c = k.prog
            ops.nl_op(mode, U.lc, u, Q.lc, Q.data(qs), lf, f, D.lc, d, k.A, c, b, e)
        elif kind == "nl_smooth":
            ops.nl_smooth(U.lc, u, D.lc, d, lf, f, k.A, k.prog[0], k.prog[1], k.s, -1 if colour is None else colour, b, e)
        else:
            raise AssertionError(kind)

    def _launch_bc_faces(self, group):
        """The faces of a boundary function that stand together (exa4_conservation.py: _merge_bc_faces) as ONE launch, each with its kind
        and program (examg_apply_bc_cell_faces); a single face, or a kernel layer without the faces call: one examg_apply_bc_cell each."""
        live = [k for k in group if k.prog[1]]
        if not live:
            return None
        D, ds, ops = live[0].D, live[0].ds, self.ops
        geom = self.domain.geom(D.level)
        if len(live) == 1 or not hasattr(ops, "apply_bc_cell_faces"):
            for k in live:
                self.launches += 1
                ops.apply_bc_cell(D.lc, D.data(ds), geom, k.prog[0], k.prog[2], k.prog[1])
            return None
        faces, mask = [None] * 6, 0
        for k in live:
            faces[k.prog[1].bit_length() - 1] = (k.prog[0], k.prog[2])
            mask |= k.prog[1]
        self.launches += 1
        ops.apply_bc_cell_faces(D.lc, D.data(ds), geom, faces, mask)
        return None

    def _launch_coloured(self, k: LoopStmt, b, e, col) -> bool:
        """The loop of `k` on the points of the colour `col` of a multi-colouring: the stencil loops have a coloured kernel
        (examg_stencil_op_coloured); False for every other kind."""
        what = "under a multi-colouring (color with several expressions)"
        D, U, F = k.D, k.U, k.F
        if k.kind.startswith("c_"):
            raise Exa4Unsupported("complex field %s %s" % (D.name, what))
        for X in (D, F, U) if k.kind == "residual" else (D, U, F):      # in the order the statement names them
            if X is not None and X.layout.transform:
                raise Exa4Unsupported("colour-split field %s %s" % (X.name, what))
        if k.kind.startswith("axis_"):
            raise Exa4Unsupported("a stencil over the grid's virtual fields %s" % what)
        if k.kind not in ("smooth", "residual", "apply"):
            return False
        # a loop that reads the array it writes: only where no point of the colour is a neighbour of another one
        if D is U and k.ds == k.us and not col.decouples(k.A.offsets):
            raise Exa4Unsupported("in-place %s %s: the colouring does not decouple the stencil (two points of one colour are "
                                  "neighbours: the generated loop depends on its order)"
                                  % ({"smooth": "smoother", "residual": "residual loop", "apply": "stencil application"}[k.kind], what))
        self.launches += 1
        d, u = D.data(k.ds), U.data(k.us)
        if k.kind == "smooth":
            self.ops.stencil_op_coloured(SMOOTH, U.lc, u, F.lc, F.data(k.fs), D.lc, d, k.A, k.s, col, b, e)
        elif k.kind == "residual":
            self.ops.stencil_op_coloured(RESIDUAL, U.lc, u, F.lc, F.data(k.fs), D.lc, d, k.A, 0.0, col, b, e)
        else:
            self.ops.stencil_op_coloured(APPLY, U.lc, u, None, None, D.lc, d, k.A, 0.0, col, b, e)
        return True
