"""Vector-valued cell fields in the ExaSlang-4 interpreter (mixin of Exa4Program): `Layout X< Vec2, Cell >`, fields of it, stencils whose
entries are matrices, stencil arithmetic on them (`Stencil S from ( a * A + B )`) and the loops of Testing/Application/OpticalFlow2D.exa4.
One launch per loop over ALL components (include/examg.h: examg_vec_*), found by the one recogniser (kinds `v_*`, exa4_statements.py) and
issued by the one launcher.  What is not built is refused as Exa4Unsupported, by name, with the words "vector-valued", before anything is
launched.  Programs with vector fields run without the one-pass fusions, without the one-kernel coarse solver and without graph replay."""
from __future__ import annotations

from .exa4_common import _Frame
from .exa4_parser import Exa4Unsupported, _contains, _walk
from .exa4_statements import LoopStmt
from .field import Field, MatrixStencil
from .lib import BC_NEUMANN, SYS_APPLY, SYS_RESIDUAL

_W = "vector-valued"


def _refuse(what):
    return Exa4Unsupported("%s fields: %s" % (_W, what))


class VectorFields:
    # -- declarations ---------------------------------------------------------------------------------------------------------------
    def _declare_vector_field(self, fd, ld, nslots: int):
        """`Field flow< global, vec2CellWComm, Neumann >`: n planes of the scalar cell layout, the component slowest."""
        from .layout import FieldLayout

        nd, dom, n = self.nd, self.domain, ld.vec_len
        who = "%s field %s" % (_W, fd.name)
        if ld.vec_elem not in ("Real", "Double"):
            raise Exa4Unsupported("%s with %s elements (complex, integer and single-precision vector fields: Real or Double only)" % (who, ld.vec_elem))
        if ld.datatype == "RowVector":
            raise Exa4Unsupported("%s: a row vector is a matrix of 1 x %d, more than one column (column vectors only)" % (who, ld.vec_len))
        if ld.vec_cols != 1:
            raise Exa4Unsupported("%s: a matrix with %d columns (column vectors only)" % (who, ld.vec_cols))
        if ld.localization != "Cell":
            raise Exa4Unsupported("%s on a %s layout (cell fields only)" % (who, ld.localization))
        if n > 3:
            raise Exa4Unsupported("%s with %d components (2 or 3)" % (who, n))
        if nslots != 1:
            raise Exa4Unsupported("%s with %d slots" % (who, nslots))
        order = self._bc_kind(fd.bc)
        if fd.bc is not None and order != 1:
            raise Exa4Unsupported("%s: a boundary condition other than Neumann (order 1) or None" % who)
        if int(self.k.get("discr_defaultNeumannOrder", 1)) != 1:
            raise Exa4Unsupported("%s: Neumann boundary conditions of order 2" % who)
        if dom.world_size != 1 or any(dom.periodic[:nd]):
            raise Exa4Unsupported("%s on more than one block or a periodic axis" % who)
        if self.grid is not None:
            raise Exa4Unsupported("%s on a non-uniform grid" % who)
        if any((ld.dup[i] if i < len(ld.dup) else 0) != 0 for i in range(nd)) or ld.inner:
            raise Exa4Unsupported("%s: duplicate layers or innerPoints on a cell layout" % who)
        self._cell_names.add(fd.name)
        self._vector_names.add(fd.name)
        self.fuse = self.fuse_coarse_solver = self.auto_graph = False
        ghost = tuple(ld.ghost[i] if i < nd and i < len(ld.ghost) else 0 for i in range(3))
        for lvl in self.levels_of(fd.levels):
            if (fd.name, lvl) in self.fields or not (self.min_level <= lvl <= self.max_level):
                continue
            nc = dom.ncells(lvl)
            lay = FieldLayout(nd, tuple(nc[i] if i < nd else 1 for i in range(3)), ghost, (0, 0, 0), (0, 0, 0), (0, 0, 0), ld.dup_comm,
                              ld.ghost_comm, localization="cell").as_vector(n)
            f = Field(fd.name, lvl, lay, self.ops, 1, None, ())
            f.cell_bc = (BC_NEUMANN, None) if order == 1 else None
            self.fields[(fd.name, lvl)] = f

    def _component_field(self, F: Field, c: int) -> Field:
        """Component c of a vector field as a scalar cell field of its own name (`rhs[0]`): what the scalar loops take."""
        key = ("%s[%d]" % (F.name, c), F.level)
        f = self.fields.get(key)
        if f is None:
            f = Field.view_of(key[0], F.level, *F.component(c, 0))
            f.cell_bc = None
            self.fields[key] = f
            self._cell_names.add(key[0])
        return f

    # -- matrix stencils ------------------------------------------------------------------------------------------------------------
    def _is_matrix_stencil(self, name: str) -> bool:
        sd = self._stencil_decls.get(name)
        if sd is None:
            return False
        if sd.from_expr is not None:
            return any(n[0] == "sten" and self._is_matrix_stencil(n[1]) for n in _walk(sd.from_expr))
        return any(e[0] == "mat" for _, e in sd.entries)

    def _touches_vector(self, e) -> bool:
        """Does the statement or expression name a vector field, a matrix stencil, or a literal of either kind?"""
        for n in _walk(e):
            if not n or not isinstance(n[0], str):
                continue
            if n[0] in ("mat", "colvec", "comp") or (n[0] == "fld" and n[1] in self._vector_names) or (n[0] in ("sten", "sentry") and self._is_matrix_stencil(n[1])):
                return True
        return False

    def matrix_stencil(self, name: str, lvl: int) -> MatrixStencil:
        key = ("matrix stencil", name, lvl)
        if key not in self._fn_cache:
            offs, elems, n = self._matrix_entries(name, lvl)
            code = lambda o: sum(1 for x in o if x != 0)
            glay = None
            for o, m in zip(offs, elems):
                if max(abs(x) for x in o) > 1 or code(o) > 1:
                    raise Exa4Unsupported("stencil %s on %s fields: the entry %s is not the centre or an axis neighbour" % (name, _W, list(o)))
                for c in range(n):
                    for d in range(n):
                        el = m[c][d]
                        if el is None:
                            continue
                        if any(o) and el[1] is not None:
                            raise Exa4Unsupported("stencil %s on %s fields: a field element off the centre" % (name, _W))
                        if any(o) and c != d:
                            raise Exa4Unsupported("stencil %s on %s fields: an off-centre matrix that is not diagonal" % (name, _W))
                        if el[1] is not None:
                            if glay is not None and el[1][0].layout != glay:
                                raise Exa4Unsupported("stencil %s on %s fields: coefficient fields of different layouts" % (name, _W))
                            glay = el[1][0].layout
            if (0, 0, 0) not in offs:
                raise Exa4Unsupported("stencil %s on %s fields has no centre entry" % (name, _W))
            dev = [[[None if el is None else (el[0], None if el[1] is None else el[1][0].data(el[1][1])) for el in row] for row in m] for m in elems]
            self._fn_cache[key] = MatrixStencil(n, offs, dev, glay)
        return self._fn_cache[key]

    def _matrix_entries(self, name: str, lvl: int):
        """(offsets, elems, n) of a declared matrix stencil; an element is None, or (constant or None, (Field, slot) or None).  A
        constant 0 is an absent element (`{ { a, 0 }, { 0, a } }` is a diagonal matrix)."""
        sd = self._stencil_decl_at.get((name, lvl)) or self._stencil_decls[name]
        fr = _Frame(lvl, {})
        if sd.from_expr is not None:
            return self._stencil_arith(sd.from_expr, fr, name)
        offs, elems, n = [], [], None
        for off, e in sd.entries:
            if e[0] != "mat":
                raise Exa4Unsupported("stencil %s on %s fields: scalar and matrix entries in one stencil" % (name, _W))
            rows = e[1]
            if n is None:
                n = len(rows)
            if len(rows) != n or any(len(r) != n for r in rows) or n not in (2, 3):
                raise Exa4Unsupported("stencil %s on %s fields: entries must be 2 x 2 or 3 x 3 matrices of one size" % (name, _W))
            m = [[None] * n for _ in range(n)]
            for c in range(n):
                for d in range(n):
                    x = rows[c][d]
                    if x[0] == "fld":
                        F, s = self._field(("fld", x[1], x[2], x[3] if x[3] is not None else ("single", lvl, 0)), fr)
                        if F.layout.is_vector or not F.layout.is_cell:
                            raise Exa4Unsupported("stencil %s on %s fields: the element %s is not a scalar cell field" % (name, _W, F.name))
                        m[c][d] = (None, (F, s))
                    elif _contains(x, ("fld", "sten", "mat", "colvec")):
                        raise Exa4Unsupported("stencil %s on %s fields: an element that is neither a constant nor a field" % (name, _W))
                    else:
                        v = float(self._eval(x, fr))
                        m[c][d] = None if v == 0.0 else (v, None)
            offs.append(tuple(off) + (0,) * (3 - len(off)))
            elems.append(m)
        return offs, elems, n

    def _stencil_arith(self, e, fr: _Frame, name: str):
        """`( s * A + B )` on the host: the scalar folds into every element; entries of equal offset merge element-wise -- constants fold,
        constant + field stays a sum per cell; a new offset is appended."""
        if e[0] == "sten":
            if not self._is_matrix_stencil(e[1]):
                raise Exa4Unsupported("stencil %s: a scalar stencil (%s) in the arithmetic of a stencil on %s fields" % (name, e[1], _W))
            return self._matrix_entries(e[1], self._level_of(e[2], fr))
        if e[0] == "bin" and e[1] == "+":
            ao, ae, n = self._stencil_arith(e[2], fr, name)
            bo, be, nb = self._stencil_arith(e[3], fr, name)
            if n != nb:
                raise Exa4Unsupported("stencil %s on %s fields: matrices of different sizes" % (name, _W))
            ao, ae = list(ao), [[list(r) for r in m] for m in ae]
            for o, m in zip(bo, be):
                if o not in ao:
                    ao.append(o)
                    ae.append([list(r) for r in m])
                    continue
                t = ae[ao.index(o)]
                for c in range(n):
                    for d in range(n):
                        x, y = t[c][d], m[c][d]
                        if x is None or y is None:
                            t[c][d] = x if y is None else y
                        elif x[1] is not None and y[1] is not None:
                            raise Exa4Unsupported("stencil %s on %s fields: the sum of two fields in one element" % (name, _W))
                        else:
                            kv = x[0] if y[0] is None else (y[0] if x[0] is None else x[0] + y[0])
                            t[c][d] = (kv, x[1] if x[1] is not None else y[1])
            return ao, ae, n
        if e[0] == "bin" and e[1] == "*" and not _contains(e[2], ("fld", "sten", "mat", "colvec")):
            s = float(self._eval(e[2], fr))
            o, el, n = self._stencil_arith(e[3], fr, name)
            out = []
            for m in el:
                mm = [[None] * n for _ in range(n)]
                for c in range(n):
                    for d in range(n):
                        x = m[c][d]
                        if x is None:
                            continue
                        if x[1] is not None and s != 1.0:
                            raise Exa4Unsupported("stencil %s on %s fields: a scalar factor other than 1 on a field element" % (name, _W))
                        mm[c][d] = (None if x[0] is None else s * x[0], x[1])
                out.append(mm)
            return o, out, n
        raise Exa4Unsupported("stencil %s on %s fields: arithmetic other than ( [s *] A + [s *] B .. )" % (name, _W))

    # -- the recogniser -------------------------------------------------------------------------------------------------------------
    def _vfield(self, e, fr, what):
        if e[0] != "fld":
            raise _refuse("%s must be a field access" % what)
        F, s = self._field(e, fr)
        if not F.layout.is_vector:
            raise _refuse("%s is the scalar field %s: scalar and vector fields mixed in one statement" % (what, F.name))
        return F, s

    def _v_sten_times(self, e, fr):
        """(stencil name, level spec, field expr) of `S * U`, None otherwise."""
        if e[0] == "bin" and e[1] == "*" and e[2][0] == "sten" and e[3][0] == "fld":
            return e[2][1], e[2][2], e[3]
        return None

    def _v_residual(self, e, fr):
        """(F expr, stencil name, level spec, U expr) of `F - S * U`."""
        if e[0] == "bin" and e[1] == "-" and e[2][0] == "fld":
            m = self._v_sten_times(e[3], fr)
            if m is not None and m[0] not in self.transfer:
                return (e[2],) + m
        return None

    def _v_operator(self, name, lspec, D, U, fr):
        if not self._is_matrix_stencil(name):
            raise _refuse("the scalar coefficient stencil %s on vector field %s" % (name, U.name))
        M = self.matrix_stencil(name, self._level_of(lspec, fr))
        if M.n != U.layout.ncomp or D.layout.ncomp != M.n:
            raise _refuse("stencil %s of %d x %d matrices on fields of %d and %d components" % (name, M.n, M.n, U.layout.ncomp, D.layout.ncomp))
        return M

    def _recognise_vector(self, st, fr: _Frame, colour=None) -> LoopStmt:
        """The record of an assignment that names a vector field or a matrix stencil: kinds v_set, v_axpby, v_op, v_smooth, v_restrict_cell,
        v_prolong_add_cell, v_components; or the refusal, by name."""
        op, lhs, rhs = st[1], st[2], st[3]
        for n in _walk(("block", [lhs, rhs])):
            if n and n[0] in ("index", "comp"):
                raise _refuse("component access")
        if lhs[0] != "fld" or lhs[1] not in self._vector_names:
            if _contains(rhs, ("mat",)) or any(n[0] == "sten" and self._is_matrix_stencil(n[1]) for n in _walk(rhs) if n and isinstance(n[0], str)):
                raise _refuse("a matrix stencil or matrix literal on the scalar field %s" % (lhs[1] if lhs[0] == "fld" else lhs[0]))
            raise _refuse("the scalar field %s assigned from vector fields" % (lhs[1] if lhs[0] == "fld" else lhs[0]))
        D, ds = self._vfield(lhs, fr, "the destination")
        n = D.layout.ncomp
        if op == "=":
            if rhs[0] == "colvec":
                if len(rhs[1]) != n:
                    raise _refuse("%d expressions assigned to the %d components of %s" % (len(rhs[1]), n, D.name))
                if colour is not None:
                    raise _refuse("a component-wise assignment in a coloured loop")
                parts = []
                for c, ec in enumerate(rhs[1]):
                    if self._touches_vector(ec):
                        raise _refuse("a vector field inside the component expression %d of %s" % (c, D.name))
                    Fc = self._component_field(D, c)
                    parts.append(self._recognise_plain(("assign", "=", ("fld", Fc.name, None, lhs[3]), ec), fr, None))
                return LoopStmt("v_components", D, ds, prog=parts)
            if not _contains(rhs, ("fld", "sten", "sentry", "mat", "colvec")):
                if self._over_position(rhs):
                    raise _refuse("a position expression assigned to %s" % D.name)
                return LoopStmt("v_set", D, ds, s=float(self._eval(rhs, fr)))
            if rhs[0] == "fld":
                return LoopStmt("v_axpby", D, ds, *self._vfield(rhs, fr, "the source"), s=1.0, t=0.0)
            r = self._v_residual(rhs, fr)
            if r is not None:
                U, us = self._vfield(r[3], fr, "the unknown")
                F, fs = self._vfield(r[0], fr, "the right-hand side")
                if colour is not None:
                    raise _refuse("a residual loop under a colouring")
                return LoopStmt("v_op", D, ds, U, us, F, fs, A=self._v_operator(r[1], r[2], D, U, fr), prog=SYS_RESIDUAL)
            m = self._v_sten_times(rhs, fr)
            if m is not None:
                U, us = self._vfield(m[2], fr, "the operand")
                if m[0] in self.transfer:
                    if self.transfer[m[0]] != "cell_restriction" or self.transfer_factor.get(m[0], 1.0) != 1.0:
                        raise _refuse("the transfer %s (the linear cell restriction and prolongation only)" % m[0])
                    if U.level != D.level + 1 or U.layout.ncomp != n:
                        raise _refuse("restriction between levels %d and %d or other component counts" % (U.level, D.level))
                    return LoopStmt("v_restrict_cell", D, ds, U, us, s=1.0)
                if colour is not None:
                    raise _refuse("an operator loop under a colouring")
                return LoopStmt("v_op", D, ds, U, us, A=self._v_operator(m[0], m[1], D, U, fr), prog=SYS_APPLY)
            if rhs[0] == "bin" and rhs[1] == "+" and rhs[2][0] == "fld":
                t = rhs[3]
                k = self._v_smoother(D, ds, lhs, rhs[2], t, colour, fr)
                if k is not None:
                    return k
                # Y + ( b * D )
                if (t[0] == "bin" and t[1] == "*" and t[3][0] == "fld" and self._same_access(lhs, t[3], fr)
                        and not _contains(t[2], ("fld", "sten", "mat", "colvec")) and not self._over_position(t[2])):
                    return LoopStmt("v_axpby", D, ds, *self._vfield(rhs[2], fr, "the source"), s=1.0, t=float(self._eval(t[2], fr)))
        elif op in ("+=", "-="):
            sign = 1.0 if op == "+=" else -1.0
            if rhs[0] == "fld":
                return LoopStmt("v_axpby", D, ds, *self._vfield(rhs, fr, "the source"), s=sign, t=1.0)
            if rhs[0] == "bin" and rhs[1] == "*":
                m = self._v_sten_times(rhs, fr)
                if m is not None and m[0] in self.transfer:
                    U, us = self._vfield(m[2], fr, "the coarse field")
                    if op != "+=" or self.transfer[m[0]] != "cell_prolongation" or U.level != D.level - 1 or U.layout.ncomp != n:
                        raise _refuse("the transfer %s in this statement (`X += P@coarser * X@coarser` with the linear cell prolongation)" % m[0])
                    return LoopStmt("v_prolong_add_cell", D, ds, U, us)
                if rhs[3][0] == "fld" and not _contains(rhs[2], ("fld", "sten", "mat", "colvec")) and not self._over_position(rhs[2]):
                    return LoopStmt("v_axpby", D, ds, *self._vfield(rhs[3], fr, "the source"), s=sign * float(self._eval(rhs[2], fr)), t=1.0)
        raise _refuse("the loop body statement `%s %s ..` is none of the recognised vector loops" % (lhs[1], op))

    def _v_smoother(self, D, ds, lhs, src, t, colour, fr):
        """`U = U + [w *] inverse ( diag ( S ) ) * ( F - S * U )`; None when `t` is not of this form."""
        if t[0] != "bin" or t[1] != "*":
            return None
        inv, w = t[2], None
        if inv[0] == "bin" and inv[1] == "*" and inv[3][0] == "call":
            w, inv = inv[2], inv[3]
        if not (inv[0] == "call" and inv[1] == "inverse" and len(inv[3]) == 1 and inv[3][0][0] == "call" and inv[3][0][1] == "diag"
                and len(inv[3][0][3]) == 1 and inv[3][0][3][0][0] == "sten"):
            return None
        r = self._v_residual(t[3], fr)
        if r is None:
            raise _refuse("inverse ( diag ( S ) ) times something other than ( F - S * U )")
        if inv[3][0][3][0][1] != r[1]:
            raise _refuse("the smoother inverts the diagonal of %s and applies %s" % (inv[3][0][3][0][1], r[1]))
        if not (self._same_access(lhs, src, fr) and self._same_access(lhs, r[3], fr)):
            raise _refuse("the smoother out of place (`U = U + inverse ( diag ( S ) ) * ( F - S * U )` updates U)")
        if fr.mcolour is not None:
            raise _refuse("the smoother under a multi-colouring")
        if colour is None:
            raise _refuse("the smoother outside a colouring (`repeat with { colour conditions .. }` or `color with`)")
        F, fs = self._vfield(r[0], fr, "the right-hand side")
        if w is not None and (_contains(w, ("fld", "sten", "mat", "colvec")) or self._over_position(w)):
            raise _refuse("a smoother weight that is not a scalar")
        return LoopStmt("v_smooth", D, ds, D, ds, F, fs, A=self._v_operator(r[1], r[2], D, D, fr), s=1.0 if w is None else float(self._eval(w, fr)))

    # -- the launcher ---------------------------------------------------------------------------------------------------------------
    def _launch_vector(self, k: LoopStmt, b, e, colour):
        ops, D, U, F = self.ops, k.D, k.U, k.F
        n = D.layout.ncomp
        if k.kind == "v_components":
            for part in k.prog:
                self._launch(part, b, e, None)
            return
        self.launches += 1
        d = D.data(k.ds)
        if k.kind == "v_set":
            ops.vec_set(n, D.lc, d, k.s, b, e)
        elif k.kind == "v_axpby":
            ops.vec_axpby(n, U.lc, U.data(k.us), D.lc, d, k.s, k.t, b, e)
        elif k.kind == "v_op":
            ops.vec_op(k.prog, n, U.lc, U.data(k.us), F.lc if F is not None else None, F.data(k.fs) if F is not None else None, D.lc, d, k.A, b, e)
        elif k.kind == "v_smooth":
            ops.vec_smooth(n, D.lc, d, F.lc, F.data(k.fs), k.A, k.s, colour, b, e)
        elif k.kind == "v_restrict_cell":
            ops.vec_restrict_cell(n, U.lc, U.data(k.us), D.lc, d, k.s, b, e)
        elif k.kind == "v_prolong_add_cell":
            ops.vec_prolong_add_cell(n, U.lc, U.data(k.us), D.lc, d, b, e)
        else:
            raise AssertionError(k.kind)

    # -- whole statements -----------------------------------------------------------------------------------------------------------
    def _apply_bc_vector(self, f: Field, slot: int):
        mask = self.domain.face_mask()
        if f.cell_bc is not None and mask:
            self.launches += 1
            self.ops.vec_apply_bc_cell(f.layout.ncomp, f.lc, f.data(slot), self.domain.geom(f.level), BC_NEUMANN, mask)

    def _exec_vector_loop(self, s, f: Field, fr: _Frame):
        """A loop whose target or body names a vector field: every statement one launch (a `{ .. }T` assignment one per component)."""
        _, target, only, where, reduction, body = s
        if only is not None or where is not None or fr.contract is not None:
            raise _refuse("a loop with `only`, `where` or under contraction")
        if fr.mcolour is not None and not any(st[0] == "assign" and self._is_v_smoother_text(st) for st in body):
            raise _refuse("a loop under a multi-colouring")
        for st in body:
            if st[0] == "solve":
                raise _refuse("`solve locally` over vector fields")
            if st[0] != "assign":
                raise _refuse("the statement %r inside a loop body" % st[0])
        boxes, colour = self._loop_boxes(f, None, None, reduction, fr)
        if reduction is not None:
            return self._exec_vector_reduction(boxes, reduction, body, fr)
        ks = [self._recognise_assign(st, fr, colour) for st in body]      # every refusal before the first launch
        for k in ks:
            for b, e in boxes:
                self._launch(k, b, e, colour)

    @staticmethod
    def _is_v_smoother_text(st) -> bool:
        return any(n and n[0] == "call" and n[1] == "inverse" for n in _walk(st[3]))

    def _exec_vector_reduction(self, boxes, reduction, body, fr: _Frame):
        op, var = reduction
        plan = []
        for st in body:
            rhs = st[3] if st[0] == "assign" else None
            if (op != "+" or rhs is None or st[1] != "+=" or st[2] != ("id", var, None) or rhs[0] != "call" or rhs[1] != "dot"
                    or len(rhs[3]) != 2):
                raise _refuse("a reduction other than `v += dot ( X, Y )` with `reduction ( + : v )`")
            X, xs = self._vfield(rhs[3][0], fr, "the first argument of dot")
            Y, ys = self._vfield(rhs[3][1], fr, "the second argument of dot")
            if X.layout.ncomp != Y.layout.ncomp:
                raise _refuse("dot of %d and %d components" % (X.layout.ncomp, Y.layout.ncomp))
            plan.append((X, xs, Y, ys))
        tgt = fr.vars if var in fr.vars or var not in self.globals else self.globals
        for X, xs, Y, ys in plan:
            acc = 0.0
            for b, e in boxes:
                self.launches += 1
                acc += self.comm.reduce_value(self.ops.vec_dot(X.layout.ncomp, X.lc, X.data(xs), Y.lc, Y.data(ys), b, e), "sum")
            tgt[var] = tgt[var] + acc
