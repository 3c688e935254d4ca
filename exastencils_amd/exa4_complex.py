"""Complex-valued node fields in the ExaSlang-4 interpreter (mixin of exa4.Exa4Program): `Layout X< Complex<Real>, Node >`.

A loop-body assignment over complex fields is recognised where every assignment is (exa4_statements.py: `_recognise_plain` hands it to
`_recognise_complex`) and becomes a LoopStmt of a kind `c_*`, which the one launcher issues through `_launch_complex`: one call of the complex
kernel layer per loop (include/examg.h: examg_cstencil_op .. examg_cfrom_parts; `set` and copies run the real entry points on the real view
of the field).  The whole-loop forms keep their places: the reduction `v += X * Y` (examg_cdot), `solve locally relax w { U => (M * U) == F }`
with one unknown under the red-black colouring (EXAMG_CRELAX) and the loops of a boundary function over one duplicate plane
(examg_cshift_div, `set`).  Host scalars are Python complex numbers, evaluated in the program's own association."""
from __future__ import annotations

import dataclasses

from .exa4_common import APPLY, RESIDUAL, SMOOTH, _Frame
from .exa4_parser import Exa4Unsupported, _contains, _walk
from .field import Field
from .layout import FieldLayout
from .lib import C_XMAY, C_XPAY, C_XPAYMBZ, CRELAX

_MODES = {"c_apply": APPLY, "c_residual": RESIDUAL, "c_smooth": SMOOTH}


class ComplexFields:
    # -- declaration -----------------------------------------------------------------------------------------------------------------
    def _declare_complex_field(self, fd, ld, nslots: int, sfield_fields):
        """A field of a `Complex<Real>` layout: a node field on one block, two doubles per point."""
        nd, dom = self.nd, self.domain
        if ld.localization != "Node":
            raise Exa4Unsupported("field %s: complex cell fields (complex fields are node fields)" % fd.name)
        if ld.vec_len != 1 or fd.name in sfield_fields:
            raise Exa4Unsupported("field %s: complex stencil fields" % fd.name)
        if dom.world_size != 1 or any(dom.periodic[:nd]):
            raise Exa4Unsupported("field %s: a complex field on more than one block or on a periodic axis" % fd.name)
        if self.grid is not None:
            raise Exa4Unsupported("field %s: complex fields on a non-uniform grid (the axis path)" % fd.name)
        if nslots != 1:
            raise Exa4Unsupported("field %s: slotted complex fields" % fd.name)
        if ld.inner:
            raise Exa4Unsupported("layout %s: innerPoints on a complex layout" % ld.name)
        bc_function = None
        if fd.bc is not None:
            if not (fd.bc[0] == "call" and fd.bc[1] in self.functions and not fd.bc[3]):
                raise Exa4Unsupported("field %s: the boundary condition of a complex field must be a boundary function without arguments" % fd.name)
            bc_function = fd.bc[1]
        self._complex_names.add(fd.name)
        # launches of complex loops are issued one by one: the one-pass forms, the one-kernel coarse solver and the cross-statement fusions
        # know real fields only
        self.fuse = self.fuse_coarse_solver = False
        ghost = tuple(ld.ghost[i] if i < nd and i < len(ld.ghost) else 0 for i in range(3))
        dup = tuple((ld.dup[i] if i < len(ld.dup) else 1) if i < nd else 0 for i in range(3))
        if any(dup[i] != 1 for i in range(nd)):
            raise Exa4Unsupported("layout %s: node fields need one duplicate layer" % ld.name)
        for lvl in self.levels_of(fd.levels):
            if (fd.name, lvl) in self.fields or not (self.min_level <= lvl <= self.max_level):
                continue
            nc = dom.ncells(lvl)
            inner = tuple(nc[i] - 1 if i < nd else 1 for i in range(3))
            lay = FieldLayout(nd, inner, ghost, dup, (0, 0, 0), (0, 0, 0), ld.dup_comm, ld.ghost_comm, element="complex")
            f = Field(fd.name, lvl, lay, self.ops, 1, None, ())
            f.rlc = lay.real_view().c_struct()
            f.bc_function = bc_function
            self.fields[(fd.name, lvl)] = f

    def _reads_complex(self, e) -> bool:
        return bool(self._complex_names) and any(n and n[0] == "fld" and n[1] in self._complex_names for n in _walk(e))

    def _complex_scalar(self, e, fr: _Frame, what: str) -> complex:
        if not self._is_scalar(e):
            raise Exa4Unsupported("%s of a loop over complex fields must be a scalar" % what)
        return complex(self._eval(e, fr))

    # -- the recogniser's complex half ---------------------------------------------------------------------------------------------------
    def _recognise_complex(self, op, lhs, rhs, D: Field, ds: int, fr: _Frame):
        """LoopStmt `c_*` of an assignment that names a complex field, or the refusal that says why it is none of the complex kernels."""
        from .exa4_statements import LoopStmt

        if not D.layout.is_complex:
            raise Exa4Unsupported("real field %s assigned from complex fields: real and complex fields mixed in one loop body" % D.name)
        for n in _walk(rhs):
            if n and n[0] == "fld" and n[1] not in self._complex_names:
                raise Exa4Unsupported("real field %s in a loop body over complex field %s: real and complex fields mixed in one loop body "
                                      "(only `%s = <real point expression>` fills a complex field from real values)" % (n[1], D.name, D.name))
            if n and n[0] == "call" and n[1] in ("conj", "conjugate"):
                raise Exa4Unsupported("a conjugated product (conj) in a loop over complex fields: the kernels multiply unconjugated")
            if n and n[0] == "sentry":
                raise Exa4Unsupported("complex stencil fields (an entry access in a loop over complex field %s)" % D.name)
        if fr.contract is not None:
            raise Exa4Unsupported("complex field %s under contraction" % D.name)
        none = Exa4Unsupported("loop body statement over complex fields is none of the recognised kernels: %s %s ..." % (lhs[1], op))
        if op == "=":
            if not _contains(rhs, ("fld", "sten", "sentry")):
                if not self._over_position(rhs):
                    v = complex(self._eval(rhs, fr))
                    if v.imag != 0.0:
                        raise Exa4Unsupported("complex field %s set to a constant with an imaginary part" % D.name)
                    return LoopStmt("c_set", D, ds, s=v.real)
                # a REAL point expression: fill a real scratch field, then lift it.  Always the expression's own program: a point source is
                # zero wherever the recogniser of the built-in point functions samples it
                from .lib import ExprC

                try:
                    return LoopStmt("c_fill", D, ds, prog=ExprC.from_program(self._compile_point_expr(rhs, D.level)))
                except ValueError as ex:
                    raise Exa4Unsupported(str(ex))
            if rhs[0] == "fld":
                return LoopStmt("c_copy", D, ds, *self._field(rhs, fr))
            r = self._residual_form(rhs, fr)
            if r is not None:
                return self._complex_stencil("c_residual", D, ds, r[2], r[0], r[1], 0.0, fr)
            m = self._sten_times_field(rhs, fr)
            if m is not None:
                if m[1] == "restriction":
                    return dataclasses.replace(self._transfer_stmt(m, +1, D, ds, *self._field(m[4], fr)), kind="c_restrict")
                if m[1] == "stencil" and m[0] == 1.0:
                    return self._complex_stencil("c_apply", D, ds, m[4], None, m[2], 0.0, fr)
                raise none
            if rhs[0] == "bin" and rhs[1] in ("+", "-") and rhs[2][0] == "fld":
                t = rhs[3]
                if t[0] == "bin" and t[1] == "*":
                    r = self._residual_form(t[3], fr)
                    if r is not None and rhs[1] == "+" and self._same_access(rhs[2], r[2], fr):      # U + w * (F - A * U)
                        return self._complex_stencil("c_smooth", D, ds, r[2], r[0], r[1], self._complex_scalar(t[2], fr, "the smoother weight"), fr)
                    X, xs = self._field(rhs[2], fr)
                    if t[3][0] == "fld":                                                              # X +- a * Y
                        a = self._complex_scalar(t[2], fr, "the factor a of X + a * Y")
                        return LoopStmt("c_lincomb", D, ds, X, xs, prog=(C_XPAY if rhs[1] == "+" else C_XMAY, a, None, self._field(t[3], fr), None))
                    y = t[3]
                    if (rhs[1] == "+" and y[0] == "bin" and y[1] == "-" and y[2][0] == "fld" and y[3][0] == "bin" and y[3][1] == "*"
                            and y[3][3][0] == "fld"):                                               # X + a * (Y - b * Z)
                        a = self._complex_scalar(t[2], fr, "the factor a of X + a * (Y - b * Z)")
                        b = self._complex_scalar(y[3][2], fr, "the factor b of X + a * (Y - b * Z)")
                        return LoopStmt("c_lincomb", D, ds, X, xs, prog=(C_XPAYMBZ, a, b, self._field(y[2], fr), self._field(y[3][3], fr)))
        elif op == "+=":
            m = self._sten_times_field(rhs, fr) if rhs[0] == "bin" and rhs[1] == "*" else None
            if m is not None and m[1] == "prolongation" and m[0] == 1.0:
                return dataclasses.replace(self._transfer_stmt(m, -1, D, ds, *self._field(m[4], fr)), kind="c_prolong_add")
        raise none

    def _complex_stencil(self, kind, D, ds, u, f, A, w, fr):
        from .exa4_statements import LoopStmt

        if A.cfield is not None or getattr(A, "is_axis", False):
            raise Exa4Unsupported("complex stencil fields (a stencil field or a stencil over the grid's virtual fields on complex field %s)" % D.name)
        U, us = self._field(u, fr)
        F, fs = self._field(f, fr) if f is not None else (None, 0)
        return LoopStmt(kind, D, ds, U, us, F, fs, A, w)

    # -- the launcher's complex half --------------------------------------------------------------------------------------------------------
    def _launch_complex(self, k, b, e, colour):
        ops, kind, D = self.ops, k.kind, k.D
        d = D.data(k.ds)
        U, F = k.U, k.F
        u = None if U is None else U.data(k.us)
        if colour is not None and kind != "c_smooth":
            raise Exa4Unsupported("a coloured loop over complex field %s other than the smoother update" % D.name)
        if kind == "c_smooth" and (D is U and k.ds == k.us) != (colour is not None):
            raise Exa4Unsupported("a smoother update of complex field %s runs out of place, or in place under the red-black colouring "
                                  "(no lexicographic sweep of complex fields)" % D.name)
        self.launches += 1
        if kind in ("c_set", "c_copy"):
            rb, re = FieldLayout.real_view_box(b, e)
            if kind == "c_set":
                ops.set(D.rlc, d, k.s, rb, re)
            else:
                ops.axpby(U.rlc, u, D.rlc, d, 1.0, 0.0, rb, re)
        elif kind == "c_fill":
            S = self._complex_scratch.get(D.level)
            if S is None:
                S = self._complex_scratch[D.level] = Field("complex_fill_scratch", D.level, dataclasses.replace(D.layout, element="real"), ops)
            ops.fill_expr(S.lc, S.data(), self.domain.geom(D.level), k.prog, b, e)
            self.launches += 1
            ops.cfrom_parts(D.lc, d, S.lc, S.data(), None, None, b, e)
        elif kind in _MODES:
            lf, f = (None, None) if F is None else (F.lc, F.data(k.fs))
            ops.cstencil_op(_MODES[kind], U.lc, u, lf, f, D.lc, d, k.A, k.s, colour if colour is not None else -1, b, e)
        elif kind == "c_restrict":
            ops.crestrict(U.lc, u, D.lc, d, k.s, b, e)
        elif kind == "c_prolong_add":
            ops.cprolong_add(U.lc, u, D.lc, d, b, e)
        elif kind == "c_lincomb":
            form, a, bb, (Y, ys), z = k.prog
            Z, zs = z if z is not None else (None, 0)
            ops.clincomb(form, U.lc, u, Y.lc, Y.data(ys), Z.lc if Z is not None else None, Z.data(zs) if Z is not None else None, D.lc, d, a, bb, b, e)
        else:
            raise AssertionError(kind)

    # -- whole-loop forms ---------------------------------------------------------------------------------------------------------------------
    def _complex_dot(self, X, xs, Y, ys, boxes) -> complex:
        """`v += X * Y` of a reduction loop over complex fields: the unconjugated sum, one examg_cdot per box."""
        if not (X.layout.is_complex and Y.layout.is_complex):
            raise Exa4Unsupported("reduction over the product of real field and complex field (%s, %s): real and complex fields mixed" % (X.name, Y.name))
        acc = 0j
        for b, e in boxes:
            self.launches += 1
            acc += self.ops.complex_value(self.ops.cdot(X.lc, X.data(xs), Y.lc, Y.data(ys), b, e))
        return acc

    def _exec_complex_solve(self, st, boxes, colour, fr: _Frame):
        """`solve locally relax w { U => (M * U) == F }` with one complex node unknown under the red-black colouring: one EXAMG_CRELAX."""
        _, jacobi, relax, rows = st
        (u, lhs, rhs), = rows
        U, us = self._field(u, fr)
        if jacobi:
            raise Exa4Unsupported("solve locally with jacobi")
        if colour is None:
            raise Exa4Unsupported("solve locally in an uncoloured loop")
        m = self._sten_times_field(lhs, fr)
        if m is None or m[1] != "stencil" or m[0] != 1.0 or not self._same_access(m[4], u, fr):
            raise Exa4Unsupported("solve locally: the row of complex unknown %s must read (M * %s) with a constant stencil M" % (U.name, U.name))
        if rhs[0] != "fld":
            raise Exa4Unsupported("solve locally: the right-hand side of a row must be a field")
        F, fs = self._field(rhs, fr)
        if not F.layout.is_complex:
            raise Exa4Unsupported("solve locally: complex unknown %s with the real right-hand side %s: real and complex fields mixed" % (U.name, F.name))
        k = self._complex_stencil("c_relax", U, us, u, rhs, m[2], 0.0, fr)
        w = complex(1.0 if relax is None else self._eval(relax, fr))
        if w.imag != 0.0:
            raise Exa4Unsupported("solve locally relax with a complex weight")
        for b, e in boxes:
            self.launches += 1
            self.ops.cstencil_op(CRELAX, U.lc, U.data(us), F.lc, F.data(fs), None, None, k.A, w.real, colour, b, e)

    def _exec_complex_only_loop(self, s, f: Field, fr: _Frame):
        """A loop of a boundary function of a complex node field over one duplicate plane without neighbour:
        `loop over u only dup [d] on boundary { u@[0, 0] = u@[o] / c }` is one examg_cshift_div, `{ u@[0, 0] = 0.0 }` one `set`."""
        _, target, only, where, reduction, body = s
        what = "loop over complex field %s only %s %s" % (f.name, only[0], list(only[1]))
        if self._bc_depth == 0:
            raise Exa4Unsupported("%s: `only` regions of complex fields outside boundary functions" % what)
        if only[0] != "dup" or not only[2] or where is not None or reduction is not None or fr.colour is not None:
            raise Exa4Unsupported("%s: the loops of a boundary function run over one duplicate plane, `on boundary`, without condition" % what)
        bad = Exa4Unsupported("%s: the body must be `%s = %s@[o] / c` or `%s = <real constant>`" % ((what,) + (f.name,) * 3))
        if len(body) != 1 or body[0][0] != "assign" or body[0][1] != "=" or body[0][2][0] != "fld" or self._field(body[0][2], fr)[0] is not f:
            raise bad
        D, ds = self._field(body[0][2], fr)
        rhs = body[0][3]
        boxes, _ = self._loop_boxes(f, only, where, reduction, fr)
        if not _contains(rhs, ("fld", "sten", "sentry", "off")) and not self._over_position(rhs):
            v = complex(self._eval(rhs, fr))
            if v.imag != 0.0:
                raise bad
            for b, e in boxes:
                self.launches += 1
                self.ops.set(D.rlc, D.data(ds), v.real, *FieldLayout.real_view_box(b, e))
            return
        if not (rhs[0] == "bin" and rhs[1] == "/" and rhs[2][0] == "off" and rhs[2][1][0] == "fld" and self._field(rhs[2][1], fr) == (D, ds)):
            raise bad
        c = self._complex_scalar(rhs[3], fr, "the divisor")
        for b, e in boxes:
            self.launches += 1
            self.ops.cshift_div(D.lc, D.data(ds), tuple(rhs[2][2]), c, b, e)
