"""Coupled systems of scalar cell fields in the ExaSlang-4 interpreter (mixin of Exa4Program): point-wise coefficient stencils
(`Stencil uvSten { [0, 0] => IxIy }`), system rows `sum_d (P_cd * F_d) + [s *] (L * F_c)`, `solve locally` inside a coloured loop
and the point-wise set-up statements of Benchmark/OptFlow2D/2D_FD_OptFlow.exa4.  One launch per loop: examg_sys_op with a one-row
mask, examg_sys_relax, examg_pointwise_mul (include/examg.h).  System rows and point-wise statements are RECOGNISED here, for the one
recogniser of loop-body assignments, and launched by its launcher (exa4_statements.py); `solve locally` is a whole-loop form and issues
its own call.  Cell fields are never deferred or fused (exa4_fusion.py), so these loops run where they stand."""
from __future__ import annotations

from .exa4_parser import Exa4Unsupported, _contains
from .exa4_statements import LoopStmt
from .field import Stencil
from .lib import SYS_APPLY, SYS_RESIDUAL


def _flatten(e, op):
    if e[0] == "bin" and e[1] == op:
        return _flatten(e[2], op) + _flatten(e[3], op)
    return [e]


class Systems:
    # -- point-wise coefficient stencils --------------------------------------------------------------------------------------
    def _coef_field(self, name: str):
        """The field expression of a point-wise coefficient stencil (its single centre entry is a field access), None for any
        other stencil.  A field anywhere else in a stencil is refused by name."""
        if name not in self._field_stencils():
            return None
        sd = self._stencil_decls[name]
        if not any(e[0] == "fld" for _, e in sd.entries):
            return None       # expressions over fields only: exa4_nonlinear.py names what it refuses
        if len(sd.entries) != 1:
            raise Exa4Unsupported("stencil %s: a field as an entry of a stencil with more than one entry" % name)
        off, e = sd.entries[0]
        if any(o != 0 for o in off):
            raise Exa4Unsupported("stencil %s: a field as an entry off the centre" % name)
        if e[0] != "fld":
            return None       # an expression over a field: a coefficient-expression stencil (exa4_nonlinear.py)
        return e

    def _field_stencils(self):
        """The declared stencils with a field access in an entry -- these and the coefficient-expression stencils of exa4_nonlinear.py
        are among them, most programs have none.  Every loop statement is asked whether it names one: found once, declarations stay."""
        if "field stencils" not in self._fn_cache:
            self._fn_cache["field stencils"] = {n for n, sd in self._stencil_decls.items() if any(_contains(e, ("fld",)) for _, e in sd.entries)}
        return self._fn_cache["field stencils"]

    # -- system rows ----------------------------------------------------------------------------------------------------------
    def _system_row(self, e, fr):
        """`sum_d (P_cd * F_d) + [s *] (L * F_c)` in either association of the scalar factor: (coefficient terms [(G, gs, F_d expr)],
        L with the factor folded into its coefficients, F_c expr), or None when the expression is nothing of the kind."""
        terms, lap = [], None
        for add in _flatten(e, "+"):
            fac = _flatten(add, "*")
            if len(fac) < 2 or fac[-1][0] != "fld":
                return None
            stens = [x for x in fac[:-1] if x[0] == "sten"]
            if len(stens) != 1 or stens[0][1] in self.transfer:
                return None
            ce = self._coef_field(stens[0][1]) if stens[0][1] in self._stencil_decls else None
            if ce is not None:
                if len(fac) != 2:
                    return None
                lvl = self._level_of(stens[0][2], fr)
                G, gs = self._field(("fld", ce[1], ce[2], ce[3] if ce[3] is not None else ("single", lvl, 0)), fr)
                terms.append((G, gs, fac[-1]))
                continue
            scal = [x for x in fac[:-1] if x[0] != "sten"]
            if lap is not None or not all(self._is_scalar(x) for x in scal):
                return None
            A = self.stencil(stens[0][1], self._level_of(stens[0][2], fr))
            if A.cfield is not None or getattr(A, "is_axis", False):      # refused below, once the expression has shown itself to be a system row
                lap = (A, fac[-1], stens[0][1])
                continue
            s = None
            for x in scal:        # the factor as written, left to right; folded into the coefficients as stencil arithmetic does
                v = float(self._eval(x, fr))
                s = v if s is None else s * v
            if s is not None and s != 1.0:
                A = Stencil(list(A.offsets), [s * c for c in A.coefs])
            lap = (A, fac[-1])
        if not terms or lap is None:
            return None
        if len(lap) == 3:
            raise Exa4Unsupported("system row: a stencil field (%s) as the constant stencil of a system" % lap[2])
        return terms, lap[0], lap[1]

    def _system_fields(self, exprs, fr, what):
        out = []
        for x in exprs:
            F, s = self._field(x, fr)
            if not F.layout.is_cell:
                raise Exa4Unsupported("%s on node field %s: systems are built for cell fields" % (what, F.name))
            if not any(F is G and s == t for G, t in out):
                out.append((F, s))
        return out

    @staticmethod
    def _one_layout(fields, what):
        for F, _ in fields[1:]:
            if F.layout != fields[0][0].layout:
                raise Exa4Unsupported("%s: %s and %s have different layouts" % (what, fields[0][0].name, F.name))

    def _recognise_system_row(self, D, ds, rhs, colour, fr):
        """`X = row` (EXAMG_SYS_APPLY) and `X = rhs - ( row )` (EXAMG_SYS_RESIDUAL): the record of one examg_sys_op with a one-row mask,
        None when the expression is no system row."""
        mode, F, row = SYS_APPLY, None, rhs
        if rhs[0] == "bin" and rhs[1] == "-" and rhs[2][0] == "fld":
            mode, F, row = SYS_RESIDUAL, rhs[2], rhs[3]
        if not self._field_stencils() or not _contains(row, ("sten",)):      # (no row without a coefficient term)
            return None
        r = self._system_row(row, fr)
        if r is None:
            return None
        terms, L, own = r
        if colour is not None:
            raise Exa4Unsupported("system row in a coloured loop outside solve locally")
        us = self._system_fields([t[2] for t in terms] + [own], fr, "system row")
        if not 2 <= len(us) <= 3:
            raise Exa4Unsupported("system row over %d unknowns (2 or 3)" % len(us))
        self._one_layout(us, "system row")
        self._one_layout([(t[0], t[1]) for t in terms], "system row")
        if not D.layout.is_cell:
            raise Exa4Unsupported("system row assigned to node field %s" % D.name)
        n = len(us)
        U, uslot = self._field(own, fr)
        c = [k for k, (X, s) in enumerate(us) if X is U and s == uslot][0]
        g = [[None] * n for _ in range(n)]
        for G, gs, fx in terms:
            X, s = self._field(fx, fr)
            d = [k for k, (Y, t) in enumerate(us) if Y is X and t == s][0]
            if g[c][d] is not None:
                raise Exa4Unsupported("system row with two coefficient terms on %s" % X.name)
            g[c][d] = (G, gs)
        FF, fs = self._field(F, fr) if F is not None else (None, 0)
        return LoopStmt("sys_row", D, ds, F=FF, fs=fs, A=L, prog=(mode, us, terms[0][0], g, c))

    # -- solve locally --------------------------------------------------------------------------------------------------------
    def _exec_solve_locally(self, st, boxes, colour, fr, only=None, where=None):
        """`solve locally [relax w] { F_c => row_c == rhs_c .. }` in a coloured loop: one examg_sys_relax per box.  Rows whose terms
        are all constant stencils are a block system of node fields (exa4_blocksys.py: one examg_bsys_relax per box)."""
        _, jacobi, relax, rows = st
        if len(rows) == 1 and rows[0][0][0] == "fld" and self._field(rows[0][0], fr)[0].layout.is_complex:
            return self._exec_complex_solve(st, boxes, colour, fr)      # one complex node unknown: EXAMG_CRELAX (exa4_complex.py)
        if any(u[0] == "fld" and self._field(u, fr)[0].layout.is_complex for u, _, _ in rows):
            raise Exa4Unsupported("solve locally with more than one unknown over complex fields (the system path knows real cell fields)")
        terms = self._block_solve_rows(rows)
        if terms is not None:
            return self._exec_block_solve(st, terms, boxes, colour, only, where, fr)
        if jacobi:
            raise Exa4Unsupported("solve locally with jacobi")
        if colour is None and fr.mcolour is None:
            raise Exa4Unsupported("solve locally in an uncoloured loop")
        if len(rows) > 3:
            raise Exa4Unsupported("solve locally with more unknowns than 3 (%d)" % len(rows))
        if len(rows) < 2:
            raise Exa4Unsupported("solve locally with one unknown")
        for u, _, _ in rows:
            if u[0] != "fld":
                raise Exa4Unsupported("solve locally: the unknowns are field accesses at the loop's cell")
        us = self._system_fields([u for u, _, _ in rows], fr, "solve locally")
        if len(us) != len(rows):
            raise Exa4Unsupported("solve locally: an unknown named twice")
        self._one_layout(us, "solve locally")
        n = len(us)
        g = [[None] * n for _ in range(n)]
        f, L, lg, lf, coefs = [], None, None, None, []
        for c, (u, lhs, rhs) in enumerate(rows):
            r = self._system_row(lhs, fr) if _contains(lhs, ("sten",)) else None
            if r is None:
                raise Exa4Unsupported("solve locally: the row of %s is not a system row sum (P * F) + [s *] (L * F)" % u[1])
            terms, A, own = r
            if not self._same_access(own, u, fr):
                raise Exa4Unsupported("solve locally: the constant stencil of the row of %s acts on another field" % u[1])
            if L is not None and (L.offsets != A.offsets or L.coefs != A.coefs):
                raise Exa4Unsupported("solve locally: rows whose Laplacians differ")
            L = A
            for G, gs, fx in terms:
                X, s = self._field(fx, fr)
                d = [k for k, (Y, t) in enumerate(us) if Y is X and t == s]
                if not d:
                    raise Exa4Unsupported("solve locally: the unknowns must be exactly the fields of the rows (%s is none)" % X.name)
                if g[c][d[0]] is not None:
                    raise Exa4Unsupported("solve locally: two coefficient terms on %s in one row" % X.name)
                g[c][d[0]] = G.data(gs)
                coefs.append((G, gs))
            if rhs[0] != "fld":
                raise Exa4Unsupported("solve locally: the right-hand side of a row must be a field")
            FF, fs = self._field(rhs, fr)
            f.append((FF, fs))
        self._one_layout(f, "solve locally")
        self._one_layout(coefs, "solve locally")
        w = 1.0 if relax is None else float(self._eval(relax, fr))
        for b, e in boxes:
            self.launches += 1
            self.ops.sys_relax(us[0][0].lc, [X.data(s) for X, s in us], f[0][0].lc, [X.data(s) for X, s in f], coefs[0][0].lc, g, L, w, colour, b, e)

    # -- point-wise set-up statements ---------------------------------------------------------------------------------------------
    def _recognise_pointwise(self, D, ds, rhs, fr):
        """`X = Y * Z`, `X = -Y * Z` (examg_pointwise_mul) and `X = Y - Z` (a copy and examg_axpby), None for anything else."""
        if not D.layout.is_cell:      # the set-up loops of the cell-field systems; node fields keep their refusal
            return None
        if rhs[0] == "bin" and rhs[1] == "*" and rhs[3][0] == "fld" and (rhs[2][0] == "fld" or (rhs[2][0] == "neg" and rhs[2][1][0] == "fld")):
            s, y = (1.0, rhs[2]) if rhs[2][0] == "fld" else (-1.0, rhs[2][1])
            return LoopStmt("pointwise_mul", D, ds, *self._field(y, fr), *self._field(rhs[3], fr), s=s)
        if rhs[0] == "bin" and rhs[1] == "-" and rhs[2][0] == "fld" and rhs[3][0] == "fld":
            Z, zs = self._field(rhs[3], fr)
            if Z is D and zs == ds:
                raise Exa4Unsupported("X = Y - X")
            return LoopStmt("pointwise_sub", D, ds, *self._field(rhs[2], fr), Z, zs)
        return None
