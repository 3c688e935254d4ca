"""Semilinear operators in the ExaSlang-4 interpreter (mixin of Exa4Program): coefficient-expression stencils
(`Stencil gamSten { [0, 0] => gam * exp ( Solution<active>@current ) }`, Testing/NonLinear/FAS_2D_Basic.exa4:26-28) and the four
statements they stand in -- `D = A * U + S * U`, `D = F - ( A * U + S * U )`, `D += A * U + S * U` (one examg_nl_op each) and the
Newton smoother `D = U + w * ( ( F - ( A * U + S * U ) ) / ( diag ( A ) + <point expression over U> ) )`, out of place or in place under
the red-black colouring (one examg_nl_smooth).  A is a constant stencil, S the coefficient-expression stencil; the field S reads need
not be U (`gamSten@coarser * Approximation@coarser` reads Solution).  Everything else around such a stencil is refused by name.
The statements are RECOGNISED here (`_recognise_nonlinear`, the first form the recogniser of exa4_statements.py tries) and launched by
that module's launcher."""
from __future__ import annotations

from .exa4_common import _Frame
from .exa4_parser import Exa4Unsupported, _contains, _walk
from .exa4_statements import LoopStmt
from .lib import MAX_NL_EXPR, NL_ADD, NL_APPLY, NL_RESIDUAL, NL_STACK, NlExprC

_FORMS = "A * U + S * U, F - ( A * U + S * U ), D += A * U + S * U and U + w * ( ( F - ( A * U + S * U ) ) / ( diag ( A ) + d ( U ) ) )"


def _fld_nodes(e):
    return [n for n in _walk(e) if n and n[0] == "fld"]


class Nonlinear:
    # -- coefficient-expression stencils --------------------------------------------------------------------------------------
    def _coef_expr(self, name: str):
        """The centre expression of a coefficient-expression stencil (one [0, .., 0] entry that is an expression over one field access
        at the point and scalars), None for any other stencil; a single bare field access is a point-wise coefficient stencil of a
        system (exa4_systems.py) and none of these."""
        sd = self._stencil_decls.get(name)
        if sd is None or not any(e[0] != "fld" and _contains(e, ("fld",)) for _, e in sd.entries):
            return None
        if len(sd.entries) != 1:
            raise Exa4Unsupported("stencil %s: a coefficient expression beside other entries" % name)
        off, e = sd.entries[0]
        if any(o != 0 for o in off):
            raise Exa4Unsupported("stencil %s: a coefficient expression off the centre" % name)
        if any(len(n) > 4 and n[4] for n in _fld_nodes(e)):       # (the parser refuses `F@[..]` today: no access here carries an offset)
            raise Exa4Unsupported("stencil %s: a coefficient expression with an offset access" % name)
        nf = len({repr(n) for n in _fld_nodes(e)})
        if nf != 1:
            raise Exa4Unsupported("stencil %s: a coefficient expression over %d fields (one field access at the point)" % (name, nf))
        return e

    def _names_coef_expr(self, e) -> bool:
        some = self._field_stencils()     # (exa4_systems.py) empty for most programs: nothing to walk
        return bool(some) and any(n and n[0] == "sten" and n[1] in some and self._coef_expr(n[1]) is not None for n in _walk(e))

    def _nl_program(self, e, lvl: int, what: str):
        """examg_nlexpr_t of a point expression over one field access: the access compiles to EXAMG_OP_U.  Globals are folded into the
        program's constants, so the compiled program is kept under the values of the globals the expression reads (through the
        functions it calls too): a `Var` assigned between two launches gives another program."""
        g = self.globals
        key = ("nl", repr(e), lvl, tuple((n, g[n].__class__, g[n]) for n in sorted(self._globals_below(e, set())[0])))
        if key not in self._fn_cache:
            prog = self._compile_point_expr(e, lvl, {"__u": True})
            if any(name in ("x", "y", "z") for name, _ in prog):
                raise Exa4Unsupported("%s: a coefficient expression over the node position" % what)
            if len(prog) > MAX_NL_EXPR:
                raise Exa4Unsupported("%s: a point program of %d instructions is longer than the bound (%d)" % (what, len(prog), MAX_NL_EXPR))
            sp = deepest = 0
            for name, _ in prog:
                sp += 1 if name in ("const", "u") else (-1 if name in ("+", "-", "*", "/", "pow", "max", "min") else 0)
                deepest = max(deepest, sp)
            if deepest > NL_STACK:
                raise Exa4Unsupported("%s: a point program with a stack of %d values is longer than the bound (%d)" % (what, deepest, NL_STACK))
            self._fn_cache[key] = NlExprC.from_program(prog)
        return self._fn_cache[key]

    # -- the statements ---------------------------------------------------------------------------------------------------------
    def _nl_sum(self, e, fr):
        """(A name, A level, S name, S level, U expr) for `A * U + S * U` in either order (the sum of two doubles does not depend on it),
        None for anything else."""
        if e[0] != "bin" or e[1] != "+":
            return None
        terms = []
        for t in (e[2], e[3]):
            if t[0] != "bin" or t[1] != "*" or t[2][0] != "sten" or t[3][0] != "fld" or t[2][1] in self.transfer:
                return None
            name, lvl = t[2][1], self._level_of(t[2][2], fr)
            if name not in self._stencil_decls and (name, lvl) not in self.stencils:      # (a stencil field is known by its level)
                return None
            terms.append((name, lvl, self._coef_expr(name) is not None, t[3]))
        if terms[0][2] == terms[1][2]:
            return None
        a, s = (terms[0], terms[1]) if terms[1][2] else (terms[1], terms[0])
        if not self._same_access(a[3], s[3], fr):
            return None
        return a[0], a[1], s[0], s[1], a[3]

    def _nl_operands(self, m, fr, what: str):
        """(A, U, uslot, Q, qslot, program c) of a matched sum."""
        aname, alvl, sname, slvl, uexpr = m
        A = self.stencil(aname, alvl)
        if A.cfield is not None:
            raise Exa4Unsupported("%s: a stencil field (%s) as the constant stencil of a semilinear operator" % (what, aname))
        ce = self._coef_expr(sname)
        U, us = self._field(uexpr, fr)
        Q, qs = self._field(_fld_nodes(ce)[0], _Frame(slvl, {}))
        if Q.level != U.level:
            raise Exa4Unsupported("%s: stencil %s reads %s on level %d beside %s on level %d" % (what, sname, Q.name, Q.level, U.name, U.level))
        return A, U, us, Q, qs, self._nl_program(ce, slvl, "stencil %s" % sname)

    def _nl_plain(self, what: str, *fields):
        for X in fields:
            if X.layout.is_cell:
                raise Exa4Unsupported("%s on cell field %s: semilinear operators are built for node fields" % (what, X.name))
            if X.layout.transform:
                raise Exa4Unsupported("%s on colour-split field %s" % (what, X.name))

    def _recognise_nonlinear(self, op, lhs, rhs, D, ds, colour, fr):
        """A loop statement that names a coefficient-expression stencil: the record of its one launch, or a refusal by name."""
        what = "semilinear operator"
        m, F = self._nl_sum(rhs, fr) if op in ("=", "+=") else None, None
        if m is None and op == "=" and rhs[0] == "bin" and rhs[1] == "-" and rhs[2][0] == "fld":
            m, F = self._nl_sum(rhs[3], fr), rhs[2]
        if m is not None:
            A, U, us, Q, qs, c = self._nl_operands(m, fr, what)
            FF, fs = self._field(F, fr) if F is not None else (None, 0)
            self._nl_plain(what, D, U, Q, *(() if FF is None else (FF,)))
            if colour is not None:
                raise Exa4Unsupported("%s in a coloured loop outside the smoother" % what)
            if D is U and ds == us:
                raise Exa4Unsupported("%s assigned to the field it acts on" % what)
            mode = NL_RESIDUAL if F is not None else (NL_APPLY if op == "=" else NL_ADD)
            return LoopStmt("nl_op", D, ds, U, us, FF, fs, A, prog=(mode, Q, qs, c))
        # D = U + w * ( ( F - ( A * U + S * U ) ) / ( diag ( A ) + d ) )   |   U += w * ( .. )
        src = t = None
        if op == "=" and rhs[0] == "bin" and rhs[1] == "+" and rhs[2][0] == "fld":
            src, t = rhs[2], rhs[3]
        elif op == "+=":
            src, t = lhs, rhs
        if t is not None and t[0] == "bin" and t[1] == "*" and self._is_scalar(t[2]) and t[3][0] == "bin" and t[3][1] == "/":
            num, den = t[3][2], t[3][3]
            m = self._nl_sum(num[3], fr) if num[0] == "bin" and num[1] == "-" and num[2][0] == "fld" else None
            if m is not None and den[0] == "bin" and den[1] == "+" and den[2][0] == "call" and den[2][1] == "diag" and len(den[2][3]) == 1:
                what = "nonlinear smoother"
                A, U, us, Q, qs, c = self._nl_operands(m, fr, what)
                da = den[2][3][0]
                if da[0] != "sten" or da[1] != m[0] or self._level_of(da[2], fr) != m[1]:
                    raise Exa4Unsupported("%s: diag of another stencil than %s" % (what, m[0]))
                if not self._same_access(src, m[4], fr):
                    raise Exa4Unsupported("%s: the update starts from another field than the operator acts on" % what)
                if not (Q is U and qs == us):
                    raise Exa4Unsupported("%s: stencil %s reads %s, not the field %s the operator acts on" % (what, m[2], Q.name, U.name))
                if any(len(n) > 4 and n[4] for n in _fld_nodes(den[3])):
                    raise Exa4Unsupported("%s: a denominator with an offset access" % what)
                if _contains(den[3], ("sten", "sentry")) or not _fld_nodes(den[3]) or not all(self._same_access(n, m[4], fr) for n in _fld_nodes(den[3])):
                    raise Exa4Unsupported("%s: a denominator whose field is not %s" % (what, U.name))
                F, fs = self._field(num[2], fr)
                self._nl_plain(what, D, U, F)
                d = self._nl_program(den[3], U.level, what)
                in_place = D is U and ds == us
                if in_place and colour is None:
                    raise Exa4Unsupported("in-place %s without colouring (lexicographic Gauss-Seidel)" % what)
                if not in_place and colour is not None:
                    raise Exa4Unsupported("coloured %s into another slot" % what)
                if colour is not None and not A.faces_only:
                    raise Exa4Unsupported("in-place %s: the red-black colouring does not decouple stencil %s" % (what, m[0]))
                return LoopStmt("nl_smooth", D, ds, U, us, F, fs, A, float(self._eval(t[2], fr)), prog=(c, d))
        names = sorted({n[1] for n in _walk(rhs) if n and n[0] == "sten" and n[1] in self._stencil_decls and self._coef_expr(n[1]) is not None})
        raise Exa4Unsupported("coefficient-expression stencil %s outside the forms %s" % (", ".join(names), _FORMS))
