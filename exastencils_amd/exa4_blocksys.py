"""Coupled systems of scalar node fields whose blocks are constant stencils, in the ExaSlang-4 interpreter (mixin of Exa4Program):
rows `sum [scalars *] (S * F)` with a factor in front of a parenthesised sum, as Examples/LinearElasticity/2D_FD_LinearElasticity_fromL2
writes them -- `( lambda + mu ) * ( dxx * u + dxy * v ) + lambda * ( Laplace * u )` -- and `solve locally` over 2 or 3 node unknowns
inside a coloured block.  Rows are RECOGNISED here for the one recogniser of loop-body assignments (exa4_statements.py) and launched
by its launcher, consecutive rows of one loop body as ONE examg_bsys_op with the combined mask; `solve locally` is a whole-loop form
and issues one examg_bsys_relax per colour and box (include/examg.h).

Stencil arithmetic is done here, as the generator does it before it prints a convolution (include/examg.h, "STENCIL ARITHMETIC"): the
scalar factor of a term, evaluated left to right as written, multiplies every coefficient; terms on one unknown are added into one
block in order of appearance -- an offset already present gets c_old + c_new, a new offset is appended."""
from __future__ import annotations

import dataclasses

from .exa4_parser import Exa4Unsupported
from .exa4_statements import LoopStmt
from .exa4_systems import _flatten
from .field import Colouring, Stencil
from .lib import SYS_APPLY, SYS_RESIDUAL


def _merge(block, offsets, coefs):
    """block (a Stencil or None) plus the entries: an offset already present gets c_old + c_new, a new one is appended."""
    offs, co = (list(block.offsets), list(block.coefs)) if block is not None else ([], [])
    for o, c in zip(offsets, coefs):
        if o in offs:
            k = offs.index(o)
            co[k] = co[k] + c
        else:
            offs.append(o)
            co.append(c)
    return Stencil(offs, co)


class BlockSystems:
    # -- rows -----------------------------------------------------------------------------------------------------------------
    def _block_terms(self, e, scal=()):
        """The terms [(scalar factors in order, stencil node, field node)] of a row, None when the expression is no sum of
        `[scalars *] (S * F)` terms and factored sums of them."""
        if e[0] == "bin" and e[1] == "+":
            a, b = self._block_terms(e[2], scal), self._block_terms(e[3], scal)
            return None if a is None or b is None else a + b
        if e[0] != "bin" or e[1] != "*":
            return None
        fac = _flatten(e, "*")
        rest = [x for x in fac if not self._is_scalar(x)]
        lead = tuple(scal) + tuple(x for x in fac if self._is_scalar(x))
        if len(rest) == 1 and rest[0][0] == "bin" and rest[0][1] == "+" and fac[-1] is rest[0]:
            return self._block_terms(rest[0], lead)      # a factor in front of a parenthesised sum
        if len(rest) == 2 and rest[0][0] == "sten" and rest[1][0] == "fld" and fac[-1] is rest[1] and rest[0][1] not in self.transfer:
            return [(lead, rest[0], rest[1])]
        return None

    def _is_block_row(self, terms) -> bool:
        """... and none of its stencils is a point-wise coefficient stencil: those rows are the cell systems' (exa4_systems.py), which
        names what it refuses of them."""
        return terms is not None and not any(t[1][1] in self._stencil_decls and self._coef_field(t[1][1]) is not None for t in terms)

    def _block_row(self, terms, us, what, fr):
        """The blocks {d: Stencil} of a row over the unknowns `us` [(Field, slot)] -- a term on a field not among them extends the list when
        `us` is open (a plain row) and is refused otherwise -- with the host's stencil arithmetic applied."""
        row, fixed = {}, what.startswith("solve locally")
        for scal, sten, fx in terms:
            X, xs = self._field(fx, fr)
            if X.layout.is_cell or X.layout.is_complex:
                raise Exa4Unsupported("%s: %s is a %s field; block systems are built for real node fields"
                                      % (what, X.name, "cell" if X.layout.is_cell else "complex"))
            d = [k for k, (Y, t) in enumerate(us) if Y is X and t == xs]
            if not d:
                if fixed:
                    raise Exa4Unsupported("%s: the unknowns must be exactly the fields of the rows (%s is none)" % (what, X.name))
                us.append((X, xs))
                d = [len(us) - 1]
            name = sten[1]
            if name in self._stencil_decls and (name in self._field_stencils() or self._coef_expr(name) is not None):
                raise Exa4Unsupported("%s: stencil %s has a field or an expression over a field in an entry; the blocks of a system are constant stencils"
                                      % (what, name))
            A = self.stencil(name, self._level_of(sten[2], fr))
            if A.cfield is not None:
                raise Exa4Unsupported("%s: a stencil field (%s) as a block of a system" % (what, name))
            if getattr(A, "is_axis", False):
                raise Exa4Unsupported("%s: a stencil over the grid's virtual fields (%s: per-axis tables) as a block of a system" % (what, name))
            if getattr(A, "has_complex_entries", False):
                raise Exa4Unsupported("%s: a stencil with complex entries (%s) as a block of a system" % (what, name))
            if any(abs(c) > 1 for o in A.offsets for c in o):
                raise Exa4Unsupported("%s: stencil %s reaches further than one point (reach 2); the blocks of a system have reach 1" % (what, name))
            s = None
            for x in scal:        # the factor as written, left to right
                v = float(self._eval(x, fr))
                s = v if s is None else s * v
            coefs = list(A.coefs) if s is None else [s * c for c in A.coefs]
            row[d[0]] = _merge(row.get(d[0]), A.offsets, coefs)
        return row

    def _check_block_fields(self, fields, what):
        for F, _ in fields:
            if F.layout.is_cell or F.layout.is_complex:
                raise Exa4Unsupported("%s: %s is a %s field; block systems are built for real node fields"
                                      % (what, F.name, "cell" if F.layout.is_cell else "complex"))
            if F.layout.transform:
                raise Exa4Unsupported("%s over colour-split field %s" % (what, F.name))
        if self.domain.world_size != 1 or any(self.domain.periodic):
            raise Exa4Unsupported("%s on more than one block or with a periodic axis" % what)

    def _recognise_block_row(self, D, ds, rhs, colour, fr):
        """`X = row` (EXAMG_SYS_APPLY) and `X = rhs - ( row )` (EXAMG_SYS_RESIDUAL) with a row over at least two node unknowns: the record
        of one examg_bsys_op with a one-row mask, None when the expression is no such row."""
        mode, F, row = SYS_APPLY, None, rhs
        if rhs[0] == "bin" and rhs[1] == "-" and rhs[2][0] == "fld":
            mode, F, row = SYS_RESIDUAL, rhs[2], rhs[3]
        terms = self._block_terms(row)
        if not self._is_block_row(terms):
            return None
        named = []
        for t in terms:
            X = self._field(t[2], fr)
            if not any(X[0] is Y and X[1] == s for Y, s in named):
                named.append(X)
        if len(named) < 2:      # one unknown: a stencil loop, or nothing the kernels know
            return None
        what = "system row"
        if colour is not None or fr.mcolour is not None:
            raise Exa4Unsupported("system row in a coloured loop outside solve locally")
        if fr.contract is not None:
            raise Exa4Unsupported("system row in a loop under contraction")
        us = []
        blocks = self._block_row(terms, us, what, fr)
        if len(us) > 3:
            raise Exa4Unsupported("system row over %d unknowns (2 or 3)" % len(us))
        FF, fs = self._field(F, fr) if F is not None else (None, 0)
        self._check_block_fields(us + [(D, ds)] + ([(FF, fs)] if FF is not None else []), what)
        self._one_layout(us, what)
        if any(D is U and ds == s for U, s in us):
            raise Exa4Unsupported("system row assigned to its own unknown %s" % D.name)
        return LoopStmt("bsys_row", D, ds, F=FF, fs=fs, prog=(mode, tuple(us), ((D, ds, FF, fs, blocks),)))

    def _merge_block_rows(self, k: LoopStmt, rest, fr):
        """The record `k` of a system row with the row statements that follow it in the loop body folded in -- same mode, same unknowns,
        destinations of one layout and right-hand sides of one layout: ONE launch with the combined mask -- and how many were folded."""
        mode, us, rows = k.prog
        taken = 0
        for st in rest:
            if len(rows) == len(us) or st[0] != "assign" or st[1] != "=" or st[2][0] != "fld":
                break
            n = self._recognise_or_none(st, fr)
            if n is None or n.kind != "bsys_row" or n.prog[0] != mode:
                break
            nus, (D, ds, F, fs, blocks) = n.prog[1], n.prog[2][0]
            if len(nus) != len(us) or any(not any(X is Y and s == t for Y, t in us) for X, s in nus):
                break
            if D.layout != rows[0][0].layout or (F is not None and F.layout != rows[0][2].layout) or any(D is R[0] and ds == R[1] for R in rows):
                break
            perm = [[j for j, (Y, t) in enumerate(us) if Y is X and s == t][0] for X, s in nus]      # the d index: first appearance in the loop
            rows = rows + ((D, ds, F, fs, {perm[d]: A for d, A in blocks.items()}),)
            taken += 1
        return dataclasses.replace(k, prog=(mode, us, rows)), taken

    def _check_block_loop(self, only, where, fr):
        if only is not None or where is not None or fr.contract is not None:
            raise Exa4Unsupported("system row in a loop with `only`, `where` or under contraction")

    def _launch_block_rows(self, k: LoopStmt, b, e):
        mode, us, rows = k.prog
        n = len(us)
        A = [[None] * n for _ in range(n)]
        f, dst = [None] * n, [None] * n
        for c, (D, ds, F, fs, blocks) in enumerate(rows):
            dst[c] = D.data(ds)
            f[c] = F.data(fs) if F is not None else None
            for d, S in blocks.items():
                A[c][d] = S
        F0 = rows[0][2]
        self.ops.bsys_op(mode, us[0][0].lc, [X.data(s) for X, s in us], F0.lc if F0 is not None else None, f, rows[0][0].lc, dst, A,
                         (1 << len(rows)) - 1, b, e)

    # -- solve locally ------------------------------------------------------------------------------------------------------------
    def _block_solve_rows(self, rows):
        """The terms of every row of a `solve locally`, None when it is no block system (a row that is no sum of stencil terms, or a
        point-wise coefficient stencil in one: the cell systems' form)."""
        out = []
        for _, lhs, _ in rows:
            t = self._block_terms(lhs)
            if not self._is_block_row(t):
                return None
            out.append(t)
        return out

    def _exec_block_solve(self, st, terms, boxes, colour, only, where, fr):
        """`solve locally [relax w] { u => rowU == f_u  v => rowV == f_v [w => ..] }` over node unknowns inside a coloured block: one
        examg_bsys_relax per box for the current colour."""
        _, jacobi, relax, rows = st
        what = "solve locally"
        if jacobi:
            raise Exa4Unsupported("solve locally with jacobi")
        if colour is None and fr.mcolour is None:
            raise Exa4Unsupported("solve locally in an uncoloured loop")
        if only is not None or where is not None or fr.contract is not None:
            raise Exa4Unsupported("solve locally over node fields in a loop with `only`, `where` or under contraction")
        if len(rows) > 3:
            raise Exa4Unsupported("solve locally with more unknowns than 3 (%d)" % len(rows))
        for u, _, _ in rows:
            if u[0] != "fld":
                raise Exa4Unsupported("solve locally: the unknowns are field accesses at the loop's point")
        us = []
        for u, _, _ in rows:
            X = self._field(u, fr)
            if any(X[0] is Y and X[1] == t for Y, t in us):
                raise Exa4Unsupported("solve locally: an unknown named twice")
            us.append(X)
        n = len(us)
        if n < 2:
            raise Exa4Unsupported("solve locally with one unknown")
        A = [[None] * n for _ in range(n)]
        f = []
        for c, (t, (u, _, rhs)) in enumerate(zip(terms, rows)):
            for d, S in self._block_row(t, us, what, fr).items():
                A[c][d] = S
            if rhs[0] != "fld":
                raise Exa4Unsupported("solve locally: the right-hand side of a row must be a field")
            f.append(self._field(rhs, fr))
        for d, (X, _) in enumerate(us):
            if all(A[c][d] is None for c in range(n)):
                raise Exa4Unsupported("solve locally: unknown %s is missing from the rows" % X.name)
        self._check_block_fields(us + f, what)
        self._one_layout(us, what)
        self._one_layout(f, what)
        col = fr.mcolour if fr.mcolour is not None else Colouring(((tuple(range(self.nd)), 0, 2),), (colour,))
        for c in range(n):
            for d in range(n):
                for o in (A[c][d].offsets if A[c][d] is not None else ()):
                    if any(o) and not col.decouples([o]):
                        raise Exa4Unsupported("solve locally: the colouring does not decouple the system: block (%s, %s) reads %s at offset %s, a point "
                                              "of the row's own colour -- the generated loop would depend on its order"
                                              % (us[c][0].name, us[d][0].name, us[d][0].name, list(o[:self.nd])))
        w = 1.0 if relax is None else float(self._eval(relax, fr))
        for b, e in boxes:
            self.launches += 1
            self.ops.bsys_relax(us[0][0].lc, [X.data(s) for X, s in us], f[0][0].lc, [X.data(s) for X, s in f], A, w, col, b, e)
