"""TEST-ONLY restatement of the block-system entry points (include/examg.h: examg_bsys_op, examg_bsys_relax, examg_bsys_route) in numpy,
on top of the node oracle layer (tests/oracle_ops.py).  Every operation in the order the header fixes: the entries of a block folded
left to right in declared order, the blocks of a row left to right, the local solves of n = 2 and n = 3 as the header spells them
for examg_sys_relax (tests/system_ops.py).  numpy evaluates each operation in IEEE double, one at a time: no contraction.  The
refusals of the library that an interpreter run could meet are restated too, so the CPU suite sees them."""
import numpy as np

from cell_ops import _empty, _view
from oracle_ops import OracleOps
from system_ops import SYS_APPLY, SYS_RESIDUAL, solve2, solve3  # noqa: F401  (the modes are re-exported)

BSYS_GATHER = 1


class BsysError(RuntimeError):
    pass


ALL = (1, 1, 1)


def _pts(a, ref, b, e, step=ALL, off=(0, 0, 0)):
    """View of the points b, b + step, .. < e of `a`, displaced by the stencil offset `off` (x, y, z)."""
    return a[tuple(slice(b[d] + off[d] + ref[d], e[d] + off[d] + ref[d], step[d]) for d in (2, 1, 0))]


def _fold(st, a, ref, b, e, step, off_centre):
    """Entries of the block folded left to right in declared order over the points; off_centre: without the centre entry.  None when
    no entry takes part."""
    acc = None
    for off, c in zip(st.offsets, st.coefs):
        if off_centre and tuple(off) == (0, 0, 0):
            continue
        t = float(c) * _pts(a, ref, b, e, step, off)
        acc = t if acc is None else acc + t
    return acc


def _row(A, c, views, b, e, step, off_centre):
    """The blocks of row c left to right in d, each folded on its own; None when no entry takes part."""
    row = None
    for d, (a, ref) in enumerate(views):
        if A[c][d] is None:
            continue
        s = _fold(A[c][d], a, ref, b, e, step, off_centre)
        if s is not None:
            row = s if row is None else row + s
    return row


def lattice(col, b, e):
    """(first, step) per axis of the coarsest lattice of the box that holds every point of the colour: an expression on a single axis
    fixes first and step of that axis; the other expressions are left to colour_mask."""
    first, step = list(b), [1, 1, 1]
    for (axes, shift, mod), rem in zip(col.exprs, col.rem):
        if len(axes) == 1 and step[axes[0]] == 1 and mod > 1:
            d = axes[0]
            step[d], first[d] = mod, b[d] + (rem - (shift + b[d])) % mod
    return first, step


def colour_mask(col, b, e, step=ALL):
    """Boolean (z, y, x) array over the points b, b + step, .. < e: those with every colour expression at its remainder."""
    i2, i1, i0 = np.meshgrid(np.arange(b[2], e[2], step[2]), np.arange(b[1], e[1], step[1]), np.arange(b[0], e[0], step[0]), indexing="ij")
    idx = (i0, i1, i2)
    sel = np.ones(i0.shape, dtype=bool)
    for (axes, shift, mod), rem in zip(col.exprs, col.rem):
        sel &= ((shift + sum(idx[d] for d in axes)) % mod) == rem
    return sel


def centre(st):
    """a_cd: the centre coefficient of a block, 0.0 for None or a block without a centre entry."""
    if st is None or (0, 0, 0) not in [tuple(o) for o in st.offsets]:
        return 0.0
    return float(st.coefs[[tuple(o) for o in st.offsets].index((0, 0, 0))])


def check_blocks(who, A, n, nd, mask):
    for c in range(n):
        for d in range(n):
            st = A[c][d]
            if st is None:
                continue
            if st.cfield is not None:
                raise BsysError("%s: block (%d, %d) is a stencil field; the blocks of a block system are constant stencils" % (who, c, d))
            seen = set()
            for k, o in enumerate(st.offsets):
                if any(abs(o[t]) > 1 or (t >= nd and o[t] != 0) for t in range(3)):
                    raise BsysError("%s: block (%d, %d), entry %d (%d, %d, %d) reaches further than one point of a %d-D node field"
                                    % (who, c, d, k, o[0], o[1], o[2], nd))
                if tuple(o) in seen:
                    raise BsysError("%s: block (%d, %d), entry %d repeats the offset (%d, %d, %d)" % (who, c, d, k, o[0], o[1], o[2]))
                seen.add(tuple(o))
        if (mask >> c) & 1 and all(A[c][d] is None for d in range(n)):
            raise BsysError("%s: row %d has no block" % (who, c))


class BlockSysOracleOps(OracleOps):
    name = "blocksys-oracle"

    def bsys_route(self, mode, lu, u, lf, f, ld, dst, A, row_mask, begin, end):
        try:
            check_blocks("examg_bsys_route", A, len(u), lu.nd, row_mask)
        except BsysError:
            return -1
        return 0 if _empty(begin, end) else BSYS_GATHER

    def bsys_op(self, mode, lu, u, lf, f, ld, dst, A, row_mask, begin, end):
        n = len(u)
        check_blocks("examg_bsys_op", A, n, lu.nd, row_mask)
        for c in range(n):
            if (row_mask >> c) & 1 and any(dst[c] is x for x in u):
                raise BsysError("examg_bsys_op: destination %d is an unknown; the operator does not run in place" % c)
            if (row_mask >> c) & 1 and mode == SYS_RESIDUAL and any(dst[c] is x for x in f):
                raise BsysError("examg_bsys_op: destination %d is a right-hand side; the rows are stored one after the other" % c)
        if _empty(begin, end):
            return
        views = [_view(lu, u[d]) for d in range(n)]
        out = {}
        for c in range(n):
            if not (row_mask >> c) & 1:
                continue
            au = _row(A, c, views, begin, end, ALL, False)
            if mode == SYS_RESIDUAL:
                fa, fref = _view(lf, f[c])
                au = _pts(fa, fref, begin, end) - au
            out[c] = au
        for c, v in out.items():
            da, dref = _view(ld, dst[c])
            _pts(da, dref, begin, end)[...] = v

    def bsys_relax(self, lu, u, lf, f, A, relax, col, begin, end):
        n = len(u)
        who = "examg_bsys_relax"
        check_blocks(who, A, n, lu.nd, (1 << n) - 1)
        for c in range(n):
            if centre(A[c][c]) == 0.0:
                raise BsysError("%s: a_%d%d, the centre coefficient of block (%d, %d), is zero" % (who, c, c, c, c))
        for c in range(n):
            for d in range(n):
                for o in (A[c][d].offsets if A[c][d] is not None else ()):
                    if any(o) and not col.decouples([o]):
                        raise BsysError("%s: the colouring does not decouple block (%d, %d): its offset (%d, %d, %d) leads to a point of the "
                                        "same colour, an in-place loop over one colour would depend on the loop order" % (who, c, d, o[0], o[1], o[2]))
        if _empty(begin, end):
            return
        first, step = lattice(col, begin, end)      # the values of the points of other colours that are still computed are thrown away
        if _empty(first, end):
            return
        sel = colour_mask(col, first, end, step)
        views = [_view(lu, u[c]) for c in range(n)]
        b = []
        for c in range(n):
            fa, fref = _view(lf, f[c])
            fv = _pts(fa, fref, first, end, step)
            off = _row(A, c, views, first, end, step, True)
            b.append(fv.copy() if off is None else fv - off)
        m = [[np.full(sel.shape, centre(A[c][d])) for d in range(n)] for c in range(n)]
        with np.errstate(all="ignore"):
            xs = solve2(m, b) if n == 2 else solve3(m, b)
        for c in range(n):
            a, ref = views[c]
            cur = _pts(a, ref, first, end, step)
            new = xs[c] if relax == 1.0 else cur + float(relax) * (xs[c] - cur)
            cur[...] = np.where(sel, new, cur)
