"""TEST-ONLY restatement of the coupled-system entry points (include/examg.h: examg_sys_op, examg_sys_relax, examg_pointwise_mul) in
numpy, on top of the cell restatement (tests/cell_ops.py).  Every operation in the order the header fixes: coefficient terms
left to right, then the stencil's entries folded in declared order; the local solves of n = 2 and n = 3 as the header spells them.
numpy evaluates each operation in IEEE double, one at a time: no contraction."""
import numpy as np

from cell_ops import CellOracleOps, _empty, _sl, _view

SYS_APPLY, SYS_RESIDUAL = 0, 1


def _shifted(a, ref, b, e, off):
    """View of the box [b, e) of `a` displaced by the stencil offset `off` (x, y, z)."""
    return a[tuple(slice(b[d] + off[d] + ref[d], e[d] + off[d] + ref[d]) for d in (2, 1, 0))]


def _fold(st, a, ref, b, e, off_centre):
    """Entries of the stencil folded left to right in declared order over the box; off_centre: without the centre entry.
    None when no entry takes part."""
    acc = None
    for off, c in zip(st.offsets, st.coefs):
        if off_centre and tuple(off) == (0, 0, 0):
            continue
        t = float(c) * _shifted(a, ref, b, e, off)
        acc = t if acc is None else acc + t
    return acc


def solve2(a, b):
    det = a[0][0] * a[1][1] - a[0][1] * a[1][0]
    return [(b[0] * a[1][1] - a[0][1] * b[1]) / det, (a[0][0] * b[1] - a[1][0] * b[0]) / det]


def solve3(a, b):
    k00 = a[1][1] * a[2][2] - a[1][2] * a[2][1]
    k01 = a[1][2] * a[2][0] - a[1][0] * a[2][2]
    k02 = a[1][0] * a[2][1] - a[1][1] * a[2][0]
    k10 = a[0][2] * a[2][1] - a[0][1] * a[2][2]
    k11 = a[0][0] * a[2][2] - a[0][2] * a[2][0]
    k12 = a[0][1] * a[2][0] - a[0][0] * a[2][1]
    k20 = a[0][1] * a[1][2] - a[0][2] * a[1][1]
    k21 = a[0][2] * a[1][0] - a[0][0] * a[1][2]
    k22 = a[0][0] * a[1][1] - a[0][1] * a[1][0]
    det = (a[0][0] * k00 + a[0][1] * k01) + a[0][2] * k02
    return [((k00 * b[0] + k10 * b[1]) + k20 * b[2]) / det,
            ((k01 * b[0] + k11 * b[1]) + k21 * b[2]) / det,
            ((k02 * b[0] + k12 * b[1]) + k22 * b[2]) / det]


class SystemOracleOps(CellOracleOps):
    name = "system-oracle"

    def sys_op(self, mode, lu, u, lf, f, lg, g, ld, dst, L, row_mask, begin, end):
        if _empty(begin, end):
            return
        n = len(u)
        box_u = []
        for d in range(n):
            a, ref = _view(lu, u[d])
            box_u.append((a, ref, a[_sl(ref, begin, end)]))
        out = {}
        for c in range(n):
            if not (row_mask >> c) & 1:
                continue
            s = None
            for d in range(n):
                if g[c][d] is None:
                    continue
                ga, gref = _view(lg, g[c][d])
                t = ga[_sl(gref, begin, end)] * box_u[d][2]
                s = t if s is None else s + t
            conv = _fold(L, box_u[c][0], box_u[c][1], begin, end, False)
            au = conv if s is None else s + conv
            if mode == SYS_RESIDUAL:
                fa, fref = _view(lf, f[c])
                au = fa[_sl(fref, begin, end)] - au
            out[c] = au
        for c, v in out.items():
            da, dref = _view(ld, dst[c])
            da[_sl(dref, begin, end)] = v

    def sys_relax(self, lu, u, lf, f, lg, g, L, relax, colour, begin, end):
        if _empty(begin, end):
            return
        n = len(u)
        i2, i1, i0 = np.meshgrid(np.arange(begin[2], end[2]), np.arange(begin[1], end[1]), np.arange(begin[0], end[0]), indexing="ij")
        sel = ((i0 + i1 + i2) % 2) == colour
        centre = float(L.coefs[L.diag_index])
        views = [_view(lu, u[c]) for c in range(n)]
        b = []
        for c in range(n):
            fa, fref = _view(lf, f[c])
            fv = fa[_sl(fref, begin, end)]
            off = _fold(L, views[c][0], views[c][1], begin, end, True)
            b.append(fv.copy() if off is None else fv - off)
        m = [[None] * n for _ in range(n)]
        for c in range(n):
            for d in range(n):
                if g[c][d] is None:
                    m[c][d] = np.zeros(sel.shape)
                else:
                    ga, gref = _view(lg, g[c][d])
                    m[c][d] = ga[_sl(gref, begin, end)].copy()
            m[c][c] = m[c][c] + centre if g[c][c] is not None else np.full(sel.shape, centre)
        with np.errstate(all="ignore"):          # cells of the other colour are computed and thrown away
            xs = solve2(m, b) if n == 2 else solve3(m, b)
        for c in range(n):
            a, ref = views[c]
            cur = a[_sl(ref, begin, end)]
            new = xs[c] if relax == 1.0 else cur + float(relax) * (xs[c] - cur)
            a[_sl(ref, begin, end)] = np.where(sel, new, cur)

    def pointwise_mul(self, lx, x, ly, y, ld, dst, s, begin, end):
        if _empty(begin, end):
            return
        xa, xr = _view(lx, x)
        ya, yr = _view(ly, y)
        da, dr = _view(ld, dst)
        da[_sl(dr, begin, end)] = (float(s) * xa[_sl(xr, begin, end)]) * ya[_sl(yr, begin, end)]
