"""TEST-ONLY restatement of the cell-centred entry points (include/examg.h: examg_*_cell, examg_sum, examg_add_scalar) in numpy,
on top of the oracle kernel layer (tests/oracle_ops.py).  Stencil loops, Jacobi, axpby and dot go on through the C oracle, which
takes any layout; what is new for cell fields is restated here, every operation in the order the HIP kernels use."""
import numpy as np

from oracle_ops import OracleOps


def _dims(l):
    ref = [l.pad_l[d] + l.ghost_l[d] for d in range(3)]
    tot = [l.pad_l[d] + l.ghost_l[d] + l.dup_l[d] + l.inner[d] + l.dup_r[d] + l.ghost_r[d] + l.pad_r[d] for d in range(3)]
    return ref, tot


def _view(l, x):
    """x as a (z, y, x) array, and the reference offsets."""
    ref, tot = _dims(l)
    return x.numpy().reshape(tot[2], tot[1], tot[0]), ref


def _sl(ref, b, e):
    return tuple(slice(b[d] + ref[d], e[d] + ref[d]) for d in (2, 1, 0))


def _empty(b, e):
    return any(e[d] <= b[d] for d in range(3))


def _cell_centres(geom, b, e):
    i2, i1, i0 = np.meshgrid(np.arange(b[2], e[2]), np.arange(b[1], e[1]), np.arange(b[0], e[0]), indexing="ij")
    return [(i * geom.h[d] + geom.pos_begin[d]) + 0.5 * geom.h[d] for d, i in enumerate((i0, i1, i2))]


class CellOracleOps(OracleOps):
    name = "cell-oracle"

    # -- sum / add scalar (any localization) ----------------------------------------------------------------------------
    def sum(self, l, x, begin, end, out=None):
        out = self.new_scalar() if out is None else out
        out[0] = 0.0
        if not _empty(begin, end):
            a, ref = _view(l, x)
            out[0] = float(np.sum(a[_sl(ref, begin, end)]))
        return out

    def add_scalar(self, l, x, c, begin, end):
        if _empty(begin, end):
            return
        a, ref = _view(l, x)
        s = _sl(ref, begin, end)
        a[s] = a[s] + float(c)

    # -- expressions at the cell centres --------------------------------------------------------------------------------
    def fill_expr_cell(self, l, x, geom, expr, begin, end):
        if _empty(begin, end):
            return
        a, ref = _view(l, x)
        px, py, pz = _cell_centres(geom, begin, end)
        a[_sl(ref, begin, end)] = self._eval_program(expr.program, px, py, pz)

    def max_err_expr_cell(self, l, x, geom, expr, begin, end, out=None):
        out = self.new_scalar() if out is None else out
        out[0] = 0.0
        if not _empty(begin, end):
            a, ref = _view(l, x)
            px, py, pz = _cell_centres(geom, begin, end)
            out[0] = float(np.max(np.abs(a[_sl(ref, begin, end)] - self._eval_program(expr.program, px, py, pz))))
        return out

    # -- apply bc -------------------------------------------------------------------------------------------------------
    def apply_bc_cell(self, l, x, geom, kind, expr, face_mask):
        """Per face of the mask: the boundary row of cells, tangentially [0, inner); the ghost one step outwards.
        Dirichlet: 2.0 * g(face centre) - interior; Neumann: interior."""
        a, ref = _view(l, x)
        nd = l.nd
        for d in range(nd):
            for side in (0, 1):
                if not face_mask & (1 << (2 * d + side)):
                    continue
                b, e = [0, 0, 0], [1, 1, 1]
                for t in range(nd):
                    b[t], e[t] = 0, l.inner[t]
                if side == 0:
                    e[d] = 1
                else:
                    b[d] = l.inner[d] - 1
                g_b, g_e = list(b), list(e)
                g_b[d] += 1 if side else -1
                g_e[d] += 1 if side else -1
                interior = a[_sl(ref, b, e)].copy()
                if kind == 1:
                    a[_sl(ref, g_b, g_e)] = interior
                    continue
                p = _cell_centres(geom, b, e)
                idx = l.inner[d] if side else 0
                p[d] = np.full_like(p[d], idx * geom.h[d] + geom.pos_begin[d])
                a[_sl(ref, g_b, g_e)] = (2.0 * self._eval_program(expr.program, *p)) - interior

    # -- transfers ------------------------------------------------------------------------------------------------------
    def restrict_cell(self, lfine, rf, lc, fc, scale, begin, end):
        """fc(I) = sum over the children in the order x offset outermost, then y, then z of (scale * 0.5^d) * rf(2I + o)."""
        if _empty(begin, end):
            return
        nd = lfine.nd
        wgt = scale * (0.125 if nd == 3 else 0.25)
        af, rff = _view(lfine, rf)
        ac, rc = _view(lc, fc)
        acc = None
        offs = [(a_, b_, c_) for a_ in (0, 1) for b_ in (0, 1) for c_ in ((0, 1) if nd == 3 else (0,))]
        for o in offs:
            sl = tuple(slice(2 * begin[d] + o[d] + rff[d], 2 * (end[d] - 1) + o[d] + rff[d] + 1, 2) if d < nd else
                       slice(begin[d] + rff[d], end[d] + rff[d]) for d in (2, 1, 0))
            tv = wgt * af[sl]
            acc = tv if acc is None else acc + tv
        ac[_sl(rc, begin, end)] = acc

    def prolong_add_cell(self, lc, uc, lfine, uf, begin, end):
        """uf(i) = uf(i) + uc(floor(i / 2)) over the fine box."""
        if _empty(begin, end):
            return
        nd = lfine.nd
        af, rff = _view(lfine, uf)
        ac, rc = _view(lc, uc)
        idx = []
        for d in (2, 1, 0):
            i = np.arange(begin[d], end[d])
            idx.append((i // 2 if d < nd else i) + rc[d])
        parent = ac[np.ix_(*idx)]
        s = _sl(rff, begin, end)
        af[s] = af[s] + parent
