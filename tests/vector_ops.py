"""TEST-ONLY restatement of the entry points of vector-valued cell fields (include/examg.h: examg_vec_*) in numpy, on top of the
system restatement (tests/system_ops.py).  A vector argument is (layout, array of n * size doubles), component c at c * size.  Every
operation in the order the header fixes: the present elements of a row of an entry left to right, the entries in declared order; the
local solves are system_ops.solve2 / solve3.  numpy evaluates each operation in IEEE double, one at a time: no contraction."""
import numpy as np

from cell_ops import _dims, _empty, _sl, _view
from system_ops import SYS_APPLY, SYS_RESIDUAL, SystemOracleOps, _shifted, solve2, solve3  # noqa: F401


def _size(l):
    _, tot = _dims(l)
    return tot[0] * tot[1] * tot[2]


def comp(l, x, c):
    """Component c of the vector argument (l, x): a view of its plane."""
    n = _size(l)
    return x[c * n:(c + 1) * n]


def _centre(el, lg, begin, end):
    """The centre element over the box: k + g, g or k (a float)."""
    kv, g = el
    if g is None:
        return float(kv)
    ga, gref = _view(lg, g)
    gv = ga[_sl(gref, begin, end)]
    return gv if kv is None else float(kv) + gv


def _mu(n, M, lg, views, begin, end):
    """Mu_c over the box for every c; views[d] = (array, ref) of u_d."""
    out = []
    for c in range(n):
        acc = None
        for k, off in enumerate(M.offsets):
            t = None
            if tuple(off) == (0, 0, 0):
                for d in range(n):
                    el = M.elems[k][c][d]
                    if el is None:
                        continue
                    p = _centre(el, lg, begin, end) * _shifted(views[d][0], views[d][1], begin, end, off)
                    t = p if t is None else t + p
            else:
                el = M.elems[k][c][c]
                if el is not None:
                    t = float(el[0]) * _shifted(views[c][0], views[c][1], begin, end, off)
            if t is not None:
                acc = t if acc is None else acc + t
        shape = tuple(end[d] - begin[d] for d in (2, 1, 0))
        out.append(np.zeros(shape) if acc is None else acc)
    return out


RED_BLOCK, RED_MAX_BLOCKS, ROW_MIN = 256, 2048, 128      # csrc/kernels_blas.hip


def _block_reduce(v):
    """v[..., 256] -> [...]: the shuffle tree of every wave of 64 (offsets 32 .. 1: lane 0 ends with ((v0 + v32) + (v16 + v48)) + ..),
    then the four wave sums one after the other."""
    w = v.reshape(v.shape[:-1] + (RED_BLOCK // 64, 64))
    o = 32
    while o:
        w = w[..., :o] + w[..., o:2 * o]
        o //= 2
    w = w[..., 0]
    r = w[..., 0]
    for k in range(1, RED_BLOCK // 64):
        r = r + w[..., k]
    return r


def _tree_sum(t):
    """Sum of the terms t[z, y, x] of a box as examg_dot's kernels add them (k_dot_partial, or k_dot_rows for rows of 128 cells and
    more; k_reduce_final): every addition in the library's order, so the result has the library's bits."""
    n2, n1, n0 = t.shape
    total = t.size
    nb = max(1, min(RED_MAX_BLOCKS, -(-total // (RED_BLOCK * 4))))
    if n0 >= ROW_MIN:
        rows = t.reshape(n2 * n1, n0)
        nw = nb * (RED_BLOCK // 64)
        s = np.zeros((nw, 64))
        for r in range(rows.shape[0]):          # wave r % nw takes row r; a lane its pairs 2 * lane + 128 * k, first cell then second
            for c in range(0, n0, 128):
                seg = rows[r, c:c + 128]
                even, odd = seg[0::2], seg[1::2]
                s[r % nw, :even.size] = s[r % nw, :even.size] + even
                s[r % nw, :odd.size] = s[r % nw, :odd.size] + odd
        acc = s.reshape(nb, RED_BLOCK)
    else:
        threads = nb * RED_BLOCK
        flat = t.reshape(-1)
        acc = np.zeros(threads)
        for k in range(0, total, threads):      # thread j takes the cells j, j + threads, ..
            chunk = flat[k:k + threads]
            acc[:chunk.size] = acc[:chunk.size] + chunk
        acc = acc.reshape(nb, RED_BLOCK)
    part = _block_reduce(acc)
    fin = np.zeros(RED_BLOCK)
    for k in range(0, nb, RED_BLOCK):           # k_reduce_final: thread i adds part[i], part[i + 256], ..
        chunk = part[k:k + RED_BLOCK]
        fin[:chunk.size] = fin[:chunk.size] + chunk
    return float(_block_reduce(fin))


class VectorOracleOps(SystemOracleOps):
    name = "vector-oracle"

    @staticmethod
    def _lg(M, lu):
        gl = M.glayout if M.glayout is not None else lu
        return gl.c_struct() if hasattr(gl, "c_struct") else gl

    def vec_op(self, mode, n, lu, u, lf, f, ld, dst, M, begin, end):
        if _empty(begin, end):
            return
        views = [_view(lu, comp(lu, u, d)) for d in range(n)]
        mu = _mu(n, M, self._lg(M, lu), views, begin, end)
        for c in range(n):
            v = mu[c]
            if mode == SYS_RESIDUAL:
                fa, fref = _view(lf, comp(lf, f, c))
                v = fa[_sl(fref, begin, end)] - v
            da, dref = _view(ld, comp(ld, dst, c))
            da[_sl(dref, begin, end)] = v

    def vec_smooth(self, n, lu, u, lf, f, M, relax, colour, begin, end):
        if _empty(begin, end):
            return
        lg = self._lg(M, lu)
        i2, i1, i0 = np.meshgrid(np.arange(begin[2], end[2]), np.arange(begin[1], end[1]), np.arange(begin[0], end[0]), indexing="ij")
        sel = ((i0 + i1 + i2) % 2) == colour
        views = [_view(lu, comp(lu, u, d)) for d in range(n)]
        mu = _mu(n, M, lg, views, begin, end)
        r = []
        for c in range(n):
            fa, fref = _view(lf, comp(lf, f, c))
            r.append(fa[_sl(fref, begin, end)] - mu[c])
        kc = M.centre_index
        m = [[None] * n for _ in range(n)]
        for c in range(n):
            for d in range(n):
                el = M.elems[kc][c][d]
                v = 0.0 if el is None else _centre(el, lg, begin, end)
                m[c][d] = np.zeros(sel.shape) + v
        with np.errstate(all="ignore"):          # cells of the other colour are computed and thrown away
            xs = solve2(m, r) if n == 2 else solve3(m, r)
        for c in range(n):
            a, ref = views[c]
            cur = a[_sl(ref, begin, end)]
            new = cur + xs[c] if relax == 1.0 else cur + float(relax) * xs[c]
            a[_sl(ref, begin, end)] = np.where(sel, new, cur)

    def vec_dot(self, n, lx, x, ly, y, begin, end, out=None):
        """The per-cell terms in the header's order, summed through the launch plan of examg_dot restated addition by addition
        (_tree_sum): the bits of the library."""
        out = self.new_scalar() if out is None else out
        out[0] = 0.0
        if not _empty(begin, end):
            t = None
            for c in range(n):
                xa, xr = _view(lx, comp(lx, x, c))
                ya, yr = _view(ly, comp(ly, y, c))
                p = xa[_sl(xr, begin, end)] * ya[_sl(yr, begin, end)]
                t = p if t is None else t + p
            out[0] = _tree_sum(np.ascontiguousarray(t))
        return out

    # -- the scalar entry point on every component --------------------------------------------------------------------------------
    def vec_set(self, n, l, x, v, begin, end):
        for c in range(n):
            self.set(l, comp(l, x, c), v, begin, end)

    def vec_axpby(self, n, lx, x, ly, y, a, b, begin, end):
        for c in range(n):
            self.axpby(lx, comp(lx, x, c), ly, comp(ly, y, c), a, b, begin, end)

    def vec_restrict_cell(self, n, lfine, rf, lc, fc, scale, begin, end):
        for c in range(n):
            self.restrict_cell(lfine, comp(lfine, rf, c), lc, comp(lc, fc, c), scale, begin, end)

    def vec_prolong_add_cell(self, n, lc, uc, lfine, uf, begin, end):
        for c in range(n):
            self.prolong_add_cell(lc, comp(lc, uc, c), lfine, comp(lfine, uf, c), begin, end)

    def vec_apply_bc_cell(self, n, l, x, geom, kind, face_mask):
        if kind != 1:
            raise ValueError("vec_apply_bc_cell: Neumann only")
        for c in range(n):
            self.apply_bc_cell(l, comp(l, x, c), geom, kind, None, face_mask)
