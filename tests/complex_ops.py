"""TEST-ONLY numpy restatement of the complex entry points of include/examg.h (examg_cstencil_op .. examg_cfrom_parts): real fp64 arithmetic on
the two parts, every sum and product in the order the header writes it.  numpy rounds each elementwise operation once and fuses nothing, so
the point-wise results are the bits the kernels must produce.

Arrays are flat float64 arrays (numpy, or CPU torch tensors: written through) of 2 * size(layout) doubles, (re, im) per point; layouts are
lib.LayoutC structs, as the kernel layer takes them.  ComplexOps has the method names of exastencils_amd.ops.HipOps."""
import math

import numpy as np

APPLY, RESIDUAL, SMOOTH, CRELAX = 0, 1, 2, 3
C_XPAY, C_XMAY, C_XPAYMBZ = 0, 1, 2


def _np(a):
    return a.numpy() if hasattr(a, "numpy") else a


def _tot(l, d):
    return l.pad_l[d] + l.ghost_l[d] + l.dup_l[d] + l.inner[d] + l.dup_r[d] + l.ghost_r[d] + l.pad_r[d]


def _ref(l, d):
    return l.pad_l[d] + l.ghost_l[d]


def cview(l, a):
    """The complex field as [z, y, x, part] (a view)."""
    return _np(a).reshape(_tot(l, 2), _tot(l, 1), _tot(l, 0), 2)


def rview(l, a):
    """A real field as [z, y, x] (a view)."""
    return _np(a).reshape(_tot(l, 2), _tot(l, 1), _tot(l, 0))


def _sl(l, begin, end, off=(0, 0, 0)):
    """Index of the box shifted by off, in [z, y, x] order."""
    return tuple(slice(begin[d] + off[d] + _ref(l, d), end[d] + off[d] + _ref(l, d)) for d in (2, 1, 0))


def cmul(c, vr, vi):
    """c . v on the parts: a real c scales (how `double * std::complex` multiplies)."""
    a, b = complex(c).real, complex(c).imag
    if b == 0.0:
        return a * vr, a * vi
    return a * vr - b * vi, a * vi + b * vr


def cdiv(zr, zi, c):
    cr, ci = complex(c).real, complex(c).imag
    if ci == 0.0:
        return zr / cr, zi / cr
    den = cr * cr + ci * ci
    return (zr * cr + zi * ci) / den, (zi * cr - zr * ci) / den


def colour_mask(begin, end, colour):
    """[z, y, x] mask of the box's points with (i0 + i1 + i2) % 2 == colour; all of them for colour -1."""
    i2, i1, i0 = np.meshgrid(*[np.arange(begin[d], end[d]) for d in (2, 1, 0)], indexing="ij")
    if colour < 0:
        return np.ones(i0.shape, dtype=bool)
    return ((i0 + i1 + i2) & 1) == colour


def fold(entries, get, skip=None):
    """The entries (offset, coefficient) folded left to right in declared order; `skip`: the index of an entry left out."""
    acc = None
    for k, (o, c) in enumerate(entries):
        if k == skip:
            continue
        vr, vi = get(o)
        tr, ti = cmul(c, vr, vi)
        acc = (tr, ti) if acc is None else (acc[0] + tr, acc[1] + ti)
    return acc


def sum_terms(terms, order="pairwise"):
    """One sum of a 1-D array of terms in a named order: numpy's pairwise tree, the same on the reversed array, or one after the other."""
    if order == "pairwise":
        return float(np.sum(terms))
    if order == "reversed":
        return float(np.sum(terms[::-1]))
    if order == "sequential":
        s = 0.0
        for t in terms.tolist():
            s = s + t
        return s
    raise ValueError(order)


class ComplexOps:
    name = "complex-numpy"

    def __init__(self, dot_order="pairwise"):
        self.dot_order = dot_order

    # -- plumbing (what a program needs of a kernel layer) ------------------------------------------------------------------------------
    def new_array(self, n):
        return np.zeros(int(n), dtype=np.float64)

    def new_complex_array(self, npoints):
        return np.zeros(2 * int(npoints), dtype=np.float64)

    def new_complex_scalar(self):
        return np.zeros(2, dtype=np.float64)

    def complex_value(self, t):
        return complex(t[0], t[1])

    def to_host(self, t):
        return _np(t)

    def from_host(self, a):
        return np.array(a, dtype=np.float64)

    def synchronize(self):
        pass

    # -- the two REAL entry points a complex program runs on the real view of its fields (include/examg.h: examg_set, examg_axpby) -------------
    def set(self, l, x, v, begin, end):
        rview(l, x)[_sl(l, begin, end)] = v

    def axpby(self, lx, x, ly, y, a, b, begin, end):
        X, Y = rview(lx, x)[_sl(lx, begin, end)], rview(ly, y)[_sl(ly, begin, end)]
        if b == 0.0:
            Y[...] = a * X
        elif b == 1.0:
            Y[...] = Y + a * X
        elif a == 1.0:
            Y[...] = X + b * Y
        else:
            Y[...] = a * X + b * Y

    # -- examg_cstencil_op ------------------------------------------------------------------------------------------------------------------
    def cstencil_op(self, mode, lu, u, lf, rhs, ld, dst, st, w, colour, begin, end):
        if any(end[d] <= begin[d] for d in range(3)):
            return
        U = cview(lu, u).copy()      # every point reads the field as it was (what the kernels guarantee where u and dst may alias)
        entries = list(zip(st.offsets, st.coefs))

        def get(o):
            v = U[_sl(lu, begin, end, o)]
            return v[..., 0], v[..., 1]

        if mode == CRELAX:
            assert colour in (0, 1) and complex(w).imag == 0.0
            dst, ld = u, lu
            diag = st.offsets.index((0, 0, 0))
            acc = fold(entries, get, skip=diag)
        else:
            acc = fold(entries, get)
        if mode != APPLY:
            F = cview(lf, rhs)[_sl(lf, begin, end)]
            fr, fi = F[..., 0], F[..., 1]
        ur, ui = get((0, 0, 0))
        if mode == APPLY:
            rr, ri = acc
        elif mode == RESIDUAL:
            rr, ri = fr - acc[0], fi - acc[1]
        elif mode == SMOOTH:
            tr, ti = cmul(w, fr - acc[0], fi - acc[1])
            rr, ri = ur + tr, ui + ti
        else:
            br, bi = (fr, fi) if acc is None else (fr - acc[0], fi - acc[1])
            xr, xi = cdiv(br, bi, st.coefs[diag])
            wr = complex(w).real
            if wr == 1.0:
                rr, ri = xr, xi
            else:
                om = 1.0 - wr
                rr, ri = ur * om + wr * xr, ui * om + wr * xi
        m = colour_mask(begin, end, colour)
        D = cview(ld, dst)[_sl(ld, begin, end)]
        D[..., 0][m] = rr[m]
        D[..., 1][m] = ri[m]

    # -- examg_clincomb ---------------------------------------------------------------------------------------------------------------------
    def clincomb(self, form, lx, x, ly, y, lz, z, ld, dst, a, b, begin, end):
        X = cview(lx, x)[_sl(lx, begin, end)]
        Y = cview(ly, y)[_sl(ly, begin, end)]
        xr, xi, yr, yi = X[..., 0].copy(), X[..., 1].copy(), Y[..., 0].copy(), Y[..., 1].copy()
        if form == C_XPAY:
            tr, ti = cmul(a, yr, yi)
            rr, ri = xr + tr, xi + ti
        elif form == C_XMAY:
            tr, ti = cmul(a, yr, yi)
            rr, ri = xr - tr, xi - ti
        else:
            Z = cview(lz, z)[_sl(lz, begin, end)]
            sr, si = cmul(b, Z[..., 0].copy(), Z[..., 1].copy())
            tr, ti = cmul(a, yr - sr, yi - si)
            rr, ri = xr + tr, xi + ti
        D = cview(ld, dst)[_sl(ld, begin, end)]
        D[..., 0] = rr
        D[..., 1] = ri

    # -- examg_cdot: the unconjugated sum; the ORDER of the sum is this object's dot_order (the kernels have a tree of their own) -----------------
    @staticmethod
    def cdot_terms(lx, x, ly, y, begin, end):
        """The 2 K rounded terms of each part, interleaved per point as the header adds them: (xr yr, -(xi yi)) and (xr yi, xi yr)."""
        X = cview(lx, x)[_sl(lx, begin, end)].reshape(-1, 2)
        Y = cview(ly, y)[_sl(ly, begin, end)].reshape(-1, 2)
        re = np.stack([X[:, 0] * Y[:, 0], -(X[:, 1] * Y[:, 1])], axis=1).reshape(-1)
        im = np.stack([X[:, 0] * Y[:, 1], X[:, 1] * Y[:, 0]], axis=1).reshape(-1)
        return re, im

    def cdot(self, lx, x, ly, y, begin, end, out=None):
        out = self.new_complex_scalar() if out is None else out
        re, im = self.cdot_terms(lx, x, ly, y, begin, end)
        out[0], out[1] = sum_terms(re, self.dot_order), sum_terms(im, self.dot_order)
        return out

    # -- the node transfer operators on each part (the terms and their order: include/examg.h, examg_restrict / examg_prolong_add) --------------
    def crestrict(self, lfine, rf, lc, fc, scale, begin, end):
        nd = lfine.nd
        F = cview(lfine, rf)
        w1 = (0.25, 0.5, 0.25)
        idx = [[2 * np.arange(begin[d], end[d]) + _ref(lfine, d) for d in range(3)]]
        i0, i1, i2 = idx[0]
        if nd == 2:
            i2 = np.arange(begin[2], end[2]) + _ref(lfine, 2)
        acc = None
        for a in (-1, 0, 1):
            for b in (-1, 0, 1):
                for c in ((-1, 0, 1) if nd == 3 else (0,)):
                    wgt = scale * (w1[a + 1] * w1[b + 1]) if nd == 2 else scale * ((w1[a + 1] * w1[b + 1]) * w1[c + 1])
                    tv = wgt * F[np.ix_(i2 + c, i1 + b, i0 + a)]
                    acc = tv if acc is None else acc + tv
        cview(lc, fc)[_sl(lc, begin, end)] = acc

    def cprolong_add(self, lc, uc, lfine, uf, begin, end):
        nd = lfine.nd
        Cc = cview(lc, uc)
        per_dim = []
        for d in range(3):
            i = np.arange(begin[d], end[d])
            if d >= nd:
                per_dim.append([(np.zeros_like(i) + _ref(lc, d), np.ones(i.shape), np.ones(i.shape, dtype=bool))])
                continue
            odd = (i & 1) == 1
            first = (np.where(odd, (i + 1) // 2, i // 2) + _ref(lc, d), np.where(odd, 0.5, 1.0), np.ones(i.shape, dtype=bool))
            second = (np.where(odd, (i - 1) // 2, i // 2) + _ref(lc, d), np.where(odd, 0.5, 0.0), odd)
            per_dim.append([first, second])
        acc = None
        for (c0, w0, m0) in per_dim[0]:
            for (c1, w1, m1) in per_dim[1]:
                for (c2, w2, m2) in per_dim[2]:
                    wgt = (w0[None, None, :] * w1[None, :, None]) * w2[:, None, None]
                    on = m0[None, None, :] & m1[None, :, None] & m2[:, None, None]
                    tv = wgt[..., None] * Cc[np.ix_(c2, c1, c0)]
                    if acc is None:
                        acc = tv.copy()      # the first term exists at every point
                    else:
                        acc = np.where(on[..., None], acc + tv, acc)
        Fv = cview(lfine, uf)[_sl(lfine, begin, end)]
        Fv[...] = Fv + acc

    # -- examg_cshift_div, examg_cfrom_parts ------------------------------------------------------------------------------------------------
    def cshift_div(self, l, x, off, c, begin, end):
        X = cview(l, x)
        S = X[_sl(l, begin, end, off)].copy()
        rr, ri = cdiv(S[..., 0], S[..., 1], c)
        D = X[_sl(l, begin, end)]
        D[..., 0] = rr
        D[..., 1] = ri

    def cfrom_parts(self, l, dst, lre, re, lim, im, begin, end):
        D = cview(l, dst)[_sl(l, begin, end)]
        D[..., 0] = rview(lre, re)[_sl(lre, begin, end)] if re is not None else 0.0
        D[..., 1] = rview(lim, im)[_sl(lim, begin, end)] if im is not None else 0.0


def fsum_bound(terms):
    """(math.fsum of the terms, fsum of their magnitudes): the reference and the scale of the error bound of a sum in any order."""
    return math.fsum(terms.tolist()), math.fsum(np.abs(terms).tolist())


def interp_ops(dot_order="pairwise"):
    """The kernel layer of the interpreter's CPU tests: the real entry points of the C oracle (tests/oracle_ops.py, CPU torch tensors) and
    the complex ones of this restatement on the same tensors."""
    from tests.oracle_ops import OracleOps

    class InterpOps(OracleOps):
        name = "oracle+complex-numpy"

        def new_complex_array(self, npoints):
            return self.new_array(2 * int(npoints))

        def new_complex_scalar(self):
            return self.new_array(2)

        def complex_value(self, t):
            v = _np(t)
            return complex(float(v[0]), float(v[1]))

    for name in ("cstencil_op", "clincomb", "cdot", "cdot_terms", "crestrict", "cprolong_add", "cshift_div", "cfrom_parts"):
        setattr(InterpOps, name, ComplexOps.__dict__[name])
    ops = InterpOps()
    ops.dot_order = dot_order
    return ops
