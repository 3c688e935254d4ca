"""Asymmetric constant stencils, exact test data and an exact reference of the constant-stencil operations (test helper).

Every stencil the reference programs declare is symmetric: the -x and +x coefficients are equal, and so are the y and z pairs.  A
kernel that applies a coefficient to the mirror neighbour gives the same bits on such a stencil.  The stencils here have pairwise
distinct coefficients (no two of them equal in magnitude for the 5- and 7-point stars) and come in several entry orders, the
centre first or not.

Exact data: small integer fields, coefficients that are multiples of 1/4 and a dyadic smoother weight.  Every product and every
partial sum is then a dyadic rational with few bits, exactly representable in fp64: any correct implementation returns exactly the
mathematical value, in any summation order, with or without FMA.  ExactOps computes that value in int64 fixed point with FRAC
fractional bits, straight from the ExaSlang definitions (numpy slicing, no call into the oracle or the library), and asserts on every
value it produces that the value -- and every partial sum of the terms it was summed from, in any order -- is exactly representable.

The compositions at the end (jacobi2, rbgs_sweep, ...) are the one-pass entry points written as their loops, on any kernel layer
that has stencil_op / restrict / prolong_add / axpby: on ExactOps they are the exact reference, on the oracle the bitwise one.
Outside the box they write nothing, and they never modify their inputs.

Stencil fields (variable coefficients, include/examg.h: cfield[k * size(clayout) + linear(clayout, i)]): ExactOps takes them in the
planes layout with per-point dyadic coefficients, the diagonal entry anywhere in the entry list and either form of the smoother
weight -- on exact data the diagonal is a power of two, so `(1.0 / c) * w` and `w / c` are the same exact value.  FoldOps is a
second reference for data that is NOT exact: a float64 numpy restatement of the statement order the header prescribes (entries folded
left to right, `rhs - acc`, `u + ww * (..)` with ww in either form).  numpy's elementwise operations are IEEE and uncontracted, so
any correct implementation returns the same bits; it separates the two weight forms, the entry order and the diagonal index, which
exact data cannot.  The builders at the end make stencil fields in several entry orders with random or exact coefficients that
fill the whole allocation of their own layout (ghost, duplicate and pad points included): a read through the wrong layout gets a
wrong value, not a zero.
"""
from fractions import Fraction

import numpy as np

from exastencils_amd.field import Stencil

APPLY, RESIDUAL, SMOOTH = 0, 1, 2

# -- stencils ------------------------------------------------------------------------------------------------------------------------
_AX = {"c": (0, 0, 0), "-x": (-1, 0, 0), "+x": (1, 0, 0), "-y": (0, -1, 0), "+y": (0, 1, 0), "-z": (0, 0, -1), "+z": (0, 0, 1)}
# entry orders: the two of the reference programs and two permutations with the centre elsewhere
ORDERS7 = {
    "mp": ["c", "-x", "+x", "-y", "+y", "-z", "+z"],
    "pm": ["c", "+x", "-x", "+y", "-y", "+z", "-z"],
    "perm_a": ["+y", "-z", "c", "-x", "+z", "+x", "-y"],
    "perm_b": ["-z", "+x", "-y", "+z", "+y", "c", "-x"],
}
ORDERS5 = {
    "mp": ["c", "-x", "+x", "-y", "+y"],
    "pm": ["c", "+x", "-x", "+y", "-y"],
    "perm_a": ["+y", "c", "-x", "-y", "+x"],
    "perm_b": ["-x", "+y", "+x", "c", "-y"],
}
OFFSETS27 = [(a, b, c) for c in (-1, 0, 1) for b in (-1, 0, 1) for a in (-1, 0, 1)]
ORDERS27 = {
    "centre_first": [(0, 0, 0)] + [o for o in OFFSETS27 if o != (0, 0, 0)],
    "perm": [OFFSETS27[i] for i in np.random.default_rng(2727).permutation(27)],
}


def _star(coef_of, order, names):
    return Stencil([_AX[n] for n in names[order]], [float(coef_of[n]) for n in names[order]])


AXES, star = _AX, _star      # for the other case modules: the offset of an entry name; a star stencil from {name: coefficient}


def _distinct_magnitudes(cs):
    m = [abs(c) for c in cs]
    assert len(set(m)) == len(m), "stencil coefficients must be pairwise distinct in magnitude: %r" % (cs,)


def convdiff7(shape, order="mp"):
    """Anisotropic diffusion + a centred convection term (cell Peclet numbers 0.35, -0.2, 0.15) + a small reaction term on the grid
    of `shape` cells: seven pairwise distinct coefficients, the diagonal dominant.  Not dyadic: for the bitwise comparisons."""
    k, pe = (1.0, 0.6, 1.4), (0.35, -0.2, 0.15)
    c = {}
    diag = 0.0
    for d, ax in enumerate("xyz"):
        s = k[d] * float(shape[d]) ** 2
        c["-" + ax], c["+" + ax] = -s * (1.0 + pe[d]), -s * (1.0 - pe[d])
        diag = diag + 2.0 * s
    c["c"] = 1.05 * diag
    _distinct_magnitudes(list(c.values()))
    return _star(c, order, ORDERS7)


def convdiff5(shape, order="mp"):
    """The 2-D analogue of convdiff7."""
    k, pe = (1.0, 0.7), (0.3, -0.25)
    c = {}
    diag = 0.0
    for d, ax in enumerate("xy"):
        s = k[d] * float(shape[d]) ** 2
        c["-" + ax], c["+" + ax] = -s * (1.0 + pe[d]), -s * (1.0 - pe[d])
        diag = diag + 2.0 * s
    c["c"] = 1.05 * diag
    _distinct_magnitudes(list(c.values()))
    return _star(c, order, ORDERS5)


def random27(order="centre_first"):
    """27 distinct coefficients (not dyadic), the diagonal dominant."""
    rng = np.random.default_rng(27)
    off = {o: -float(v) for o, v in zip([o for o in OFFSETS27 if o != (0, 0, 0)], rng.uniform(0.1, 1.3, 26))}
    off[(0, 0, 0)] = 1.1 * sum(-v for v in off.values())
    offs = ORDERS27[order]
    st = Stencil(offs, [off[o] for o in offs])
    assert len(set(st.coefs)) == 27
    return st


# exact data: multiples of 1/4 with |c| <= 8, pairwise distinct in magnitude, the diagonal dominant
EXACT7 = {"c": 7.5, "-x": -2.25, "+x": 0.5, "-y": -1.25, "+y": -0.75, "-z": -1.5, "+z": -0.25}
EXACT5 = {"c": 6.0, "-x": -1.75, "+x": 0.5, "-y": -1.25, "+y": -0.25}
# integer coefficients (residual_norm2: integer residuals, their squares summed exactly)
INT7 = {"c": 8.0, "-x": -3.0, "+x": 1.0, "-y": -2.0, "+y": -4.0, "-z": 5.0, "+z": -6.0}
EXACT_W = 1.0 / 16.0         # a dyadic smoother weight, not omega / diag for any omega of the programs


def exact7(order="mp", coefs=EXACT7):
    _distinct_magnitudes(list(coefs.values()))
    return _star(coefs, order, ORDERS7)


def exact5(order="mp"):
    _distinct_magnitudes(list(EXACT5.values()))
    return _star(EXACT5, order, ORDERS5)


def exact27(order="centre_first"):
    """27 distinct multiples of 1/4 (the off-diagonal ones +-1/4 .. +-13/4), centre 8."""
    vals = [0.25 * s * m for m in range(1, 14) for s in (1, -1)]
    perm = np.random.default_rng(2028).permutation(26)
    others = [o for o in OFFSETS27 if o != (0, 0, 0)]
    off = {o: vals[int(p)] for o, p in zip(others, perm)}
    off[(0, 0, 0)] = 8.0
    offs = ORDERS27[order]
    st = Stencil(offs, [off[o] for o in offs])
    assert len(set(st.coefs)) == 27
    return st


def is_star(st):
    return all(sum(1 for v in o if v != 0) <= 1 and all(abs(v) <= 1 for v in o) for o in st.offsets)


def free_weight(st):
    """A smoother weight for the bitwise comparisons that is not 0.8 / diag (what every program passes)."""
    return 0.713 / st.diag


def int_field(size, seed, lo=-16, hi=16):
    """Small integers from a seeded generator, as float64 (the whole allocation: ghost, duplicate and pad points included)."""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=int(size)).astype(np.float64)


# -- exact reference ----------------------------------------------------------------------------------------------------------------
FRAC = 32                    # fractional bits of the fixed-point values
_LIM = 1 << 53               # |value| * 2^FRAC below this: a multiple of 2^-FRAC below 2^(53 - FRAC) in magnitude is exact in fp64


class _Lay:
    """Regions of a layout (a LayoutC or a FieldLayout), the index arithmetic of the ExaSlang field layout."""

    def __init__(self, l):
        if hasattr(l, "c_struct"):
            l = l.c_struct()
        if int(getattr(l, "transform", 0)) != 0:
            raise ValueError("the exact reference works on untransformed layouts")
        self.nd = int(l.nd)
        self.ref = [int(l.pad_l[d]) + int(l.ghost_l[d]) for d in range(3)]
        self.tot = [sum(int(getattr(l, k)[d]) for k in ("pad_l", "ghost_l", "dup_l", "inner", "dup_r", "ghost_r", "pad_r"))
                    for d in range(3)]

    @property
    def shape(self):
        return (self.tot[2], self.tot[1], self.tot[0])

    def box(self, b, e, off=(0, 0, 0), step=1):
        """numpy index of the iterator box [b, e) shifted by `off` (step 2: the points 2I + off of the coarse box I in [b, e))."""
        sl = []
        for d in (2, 1, 0):
            lo = step * b[d] + off[d] + self.ref[d]
            hi = step * (e[d] - 1) + off[d] + self.ref[d] + 1
            if lo < 0 or hi > self.tot[d]:
                raise IndexError("box %r..%r + %r leaves the allocation in dim %d" % (b, e, off, d))
            sl.append(slice(lo, hi, step))
        return tuple(sl)


Lay = _Lay                   # for the other case modules


def _dyadic(c):
    f = Fraction(c)            # every float is a dyadic rational: m / 2^k
    return int(f.numerator), f.denominator.bit_length() - 1


def _check(v):
    if v.size and int(np.abs(v).max()) >= _LIM:
        raise AssertionError("exact reference: a value leaves the exactly representable range (%.3g)" % (float(np.abs(v).max()) / 2.0 ** FRAC))
    return v


def _mul(v, c):
    m, k = _dyadic(c)
    if k > FRAC:
        raise ValueError("exact reference: coefficient %r needs more fractional bits than %d" % (c, FRAC))
    if v.size and int(np.abs(v).max()) * abs(m) >= _LIM:
        raise AssertionError("exact reference: product leaves the exactly representable range")
    p = v * m
    if k and np.any(p & ((1 << k) - 1)):
        raise AssertionError("exact reference: %d fractional bits are not enough" % FRAC)
    return p >> k


def _sum(terms):
    """The exact sum; every partial sum in any order is bounded by the sum of the magnitudes, which must stay representable."""
    _check(sum(np.abs(t) for t in terms))
    return sum(terms[1:], terms[0].copy())


CFRAC = 8                    # per-point coefficients: multiples of 2^-CFRAC


def _mulv(v, c):
    """v * c point by point, both in fixed point; c must be a multiple of 2^-CFRAC."""
    sh = FRAC - CFRAC
    if np.any(c & ((1 << sh) - 1)):
        raise ValueError("exact reference: a per-point coefficient needs more than %d fractional bits" % CFRAC)
    cq = c >> sh
    if v.size and int(np.abs(v).max()) * int(np.abs(cq).max()) >= (_LIM << CFRAC):
        raise AssertionError("exact reference: product leaves the exactly representable range")
    p = v * cq
    if np.any(p & ((1 << CFRAC) - 1)):
        raise AssertionError("exact reference: %d fractional bits are not enough" % FRAC)
    return p >> CFRAC


def _divp2(v, c):
    """v / c point by point for c a positive power of two (fixed point): exact, or an error."""
    if np.any(c <= 0) or np.any(c & (c - 1)):
        raise ValueError("exact reference: the diagonal of a stencil field must be a positive power of two (1.0 / c exact)")
    e = np.round(np.log2(c.astype(np.float64))).astype(np.int64) - FRAC          # c = 2^e
    if np.any(e < 0):
        raise ValueError("exact reference: diagonal below 1")
    if np.any(v & ((np.int64(1) << e) - 1)):
        raise AssertionError("exact reference: %d fractional bits are not enough" % FRAC)
    return v >> e


class ExactOps:
    """Kernel layer of exact values: arrays are int64 fixed point (value * 2^FRAC), layouts LayoutC or FieldLayout, stencils with
    dyadic coefficients.  Same method signatures as the HIP and oracle kernel layers, for the calls the tests make."""

    name = "exact"

    def new_array(self, n):
        return np.zeros(int(n), dtype=np.int64)

    def from_host(self, a):
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        v = np.ldexp(a, FRAC)
        if not np.array_equal(v, np.round(v)):
            raise ValueError("exact data needs multiples of 2^-%d" % FRAC)
        return _check(v.astype(np.int64))

    def to_host(self, t):
        return np.ldexp(t.astype(np.float64), -FRAC)

    def clone(self, t):
        return t.copy()

    def synchronize(self):
        pass

    @staticmethod
    def _v(t, l):
        return t.reshape(_Lay(l).shape)

    def stencil_op(self, mode, lu, u, lf, rhs, ld, dst, st, w, colour, begin, end):
        Lu, Ld = _Lay(lu), _Lay(ld)
        U, D = self._v(u, lu), self._v(dst, ld)
        if st.cfield is not None:
            # include/examg.h: entry k of point i is cfield[k * size(clayout) + linear(clayout, i)]
            if int(getattr(st, "ctransform", 0)) != 0:
                raise ValueError("the exact reference reads stencil fields in the planes layout (a transformed array holds the same values)")
            if int(getattr(st, "wform", 0)) not in (0, 1):
                raise ValueError("unknown weight form %r" % (st.wform,))
            Lc = _Lay(st.clayout)
            CF = st.cfield.reshape((len(st.offsets),) + Lc.shape)
            cb = Lc.box(begin, end)
            acc = _sum([_mulv(U[Lu.box(begin, end, o)], CF[k][cb]) for k, o in enumerate(st.offsets)])
        else:
            acc = _sum([_mul(U[Lu.box(begin, end, o)], c) for o, c in zip(st.offsets, st.coefs)])
        if mode == APPLY:
            out = acc
        else:
            F = self._v(rhs, lf)[_Lay(lf).box(begin, end)]
            out = _check(F - acc)
            if mode == SMOOTH:
                out = _mul(out, w)
                if st.cfield is not None:
                    # ww = (1.0 / c_diag) * w or w / c_diag, c_diag = entry st.diag_index of the point: a power of two here, so
                    # 1.0 / c_diag, both forms of ww and ww * (rhs - acc) are exact and equal w * (rhs - acc) / c_diag
                    out = _divp2(out, CF[st.diag_index][cb])
                out = _check(U[Lu.box(begin, end)] + _check(out))
        db = Ld.box(begin, end)
        if colour < 0:
            D[db] = out
            return
        if u is dst and not is_star(st):
            raise ValueError("an in-place colour loop of a stencil that reaches its own colour depends on the loop order")
        i2, i1, i0 = np.meshgrid(*[np.arange(begin[d], end[d]) for d in (2, 1, 0)], indexing="ij")
        D[db] = np.where((i0 + i1 + i2) % 2 == colour, out, D[db])

    def restrict(self, lfine, rf, lc, fc, scale, begin, end):
        Lf, Lc = _Lay(lfine), _Lay(lc)
        R = self._v(rf, lfine)
        w1 = {-1: 0.25, 0: 0.5, 1: 0.25}
        nd = Lf.nd
        offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in ((-1, 0, 1) if nd == 3 else (0,))]
        terms = []
        for o in offs:
            wgt = w1[o[0]] * w1[o[1]] * (w1[o[2]] if nd == 3 else 1.0)
            terms.append(_mul(R[Lf.box(begin, end, (o[0], o[1], o[2] if nd == 3 else 0), step=2)], scale * wgt))
        self._v(fc, lc)[Lc.box(begin, end)] = _sum(terms)

    def prolong_add(self, lc, uc, lfine, uf, begin, end):
        Lc, Lf = _Lay(lc), _Lay(lfine)
        Uc, Uf = self._v(uc, lc), self._v(uf, lfine)
        lo, hi = [], []
        for d in range(3):
            i = np.arange(begin[d], end[d])
            if d < Lf.nd:
                lo.append(i // 2 + Lc.ref[d])
                hi.append((i + 1) // 2 + Lc.ref[d])
            else:
                lo.append(i + Lc.ref[d])
                hi.append(i + Lc.ref[d])
        for d in range(3):
            if lo[d].size and (lo[d].min() < 0 or hi[d].max() >= Lc.tot[d]):
                raise IndexError("coarse footprint leaves the allocation")
        # per dimension 1/2 (c[lo] + c[hi]): weight 1 on an even index (lo == hi), 1/2 + 1/2 on an odd one
        terms = []
        for sx in (lo[0], hi[0]):
            for sy in (lo[1], hi[1]):
                for sz in (lo[2], hi[2]):
                    terms.append(_mul(Uc[np.ix_(sz, sy, sx)], 0.125))
        fb = Lf.box(begin, end)
        Uf[fb] = _check(Uf[fb] + _sum(terms))

    def axpby(self, lx, x, ly, y, a, b, begin, end):
        Lx, Ly = _Lay(lx), _Lay(ly)
        X, Y = self._v(x, lx), self._v(y, ly)
        yb = Ly.box(begin, end)
        Y[yb] = _sum([_mul(X[Lx.box(begin, end)], a), _mul(Y[yb], b)])

    def residual_norm2(self, lu, u, lf, rhs, st, begin, end, lr=None, res=None, out=None):
        """sum over the box of (rhs - A u)^2 as a float: the residuals must be integers here (their squares are summed exactly)."""
        r = self.new_array(u.size)
        self.stencil_op(RESIDUAL, lu, u, lf, rhs, lu, r, st, 0.0, -1, begin, end)
        v = r.reshape(_Lay(lu).shape)[_Lay(lu).box(begin, end)]
        if np.any(v & ((1 << FRAC) - 1)):
            raise ValueError("residual_norm2 of the exact reference needs integer residuals")
        iv = v >> FRAC
        s = int(np.sum(iv * iv))
        assert s < _LIM
        return float(s)


# -- the one-pass entry points as their loops (any kernel layer with the loops above; box-only writes, inputs untouched) -------
def _clone(P, t):
    return P.clone(t) if hasattr(P, "clone") else t.clone()


def _zeros_like(P, t):
    return P.new_array(t.numel() if hasattr(t, "numel") else t.size)


def jacobi2(P, lu, u_in, u_out, lf, rhs, st, w, b, e):
    t = _clone(P, u_in)
    P.stencil_op(SMOOTH, lu, u_in, lf, rhs, lu, t, st, w, -1, b, e)
    P.stencil_op(SMOOTH, lu, t, lf, rhs, lu, u_out, st, w, -1, b, e)


def jacobi3(P, lu, u_in, u_out, lf, rhs, st, w, b, e):
    t1, t2 = _clone(P, u_in), _clone(P, u_in)
    P.stencil_op(SMOOTH, lu, u_in, lf, rhs, lu, t1, st, w, -1, b, e)
    P.stencil_op(SMOOTH, lu, t1, lf, rhs, lu, t2, st, w, -1, b, e)
    P.stencil_op(SMOOTH, lu, t2, lf, rhs, lu, u_out, st, w, -1, b, e)


def jacobi2_boxes(P, lu, u_in, u_out, lf, rhs, st, w, b1, e1, b2, e2):
    t = _clone(P, u_in)
    P.stencil_op(SMOOTH, lu, u_in, lf, rhs, lu, t, st, w, -1, b1, e1)
    P.stencil_op(SMOOTH, lu, t, lf, rhs, lu, u_out, st, w, -1, b2, e2)


def jacobi2_prolong(P, lu, u_in, u_out, lf, rhs, st, w, b, e, lc, uc):
    work = _clone(P, u_in)
    P.prolong_add(lc, uc, lu, work, b, e)
    jacobi2(P, lu, work, u_out, lf, rhs, st, w, b, e)


def colours(P, lu, u_in, u_out, lf, rhs, st, w, cols, b, e, correction=None):
    """The colour loops `cols` in place on a copy of u_in (optionally after `u += P uc`); u_out receives the box."""
    work = _clone(P, u_in)
    if correction is not None:
        P.prolong_add(correction[0], correction[1], lu, work, b, e)
    for c in cols:
        P.stencil_op(SMOOTH, lu, work, lf, rhs, lu, work, st, w, c, b, e)
    P.axpby(lu, work, lu, u_out, 1.0, 0.0, b, e)


def rbgs_sweep(P, lu, u_in, u_out, lf, rhs, st, w, first, b, e):
    colours(P, lu, u_in, u_out, lf, rhs, st, w, (first, 1 - first), b, e)


def rbgs_sweep_zero(P, lu, u_out, lf, rhs, st, w, first, b, e):
    colours(P, lu, _zeros_like(P, u_out), u_out, lf, rhs, st, w, (first, 1 - first), b, e)


def rbgs_sweep_prolong(P, lu, u_in, u_out, lf, rhs, st, w, first, b, e, lc, uc):
    colours(P, lu, u_in, u_out, lf, rhs, st, w, (first, 1 - first), b, e, (lc, uc))


def rbgs_colours3(P, lu, u_in, u_out, lf, rhs, st, w, first, b, e):
    colours(P, lu, u_in, u_out, lf, rhs, st, w, (first, 1 - first, first), b, e)


def rbgs_sweep_boxes(P, lu, u_in, u_out, lf, rhs, st, w, first, b1, e1, b2, e2):
    t = _clone(P, u_in)
    P.stencil_op(SMOOTH, lu, t, lf, rhs, lu, t, st, w, first, b1, e1)
    P.axpby(lu, t, lu, u_out, 1.0, 0.0, b2, e2)
    P.stencil_op(SMOOTH, lu, t, lf, rhs, lu, u_out, st, w, 1 - first, b2, e2)


def jacobi_residual(P, lu, u_in, u_out, lf, rhs, lr, res, st, w, b, e):
    P.stencil_op(SMOOTH, lu, u_in, lf, rhs, lu, u_out, st, w, -1, b, e)
    P.stencil_op(RESIDUAL, lu, u_out, lf, rhs, lr, res, st, 0.0, -1, b, e)


def residual_restrict(P, lu, u, lf, rhs, st, lc, fc, scale, fb, fe, cb, ce):
    r = _zeros_like(P, u)
    P.stencil_op(RESIDUAL, lu, u, lf, rhs, lu, r, st, 0.0, -1, fb, fe)
    P.restrict(lu, r, lc, fc, scale, cb, ce)


def shell_mask(l, b, e, reach=1):
    """Flat boolean mask of the points within `reach` of the box [b, e) but outside it (the dimensions of the layout only)."""
    L = _Lay(l)
    m = np.zeros(L.shape, dtype=bool)
    bb = [b[d] - (reach if d < L.nd else 0) for d in range(3)]
    ee = [e[d] + (reach if d < L.nd else 0) for d in range(3)]
    m[L.box(bb, ee)] = True
    m[L.box(b, e)] = False
    return m.reshape(-1)


def box_mask(l, b, e):
    L = _Lay(l)
    m = np.zeros(L.shape, dtype=bool)
    m[L.box(b, e)] = True
    return m.reshape(-1)


# -- a float64 restatement of the statement order (data that is not exact) -----------------------------------------------------------
class FoldOps:
    """include/examg.h, statement by statement in float64 numpy: acc = c_0 * u[i + o_0]; acc = acc + c_k * u[i + o_k] for k = 1 .. in
    entry order; EXAMG_RESIDUAL: rhs - acc; EXAMG_SMOOTH: u + ww * (rhs - acc) with ww = w (constant stencils), (1.0 / c_diag) * w
    (EXAMG_WEIGHT_INV_TIMES) or w / c_diag (EXAMG_WEIGHT_DIVIDE), c_diag = cfield[diag * size(clayout) + linear(clayout, i)].  Every
    argument is indexed through its own layout.  No call into the oracle or the library."""

    name = "fold"

    def new_array(self, n):
        return np.zeros(int(n), dtype=np.float64)

    def from_host(self, a):
        return np.array(a, dtype=np.float64, copy=True).reshape(-1)

    def to_host(self, t):
        return t

    def clone(self, t):
        return t.copy()

    def synchronize(self):
        pass

    def stencil_op(self, mode, lu, u, lf, rhs, ld, dst, st, w, colour, begin, end):
        Lu, Ld = _Lay(lu), _Lay(ld)
        U, D = u.reshape(Lu.shape), dst.reshape(Ld.shape)
        cf = None
        if st.cfield is not None:
            if int(getattr(st, "ctransform", 0)) != 0:
                raise ValueError("planes layout only")
            Lc = _Lay(st.clayout)
            cb = Lc.box(begin, end)
            CF = st.cfield.reshape((len(st.offsets),) + Lc.shape)
            cf = [CF[k][cb] for k in range(len(st.offsets))]
        acc = None
        for k, o in enumerate(st.offsets):
            c = cf[k] if cf is not None else np.float64(st.coefs[k])
            t = c * U[Lu.box(begin, end, o)]
            acc = t if acc is None else acc + t
        if mode == APPLY:
            out = acc
        else:
            r = rhs.reshape(_Lay(lf).shape)[_Lay(lf).box(begin, end)] - acc
            if mode == RESIDUAL:
                out = r
            else:
                w = np.float64(w)
                if cf is None:
                    ww = w
                else:
                    dg = cf[st.diag_index]
                    ww = (w / dg) if int(getattr(st, "wform", 0)) == 1 else ((np.float64(1.0) / dg) * w)
                out = U[Lu.box(begin, end)] + ww * r
        db = Ld.box(begin, end)
        if colour < 0:
            D[db] = out
            return
        if u is dst and not is_star(st):
            raise ValueError("an in-place colour loop of a stencil that reaches its own colour depends on the loop order")
        i2, i1, i0 = np.meshgrid(*[np.arange(begin[d], end[d]) for d in (2, 1, 0)], indexing="ij")
        D[db] = np.where((i0 + i1 + i2) % 2 == colour, out, D[db])


# -- stencil fields --------------------------------------------------------------------------------------------------------------------
def field_offsets(kind):
    """Entry lists of the stencil fields under test.  vc7 / vc5: the order Testing/SISC/3D_VarCoeff.exa4 declares (centre, +x, -x, +y,
    -y, ..: field.stencil_field_offsets); h27: the order of examg_init_helmholtz27 (centre, then dz slowest and dx fastest); the
    *_perm* lists are permutations with the centre elsewhere."""
    from exastencils_amd.field import helmholtz27_offsets, stencil_field_offsets

    offs = {"vc7": lambda: stencil_field_offsets(3), "vc7_perm_a": lambda: [_AX[n] for n in ORDERS7["perm_a"]],
            "vc7_perm_b": lambda: [_AX[n] for n in ORDERS7["perm_b"]], "vc5": lambda: stencil_field_offsets(2),
            "vc5_perm": lambda: [_AX[n] for n in ORDERS5["perm_b"]], "h27": helmholtz27_offsets,
            "h27_perm": lambda: list(ORDERS27["perm"])}[kind]()
    offs = [tuple(o) for o in offs]
    assert (offs[0] != (0, 0, 0)) == ("perm" in kind) and len(set(offs)) == len(offs)
    return offs


EXACT_DIAGS = (4.0, 8.0, 16.0)


def coefficient_array(offsets, clayout, data, seed, unit=0.25):
    """Host array (entries x size(clayout), flat) of a stencil field's coefficients over the WHOLE allocation of `clayout`.
    data 'random': U(-1, 1), the diagonal entry U(2, 4) (mixed signs off the diagonal, the smoother weight finite);
    data 'exact': off the diagonal k * unit with k in -12 .. 12 without 0, drawn per point and entry; the diagonal per point from
    {4, 8, 16}: 1.0 / c, (1.0 / c) * w and w / c are exact for a dyadic w."""
    K, n = len(offsets), int(clayout.size)
    d = offsets.index((0, 0, 0))
    rng = np.random.default_rng(seed)
    if data == "exact":
        k = rng.integers(1, 13, size=(K, n)) * rng.choice(np.array([-1, 1]), size=(K, n))
        a = k.astype(np.float64) * unit
        a[d] = rng.choice(np.array(EXACT_DIAGS), size=n)
    else:
        a = rng.uniform(-1.0, 1.0, size=(K, n))
        a[d] += 3.0
    return a.reshape(-1)


def stencil_field(ops, offsets, clayout, data, seed, wform=0, unit=0.25):
    """A Stencil with a coefficient field in the planes layout, its array on kernel layer `ops` (same values on every layer)."""
    return Stencil(list(offsets), [], ops.from_host(coefficient_array(offsets, clayout, data, seed, unit)), clayout, 0, wform)


def data_field(ops, size, data, seed):
    """A field array over the whole allocation: small integers (exact) or U(-1, 1) (random), the same values on every layer."""
    if data == "exact":
        return ops.from_host(int_field(size, seed))
    return ops.from_host(np.random.default_rng(seed).uniform(-1.0, 1.0, int(size)))


# -- stencil-field initialisation, restated from include/examg.h ---------------------------------------------------------------------
def asym_coefficient(x, y, z):
    """1 + x + 2 y^2 + 4 z as the tree ((1.0 + x) + ((2.0 * y) * y)) + (4.0 * z): +, * and constants only (no libm), different under
    every mirroring and every permutation of the axes."""
    return ((1.0 + x) + ((2.0 * y) * y)) + (4.0 * z)


ASYM_PROGRAM = [("const", 1.0), ("x", None), ("+", None), ("const", 2.0), ("y", None), ("*", None), ("y", None), ("*", None), ("+", None),
                ("const", 4.0), ("z", None), ("*", None), ("+", None)]


def _positions(geom, begin, end):
    i2, i1, i0 = np.meshgrid(*[np.arange(begin[d], end[d]).astype(np.float64) for d in (2, 1, 0)], indexing="ij")
    return (i0 * geom.h[0] + geom.pos_begin[0], i1 * geom.h[1] + geom.pos_begin[1], i2 * geom.h[2] + geom.pos_begin[2])


def init_varcoeff7_ref(lc, cf, geom, a, begin, end):
    """examg_init_varcoeff7 (Testing/SISC/3D_VarCoeff.exa4:206-217) on the box of the host array `cf` (entries x size(lc)):
    -div(a grad u), a evaluated half a mesh width to either side of the node; entry order centre, +x, -x, +y, -y[, +z, -z]."""
    L = _Lay(lc)
    nd = L.nd
    CF = cf.reshape((2 * nd + 1,) + L.shape)
    x, y, z = _positions(geom, begin, end)
    h = [np.float64(geom.h[d]) for d in range(3)]
    p = [x, y, z]
    ap, am = [], []
    for d in range(nd):
        q, r = list(p), list(p)
        q[d] = p[d] + (0.5 * h[d])
        r[d] = p[d] - (0.5 * h[d])
        ap.append(a(*q))
        am.append(a(*r))
    b = L.box(begin, end)
    diag = None
    for d in range(nd):
        t = (ap[d] + am[d]) / (h[d] * h[d])
        diag = t if diag is None else diag + t
        CF[1 + 2 * d][b] = (-1.0 * ap[d]) / (h[d] * h[d])
        CF[2 + 2 * d][b] = (-1.0 * am[d]) / (h[d] * h[d])
    CF[0][b] = diag


def init_helmholtz27_ref(lc, cf, geom, a, ksq, begin, end):
    """examg_init_helmholtz27 on the box of the host array `cf` (27 x size(lc)): trilinear elements, a constant per element (its
    value at the element centre), lumped mass, scaled by 1 / h^3, minus ksq on the diagonal.  Entry (dx, dy, dz): the sum of a over
    the elements that hold both nodes (x outermost, z innermost), times 1/3 (centre), 0 (across an edge) or -1/12 (across a face or
    body diagonal), divided by h * h.  Entry order: centre first, then dz slowest and dx fastest."""
    L = _Lay(lc)
    CF = cf.reshape((27,) + L.shape)
    x, y, z = _positions(geom, begin, end)
    h = np.float64(geom.h[0])
    ae = {}
    for sx in (0, 1):
        for sy in (0, 1):
            for sz in (0, 1):
                ae[(sx, sy, sz)] = a(x + (0.5 if sx else -0.5) * h, y + (0.5 if sy else -0.5) * h, z + (0.5 if sz else -0.5) * h)
    b = L.box(begin, end)
    ent = 1
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nnz = (dx != 0) + (dy != 0) + (dz != 0)
                s = None
                for sx in (0, 1):
                    for sy in (0, 1):
                        for sz in (0, 1):
                            if (dx == 0 or (dx > 0) == bool(sx)) and (dy == 0 or (dy > 0) == bool(sy)) and (dz == 0 or (dz > 0) == bool(sz)):
                                s = ae[(sx, sy, sz)] if s is None else s + ae[(sx, sy, sz)]
                kf = (1.0 / 3.0) if nnz == 0 else (0.0 if nnz == 1 else (-1.0 / 12.0))
                c = (s * kf) / (h * h)
                if nnz == 0:
                    CF[0][b] = c - ksq
                else:
                    CF[ent][b] = c
                    ent += 1


# -- cell transfers, exact (include/examg.h: examg_restrict_cell / examg_prolong_add_cell) -------------------------------------------
def _exact_restrict_cell(self, lfine, rf, lc, fc, scale, begin, end):
    """fc(I) = scale * 2^-d * (sum of the 2^d children rf(2I + o), o in {0, 1}^d), straight from the definition."""
    if any(end[d] <= begin[d] for d in range(3)):
        return
    Lf, Lc = _Lay(lfine), _Lay(lc)
    nd = Lf.nd
    if Lc.nd != nd or (nd == 2 and (begin[2] != 0 or end[2] != 1)):
        raise ValueError("cell restriction: layouts of one dimensionality, a 2-D box with [0, 1) in dim 2")
    R = self._v(rf, lfine)
    children = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in ((0, 1) if nd == 3 else (0,))]
    terms = [_mul(R[Lf.box(begin, end, o, step=2)], scale * 0.5 ** nd) for o in children]
    self._v(fc, lc)[Lc.box(begin, end)] = _sum(terms)


def _exact_prolong_add_cell(self, lc, uc, lfine, uf, begin, end):
    """uf(i) += uc(floor(i / 2)); numpy's // floors negative indices too."""
    if any(end[d] <= begin[d] for d in range(3)):
        return
    Lc, Lf = _Lay(lc), _Lay(lfine)
    nd = Lf.nd
    if Lc.nd != nd or (nd == 2 and (begin[2] != 0 or end[2] != 1)):
        raise ValueError("cell prolongation: layouts of one dimensionality, a 2-D box with [0, 1) in dim 2")
    idx = []
    for d in (2, 1, 0):
        i = np.arange(begin[d], end[d])
        p = (i // 2 if d < nd else i) + Lc.ref[d]
        if p.min() < 0 or p.max() >= Lc.tot[d]:
            raise IndexError("parent cells leave the coarse allocation in dim %d" % d)
        idx.append(p)
    fb = Lf.box(begin, end)
    Uf = self._v(uf, lfine)
    Uf[fb] = _check(Uf[fb] + self._v(uc, lc)[np.ix_(*idx)])


ExactOps.restrict_cell = _exact_restrict_cell
ExactOps.prolong_add_cell = _exact_prolong_add_cell


# -- transfer cases: geometry, linear fields, the adjoint identity --------------------------------------------------------------------
def restrict_geometry(nd, n, kind):
    """(fine cells, coarse cells, begin, end) of a node restriction whose coarse box has the extents n[0] x n[1] (x n[2]).
    inner: the inner points [1, cells); faces: a block with neighbours -- x over both duplicate planes (begin 0, end cells + 1), y
    over the lower one, z over the upper one, the fine footprint in the ghost layer there; inside_odd / inside_even: strictly inside
    the inner points, begin (3, 2, 1) / (2, 1, 3)."""
    lo = {"inner": (1, 1, 1), "faces": (0, 0, 1), "inside_odd": (3, 2, 1), "inside_even": (2, 1, 3)}[kind]
    top = {"inner": (0, 0, 0), "faces": (-1, 0, -1), "inside_odd": (1, 2, 1), "inside_even": (2, 1, 1)}[kind]      # cells - end
    b = [lo[d] if d < nd else 0 for d in range(3)]
    e = [b[d] + n[d] if d < nd else 1 for d in range(3)]
    cs = tuple(e[d] + top[d] if d < nd else 0 for d in range(3))
    return tuple(2 * c for c in cs), cs, b, e


def linear_field(l, coef, const=0, mul=1, add=0):
    """Host float64 array over the whole allocation of `l`: sum_d coef[d] * (mul * i_d + add) + const at iterator point i (integer
    arguments: exact).  Dimensions the layout does not have contribute nothing."""
    L = _Lay(l)
    ax = [np.arange(L.tot[d], dtype=np.int64) - L.ref[d] for d in range(3)]
    v = np.full(L.shape, int(const), dtype=np.int64)
    for d in range(L.nd):
        sh = [1, 1, 1]
        sh[2 - d] = -1
        v = v + (int(coef[d]) * (int(mul) * ax[d] + int(add))).reshape(sh)
    return v.astype(np.float64).reshape(-1)


LINEAR = (3, 7, 11)          # pairwise distinct and coprime: no two axes, and no axis and its mirror, give the same field


def box_values(l, a, b, e):
    return np.asarray(a).reshape(_Lay(l).shape)[_Lay(l).box(b, e)]


def supported_int_field(l, b, e, seed, lo=-9, hi=9):
    """Host array: small integers inside the box, zero elsewhere."""
    L = _Lay(l)
    a = np.zeros(L.shape)
    s = L.box(b, e)
    a[s] = np.random.default_rng(seed).integers(lo, hi + 1, size=a[s].shape)
    return a.reshape(-1)


def transfer_adjoint(ops, cell, lf, lc, cb, ce, fb, fe, scale, seed):
    """(sum(fc * w) * 2^d, scale * sum(r * P w)), both times a common power of two, in int64 for r supported in the fine box, w in the coarse box: equal,
    because the restriction is scale * 2^-d * P^T.  Both operators run on kernel layer `ops`."""
    nd = lf.nd
    r, w = supported_int_field(lf, fb, fe, seed), supported_int_field(lc, cb, ce, seed + 1)
    fc, pw = ops.from_host(np.zeros(lc.size)), ops.from_host(np.zeros(lf.size))
    if cell:
        ops.restrict_cell(lf.c_struct(), ops.from_host(r.copy()), lc.c_struct(), fc, scale, cb, ce)
        ops.prolong_add_cell(lc.c_struct(), ops.from_host(w.copy()), lf.c_struct(), pw, fb, fe)
    else:
        ops.restrict(lf.c_struct(), ops.from_host(r.copy()), lc.c_struct(), fc, scale, cb, ce)
        ops.prolong_add(lc.c_struct(), ops.from_host(w.copy()), lf.c_struct(), pw, fb, fe)
    ops.synchronize()
    # node: the full-weighting entries are multiples of 4^-d, the interpolation's of 2^-d; cell: 2^-d and 1
    kf, kp = (2 ** nd, 1) if cell else (4 ** nd, 2 ** nd)
    fck, pwk = np.asarray(ops.to_host(fc)) * kf, np.asarray(ops.to_host(pw)) * kp
    assert np.array_equal(fck, np.round(fck)) and np.array_equal(pwk, np.round(pwk)) and float(scale) == int(scale)
    lhs = int(np.sum(fck.astype(np.int64) * w.astype(np.int64))) * 2 ** nd * kp
    rhs = int(scale) * int(np.sum(r.astype(np.int64) * pwk.astype(np.int64))) * kf
    assert lhs != 0
    return lhs, rhs
