"""Lexicographic Gauss-Seidel on the reference kernel layers (test helper, no test functions).

GsMixin gives a kernel layer that has `stencil_op` (FoldOps, ExactOps of stencil_cases.py, OracleOps) the method `gs_sweep` of the
lexicographic sweep without touching those classes, built like MulticolourMixin: for t ascending the UNCOLOURED out-of-place loop
(colour = -1) runs into a scratch copy of u, then exactly the points of the box with  i0 + a * i1 + b * i2 == t  are copied back.
With a skew (a, b) under which every lexicographically later offset o of the stencil -- and the negative of every earlier one -- has
o0 + a * o1 + b * o2 > 0, the points of one t are independent of each other, all earlier neighbours of a point have a smaller t and
all later ones a larger t: the copy at time t holds, for each of its points, what the sequential nest computes there.  `skew` picks
(1, 1) where it is enough and (2, 4) otherwise, from this rule alone, and asserts it.  The arithmetic is the layers' own stencil_op,
pinned elsewhere; nothing here is shared with the HIP code.  `gs_nest` is the literal nest over Python floats, for the small cases
that pin the helper itself.

The stencils of the cases have pairwise distinct coefficients that are not dyadic, so a wrong neighbour or a stale value changes bits.
"""
import numpy as np

from exastencils_amd.field import Stencil
from stencil_cases import OFFSETS27, SMOOTH, ExactOps, FoldOps, _Lay


def later(o):
    """Does the point i + o come after i in the nest `for i2: for i1: for i0`?"""
    return o[2] > 0 or (o[2] == 0 and (o[1] > 0 or (o[1] == 0 and o[0] > 0)))


def skew(offsets):
    deps = [tuple(o) if later(o) else tuple(-v for v in o) for o in offsets if any(o)]
    for a, b in ((1, 1), (2, 4)):
        if all(o[0] + a * o[1] + b * o[2] > 0 for o in deps):
            return a, b
    raise AssertionError("no skew for offsets of reach 2")


def time_mask(l, a, b, t, begin, end):
    """Flat boolean mask over the allocation of layout `l`: the points of [begin, end) with i0 + a * i1 + b * i2 == t."""
    L = _Lay(l)
    m = np.zeros(L.shape, dtype=bool)
    i2, i1, i0 = np.meshgrid(*[np.arange(begin[d], end[d]) for d in (2, 1, 0)], indexing="ij")
    m[L.box(begin, end)] = (i0 + a * i1 + b * i2) == t
    return m.reshape(-1)


def _host(t):
    return t.numpy() if hasattr(t, "numpy") and not isinstance(t, np.ndarray) else t


class GsMixin:
    def gs_sweep(self, lu, u, lf, rhs, st, w, begin, end):
        self.gs_calls = getattr(self, "gs_calls", 0) + 1
        if any(end[d] <= begin[d] for d in range(3)):
            return
        a, b = skew(st.offsets)
        t_lo = begin[0] + a * begin[1] + b * begin[2]
        t_hi = (end[0] - 1) + a * (end[1] - 1) + b * (end[2] - 1)
        for t in range(t_lo, t_hi + 1):
            scratch = self.clone(u) if hasattr(self, "clone") else u.clone()
            self.stencil_op(SMOOTH, lu, u, lf, rhs, lu, scratch, st, w, -1, begin, end)
            m = time_mask(lu, a, b, t, begin, end)
            _host(u)[m] = _host(scratch)[m]


class FoldGS(GsMixin, FoldOps):
    pass


class ExactGS(GsMixin, ExactOps):
    pass


def oracle_gs():
    """OracleOps with gs_sweep (imported late: the oracle library is built on first use)."""
    from oracle_ops import OracleOps

    class OracleGS(GsMixin, OracleOps):
        pass

    return OracleGS()


def gs_nest(lu, u, lf, rhs, st, w, begin, end):
    """The statement itself: the sequential nest over Python floats on the flat host arrays u (in place) and rhs; coefficient fields in
    planes; entries folded left to right, `rhs - acc`, `u + ww * (..)` with ww in the stencil's weight form."""
    Lu, Lf = _Lay(lu), _Lay(lf)

    def lin(L, i0, i1, i2):
        return (i0 + L.ref[0]) + L.tot[0] * ((i1 + L.ref[1]) + L.tot[1] * (i2 + L.ref[2]))

    cf, Lc, csize = None, None, 0
    if st.cfield is not None:
        cf, Lc = _host(st.cfield), _Lay(st.clayout)
        csize = Lc.tot[0] * Lc.tot[1] * Lc.tot[2]
    w = float(w)
    for i2 in range(begin[2], end[2]):
        for i1 in range(begin[1], end[1]):
            for i0 in range(begin[0], end[0]):
                ic = lin(Lc, i0, i1, i2) if cf is not None else 0
                acc = None
                for k, o in enumerate(st.offsets):
                    c = float(cf[k * csize + ic]) if cf is not None else float(st.coefs[k])
                    term = c * float(u[lin(Lu, i0 + o[0], i1 + o[1], i2 + o[2])])
                    acc = term if acc is None else acc + term
                ww = w
                if cf is not None:
                    dg = float(cf[st.diag_index * csize + ic])
                    ww = (w / dg) if int(getattr(st, "wform", 0)) == 1 else ((1.0 / dg) * w)
                iu = lin(Lu, i0, i1, i2)
                u[iu] = float(u[iu]) + ww * (float(rhs[lin(Lf, i0, i1, i2)]) - acc)


# -- the stencils of the cases: pairwise distinct, non-dyadic coefficients, the diagonal dominant ---------------------------------------
def _stencil(offsets, seed, centre_last=False):
    others = [o for o in offsets if any(o)]
    r = np.random.default_rng(seed).uniform(0.1, 1.3, len(others))
    coef = {o: -float(v) for o, v in zip(others, r)}
    coef[(0, 0, 0)] = 1.1 * float(r.sum())
    order = others + [(0, 0, 0)] if centre_last else [(0, 0, 0)] + others
    st = Stencil(order, [coef[o] for o in order])
    assert len(set(st.coefs)) == len(order)
    return st


OFFSETS5 = [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0)]
OFFSETS7 = OFFSETS5 + [(0, 0, -1), (0, 0, 1)]
OFFSETS9 = [(a, b, 0) for b in (-1, 0, 1) for a in (-1, 0, 1)]


def five_point(centre_last=False):
    return _stencil(OFFSETS5, 105, centre_last)


def seven_point(centre_last=False):
    return _stencil(OFFSETS7, 107, centre_last)


def nine_point(centre_last=False):
    return _stencil(OFFSETS9, 109, centre_last)


def twentyseven_point(centre_last=False):
    return _stencil(OFFSETS27, 127, centre_last)


def upwind(nd):
    """An asymmetric stencil: the centre, the lower x neighbour, one diagonal whose mirror image is absent (its skew must still hold
    for the points that read it) and, in 3-D, one body diagonal."""
    offs = [(1, -1, 0), (0, 0, 0), (-1, 0, 0), (0, 1, 0)] + ([(-1, 1, -1), (0, 0, 1)] if nd == 3 else [])
    return Stencil(offs, [-0.37, 3.3, -0.91, -0.53] + ([-0.29, -0.61] if nd == 3 else []))


def coefficient_field(ops, clayout, wform, seed=131):
    """The 7-entry coefficient field (planes) over the whole allocation of `clayout`: U(-1, 1), the diagonal U(2, 4); the diagonal is
    entry 2 of the list."""
    from stencil_cases import AXES, ORDERS7, coefficient_array

    offs = [AXES[n] for n in ORDERS7["perm_a"]]
    return Stencil(offs, [], ops.from_host(coefficient_array(offs, clayout, "random", seed)), clayout, 0, wform)


def field_of(ops, offsets, clayout, wform, seed=137):
    """A coefficient field (planes) with the entry list `offsets` over the whole allocation of `clayout`, wherever the centre stands
    in the list: the diagonal U(2, 4), the others U(-1, 1) * 4 / entries -- their magnitudes sum to about 2, so a sweep over a long
    chain of dependent points stays bounded."""
    from stencil_cases import coefficient_array

    offs = [tuple(o) for o in offsets]
    a = coefficient_array(offs, clayout, "random", seed).reshape(len(offs), -1)
    for k, o in enumerate(offs):
        if any(o):
            a[k] *= 4.0 / len(offs)
    return Stencil(offs, [], ops.from_host(a.reshape(-1)), clayout, 0, wform)


def centre_only():
    """A diagonal operator: reach 0, no dependency at all."""
    return Stencil([(0, 0, 0)], [2.3])
