"""Multi-colour loops on the reference kernel layers (test helper, no test functions).

MulticolourMixin gives a kernel layer that has `stencil_op` (FoldOps, ExactOps of stencil_cases.py, OracleOps) the two methods of the
multi-colour ABI, `stencil_op_coloured` and `mcgs_sweep`, without touching those classes: the UNCOLOURED loop (colour = -1) runs out of
place into a scratch copy of dst, then exactly the points of the box that belong to the colour are copied into dst.  The colour test
is include/examg.h's definition in plain numpy: a point belongs to a colour when (shift_k + sum of i_d over the axes of expression k)
% mod_k == rem_k for every expression k.  For a colouring that decouples the stencil this is the in-place loop bit for bit -- no
point of the colour reads another point of the colour, so every point sees the values it would see in any loop order -- and the mixin
asserts decoupling itself when u is dst.  The colour order of a sweep is written out here as nested loops (the first expression
fastest), independently of exastencils_amd.field.Colouring.colours.
"""
import numpy as np

from exastencils_amd.field import Colouring
from stencil_cases import SMOOTH, ExactOps, FoldOps, _Lay


def decouples(exprs, offsets):
    """include/examg.h: every entry offset o != 0 has an expression with (sum of o_d over its axes) mod n != 0."""
    for o in offsets:
        if not any(o):
            continue
        if not any(sum(o[d] for d in axes) % mod != 0 for axes, _, mod in exprs):
            return False
    return True


def colour_mask(l, col, begin, end):
    """Flat boolean mask over the allocation of layout `l`: the points of [begin, end) that belong to the colour `col`."""
    L = _Lay(l)
    m = np.zeros(L.shape, dtype=bool)
    if any(end[d] <= begin[d] for d in range(3)):
        return m.reshape(-1)
    i2, i1, i0 = np.meshgrid(*[np.arange(begin[d], end[d]) for d in (2, 1, 0)], indexing="ij")
    idx = (i0, i1, i2)
    inside = np.ones(i0.shape, dtype=bool)
    for (axes, shift, mod), rem in zip(col.exprs, col.rem):
        v = shift + sum(idx[d] for d in axes)
        assert v.min() >= 0, "a colour expression is negative in the box: C's % and the remainder differ there"
        inside &= (v % mod) == rem
    m[L.box(begin, end)] = inside
    return m.reshape(-1)


def colours_in_order(col):
    """The colours of a colouring in the order of the reference's colour loops (L4_ColorLoops.toRepeatLoops): the LAST expression is
    the outermost loop, the first one the innermost."""
    mods = [e[2] for e in col.exprs] + [1, 1]
    out = []
    for r2 in range(mods[2]):
        for r1 in range(mods[1]):
            for r0 in range(mods[0]):
                out.append(Colouring(col.exprs, (r0, r1, r2)[:len(col.exprs)]))
    return out


def _host(t):
    return t.numpy() if hasattr(t, "numpy") and not isinstance(t, np.ndarray) else t


def _same(a, b):
    return a is b or (hasattr(a, "data_ptr") and hasattr(b, "data_ptr") and a.data_ptr() == b.data_ptr())


class MulticolourMixin:
    def stencil_op_coloured(self, mode, lu, u, lf, rhs, ld, dst, st, w, col, begin, end):
        if any(end[d] <= begin[d] for d in range(3)):
            return
        if _same(u, dst):
            assert decouples(col.exprs, st.offsets), "in-place loop over a colour that the colouring does not decouple"
        scratch = self.clone(dst) if hasattr(self, "clone") else dst.clone()
        self.stencil_op(mode, lu, u, lf, rhs, ld, scratch, st, w, -1, begin, end)
        m = colour_mask(ld, col, begin, end)
        _host(dst)[m] = _host(scratch)[m]

    def mcgs_sweep(self, lu, u, lf, rhs, st, w, col, begin, end):
        assert decouples(col.exprs, st.offsets)
        for c in colours_in_order(col):
            self.stencil_op_coloured(SMOOTH, lu, u, lf, rhs, lu, u, st, w, c, begin, end)


class FoldMC(MulticolourMixin, FoldOps):
    pass


class ExactMC(MulticolourMixin, ExactOps):
    pass


def oracle_mc():
    """OracleOps with the two methods (imported late: the oracle library is built on first use)."""
    from oracle_ops import OracleOps

    class OracleMC(MulticolourMixin, OracleOps):
        pass

    return OracleMC()


# -- colourings and stencils of the tests ---------------------------------------------------------------------------------------------
AXIS8 = Colouring((((0,), 0, 2), ((1,), 0, 2), ((2,), 0, 2)))          # i0 % 2, i1 % 2, i2 % 2
AXIS4 = Colouring((((0,), 0, 2), ((1,), 0, 2)))                        # i0 % 2, i1 % 2
AXIS9 = Colouring((((0,), 0, 3), ((1,), 0, 3)))                        # i0 % 3, i1 % 3
PARITY3 = Colouring((((0, 1, 2), 0, 2),))                              # (i0 + i1 + i2) % 2
PARITY2 = Colouring((((0, 1), 0, 2),))
MIXED = Colouring((((0, 1), 1, 3), ((2,), 1, 2)))                      # (1 + i0 + i1) % 3, (1 + i2) % 2: a row start and stride + a lattice


def nine_point(data="random"):
    """A 2-D 9-point stencil with pairwise distinct coefficients, the centre first: random (not dyadic) or multiples of 1/4."""
    from exastencils_amd.field import Stencil

    offs = [(0, 0, 0)] + [(a, b, 0) for b in (-1, 0, 1) for a in (-1, 0, 1) if (a, b) != (0, 0)]
    if data == "exact":
        coefs = [8.0] + [0.25 * s * k for k, s in zip(range(1, 9), (1, -1, -1, 1, -1, 1, 1, -1))]
    else:
        r = np.random.default_rng(99).uniform(0.1, 1.3, 8)
        coefs = [1.1 * float(r.sum())] + [-float(v) for v in r]
    assert len(set(coefs)) == 9
    return Stencil(offs, coefs)
