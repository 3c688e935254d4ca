"""The three-step pass under whole-round launch plans (csrc/ts3_plan.h): a main segment of several rounds of the CUs, a trailing segment
of short chunks for the leftover columns, layers in natural order and in interleaved halves -- forced on small boxes through the debug
build with the assumed CU count set to 8 and to 12.  Every plan must give the bits of the oracle's three loops and leave the output
array alone outside the box."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_kernels import assert_same, hip, hipd, orc  # noqa: F401  (fixtures and helpers of the kernel parity tests)

from exastencils_amd.field import laplace_fd
from exastencils_amd.layout import FieldLayout

SHAPES = [((130, 130, 130), None, None), ((165, 150, 141), None, None), ((150, 130, 110), [3, 2, 5], [148, 127, 108])]
# (assumed CUs, layers per round, rounds): 14 or 16 tile columns -> 8 columns x 3 layers + 6 or 8 leftover columns in two chunks each;
# 6 columns x 6 layers + 8 or 10 leftover columns; 12 columns x 4 layers + 2 or 4 leftover columns in short chunks
PLANS = [(8, 1, 3), (12, 2, 3), (12, 1, 4)]
_reference = {}


def _run(ops, kind, shape, st, b, e):
    lu, lf = FieldLayout.node(3, shape, 1), FieldLayout.node(3, shape, 0)
    u, fr, out, tmp = ops.new_array(lu.size), ops.new_array(lf.size), ops.new_array(lu.size), ops.new_array(lu.size)
    ops.fill_random(u, 12345)
    ops.fill_random(fr, 4711)
    ops.fill_random(out, 5)          # whatever the output array holds outside the box must survive
    if kind == "jacobi3":
        ops.jacobi3(lu.c_struct(), u, out, tmp, lf.c_struct(), fr, st, 0.8 / st.diag, b, e)
    else:
        ops.rbgs_colours3(lu.c_struct(), u, out, lf.c_struct(), fr, st, 0.8 / st.diag, int(kind[-1]), b, e)
    return [out, u]


def _want(orc, kind, shape, order, st, b, e):
    """The oracle's three loops, computed once per case and shared by all plans."""
    key = (kind, shape, order, tuple(b), tuple(e))
    if key not in _reference:
        ref = [orc.to_host(t).copy() for t in _run(orc, kind, shape, st, b, e)]
        for a in ref:
            a.setflags(write=False)
        _reference[key] = ref
    return _reference[key]


def _outside_untouched(out, shape, b, e):
    """The output array outside the box still holds fill_random(seed 5)."""
    lu = FieldLayout.node(3, shape, 1)
    if ("init", shape) not in _reference:
        from oracle_ops import OracleOps

        ops = OracleOps()
        init = ops.new_array(lu.size)
        ops.fill_random(init, 5)
        _reference[("init", shape)] = ops.to_host(init).reshape(lu.tot(2), lu.tot(1), lu.tot(0)).copy()
    init = _reference[("init", shape)]
    got = out.reshape(lu.tot(2), lu.tot(1), lu.tot(0))
    mask = np.ones(got.shape, dtype=bool)
    mask[tuple(slice(b[d] + lu.ref(d), e[d] + lu.ref(d)) for d in (2, 1, 0))] = False
    return np.array_equal(got[mask], init[mask])


@pytest.fixture
def hip3plan(hipd):
    """The debug build with the size bound of the three-step pass lowered to 2^20 points, and the plan hook bound."""
    hipd.L.examg_debug_three_stage.argtypes = [C.c_int] * 2
    hipd.L.examg_debug_three_stage_plan.argtypes = [C.c_int] * 4
    hipd.L.examg_debug_three_stage(2, -1)
    yield hipd
    hipd.L.examg_debug_three_stage_plan(0, 0, -1, 0)
    hipd.L.examg_debug_three_stage(0, -1)


@pytest.mark.parametrize("order", ["mp", "pm"])
@pytest.mark.parametrize("kind", ["jacobi3", "colours3_0", "colours3_1"])
@pytest.mark.parametrize("shape,b,e", SHAPES)
def test_whole_round_plans_bit_exact(hip3plan, orc, shape, b, e, kind, order):
    hipd = hip3plan
    st = laplace_fd(3, tuple(1.0 / n for n in shape), order)
    if b is None:
        b, e = [1, 1, 1], list(shape)
    assert hipd.three_stage_eligible(FieldLayout.node(3, shape, 1).c_struct(), FieldLayout.node(3, shape, 0).c_struct(), st, b, e)
    want = _want(orc, kind, shape, order, st, b, e)
    for cus, m, rounds in PLANS:
        for layer_order in (0, 1):
            hipd.L.examg_debug_three_stage_plan(m, rounds, layer_order, cus)
            got = _run(hipd, kind, shape, st, b, e)
            hipd.synchronize()
            got = [hipd.to_host(t) for t in got]
            what = "%s, %d CUs, %d layers per round, %d rounds, order %d" % (kind, cus, m, rounds, layer_order)
            assert_same(got, want, what)
            assert _outside_untouched(got[0], shape, b, e), what


@pytest.mark.parametrize("kind", ["jacobi3", "colours3_0", "colours3_1"])
def test_default_plan_on_the_product_library(hip, orc, kind):
    """The product library and its own plan at the smallest shape it takes (8e6 points): 264 x 200 x 170 against the oracle's three loops."""
    shape = (264, 200, 170)
    st = laplace_fd(3, tuple(1.0 / n for n in shape), "mp")
    b, e = [1, 1, 1], list(shape)
    lu, lf = FieldLayout.node(3, shape, 1), FieldLayout.node(3, shape, 0)
    assert hip.three_stage_eligible(lu.c_struct(), lf.c_struct(), st, b, e)
    got = _run(hip, kind, shape, st, b, e)
    hip.synchronize()
    got = [hip.to_host(t) for t in got]
    assert_same(got, _want(orc, kind, shape, "mp", st, b, e), kind)
    assert _outside_untouched(got[0], shape, b, e)
