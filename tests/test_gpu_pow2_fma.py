"""Off-centre coefficients +-2^e, e >= 0 (every power-of-two grid): the three-step Jacobi pass and the plain Jacobi pair of eight waves
with streaming stores fuse the six off-centre products of a convolution into their sums (conv7<ORDER, FMA>; examg_pow2_fma_eligible).
The products are exact, so every value must keep the bits of the separate loops: all comparisons here are bit for bit (as 64-bit
integers: the sign of a zero counts) against the CPU oracle's loops one after the other, at power-of-two shapes -- the shapes at which
the fused forms run."""
import ctypes as C

import numpy as np
import pytest

from oracle_ops import OracleOps

from exastencils_amd.field import Stencil, laplace_fd, laplace_unit
from exastencils_amd.layout import FieldLayout

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def hipd():
    from exastencils_amd import lib
    from exastencils_amd.ops import HipOps

    return HipOps(0, lib.DBG_LIB_PATH)


@pytest.fixture
def hip3(hipd):
    """The debug build with the size bound of the three-stage pass lowered to 2^20 points: 128^3 reaches the kernel."""
    hipd.L.examg_debug_three_stage.argtypes = [C.c_int] * 2
    hipd.L.examg_debug_pow2_fma.argtypes = [C.c_int]
    hipd.L.examg_debug_three_stage(2, -1)
    yield hipd
    hipd.L.examg_debug_three_stage(0, -1)
    hipd.L.examg_debug_pow2_fma(1)


@pytest.fixture(params=[8, 83], ids=["two_rows", "three_rows"])
def pair8(hipd, request):
    """The debug build with the two-step pass forced to its eight-wave workgroups (two / three rows per wave: the forms of 192 rows and
    more) and to streaming stores (the store policy from 8.4 * 10^6 points on): 128^3 reaches the forms that have the fused arithmetic."""
    hipd.L.examg_debug_two_stage_lds.argtypes = [C.c_int]
    hipd.L.examg_debug_two_stage_nt.argtypes = [C.c_int]
    hipd.L.examg_debug_pow2_fma.argtypes = [C.c_int]
    hipd.L.examg_debug_two_stage_lds(request.param)
    hipd.L.examg_debug_two_stage_nt(1)
    yield hipd
    hipd.L.examg_debug_two_stage_lds(-1)
    hipd.L.examg_debug_two_stage_nt(-1)
    hipd.L.examg_debug_pow2_fma(1)


@pytest.fixture(scope="module")
def orc():
    return OracleOps()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_same_bits(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        d = bits(a) != bits(b)
        if d.any():
            j = int(np.flatnonzero(d)[0])
            raise AssertionError("%s[%d]: %d of %d values differ in their bits, first at %d: %r against %r"
                                 % (what, i, int(d.sum()), d.size, j, float(a[j]), float(b[j])))


def layouts(shape):
    return FieldLayout.node(3, shape, 1), FieldLayout.node(3, shape, 0)


def steps(ops, kind, lu, u, out, tmp, lf, fr, st, b, e):
    if kind == "jacobi3":
        ops.jacobi3(lu.c_struct(), u, out, tmp, lf.c_struct(), fr, st, 0.8 / st.diag, b, e)
    else:
        tmp.copy_(u)      # the separate loops step through tmp: outside the box it must hold u's values (the one-pass kernel never touches it)
        ops.jacobi2(lu.c_struct(), u, out, tmp, lf.c_struct(), fr, st, 0.8 / st.diag, b, e)


def jacobi3_random(ops, shape, st, b, e, kind="jacobi3"):
    lu, lf = layouts(shape)
    u, fr, out, tmp = ops.new_array(lu.size), ops.new_array(lf.size), ops.new_array(lu.size), ops.new_array(lu.size)
    ops.fill_random(u, 12345)
    ops.fill_random(fr, 4711)
    ops.fill_random(out, 5)
    steps(ops, kind, lu, u, out, tmp, lf, fr, st, b, e)
    return [out, u]


def jacobi3_given(ops, shape, st, b, e, u_host, f_host, kind="jacobi3"):
    """The same with fields uploaded from host arrays; the output starts as zeros outside the box on both sides."""
    lu, lf = layouts(shape)
    u, fr = ops.from_host(u_host.copy()), ops.from_host(f_host.copy())
    out, tmp = ops.new_array(lu.size), ops.new_array(lu.size)
    steps(ops, kind, lu, u, out, tmp, lf, fr, st, b, e)
    return [out, u]


def both(hip, orc, fn):
    g = fn(hip)
    hip.synchronize()
    c = fn(orc)
    return [hip.to_host(t) for t in g], [orc.to_host(t) for t in c]


def full_box(shape):
    return [1, 1, 1], list(shape)


@gpu
@pytest.mark.parametrize("order", ["mp", "pm"])
@pytest.mark.parametrize("shape,b,e", [((128, 128, 128), None, None),
                                       ((128, 128, 128), [3, 2, 5], [125, 126, 123]),      # ragged box inside the inner points
                                       ((256, 128, 64), None, None)])                      # coefficients -2^16, -2^14, -2^12
def test_fused_route_taken_and_exact(hip3, orc, shape, b, e, order):
    """examg_jacobi3 on power-of-two grids: the one-pass kernel in its fused form (both queries say so), against three loops."""
    st = laplace_fd(3, tuple(1.0 / n for n in shape), order)
    if b is None:
        b, e = full_box(shape)
    lu, lf = layouts(shape)
    assert hip3.pow2_fma_eligible(st)
    assert hip3.three_stage_eligible(lu.c_struct(), lf.c_struct(), st, b, e)
    g, c = both(hip3, orc, lambda ops: jacobi3_random(ops, shape, st, b, e))
    assert_same_bits(g, c, "jacobi3 %s %s" % (shape, order))


@gpu
def test_route_not_taken_off_power_of_two(hip3, orc):
    """130 x 128 x 128: the x coefficient is -16900 -- the separate products and sums, and the oracle's bits as before."""
    shape = (130, 128, 128)
    st = laplace_fd(3, tuple(1.0 / n for n in shape), "mp")
    assert st.coefs[1] == -16900.0
    b, e = full_box(shape)
    lu, lf = layouts(shape)
    assert not hip3.pow2_fma_eligible(st)
    assert hip3.three_stage_eligible(lu.c_struct(), lf.c_struct(), st, b, e)
    g, c = both(hip3, orc, lambda ops: jacobi3_random(ops, shape, st, b, e))
    assert_same_bits(g, c, "jacobi3 130 x 128 x 128")


def exact_integer_fields(shape, st):
    """u: small integers (zeros of both signs among them), rhs = A u in integer arithmetic: every product and sum of the first step is
    exact and every residual rhs - A u cancels to a zero."""
    lu, lf = layouts(shape)
    rng = np.random.default_rng(20)
    tu = tuple(lu.tot(d) for d in (2, 1, 0))
    ui = rng.integers(-8, 9, size=tu, dtype=np.int64)
    k = [int(c) for c in st.coefs]
    assert [float(c) for c in k] == list(st.coefs)
    au = k[0] * ui[1:-1, 1:-1, 1:-1]
    for kk, o in zip(k[1:], st.offsets[1:]):
        au = au + kk * ui[1 + o[2]:tu[0] - 1 + o[2], 1 + o[1]:tu[1] - 1 + o[1], 1 + o[0]:tu[2] - 1 + o[0]]
    # array position = index + ref: u has one ghost layer (ref 1), the rhs none (ref 0); A u exists on indices 0 .. n of every axis
    f = np.zeros(tuple(lf.tot(d) for d in (2, 1, 0)))
    f[...] = au[:f.shape[0], :f.shape[1], :f.shape[2]].astype(np.float64)
    u = ui.astype(np.float64)
    u[(ui == 0) & (rng.integers(0, 2, size=tu) == 1)] = -0.0
    assert np.abs(au).max() < 2 ** 52
    return u.reshape(-1), f.reshape(-1)


def wide_range_fields(shape):
    """Magnitudes 2^p, p uniform in [-1060, 900], random signs: subnormals, no inf or NaN, and nothing overflows in three steps
    (coefficients up to 2^17, weight about 2^-17)."""
    lu, lf = layouts(shape)
    rng = np.random.default_rng(21)

    def draw(n):
        x = np.ldexp(1.0, rng.integers(-1060, 901, size=n).astype(np.int32))
        return np.where(rng.integers(0, 2, size=n) == 1, -x, x)

    u, f = draw(lu.size), draw(lf.size)
    assert np.isfinite(u).all() and np.isfinite(f).all() and (np.abs(u) < 2.0 ** -1022).any()
    return u, f


def host_fields(orc, data, shape, st):
    if data == "integers":
        return exact_integer_fields(shape, st)
    if data == "wide":
        return wide_range_fields(shape)
    lu, lf = layouts(shape)
    u, f = orc.new_array(lu.size), orc.new_array(lf.size)
    orc.fill_random(u, 31)
    orc.fill_random(f, 32)
    return orc.to_host(u), orc.to_host(f)


@gpu
@pytest.mark.parametrize("data", ["random", "integers", "wide"])
def test_data_that_would_expose_a_wrong_fusion(hip3, orc, data):
    shape = (128, 128, 128)
    st = laplace_fd(3, (1.0 / 128,) * 3, "mp")
    b, e = full_box(shape)
    assert hip3.pow2_fma_eligible(st)
    u, f = host_fields(orc, data, shape, st)
    g, c = both(hip3, orc, lambda ops: jacobi3_given(ops, shape, st, b, e, u, f))
    assert np.isfinite(c[0]).all()
    assert_same_bits(g, c, "jacobi3, %s data" % data)


@gpu
@pytest.mark.parametrize("zc", [28, 24, 5])
def test_fused_form_with_forced_chunks(hip3, orc, zc):
    """The fused form takes chunks of at most 28 planes on boxes of 10^8 points and more: those chunk lengths here, on a box the oracle
    sweeps in a moment (127 planes: partial last chunks)."""
    shape = (128, 128, 128)
    st = laplace_fd(3, (1.0 / 128,) * 3, "mp")
    b, e = full_box(shape)
    want = [orc.to_host(t) for t in jacobi3_random(orc, shape, st, b, e)]
    hip3.L.examg_debug_three_stage(2, zc)
    got = jacobi3_random(hip3, shape, st, b, e)
    hip3.synchronize()
    assert_same_bits([hip3.to_host(t) for t in got], want, "jacobi3, chunks of %d planes" % zc)


@gpu
@pytest.mark.parametrize("order", ["mp", "pm"])
@pytest.mark.parametrize("shape,b,e", [((128, 128, 128), None, None),
                                       ((128, 128, 128), [3, 2, 5], [125, 126, 123]),
                                       ((256, 128, 64), None, None)])
def test_jacobi_pair_fused_route_taken_and_exact(pair8, orc, shape, b, e, order):
    """examg_jacobi2 through the eight-wave forms with streaming stores, against two loops."""
    st = laplace_fd(3, tuple(1.0 / n for n in shape), order)
    if b is None:
        b, e = full_box(shape)
    lu, lf = layouts(shape)
    assert pair8.pow2_fma_eligible(st)
    assert pair8.two_stage_eligible(lu.c_struct(), lf.c_struct(), st, b, e, b, e)
    g, c = both(pair8, orc, lambda ops: jacobi3_random(ops, shape, st, b, e, "jacobi2"))
    assert_same_bits(g, c, "jacobi2 %s %s" % (shape, order))


@gpu
@pytest.mark.parametrize("data", ["random", "integers", "wide"])
def test_jacobi_pair_data_that_would_expose_a_wrong_fusion(pair8, orc, data):
    shape = (128, 128, 128)
    st = laplace_fd(3, (1.0 / 128,) * 3, "mp")
    b, e = full_box(shape)
    u, f = host_fields(orc, data, shape, st)
    g, c = both(pair8, orc, lambda ops: jacobi3_given(ops, shape, st, b, e, u, f, "jacobi2"))
    assert np.isfinite(c[0]).all()
    assert_same_bits(g, c, "jacobi2, %s data" % data)
    if data == "wide":      # and the switch: the separate products on the same launch path
        try:
            pair8.L.examg_debug_pow2_fma(0)
            off = jacobi3_given(pair8, shape, st, b, e, u, f, "jacobi2")
            pair8.synchronize()
            assert_same_bits([pair8.to_host(t) for t in off], g, "jacobi2, switch off against on")
        finally:
            pair8.L.examg_debug_pow2_fma(1)


@gpu
def test_switch_off_and_on_give_the_same_bits(hip3, orc):
    """examg_debug_pow2_fma(0): the separate products and sums on the same launch path; (1): the fused form again."""
    shape = (128, 128, 128)
    st = laplace_fd(3, (1.0 / 128,) * 3, "pm")
    b, e = full_box(shape)
    u, f = wide_range_fields(shape)
    want = [orc.to_host(t) for t in jacobi3_given(orc, shape, st, b, e, u, f)]
    got = []
    try:
        for on in (0, 1):
            hip3.L.examg_debug_pow2_fma(on)
            out = jacobi3_given(hip3, shape, st, b, e, u, f)
            hip3.synchronize()
            got.append([hip3.to_host(t) for t in out])
    finally:
        hip3.L.examg_debug_pow2_fma(1)
    assert_same_bits(got[0], got[1], "switch off against on")
    assert_same_bits(got[1], want, "switch on against the oracle")


def star(coefs, offsets=None):
    st = laplace_fd(3, (1.0, 1.0, 1.0), "mp")
    return Stencil(list(offsets) if offsets else list(st.offsets), [float(c) for c in coefs])


def test_predicate_truth_table():
    """examg_pow2_fma_eligible needs no device: the product library, loaded as tests/test_abi.py loads it."""
    import __graft_entry__ as ge

    from exastencils_amd import lib

    ge.build_examg()
    L = C.CDLL(lib.LIB_PATH)
    L.examg_pow2_fma_eligible.argtypes = [C.POINTER(lib.StencilC)]
    L.examg_pow2_fma_eligible.restype = C.c_int

    def ask(st, field=False):
        sc = st.c_struct()
        keep = C.create_string_buffer(8)
        if field:
            sc.cfield = C.addressof(keep)      # a stencil field: the coefficients live in an array (never read by the query)
        return L.examg_pow2_fma_eligible(C.byref(sc))

    inf, nan, p18 = float("inf"), float("nan"), 2.0 ** 18
    assert ask(star([6 * p18] + [-p18] * 6)) == 1
    assert ask(laplace_fd(3, (2.0 ** -9,) * 3, "mp")) == 1 and ask(laplace_fd(3, (2.0 ** -9,) * 3, "pm")) == 1
    assert ask(laplace_unit(3)) == 1                                      # -1.0 = -2^0
    assert ask(star([6.0] + [1.0] * 6)) == 1                              # +2^0
    assert ask(star([1.0, -2.0 ** 16, -2.0 ** 16, -2.0 ** 14, -2.0 ** 14, 2.0 ** 12, -1.0])) == 1     # mixed exponents and signs
    assert ask(star([3.0] + [-0.5] * 6)) == 0                             # 2^-1: e < 0
    assert ask(star([18 * p18] + [-3 * p18] * 6)) == 0
    for bad in (0.0, -0.0, inf, -inf, nan, -0.5, 3.0, 16900.0):
        for at in (1, 6):
            co = [6 * p18] + [-p18] * 6
            co[at] = bad
            assert ask(star(co)) == 0, (bad, at)                          # five powers of two and one other value
    o = laplace_fd(3, (1.0, 1.0, 1.0), "mp").offsets
    assert ask(star([6.0] + [-1.0] * 6, [o[0], o[1], o[2], o[5], o[6], o[3], o[4]])) == 0          # seven entries, no canonical order
    assert ask(star([6 * p18] + [-p18] * 6), field=True) == 0
    assert L.examg_pow2_fma_eligible(None) == 0
