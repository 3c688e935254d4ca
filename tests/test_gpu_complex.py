"""The complex-field kernels on the MI355X against the numpy restatement tests/complex_ops.py.

Point-wise entry points (examg_cstencil_op in its four modes on both kernels, examg_clincomb, the transfers, examg_cshift_div,
examg_cfrom_parts) are compared bit for bit over the WHOLE arrays: the box holds numpy's bits, every double outside the box and every input
keeps its own.  + - * / are one IEEE rounding each on both sides.  examg_cdot is compared with exact integers and with the derived bound of a
sum of 2 K rounded terms.  Shapes, stencils and data: tests/complex_cases.py."""

import numpy as np
import pytest

from exastencils_amd import lib
from exastencils_amd.layout import FieldLayout
from exastencils_amd.lib import ExamgError
from tests import complex_cases as cases
from tests import complex_ops as cops

pytestmark = pytest.mark.gpu

ORC = cops.ComplexOps()


@pytest.fixture(scope="module")
def hip():
    from exastencils_amd.ops import HipOps

    return HipOps(0)


@pytest.fixture(scope="module")
def hipd():
    """The debug library: examg_debug_cstencil_route forces either kernel and the rows per wave of the marching one."""
    from exastencils_amd.ops import HipOps

    ops = HipOps(0, lib.DBG_LIB_PATH)
    yield ops
    ops.L.examg_debug_cstencil_route(0, 0)


def host(ops, t):
    ops.synchronize()
    return np.array(ops.to_host(t), dtype=np.float64, copy=True)


def same_bits(got, want, what):
    if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
        bad = got.view(np.uint64) != want.view(np.uint64)
        raise AssertionError("%s: %d of %d values differ, max abs %.3e" % (what, int(bad.sum()), bad.size, float(np.nanmax(np.abs(got - want)[bad]))))


def run_stencil(ops, mode, lu, u, lf, f, ld, d, st, w, colour, b, e, alias=False):
    """One cstencil_op from host data; (u, rhs, dst) afterwards.  alias: dst is u (in place)."""
    tu, tf = ops.from_host(u.copy()), ops.from_host(f.copy())
    td = tu if alias else ops.from_host(d.copy())
    if mode == cops.CRELAX:
        ops.cstencil_op(mode, lu.c_struct(), tu, lf.c_struct(), tf, None, None, st, w, colour, b, e)
    else:
        ops.cstencil_op(mode, lu.c_struct(), tu, lf.c_struct(), tf, (lu if alias else ld).c_struct(), td, st, w, colour, b, e)
    return host(ops, tu), host(ops, tf), host(ops, td)


# route, rows per wave of the marching kernel (2: several runs per column at these sizes, the rows between two runs are read by both)
ROUTES = [(lib.CSTENCIL_GATHER, 0), (lib.CSTENCIL_MARCH, 0), (lib.CSTENCIL_MARCH, 2)]


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_star_stencils_both_kernels_give_numpys_bits(hip, hipd, shape):
    nd, inner = cases.SHAPES[shape]
    lu, lf, ld = cases.layouts(nd, inner)
    u, f, d = cases.random_field(lu, 21), cases.random_field(lf, 22), cases.random_field(ld, 23)
    runs = 0
    for sname, st in cases.star_stencils(nd).items():
        for bname, (b, e) in cases.boxes(nd, inner).items():
            for mode, w in ((cops.APPLY, 0.0), (cops.RESIDUAL, 0.0), (cops.SMOOTH, 0.8 / st.coefs[st.offsets.index((0, 0, 0))]), (cops.CRELAX, 0.6),
                            (cops.CRELAX, 1.0)):
                for colour in ((0, 1) if mode == cops.CRELAX else (-1, 0, 1)):
                    # in place where the loop kind allows it: the coloured smoother of a star stencil, and the local solve
                    alias = mode == cops.CRELAX or (mode == cops.SMOOTH and colour >= 0)
                    what = "%s %s box %s mode %d colour %d" % (shape, sname, bname, mode, colour)
                    wu, wf, wd = u.copy(), f.copy(), d.copy()
                    ORC.cstencil_op(mode, lu.c_struct(), wu, lf.c_struct(), wf, (lu if alias else ld).c_struct(), wu if alias else wd, st, w, colour, b, e)
                    for route, chunk in ROUTES:
                        assert hipd.L.examg_debug_cstencil_route(route, chunk) == 0
                        args = (mode, lu.c_struct(), hipd.from_host(u), lf.c_struct(), hipd.from_host(f), ld.c_struct(), hipd.from_host(d), st, w, colour, b, e)
                        if mode == cops.CRELAX:
                            args = args[:5] + (None, None) + args[7:]
                        assert hipd.cstencil_route(*args) == route, what
                        gu, gf, gd = run_stencil(hipd, mode, lu, u, lf, f, ld, d, st, w, colour, b, e, alias)
                        same_bits(gu, wu, "%s route %d/%d: u" % (what, route, chunk))
                        same_bits(gf, f, "%s route %d/%d: rhs was written" % (what, route, chunk))
                        if not alias:
                            same_bits(gd, wd, "%s route %d/%d: dst" % (what, route, chunk))
                        runs += 1
                    # the product library, on the route of its own
                    gu, gf, gd = run_stencil(hip, mode, lu, u, lf, f, ld, d, st, w, colour, b, e, alias)
                    same_bits(gu, wu, what + " default route: u")
                    if not alias:
                        same_bits(gd, wd, what + " default route: dst")
    assert runs == 7 * 2 * (3 + 3 + 3 + 2 + 2) * 3


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_general_stencils_on_the_gather_kernel(hip, hipd, shape):
    """The asymmetric 9- / 27-point stencil and a star with an entry missing: no kernel but gather takes them, whatever is asked for."""
    nd, inner = cases.SHAPES[shape]
    lu, lf, ld = cases.layouts(nd, inner)
    u, f, d = cases.random_field(lu, 31), cases.random_field(lf, 32), cases.random_field(ld, 33)
    for sname, st in cases.gather_stencils(nd).items():
        for bname, (b, e) in cases.boxes(nd, inner).items():
            for mode, w in ((cops.APPLY, 0.0), (cops.RESIDUAL, 0.0), (cops.SMOOTH, 0.1 - 0.05j)):
                for colour in (-1, 0, 1):
                    what = "%s %s box %s mode %d colour %d" % (shape, sname, bname, mode, colour)
                    wu, wf, wd = u.copy(), f.copy(), d.copy()
                    ORC.cstencil_op(mode, lu.c_struct(), wu, lf.c_struct(), wf, ld.c_struct(), wd, st, w, colour, b, e)
                    for ops, forced in ((hip, 0), (hipd, lib.CSTENCIL_MARCH)):
                        if forced:
                            hipd.L.examg_debug_cstencil_route(forced, 0)
                        assert ops.cstencil_route(mode, lu.c_struct(), ops.from_host(u), lf.c_struct(), ops.from_host(f), ld.c_struct(), ops.from_host(d), st,
                                                  w, colour, b, e) == lib.CSTENCIL_GATHER, what
                        gu, gf, gd = run_stencil(ops, mode, lu, u, lf, f, ld, d, st, w, colour, b, e)
                        same_bits(gu, u, what + ": u was written")
                        same_bits(gf, f, what + ": rhs was written")
                        same_bits(gd, wd, what + ": dst")


def test_default_route_and_empty_box(hip):
    """Without a colour, star stencils on 10^6 points and more (rows of at least 64) march; smaller boxes, single colours and every other
    stencil gather (the measured table).  The route is decided from the arguments alone: nothing is launched, so small arrays
    stand in for the large fields.  An empty box is 0 and a no-op."""
    t, t2 = hip.new_complex_array(8), hip.new_complex_array(8)
    for nd, n, colour, stencil, want in ((2, 1024, -1, "star", lib.CSTENCIL_MARCH), (3, 128, -1, "star", lib.CSTENCIL_MARCH),
                                         (2, 1024, 0, "star", lib.CSTENCIL_GATHER), (2, 512, -1, "star", lib.CSTENCIL_GATHER),
                                         (3, 64, -1, "star", lib.CSTENCIL_GATHER), (3, 128, -1, "full", lib.CSTENCIL_GATHER)):
        lu = FieldLayout.node(nd, (n,) * nd, 1).c_struct()
        b, e = [0, 0, 0], [n + 1 if d < nd else 1 for d in range(3)]
        st = cases.star_stencils(nd)["mp_shifted"] if stencil == "star" else cases.gather_stencils(nd)["full"]
        assert hip.cstencil_route(cops.RESIDUAL, lu, t, lu, t, lu, t2, st, 0.0, colour, b, e) == want, (nd, n, colour, stencil)
    for shape in sorted(cases.SHAPES):
        nd, inner = cases.SHAPES[shape]
        lu, lf, ld = cases.layouts(nd, inner)
        tu, tf, td = (hip.from_host(cases.random_field(l, 41)) for l in (lu, lf, ld))
        b, e = cases.boxes(nd, inner)["whole"]
        st = cases.star_stencils(nd)["mp_shifted"]
        assert hip.cstencil_route(cops.RESIDUAL, lu.c_struct(), tu, lf.c_struct(), tf, ld.c_struct(), td, st, 0.0, -1, b, e) == lib.CSTENCIL_GATHER
        assert hip.cstencil_route(cops.RESIDUAL, lu.c_struct(), tu, lf.c_struct(), tf, ld.c_struct(), td, st, 0.0, -1, b, [e[0], b[1], e[2]]) == 0
        before = host(hip, td)
        hip.cstencil_op(cops.RESIDUAL, lu.c_struct(), tu, lf.c_struct(), tf, ld.c_struct(), td, st, 0.0, -1, b, [e[0], b[1], e[2]])
        same_bits(host(hip, td), before, "empty box")


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_lincomb_shift_and_parts_give_numpys_bits(hip, shape):
    nd, inner = cases.SHAPES[shape]
    lu, lf, ld = cases.layouts(nd, inner)
    lays = (lu, lf, ld)
    data = [cases.random_field(l, 51 + k) for k, l in enumerate(lays)]
    for bname, (b, e) in cases.boxes(nd, inner).items():
        for form in (cops.C_XPAY, cops.C_XMAY, cops.C_XPAYMBZ):
            for a, bb in ((0.3 - 1.1j, -0.8 + 0.25j), (1.75, -0.5), (0.0 + 2.0j, 1.0 + 0.0j)):
                for target in (0, 1, 2, 3):      # dst: x, y, z or an array of its own
                    if target == 2 and form != cops.C_XPAYMBZ:
                        continue
                    want = [x.copy() for x in data] + [cases.random_field(lu, 60)]
                    lt = lays[target] if target < 3 else lu
                    ORC.clincomb(form, lu.c_struct(), want[0], lf.c_struct(), want[1], ld.c_struct(), want[2], lt.c_struct(), want[target], a, bb, b, e)
                    t = [hip.from_host(x.copy()) for x in data] + [hip.from_host(cases.random_field(lu, 60))]
                    hip.clincomb(form, lu.c_struct(), t[0], lf.c_struct(), t[1], ld.c_struct(), t[2], lt.c_struct(), t[target], a, bb, b, e)
                    for k in range(4):
                        same_bits(host(hip, t[k]), want[k], "%s box %s form %d a %r target %d: array %d" % (shape, bname, form, a, target, k))
    # the absorbing-boundary assignment on both x faces and one y face, complex and real divisor
    b, e = cases.boxes(nd, inner)["whole"]
    for off, pb, pe in (((1, 0, 0), [0, 0, 0], [1, e[1], e[2]]), ((-1, 0, 0), [e[0] - 1, 0, 0], e), ((0, 2, 0), [1, 0, 0], [e[0] - 1, 1, e[2]])):
        for c in (1.0 - 0.625j, 2.5):
            want = data[0].copy()
            ORC.cshift_div(lu.c_struct(), want, off, c, pb, pe)
            t = hip.from_host(data[0].copy())
            hip.cshift_div(lu.c_struct(), t, off, c, pb, pe)
            same_bits(host(hip, t), want, "%s cshift_div off %r c %r" % (shape, off, c))
    # a complex field from real parts, each in a layout of its own; a missing part is 0.0
    lre = FieldLayout.node(nd, tuple(inner[d] + 1 for d in range(nd)), 0)
    lim = FieldLayout.node(nd, tuple(inner[d] + 1 for d in range(nd)), 1, align=2)
    re, im = np.random.default_rng(71).uniform(-1, 1, lre.size), np.random.default_rng(72).uniform(-1, 1, lim.size)
    for bname, (b, e) in cases.boxes(nd, inner).items():
        for use_re, use_im in ((True, True), (True, False), (False, True)):
            want = data[2].copy()
            ORC.cfrom_parts(ld.c_struct(), want, lre.c_struct(), re if use_re else None, lim.c_struct(), im if use_im else None, b, e)
            t, tre, tim = hip.from_host(data[2].copy()), hip.from_host(re.copy()), hip.from_host(im.copy())
            hip.cfrom_parts(ld.c_struct(), t, lre.c_struct(), tre if use_re else None, lim.c_struct(), tim if use_im else None, b, e)
            same_bits(host(hip, t), want, "%s cfrom_parts box %s" % (shape, bname))
            same_bits(host(hip, tre), re, "re was written")
            same_bits(host(hip, tim), im, "im was written")


@pytest.mark.parametrize("nd,inner_coarse", [(2, (3, 2, 1)), (2, (66, 4, 1)), (3, (3, 2, 2)), (3, (33, 3, 2))])
def test_transfers_give_numpys_bits_and_the_real_kernels_bits_on_the_parts(hip, nd, inner_coarse):
    lfine, lc = cases.transfer_layouts(nd, inner_coarse)
    fine, coarse = cases.random_field(lfine, 81), cases.random_field(lc, 82)
    whole_c = ([0, 0, 0], [inner_coarse[d] + 2 if d < nd else 1 for d in range(3)])
    inner_c = ([1 if d < nd else 0 for d in range(3)], [inner_coarse[d] + 1 if d < nd else 1 for d in range(3)])
    whole_f = ([0, 0, 0], [lfine.inner[d] + 2 if d < nd else 1 for d in range(3)])
    inner_f = ([1 if d < nd else 0 for d in range(3)], [lfine.inner[d] + 1 if d < nd else 1 for d in range(3)])
    for (cb, ce), (fb, fe) in ((whole_c, whole_f), (inner_c, inner_f)):
        for scale in (1.0, 4.0):
            want = coarse.copy()
            ORC.crestrict(lfine.c_struct(), fine, lc.c_struct(), want, scale, cb, ce)
            tf, tc = hip.from_host(fine.copy()), hip.from_host(coarse.copy())
            hip.crestrict(lfine.c_struct(), tf, lc.c_struct(), tc, scale, cb, ce)
            got = host(hip, tc)
            same_bits(got, want, "crestrict")
            same_bits(host(hip, tf), fine, "crestrict wrote its input")
            for part in (0, 1):
                rf, rc = hip.from_host(cases.deinterleave(fine)[part]), hip.from_host(cases.deinterleave(coarse)[part])
                hip.restrict(lfine.c_struct(), rf, lc.c_struct(), rc, scale, cb, ce)
                same_bits(cases.deinterleave(got)[part], host(hip, rc), "crestrict against examg_restrict on part %d" % part)
        want = fine.copy()
        ORC.cprolong_add(lc.c_struct(), coarse, lfine.c_struct(), want, fb, fe)
        tf, tc = hip.from_host(fine.copy()), hip.from_host(coarse.copy())
        hip.cprolong_add(lc.c_struct(), tc, lfine.c_struct(), tf, fb, fe)
        got = host(hip, tf)
        same_bits(got, want, "cprolong_add")
        same_bits(host(hip, tc), coarse, "cprolong_add wrote its input")
        for part in (0, 1):
            rf, rc = hip.from_host(cases.deinterleave(fine)[part]), hip.from_host(cases.deinterleave(coarse)[part])
            hip.prolong_add(lc.c_struct(), rc, lfine.c_struct(), rf, fb, fe)
            same_bits(cases.deinterleave(got)[part], host(hip, rf), "cprolong_add against examg_prolong_add on part %d" % part)


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_cdot_exact_on_integers_bounded_on_random_data_and_reproducible(hip, shape):
    nd, inner = cases.SHAPES[shape]
    lu, lf, ld = cases.layouts(nd, inner)
    for bname, (b, e) in cases.boxes(nd, inner).items():
        # integer-valued data: every product and every partial sum is an integer below 2^53 -- any order gives the Python integers
        x, y = cases.integer_field(lu, 91), cases.integer_field(lf, 92)
        re, im = ORC.cdot_terms(lu.c_struct(), x, lf.c_struct(), y, b, e)
        got = hip.complex_value(hip.cdot(lu.c_struct(), hip.from_host(x), lf.c_struct(), hip.from_host(y), b, e))
        assert (got.real, got.imag) == (float(sum(int(t) for t in re)), float(sum(int(t) for t in im))), (shape, bname)
        # random data: each part is a sum of 2 K rounded products in an order of the kernel's own; any order of n terms lies within
        # (n - 1) u sum|t| (1 + O(n u)) of the exact sum, u = 2^-53; (2 K + 1) u sum|t| is the bound tests/test_gpu_blas.py derives for examg_dot
        x, y = cases.random_field(lu, 93), cases.random_field(lf, 94)
        re, im = ORC.cdot_terms(lu.c_struct(), x, lf.c_struct(), y, b, e)
        K = re.size // 2
        tx, ty = hip.from_host(x), hip.from_host(y)
        got = host(hip, hip.cdot(lu.c_struct(), tx, lf.c_struct(), ty, b, e))
        for part, terms in ((0, re), (1, im)):
            exact, mag = cops.fsum_bound(terms)
            err = abs(got[part] - exact)
            print("%s %s part %d: K %d error %.3e bound %.3e" % (shape, bname, part, K, err, (2 * K + 1) * 2.0 ** -53 * mag))
            assert err <= (2 * K + 1) * 2.0 ** -53 * mag, (shape, bname, part)
        again = host(hip, hip.cdot(lu.c_struct(), tx, lf.c_struct(), ty, b, e))
        same_bits(again, got, "two calls of cdot")
        same_bits(host(hip, tx), x, "cdot wrote x")
    # an empty box gives (0, 0)
    out = hip.from_host(np.array([3.0, 4.0]))
    hip.cdot(lu.c_struct(), tx, lf.c_struct(), ty, b, [e[0], b[1], e[2]], out)
    assert host(hip, out).tolist() == [0.0, 0.0]


def test_a_large_dot_uses_every_stage_of_the_tree(hip):
    """More points than one pass of the grid covers: 2048 workgroups, several points per thread, the final workgroup sums 2048 partial sums."""
    lu = FieldLayout.node(2, (1500, 1500), 0)
    x, y = cases.integer_field(lu, 95, -3, 4), cases.integer_field(lu, 96, -3, 4)
    b, e = [0, 0, 0], [1501, 1501, 1]
    re, im = ORC.cdot_terms(lu.c_struct(), x, lu.c_struct(), y, b, e)
    got = hip.complex_value(hip.cdot(lu.c_struct(), hip.from_host(x), lu.c_struct(), hip.from_host(y), b, e))
    assert (got.real, got.imag) == (float(re.sum()), float(im.sum()))


def test_set_copy_and_pack_run_on_the_real_view(hip):
    """A complex field seen as a real field with every x count doubled: `set` to a real constant, a copy and pack / unpack are the real
    entry points on that view."""
    nd, inner = cases.SHAPES["2d_7x5"]
    lu = cases.layouts(nd, inner)[0].as_complex()
    rv = lu.real_view()
    b, e = cases.boxes(nd, inner)["interior"]
    rb, re_ = FieldLayout.real_view_box(b, e)
    x = cases.random_field(lu, 97)
    t = hip.from_host(x.copy())
    hip.set(rv.c_struct(), t, 0.0, rb, re_)
    want = x.copy()
    cops.cview(lu.c_struct(), want)[cops._sl(lu.c_struct(), b, e)] = 0.0
    same_bits(host(hip, t), want, "set on the real view")
    src, dst = hip.from_host(x.copy()), hip.from_host(cases.random_field(lu, 98))
    hip.axpby(rv.c_struct(), src, rv.c_struct(), dst, 1.0, 0.0, rb, re_)
    want = cases.random_field(lu, 98)
    cops.cview(lu.c_struct(), want)[cops._sl(lu.c_struct(), b, e)] = cops.cview(lu.c_struct(), x)[cops._sl(lu.c_struct(), b, e)]
    same_bits(host(hip, dst), want, "copy on the real view")
    n = 2 * (e[0] - b[0]) * (e[1] - b[1])
    buf, back = hip.new_array(n), hip.from_host(cases.random_field(lu, 99))
    hip.pack(rv.c_struct(), src, buf, rb, re_)
    hip.unpack(rv.c_struct(), back, buf, rb, re_)
    want = cases.random_field(lu, 99)
    cops.cview(lu.c_struct(), want)[cops._sl(lu.c_struct(), b, e)] = cops.cview(lu.c_struct(), x)[cops._sl(lu.c_struct(), b, e)]
    same_bits(host(hip, back), want, "pack / unpack on the real view")


def test_refusals_launch_nothing(hip):
    """Every refusal the header lists: non-zero with a text of its own, and the arrays keep their bits."""
    nd, inner = cases.SHAPES["2d_7x5"]
    lu, lf, ld = cases.layouts(nd, inner)
    b, e = cases.boxes(nd, inner)["interior"]
    st = cases.star_stencils(nd)["mp_shifted"]
    u, f, d = cases.random_field(lu, 101), cases.random_field(lf, 102), cases.random_field(ld, 103)
    tu, tf, td = hip.from_host(u), hip.from_host(f), hip.from_host(d)
    from exastencils_amd.field import Stencil

    def refused(text, fn, *args):
        with pytest.raises(ExamgError) as err:
            fn(*args)
        assert text in str(err.value), str(err.value)

    LU, LF, LD = lu.c_struct(), lf.c_struct(), ld.c_struct()
    SMALL = FieldLayout.node(nd, (4, 4), 0).c_struct()      # an allocation the box leaves
    refused("bad mode", hip.cstencil_op, 4, LU, tu, LF, tf, LD, td, st, 0.0, -1, b, e)
    refused("rhs required", hip.cstencil_op, cops.RESIDUAL, LU, tu, None, None, LD, td, st, 0.0, -1, b, e)
    refused("null argument", hip.cstencil_op, cops.APPLY, LU, tu, None, None, LD, None, st, 0.0, -1, b, e)
    field = Stencil(st.offsets, [c.real for c in st.coefs], cfield=tu, clayout=lu)
    refused("stencil fields", hip.cstencil_op, cops.APPLY, LU, tu, None, None, LD, td, field, 0.0, -1, b, e)
    refused("layout transformation", hip.cstencil_op, cops.APPLY, lu.split_x().c_struct(), tu, None, None, LD, td, st, 0.0, -1, b, e)
    refused("layout transformation", hip.cstencil_op, cops.APPLY, LU, tu, None, None, ld.split_x().c_struct(), td, st, 0.0, -1, b, e)
    l1 = FieldLayout(1, (7, 1, 1), (1, 0, 0), (1, 0, 0)).c_struct()
    refused("not 2-D or 3-D", hip.cstencil_op, cops.APPLY, l1, tu, None, None, l1, td, st, 0.0, -1, [1, 0, 0], [3, 1, 1])
    refused("outside {-1, 0, 1}", hip.cstencil_op, cops.APPLY, LU, tu, None, None, LD, td, Stencil([(0, 0, 0), (2, 0, 0)], [1.0, 1.0]), 0.0, -1, b, e)
    refused("dimension the layouts do not have", hip.cstencil_op, cops.APPLY, LU, tu, None, None, LD, td, Stencil([(0, 0, 0), (0, 0, 1)], [1.0, 1.0]), 0.0,
            -1, b, e)
    refused("16-byte aligned", hip.cstencil_op, cops.APPLY, LU, tu[1:], None, None, LD, td, st, 0.0, -1, b, e)
    refused("leaves the u allocation", hip.cstencil_op, cops.APPLY, LU, tu, None, None, LD, td, st, 0.0, -1, [-1, 0, 0], [inner[0] + 3, 2, 1])
    refused("leaves the dst allocation", hip.cstencil_op, cops.APPLY, LU, tu, None, None, SMALL, td, st, 0.0, -1, b, e)
    refused("leaves the rhs allocation", hip.cstencil_op, cops.RESIDUAL, LU, tu, SMALL, tf, LD, td, st, 0.0, -1, b, e)
    refused("needs a colour", hip.cstencil_op, cops.CRELAX, LU, tu, LF, tf, None, None, st, 0.6, -1, b, e)
    refused("real relaxation weight", hip.cstencil_op, cops.CRELAX, LU, tu, LF, tf, None, None, st, 0.6 + 0.1j, 0, b, e)
    refused("dst must be u", hip.cstencil_op, cops.CRELAX, LU, tu, LF, tf, LD, td, st, 0.6, 0, b, e)
    full = cases.gather_stencils(nd)["full"]      # its diagonal entries reach points of the same colour
    refused("u and dst alias", hip.cstencil_op, cops.SMOOTH, LU, tu, LF, tf, LU, tu, st, 0.1, -1, b, e)
    refused("u and dst alias", hip.cstencil_op, cops.SMOOTH, LU, tu, LF, tf, LU, tu, full, 0.1, 0, b, e)
    refused("all reach the other colour", hip.cstencil_op, cops.CRELAX, LU, tu, LF, tf, None, None, full, 0.6, 0, b, e)
    assert hip.cstencil_route(4, LU, tu, LF, tf, LD, td, st, 0.0, -1, b, e) == -1 and b"bad mode" in hip.L.examg_last_error()

    a = 0.5 + 0.5j
    refused("unknown form", hip.clincomb, 3, LU, tu, LF, tf, None, None, LD, td, a, None, b, e)
    refused("needs z and b", hip.clincomb, cops.C_XPAYMBZ, LU, tu, LF, tf, None, None, LD, td, a, None, b, e)
    refused("layout transformation", hip.clincomb, cops.C_XPAY, lu.split_x().c_struct(), tu, LF, tf, None, None, LD, td, a, None, b, e)
    refused("16-byte aligned", hip.clincomb, cops.C_XPAY, LU, tu, LF, tf[1:], None, None, LD, td, a, None, b, e)
    refused("leaves the y allocation", hip.clincomb, cops.C_XPAY, LU, tu, SMALL, tf, None, None, LD, td, a, None, b, e)
    refused("leaves the y allocation", hip.cdot, LU, tu, SMALL, tf, b, e)
    refused("layout transformation", hip.cdot, lu.split_x().c_struct(), tu, LF, tf, b, e)

    lfine, lc = cases.transfer_layouts(2, (3, 2, 1))
    tfi, tco = hip.from_host(cases.random_field(lfine, 104)), hip.from_host(cases.random_field(lc, 105))
    refused("leaves the coarse allocation", hip.crestrict, lfine.c_struct(), tfi, lc.c_struct(), tco, 1.0, [0, 0, 0], [9, 3, 1])
    refused("fine footprint", hip.crestrict, FieldLayout.node(2, (8, 6), 0).c_struct(), tfi, lc.c_struct(), tco, 1.0, [0, 0, 0], [5, 4, 1])
    refused("layout transformation", hip.crestrict, lfine.split_x().c_struct(), tfi, lc.c_struct(), tco, 1.0, [1, 1, 0], [4, 3, 1])
    refused("leaves the fine allocation", hip.cprolong_add, lc.c_struct(), tco, lfine.c_struct(), tfi, [0, 0, 0], [11, 7, 1])
    refused("negative fine index", hip.cprolong_add, lc.c_struct(), tco, lfine.c_struct(), tfi, [-1, 0, 0], [3, 3, 1])
    refused("coarse footprint", hip.cprolong_add, FieldLayout.node(2, (2, 2), 0).c_struct(), tco, lfine.c_struct(), tfi, [0, 0, 0], [9, 7, 1])

    refused("overlaps its own shifted image", hip.cshift_div, LU, tu, (1, 0, 0), a, [0, 0, 0], [2, 3, 1])
    refused("overlaps its own shifted image", hip.cshift_div, LU, tu, (0, 0, 0), a, [0, 0, 0], [1, 3, 1])
    refused("shifted box leaves", hip.cshift_div, LU, tu, (-2, 0, 0), a, [0, 0, 0], [1, 3, 1])
    refused("dimension the layout does not have", hip.cshift_div, LU, tu, (0, 0, 1), a, [0, 0, 0], [1, 3, 1])
    lre = FieldLayout.node(nd, (8, 6), 0)
    tre = hip.from_host(np.zeros(lre.size))
    refused("leaves the re allocation", hip.cfrom_parts, LU, tu, SMALL, tre, None, None, b, e)
    refused("different dimensionality", hip.cfrom_parts, LU, tu, FieldLayout.node(3, (8, 6, 2), 0).c_struct(), tre, None, None, b, e)
    refused("leaves the dst allocation", hip.cfrom_parts, SMALL, td, lre.c_struct(), tre, None, None, b, e)

    for t, x, name in ((tu, u, "u"), (tf, f, "rhs"), (td, d, "dst")):
        same_bits(host(hip, t), x, "a refused call wrote " + name)


@pytest.mark.parametrize("nd,n", [(2, 1024), (3, 128)], ids=["1024x1024", "128x128x128"])
def test_the_default_route_of_a_large_box_marches_and_gives_numpys_bits(hip, nd, n):
    """10^6 points and more: the product library takes the marching kernel with the run lengths of its own (many windows per row, many runs
    per column) -- the sizes at which the route and the launch geometry are not those of the small cases."""
    lu, lf = FieldLayout.node(nd, (n,) * nd, 1), FieldLayout.node(nd, (n,) * nd, 0)
    b, e = [1 if d < nd else 0 for d in range(3)], [n if d < nd else 1 for d in range(3)]
    st = cases.star_stencils(nd)["pm_shifted"]
    u, f, d = cases.random_field(lu, 121), cases.random_field(lf, 122), cases.random_field(lf, 123)
    for mode, w in ((cops.RESIDUAL, 0.0), (cops.SMOOTH, 0.8 / st.coefs[0])):
        tu, tf, td = hip.from_host(u), hip.from_host(f), hip.from_host(d.copy())
        assert hip.cstencil_route(mode, lu.c_struct(), tu, lf.c_struct(), tf, lf.c_struct(), td, st, w, -1, b, e) == lib.CSTENCIL_MARCH
        hip.cstencil_op(mode, lu.c_struct(), tu, lf.c_struct(), tf, lf.c_struct(), td, st, w, -1, b, e)
        want = d.copy()
        ORC.cstencil_op(mode, lu.c_struct(), u, lf.c_struct(), f, lf.c_struct(), want, st, w, -1, b, e)
        same_bits(host(hip, td), want, "%d-D n %d mode %d" % (nd, n, mode))
        same_bits(host(hip, tu), u, "u was written")


# -- the programs of examples/exa4/ through the interpreter on the kernels ---------------------------------------------------------------------
def _program(name, ops, **kw):
    import os

    from exastencils_amd import exa4

    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "exa4")
    return exa4.load(os.path.join(ex, name + ".exa4"), os.path.join(ex, name + ".knowledge"), ops=ops, **kw)


@pytest.mark.parametrize("name,start", [("helmholtz2d_complex", 1024.0), ("helmholtz3d_complex", 4096.0)], ids=["2d", "3d"])
def test_the_own_program_prints_the_restatements_residuals(hip, name, start):
    """The outer loop capped at 3 iterations (levels 3..5 with k = 20 in 2-D, 2..4 with k = 10 in 3-D): the residuals the interpreter prints
    on the GPU against those it prints on the restatement with numpy's order of the dot products.  Everything but the dot products is
    bit-equal; the tolerance is what the ORDER of a dot product moves a residual by, measured on the CPU at these steps (the largest
    relative spread between numpy's pairwise order, the reversed array and a sequential sum: 9.9e-14 in 2-D, 1.7e-14 in 3-D), times
    100: the GPU's tree is a fourth order.  At six iterations the spread is 5e-06 in 2-D -- an indefinite BiCGStab amplifies the last bit
    of every dot product; hence the cap."""
    from tests.test_complex_exa4 import capped_residuals

    want, spread = capped_residuals(name, 3)
    P = _program(name, hip, auto_graph=False)
    P.globals["maxIt"] = 3
    P.run()
    got = np.array(P.printed_values[1:4])
    rel = np.abs(got - want) / np.abs(want)
    print("%s: CPU spread %.3e, GPU against numpy %s" % (name, spread, rel))
    assert P.printed_values[0] == start
    assert len(got) == 3 and spread > 0.0 and np.all(rel <= 100.0 * spread), (rel, spread)


def test_the_2d_program_converges_on_the_gpu(hip):
    P = _program("helmholtz2d_complex", hip)
    P.run()
    print(P.out[-1], "-- %d launches, %d graph replays" % (P.launches, P.graph_replays))
    assert P.out[-1].startswith("Residual after") and int(P.out[-1].split()[2]) + 1 <= 2 * 41


def test_a_graph_replay_of_the_smoothers_leaves_the_bits_of_interpretation(hip):
    """auto_graph: PreSmoother@5 / PostSmoother@5 (local solves and their boundary functions, no host value) are recorded into a hipGraph at
    their second call and replayed from then on; the residuals and the solution have the bits of the statement-by-statement run."""
    runs = []
    for graph in (False, True):
        P = _program("helmholtz2d_complex", hip, auto_graph=graph)
        P.globals["maxIt"] = 3
        P.run()
        runs.append(P)
    plain, G = runs
    assert G.auto_graph and G.graph_replays >= 4 and G._auto_graphs[("PreSmoother", 5)]["replays"] >= 1
    assert G.printed_values == plain.printed_values
    same_bits(host(hip, G.fields[("Solution", 5)].data()), host(hip, plain.fields[("Solution", 5)].data()), "Solution after graph replays")
