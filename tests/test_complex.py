"""Complex-valued node fields on the CPU: the numpy restatement tests/complex_ops.py against independent forms (numpy complex128, the real
oracle on the parts), the data model, the C ABI mirror and the registers of the kernels."""
import os
import re
import subprocess

import numpy as np
import pytest

from exastencils_amd.field import Field
from exastencils_amd.layout import FieldLayout
from tests import complex_cases as cases
from tests import complex_ops as cops

OPS = cops.ComplexOps()


def _as_complex(layout, a):
    return cops.cview(layout.c_struct(), a)[..., 0] + 1j * cops.cview(layout.c_struct(), a)[..., 1]


def _box_index(layout, begin, end, off=(0, 0, 0)):
    return cops._sl(layout.c_struct(), begin, end, off)


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_apply_agrees_with_complex128(shape):
    """dst = A u on the parts against numpy's own complex arithmetic: 1e-14 of the sum of the magnitudes of the products."""
    nd, inner = cases.SHAPES[shape]
    lu, lf, ld = cases.layouts(nd, inner)
    u = cases.random_field(lu, 1)
    stencils = dict(cases.star_stencils(nd), **cases.gather_stencils(nd))
    for bname, (b, e) in cases.boxes(nd, inner).items():
        for sname, st in stencils.items():
            dst = cases.random_field(ld, 2)
            OPS.cstencil_op(cops.APPLY, lu.c_struct(), u, None, None, ld.c_struct(), dst, st, 0.0, -1, b, e)
            U = _as_complex(lu, u)
            want = sum(c * U[_box_index(lu, b, e, o)] for o, c in zip(st.offsets, st.coefs))
            scale = sum(abs(c) * np.abs(U[_box_index(lu, b, e, o)]) for o, c in zip(st.offsets, st.coefs))
            got = _as_complex(ld, dst)[_box_index(ld, b, e)]
            assert np.all(np.abs(got - want) <= 1e-14 * scale), (shape, bname, sname)


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_residual_and_smooth_agree_with_complex128(shape):
    nd, inner = cases.SHAPES[shape]
    lu, lf, ld = cases.layouts(nd, inner)
    u, f = cases.random_field(lu, 3), cases.random_field(lf, 4)
    w = 0.37 - 0.21j
    b, e = cases.boxes(nd, inner)["interior"]
    for sname, st in cases.star_stencils(nd).items():
        U, F = _as_complex(lu, u), _as_complex(lf, f)
        conv = sum(c * U[_box_index(lu, b, e, o)] for o, c in zip(st.offsets, st.coefs))
        scale = sum(abs(c) * np.abs(U[_box_index(lu, b, e, o)]) for o, c in zip(st.offsets, st.coefs)) + 1.0
        for mode, want in ((cops.RESIDUAL, F[_box_index(lf, b, e)] - conv),
                           (cops.SMOOTH, U[_box_index(lu, b, e)] + w * (F[_box_index(lf, b, e)] - conv))):
            dst = cases.random_field(ld, 5)
            OPS.cstencil_op(mode, lu.c_struct(), u, lf.c_struct(), f, ld.c_struct(), dst, st, w, -1, b, e)
            got = _as_complex(ld, dst)[_box_index(ld, b, e)]
            assert np.all(np.abs(got - want) <= 4e-14 * scale), (shape, sname, mode)


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_crelax_solves_the_colour_and_keeps_the_other(shape):
    """After the local solves of one colour with relax 1.0 the residual at the colour's points is at most 1e-12 max|f|; the points of the
    other colour and everything outside the box keep their bits.  f has the size of A u (the centre coefficient's magnitude)."""
    nd, inner = cases.SHAPES[shape]
    lu, lf, ld = cases.layouts(nd, inner)
    b, e = cases.boxes(nd, inner)["interior"]
    for sname, st in cases.star_stencils(nd).items():
        centre = abs(st.coefs[st.offsets.index((0, 0, 0))])
        for colour in (0, 1):
            u, f = cases.random_field(lu, 6), cases.random_field(lf, 7) * centre
            before = u.copy()
            OPS.cstencil_op(cops.CRELAX, lu.c_struct(), u, lf.c_struct(), f, None, None, st, 1.0, colour, b, e)
            res = cases.random_field(ld, 8)
            OPS.cstencil_op(cops.RESIDUAL, lu.c_struct(), u, lf.c_struct(), f, ld.c_struct(), res, st, 0.0, -1, b, e)
            m = cops.colour_mask(b, e, colour)
            R = _as_complex(ld, res)[_box_index(ld, b, e)]
            assert np.abs(R[m]).max() <= 1e-12 * np.abs(f).max(), (shape, sname, colour)
            changed = cops.cview(lu.c_struct(), u) != cops.cview(lu.c_struct(), before)
            inside = np.zeros(changed.shape[:3], dtype=bool)
            inside[_box_index(lu, b, e)] = m
            assert not changed[~inside].any()
            assert changed[inside].any()


def test_crelax_underrelaxation_is_the_convex_form():
    nd, inner = cases.SHAPES["2d_7x5"]
    lu, lf, ld = cases.layouts(nd, inner)
    b, e = cases.boxes(nd, inner)["interior"]
    st = cases.star_stencils(nd)["mp_shifted"]
    u, f = cases.random_field(lu, 9), cases.random_field(lf, 10)
    full, part = u.copy(), u.copy()
    OPS.cstencil_op(cops.CRELAX, lu.c_struct(), full, lf.c_struct(), f, None, None, st, 1.0, 0, b, e)
    OPS.cstencil_op(cops.CRELAX, lu.c_struct(), part, lf.c_struct(), f, None, None, st, 0.6, 0, b, e)
    solved = full != u
    assert solved.any() and np.array_equal(part[~solved], u[~solved])
    assert np.array_equal(part[solved], (u * (1.0 - 0.6) + 0.6 * full)[solved])


@pytest.mark.parametrize("nd,inner_coarse", [(2, (3, 2, 1)), (3, (3, 2, 2)), (2, (33, 4, 1))])
def test_transfers_are_the_real_oracle_on_the_parts(nd, inner_coarse):
    """Bit for bit: the complex restriction and prolongation are the real ones (the C oracle) on the de-interleaved parts."""
    from tests.oracle_ops import OracleOps
    import torch

    orc = OracleOps()
    lfine, lc = cases.transfer_layouts(nd, inner_coarse)
    cb, ce = [1 if d < nd else 0 for d in range(3)], [inner_coarse[d] + 1 if d < nd else 1 for d in range(3)]
    fb, fe = [1 if d < nd else 0 for d in range(3)], [lfine.inner[d] + 1 if d < nd else 1 for d in range(3)]
    fine, coarse = cases.random_field(lfine, 11), cases.random_field(lc, 12)

    got = coarse.copy()
    OPS.crestrict(lfine.c_struct(), fine, lc.c_struct(), got, 4.0, cb, ce)
    for part in (0, 1):
        want = torch.from_numpy(cases.deinterleave(coarse)[part].copy())
        orc.restrict(lfine.c_struct(), torch.from_numpy(cases.deinterleave(fine)[part]), lc.c_struct(), want, 4.0, cb, ce)
        assert np.array_equal(cases.deinterleave(got)[part], want.numpy())

    got = fine.copy()
    OPS.cprolong_add(lc.c_struct(), coarse, lfine.c_struct(), got, fb, fe)
    for part in (0, 1):
        want = torch.from_numpy(cases.deinterleave(fine)[part].copy())
        orc.prolong_add(lc.c_struct(), torch.from_numpy(cases.deinterleave(coarse)[part]), lfine.c_struct(), want, fb, fe)
        assert np.array_equal(cases.deinterleave(got)[part], want.numpy())


def test_lincomb_dot_shift_and_parts_against_complex128():
    nd, inner = cases.SHAPES["3d_5x4x3"]
    lu, lf, ld = cases.layouts(nd, inner)
    b, e = cases.boxes(nd, inner)["whole"]
    x, y, z = cases.random_field(lu, 13), cases.random_field(lf, 14), cases.random_field(ld, 15)
    X, Y, Z = (_as_complex(l, a)[_box_index(l, b, e)] for l, a in ((lu, x), (lf, y), (ld, z)))
    a, bb = 0.3 - 1.1j, -0.8 + 0.25j
    for form, want in ((cops.C_XPAY, X + a * Y), (cops.C_XMAY, X - a * Y), (cops.C_XPAYMBZ, X + a * (Y - bb * Z))):
        dst = cases.random_field(lu, 16)
        OPS.clincomb(form, lu.c_struct(), x, lf.c_struct(), y, ld.c_struct(), z, lu.c_struct(), dst, a, bb, b, e)
        assert np.allclose(_as_complex(lu, dst)[_box_index(lu, b, e)], want, rtol=0, atol=1e-14)
    # dst may be any operand
    for alias in (0, 1, 2):
        ops_in = [x.copy(), y.copy(), z.copy()]
        lay = (lu, lf, ld)
        OPS.clincomb(cops.C_XPAYMBZ, lu.c_struct(), ops_in[0], lf.c_struct(), ops_in[1], ld.c_struct(), ops_in[2], lay[alias].c_struct(), ops_in[alias],
                     a, bb, b, e)
        assert np.allclose(_as_complex(lay[alias], ops_in[alias])[_box_index(lay[alias], b, e)], X + a * (Y - bb * Z), rtol=0, atol=1e-14)
    # the unconjugated dot
    d = OPS.complex_value(OPS.cdot(lu.c_struct(), x, lf.c_struct(), y, b, e))
    assert abs(d - np.sum(X * Y)) <= 1e-13
    for order in ("reversed", "sequential"):
        d2 = cops.ComplexOps(order)
        assert abs(d2.complex_value(d2.cdot(lu.c_struct(), x, lf.c_struct(), y, b, e)) - d) <= 1e-13
    # the absorbing-boundary assignment: the lower x plane from its neighbour
    c = 1.0 - 1j * 20.0 * 0.03125
    pb, pe = [0, 0, 0], [1, e[1], e[2]]
    xx = x.copy()
    OPS.cshift_div(lu.c_struct(), xx, (1, 0, 0), c, pb, pe)
    assert np.allclose(_as_complex(lu, xx)[_box_index(lu, pb, pe)], _as_complex(lu, x)[_box_index(lu, pb, pe, (1, 0, 0))] / c, rtol=0, atol=1e-15)
    assert np.array_equal(_as_complex(lu, xx)[_box_index(lu, [1, 0, 0], e)], _as_complex(lu, x)[_box_index(lu, [1, 0, 0], e)])
    # from real parts
    lr = FieldLayout.node(nd, tuple(inner[d] + 1 for d in range(nd)), 0)
    re = np.random.default_rng(17).uniform(-1, 1, lr.size)
    dst = cases.random_field(lu, 18)
    OPS.cfrom_parts(lu.c_struct(), dst, lr.c_struct(), re, None, None, b, e)
    assert np.array_equal(_as_complex(lu, dst)[_box_index(lu, b, e)], cops.rview(lr.c_struct(), re)[_box_index(lr, b, e)] + 0j)


# -- the data model ---------------------------------------------------------------------------------------------------------------------------
def test_a_complex_layout_counts_points_and_its_real_view_doubles_x():
    lu = FieldLayout.node(2, (8, 6), 1).as_complex()
    assert lu.is_complex and lu.doubles == 2 * lu.size
    assert lu.c_struct().inner[0] == 7          # examg_layout_t is unchanged: counts in points
    rv = lu.real_view()
    assert not rv.is_complex and rv.size == lu.doubles and rv.tot(0) == 2 * lu.tot(0) and rv.tot(1) == lu.tot(1)
    # the real and the imaginary part of point i are the points 2 i and 2 i + 1 of the view
    for i in (-1, 0, 3, 8):
        assert rv.linear(2 * i, 2) == 2 * lu.linear(i, 2) and rv.linear(2 * i + 1, 2) == 2 * lu.linear(i, 2) + 1
    assert FieldLayout.real_view_box([1, 2, 0], [5, 4, 1]) == ([2, 2, 0], [10, 4, 1])
    with pytest.raises(ValueError):
        FieldLayout.cell(2, (8, 6), 1).as_complex()
    with pytest.raises(ValueError):
        FieldLayout.node(2, (8, 6), 1).split_x().as_complex()


def test_a_field_of_a_complex_layout_allocates_twice_the_doubles():
    lu = FieldLayout.node(3, (4, 4, 4), 1)
    assert len(Field("u", 2, lu.as_complex(), OPS).data()) == 2 * lu.size
    assert len(Field("u", 2, lu, OPS).data()) == lu.size


# -- the C ABI mirror ----------------------------------------------------------------------------------------------------------------------------
def test_every_complex_entry_point_is_declared_mirrored_and_wrapped():
    from exastencils_amd import lib
    from exastencils_amd.ops import HipOps

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "examg.h")).read()
    names = ["examg_cstencil_op", "examg_cstencil_route", "examg_clincomb", "examg_cdot", "examg_crestrict", "examg_cprolong_add",
             "examg_cshift_div", "examg_cfrom_parts"]
    L = lib.load()
    for n in names:
        assert re.search(r"\bint %s\(" % n, header) and n in lib.SYMBOLS
        assert getattr(L, n).argtypes, n
        assert hasattr(HipOps, n[len("examg_"):]), n
        assert hasattr(cops.ComplexOps, n[len("examg_"):]) or n == "examg_cstencil_route", n      # the route is a question about the kernels
    assert (lib.CRELAX, lib.CSTENCIL_GATHER, lib.CSTENCIL_MARCH) == (3, 1, 2) and "EXAMG_CRELAX 3" in header
    assert not hasattr(L, "examg_debug_cstencil_route")
    assert hasattr(lib.load(lib.DBG_LIB_PATH), "examg_debug_cstencil_route")


# -- the kernels' registers -------------------------------------------------------------------------------------------------------------------
def test_the_complex_kernels_use_no_scratch(tmp_path):
    """The marching kernel selects an entry's point among named registers: kernels_complex.hip, compiled for the device with the flags of the
    build, reports private segment 0 and no VGPR spill for every kernel."""
    import __graft_entry__ as ge

    out = str(tmp_path / "complex.s")
    flags = [f for f in ge.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([os.environ.get("HIPCC", "hipcc")] + flags + ["--cuda-device-only", "-S", os.path.join(ge.CSRC, "kernels_complex.hip"), "-o", out],
                   check=True, capture_output=True)
    with open(out) as f:
        meta = f.read().split("amdhsa.kernels:")[1]
    kernels = re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", meta)
    names = " ".join(k[0] for k in kernels)
    for want in ("k_cstencil_march", "k_cstencil_gather", "k_clincomb", "k_cdot_partial", "k_crestrict", "k_cprolong_add", "k_cshift_div", "k_cfrom_parts"):
        assert want in names
    assert len(kernels) >= 23
    assert all(int(seg) == 0 and int(spill) == 0 for _, seg, spill in kernels), kernels
