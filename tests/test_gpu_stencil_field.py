"""Stencil fields (variable coefficients) on every kernel that takes them, and every argument of the stencil loops in a layout of
its own.  Each case runs twice, as tests/test_gpu_stencil_asym.py does for constant stencils:

  (a) random data (coefficients of both signs off the diagonal), compared bit for bit with the oracle's loops over whole arrays,
      the inputs and the coefficient array included;
  (b) exact data (coefficients k / 4 that differ at every point and entry, the diagonal from {4, 8, 16}), compared with equality
      against the exact reference of tests/stencil_cases.py -- independent of the summation order.

All arrays are filled over their whole allocation, and in the 'own' layout sets u, rhs, the destination and the coefficient field
differ in ghost width (2 / 0 / 1 / 1) and alignment (0 / 2 / 4 / 16): an index formed with another argument's layout reads or writes
another point.  Every case names the kernel it pins (PINS at the end lists them); where the library offers an eligibility query the
path is asserted through it, the variants without a query are forced through the debug build's hooks.  The kernel of an
examg_stencil_op call is asked of the debug build (stencil_route: with no hook set, the product library's route)."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import stencil_cases as S
from oracle_ops import OracleOps
from stencil_cases import APPLY, RESIDUAL, SMOOTH, ExactOps
from test_gpu_kernels import hip, hip3, hipd  # noqa: F401  (fixtures)
from test_gpu_stencil_asym import _boxes2, _expected_outside, _sweep_run, _three_run, assert_same, box, host, stencil_route

from exastencils_amd.layout import FieldLayout

pytestmark = pytest.mark.gpu

DATA = ["random", "exact"]
OMEGA = 0.713                 # smoother weight of the random runs (stencil fields: w = omega, divided by the diagonal per point)


@pytest.fixture(scope="module")
def orc():
    return OracleOps()


@pytest.fixture(scope="module")
def ex():
    return ExactOps()


def ref_ops(data, orc, ex):
    return ex if data == "exact" else orc


def weight(data):
    return S.EXACT_W if data == "exact" else OMEGA


def layouts(nd, shape, lay):
    """(u, rhs, destination, coefficient) layouts.  'same': what the older tests pass (destination = u layout, coefficients in the
    rhs layout object); 'own' / 'own2': four different layouts."""
    if lay == "same":
        lu, lf = FieldLayout.node(nd, shape, 1), FieldLayout.node(nd, shape, 0, True, False)
        return lu, lf, lu, lf
    if lay == "own":
        return (FieldLayout.node(nd, shape, 2), FieldLayout.node(nd, shape, 0, True, False, 2), FieldLayout.node(nd, shape, 1, align=4),
                FieldLayout.node(nd, shape, 1, align=16))
    assert lay == "own2"
    return (FieldLayout.node(nd, shape, 1, align=16), FieldLayout.node(nd, shape, 1), FieldLayout.node(nd, shape, 2, align=2),
            FieldLayout.node(nd, shape, 0, align=8))


def test_the_distinct_layouts_are_distinct():
    for nd, shape in ((3, (65, 21, 9)), (2, (80, 33, 0))):
        for lay in ("own", "own2"):
            L = [S._Lay(l) for l in layouts(nd, shape, lay)]
            assert len({(tuple(x.tot), tuple(x.ref)) for x in L}) == 4 and len({x.tot[0] for x in L}) == 4


# -- examg_stencil_op ------------------------------------------------------------------------------------------------------------------
MODES = [(APPLY, -1, 0), (RESIDUAL, -1, 0), (SMOOTH, -1, 0)]
# the generic kernel also takes `omega / diag(A)` and colour loops (in place for the stars, out of place for 27 entries)
MODES_GENERIC = MODES + [(SMOOTH, -1, 1), (SMOOTH, 0, 1), (SMOOTH, 1, 0)]


def _op_run(ops, nd, shape, lay, kind, data, mode, colour, wform, b, e, entry_fastest=False, route=None):
    """One examg_stencil_op; returns [u, rhs, destination, coefficient planes] (+ the transformed coefficient array).
    route = (debug build, name or function of (mode, colour, wform)): the kernel the call must take, asserted before it runs."""
    lu, lf, ld, lc = layouts(nd, shape, lay)
    st = S.stencil_field(ops, S.field_offsets(kind), lc, data, 900, wform)
    u, f, d = (S.data_field(ops, l.size, data, 901 + i) for i, l in enumerate((lu, lf, ld)))
    call = st.entry_fastest(ops) if entry_fastest else st
    assert call.ctransform == (1 if entry_fastest else 0)
    in_place = colour >= 0 and S.is_star(st)
    if route is not None:
        hipd, want = route
        want = want if isinstance(want, str) else want(mode, colour, wform)
        assert stencil_route(hipd, mode, lu, lf, lu if in_place else ld, call, colour, b, e, in_place) == want, (kind, mode, colour, wform)
    if in_place:
        ops.stencil_op(mode, lu.c_struct(), u, lf.c_struct(), f, lu.c_struct(), u, call, weight(data), colour, b, e)
    else:
        ops.stencil_op(mode, lu.c_struct(), u, lf.c_struct(), f, ld.c_struct(), d, call, weight(data), colour, b, e)
    return [u, f, d, st.cfield] + ([call.cfield] if entry_fastest else [])


def check_op(gpu, orc, ex, nd, shape, lay, kind, which, data, modes, entry_fastest=False, b=None, e=None, what="", route=None):
    if b is None:
        b, e = box(nd, shape, which)
    R = ref_ops(data, orc, ex)
    for mode, colour, wform in modes:
        got = host(gpu, _op_run(gpu, nd, shape, lay, kind, data, mode, colour, wform, b, e, entry_fastest, route))
        want = host(R, _op_run(R, nd, shape, lay, kind, data, mode, colour, wform, b, e))
        if entry_fastest:          # `[x, y, z, i] => [i, x, y, z]` of the same values, untouched by the loop
            K = len(S.field_offsets(kind))
            assert np.array_equal(got.pop().reshape(-1, K), want[3].reshape(K, -1).T)
        assert_same(got, want, "%s %s %s %s %s, mode %d colour %d wform %d" % (what, kind, lay, which, data, mode, colour, wform))


# rows of 64 points (the lowest the kernel takes), 65, 130 and 129 (two and three tiles of 128, ragged and odd); 9 and 21 rows: tiles of
# 8 rows with one and five rows left over
ZM7_CASES = [((65, 21, 9), "own", "inner"), ((65, 10, 6), "same", "dup"), ((66, 12, 7), "own2", "inner"), ((131, 14, 9), "own", "inner"),
             ((131, 10, 6), "own", "dup"), ((134, 12, 21), "own2", "odd"), ((130, 9, 18), "same", "inner")]


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("shape,lay,which", ZM7_CASES, ids=["%d-%s-%s" % (c[0][0], c[1], c[2]) for c in ZM7_CASES])
def test_stencilfield7_zmarch(hip, hipd, orc, ex, shape, lay, which, data):
    """pins k_stencilfield7_zmarch<., 2, 4, 0> (the product's variant): 7 entries in the reference's order, rows of at least 64 points,
    `(1.0 / diag) * omega`."""
    check_op(hip, orc, ex, 3, shape, lay, "vc7", which, data, MODES, what="z-march", route=(hipd, "field7"))


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("variant,blocks", [(0, -1), (2, 7), (3, 40), (1, 3)], ids=["ry1pf1", "ry2pf1-7wg", "ry1pf2-40wg", "ry2pf0-3wg"])
def test_stencilfield7_zmarch_variants(hipd, orc, ex, variant, blocks, data):
    """pins k_stencilfield7_zmarch<., 1, 4, 1>, <., 2, 4, 1>, <., 1, 4, 2> and the product's <., 2, 4, 0> with a forced workgroup
    count (z chunks of 16 planes at least: 37 planes make chunks of 16, 16 and 5), through examg_debug_stencilfield."""
    hipd.L.examg_debug_stencilfield.argtypes = [C.c_int, C.c_int]
    hipd.L.examg_debug_stencilfield(variant, blocks)
    try:
        check_op(hipd, orc, ex, 3, (131, 11, 38), "own", "vc7", "inner", data, MODES, what="z-march variant %d" % variant)
        check_op(hipd, orc, ex, 3, (65, 9, 6), "own2", "vc7", "dup", data, MODES, what="z-march variant %d" % variant)
    finally:
        hipd.L.examg_debug_stencilfield(1, -1)


SF27_CASES = [((70, 20, 12), "own", "inner"), ((40, 12, 9), "same", "dup"), ((66, 14, 10), "own2", "odd"), ((130, 9, 6), "own", "dup")]


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("shape,lay,which", SF27_CASES, ids=["%d-%s-%s" % (c[0][0], c[1], c[2]) for c in SF27_CASES])
def test_stencilfield27_unrolled(hip, hipd, orc, ex, shape, lay, which, data):
    """pins k_stencilfield_unrolled<., 27>: 27 entries in planes, the centre first, `(1.0 / diag) * omega`, no colour; the product
    library and the debug build with the unrolled kernel switched on (examg_debug_sf27(1))."""
    check_op(hip, orc, ex, 3, shape, lay, "h27", which, data, MODES, what="unrolled", route=(hipd, "field27_planes"))
    hipd.L.examg_debug_sf27(1)
    check_op(hipd, orc, ex, 3, shape, lay, "h27", which, data, MODES, what="unrolled (debug build)", route=(hipd, "field27_planes"))


def _holds_last_point(lc, b, e):
    """Does the box hold the last allocated point of the coefficient layout?  (The record kernel's clamped 16-byte loads would shift
    that point's last entry: the dispatch leaves such a box to the generic kernel.)"""
    L = S._Lay(lc)
    return all(s.stop == t for s, t in zip(L.box(b, e), L.shape))


# tiles of 64 points: 1 x 7 x 7 = 49 and 3 x 5 x 3 = 45 tiles (1 mod 4: the last wave of runs of 2 and of 4 holds one tile), and
# boxes with other tile counts
REC_CASES = [((41, 8, 8), "own", "inner"), ((131, 6, 4), "own2", "inner"), ((70, 13, 9), "own", "odd"), ((66, 9, 5), "same", "inner"),
             ((66, 9, 5), "own", "dup")]


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("run", [1, 2, 4])
@pytest.mark.parametrize("shape,lay,which", REC_CASES, ids=["%d-%s-%s" % (c[0][0], c[1], c[2]) for c in REC_CASES])
def test_stencilfield27_records(hipd, orc, ex, shape, lay, which, run, data):
    """pins k_stencilfield27_rec: 27 entries entry-fastest (one 216-byte record per point), 1, 2 and 4 tiles per wave
    (examg_debug_sf27_run)."""
    b, e = box(3, shape, which)
    assert not _holds_last_point(layouts(3, shape, lay)[3], b, e)
    hipd.L.examg_debug_sf27_run(run)
    try:
        check_op(hipd, orc, ex, 3, shape, lay, "h27", which, data, MODES, entry_fastest=True, what="records, run %d" % run,
                 route=(hipd, "field27_rec"))
    finally:
        hipd.L.examg_debug_sf27_run(0)


@pytest.mark.parametrize("data", DATA)
def test_stencilfield27_records_product_and_last_point(hip, hipd, orc, ex, data):
    """pins k_stencilfield27_rec as the product library launches it, and the dispatch bound beside it: a box that holds the LAST
    allocated point of a coefficient layout without ghost or pad layers must give the right result (the record kernel's clamped
    16-byte loads would shift that point's last entry: the dispatch leaves the box to k_stencil_generic)."""
    check_op(hip, orc, ex, 3, (70, 13, 9), "own", "h27", "inner", data, MODES, entry_fastest=True, what="records", route=(hipd, "field27_rec"))
    shape = (70, 12, 9)
    b, e = box(3, shape, "dup")
    assert _holds_last_point(layouts(3, shape, "same")[3], b, e)
    check_op(hip, orc, ex, 3, shape, "same", "h27", "dup", data, MODES_GENERIC[:4], entry_fastest=True, what="last point", route=(hipd, "generic"))


GENERIC_CASES = [
    # (nd, cells, layouts, box, entry list, entry-fastest?)
    (3, (70, 20, 12), "own", "inner", "vc7_perm_a", False),     # long rows, permuted orders: not the z-march kernel's entry list
    (3, (131, 9, 7), "own2", "dup", "vc7_perm_b", False),
    (3, (70, 20, 12), "own", "odd", "vc7_perm_b", True),
    (3, (33, 17, 9), "own", "dup", "vc7", False),                # rows shorter than 64 points
    (3, (33, 17, 9), "same", "inner", "vc7", True),
    (2, (80, 33, 0), "own", "inner", "vc5", False),
    (2, (257, 20, 0), "own2", "dup", "vc5_perm", False),
    (2, (80, 33, 0), "own", "odd", "vc5_perm", True),
    (3, (40, 12, 9), "own", "inner", "h27_perm", False),         # 27 entries, the centre not first
    (3, (70, 11, 6), "own2", "dup", "h27_perm", True),
]


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("nd,shape,lay,which,kind,ef", GENERIC_CASES, ids=["%s-%d-%s-%s-%s" % (c[4], c[1][0], c[2], c[3], "records" if c[5] else "planes")
                                                                           for c in GENERIC_CASES])
def test_generic_kernel_with_a_stencil_field(hip, orc, ex, nd, shape, lay, which, kind, ef, data):
    """pins k_stencil_generic, cfield branch (plain u): permuted entry lists with the centre elsewhere, 2-D, short rows, both weight
    forms, coefficients in planes and entry-fastest, colour loops of both colours (in place for the stars)."""
    check_op(hip, orc, ex, nd, shape, lay, kind, which, data, MODES_GENERIC, entry_fastest=ef, what="generic")


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("kind,ef", [("vc7", False), ("h27", False), ("h27", True)])
def test_generic_kernel_forced_on_the_fast_kernels_inputs(hipd, orc, ex, kind, ef, data):
    """pins k_stencil_generic, cfield branch, on the inputs of the three fast kernels (examg_debug_force_generic): `omega / diag(A)`
    and colour loops too, which those kernels leave to it anyway."""
    old = hipd.L.examg_debug_force_generic(1)
    try:
        check_op(hipd, orc, ex, 3, (70, 12, 9), "own", kind, "inner", data, MODES_GENERIC, entry_fastest=ef, what="forced generic",
                 route=(hipd, "generic"))
    finally:
        hipd.L.examg_debug_force_generic(old)


SPLIT_CASES = [(3, (40, 20, 12), None, None), (3, (33, 17, 9), [0, 1, 0], [34, 17, 10]), (3, (200, 12, 40), None, None),
               (3, (131, 9, 7), [0, 0, 0], [132, 10, 8]), (3, (24, 14, 8), None, None), (2, (64, 48, 0), None, None)]


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("nd,shape,b,e", SPLIT_CASES, ids=["%dd-%d" % (c[0], c[1][0]) for c in SPLIT_CASES])
def test_stencil_field_on_colour_split_fields(hip, orc, ex, nd, shape, b, e, data):
    """pins k_stencil_generic, cfield branch for a colour-split u (`[x, y, z] => [x / 2, y, z, x % 2]`): u, rhs and the destination
    split, each from its own plain layout, the coefficients plain in theirs; the cases of tests/test_gpu_layout_split.py, transformed
    back: the reference's loop on the plain layouts."""
    if b is None:
        b, e = box(nd, shape, "inner")
    R = ref_ops(data, orc, ex)
    lu, lf, ld, lc = layouts(nd, shape, "own")
    for kind, ef in ((("vc7", False), ("vc7_perm_a", True)) if nd == 3 else (("vc5_perm", False),)):
        for mode, colour, wform in ((SMOOTH, 0, 0), (SMOOTH, 1, 1), (SMOOTH, -1, 0), (SMOOTH, -1, 1), (RESIDUAL, -1, 0), (APPLY, -1, 0)):
            st = S.stencil_field(hip, S.field_offsets(kind), lc, data, 900, wform)
            call = st.entry_fastest(hip) if ef else st
            u, f, d = (S.data_field(hip, l.size, data, 901 + i) for i, l in enumerate((lu, lf, ld)))
            lays = (lu, lf, lu if colour >= 0 else ld)
            split = [hip.new_array(l.split_x().size) for l in lays]
            for x, xs, l in zip((u, f, d), split, lays):
                if not (colour >= 0 and x is d):
                    hip.transform_field(l.c_struct(), x, l.split_x().c_struct(), xs)
            Su, Sf, Sd = (l.split_x().c_struct() for l in lays)
            hip.stencil_op(mode, Su, split[0], Sf, split[1], Sd, split[0] if colour >= 0 else split[2], call, weight(data), colour, b, e)
            for x, xs, l in zip((u, f, d), split, lays):
                if not (colour >= 0 and x is d):
                    hip.transform_field(l.split_x().c_struct(), xs, l.c_struct(), x)
            got = host(hip, (u, f, d, st.cfield))
            want = host(R, _op_run(R, nd, shape, "own", kind, data, mode, colour, wform, b, e))
            assert_same(got, want, "split %s mode %d colour %d wform %d" % (kind, mode, colour, wform))


# -- two Jacobi steps / a step + the residual on 27-entry records: one pass ---------------------------------------------------------
def _pair_run(ops, shape, lay, data, kind, b1, e1, b2, e2, ref, seed=950):
    lu, lf, lr, lc = layouts(3, shape, lay)
    st = S.stencil_field(ops, S.field_offsets("h27"), lc, data, seed)
    u, f, out, res = (S.data_field(ops, l.size, data, seed + 1 + i) for i, l in enumerate((lu, lf, lu, lr)))
    L, F, Lr = lu.c_struct(), lf.c_struct(), lr.c_struct()
    w = weight(data)
    call = st if ref else st.entry_fastest(ops)
    tmp = None if ref else S.data_field(ops, lu.size, data, seed + 7)
    if kind == "jacobi_residual":
        out = S._clone(ops, u)       # include/examg.h: u_out holds u_in's values on the box's shell
        if ref:
            S.jacobi_residual(ops, L, u, out, F, f, Lr, res, st, w, b2, e2)
        else:
            ops.jacobi_residual(L, u, out, F, f, Lr, res, call, w, b2, e2)
    elif kind == "jacobi2":
        if ref:
            S.jacobi2(ops, L, u, out, F, f, st, w, b2, e2)
        else:
            ops.jacobi2(L, u, out, tmp, F, f, call, w, b2, e2)
    elif ref:
        S.jacobi2_boxes(ops, L, u, out, F, f, st, w, b1, e1, b2, e2)
    else:
        ops.jacobi2_boxes(L, u, out, tmp, F, f, call, w, b1, e1, b2, e2)
    return [out, res, u, f, st.cfield]


def _r2_fits(lc, b2, e2):
    """kernels_sf27pair.hip: the two-rows-per-wave kernel streams 64 records per row; it needs them inside the coefficient rows."""
    L = S._Lay(lc)
    return L.tot[0] >= 64 and b2[0] - 1 + L.ref[0] >= 0 and e2[0] + L.ref[0] <= L.tot[0] - 1


PAIR_CASES = [
    # (cells, layouts, box 1, box 2)
    ((66, 30, 12), "own", "inner", "inner"),
    ((130, 20, 9), "own", "odd", "odd"),
    ((70, 47, 10), "same", "inner", "inner"),
    ((136, 30, 9), "own", "dup", "inner"),       # separate stage boxes: a block with neighbours
]


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("kind", ["jacobi2", "jacobi2_boxes", "jacobi_residual"])
@pytest.mark.parametrize("rows,zc", [(1, 0), (1, 5), (2, 0), (2, 4)], ids=["one-row", "one-row-chunks", "two-rows", "two-rows-chunks"])
@pytest.mark.parametrize("shape,lay,w1,w2", PAIR_CASES, ids=["%d-%s-%s" % (c[0][0], c[1], c[2]) for c in PAIR_CASES])
def test_sf27_two_stage_kernels(hipd, orc, ex, shape, lay, w1, w2, rows, zc, kind, data):
    """pins k_sf27_two_stage (one row per wave) and k_sf27_two_stage_r2 (two), forced through examg_debug_sf27_pair, through
    examg_jacobi2, examg_jacobi2_boxes and examg_jacobi_residual: whole arrays -- outside the box (box 2) nothing of u_out or res is
    written, the inputs and the scratch array's absence do not matter."""
    b1, e1 = box(3, shape, w1)
    b2, e2 = box(3, shape, w2)
    if kind == "jacobi2_boxes":
        if (b1, e1) == (b2, e2):
            b2, e2 = _boxes2(b1, e1, 3)
    elif (b1, e1) != (b2, e2):
        b1, e1 = b2, e2               # the one-box forms on box 2
    if rows == 2:
        assert _r2_fits(layouts(3, shape, lay)[3], b2, e2), "the case was meant for the two-rows-per-wave kernel"
    R = ref_ops(data, orc, ex)
    hipd.L.examg_debug_sf27_pair.argtypes = [C.c_int, C.c_int]
    hipd.L.examg_debug_sf27_pair(10 + rows, zc)
    try:
        got = host(hipd, _pair_run(hipd, shape, lay, data, kind, b1, e1, b2, e2, False))
    finally:
        hipd.L.examg_debug_sf27_pair(1, 0)
    want = host(R, _pair_run(R, shape, lay, data, kind, b1, e1, b2, e2, True))
    assert_same(got, want, "27-entry records, %s, %d rows per wave" % (kind, rows))


@pytest.mark.parametrize("kind", ["jacobi2", "jacobi_residual"])
def test_sf27_two_stage_product_library_exact(hip, ex, kind):
    """pins the pass as the product library launches it (from 2^20 points; its own choice of kernel and chunk length) on exact data
    in distinct layouts."""
    shape = (130, 100, 90)
    b, e = box(3, shape, "inner")
    got = host(hip, _pair_run(hip, shape, "own", "exact", kind, b, e, b, e, False))
    want = host(ex, _pair_run(ex, shape, "own", "exact", kind, b, e, b, e, True))
    assert_same(got, want, "27-entry records, product library, %s" % kind)


# -- the one-pass entry points handed a stencil field: their loops -------------------------------------------------------------------
# (cells, layouts, box, entry list, entry-fastest?)
FALLBACK_CASES = [
    ((130, 20, 12), "own", "inner", "vc7", False),        # the inputs of the constant-stencil one-pass kernels, but for the cfield
    ((70, 20, 12), "own2", "dup", "vc7_perm_a", False),
    ((40, 20, 10), "own", "odd", "vc7_perm_b", True),     # short rows: not the small-level kernels either
    ((70, 20, 12), "own", "inner", "h27", True),
    ((40, 14, 10), "own2", "odd", "h27_perm", False),
]
FALLBACK_IDS = ["%s-%d-%s-%s" % (c[3], c[0][0], c[1], c[2]) for c in FALLBACK_CASES]
SWEEP_KINDS = ["rbgs", "rbgs_zero", "rbgs_prolong", "rbgs_boxes", "jacobi2", "jacobi2_prolong", "jacobi2_boxes"]


def _case_stencils(gpu, R, shape, lay, kind, ef, data, unit=0.25):
    lc = layouts(3, shape, lay)[3]
    st_r = S.stencil_field(R, S.field_offsets(kind), lc, data, 970, unit=unit)
    st_g = S.stencil_field(gpu, S.field_offsets(kind), lc, data, 970, unit=unit)
    return (st_g.entry_fastest(gpu) if ef else st_g), st_g, st_r


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case,kind", [(c, k) for c in FALLBACK_CASES for k in SWEEP_KINDS if not (c[3].startswith("h27") and "rbgs" in k)],
                         ids=["%s-%s" % (i, k) for c, i in zip(FALLBACK_CASES, FALLBACK_IDS) for k in SWEEP_KINDS
                              if not (c[3].startswith("h27") and "rbgs" in k)])
def test_one_pass_sweeps_with_a_stencil_field(hip, orc, ex, case, kind, data):
    """examg_rbgs_sweep_fused / _zero / _prolong / _boxes and examg_jacobi2 / _prolong / _boxes handed a stencil field run their
    loops (pins k_stencilfield7_zmarch, k_stencilfield27_rec, k_stencilfield_unrolled and k_stencil_generic behind them):
    examg_two_stage_eligible says so; u_out over the whole array -- the box, and outside it what include/examg.h names: nothing for
    examg_jacobi2 and the two-box forms, u_in's values (zeros for the zero-field form) on the box's one-reach shell for the other
    sweep forms -- and the inputs unchanged."""
    shape, lay, which, skind, ef = case
    lu, lf, _, lc = layouts(3, shape, lay)
    lco = FieldLayout.node(3, tuple(s // 2 for s in shape), 1, align=2)
    b, e = box(3, shape, which)
    if kind.endswith("prolong") and which == "dup":
        b = [1, 1, 1]
    b2, e2 = _boxes2(b, e, 3)
    R = ref_ops(data, orc, ex)
    call, st_g, st_r = _case_stencils(hip, R, shape, lay, skind, ef, data)
    assert not hip.two_stage_eligible(lu.c_struct(), lf.c_struct(), call, b, e, *((b2, e2) if kind.endswith("_boxes") else (b, e)))
    first = 1 if lay == "own2" else 0
    got = host(hip, _sweep_run(hip, data, kind, lu, lf, lco, call, weight(data), b, e, first, False) + [st_g.cfield])
    want = host(R, _sweep_run(R, data, kind, lu, lf, lco, st_r, weight(data), b, e, first, True) + [st_r.cfield])
    want[0] = _expected_outside(kind, "fallback", want, lu, b, e, st_r)
    assert_same(got, want, "%s on a stencil field (%s)" % (kind, skind))


# (an in-place colour loop of a 27-entry stencil depends on the loop order: those fields take examg_jacobi3 only)
THREE_CASES = [(c, k) for c in FALLBACK_CASES for k in ("jacobi3", "colours3_0", "colours3_1") if k == "jacobi3" or not c[3].startswith("h27")]


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case,kind", THREE_CASES, ids=["%s-%s" % (FALLBACK_IDS[FALLBACK_CASES.index(c)], k) for c, k in THREE_CASES])
def test_three_steps_with_a_stencil_field(hip, hip3, orc, ex, case, kind, data):
    """examg_jacobi3 / examg_rbgs_colours3 handed a stencil field: the loops one after the other (examg_three_stage_eligible and
    examg_two_stage_eligible say so, on the product library and with the debug build's lowered size bound); u_in's values on the
    box's one-reach shell of u_out, nothing further out."""
    from test_gpu_stencil_asym import reach, with_shell

    shape, lay, which, skind, ef = case
    lu, lf, _, lc = layouts(3, shape, lay)
    b, e = box(3, shape, which)
    R = ref_ops(data, orc, ex)
    for gpu in (hip, hip3):
        call, st_g, st_r = _case_stencils(gpu, R, shape, lay, skind, ef, data)
        assert not gpu.three_stage_eligible(lu.c_struct(), lf.c_struct(), call, b, e)
        assert not gpu.two_stage_eligible(lu.c_struct(), lf.c_struct(), call, b, e, b, e)
        got = host(gpu, _three_run(gpu, data, kind, lu, lf, call, weight(data), b, e, False) + [st_g.cfield])
        want = host(R, _three_run(R, data, kind, lu, lf, st_r, weight(data), b, e, True) + [st_r.cfield])
        want[0] = with_shell(want[0], want[1], lu, b, e, reach(st_r))
        assert_same(got, want, "%s on a stencil field (%s)" % (kind, skind))


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case", FALLBACK_CASES, ids=FALLBACK_IDS)
def test_jacobi_residual_with_a_stencil_field(hip, orc, ex, case, data):
    """examg_jacobi_residual on the product library below its one-pass bound (2^20 points) and on entry lists the pass does not take:
    examg_jacobi + examg_residual; nothing of u_out or res written outside the box; the residual in a layout of its own."""
    shape, lay, which, skind, ef = case
    lu, lf, lr, lc = layouts(3, shape, lay)
    b, e = box(3, shape, which)
    R = ref_ops(data, orc, ex)
    call, st_g, st_r = _case_stencils(hip, R, shape, lay, skind, ef, data)

    def run(ops, st, ref):
        u, f, res = (S.data_field(ops, l.size, data, 980 + i) for i, l in enumerate((lu, lf, lr)))
        out = S._clone(ops, u)
        if ref:
            S.jacobi_residual(ops, lu.c_struct(), u, out, lf.c_struct(), f, lr.c_struct(), res, st, weight(data), b, e)
        else:
            ops.jacobi_residual(lu.c_struct(), u, out, lf.c_struct(), f, lr.c_struct(), res, st, weight(data), b, e)
        return [out, res, u, f]

    assert_same(host(hip, run(hip, call, False) + [st_g.cfield]), host(R, run(R, st_r, True) + [st_r.cfield]), "jacobi_residual (%s)" % skind)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case", FALLBACK_CASES, ids=FALLBACK_IDS)
def test_residual_restrict_with_a_stencil_field(hip, orc, ex, case, data):
    """examg_residual_restrict handed a stencil field: examg_residual + examg_restrict through `res` (examg_residual_restrict_one_pass
    says so); the coarse array outside the restriction's box keeps what it held; the residual in a layout of its own."""
    shape, lay, _, skind, ef = case
    lu, lf, lr, lc = layouts(3, shape, lay)
    cs = tuple(s // 2 for s in shape)
    lco = FieldLayout.node(3, cs, 0, True, False, 4)
    fb, fe, cb, ce = [1, 1, 1], list(shape), [1, 1, 1], list(cs)
    R = ref_ops(data, orc, ex)
    call, st_g, st_r = _case_stencils(hip, R, shape, lay, skind, ef, data)
    assert not hip.residual_restrict_one_pass(lu.c_struct(), lf.c_struct(), call, lco.c_struct(), fb, fe, cb, ce)

    def run(ops, st, ref):
        u, f, fc = (S.data_field(ops, l.size, data, 985 + i) for i, l in enumerate((lu, lf, lco)))
        if ref:
            r = S._zeros_like(ops, S.data_field(ops, lr.size, data, 1))
            ops.stencil_op(RESIDUAL, lu.c_struct(), u, lf.c_struct(), f, lr.c_struct(), r, st, 0.0, -1, fb, fe)
            ops.restrict(lr.c_struct(), r, lco.c_struct(), fc, 4.0, cb, ce)
        else:
            r = ops.new_array(lr.size)
            ops.residual_restrict(lu.c_struct(), u, lf.c_struct(), f, lr.c_struct(), r, st, lco.c_struct(), fc, 4.0, fb, fe, cb, ce)
        return [fc, u, f]

    assert_same(host(hip, run(hip, call, False) + [st_g.cfield]), host(R, run(R, st_r, True) + [st_r.cfield]), "residual_restrict (%s)" % skind)


@pytest.mark.parametrize("case", FALLBACK_CASES, ids=FALLBACK_IDS)
def test_residual_norm2_with_a_stencil_field(hip, orc, ex, case):
    """examg_residual_norm2 handed a stencil field: examg_residual + examg_dot.  Integer coefficients and data give integer
    residuals, whose squares sum exactly in any order: equality with the exact value; random data: 1e-13 relative against the
    oracle's two loops (the summation order differs)."""
    shape, lay, which, skind, ef = case
    lu, lf, lr, lc = layouts(3, shape, lay)
    b, e = box(3, shape, which)
    for data in DATA:
        R = ref_ops(data, orc, ex)
        call, st_g, st_r = _case_stencils(hip, R, shape, lay, skind, ef, data, unit=1.0)

        def run(ops, st):
            u, f = S.data_field(ops, lu.size, data, 990), S.data_field(ops, lf.size, data, 991)
            if ops is hip:
                s = ops.residual_norm2(lu.c_struct(), u, lf.c_struct(), f, st, b, e, lr.c_struct(), ops.new_array(lr.size))
            else:
                s = ops.residual_norm2(lu.c_struct(), u, lf.c_struct(), f, st, b, e)
            return s if isinstance(s, float) else ops.scalar_value(s)

        got, want = run(hip, call), run(R, st_r)
        if data == "exact":
            assert got == want and want > 0, (got, want)
        else:
            assert abs(got - want) <= 1e-13 * want, (got, want)


# -- constant stencils, one layout per argument: the window start of the z-march kernel, the row-marching kernel -----------------
def _origin_parity(l, b0):
    L = S._Lay(l)
    return (L.ref[0] + L.tot[0] * (L.ref[1] + L.tot[1] * L.ref[2]) + b0) & 1


def _even_strides(l):
    L = S._Lay(l)
    return L.tot[0] % 2 == 0 and (L.tot[0] * L.tot[1]) % 2 == 0


def _const_run(ops, lu, lf, ld, st, data, mode, colour, b, e):
    u, f, d = (S.data_field(ops, l.size, data, 1000 + i) for i, l in enumerate((lu, lf, ld)))
    w = S.EXACT_W if data == "exact" else S.free_weight(st)
    ops.stencil_op(mode, lu.c_struct(), u, lf.c_struct(), f, ld.c_struct(), d, st, w, colour, b, e)
    return [u, f, d]


PARITIES = [(gu, gf, gd) for gu in (1, 2) for gf in (0, 1) for gd in (0, 1)]


def test_the_parity_cases_reach_all_eight_parities():
    seen = set()
    for gu, gf, gd in PARITIES:
        lays = [FieldLayout.node(3, (131, 14, 10), g) for g in (gu, gf, gd)]
        assert all(_even_strides(l) for l in lays)
        seen.add(tuple(_origin_parity(l, 1) for l in lays))
    assert len(seen) == 8


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("store", [0, 1, 2])
@pytest.mark.parametrize("odd_dst", [False, True], ids=["even-strides", "dst-odd-strides"])
@pytest.mark.parametrize("gu,gf,gd", PARITIES, ids=["g%d%d%d" % p for p in PARITIES])
def test_zmarch_window_start_for_every_parity_of_the_three_layouts(hipd, orc, ex, gu, gf, gd, odd_dst, store, data):
    """pins k_stencil7_zmarch with u, rhs and the destination in three layouts: 131 cells make every stride even, the ghost widths
    (1 or 2 / 0 or 1 / 0 or 1) then give all eight parities (pu, pf, pd) of the box's first point, from which the dispatch decides to
    start the windows one point to the left; a destination with a pad column has odd strides, so that the strides are not all even
    because of the destination alone.  Every store mode of examg_debug_zmarch_store (1 computes the store alignment from the
    destination's layout), all three loop kinds, both canonical entry orders."""
    shape = (131, 14, 10)
    lu, lf, ld = (FieldLayout.node(3, shape, g) for g in (gu, gf, gd))
    if odd_dst:
        ld = dataclasses.replace(ld, pad_r=(1, 0, 0))
        assert not _even_strides(ld) and _even_strides(lu) and _even_strides(lf)
    b, e = box(3, shape, "inner")
    R = ref_ops(data, orc, ex)
    hipd.L.examg_debug_zmarch_store(store)
    try:
        for order in ("mp", "pm"):
            st = S.exact7(order) if data == "exact" else S.convdiff7(shape, order)
            for mode in (APPLY, RESIDUAL, SMOOTH):
                got = host(hipd, _const_run(hipd, lu, lf, ld, st, data, mode, -1, b, e))
                want = host(R, _const_run(R, lu, lf, ld, st, data, mode, -1, b, e))
                assert_same(got, want, "z-march, ghosts %d %d %d, %s, mode %d" % (gu, gf, gd, order, mode))
    finally:
        hipd.L.examg_debug_zmarch_store(-1)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("gu,gf,gd", [(1, 0, 2), (2, 1, 1), (1, 1, 0)])
def test_zmarch_product_library_with_three_layouts(hip, orc, ex, gu, gf, gd, data):
    """pins k_stencil7_zmarch as the product library launches it, u, rhs and the destination in three layouts (even strides), on a
    box inside the inner points with an odd origin."""
    shape = (131, 14, 10)
    lu, lf, ld = (FieldLayout.node(3, shape, g) for g in (gu, gf, gd))
    R = ref_ops(data, orc, ex)
    for which in ("inner", "odd"):
        b, e = box(3, shape, which)
        st = S.exact7("pm") if data == "exact" else S.convdiff7(shape, "pm")
        for mode in (APPLY, RESIDUAL, SMOOTH):
            got = host(hip, _const_run(hip, lu, lf, ld, st, data, mode, -1, b, e))
            want = host(R, _const_run(R, lu, lf, ld, st, data, mode, -1, b, e))
            assert_same(got, want, "z-march, ghosts %d %d %d, %s, mode %d" % (gu, gf, gd, which, mode))


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("shape,forced,unforced", [((420, 70, 17), 1, "rowmarch"), ((200, 30, 9), 12, "zmarch"), ((420, 20, 6), 1, "zmarch")],
                         ids=["four-segments", "two-segments", "short-box"])
def test_rowmarch_with_three_layouts(hipd, orc, ex, shape, forced, unforced, data):
    """pins k_stencil7_rowmarch (rows of 400 .. 512 points in four segments; 144 .. 256 in two, a debug variant), forced through
    examg_debug_rowmarch, with u, rhs and the destination in three layouts (ghost widths 2 / 0 / 1, alignments 0 / 4 / 2).  Left to
    itself the dispatch takes the kernel for the first box only: the second has short rows, the third too few rows and planes."""
    lu, lf, ld = FieldLayout.node(3, shape, 2), FieldLayout.node(3, shape, 0, True, False, 4), FieldLayout.node(3, shape, 1, align=2)
    b, e = box(3, shape, "inner")
    R = ref_ops(data, orc, ex)
    for mode in (APPLY, RESIDUAL, SMOOTH):
        assert stencil_route(hipd, mode, lu, lf, ld, S.exact7("mp"), -1, b, e, False) == unforced
    hipd.L.examg_debug_rowmarch.argtypes = [C.c_int] * 3
    hipd.L.examg_debug_rowmarch(forced, -1, -1)
    try:
        for order in ("mp", "pm"):
            st = S.exact7(order) if data == "exact" else S.convdiff7(shape, order)
            for mode in (APPLY, RESIDUAL, SMOOTH):
                assert stencil_route(hipd, mode, lu, lf, ld, st, -1, b, e, False) == "rowmarch"
                got = host(hipd, _const_run(hipd, lu, lf, ld, st, data, mode, -1, b, e))
                want = host(R, _const_run(R, lu, lf, ld, st, data, mode, -1, b, e))
                assert_same(got, want, "row-march %s mode %d" % (order, mode))
    finally:
        hipd.L.examg_debug_rowmarch(-1, -1, -1)


# -- stencil-field initialisation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [3, 2])
def test_init_varcoeff7_equals_the_definition(hip, nd):
    """pins k_init_varcoeff: examg_init_varcoeff7 with the asymmetric +, * coefficient program (1 + x + 2 y^2 + 4 z) on a layout with
    ghost layers and padding, a box off the array edges, power-of-two mesh widths: equal to the numpy restatement of include/examg.h,
    and nothing written outside the box."""
    from exastencils_amd.lib import ExprC
    from test_stencil_exact import _init_geometry

    lc, g, b, e = _init_geometry(nd)
    K = 2 * nd + 1
    start = np.random.default_rng(5).uniform(-1.0, 1.0, K * lc.size)
    cf = hip.from_host(start.copy())
    hip.init_varcoeff7(lc.c_struct(), cf, g, ExprC.from_program(S.ASYM_PROGRAM), (), b, e)
    want = start.copy()
    S.init_varcoeff7_ref(lc, want, g, S.asym_coefficient, b, e)
    hip.synchronize()
    assert np.array_equal(hip.to_host(cf), want)


def test_init_helmholtz27_equals_the_definition(hip):
    """pins k_init_helmholtz27, likewise (ksq = 2.5; entry order: the centre, then dz slowest and dx fastest)."""
    from exastencils_amd.lib import ExprC
    from test_stencil_exact import _init_geometry

    lc, g, b, e = _init_geometry(3)
    for d in range(3):
        g.h[d] = 1.0 / 16
    start = np.random.default_rng(6).uniform(-1.0, 1.0, 27 * lc.size)
    cf = hip.from_host(start.copy())
    hip.init_helmholtz27(lc.c_struct(), cf, g, ExprC.from_program(S.ASYM_PROGRAM), (0.0, 2.5), b, e)
    want = start.copy()
    S.init_helmholtz27_ref(lc, want, g, S.asym_coefficient, 2.5, b, e)
    hip.synchronize()
    assert np.array_equal(hip.to_host(cf), want)


# which test pins which kernel or dispatch branch, with exact data and with distinct layouts (every test here runs both)
PINS = {
    "k_stencilfield7_zmarch<2,4,0>": "test_stencilfield7_zmarch, test_stencilfield7_zmarch_variants[ry2pf0-3wg]",
    "k_stencilfield7_zmarch<1,4,1> <2,4,1> <1,4,2>": "test_stencilfield7_zmarch_variants",
    "k_stencilfield_unrolled<.,27>": "test_stencilfield27_unrolled",
    "k_stencilfield27_rec": "test_stencilfield27_records, test_stencilfield27_records_product_and_last_point",
    "k_stencil_generic, cfield": "test_generic_kernel_with_a_stencil_field, test_generic_kernel_forced_on_the_fast_kernels_inputs",
    "k_stencil_generic, cfield, colour-split u": "test_stencil_field_on_colour_split_fields",
    "k_sf27_two_stage, k_sf27_two_stage_r2": "test_sf27_two_stage_kernels, test_sf27_two_stage_product_library_exact",
    "one-pass entry points, stencil field": "test_one_pass_sweeps_with_a_stencil_field, test_three_steps_with_a_stencil_field, "
                                            "test_jacobi_residual_with_a_stencil_field, test_residual_restrict_with_a_stencil_field, "
                                            "test_residual_norm2_with_a_stencil_field",
    "k_stencil7_zmarch, three layouts": "test_zmarch_window_start_for_every_parity_of_the_three_layouts, "
                                        "test_zmarch_product_library_with_three_layouts",
    "k_stencil7_rowmarch, three layouts": "test_rowmarch_with_three_layouts",
    "k_init_varcoeff, k_init_helmholtz27": "test_init_varcoeff7_equals_the_definition, test_init_helmholtz27_equals_the_definition",
}


def test_every_pinned_test_exists():
    for tests in PINS.values():
        for name in tests.split(", "):
            assert name.split("[")[0] in globals(), name
