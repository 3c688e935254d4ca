"""The inter-grid transfer entry points (examg_restrict, examg_prolong_add, examg_restrict_cell, examg_prolong_add_cell) on every
kernel they dispatch to, the fine and the coarse argument each in a layout of its own.  Each case runs twice, as the stencil suites
do (tests/test_gpu_stencil_asym.py, tests/test_gpu_stencil_field.py):

  (a) random data (fill_random), compared bit for bit with the oracle's loops (node fields) or the numpy restatement of
      tests/cell_ops.py (cell fields);
  (b) small integers and a dyadic scale, compared with equality against the exact reference of tests/stencil_cases.py, which is
      written from the definitions and does not depend on the order of the terms.

Every array of a call is compared as a whole allocation: the output is filled beforehand and keeps what it held outside the box,
the inputs come back unchanged.  The boxes are anisotropic (no two extents alike), so a kernel that swaps two extents, row groups or
z chunks fails.  The shapes are the smallest that reach each branch of the dispatch code (csrc/kernels_transfer.hip,
csrc/kernels_cell.hip); `_wide_plan` and `cell_form` restate the dispatch decisions and the cases are asserted against them.
Variants that only the debug build can select go through its hooks, always under try / finally (`hooks`)."""
import contextlib
import dataclasses
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import stencil_cases as S
from cell_ops import CellOracleOps
from stencil_cases import ExactOps
from test_gpu_kernels import hip, hipd  # noqa: F401  (fixtures)
from test_gpu_stencil_asym import assert_same, fields, host

from exastencils_amd.layout import FieldLayout
from exastencils_amd.lib import ExamgError

pytestmark = pytest.mark.gpu

DATA = ["random", "exact"]
SCALES = {"random": (1.0, 4.0, 0.3), "exact": (1.0, 4.0)}       # 0.3: not a power of two -- random data only, by construction


@pytest.fixture(scope="module")
def orc():
    return CellOracleOps()          # the oracle's loops, and the restatement of the cell entry points on top of them


@pytest.fixture(scope="module")
def ex():
    return ExactOps()


def ref_ops(data, orc, ex):
    return ex if data == "exact" else orc


@contextlib.contextmanager
def hooks(gpu, restrict=(), prolong=None, narrow=None):
    """Debug-build variant selection; the defaults come back whatever happens (the hooks are state of the shared library)."""
    L = gpu.L
    try:
        for v in restrict:
            L.examg_debug_restrict(int(v))
        if prolong is not None:
            L.examg_debug_prolong(int(prolong))
        if narrow is not None:
            L.examg_debug_cell_narrow(int(narrow))
        yield
    finally:
        L.examg_debug_restrict(1)
        L.examg_debug_restrict(-2)
        L.examg_debug_prolong(-1)
        L.examg_debug_cell_narrow(0)


# -- layouts ---------------------------------------------------------------------------------------------------------------------------
# (fine, coarse): (ghost, align, communicates duplicate layers, communicates ghost layers)
NODE_LAYS = {
    "same": ((1, 0, True, True), (1, 0, True, True)),            # what the older tests pass
    "own": ((2, 0, True, True), (0, 2, True, False)),
    "own2": ((1, 16, True, False), (2, 2, False, True)),
    "own3": ((1, 2, False, True), (0, 16, True, True)),
    "own4": ((2, 2, True, True), (1, 0, True, True)),
}


def node_pair(nd, fs, cs, lay):
    f, c = NODE_LAYS[lay]
    return FieldLayout.node(nd, fs, f[0], f[2], f[3], f[1]), FieldLayout.node(nd, cs, c[0], c[2], c[3], c[1])


def test_the_distinct_layouts_are_distinct():
    for nd, fs, cs in ((3, (130, 18, 10), (65, 9, 5)), (2, (60, 22, 0), (30, 11, 0))):
        for lay in NODE_LAYS:
            lf, lc = (S._Lay(l) for l in node_pair(nd, fs, cs, lay))
            if lay != "same":
                assert (lf.ref[0], lf.tot[0] - fs[0]) != (lc.ref[0], lc.tot[0] - cs[0])


def _split(ops, l, x):
    xs = ops.new_array(l.split_x().size)
    ops.transform_field(l.c_struct(), x, l.split_x().c_struct(), xs)
    return xs


def _unsplit(ops, l, xs):
    x = ops.new_array(l.size)
    ops.transform_field(l.split_x().c_struct(), xs, l.c_struct(), x)
    return x


# -- examg_restrict ---------------------------------------------------------------------------------------------------------------------
def restrict_run(ops, lf, lc, data, scale, b, e, split=(False, False)):
    """[coarse rhs, fine residual] after one examg_restrict; the coarse array starts filled.  split: the fine / the coarse array
    under the colour split (GPU layer only), transformed there and back: the reference runs on the plain layouts."""
    rf, fc = fields(ops, data, (lf, lc), 300)
    Lf, Lc = (lf.split_x() if split[0] else lf), (lc.split_x() if split[1] else lc)
    rf_, fc_ = (_split(ops, lf, rf) if split[0] else rf), (_split(ops, lc, fc) if split[1] else fc)
    ops.restrict(Lf.c_struct(), rf_, Lc.c_struct(), fc_, scale, b, e)
    return [_unsplit(ops, lc, fc_) if split[1] else fc_, _unsplit(ops, lf, rf_) if split[0] else rf_]


def check_restrict(gpu, orc, ex, nd, n, kind, lay, data, split=(False, False), what=""):
    fs, cs, b, e = S.restrict_geometry(nd, n, kind)
    lf, lc = node_pair(nd, fs, cs, lay)
    R = ref_ops(data, orc, ex)
    for scale in SCALES[data]:
        got = host(gpu, restrict_run(gpu, lf, lc, data, scale, b, e, split))
        want = host(R, restrict_run(R, lf, lc, data, scale, b, e))
        assert_same(got, want, "restrict %s %r %s %s %s scale %g" % (what, n, kind, lay, data, scale))


def _wide_plan(n, rw, target=4096):
    """csrc/kernels_transfer.hip, examg_restrict: the launch of k_restrict3_wide<rw> for a coarse box of n points."""
    ntx = (n[0] + 63) // 64
    n1w = (n[1] + rw - 1) // rw
    cols = ntx * n1w
    ntz = max((target + cols - 1) // cols, 1)
    zc = min(max((n[2] + ntz - 1) // ntz, 8), n[2])
    ntz = (n[2] + zc - 1) // zc
    nwaves = cols * ntz
    banded = cols % 4 == 0
    wpl = cols // 4
    band = "none" if not banded else ("below8" if wpl < 8 else ("exact" if wpl % 8 == 0 else "remainder"))
    return dict(ntx=ntx, n1w=n1w, cols=cols, chunks=[min(zc, n[2] - k) for k in range(0, n[2], zc)], nwaves=nwaves, band=band,
                phantom=rw == 2 and n[1] % 2 == 1)


# coarse box extents; which quantity each sets (rw = 2: two coarse rows per wave, the product; rw = 1 through the debug hook):
WIDE_CASES = [
    ((32, 9, 8), "inner", "own"),            # the shortest wide row; 9 rows: a phantom second row; cols 5 / 9: no band permutation
    ((33, 7, 5), "inside_even", "own4"),     # one point past half a tile; 5 planes: one chunk shorter than 8
    ((64, 16, 9), "inner", "own2"),          # a full tile; cols 8 / 16: bands with fewer than 8 workgroups per layer; planes 8 + 1
    ((65, 32, 8), "faces", "own3"),          # lane 0 of a second tile reads its edge column; cols 32 / 64: exactly 8k workgroups; 8 planes
    ((127, 31, 8), "inside_odd", "own"),     # one point short of two tiles; 31 rows: phantom; rw 2: cols 32, rw 1: 62 (none)
    ((128, 12, 20), "inside_even", "same"),  # two full tiles; cols 12 / 24: below 8; planes 8 + 8 + 4
    ((129, 24, 9), "inner", "own2"),         # a third tile of one point; cols 36 / 72: 8k + remainder; planes 8 + 1
    ((129, 23, 20), "faces", "own"),         # the same with a phantom row (rw 2) and 69 columns (rw 1: none); three chunks
    ((64, 10, 20), "inner", "own3"),         # cols 5: 15 waves, the last workgroup holds three; rw 1: 10 columns, 30 waves: two
]
WIDE_IDS = ["%dx%dx%d-%s-%s" % (c[0] + (c[1], c[2])) for c in WIDE_CASES]


def test_the_wide_cases_reach_every_dispatch_branch():
    for rw in (1, 2):
        plans = [_wide_plan(c[0], rw, 1 << 20) for c in WIDE_CASES]
        assert {p["band"] for p in plans} == {"none", "below8", "exact", "remainder"}
        assert any(p["nwaves"] % 4 for p in plans) and any(p["nwaves"] % 4 == 0 for p in plans)
        assert [8, 8, 4] in [p["chunks"] for p in plans] and [8, 1] in [p["chunks"] for p in plans] and [8] in [p["chunks"] for p in plans]
        assert {p["ntx"] for p in plans} == {1, 2, 3}
    assert {c[0][0] for c in WIDE_CASES} >= {32, 33, 64, 65, 127, 128, 129}
    assert {_wide_plan(c[0], 2)["phantom"] for c in WIDE_CASES} == {True, False}
    assert {c[1] for c in WIDE_CASES} == {"inner", "faces", "inside_odd", "inside_even"}
    # the product's wave target gives the same chunks of 8 planes at these sizes; a target of 2 waves gives one chunk
    assert all(_wide_plan(c[0], 2) == _wide_plan(c[0], 2, 1 << 20) and len(_wide_plan(c[0], 2, 2)["chunks"]) == 1 for c in WIDE_CASES)
    for c in WIDE_CASES:
        b = S.restrict_geometry(3, *c[:2])[2]
        assert (b[0] & 1) == {"inner": 1, "faces": 0, "inside_odd": 1, "inside_even": 0}[c[1]]


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("n,kind,lay", WIDE_CASES, ids=WIDE_IDS)
def test_restrict_wide_product(hip, orc, ex, n, kind, lay, data):
    """pins k_restrict3_wide<2> as the product library launches it."""
    check_restrict(hip, orc, ex, 3, n, kind, lay, data, what="wide, product")


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("rows,target", [(-2, 2), (-2, 1 << 20), (-1, 2), (-1, 1 << 20)], ids=["rw2-one-chunk", "rw2-chunks-of-8", "rw1-one-chunk", "rw1-chunks-of-8"])
@pytest.mark.parametrize("n,kind,lay", WIDE_CASES, ids=WIDE_IDS)
def test_restrict_wide_rows_and_chunks(hipd, orc, ex, n, kind, lay, rows, target, data):
    """pins k_restrict3_wide<2> and <1> (examg_debug_restrict(-2 / -1)) with the z chunks forced (examg_debug_restrict(n > 1): a
    target of 2 waves marches the whole box in one chunk, a large one cuts chunks of 8 planes: the carry P[0] = P[2] starts afresh
    at every chunk)."""
    with hooks(hipd, restrict=(target, rows)):
        check_restrict(hipd, orc, ex, 3, n, kind, lay, data, what="wide, rows %d target %d" % (rows, target))


# n0 = 31: the longest row of the generic kernel (32 and 33 are in WIDE_CASES); short boxes of every kind
GENERIC3_CASES = [((31, 7, 5), "inner", "own"), ((31, 6, 4), "faces", "own2"), ((9, 13, 6), "inside_odd", "own3"), ((12, 5, 7), "inside_even", "same")]
GENERIC2_CASES = [((20, 9, 0), "inner", "own"), ((150, 11, 0), "faces", "own2"), ((70, 6, 0), "inside_odd", "own3"), ((31, 40, 0), "inside_even", "own4")]


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("nd,n,kind,lay", [(3,) + c for c in GENERIC3_CASES] + [(2,) + c for c in GENERIC2_CASES])
def test_restrict_generic(hip, orc, ex, nd, n, kind, lay, data):
    """pins k_restrict<3> (rows below 32 points) and k_restrict<2> (short and long rows: 2-D has no wide kernel)."""
    assert nd == 2 or n[0] < 32
    check_restrict(hip, orc, ex, nd, n, kind, lay, data, what="generic")


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("n,kind,lay", [((129, 9, 8), "inner", "own"), ((64, 10, 9), "faces", "own3"), ((65, 7, 20), "inside_odd", "own2")])
def test_restrict_generic_forced_on_long_rows(hipd, orc, ex, n, kind, lay, data):
    """pins k_restrict<3> on the wide kernel's inputs (examg_debug_restrict(0))."""
    with hooks(hipd, restrict=(0,)):
        check_restrict(hipd, orc, ex, 3, n, kind, lay, data, what="forced generic")


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("split", [(True, False), (False, True), (True, True)], ids=["fine-split", "coarse-split", "both-split"])
@pytest.mark.parametrize("nd,n,kind,lay", [(3, (66, 9, 8), "inner", "own"), (3, (33, 6, 5), "faces", "own4"), (2, (40, 9, 0), "inside_odd", "own2")])
def test_restrict_on_colour_split_fields(hip, orc, ex, nd, n, kind, lay, split, data):
    """pins k_restrict<3> / <2>, transformed index (`[x, y, z] => [x / 2, y, z, x % 2]`) for the fine array only, the coarse array only
    and both, on rows that the wide kernel would take were the layouts plain."""
    check_restrict(hip, orc, ex, nd, n, kind, lay, data, split, what="split %r" % (split,))


# -- examg_prolong_add -----------------------------------------------------------------------------------------------------------------
def prolong_run(ops, lc, lf, data, b, e, split=(False, False)):
    """[fine solution, coarse solution] after one examg_prolong_add."""
    uc, uf = fields(ops, data, (lc, lf), 400)
    Lf, Lc = (lf.split_x() if split[0] else lf), (lc.split_x() if split[1] else lc)
    uf_, uc_ = (_split(ops, lf, uf) if split[0] else uf), (_split(ops, lc, uc) if split[1] else uc)
    ops.prolong_add(Lc.c_struct(), uc_, Lf.c_struct(), uf_, b, e)
    return [_unsplit(ops, lf, uf_) if split[0] else uf_, _unsplit(ops, lc, uc_) if split[1] else uc_]


def check_prolong(gpu, orc, ex, nd, fs, b, e, lay, data, split=(False, False), what=""):
    cs = tuple((s + 1) // 2 for s in fs)
    lf, lc = node_pair(nd, fs, cs, lay)
    R = ref_ops(data, orc, ex)
    got = host(gpu, prolong_run(gpu, lc, lf, data, b, e, split))
    want = host(R, prolong_run(R, lc, lf, data, b, e))
    assert_same(got, want, "prolong_add %s %r..%r %s %s" % (what, b, e, lay, data))


def _pairs_plan(b, e):
    x0 = b[0] & ~1
    return dict(npairs=(e[0] - x0 + 1) // 2, first_whole=b[0] % 2 == 0, last_whole=e[0] % 2 == 0, rows=e[1] - b[1], planes=e[2] - b[2])


# fine cells (130, 14, 10) -- 131 points a row: with align 0 the rows have an odd length and start on odd and even elements in turn
# ('same', 'own'), with align 2 / 16 every row starts even.  (begin, end, layouts): which quantity each sets
PAIRS_FS = (130, 14, 10)
PAIRS_CASES = [
    ([1, 1, 1], [126, 9, 8], "own"),         # b0 odd (the first pair stores b only), e0 even (last pair whole): 63 pairs; 8 rows, 7 planes
    ([1, 2, 2], [127, 11, 9], "own2"),       # odd / odd (the last pair stores a only): 64 pairs; 9 rows; b1, b2 even
    ([2, 1, 2], [130, 11, 9], "same"),       # even / even (both end pairs whole, x0 = b0): 64 pairs; 10 rows
    ([2, 2, 1], [131, 13, 8], "own3"),       # even / odd: 65 pairs, a second tile of one pair; 11 rows
    ([0, 0, 0], [131, 15, 11], "own4"),      # over the duplicate planes: 66 pairs, 15 rows, 11 planes
    ([3, 1, 1], [35, 6, 4], "own"),          # 32 points, the shortest row of the pairs kernel
    ([4, 3, 3], [129, 10, 8], "own2"),       # even / odd with b1, b2 odd: 63 pairs; 7 rows, 5 planes
]
PAIRS_IDS = ["%d-%d-%s" % (c[0][0], c[1][0], c[2]) for c in PAIRS_CASES]


def test_the_pairs_cases_reach_every_branch():
    plans = [_pairs_plan(b, e) for b, e, _ in PAIRS_CASES]
    assert {(p["first_whole"], p["last_whole"]) for p in plans} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {p["npairs"] for p in plans} >= {63, 64, 65} and {p["rows"] % 4 for p in plans} == {0, 1, 2, 3}
    assert {(b[1] % 2, b[2] % 2) for b, _, _ in PAIRS_CASES} == {(0, 0), (1, 1), (0, 1), (1, 0)}
    assert all(e[0] - b[0] >= 32 for b, e, _ in PAIRS_CASES) and any(p["planes"] % 2 and p["planes"] % 3 for p in plans)
    odd = {S._Lay(node_pair(3, PAIRS_FS, (65, 7, 5), lay)[0]).tot[0] % 2 for _, _, lay in PAIRS_CASES}
    assert odd == {0, 1}


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("b,e,lay", PAIRS_CASES, ids=PAIRS_IDS)
def test_prolong_pairs_product(hip, orc, ex, b, e, lay, data):
    """pins k_prolong_add3_pairs as the product library launches it (two planes per workgroup)."""
    check_prolong(hip, orc, ex, 3, PAIRS_FS, b, e, lay, data, what="pairs, product")


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("zb", [1, 2, 3])
@pytest.mark.parametrize("b,e,lay", PAIRS_CASES, ids=PAIRS_IDS)
def test_prolong_pairs_planes_per_workgroup(hipd, orc, ex, b, e, lay, zb, data):
    """pins k_prolong_add3_pairs with 1, 2 and 3 planes per workgroup (examg_debug_prolong); 7, 5 and 11 planes leave a short last
    run."""
    with hooks(hipd, prolong=zb):
        check_prolong(hipd, orc, ex, 3, PAIRS_FS, b, e, lay, data, what="pairs, zb %d" % zb)


PROLONG_GENERIC = [
    (3, (30, 9, 7), [1, 1, 1], [30, 9, 7], "own"), (3, (32, 7, 9), [0, 0, 0], [31, 8, 10], "own2"), (3, (20, 12, 8), [3, 2, 1], [18, 11, 6], "own3"),
    (2, (150, 11, 0), [1, 1, 0], [150, 11, 1], "own"), (2, (21, 40, 0), [0, 0, 0], [22, 41, 1], "own2"), (2, (70, 9, 0), [2, 3, 0], [67, 8, 1], "own4"),
]


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("nd,fs,b,e,lay", PROLONG_GENERIC)
def test_prolong_generic(hip, orc, ex, nd, fs, b, e, lay, data):
    """pins k_prolong_add<3> (rows below 32 points) and k_prolong_add<2> (short and long rows)."""
    assert nd == 2 or e[0] - b[0] < 32
    check_prolong(hip, orc, ex, nd, fs, b, e, lay, data, what="generic")


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("split", [(True, False), (False, True), (True, True)], ids=["fine-split", "coarse-split", "both-split"])
@pytest.mark.parametrize("nd,fs,b,e,lay", [(3, (130, 9, 7), [1, 1, 1], [130, 9, 7], "own"), (3, (67, 6, 5), [0, 0, 0], [68, 7, 6], "own4"),
                                           (2, (80, 13, 0), [3, 2, 0], [78, 12, 1], "own2")])
def test_prolong_on_colour_split_fields(hip, orc, ex, nd, fs, b, e, lay, split, data):
    """pins k_prolong_add<3> / <2>, transformed index for the fine array only, the coarse array only and both, on rows that the pairs
    kernel would take were the layouts plain."""
    check_prolong(hip, orc, ex, nd, fs, b, e, lay, data, split, what="split %r" % (split,))


# -- examg_restrict_cell / examg_prolong_add_cell ------------------------------------------------------------------------------------
def cell_layout(nd, cells, form, ghost=0, align=0):
    """A cell layout on either side of `pairs_aligned` (csrc/kernels_cell.hip) by its index arithmetic alone:
    '16': even reference offset and row strides (align 2 / 16, or two ghost layers);
    '8-origin': one ghost layer, no padding: the linear index of cell 0 is odd, the strides even;
    '8-s1': a pad column makes the row length odd, the plane stride (an even number of rows) and the origin stay even;
    '8-s1s2': a pad column and a pad row: both strides odd.  (An odd plane stride needs an odd row length: it cannot come alone.)"""
    c = [int(v) for v in cells[:nd]]
    assert all(v % 2 == 0 for v in c[:2])
    if form == "16":
        l = FieldLayout.cell(nd, c, ghost, align=align or (0 if ghost == 2 else 2))
    elif form == "8-origin":
        l = FieldLayout.cell(nd, c, 1)
    else:
        l = dataclasses.replace(FieldLayout.cell(nd, c, 0), pad_r=(1, 1 if form == "8-s1s2" else 0, 0))
    return l


def cell_form(l):
    """The form the product library takes for this fine layout: the facts `pairs_aligned` tests."""
    L = S._Lay(l)
    s1, s2 = L.tot[0], L.tot[0] * L.tot[1]
    origin = L.ref[0] + s1 * L.ref[1] + s2 * L.ref[2]
    facts = dict(origin=origin % 2, s1=s1 % 2, s2=s2 % 2 if L.nd == 3 else 0)
    return ("16" if not any(facts.values()) else "8"), facts


def test_the_cell_layouts_are_on_the_intended_side_of_pairs_aligned():
    for nd in (2, 3):
        c = (128, 16, 6)
        assert cell_form(cell_layout(nd, c, "16", 1, 2)) == ("16", dict(origin=0, s1=0, s2=0))
        assert cell_form(cell_layout(nd, c, "16", 0, 16))[0] == "16" and cell_form(cell_layout(nd, c, "16", 2))[0] == "16"
        assert cell_form(cell_layout(nd, c, "8-origin")) == ("8", dict(origin=1, s1=0, s2=0))
        assert cell_form(cell_layout(nd, c, "8-s1")) == ("8", dict(origin=0, s1=1, s2=0))
        assert cell_form(cell_layout(nd, c, "8-s1s2")) == ("8", dict(origin=0, s1=1, s2=1 if nd == 3 else 0))


# (nd, coarse box extents, offset of the box in the coarse field, fine form / ghost / align, coarse ghost / align)
# wpl = ceil(n0 / 64) * ceil(n1 / 4) workgroups per layer: the XCD band permutation is on when wpl % 8 == 0
CELL_CASES = [
    (3, (63, 8, 3), (0, 0, 0), ("16", 1, 2), (0, 0)),            # one lane short of a tile; wpl 2; n1 = 4k
    (3, (64, 32, 2), (1, 2, 1), ("8-origin", 1, 0), (2, 2)),     # a full tile; wpl 8: banded
    (3, (65, 13, 3), (0, 0, 0), ("8-s1", 0, 0), (1, 16)),        # a second tile of one lane; wpl 2 * 4 = 8: banded; n1 = 4k + 1
    (3, (130, 31, 2), (2, 1, 0), ("16", 2, 0), (1, 0)),          # three tiles; wpl 24: banded; n1 = 4k + 3
    (3, (130, 7, 3), (0, 0, 0), ("8-s1s2", 0, 0), (0, 2)),       # wpl 6; n1 = 4k + 3
    (3, (64, 9, 4), (1, 1, 1), ("16", 0, 16), (2, 0)),           # wpl 3; n1 = 4k + 1
    (2, (64, 32, 0), (0, 0, 0), ("16", 1, 2), (0, 0)),           # wpl 8: banded
    (2, (65, 13, 0), (1, 2, 0), ("8-origin", 1, 0), (2, 2)),     # wpl 8: banded; n1 = 4k + 1
    (2, (130, 31, 0), (0, 0, 0), ("8-s1", 0, 0), (1, 16)),       # wpl 24: banded
    (2, (63, 7, 0), (2, 1, 0), ("16", 2, 0), (0, 2)),            # wpl 2; n1 = 4k + 3
]
CELL_IDS = ["%dd-%dx%d-%s" % (c[0], c[1][0], c[1][1], c[3][0]) for c in CELL_CASES]


def test_the_cell_cases_reach_every_branch():
    wpl = {((c[1][0] + 63) // 64) * ((c[1][1] + 3) // 4) % 8 == 0 for c in CELL_CASES}
    assert wpl == {True, False}
    for nd in (2, 3):
        cs = [c for c in CELL_CASES if c[0] == nd]
        assert {c[1][0] for c in cs} >= {63, 64, 65, 130} and {c[1][1] % 4 for c in cs} >= {0, 1, 3}
        assert {c[3][0] for c in cs} >= {"16", "8-origin", "8-s1"}


def cell_geometry(case):
    nd, n, off, (form, gf, af), (gc, ac) = case
    cb = [off[d] if d < nd else 0 for d in range(3)]
    ce = [off[d] + n[d] if d < nd else 1 for d in range(3)]
    cells = [ce[d] + (1 if off[d] else 0) for d in range(nd)]
    cells = [v + v % 2 for v in cells]                              # even counts: the stride facts of cell_layout
    lf = cell_layout(nd, [2 * v for v in cells], form, gf, af)
    lc = FieldLayout.cell(nd, cells, gc, gc != 1, ac)
    return nd, lf, lc, cb, ce


def restrict_cell_run(ops, lf, lc, data, scale, b, e):
    rf, fc = fields(ops, data, (lf, lc), 500)
    if hasattr(rf, "data_ptr") and data == "random":
        assert rf.data_ptr() % 16 == 0                  # the pointer is not what decides between the forms here
    ops.restrict_cell(lf.c_struct(), rf, lc.c_struct(), fc, scale, b, e)
    return [fc, rf]


def prolong_cell_run(ops, lc, lf, data, b, e):
    uc, uf = fields(ops, data, (lc, lf), 600)
    if hasattr(uf, "data_ptr") and data == "random":
        assert uf.data_ptr() % 16 == 0
    ops.prolong_add_cell(lc.c_struct(), uc, lf.c_struct(), uf, b, e)
    return [uf, uc]


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case", CELL_CASES, ids=CELL_IDS)
def test_restrict_cell_forms(hip, hipd, orc, ex, case, data):
    """pins k_restrict_cell<2 | 3, true | false>: the product library takes the form that the fine layout's index arithmetic decides
    (cell_form), the debug build once as decided and once with the 8-byte form forced: the same bits, each equal to the
    reference."""
    nd, lf, lc, cb, ce = cell_geometry(case)
    assert cell_form(lf)[0] == case[3][0][:2].rstrip("-")
    R = ref_ops(data, orc, ex)
    for scale in SCALES[data] + ((0.25,) if data == "exact" else ()):
        want = host(R, restrict_cell_run(R, lf, lc, data, scale, cb, ce))
        assert_same(host(hip, restrict_cell_run(hip, lf, lc, data, scale, cb, ce)), want, "restrict_cell, product, scale %g" % scale)
        for narrow in (0, 1):
            with hooks(hipd, narrow=narrow):
                got = host(hipd, restrict_cell_run(hipd, lf, lc, data, scale, cb, ce))
            assert_same(got, want, "restrict_cell, debug build, narrow %d, scale %g" % (narrow, scale))


# parity shifts of the fine box against the children of the coarse box: (begin, end) per dimension, 1 = one cell inside
SHIFTS = [((0, 0, 0), (0, 0, 0)), ((1, 0, 1), (0, 1, 0)), ((0, 1, 0), (1, 0, 1)), ((1, 1, 1), (1, 1, 1))]


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case", CELL_CASES, ids=CELL_IDS)
def test_prolong_add_cell_forms(hip, hipd, orc, ex, case, data):
    """pins k_prolong_add_cell<2 | 3, true | false>, as test_restrict_cell_forms; the fine box is the children of the coarse box of
    the case, and that box with one cell less at either end in some dimensions (a lane's pair straddles the box edge: the 16-byte
    form stores one half)."""
    nd, lf, lc, cb, ce = cell_geometry(case)
    assert cell_form(lf)[0] == case[3][0][:2].rstrip("-")
    R = ref_ops(data, orc, ex)
    for sb, se in SHIFTS:
        fb = [2 * cb[d] + sb[d] if d < nd else 0 for d in range(3)]
        fe = [2 * ce[d] - se[d] if d < nd else 1 for d in range(3)]
        want = host(R, prolong_cell_run(R, lc, lf, data, fb, fe))
        assert_same(host(hip, prolong_cell_run(hip, lc, lf, data, fb, fe)), want, "prolong_add_cell, product, %r..%r" % (fb, fe))
        for narrow in (0, 1):
            with hooks(hipd, narrow=narrow):
                got = host(hipd, prolong_cell_run(hipd, lc, lf, data, fb, fe))
            assert_same(got, want, "prolong_add_cell, debug build, narrow %d, %r..%r" % (narrow, fb, fe))


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("nd,form", [(3, "16"), (3, "8-origin"), (2, "16"), (2, "8-origin")])
def test_prolong_add_cell_every_parity_of_the_box(hip, orc, ex, nd, form, data):
    """pins the box edges of k_prolong_add_cell: every combination of an odd or even begin and end in every dimension, the begins in
    the ghost layer among them (cell -1: its parent is floor(-1 / 2) = -1, the arithmetic shift)."""
    cells = (20, 12, 8)
    lf = cell_layout(nd, cells, form, 1, 2)
    lc = FieldLayout.cell(nd, [v // 2 for v in cells[:nd]], 2, align=0)
    assert cell_form(lf)[0] == form[:2].rstrip("-") and lf.ghost[0] == 1
    R = ref_ops(data, orc, ex)
    choices = [[(b, e) for b in (-1, 2) for e in (cells[d] - 1, cells[d])] if d < nd else [(0, 1)] for d in range(3)]
    for b0, e0 in choices[0]:
        for b1, e1 in choices[1]:
            for b2, e2 in choices[2]:
                fb, fe = [b0, b1, b2], [e0, e1, e2]
                got = host(hip, prolong_cell_run(hip, lc, lf, data, fb, fe))
                want = host(R, prolong_cell_run(R, lc, lf, data, fb, fe))
                assert_same(got, want, "prolong_add_cell %r..%r" % (fb, fe))


# -- closed forms and the adjoint identity, once per kernel family --------------------------------------------------------------------
# (family, nd, coarse box extents, box kind, layouts)
NODE_FAMILIES = [("wide / pairs", 3, (65, 9, 12), "inner", "own"), ("wide / pairs", 3, (40, 7, 9), "faces", "own2"),
                 ("generic", 3, (13, 6, 9), "inside_odd", "own3"), ("generic", 2, (40, 9, 0), "faces", "own4")]


def _fine_box(nd, fs, cb, ce):
    """The fine points of the restriction's footprint that examg_prolong_add takes (no negative index) and the fine field has."""
    return ([max(2 * cb[d] - 1, 0) if d < nd else 0 for d in range(3)], [min(2 * ce[d], fs[d] + 1) if d < nd else 1 for d in range(3)])


@pytest.mark.parametrize("family,nd,n,kind,lay", NODE_FAMILIES)
def test_node_transfers_of_linear_fields_and_adjointness(hip, family, nd, n, kind, lay):
    """pins k_restrict3_wide / k_prolong_add3_pairs and the generic kernels against facts that need no reference: v = 3 i + 7 j + 11 k
    + 5 restricts to scale * v(2I), uc(I) = v(2I) interpolates onto zeros as v, and sum(fc * w) * 2^d == scale * sum(r * P w) in
    int64 for integer fields that vanish outside the boxes."""
    fs, cs, cb, ce = S.restrict_geometry(nd, n, kind)
    lf, lc = node_pair(nd, fs, cs, lay)
    fb, fe = _fine_box(nd, fs, cb, ce)
    assert (nd == 3 and n[0] >= 32 and fe[0] - fb[0] >= 32) == (family != "generic")
    for scale in (1.0, 4.0):
        fc, uf = hip.from_host(np.zeros(lc.size)), hip.from_host(np.zeros(lf.size))
        hip.restrict(lf.c_struct(), hip.from_host(S.linear_field(lf, S.LINEAR, 5)), lc.c_struct(), fc, scale, cb, ce)
        hip.prolong_add(lc.c_struct(), hip.from_host(S.linear_field(lc, S.LINEAR, 5, mul=2)), lf.c_struct(), uf, fb, fe)
        fc, uf = host(hip, (fc, uf))
        assert np.array_equal(S.box_values(lc, fc, cb, ce), scale * S.box_values(lc, S.linear_field(lc, S.LINEAR, 5, mul=2), cb, ce))
        assert np.array_equal(S.box_values(lf, uf, fb, fe), S.box_values(lf, S.linear_field(lf, S.LINEAR, 5), fb, fe))
        lhs, rhs = S.transfer_adjoint(hip, False, lf, lc, cb, ce, fb, fe, scale, 700)
        assert lhs == rhs


@pytest.mark.parametrize("case", [CELL_CASES[i] for i in (1, 2, 3, 7, 8)], ids=[CELL_IDS[i] for i in (1, 2, 3, 7, 8)])
def test_cell_transfers_of_linear_fields_and_adjointness(hip, case):
    """pins both forms of k_restrict_cell / k_prolong_add_cell likewise: fine values 2 v at the cell centres restrict to scale * 2 v at
    the parent's centre, a linear coarse field prolongs onto zeros as uc(i >> 1), and the adjoint identity of the pair."""
    nd, lf, lc, cb, ce = cell_geometry(case)
    fb = [2 * cb[d] + (d == 1) if d < nd else 0 for d in range(3)]
    fe = [2 * ce[d] - (d == 0) if d < nd else 1 for d in range(3)]
    for scale in (1.0, 4.0):
        fc, uf = hip.from_host(np.zeros(lc.size)), hip.from_host(np.zeros(lf.size))
        hip.restrict_cell(lf.c_struct(), hip.from_host(S.linear_field(lf, S.LINEAR, 10, mul=2, add=1)), lc.c_struct(), fc, scale, cb, ce)
        hip.prolong_add_cell(lc.c_struct(), hip.from_host(S.linear_field(lc, S.LINEAR, 4)), lf.c_struct(), uf, fb, fe)
        fc, uf = host(hip, (fc, uf))
        assert np.array_equal(S.box_values(lc, fc, cb, ce), scale * S.box_values(lc, S.linear_field(lc, S.LINEAR, 10, mul=4, add=2), cb, ce))
        idx = np.meshgrid(*[np.arange(fb[d], fe[d]) >> (1 if d < nd else 0) for d in (2, 1, 0)], indexing="ij")
        want = 4 + sum(S.LINEAR[d] * idx[2 - d] for d in range(nd))
        assert np.array_equal(S.box_values(lf, uf, fb, fe), want.astype(np.float64))
        lhs, rhs = S.transfer_adjoint(hip, True, lf, lc, cb, ce, fb, fe, scale, 710)
        assert lhs == rhs


# -- argument checks --------------------------------------------------------------------------------------------------------------------
def _refused(hip, entry, call, out, message):
    """The call fails with an error that names the entry point, and the output array keeps its bits (nothing was launched)."""
    before = host(hip, (out,))[0]
    with pytest.raises(ExamgError, match=r"\): %s: .*%s" % (entry, message)):
        call()
    assert np.array_equal(host(hip, (out,))[0], before, equal_nan=True)


def _nd(l, nd):
    s = l.c_struct()
    s.nd = nd
    return s


def test_node_transfer_argument_checks(hip):
    """Every set_error branch of examg_restrict and examg_prolong_add (tests/test_gpu_kernels.py::test_bad_arguments_fail_loudly has
    none of them): a nonzero return, the entry point's name in examg_last_error(), no launch.  The empty box returns 0 and is a
    no-op."""
    lf, lc = node_pair(3, (16, 12, 8), (8, 6, 4), "own4")               # fine ghost 2, coarse ghost 1
    small_f, small_c = FieldLayout.node(3, (12, 12, 8), 0), FieldLayout.node(3, (6, 6, 4), 0)
    rf, fc, uc, uf = fields(hip, "random", (lf, lc, lc, lf), 800)
    F, Cc = lf.c_struct(), lc.c_struct()
    R = lambda *a: (lambda: hip.restrict(*a))                           # noqa: E731
    P = lambda *a: (lambda: hip.prolong_add(*a))                        # noqa: E731
    _refused(hip, "examg_restrict", R(F, rf, Cc, fc, 1.0, [1, 1, 1], [8, 6, 7]), fc, "coarse allocation")
    _refused(hip, "examg_restrict", R(F, rf, Cc, fc, 1.0, [-2, 1, 1], [8, 6, 4]), fc, "coarse allocation")
    _refused(hip, "examg_restrict", R(small_f.c_struct(), rf, Cc, fc, 1.0, [1, 1, 1], [8, 6, 4]), fc, "fine footprint")
    _refused(hip, "examg_restrict", R(small_f.c_struct(), rf, Cc, fc, 1.0, [0, 1, 1], [6, 6, 4]), fc, "fine footprint")   # 2 * 0 - 1: no ghost layer
    for nd in (1, 4):
        _refused(hip, "examg_restrict", R(_nd(lf, nd), rf, _nd(lc, nd), fc, 1.0, [1, 1, 1], [8, 6, 4]), fc, "nd must be 2 or 3")
        _refused(hip, "examg_prolong_add", P(_nd(lc, nd), uc, _nd(lf, nd), uf, [1, 1, 1], [16, 12, 4]), uf, "nd must be 2 or 3")   # dim 2 is not halved unless nd == 3: [1, 4) lies in both
    _refused(hip, "examg_prolong_add", P(Cc, uc, F, uf, [1, 1, 1], [16, 12, 12]), uf, "fine allocation")
    _refused(hip, "examg_prolong_add", P(Cc, uc, F, uf, [-1, 1, 1], [16, 12, 8]), uf, "negative fine index")     # inside the ghost layers
    _refused(hip, "examg_prolong_add", P(Cc, uc, F, uf, [1, -2, 1], [16, 12, 8]), uf, "negative fine index")
    _refused(hip, "examg_prolong_add", P(small_c.c_struct(), uc, F, uf, [1, 1, 1], [16, 12, 8]), uf, "coarse footprint")
    _refused(hip, "examg_prolong_add", P(Cc, uc, F, uf, [1, 1, 1], [20, 12, 8]), uf, "coarse footprint")         # fine point 19 is the pad column of the row (allocated): it needs coarse 10, past the ghost 9
    assert lf.pad_r[0] == 1 and lf.ghost[0] == 2 and lc.ghost[0] == 1 and lc.pad_r[0] == 0
    before = host(hip, (fc, uf))
    for b, e in (([1, 1, 1], [1, 6, 4]), ([3, 4, 2], [8, 2, 4]), ([1, 1, 4], [8, 6, 4])):
        hip.restrict(F, rf, Cc, fc, 1.0, b, e)
        hip.prolong_add(Cc, uc, F, uf, b, e)
    assert_same(host(hip, (fc, uf)), before, "empty boxes")


def test_cell_transfer_argument_checks(hip):
    """Every set_error branch of examg_restrict_cell and examg_prolong_add_cell, likewise."""
    lf3, lc3 = FieldLayout.cell(3, (16, 12, 8), 1, align=2), FieldLayout.cell(3, (8, 6, 4), 1)
    lf2, lc2 = FieldLayout.cell(2, (16, 12), 1), FieldLayout.cell(2, (8, 6), 0, align=2)
    node_f, node_c = FieldLayout.node(3, (16, 12, 8), 1), FieldLayout.node(3, (8, 6, 4), 1)
    deep2_f, deep2_c = (dataclasses.replace(l, pad_r=(0, 0, 1)) for l in (lf2, lc2))           # 2-D layouts with a second (pad) plane
    rf, fc, uc, uf = fields(hip, "random", (lf3, lc3, lc3, lf3), 810)
    F3, C3, F2, C2 = lf3.c_struct(), lc3.c_struct(), lf2.c_struct(), lc2.c_struct()
    b3, ce3, fe3 = [0, 0, 0], [8, 6, 4], [16, 12, 8]
    R = lambda *a: (lambda: hip.restrict_cell(*a))                      # noqa: E731
    P = lambda *a: (lambda: hip.prolong_add_cell(*a))                   # noqa: E731
    for entry, mk, out in (("examg_restrict_cell", lambda f, c, b, e: R(f, rf, c, fc, 1.0, b, e), fc),
                           ("examg_prolong_add_cell", lambda f, c, b, e: P(c, uc, f, uf, b, e), uf)):
        r = entry == "examg_restrict_cell"
        full = ce3 if r else fe3
        _refused(hip, entry, mk(F3, C3, [0, 0, 0], [v + 3 for v in full]), out, "leaves an allocation")                 # past the ghost layer of both
        _refused(hip, entry, mk(F3, C3, [-2 if r else -3, 0, 0], full), out, "leaves an allocation")
        _refused(hip, entry, mk(FieldLayout.cell(3, (12, 12, 8), 0).c_struct(), C3, b3, full), out, "leaves an allocation")    # the fine field too small
        _refused(hip, entry, mk(F3, FieldLayout.cell(3, (6, 6, 4), 0).c_struct(), b3, full), out, "leaves an allocation")      # the coarse field too small
        _refused(hip, entry, mk(F3, C2, b3, full), out, "one dimensionality")
        _refused(hip, entry, mk(F2, C3, b3, full), out, "one dimensionality")
        for nd in (1, 4):
            _refused(hip, entry, mk(_nd(lf3, nd), _nd(lc3, nd), b3, full), out, "2-D or 3-D")
        _refused(hip, entry, mk(node_f.c_struct(), C3, b3, full), out, "no duplicate layers")
        _refused(hip, entry, mk(F3, node_c.c_struct(), b3, full), out, "no duplicate layers")
        _refused(hip, entry, mk(lf3.split_x().c_struct(), C3, b3, full), out, "layout transformation")
        _refused(hip, entry, mk(F3, lc3.split_x().c_struct(), b3, full), out, "layout transformation")
        full2 = [full[0], full[1], 1]
        _refused(hip, entry, mk(deep2_f.c_struct(), deep2_c.c_struct(), [0, 0, 1], full2[:2] + [2]), out, r"2-D box must have \[0,1\)")
        _refused(hip, entry, mk(deep2_f.c_struct(), deep2_c.c_struct(), [0, 0, 0], full2[:2] + [2]), out, r"2-D box must have \[0,1\)")
    before = host(hip, (fc, uf))
    for b, e in (([0, 0, 0], [0, 6, 4]), ([3, 4, 2], [8, 2, 4]), ([1, 1, 4], [8, 6, 4])):
        hip.restrict_cell(F3, rf, C3, fc, 1.0, b, e)
        hip.prolong_add_cell(C3, uc, F3, uf, b, e)
    assert_same(host(hip, (fc, uf)), before, "empty boxes")


# which test pins which kernel or dispatch branch (every test named here runs random and exact data, the fine and the coarse
# argument in layouts of their own)
PINS = {
    "k_restrict<2>": "test_restrict_generic, test_restrict_on_colour_split_fields, test_node_transfers_of_linear_fields_and_adjointness",
    "k_restrict<3>": "test_restrict_generic, test_restrict_generic_forced_on_long_rows, test_restrict_on_colour_split_fields, "
                     "test_node_transfers_of_linear_fields_and_adjointness",
    "k_restrict3_wide<2>": "test_restrict_wide_product, test_restrict_wide_rows_and_chunks[rw2-one-chunk], "
                           "test_restrict_wide_rows_and_chunks[rw2-chunks-of-8], test_node_transfers_of_linear_fields_and_adjointness",
    "k_restrict3_wide<1>": "test_restrict_wide_rows_and_chunks[rw1-one-chunk], test_restrict_wide_rows_and_chunks[rw1-chunks-of-8]",
    "k_restrict3_wide, band permutation / last workgroup / phantom row / chunks": "test_the_wide_cases_reach_every_dispatch_branch",
    "k_prolong_add<2>": "test_prolong_generic, test_prolong_on_colour_split_fields, test_node_transfers_of_linear_fields_and_adjointness",
    "k_prolong_add<3>": "test_prolong_generic, test_prolong_on_colour_split_fields, test_node_transfers_of_linear_fields_and_adjointness",
    "k_prolong_add3_pairs": "test_prolong_pairs_product, test_prolong_pairs_planes_per_workgroup, test_the_pairs_cases_reach_every_branch, "
                            "test_node_transfers_of_linear_fields_and_adjointness",
    "k_restrict_cell<2,true> <2,false> <3,true> <3,false>": "test_restrict_cell_forms, test_cell_transfers_of_linear_fields_and_adjointness, "
                                                            "test_the_cell_layouts_are_on_the_intended_side_of_pairs_aligned",
    "k_prolong_add_cell<2,true> <2,false> <3,true> <3,false>": "test_prolong_add_cell_forms, test_prolong_add_cell_every_parity_of_the_box, "
                                                               "test_cell_transfers_of_linear_fields_and_adjointness",
    "argument checks (no launch)": "test_node_transfer_argument_checks, test_cell_transfer_argument_checks",
}


def test_every_pinned_test_exists():
    for tests in PINS.values():
        for name in tests.split(", "):
            assert name.split("[")[0] in globals(), name
