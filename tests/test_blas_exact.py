"""The references of tests/blas_cases.py on their own, without a GPU: what the GPU comparison of tests/test_gpu_blas.py rests on.

Every reference is run against the oracle (OracleOps / CellOracleOps) on every case where the oracle has the operation -- set, axpby,
add_scalar, dot, sum, max_err, the expression fills, `apply bc`, the planes of `only dup on boundary`, pack, unpack, fill_random -- so a
wrong reference shows here.  The case tables are checked against the restated dispatch: every (kernel, tail, final stage) combination
reduction_plan can return is reached, the layouts of each pair differ in origin and row pitch, the elementwise table passes the
workgroup cap, the (a, b) pairs select all five forms.  The host check of expression programs (expr_ok) refuses 257 instructions
and a stack of 25; it runs without a device.
"""
import ctypes as C
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import blas_cases as B
import stencil_cases as S
from cell_ops import CellOracleOps

from exastencils_amd.lib import ExprC

BY_NAME = dict(ids=lambda c: c.name)


@pytest.fixture(scope="module")
def orc():
    return CellOracleOps()


def T(orc, a):
    return orc.from_host(np.array(a, dtype=np.float64, copy=True))


# ---- the tables ---------------------------------------------------------------------------------------------------------------------
def test_reduction_cases_reach_every_plan():
    """Every (kernel, tail shape, final-stage shape) reduction_plan can return is reached by the table (with the two empty boxes), each
    case takes the route its row names, and the capped cases are the capped ones."""
    reached = set()
    for c in B.REDUCTIONS:
        for sum_only in (False, True):
            p = B.plan_of(c, sum_only)
            if not (sum_only and c.lays == "split_y"):               # examg_sum reads x alone: y's split does not count
                assert (p.kernel, p.tail, p.final) == (c.kernel, c.tail, c.final), (c.name, p)
            assert p.capped == (c.name in B.CAPPED) and (p.nb == B.RED_MAX_BLOCKS) == p.capped
            assert p.K == p.serial + 18 + -(-p.nb // 256)
            reached.add((p.kernel, p.tail, p.final))
    lx, ly = B.layouts(B.REDUCTIONS[1])
    for box in B.EMPTY_BOXES:
        p = B.reduction_plan(box, lx, ly)
        reached.add((p.kernel, p.tail, p.final))
    assert reached == B.reachable_plans()
    n = {c.name: c.n for c in B.REDUCTIONS}
    assert n["127x9x4"][0] == B.ROW_MIN - 1 and n["128x7x3_even"][0] == B.ROW_MIN
    assert {c.begin[0] % 2 for c in B.REDUCTIONS if c.name.startswith("128x7x3")} == {0, 1}
    assert B.plan_of(next(c for c in B.REDUCTIONS if c.name == "130x48x45")).nb > 256
    assert B.plan_of(next(c for c in B.REDUCTIONS if c.name == "127x130x131")).serial > 1
    c = next(c for c in B.REDUCTIONS if c.name == "1030x3x2")
    assert B.plan_of(c).nb * 4 > c.n[1] * c.n[2]                      # more waves than rows
    assert all(max(c.n[0] * c.n[1] * c.n[2] for c in t) <= 1 << 22 for t in (B.REDUCTIONS, B.ELEMENTWISE))


def test_a_split_argument_forces_the_partial_kernel():
    for name in ("splitx_257x3x2", "splity_257x3x2"):
        c = next(c for c in B.REDUCTIONS if c.name == name)
        lx, ly = B.layouts(c)
        assert c.n[0] >= B.ROW_MIN and B.reduction_plan(B.box_of(c), lx, ly).kernel == "rows"      # the rows alone would qualify
        assert B.plan_of(c).kernel == "partial"
    assert B.plan_of(next(c for c in B.REDUCTIONS if c.name == "splitx_257x3x2"), sum_only=True).kernel == "partial"


@pytest.mark.parametrize("case", B.REDUCTIONS + B.ELEMENTWISE + B.MAXERR, **BY_NAME)
def test_layouts_of_a_pair_differ(case):
    lx, ly = (S.Lay(l) for l in B.layouts(case))
    fx, fy = B.layouts(case)
    origin = lambda L: L.ref[0] + L.tot[0] * (L.ref[1] + L.tot[1] * L.ref[2])
    assert origin(lx) != origin(ly) and lx.tot[0] != ly.tot[0]                     # origin and row pitch
    assert fx.ghost != fy.ghost
    assert (fx.communicates_dup, fx.communicates_ghost) != (fy.communicates_dup, fy.communicates_ghost)
    assert all(len({l.tot(d) for d in range(l.nd)}) == l.nd for l in (fx, fy))     # no two extents of an allocation alike


def test_elementwise_tables():
    big = next(c for c in B.ELEMENTWISE if c.name == "127x130x131")
    count = big.n[0] * big.n[1] * big.n[2]
    assert B.ELEMENTWISE_CAP < count <= 2 * B.ELEMENTWISE_CAP                       # exactly one trip past the cap
    c = B.ELEMENTWISE[0]
    assert c.begin[0] < 0 and B.layouts(c)[0].ghost[0] == 2
    assert [B.axpby_form(a, b) for a, b in B.AXPBY_SCALARS] == B.AXPBY_FORMS and set(B.AXPBY_FORMS) == {0, 1, 2, 3, 4}
    assert {(1.0, 1.0), (1.0, 0.0)} <= set(B.AXPBY_SCALARS) and any(b == 0.0 and math.copysign(1.0, b) < 0 for _, b in B.AXPBY_SCALARS)
    assert [B.axpby_dev_form(w, a, b) for w, a, b, s, f in B.AXPBY_DEV] == [f for *_, f in B.AXPBY_DEV]
    assert {(w, f) for w, *_, f in B.AXPBY_DEV} == {(0, 2), (0, 0), (0, 4), (1, 3), (1, 4)}
    q = B.DEV_NUM / B.DEV_DEN
    assert Fraction(q) != Fraction(B.DEV_NUM) / Fraction(B.DEV_DEN)                 # the quotient is inexact


# ---- elementwise references against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", ["int", "random"])
@pytest.mark.parametrize("case", B.ELEMENTWISE, **BY_NAME)
def test_elementwise_references_equal_the_oracle(orc, case, data):
    lx, ly = B.layouts(case)
    box = B.box_of(case)
    x, y = B.field(lx.size, data, 5), B.field(ly.size, data, 6)
    for a, b in B.AXPBY_SCALARS:
        t = T(orc, y)
        orc.axpby(lx.c_struct(), T(orc, x), ly.c_struct(), t, a, b, *box)
        want = B.ref_axpby(lx, x, ly, y, a, b, box)
        assert np.array_equal(orc.to_host(t), want), (a, b)
        if data == "int":
            assert np.array_equal(B.ref_axpby(lx, x, ly, y, a, b, box, exact=True), want), (a, b)      # the two references agree
    for which, a, b, sign, form in B.AXPBY_DEV:
        a2, b2 = B.dev_scalars(which, a, b, sign)
        t = T(orc, y)
        orc.axpby(lx.c_struct(), T(orc, x), ly.c_struct(), t, a2, b2, *box)
        assert np.array_equal(orc.to_host(t), B.ref_axpby(lx, x, ly, y, a2, b2, box, form=form))
    t = T(orc, x)
    orc.set(lx.c_struct(), t, -2.75, *box)
    assert np.array_equal(orc.to_host(t), B.ref_set(lx, x, -2.75, box))
    t = T(orc, y)
    orc.add_scalar(ly.c_struct(), t, -0.375, *box)
    assert np.array_equal(orc.to_host(t), B.ref_add_scalar(ly, y, -0.375, box, exact=data == "int"))
    assert np.array_equal(orc.to_host(t), B.ref_add_scalar(ly, y, -0.375, box))


# ---- reductions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", ["int", "random"])
@pytest.mark.parametrize("case", B.REDUCTIONS, **BY_NAME)
def test_reduction_references_against_the_oracle(orc, case, data):
    """Integer data: the oracle's loop equals the Python integer.  Random data: its serial loop of n terms stays within
    (n + 1) * 2^-53 * fsum(|terms|) of math.fsum -- the bound of the GPU test with K = n."""
    lx, ly = B.layouts(case)
    box = B.box_of(case)
    x, y = B.reduction_inputs(case.name, data)
    n = case.n[0] * case.n[1] * case.n[2]
    for sum_only in (False, True):
        want, unit = B.reduction_reference(case.name, data, sum_only)
        if sum_only:
            got = orc.scalar_value(orc.sum(lx.c_struct(), T(orc, x), *box))
        else:
            got = orc.scalar_value(orc.dot(lx.c_struct(), T(orc, x), ly.c_struct(), T(orc, y), *box))
        if data == "int":
            assert isinstance(want, int) and abs(want) < 1 << 31 and got == want
        else:
            assert abs(got - want) <= (n + 1) * unit


@pytest.mark.parametrize("name", B.NEEDLE_CASES)
def test_needles_sum_to_one(orc, name):
    case = next(c for c in B.REDUCTIONS if c.name == name)
    lx, ly = B.layouts(case)
    pts = B.needle_points(case)
    assert len({p for p, _ in pts}) == 6 and pts[-1][0][0] == -min(lx.ghost[0], ly.ghost[0]) < case.begin[0]
    if case.tail != "none":
        assert (pts[4][0][0] - case.begin[0]) % 2 == 0 and pts[4][0][0] == B.box_of(case)[1][0] - 1      # the tail element
    for p, box in pts:
        x, y = B.needle_field(lx, box, p), B.needle_field(ly, box, p)
        assert B.ref_reduction(lx, x, ly, y, box, True)[0] == 1 and B.ref_reduction(lx, x, None, None, box, True)[0] == 1
        assert orc.scalar_value(orc.dot(lx.c_struct(), T(orc, x), ly.c_struct(), T(orc, y), *box)) == 1.0
        assert orc.scalar_value(orc.sum(lx.c_struct(), T(orc, x), *box)) == 1.0


@pytest.mark.parametrize("case", B.MAXERR, **BY_NAME)
def test_max_err_reference_equals_the_oracle(orc, case):
    l = B.layouts(case)[0]
    expr = ExprC.from_program(B.prog(case.program))
    f = orc.max_err_expr_cell if case.lays == "cell" else orc.max_err_expr
    for where in B.maxerr_plants(case):
        a, want = B.maxerr_field(case, where)
        assert want == 3.0 and f(l.c_struct(), T(orc, a), B.MGEOM, expr, *B.box_of(case)).item() == want


# ---- the interpreter ------------------------------------------------------------------------------------------------------------------
def test_exact_programs_cover_the_exact_class():
    used = {n for p, _, _ in B.EXACT_PROGRAMS.values() for n, _ in p}
    assert used == set(B.EXACT_OPS)
    assert set(B.EXACT_OPS) | set(B.LIBM_OPS) == set(__import__("exastencils_amd.lib", fromlist=["OPS"]).OPS)
    p = B.EXACT_PROGRAMS["256_instructions"][0]
    assert len(p) == 256 == B.MAX_EXPR
    assert B.stack_depth(B.EXACT_PROGRAMS["depth_24"][0]) == 24
    assert [n for n, _ in B.EXACT_PROGRAMS["depth_24"][0][24:]] == ["/"] + ["-"] * 22
    # the operand order shows: swapping the operands of -, / changes the value at every point, max / min meet both x < y and x > y
    px, py, pz = B.positions(B.EGEOM, *B.EBOX)
    assert any(x < y for x in px for y in py) and any(x > y for x in px for y in py) and min(px) < 0 and min(py) < 0 and min(pz) < 0
    assert all(Fraction(4) / x != x / 4 for x in B.positions(B.PGEOM, *B.PBOX)[0])
    assert all(x.numerator == 1 for x in B.positions(B.PGEOM, *B.PBOX)[0])           # powers of two


@pytest.mark.parametrize("name", sorted(B.EXACT_PROGRAMS))
def test_exact_programs_equal_the_oracle(orc, name):
    program, geom, (b, e) = B.EXACT_PROGRAMS[name]
    want = B.exact_values(program, geom, b, e)
    l = B.EXPR_LAYOUT
    t = T(orc, np.full(l.size, B.SENTINEL))
    orc.fill_expr(l.c_struct(), t, geom, ExprC.from_program(program), b, e)
    exp = np.full(l.size, B.SENTINEL)
    B.view(l, exp)[B.box_index(l, b, e)] = want
    assert np.array_equal(orc.to_host(t), exp)
    want_cell = B.exact_values(program, geom, b, e, cell=True) if name != "4_div_by_x" else None
    if want_cell is not None:
        orc.fill_expr_cell(l.c_struct(), t, geom, ExprC.from_program(program), b, e)
        assert np.array_equal(B.view(l, orc.to_host(t))[B.box_index(l, b, e)], want_cell)


def test_programs_past_the_limits_are_refused():
    """257 instructions: ExprC.from_program, and the library for a structure that claims them; a stack of 25: the library (expr_ok runs
    on the host before anything else)."""
    from exastencils_amd import lib

    with pytest.raises(ValueError, match="257 instructions"):
        ExprC.from_program(B.long_program() + [("neg", None)])
    L = lib.load()
    l, x = B.EXPR_LAYOUT.c_struct(), np.zeros(B.EXPR_LAYOUT.size)
    b, e = B.EBOX
    call = lambda ex: L.examg_fill_expr(C.byref(l), x.ctypes.data, C.byref(B.EGEOM), C.byref(ex), lib.ivec(e), lib.ivec(b), None)
    ok = ExprC.from_program(B.long_program())
    assert call(ok) == 0 and not x.any()                      # accepted; the box is empty (end and begin exchanged): nothing is launched
    ok.n = 257
    assert call(ok) == 1 and b"too long" in L.examg_last_error()
    assert call(ExprC.from_program(B.deep_program(24))) == 0
    assert call(ExprC.from_program(B.deep_program(25))) == 1 and b"stack deeper than 24" in L.examg_last_error()


@pytest.mark.parametrize("fn", B.LIBM_OPS)
def test_libm_table_holds_for_the_oracle(orc, fn):
    measured, bound = B.LIBM_ULP[fn]
    assert bound == measured + 1 and measured <= 4
    l = B.LIBM_LAYOUT
    t = T(orc, np.zeros(l.size))
    orc.fill_expr(l.c_struct(), t, B.LGEOM, ExprC.from_program(B.libm_program(fn)), *B.LBOX)
    got = B.view(l, orc.to_host(t))[B.box_index(l, *B.LBOX)]
    err = B.ulp_error(got, B.libm_reference(fn))
    print("%s: oracle %.0f ulp, bound %d" % (fn, err, bound))
    assert err <= bound


# ---- boundary fills ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lname", sorted(B.FILL_LAYOUTS))
def test_boundary_fill_references_equal_the_oracle(orc, lname):
    from exastencils_amd.field import FN_POLY3D, FN_XSQ

    l = B.FILL_LAYOUTS[lname]
    expr = ExprC.from_program(B.FILL_PROGRAM)
    for mask in B.fill_masks(l.nd):
        t = T(orc, np.full(l.size, B.SENTINEL))
        orc.apply_dirichlet_expr(l.c_struct(), t, B.FGEOM, expr, mask)
        assert np.array_equal(orc.to_host(t), B.ref_boundary_fill(lname, mask, True)), mask
        # the oracle fills the planes of `only dup on boundary` with built-in functions only: the same points are written
        t = T(orc, np.full(l.size, B.SENTINEL))
        orc.fill_dup_faces(l.c_struct(), t, B.FGEOM, FN_POLY3D if l.nd == 3 else FN_XSQ, (), mask)
        assert np.array_equal(orc.to_host(t) != B.SENTINEL, B.ref_boundary_fill(lname, mask, False) != B.SENTINEL), mask
    full, dup = B.face_mask_array(l, (1 << 2 * l.nd) - 1, True), B.face_mask_array(l, (1 << 2 * l.nd) - 1, False)
    assert dup.sum() < full.sum() and not (dup & ~full).any()                      # the ghost layers make the difference
    assert not B.face_mask_array(l, 0, True).any()


def test_a_layout_without_duplicate_communication_keeps_its_duplicate_planes():
    """FieldLayout.node(communicates_dup=False) still has one duplicate layer per side: no zero-width case exists to add."""
    from exastencils_amd.layout import FieldLayout

    assert FieldLayout.node(3, (12, 10, 8), 1, communicates_dup=False).dup == (1, 1, 1)


# ---- data movers and the generator ----------------------------------------------------------------------------------------------------------
def test_pack_references_equal_the_oracle(orc):
    l = B.PACK_LAYOUT
    assert l.ghost == (2, 2, 2) and l.pad_l[0] + l.pad_r[0] > 0 and len({l.tot(d) for d in range(3)}) == 3
    x = np.arange(l.size, dtype=np.float64)
    boxes = B.pack_boxes()
    assert len(boxes) == 3 * 6
    for box in boxes:
        n = B.ref_pack(l, x, box).size
        buf = T(orc, np.full(n + 3, B.SENTINEL))
        orc.pack(l.c_struct(), T(orc, x), buf, *box)
        assert np.array_equal(orc.to_host(buf), np.concatenate([B.ref_pack(l, x, box), [B.SENTINEL] * 3]))
        src = np.arange(n + 3, dtype=np.float64) + 0.5
        t = T(orc, np.full(l.size, B.SENTINEL))
        orc.unpack(l.c_struct(), t, T(orc, src), *box)
        assert np.array_equal(orc.to_host(t), B.ref_unpack(l, np.full(l.size, B.SENTINEL), src, box))


def test_random_generator_restatements_agree(orc):
    """The numpy form equals the Python-integer form, and both the oracle's stream."""
    for seed in B.RANDOM_SEEDS:
        a = B.random_field(300, seed)
        assert a.tolist() == [B.random_value(seed, i) for i in range(300)] and -1.0 <= a.min() and a.max() < 1.0
        t = orc.new_array(300)
        orc.fill_random(t, seed)
        assert np.array_equal(orc.to_host(t), a)
    n = B.RANDOM_SIZES[-1]
    a = B.random_field(n, 1 << 63)
    assert [a[i] for i in (n - 3, n - 2, n - 1)] == [B.random_value(1 << 63, i) for i in (n - 3, n - 2, n - 1)]


def test_split_and_entry_transformations_are_inverses():
    for l in B.TRANSFORM_LAYOUTS.values():
        x = np.arange(l.size, dtype=np.float64)
        s = B.ref_split(l, x)
        assert s.size == l.split_x().size and np.array_equal(B.ref_unsplit(l, s), x)
        assert all(s[l.split_x().linear(i, j, 0)] == x[l.linear(i, j, 0)] for i in range(-l.ghost[0], 3) for j in (0, 2))
    assert {l.tot(0) % 2 for l in B.TRANSFORM_LAYOUTS.values()} == {0, 1}
    for K in B.SF_ENTRIES:
        for size in B.SF_SIZES:
            assert B.sf_layout(size).size == size
            src = np.arange(K * size, dtype=np.float64)
            aos = B.ref_transform_sf(src, size, K, True)
            assert aos[5 % size * K + K - 1] == src[(K - 1) * size + 5 % size]
            assert np.array_equal(B.ref_transform_sf(aos, size, K, False), src)
