"""GPU parity of the entry points of vector-valued cell fields (include/examg.h: examg_vec_*).  examg_vec_op and examg_vec_smooth
against their numpy restatement (tests/vector_ops.py), bit-identical over the WHOLE arrays -- a stray write outside the box, to the
other colour or to another component shows -- in both access widths (the debug library is told to take 8-byte accesses); the batched
transfers, boundary update and BLAS-1 loops against the scalar entry points of the same library, per component; examg_vec_dot against
math.fsum within the bound its reduction plan gives; refusals launch nothing."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import blas_cases as B
from vector_cases import ORDERS, PATTERNS, SHAPES, VecData, boxes, layouts
from vector_ops import SYS_APPLY, SYS_RESIDUAL, VectorOracleOps

from exastencils_amd import lib
from exastencils_amd.field import MatrixStencil
from exastencils_amd.layout import FieldLayout
from exastencils_amd.lib import ExamgError, GeomC


@pytest.fixture(scope="module")
def hip():
    from exastencils_amd.ops import HipOps

    return HipOps(0)


@pytest.fixture(scope="module")
def hipd():
    from exastencils_amd.ops import HipOps

    return HipOps(0, lib.DBG_LIB_PATH)


@pytest.fixture(scope="module")
def orc():
    return VectorOracleOps()


@pytest.fixture(params=["pairs", "narrow"])
def gpu(request, hip, hipd):
    if request.param == "pairs":
        yield hip
        return
    hipd.L.examg_debug_vec_narrow(1)
    try:
        yield hipd
    finally:
        hipd.L.examg_debug_vec_narrow(0)


def same(a, b, what):
    if not np.array_equal(a, b):
        d = np.abs(a - b)
        raise AssertionError("%s: %d of %d values differ, max abs %.3e" % (what, int((d > 0).sum()), d.size, d.max()))


def compare(gpu, orc, fn, what):
    """fn(ops) -> list of VecData after the calls under test; every array of each is compared whole."""
    g = fn(gpu)
    gpu.synchronize()
    c = fn(orc)
    for k, (sg, sc) in enumerate(zip(g, c)):
        for j, (x, y) in enumerate(zip(sg.arrays(), sc.arrays())):
            same(gpu.to_host(x), orc.to_host(y), "%s, call %d, array %d" % (what, k, j))


CASES = [(nd, n, cells, align, box) for nd, n, cells in SHAPES for align in (0, 2) for box in ("full", "interior")]
IDS = ["%dd-n%d-%s-a%d-%s" % (nd, n, "x".join(map(str, cells)), align, box) for nd, n, cells, align, box in CASES]


def vec_op_all(ops, nd, n, cells, align, box, ghost_other=1):
    lu, lo = layouts(nd, cells, align, ghost_other)
    b, e = boxes(nd, cells)[box]
    out = []
    for pattern in PATTERNS:
        for order in ORDERS:
            for mode in (SYS_APPLY, SYS_RESIDUAL):
                s = VecData(ops, nd, n, lu, lo, pattern, order)
                ops.vec_op(mode, n, lu.c_struct(), s.u, lo.c_struct(), s.f, lo.c_struct(), s.dst, s.M, b, e)
                out.append(s)
    return out


def vec_smooth_all(ops, nd, n, cells, align, box, ghost_other=1):
    lu, lo = layouts(nd, cells, align, ghost_other)
    b, e = boxes(nd, cells)[box]
    out = []
    for k, pattern in enumerate(PATTERNS):
        for order in ORDERS:
            for relax in (1.0, 0.8):
                for colours in ((0,), (1,), (0, 1)):
                    s = VecData(ops, nd, n, lu, lo, pattern, order)
                    for colour in colours:
                        ops.vec_smooth(n, lu.c_struct(), s.u, lo.c_struct(), s.f, s.M, relax, colour, b, e)
                    out.append(s)
    return out


@pytest.mark.parametrize("nd,n,cells,align,box", CASES, ids=IDS)
def test_vec_op_bitwise(gpu, orc, nd, n, cells, align, box):
    compare(gpu, orc, lambda ops: vec_op_all(ops, nd, n, cells, align, box), "vec_op")


@pytest.mark.parametrize("nd,n,cells,align,box", CASES, ids=IDS)
def test_vec_smooth_bitwise(gpu, orc, nd, n, cells, align, box):
    compare(gpu, orc, lambda ops: vec_smooth_all(ops, nd, n, cells, align, box), "vec_smooth")


@pytest.mark.parametrize("nd,n,cells", SHAPES, ids=["%dd-n%d" % (s[0], s[1]) for s in SHAPES])
@pytest.mark.parametrize("align", [0, 2])
def test_rhs_dst_and_coefficients_in_a_layout_without_ghost_layers(hip, orc, nd, n, cells, align):
    """The other origin parity: without alignment padding the pairs of the arguments do not line up with those of the unknowns."""
    for fn in (vec_op_all, vec_smooth_all):
        compare(hip, orc, lambda ops: fn(ops, nd, n, cells, align, "interior", 0), fn.__name__)


def test_empty_box_is_a_no_op(hip, orc):
    nd, n, cells = SHAPES[0]
    lu, lo = layouts(nd, cells, 2)

    def run(ops):
        s = VecData(ops, nd, n, lu, lo)
        ops.vec_op(SYS_RESIDUAL, n, lu.c_struct(), s.u, lo.c_struct(), s.f, lo.c_struct(), s.dst, s.M, [3, 2, 0], [3, 5, 1])
        ops.vec_smooth(n, lu.c_struct(), s.u, lo.c_struct(), s.f, s.M, 1.0, 0, [0, 4, 0], [9, 4, 1])
        ops.vec_set(n, lo.c_struct(), s.dst, 5.0, [5, 0, 0], [5, 6, 1])
        ops.vec_axpby(n, lo.c_struct(), s.f, lo.c_struct(), s.dst, 2.0, 1.0, [0, 6, 0], [9, 6, 1])
        return [s]

    compare(hip, orc, run, "empty box")
    s = VecData(hip, nd, n, lu, lo)
    out = hip.from_host(np.array([np.nan]))
    hip.vec_dot(n, lu.c_struct(), s.u, lo.c_struct(), s.f, [2, 2, 0], [2, 5, 1], out=out)
    assert float(hip.to_host(out)[0]) == 0.0


# -- the batched entry points against the scalar ones of the same library --------------------------------------------------------------
@pytest.mark.parametrize("nd,n,cells", SHAPES, ids=["%dd-n%d" % (s[0], s[1]) for s in SHAPES])
@pytest.mark.parametrize("align", [0, 2])
def test_batched_entry_points_equal_the_scalar_ones_per_component(hip, nd, n, cells, align):
    """One launch over n components writes, on every component, the bits of the scalar entry point called on that component: set, the
    forms of axpby (copy, a * x, y + a * x, y - a * x, x + b * y, a * x + b * y), the cell transfers, the Neumann update with a partial
    face mask and with all faces."""
    lf = FieldLayout.cell(nd, cells, 1, align=align)
    lo = FieldLayout.cell(nd, cells, 2 if align else 0, align=align)
    coarse = tuple(c // 2 for c in cells)
    lc = FieldLayout.cell(nd, coarse, 1, align=align)
    fb, fe = boxes(nd, cells)["interior"]
    cb, ce = boxes(nd, coarse)["full"]
    pb, pe = [1, 0, 0], [cells[0] - 1, cells[1], cells[2] if nd == 3 else 1]      # odd begin: the fine pairs of the ends are halves
    geom = GeomC()
    LF, LO, LC = lf.c_struct(), lo.c_struct(), lc.c_struct()

    def fresh(l, seed):
        v = hip.new_array(n * l.size)
        hip.fill_random(v, seed)
        return v, [v[c * l.size:(c + 1) * l.size].clone() for c in range(n)]

    def check(v, parts, l, what):
        hip.synchronize()
        for c in range(n):
            same(hip.to_host(v[c * l.size:(c + 1) * l.size]), hip.to_host(parts[c]), "%s, component %d" % (what, c))

    F, Fs = fresh(lf, 1)
    O, Os = fresh(lo, 2)
    Cv, Cs = fresh(lc, 3)
    for a, b_ in ((1.0, 0.0), (0.3, 0.0), (0.75, 1.0), (-0.75, 1.0), (1.0, 0.3), (0.5, -1.5)):
        hip.vec_axpby(n, LO, O, LF, F, a, b_, fb, fe)
        for c in range(n):
            hip.axpby(LO, Os[c], LF, Fs[c], a, b_, fb, fe)
        check(F, Fs, lf, "axpby a = %r, b = %r" % (a, b_))
    hip.vec_restrict_cell(n, LF, F, LC, Cv, 0.5, cb, ce)
    for c in range(n):
        hip.restrict_cell(LF, Fs[c], LC, Cs[c], 0.5, cb, ce)
    check(Cv, Cs, lc, "restrict_cell")
    for box in ((fb, fe), (pb, pe)):
        hip.vec_prolong_add_cell(n, LC, Cv, LF, F, *box)
        for c in range(n):
            hip.prolong_add_cell(LC, Cs[c], LF, Fs[c], *box)
        check(F, Fs, lf, "prolong_add_cell")
    for mask in (0b100110 if nd == 3 else 0b0110, (1 << (2 * nd)) - 1):
        hip.vec_apply_bc_cell(n, LF, F, geom, lib.BC_NEUMANN, mask)
        for c in range(n):
            hip.apply_bc_cell(LF, Fs[c], geom, lib.BC_NEUMANN, None, mask)
        check(F, Fs, lf, "apply_bc_cell mask 0x%x" % mask)
    hip.vec_set(n, LO, O, -2.5, fb, fe)
    for c in range(n):
        hip.set(LO, Os[c], -2.5, fb, fe)
    check(O, Os, lo, "set")
    check(Cv, Cs, lc, "the coarse field at the end")


@pytest.mark.parametrize("nd,n,cells,begin", [(3, 3, (37, 5, 3), (0, 0, 0)), (2, 2, (130, 6), (0, 0, 0)), (2, 2, (130, 6), (1, 1, 0))],
                         ids=["37x5x3-n3", "130x6-n2", "129x5-n2-odd-begin"])
def test_vec_dot_within_the_bound_of_its_reduction_plan(hip, nd, n, cells, begin):
    """|result - fsum(products)| <= (K + n) * 2^-53 * fsum(|products|): one rounding per product, n - 1 additions in the cell, K additions
    in the tree -- K the longest chain of the launch plan of examg_dot on the same box (blas_cases.reduction_plan), which examg_vec_dot
    takes."""
    lx, ly = FieldLayout.cell(nd, cells, 1), FieldLayout.cell(nd, cells, 0, align=2)
    b, e = list(begin), [cells[0], cells[1], cells[2] if nd == 3 else 1]
    x, y = hip.new_array(n * lx.size), hip.new_array(n * ly.size)
    hip.fill_random(x, 11)
    hip.fill_random(y, 12)
    got = float(hip.to_host(hip.vec_dot(n, lx.c_struct(), x, ly.c_struct(), y, b, e))[0])
    hx, hy = hip.to_host(x).reshape((n,) + lx.shape_zyx), hip.to_host(y).reshape((n,) + ly.shape_zyx)

    def box_of(a, l):
        return a[(slice(None),) + tuple(slice(b[d] + l.ref(d), e[d] + l.ref(d)) for d in (2, 1, 0))]

    ax, ay = box_of(hx, lx).reshape(-1), box_of(hy, ly).reshape(-1)
    assert ax.size == n * (e[0] - b[0]) * (e[1] - b[1]) * (e[2] - b[2])
    from fractions import Fraction       # the reference sum in exact rational arithmetic

    exact = sum(Fraction(float(p)) * Fraction(float(q)) for p, q in zip(ax, ay))
    abs_sum = math.fsum(abs(float(p) * float(q)) for p, q in zip(ax, ay))
    plan = B.reduction_plan((b, e), lx, ly)
    assert plan.kernel == ("rows" if e[0] - b[0] >= B.ROW_MIN else "partial")
    bound = (plan.K + n) * 2.0 ** -53 * abs_sum
    err = abs(float(Fraction(got) - exact))
    print("vec_dot %s: error %.3e, bound %.3e (K = %d)" % (cells, err, bound, plan.K))
    assert err <= bound


# -- refusals --------------------------------------------------------------------------------------------------------------------
def _stencil(n, entries, lg=None):
    """entries: [(offset, {(c, d): (k, g)})]"""
    elems = []
    for _, el in entries:
        m = [[None] * n for _ in range(n)]
        for (c, d), v in el.items():
            m[c][d] = v
        elems.append(m)
    return MatrixStencil(n, [o for o, _ in entries], elems, lg)


def _diag(n, v):
    return {(c, c): (v, None) for c in range(n)}


def _refusals():
    nd, cells, n = 2, (8, 6), 2
    lu, lo = layouts(nd, cells, 0)
    centre = ((0, 0, 0), _diag(n, 4.0))
    left, right = ((-1, 0, 0), _diag(n, -1.0)), ((1, 0, 0), _diag(n, -1.0))
    good = dict(n=n, lu=lu, lf=lo, ld=lo, lg=lo, ent=[centre, left, right], box=([0, 0, 0], [8, 6, 1]), dst="dst", field_at=None)
    split = lo.c_struct()
    split.transform = 1          # EXAMG_LAYOUT_SPLIT_X
    other = FieldLayout.cell(nd, (10, 6), 1)
    return [
        ("n = 1", dict(good, n=1), "2 or 3", "both"),
        ("n = 4", dict(good, n=4), "2 or 3", "both"),
        ("node layout", dict(good, lf=FieldLayout.node(nd, cells, 0)), "not a cell layout", "both"),
        ("colour-split layout", dict(good, lf=split), "colour-split", "both"),
        ("3-D rhs layout", dict(good, lf=FieldLayout.cell(3, (8, 6, 2), 0)), "dimensions", "both"),
        ("rhs layout of another size", dict(good, lf=other), "rhs layout has", "both"),
        ("coefficient layout of another size", dict(good, lg=other, field_at=(0, (0, 1))), "coefficient layout has", "both"),
        ("dst layout of another size", dict(good, ld=other), "dst layout has", "op"),
        ("u without ghost layer", dict(good, lu=FieldLayout.cell(nd, cells, 0)), "ghost layer", "both"),
        ("off-axis entry", dict(good, ent=[centre, ((1, 1, 0), _diag(n, -1.0))]), "not an axis entry", "both"),
        ("reach-2 entry", dict(good, ent=[centre, ((2, 0, 0), _diag(n, -1.0))]), "not an axis entry", "both"),
        ("z entry in 2-D", dict(good, ent=[centre, ((0, 0, 1), _diag(n, -1.0))]), "not an axis entry", "both"),
        ("repeated entry", dict(good, ent=[centre, left, left]), "repeats an offset", "both"),
        ("no centre entry", dict(good, ent=[left, right]), "no centre entry", "both"),
        ("off-centre entry off the diagonal", dict(good, ent=[centre, ((1, 0, 0), {(0, 0): (-1.0, None), (0, 1): (0.5, None)})]), "off the diagonal", "both"),
        ("field element off the centre", dict(good, ent=[centre, left], field_at=(1, (1, 1))), "centre entry only", "both"),
        ("box leaves the allocation of u", dict(good, box=([-1, 0, 0], [8, 6, 1])), "leaves the allocation of the unknowns", "both"),
        ("box leaves the rhs allocation", dict(good, lu=FieldLayout.cell(nd, cells, 2), lf=FieldLayout.cell(nd, cells, 0), ld=FieldLayout.cell(nd, cells, 2),
                                               box=([-1, 0, 0], [8, 6, 1])), "leaves the rhs allocation", "both"),
        ("dst is u", dict(good, ld=lu, dst="u"), "overlaps the unknowns", "op"),
        ("dst is f", dict(good, dst="f"), "overlaps the right-hand side", "op"),
    ]


# (the smoother has no destination: the refusals about one are cases of the operator alone)
REFUSAL_CASES = [(entry,) + r[:3] for r in _refusals() for entry in ("op", "smooth") if not (r[3] == "op" and entry == "smooth")]


@pytest.mark.parametrize("entry,name,args,text", REFUSAL_CASES, ids=["%s-%s" % (c[0], c[1].replace(" ", "-")) for c in REFUSAL_CASES])
def test_refusals_launch_nothing(hip, entry, name, args, text):
    """Each refusal returns its error (examg_last_error in the exception) and leaves every array as it was."""
    big = FieldLayout.cell(3, (12, 8, 2), 2)          # every array large enough for four components of any of the layouts
    t = [hip.new_array(4 * big.size) for _ in range(4)]
    for k, a in enumerate(t):
        hip.fill_random(a, 70 + k)
    before = [hip.to_host(a).copy() for a in t]
    arrays = dict(u=t[0], f=t[1], dst=t[2])
    n = args["n"]
    ent = args["ent"]
    if args["field_at"]:
        k, cd = args["field_at"]
        ent = [(o, dict(el)) for o, el in ent]
        ent[k][1][cd] = (None, t[3])
    M = _stencil(2, ent, args["lg"])          # the tables have rows of two; a refused n never reads them
    cs = lambda l: l if not hasattr(l, "c_struct") else l.c_struct()
    b, e = args["box"]
    with pytest.raises(ExamgError, match=text):
        if entry == "op":
            hip.vec_op(SYS_RESIDUAL, n, cs(args["lu"]), arrays["u"], cs(args["lf"]), arrays["f"], cs(args["ld"]), arrays[args["dst"]], M, b, e)
        else:
            hip.vec_smooth(n, cs(args["lu"]), arrays["u"], cs(args["lf"]), arrays["f"], M, 1.0, 0, b, e)
    hip.synchronize()
    for k, a in enumerate(t):
        same(hip.to_host(a), before[k], "array %d after the refused call" % k)


def test_batched_refusals_launch_nothing(hip):
    l = FieldLayout.cell(2, (8, 6), 1)
    node = FieldLayout.node(2, (8, 6), 1)
    lc = FieldLayout.cell(2, (4, 3), 1)
    x, y, c = hip.new_array(4 * node.size), hip.new_array(4 * node.size), hip.new_array(4 * lc.size)
    for k, a in enumerate((x, y, c)):
        hip.fill_random(a, 90 + k)
    before = [hip.to_host(a).copy() for a in (x, y, c)]
    L, LC, geom = l.c_struct(), lc.c_struct(), GeomC()
    b, e = [0, 0, 0], [8, 6, 1]
    calls = [
        (lambda: hip.vec_set(4, L, x, 1.0, b, e), "2 or 3"),
        (lambda: hip.vec_set(2, L, x, 1.0, [-2, 0, 0], e), "leaves the allocation"),
        (lambda: hip.vec_axpby(1, L, x, L, y, 1.0, 1.0, b, e), "2 or 3"),
        (lambda: hip.vec_set(2, node.c_struct(), x, 1.0, b, e), "examg_vec_set: a cell layout has no duplicate layers"),
        (lambda: hip.vec_axpby(2, L, x, node.c_struct(), y, 1.0, 1.0, b, e), "examg_vec_axpby: a cell layout has no duplicate layers"),
        (lambda: hip.vec_dot(2, node.c_struct(), x, L, y, b, e), "examg_vec_dot: a cell layout has no duplicate layers"),
        (lambda: hip.vec_prolong_add_cell(2, LC, c, node.c_struct(), x, b, e), "examg_vec_prolong_add_cell: a cell layout has no duplicate layers"),
        (lambda: hip.vec_axpby(2, L, x, L, y, 1.0, 1.0, b, [8, 9, 1]), "leaves an allocation"),
        (lambda: hip.vec_dot(5, L, x, L, y, b, e), "2 or 3"),
        (lambda: hip.vec_restrict_cell(4, L, x, LC, c, 1.0, b, [4, 3, 1]), "2 or 3"),
        (lambda: hip.vec_restrict_cell(2, L, x, LC, c, 1.0, b, [6, 3, 1]), "leaves an allocation"),
        (lambda: hip.vec_restrict_cell(2, node.c_struct(), x, LC, c, 1.0, b, [4, 3, 1]), "examg_vec_restrict_cell: a cell layout has no duplicate layers"),
        (lambda: hip.vec_prolong_add_cell(0, LC, c, L, x, b, e), "2 or 3"),
        (lambda: hip.vec_prolong_add_cell(2, LC, c, L, x, b, [8, 9, 1]), "leaves an allocation"),
        (lambda: hip.vec_apply_bc_cell(4, L, x, geom, lib.BC_NEUMANN, 0xF), "2 or 3"),
        (lambda: hip.vec_apply_bc_cell(2, L, x, geom, lib.BC_DIRICHLET, 0xF), "NEUMANN only"),
        (lambda: hip.vec_apply_bc_cell(2, L, x, geom, lib.BC_NEGATE, 0xF), "NEUMANN only"),
        (lambda: hip.vec_apply_bc_cell(2, FieldLayout.cell(2, (8, 6), 0).c_struct(), x, geom, lib.BC_NEUMANN, 0xF), "no ghost layer"),
    ]
    for call, text in calls:
        with pytest.raises(ExamgError, match=text):
            call()
    hip.synchronize()
    for k, a in enumerate((x, y, c)):
        same(hip.to_host(a), before[k], "array %d after the refused calls" % k)


def test_a_stencil_of_constants_needs_no_coefficient_layout(hip, orc):
    """A caller of the C ABI may leave `lg` zeroed when no element has a coefficient field."""
    import ctypes as C

    nd, n, cells = 2, 2, (10, 6)
    lu, lo = layouts(nd, cells, 0)
    b, e = [0, 0, 0], [10, 6, 1]
    M = _stencil(n, [((0, 0, 0), _diag(n, 4.0)), ((-1, 0, 0), _diag(n, -1.0)), ((0, 1, 0), {(0, 0): (-1.5, None)})])

    def arrays(ops):
        t = [ops.new_array(n * lu.size), ops.new_array(n * lo.size), ops.new_array(n * lo.size)]
        for k, a in enumerate(t):
            ops.fill_random(a, 60 + k)
        return t

    u, f, d = arrays(hip)
    mc = M.c_struct(hip.ptr)          # no default layout: lg stays zeroed
    assert mc.lg.nd == 0
    L_u, L_o = lu.c_struct(), lo.c_struct()
    lib.check(hip.L.examg_vec_op(SYS_RESIDUAL, n, C.byref(L_u), hip.ptr(u), C.byref(L_o), hip.ptr(f), C.byref(L_o), hip.ptr(d), C.byref(mc),
                                 lib.ivec(b), lib.ivec(e), hip._stream()), "examg_vec_op")
    lib.check(hip.L.examg_vec_smooth(n, C.byref(L_u), hip.ptr(u), C.byref(L_o), hip.ptr(f), C.byref(mc), 0.8, 1, lib.ivec(b), lib.ivec(e),
                                     hip._stream()), "examg_vec_smooth")
    hip.synchronize()
    uo, fo, do = arrays(orc)
    orc.vec_op(SYS_RESIDUAL, n, L_u, uo, L_o, fo, L_o, do, M, b, e)
    orc.vec_smooth(n, L_u, uo, L_o, fo, M, 0.8, 1, b, e)
    for k, (x, y) in enumerate(((u, uo), (f, fo), (d, do))):
        same(hip.to_host(x), orc.to_host(y), "array %d" % k)


# -- the interpreted own programs on the HIP kernels ------------------------------------------------------------------------------
import os  # noqa: E402

from exastencils_amd import exa4  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _program(nd, hi, ops):
    with open(os.path.join(ROOT, "examples", "exa4", "optflow%dd_vec.exa4" % nd)) as fh:
        return exa4.Exa4Program(fh.read(), dict(dimensionality=nd, minLevel=2, maxLevel=hi), ops=ops)


@pytest.mark.parametrize("nd,hi", [(2, 8), (3, 6)])
def test_own_vector_examples_print_the_golden_lines_on_the_gpu(hip, nd, hi):
    with open(os.path.join(ROOT, "tests", "golden", "Application_OpticalFlow%dD.results" % nd)) as fh:
        golden = fh.read()
    assert "\n".join(_program(nd, hi, hip).run()) + "\n" == golden


@pytest.mark.parametrize("nd,hi", [(2, 5), (3, 4)])
def test_flow_after_one_cycle_equals_the_restatement_bit_for_bit(hip, orc, nd, hi):
    """Coefficients, right-hand side and one V-cycle at levels 2..hi on both kernel layers: every component of `flow` on every level, ghost
    cells included (the restatement adds the terms of vec_dot in the library's order, so the coarse solver takes the same steps).  The two
    images are computed once, on the restatement, and handed to both runs: they are sums of sin and cos, and the device's sin and cos are
    not libm's to the last bit -- an input of the feature, not a loop of it."""
    ref = _program(nd, hi, orc)
    ref.call("Images", hi)
    images = {name: orc.to_host(ref.fields[(name, hi)].data()).copy() for name in ("first", "second")}

    def run(ops):
        P = _program(nd, hi, ops)
        for name, a in images.items():
            P.fields[(name, hi)].data().copy_(ops.from_host(a))
        P.call("Data", hi)
        P.call("Cycle", hi)
        ops.synchronize()
        return P

    G, C = run(hip), run(orc)
    assert np.abs(hip.to_host(G.fields[("flow", hi)].data())).max() > 0.0
    for lvl in range(2, hi + 1):
        same(hip.to_host(G.fields[("flow", lvl)].data()), orc.to_host(C.fields[("flow", lvl)].data()), "flow@%d" % lvl)


@pytest.mark.parametrize("nd,n,cells", [(3, 3, (37, 5, 3)), (2, 2, (130, 6)), (2, 2, (129, 5)), (2, 2, (300, 40))],
                         ids=["37x5x3-n3", "130x6-n2", "129x5-n2", "300x40-n2"])
def test_vec_dot_has_the_bits_of_the_restated_reduction_tree(hip, orc, nd, n, cells):
    lx, ly = FieldLayout.cell(nd, cells, 1), FieldLayout.cell(nd, cells, 0, align=2)
    b, e = [0, 0, 0], [cells[0], cells[1], cells[2] if nd == 3 else 1]

    def run(ops):
        x, y = ops.new_array(n * lx.size), ops.new_array(n * ly.size)
        ops.fill_random(x, 21)
        ops.fill_random(y, 22)
        return float(ops.to_host(ops.vec_dot(n, lx.c_struct(), x, ly.c_struct(), y, b, e))[0])

    assert run(hip) == run(orc)
