"""The y-marching 2-D 5-point star (csrc/kernels_star2d.hip, route `ymarch` of examg_stencil_op) and the boundary kinds of the 5-point
benchmark on the GPU.

Kernel: bit for bit against the oracle's loops on random data and with equality against the exact reference on integer data, the whole
u, rhs and destination arrays (a write outside the box shows), on the debug build with the route forced on at every size
(examg_debug_star2d(1, chunk)); the route is asked before every call.  Rows of 1 .. 257 points and 1 .. 9 rows, forced chunks of 1, 2
and 4 rows and the launcher's rule, node and cell layouts (plain, padded, deep halo; the right-hand side without ghost layers), boxes that
reach the first and the last allocated rows, both recognised entry orders; permuted orders keep the generic kernel.  The product
library on one box just above the default threshold.  Boundary kinds against tests/star2d_ops.py; examples/exa4/jacobi2d_cell.exa4."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import stencil_cases as S  # noqa: E402
import test_gpu_stencil_asym as T  # noqa: E402
from star2d_ops import BC_DIRICHLET, BC_NEGATE, BC_NEUMANN, BC_VALUE_MINUS, Star2dOracleOps  # noqa: E402
from stencil_cases import APPLY, RESIDUAL, SMOOTH  # noqa: E402
from test_gpu_kernels import hip, hipd  # noqa: E402,F401  (fixtures)
from test_gpu_stencil_asym import ex, orc  # noqa: E402,F401  (fixtures)

from exastencils_amd import exa4  # noqa: E402
from exastencils_amd.layout import FieldLayout  # noqa: E402
from exastencils_amd.lib import ExprC, GeomC, ivec  # noqa: E402

pytestmark = pytest.mark.gpu

EX = os.path.join(ROOT, "examples", "exa4")
ROUTES = T.ROUTES + ("ymarch",)      # enum StencilRoute: the new route is appended
THRESHOLD = 1 << 20                  # YM_MIN_POINTS of csrc/kernels_star2d.hip: boxes from this many points take the route by default


def route(hipd, mode, lu, lf, ld, st, colour, b, e, in_place):
    sc = st.c_struct(hipd.ptr)
    r = hipd.L.examg_debug_stencil_route(int(mode), C.byref(lu.c_struct()), C.byref(lf.c_struct()) if lf is not None else None,
                                         C.byref(ld.c_struct()), C.byref(sc), int(colour), ivec(b), ivec(e), int(in_place), 0)
    return ROUTES[r]


@pytest.fixture()
def forced(hipd):
    """The debug build; the hook is back at the rule when the test ends."""
    yield hipd
    hipd.L.examg_debug_star2d(-1, 0)


ROW_POINTS = (1, 2, 63, 64, 65, 127, 128, 129, 130, 257)
ROWS = (1, 2, 3, 5, 9)
CHUNKS = (1, 2, 4, 0)      # 0: the launcher's rule
MODES = ((APPLY, -1), (RESIDUAL, -1), (SMOOTH, -1), (SMOOTH, 0), (SMOOTH, 1))


def _shape(which, n0, n1):
    """Cells of a node layout whose box `which` (test_gpu_stencil_asym.box) has n0 x n1 points; None where there is none."""
    s = {"inner": (n0 + 1, n1 + 1), "dup": (n0 - 1, n1 - 1), "odd": (n0 + 5, n1 + 2)}[which]
    return None if min(s) < 1 else s + (0,)


# (localization, layout, box): every node layout with every box, cell layouts with the loop bounds of a cell field
LAYOUT_CASES = [("node", lay, which) for lay in ("plain", "align2", "align16", "halo2") for which in ("inner", "dup", "odd")] + \
    [("cell", lay, "all") for lay in ("plain", "align2", "align16", "halo2")]


def _layouts(loc, lay, which, n0, n1):
    if loc == "node":
        shape = _shape(which, n0, n1)
        if shape is None:
            return None
        lu, lf = T.layouts(2, shape, lay)
        b, e = T.box(2, shape, which)
        return lu, lf, b, e
    g, gf, align = (2, 1, 0) if lay == "halo2" else (1, 0, T.ALIGN[lay])
    return FieldLayout.cell(2, (n0, n1), g, align=align), FieldLayout.cell(2, (n0, n1), gf, align=align), [0, 0, 0], [n0, n1, 1]


@pytest.mark.parametrize("data", T.DATA)
@pytest.mark.parametrize("loc,lay,which", LAYOUT_CASES, ids=["%s-%s-%s" % c for c in LAYOUT_CASES])
def test_ymarch_bitwise(forced, orc, ex, loc, lay, which, data):
    """Every row length with every row count; the chunk length and the entry order go round with them so that every row length meets
    every chunk length and both orders, every mode and colour each time."""
    R = T.ref_ops(data, orc, ex)
    ran = 0
    for i, n0 in enumerate(ROW_POINTS):
        for j, n1 in enumerate(ROWS):
            L = _layouts(loc, lay, which, n0, n1)
            if L is None:
                continue      # a box over the duplicate points has at least two points per direction: 9 x 4 shapes
            lu, lf, b, e = L
            assert (e[0] - b[0], e[1] - b[1]) == (n0, n1)
            chunk = CHUNKS[(i + j) % 4]
            order = ("mp", "pm")[(i // 4 + j) % 2]
            st = T.stencil("5", order, data, (n0 + 1, n1 + 1, 0))
            w = T.weight(st, data)
            forced.L.examg_debug_star2d(1, chunk)
            for mode, colour in MODES:
                in_place = colour >= 0
                assert route(forced, mode, lu, lf, lu, st, colour, b, e, in_place) == "ymarch", (n0, n1, mode, colour)
                g = T.host(forced, T._stencil_op_run(forced, data, lu, lf, st, w, mode, colour, b, e, in_place, 500 + ran))
                r = T.host(R, T._stencil_op_run(R, data, lu, lf, st, w, mode, colour, b, e, in_place, 500 + ran))
                T.assert_same(g, r, "%dx%d chunk %d %s mode %d colour %d" % (n0, n1, chunk, order, mode, colour))
            ran += 1
    assert ran == (36 if which == "dup" else 50)      # a box over the duplicate points has no row of one point


@pytest.mark.parametrize("chunk", CHUNKS)
def test_ymarch_every_chunk_length_on_one_box(forced, orc, chunk):
    """257 x 9 points over the duplicate layers (the first and the last allocated rows of the ghost-0 right-hand side), both orders."""
    lu, lf = T.layouts(2, (256, 8, 0), "plain")
    b, e = T.box(2, (256, 8, 0), "dup")
    forced.L.examg_debug_star2d(1, chunk)
    for order in ("mp", "pm"):
        st = S.convdiff5((256, 8, 0), order)
        w = S.free_weight(st)
        for mode, colour in MODES:
            assert route(forced, mode, lu, lf, lu, st, colour, b, e, colour >= 0) == "ymarch"
            g = T.host(forced, T._stencil_op_run(forced, "random", lu, lf, st, w, mode, colour, b, e, colour >= 0, 900))
            r = T.host(orc, T._stencil_op_run(orc, "random", lu, lf, st, w, mode, colour, b, e, colour >= 0, 900))
            T.assert_same(g, r, "chunk %d %s mode %d colour %d" % (chunk, order, mode, colour))


def test_permuted_orders_and_other_shapes_keep_the_generic_kernel(forced):
    lu, lf = T.layouts(2, (130, 10, 0), "plain")
    b, e = T.box(2, (130, 10, 0), "inner")
    forced.L.examg_debug_star2d(1, 0)
    for order in ("perm_a", "perm_b"):
        st = S.convdiff5((130, 10, 0), order)
        for mode, colour in MODES:
            assert route(forced, mode, lu, lf, lu, st, colour, b, e, colour >= 0) == "generic"
    st = S.convdiff5((130, 10, 0), "pm")
    assert route(forced, SMOOTH, lu, lf, lu, st, 0, b, e, False) == "generic"      # a coloured loop out of place
    ls = lu.split_x()
    assert route(forced, SMOOTH, ls, lf, ls, st, -1, b, e, False) == "generic"     # a layout transformation
    forced.L.examg_debug_star2d(0, 0)
    assert route(forced, SMOOTH, lu, lf, lu, st, -1, b, e, False) == "generic"     # the hook: never


def test_product_library_takes_the_route_just_above_the_threshold(hip, hipd, orc):
    hipd.L.examg_debug_star2d(-1, 0)
    shape = (1030, 1025, 0)      # the inner box: 1029 x 1024 points
    lu, lf = T.layouts(2, shape, "plain")
    b, e = T.box(2, shape, "inner")
    assert THRESHOLD <= (e[0] - b[0]) * (e[1] - b[1]) < THRESHOLD + THRESHOLD // 64
    st = S.convdiff5(shape, "pm")
    w = S.free_weight(st)
    for mode, colour in MODES:
        assert route(hipd, mode, lu, lf, lu, st, colour, b, e, colour >= 0) == "ymarch"
    below = T.box(2, (1030, 1017, 0), "inner")
    assert route(hipd, SMOOTH, lu, lf, lu, st, -1, below[0], below[1], False) == "generic"      # 1029 x 1016 points
    for mode, colour in ((SMOOTH, -1), (RESIDUAL, -1), (SMOOTH, 1)):
        g = T.host(hip, T._stencil_op_run(hip, "random", lu, lf, st, w, mode, colour, b, e, colour >= 0, 700))
        r = T.host(orc, T._stencil_op_run(orc, "random", lu, lf, st, w, mode, colour, b, e, colour >= 0, 700))
        T.assert_same(g, r, "product library mode %d colour %d" % (mode, colour))
    # with no hook, the small 2-D shapes of the existing route assertions stay where they were
    for small, lay, which in (((257, 40, 0), "plain", "inner"), ((60, 30, 0), "align2", "odd")):
        su, sf = T.layouts(2, small, lay)
        sb, se = T.box(2, small, which)
        for order in ("mp", "pm"):
            assert route(hipd, SMOOTH, su, sf, su, S.convdiff5(small, order), -1, sb, se, False) == "generic"


# -- boundary kinds ---------------------------------------------------------------------------------------------------------------------
def _geom(n, lo=-0.25):
    g = GeomC()
    for d in range(3):
        g.h[d] = 1.0 / n[d] if d < len(n) else 1.0
        g.pos_begin[d] = lo if d < len(n) else 0.0
    return g


POLY = ExprC.from_program([("nx", None), ("const", 10.0), ("y", None), ("*", None), ("+", None), ("x", None), ("ny", None), ("*", None), ("-", None)])
DPOLY = ExprC.from_program([("x", None), ("const", 3.0), ("y", None), ("*", None), ("+", None)])
CONST = ExprC.from_program([("const", 0.0)])
# sin(2 pi x_node) * sinh(2 pi): the upper wall of the benchmark
TOP = ExprC.from_program([("const", 2.0 * np.pi), ("nx", None), ("*", None), ("sin", None), ("const", float(np.sinh(2.0 * np.pi))), ("*", None)])
BC_LAYOUTS = [(2, (96, 48), 1, 2), (2, (6, 12), 1, 0), (2, (4, 3), 2, 0), (3, (20, 12, 6), 1, 2)]


def _bc_both(hip, l, fn, seed=31):
    outs = []
    for ops in (hip, Star2dOracleOps()):
        x = ops.new_array(l.size)
        ops.fill_random(x, seed)
        fn(ops, x)
        ops.synchronize()
        outs.append(np.array(ops.to_host(x), dtype=np.float64, copy=True))
    return outs


@pytest.mark.parametrize("nd,n,ghost,align", BC_LAYOUTS)
def test_value_minus_polynomial_programs_bitwise(hip, nd, n, ghost, align):
    l = FieldLayout.cell(nd, n, ghost, align=align)
    g = _geom(n)
    full = (1 << (2 * nd)) - 1
    for prog in (POLY, CONST):
        for mask in (full, 0b100110 & full, 1):
            got, want = _bc_both(hip, l, lambda ops, x: ops.apply_bc_cell(l.c_struct(), x, g, BC_VALUE_MINUS, prog, mask))
            assert np.array_equal(got, want), (mask,)
    # signed zero on the device: 0.0 - (+0.0) = +0.0, -(+0.0) = -0.0
    for kind, neg in ((BC_VALUE_MINUS, False), (BC_NEGATE, True)):
        x = hip.from_host(np.zeros(l.size))
        hip.apply_bc_cell(l.c_struct(), x, g, kind, CONST, full)
        hip.synchronize()
        a = np.asarray(hip.to_host(x))
        assert int(np.signbit(a).sum()) == (2 * sum(int(np.prod(n)) // n[d] for d in range(nd)) if neg else 0)


@pytest.mark.parametrize("nd,n,ghost,align", BC_LAYOUTS)
def test_faces_call_equals_single_face_launches(hip, nd, n, ghost, align):
    l = FieldLayout.cell(nd, n, ghost, align=align)
    g = _geom(n)
    full = (1 << (2 * nd)) - 1
    faces = [(BC_VALUE_MINUS, POLY), (BC_NEGATE, None), (BC_DIRICHLET, DPOLY), (BC_VALUE_MINUS, TOP), (BC_NEUMANN, None), (BC_VALUE_MINUS, CONST)]
    got, want = _bc_both(hip, l, lambda ops, x: ops.apply_bc_cell_faces(l.c_struct(), x, g, faces, full))
    for order in (range(2 * nd), reversed(range(2 * nd))):
        def single(ops, x):
            for f in order:
                ops.apply_bc_cell(l.c_struct(), x, g, faces[f][0], faces[f][1], 1 << f)
        one = _bc_both(hip, l, single)[0]
        assert np.array_equal(one, got)      # the device: one launch = the single-face launches, the libm face included
    # face 3 (the sin * sinh value) within the libm rule of test_sin_sinh_wall_within_the_libm_rule, everything else bit for bit
    shape = tuple(l.tot(d) for d in range(nd - 1, -1, -1))
    G, W = got.reshape(shape), want.reshape(shape)
    sl = (slice(l.ref(1) + n[1], l.ref(1) + n[1] + 1), slice(l.ref(0), l.ref(0) + n[0]))
    if nd == 3:
        sl = (slice(l.ref(2), l.ref(2) + n[2]),) + sl
    libm = np.zeros(shape, dtype=bool)
    libm[sl] = True
    assert np.array_equal(G[~libm], W[~libm])
    gval = np.sin((2.0 * np.pi) * (np.arange(n[0]) * g.h[0] + g.pos_begin[0])) * float(np.sinh(2.0 * np.pi))
    bound = 8.0 * np.spacing(np.abs(gval)) + 0.5 * np.spacing(np.abs(G[sl])) + 0.5 * np.spacing(np.abs(W[sl]))
    assert np.all(np.abs(G[sl] - W[sl]) <= bound)


@pytest.mark.parametrize("n", [(96, 48), (6, 12), (257, 5)])
def test_sin_sinh_wall_within_the_libm_rule(hip, n):
    """ghost = g - interior with g = sin(2 pi x_node) sinh(2 pi).  The device's g is within 8 ulp of the host's (the project's libm rule),
    and the subtraction rounds once on either side: |got - want| <= 8 ulp(g) + ulp(got) / 2 + ulp(want) / 2.  Where the interior is 0 the
    ghost IS g: 8 ulp of g alone."""
    l = FieldLayout.cell(2, n, 1)
    geo = _geom(n, 0.0)
    ref = Star2dOracleOps()
    for zero_interior in (True, False):
        def run(ops):
            x = ops.new_array(l.size)
            ops.fill_random(x, 77)
            if zero_interior:
                x = ops.from_host(np.zeros(l.size))
            ops.apply_bc_cell(l.c_struct(), x, geo, BC_VALUE_MINUS, TOP, 8)
            ops.synchronize()
            return np.array(ops.to_host(x), dtype=np.float64, copy=True).reshape(n[1] + 2, n[0] + 2)
        got, want = run(hip), run(ref)
        i = np.arange(n[0])
        gval = np.sin((2.0 * np.pi) * (i * geo.h[0] + 0.0)) * float(np.sinh(2.0 * np.pi))
        bound = 8.0 * np.spacing(np.abs(gval))
        if not zero_interior:
            bound = bound + 0.5 * np.spacing(np.abs(got[-1, 1:-1])) + 0.5 * np.spacing(np.abs(want[-1, 1:-1]))
        d = np.abs(got[-1, 1:-1] - want[-1, 1:-1])
        print("sin*sinh wall %s: max |got - want| / bound = %.3f" % (n, float(np.max(d / np.maximum(bound, 1e-300)))))
        assert np.all(d <= bound)
        assert np.array_equal(got[:-1], want[:-1])      # everything but the ghost row is untouched


def test_refusals_of_the_new_kind(hip):
    from exastencils_amd.lib import ExamgError

    l = FieldLayout.cell(2, (8, 6), 1)
    x = hip.new_array(l.size)
    g = _geom((8, 6))
    node = ExprC.from_program([("nx", None)])
    for call, words in (
            (lambda: hip.apply_bc_cell(l.c_struct(), x, g, BC_DIRICHLET, node, 15), "unknown opcode"),
            (lambda: hip.fill_expr_cell(l.c_struct(), x, g, node, [0, 0, 0], [8, 6, 1]), "unknown opcode"),
            (lambda: hip.apply_bc_cell_faces(l.c_struct(), x, g, [(BC_DIRICHLET, node)] * 4, 15), "unknown opcode"),
            (lambda: hip.apply_bc_cell_faces(l.c_struct(), x, g, [(7, None)] * 4, 15), "unknown kind 7"),
            (lambda: hip.apply_bc_cell(l.c_struct(), x, g, 3, CONST, 1), "unknown kind 3"),      # the new kind is 4; 3 stays no kind
            (lambda: hip.apply_bc_cell(FieldLayout.cell(2, (8, 6), 0).c_struct(), x, g, BC_VALUE_MINUS, CONST, 1), "no ghost layer"),
            (lambda: hip.vec_apply_bc_cell(2, l.c_struct(), x, g, BC_VALUE_MINUS, 15), "EXAMG_BC_VALUE_MINUS"),
            (lambda: hip.apply_bc_face(0, FieldLayout.face(2, (8, 6), 0, 1).c_struct(), x, g, BC_VALUE_MINUS, CONST, 15), "EXAMG_BC_VALUE_MINUS")):
        with pytest.raises(ExamgError, match=words):
            call()


# -- the own program ------------------------------------------------------------------------------------------------------------------------
def _own(ops, text=None, **kw):
    with open(os.path.join(EX, "jacobi2d_cell.exa4")) as f:
        src = f.read()
    from exastencils_amd import knowledge

    return exa4.Exa4Program(text(src) if text else src, knowledge.parse_file(os.path.join(EX, "jacobi2d_cell.knowledge")), ops=ops, **kw)


def test_own_program_on_hip_prints_its_golden(hip):
    from oracle import mg

    P = _own(hip)
    out = P.run()
    with open(os.path.join(ROOT, "tests", "golden", "own", "jacobi2d_cell.results")) as f:
        assert mg.compare_with_golden(out, f.read()) == []
    Q = _own(Star2dOracleOps())
    Q.run()
    assert len(P.printed_values) == len(Q.printed_values) == 11      # the Reals: the start residual and ten more
    for a, b in zip(P.printed_values, Q.printed_values):
        assert abs(a - b) <= 1e-10 * abs(b)


def test_own_program_fields_equal_with_the_route_off_and_on(forced):
    """20 iterations on the debug build: the generic kernel (the route off) and the y-march kernel (on at every size) leave the same bits
    in u and r."""
    fields = []
    for on in (0, 1):
        forced.L.examg_debug_star2d(on, 0)
        P = _own(forced, text=lambda s: s.replace("n >= 100", "n >= 20"), auto_graph=False)
        out = P.run()
        assert out[-1] == "20"
        u, r = P.fields[("u", 6)], P.fields[("r", 6)]
        forced.synchronize()
        fields.append([np.array(forced.to_host(u.data(u.active)), copy=True), np.array(forced.to_host(r.data(0)), copy=True)])
    assert np.array_equal(fields[0][0], fields[1][0]) and np.array_equal(fields[0][1], fields[1][1])
