"""The kernels of axis-aligned non-uniform grids on the MI355X against the numpy restatement (tests/grid_ops.py), bit for bit.

  examg_axis_op    the 3-D star stencil (the finite-difference operator of examples/exa4/poisson3d_nonuniform.exa4 on random node
                   tables that differ per axis, entries in the declared and in a shuffled order) on BOTH kernels: all three modes, both
                   weight forms, colour -1, 0, 1, the coloured smoother in place; boxes 131 x 11 x 9 (two x windows with a remainder of 3,
                   rows that do not fill the last workgroup, more than one z chunk), 1 x 1 x 1 and 2 x 1 x 3, begins off 0.  The generic
                   kernel on a 27-entry reach-1 stencil with 32 terms at 19 x 7 x 5 and on 5- and 9-entry stencils at 67 x 9.  u, rhs
                   and dst each in a layout of its own; the whole dst array is compared (sentinels outside the box), every input with
                   its copy.
  refusals         an error, examg_axis_route -1, and nothing is written.
  _grid entry points   arithmetic programs (x * y + wx * wz - z) are exact; a transcendental one follows numpy as tests/test_gpu_kernels.py
                   compares such programs (8 ulp of the magnitude).
  programs         the two example programs print the lines of the restatement's run; the cycle replayed from a hipGraph prints them too."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import grid_cases as G  # noqa: E402
import nonlinear_cases as N  # noqa: E402
from grid_ops import APPLY, AXIS_GENERIC, AXIS_STAR, RESIDUAL, SMOOTH, GridOracleOps  # noqa: E402

from exastencils_amd.grid import GHOST, AxisGrid  # noqa: E402
from exastencils_amd.layout import FieldLayout  # noqa: E402
from exastencils_amd.lib import ExamgError, ExprC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from exastencils_amd.ops import HipOps

    return HipOps(0)


@pytest.fixture(scope="module")
def orc():
    return GridOracleOps()


def host(ops, t):
    ops.synchronize()
    return np.array(ops.to_host(t), dtype=np.float64, copy=True)


def same_bits(got, want, what):
    if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
        bad = got.view(np.uint64) != want.view(np.uint64)
        raise AssertionError("%s: %d of %d values differ, max abs %.3e" % (what, int(bad.sum()), bad.size, float(np.nanmax(np.abs(got - want)[bad]))))


def run(ops, mode, data, lays, st, w, colour, b, e, route):
    """One examg_axis_op on kernel layer `ops` from the host arrays data = (u, f, dst); the host copies of (u, f, dst) afterwards.  The
    coloured smoother runs in place: dst is u."""
    lu, lf, ld = [x.c_struct() for x in lays]
    u, f, dst = [ops.from_host(a.copy()) for a in data]
    if mode == SMOOTH and colour >= 0:
        ld, dst = lu, u
    ops.axis_op(mode, lu, u, lf if mode != APPLY else None, f if mode != APPLY else None, ld, dst, st, w, colour, b, e, route=route)
    return host(ops, u), host(ops, f), host(ops, dst)


def check_all_forms(hip, orc, st, nd, ext, begin, route, what):
    shape, b, e = N.geometry(nd, ext, begin)
    lays = G.layouts(nd, shape)
    rng = np.random.default_rng(11)
    data = [rng.uniform(-1.0, 1.0, int(l.size)) for l in lays]
    data[2][:] = N.SENTINEL
    assert hip.axis_route(SMOOTH, *[x.c_struct() for x in lays], st, -1, b, e, route=route) == route
    n = 0
    for mode in (APPLY, RESIDUAL, SMOOTH):
        for wform in ((0, 1) if mode == SMOOTH else (0,)):
            for colour in (-1, 0, 1):
                s = st.with_wform(wform)
                got = run(hip, mode, data, lays, s, 0.8, colour, b, e, route)
                want = run(orc, mode, data, lays, s, 0.8, colour, b, e, None)
                tag = "%s mode %d wform %d colour %d" % (what, mode, wform, colour)
                for g, w_, name in zip(got, want, ("u", "rhs", "dst")):
                    same_bits(g, w_, tag + " " + name)
                if not (mode == SMOOTH and colour >= 0):
                    same_bits(got[0], data[0], tag + " u untouched")
                same_bits(got[1], data[1], tag + " rhs untouched")
                if colour < 0:      # (a colour may have no point in a box of one)
                    assert np.count_nonzero(got[2] != data[2]) > 0
                n += 1
    return n


STAR_BOXES = [("131x11x9", (131, 11, 9), (2, 1, 3)), ("1x1x1", (1, 1, 1), (1, 2, 1)), ("2x1x3", (2, 1, 3), (3, 1, 2))]


@pytest.mark.parametrize("route", [AXIS_GENERIC, AXIS_STAR], ids=["generic", "star"])
@pytest.mark.parametrize("name,ext,begin", STAR_BOXES, ids=[b[0] for b in STAR_BOXES])
def test_star_stencil_on_both_kernels(hip, orc, name, ext, begin, route):
    shape, _, _ = N.geometry(3, ext, begin)
    grid = G.random_grid(3, shape, 3)
    st = G.separated(G.fd_text(3), 3, grid)
    assert len(st.terms) == 12
    n = check_all_forms(hip, orc, st, 3, ext, begin, route, name)
    n += check_all_forms(hip, orc, G.permuted(st, [4, 1, 6, 0, 3, 5, 2]), 3, ext, begin, route, name + " shuffled")
    assert n == 24


def test_finite_volume_star_stencil_routes_equal(hip, orc):
    """Every term of the finite-volume operator has a table of each axis."""
    ext, begin = (70, 6, 5), (1, 1, 1)
    shape, _, _ = N.geometry(3, ext, begin)
    st = G.separated(G.fv_text(3), 3, G.random_grid(3, shape, 5))
    for route in (AXIS_GENERIC, AXIS_STAR):
        check_all_forms(hip, orc, st, 3, ext, begin, route, "fv")


def test_generic_kernel_on_a_full_stencil(hip, orc):
    ext, begin = (19, 7, 5), (1, 2, 1)
    shape, _, _ = N.geometry(3, ext, begin)
    st = G.full_stencil(3, shape, 21, 5)
    assert len(st.offsets) == 27 and len(st.terms) == 32
    lays = [x.c_struct() for x in G.layouts(3, shape)]
    with pytest.raises(ExamgError, match="star route"):
        hip.axis_op(APPLY, lays[0], hip.new_array(G.layouts(3, shape)[0].size), None, None, lays[2], hip.new_array(G.layouts(3, shape)[2].size), st,
                    0.0, -1, begin, [begin[d] + ext[d] for d in range(3)], route=AXIS_STAR)
    # the full stencil couples the points of one colour: the coloured smoother in place is the restatement's only where it reads old values,
    # so the colours are checked out of place (APPLY, RESIDUAL) and the smoother without a colour
    shape, b, e = N.geometry(3, ext, begin)
    lays = G.layouts(3, shape)
    rng = np.random.default_rng(12)
    data = [rng.uniform(-1.0, 1.0, int(l.size)) for l in lays]
    data[2][:] = N.SENTINEL
    for mode, colour, wform in [(APPLY, -1, 0), (APPLY, 0, 0), (RESIDUAL, 1, 0), (RESIDUAL, -1, 0), (SMOOTH, -1, 0), (SMOOTH, -1, 1)]:
        s = st.with_wform(wform)
        got, want = run(hip, mode, data, lays, s, 0.7, colour, b, e, None), run(orc, mode, data, lays, s, 0.7, colour, b, e, None)
        for g, w_, name in zip(got, want, ("u", "rhs", "dst")):
            same_bits(g, w_, "27 entries mode %d colour %d wform %d %s" % (mode, colour, wform, name))


@pytest.mark.parametrize("kind", [5, 9])
def test_generic_kernel_in_two_dimensions(hip, orc, kind):
    ext, begin = (67, 9, 1), (2, 1, 0)
    shape, _, _ = N.geometry(2, ext, begin)
    st = G.separated(G.fd_text(2), 2, G.random_grid(2, shape, 8)) if kind == 5 else G.full_stencil(2, shape, 22, 9)
    assert len(st.offsets) == kind
    if kind == 5:
        assert check_all_forms(hip, orc, st, 2, ext, begin, AXIS_GENERIC, "5-point") == 12
        return
    shape, b, e = N.geometry(2, ext, begin)
    lays = G.layouts(2, shape)
    rng = np.random.default_rng(13)
    data = [rng.uniform(-1.0, 1.0, int(l.size)) for l in lays]
    data[2][:] = N.SENTINEL
    for mode, colour, wform in [(APPLY, -1, 0), (APPLY, 1, 0), (RESIDUAL, 0, 0), (SMOOTH, -1, 0), (SMOOTH, -1, 1)]:
        s = st.with_wform(wform)
        got, want = run(hip, mode, data, lays, s, 0.7, colour, b, e, None), run(orc, mode, data, lays, s, 0.7, colour, b, e, None)
        for g, w_, name in zip(got, want, ("u", "rhs", "dst")):
            same_bits(g, w_, "9 entries mode %d colour %d wform %d %s" % (mode, colour, wform, name))


def test_refusals_write_nothing(hip):
    n = 12
    grid = G.random_grid(3, (n, n, n), 4)
    st = G.separated(G.fd_text(3), 3, grid)
    lu, lf, ld = G.layouts(3, (n, n, n))
    cases = [
        ("tables", lu, [1, 1, 1], [n + 2, n, n], "the tables of axis 0 cover"),                     # an index the tables do not hold
        ("shell", FieldLayout.node(3, (n, n, n), 0), [0, 1, 1], [n, n, n], "one-point shell of the box leaves the u allocation"),
        ("transformed", lu.split_x(), [1, 1, 1], [n, n, n], "layout transformation"),
    ]
    for name, l_u, b, e, words in cases:
        big = FieldLayout.node(3, (n + 4, n, n), 1) if name == "tables" else None       # the box itself lies in every allocation
        layouts = [(big or l_u), (big or lf), (big or ld)]
        u, f = hip.new_array(layouts[0].size), hip.new_array(layouts[1].size)
        dst = hip.from_host(np.full(int(layouts[2].size), N.SENTINEL))
        for route in (None, AXIS_GENERIC, AXIS_STAR):
            with pytest.raises(ExamgError, match=words):
                hip.axis_op(RESIDUAL, layouts[0].c_struct(), u, layouts[1].c_struct(), f, layouts[2].c_struct(), dst, st, 0.0, -1, b, e, route=route)
            assert hip.axis_route(RESIDUAL, layouts[0].c_struct(), layouts[1].c_struct(), layouts[2].c_struct(), st, -1, b, e, route=route) == -1
        assert np.all(host(hip, dst) == N.SENTINEL), name
    u = hip.new_array(lu.size)
    with pytest.raises(ExamgError, match="only a coloured loop runs in place"):
        hip.axis_op(SMOOTH, lu.c_struct(), u, lf.c_struct(), hip.new_array(lf.size), lu.c_struct(), u, st, 0.8, -1, [1, 1, 1], [n, n, n])


def test_point_expressions_over_the_tables(hip, orc):
    n = (14, 9, 11)
    grid = G.random_grid(3, n, 6)
    l = FieldLayout.node(3, n, 1, align=16)
    b, e = [1, 0, 2], [n[0], n[1] + 1, n[2]]
    exact = ExprC.from_program([("x", None), ("y", None), ("*", None), ("wx", None), ("wz", None), ("*", None), ("+", None), ("z", None), ("-", None)])
    volume = ExprC.from_program([("wx", None), ("wy", None), ("*", None), ("wz", None), ("*", None), ("x", None), ("/", None)])
    trig = ExprC.from_program([("x", None), ("tan", None), ("y", None), ("wz", None), ("*", None), ("exp", None), ("+", None), ("const", 2.0),
                               ("wx", None), ("pow", None), ("-", None)])

    def go(ops, expr):
        g = grid.device(ops, G.LVL)
        x, y = ops.from_host(np.full(int(l.size), N.SENTINEL)), ops.from_host(np.full(int(l.size), N.SENTINEL))
        ops.fill_expr_grid(l.c_struct(), x, g, expr, b, e)
        ops.apply_dirichlet_expr_grid(l.c_struct(), y, g, expr, 63)
        err = ops.scalar_value(ops.max_err_expr_grid(l.c_struct(), x, g, ExprC.from_program(expr.program + [("const", 0.75), ("*", None)]), b, e))
        return host(ops, x), host(ops, y), err

    for expr in (exact, volume):
        gx, gy, gerr = go(hip, expr)
        cx, cy, cerr = go(orc, expr)
        same_bits(gx, cx, "fill")
        same_bits(gy, cy, "dirichlet")
        assert gerr == cerr and gerr > 0.0
    gx, gy, gerr = go(hip, trig)
    cx, cy, cerr = go(orc, trig)
    inside = cx != N.SENTINEL
    assert np.array_equal(gx != N.SENTINEL, inside) and np.array_equal(gy != N.SENTINEL, cy != N.SENTINEL)
    scale = np.maximum(np.abs(cx), 1.0)
    assert np.all(np.abs(gx - cx)[inside] <= 8 * np.spacing(scale)[inside])
    assert np.all(np.abs(gy - cy)[cy != N.SENTINEL] <= 8 * np.spacing(np.maximum(np.abs(cy), 1.0))[cy != N.SENTINEL])
    assert abs(gerr - cerr) <= 1e-12 * max(1.0, cerr)
    # a point whose cell's upper node the table does not hold; a width operand in an entry point of the uniform grid
    g = grid.device(hip, G.LVL)
    x = hip.from_host(np.full(int(l.size), N.SENTINEL))
    wide = FieldLayout.node(3, (n[0] + 6, n[1], n[2]), 1)
    xw = hip.from_host(np.full(int(wide.size), N.SENTINEL))
    with pytest.raises(ExamgError, match="node table of axis 0 covers"):
        hip.fill_expr_grid(wide.c_struct(), xw, g, exact, [0, 0, 0], [n[0] + 5, 2, 2])
    assert np.all(host(hip, xw) == N.SENTINEL)
    from exastencils_amd.lib import GeomC

    with pytest.raises(ExamgError, match="unknown opcode"):
        hip.fill_expr(l.c_struct(), x, GeomC(), exact, b, e)
    assert np.all(host(hip, x) == N.SENTINEL)


@pytest.mark.parametrize("nd,hi", [(3, 4), (2, 5)])
def test_example_programs_on_the_device(hip, orc, nd, hi):
    P, out = G.run_own(nd, hip, maxLevel=hi, auto_graph=False)
    Q, want = G.run_own(nd, orc, maxLevel=hi)
    print(nd, out)
    assert out == want
    Gp, replayed = G.run_own(nd, hip, maxLevel=hi, auto_graph=True)
    rec = {k: v for k, v in Gp._auto_calls.items()}
    print("recorded", rec, "replays", Gp.graph_replays)
    assert replayed == out and Gp.graph_replays > 0
    assert [float(v).hex() for v in Gp.printed_values] == [float(v).hex() for v in P.printed_values]
