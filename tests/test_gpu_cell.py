"""GPU parity of the cell-centred entry points (include/examg.h: examg_*_cell, examg_sum, examg_add_scalar) against their
CPU restatement (tests/cell_ops.py), and the cell example programs on the HIP kernels.  Point-wise kernels: bit-exact;
reductions: 1e-13 relative."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from cell_ops import CellOracleOps

from exastencils_amd import exa4, lib
from exastencils_amd.field import Stencil
from exastencils_amd.layout import FieldLayout
from exastencils_amd.lib import ExprC, GeomC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples", "exa4")


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
    return CellOracleOps()


def geom(nd, n, lo=0.0):
    g = GeomC()
    for d in range(3):
        g.pos_begin[d] = lo if d < nd else 0.0
        g.h[d] = 1.0 / n[d] if d < nd else 0.0
    return g


POLY = ExprC.from_program([("x", None), ("x", None), ("*", None), ("const", 0.5), ("y", None), ("*", None), ("-", None),
                           ("z", None), ("const", 3.0), ("*", None), ("+", None)])     # x*x - 0.5*y + z*3.0
CONST = ExprC.from_program([("const", 1.25)])


def same(a, b, what):
    if not np.array_equal(a, b):
        d = np.abs(a - b)
        raise AssertionError("%s: %d of %d values differ, max abs %.3e" % (what, int((d > 0).sum()), d.size, d.max()))


def run_both(hip, orc, fn):
    g = fn(hip)
    hip.synchronize()
    c = fn(orc)
    return [hip.to_host(t).copy() for t in g], [orc.to_host(t).copy() for t in c]


# (nd, fine cells, ghost, align)
LAYOUTS = [(3, (48, 24, 12), 1, 0), (3, (48, 24, 12), 1, 2), (3, (96, 40, 24), 0, 0), (3, (96, 40, 24), 0, 2),
           (2, (192, 96), 1, 0), (2, (192, 96), 1, 2), (2, (24, 12), 0, 0)]


@pytest.mark.parametrize("nd,n,ghost,align", LAYOUTS)
@pytest.mark.parametrize("interior", [False, True])
def test_restrict_cell_bitwise(hip, orc, nd, n, ghost, align, interior):
    lf = FieldLayout.cell(nd, n, ghost, align=align)
    lc = FieldLayout.cell(nd, [v // 2 for v in n], ghost, align=align)
    nc = [lc.inner[d] for d in range(3)]
    b, e = [0, 0, 0], [nc[0], nc[1], nc[2] if nd == 3 else 1]
    if interior:
        b = [1, 2, 1 if nd == 3 else 0]
        e = [nc[0] - 1, nc[1] - 1, (nc[2] - 2) if nd == 3 else 1]
    scale = 1.0 if not interior else 0.3

    def run(ops):
        rf, fc = ops.new_array(lf.size), ops.new_array(lc.size)
        ops.fill_random(rf, 11)
        ops.fill_random(fc, 12)
        ops.restrict_cell(lf.c_struct(), rf, lc.c_struct(), fc, scale, b, e)
        return [fc]

    g, c = run_both(hip, orc, run)
    same(g[0], c[0], "restrict_cell")


@pytest.mark.parametrize("nd,n,ghost,align", LAYOUTS)
@pytest.mark.parametrize("interior", [False, True])
def test_prolong_add_cell_bitwise(hip, orc, nd, n, ghost, align, interior):
    lf = FieldLayout.cell(nd, n, ghost, align=align)
    lc = FieldLayout.cell(nd, [v // 2 for v in n], ghost, align=align)
    b, e = [0, 0, 0], [n[0], n[1], n[2] if nd == 3 else 1]
    if interior:        # odd starts: a lane's pair straddles the box edge
        b = [1, 3, 1 if nd == 3 else 0]
        e = [n[0] - 3, n[1] - 1, (n[2] - 2) if nd == 3 else 1]

    def run(ops):
        uc, uf = ops.new_array(lc.size), ops.new_array(lf.size)
        ops.fill_random(uc, 21)
        ops.fill_random(uf, 22)
        ops.prolong_add_cell(lc.c_struct(), uc, lf.c_struct(), uf, b, e)
        return [uf]

    g, c = run_both(hip, orc, run)
    same(g[0], c[0], "prolong_add_cell")


def test_transfer_load_widths_give_the_same_bits(hipd, orc):
    """The 16-byte form (aligned layout) and the forced 8-byte form of the same call: identical to the restatement."""
    lf = FieldLayout.cell(3, (128, 16, 8), 1, align=2)
    lc = FieldLayout.cell(3, (64, 8, 4), 1, align=2)
    L = hipd.L
    outs = []
    for narrow in (0, 1):
        L.examg_debug_cell_narrow(narrow)
        try:
            def run(ops):
                rf, fc = ops.new_array(lf.size), ops.new_array(lc.size)
                uf = ops.new_array(lf.size)
                ops.fill_random(rf, 5)
                ops.fill_random(uf, 6)
                ops.restrict_cell(lf.c_struct(), rf, lc.c_struct(), fc, 1.0, [0, 0, 0], [64, 8, 4])
                ops.prolong_add_cell(lc.c_struct(), fc, lf.c_struct(), uf, [0, 0, 0], [128, 16, 8])
                return [fc, uf]

            g, c = run_both(hipd, orc, run)
        finally:
            L.examg_debug_cell_narrow(0)
        same(g[0], c[0], "restrict narrow=%d" % narrow)
        same(g[1], c[1], "prolong narrow=%d" % narrow)
        outs.append(g)
    same(outs[0][1], outs[1][1], "16-byte vs 8-byte form")


@pytest.mark.parametrize("nd,n,ghost,align", [(3, (40, 24, 12), 1, 0), (3, (40, 24, 12), 2, 2), (2, (96, 48), 1, 2), (2, (6, 12), 1, 0)])
@pytest.mark.parametrize("kind,expr,mask", [(lib.BC_DIRICHLET, "poly", 63), (lib.BC_DIRICHLET, "const", 63), (lib.BC_NEUMANN, None, 63),
                                            (lib.BC_DIRICHLET, "poly", 0b100110)])
def test_apply_bc_cell_bitwise(hip, orc, nd, n, ghost, align, kind, expr, mask):
    l = FieldLayout.cell(nd, n, ghost, align=align)
    g = geom(nd, n, -0.25)
    ex = {"poly": POLY, "const": CONST, None: None}[expr]
    m = mask & ((1 << (2 * nd)) - 1)

    def run(ops):
        x = ops.new_array(l.size)
        ops.fill_random(x, 31)
        ops.apply_bc_cell(l.c_struct(), x, g, kind, ex, m)
        return [x]

    gg, c = run_both(hip, orc, run)
    same(gg[0], c[0], "apply_bc_cell")


@pytest.mark.parametrize("nd,n,ghost,align", [(3, (40, 24, 12), 1, 2), (2, (200, 12), 0, 0)])
def test_fill_and_max_err_cell(hip, orc, nd, n, ghost, align):
    l = FieldLayout.cell(nd, n, ghost, align=align)
    g = geom(nd, n)
    b, e = [0, 0, 0], [n[0], n[1], n[2] if nd == 3 else 1]

    def run(ops):
        x, y = ops.new_array(l.size), ops.new_array(l.size)
        ops.fill_expr_cell(l.c_struct(), x, g, POLY, b, e)
        ops.fill_random(y, 41)
        err = ops.max_err_expr_cell(l.c_struct(), y, g, POLY, b, e)
        return [x, err]

    gg, c = run_both(hip, orc, run)
    same(gg[0], c[0], "fill_expr_cell")
    assert abs(gg[1][0] - c[1][0]) <= 1e-13 * abs(c[1][0])


@pytest.mark.parametrize("lay", [FieldLayout.cell(3, (130, 20, 6), 1, align=2), FieldLayout.cell(2, (30, 20), 0),
                                 FieldLayout.node(3, (64, 16, 8), 1)])
def test_sum_and_add_scalar(hip, orc, lay):
    b = [lay.idx("DLB", d) for d in range(3)]
    e = [lay.idx("DRE", d) if d < lay.nd else 1 for d in range(3)]

    def run(ops):
        x = ops.new_array(lay.size)
        ops.fill_random(x, 51)
        s = ops.sum(lay.c_struct(), x, b, e)
        ops.add_scalar(lay.c_struct(), x, -0.375, b, e)
        return [x, s]

    gg, c = run_both(hip, orc, run)
    same(gg[0], c[0], "add_scalar")
    assert abs(gg[1][0] - c[1][0]) <= 1e-13 * np.abs(c[0]).sum()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_seven_point_loops_on_cell_layouts(hip, orc, mode):
    """examg_stencil_op on a cell layout with n0 >= 64: the layout-generic z-march of the node fields, same bits as the oracle."""
    n = (64, 24, 16)
    lu = FieldLayout.cell(3, n, 1, align=2)
    lf = FieldLayout.cell(3, n, 0)
    h = [1.0 / v for v in n]
    A = Stencil([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)],
                [2.0 / (h[0] * h[0]) + 2.0 / (h[1] * h[1]) + 2.0 / (h[2] * h[2]), -1.0 / (h[0] * h[0]), -1.0 / (h[0] * h[0]),
                 -1.0 / (h[1] * h[1]), -1.0 / (h[1] * h[1]), -1.0 / (h[2] * h[2]), -1.0 / (h[2] * h[2])])
    b, e = [0, 0, 0], list(n)

    def run(ops):
        u, f, d = ops.new_array(lu.size), ops.new_array(lf.size), ops.new_array(lu.size)
        ops.fill_random(u, 61)
        ops.fill_random(f, 62)
        ops.stencil_op(mode, lu.c_struct(), u, lf.c_struct() if mode else None, f if mode else None, lu.c_struct(), d, A,
                       0.8 / A.coefs[0], -1, b, e)
        return [d]

    gg, c = run_both(hip, orc, run)
    same(gg[0], c[0], "stencil_op mode %d" % mode)


# -- example programs ---------------------------------------------------------------------------------------------------------
EXAMPLES = [("cell3d_dirichlet.exa4", 3, "CellBased_3D_Basic.results"), ("cell3d_neumann.exa4", 3, "CellBased_3D_Neumann.results"),
            ("cell2d_dirichlet.exa4", 2, "CellBased_2D_Basic.results")]


def knowledge(nd):
    return dict(dimensionality=nd, minLevel=0, maxLevel=6, domain_fragmentLength_x=4, domain_fragmentLength_y=4, domain_fragmentLength_z=4)


@pytest.mark.parametrize("name,nd,gold", EXAMPLES)
def test_cell_example_on_hip_prints_its_fixture(hip, name, nd, gold):
    from oracle import mg

    with open(os.path.join(EX, name)) as f:
        src = f.read()
    P = exa4.Exa4Program(src, knowledge(nd), ops=hip)
    out = P.run()
    with open(os.path.join(ROOT, "tests", "golden", gold)) as f:
        assert mg.compare_with_golden(out, f.read()) == []
    Q = exa4.Exa4Program(src, knowledge(nd), ops=CellOracleOps())
    Q.run()
    assert len(P.printed_values) == len(Q.printed_values)
    for a, b in zip(P.printed_values, Q.printed_values):
        assert abs(a - b) <= 1e-10 * abs(b)


def test_cell_example_auto_graph_gives_the_same_output(hip):
    with open(os.path.join(EX, "cell3d_dirichlet.exa4")) as f:
        src = f.read()
    k = dict(knowledge(3), maxLevel=5)
    P = exa4.Exa4Program(src, k, ops=hip, auto_graph=True)
    Q = exa4.Exa4Program(src, k, ops=hip, auto_graph=False)
    assert P.run() == Q.run()
    assert P.printed_values == Q.printed_values
