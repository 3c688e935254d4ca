"""The references of tests/setup_cases.py, pinned on the CPU before tests/test_gpu_setup.py lets them judge the library: the rounded
references of the two stencil-field initialisers against the C oracle (bit for bit, with the libm-free named functions passed to the
reference as their programs), the exact against the rounded reference of each operation on exact data, and the cell, face and grid
references against the older numpy restatements (CellOracleOps, FluxOracleOps, MacOracleOps, GridOracleOps) -- which pins those too."""
import numpy as np
import pytest

import setup_cases as T
from blas_cases import SENTINEL, geometry
from cell_ops import CellOracleOps
from flux_ops import FluxOracleOps
from grid_ops import GridOracleOps
from mac_ops import MacOracleOps
from oracle_ops import OracleOps

from exastencils_amd.field import FN_KAPPA_POLY, FN_KAPPA_POLY2D, FN_POLY3D, _fn_program
from exastencils_amd.lib import ExprC, GridC

NGEOM = geometry((0.1, -0.3, 0.7), (1.0 / 7.0, 1.0 / 5.0, 1.0 / 3.0))          # not dyadic
NGEOM_EQ = geometry((0.1, -0.3, 0.7), (1.0 / 7.0, 1.0 / 7.0, 1.0 / 7.0))


def same(got, want, what=""):
    msg = T.differing(np.ascontiguousarray(got), np.ascontiguousarray(want))
    assert msg is None, "%s: %s" % (what, msg)


def run(ops, start, call):
    x = ops.from_host(start.copy())
    call(x)
    ops.synchronize()
    return ops.to_host(x)


# ---- the initialisers: rounded reference == C oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", [FN_KAPPA_POLY, FN_POLY3D, FN_KAPPA_POLY2D])
@pytest.mark.parametrize("case", T.VARCOEFF_CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("geom", [NGEOM, T.EGEOM], ids=["nondyadic", "dyadic"])
def test_rounded_varcoeff7_equals_the_oracle(case, fn, geom):
    orc = OracleOps()
    start = T.init_start(case)
    got = run(orc, start, lambda x: orc.init_varcoeff7(case.layout.c_struct(), x, geom, fn, (10.0,), *case.box))
    want = T.rounded_varcoeff7(case.layout, start, geom, _fn_program(fn, 10.0), *case.box)
    same(got, want)
    assert np.count_nonzero(want != SENTINEL) == (2 * case.layout.nd + 1) * np.prod([e - b for b, e in zip(*case.box)])


@pytest.mark.parametrize("fn", [FN_KAPPA_POLY, FN_POLY3D])
@pytest.mark.parametrize("case", T.HELMHOLTZ_CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("geom", [NGEOM_EQ, T.EGEOM_EQ], ids=["nondyadic", "dyadic"])
def test_rounded_helmholtz27_equals_the_oracle(case, fn, geom):
    orc = OracleOps()
    start = T.init_start(case)
    got = run(orc, start, lambda x: orc.init_helmholtz27(case.layout.c_struct(), x, geom, fn, (10.0, T.KSQ), *case.box))
    want = T.rounded_helmholtz27(case.layout, start, geom, _fn_program(fn, 10.0), T.KSQ, *case.box)
    same(got, want)


def test_the_oracle_layer_refuses_unequal_widths_as_the_library_does():
    orc, case = OracleOps(), T.HELMHOLTZ_CASES[0]
    x = orc.from_host(T.init_start(case))
    with pytest.raises(ValueError, match="unequal mesh widths"):
        orc.init_helmholtz27(case.layout.c_struct(), x, T.EGEOM, FN_POLY3D, (0.0, T.KSQ), *case.box)
    assert np.all(orc.to_host(x) == SENTINEL)


# ---- exact data: exact reference == rounded reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.VARCOEFF_CASES, ids=lambda c: c.name)
def test_varcoeff7_references_agree_on_exact_data(case):
    same(T.varcoeff_reference(case.name, "exact"), T.rounded_varcoeff7(case.layout, T.init_start(case), T.EGEOM, T.ECOEF, *case.box))
    if case.layout.nd == 2:          # planes 5 and 6 of the 7-plane allocation
        assert np.all(T.varcoeff_reference(case.name, "exact")[5 * case.layout.size:] == SENTINEL)


@pytest.mark.parametrize("case", T.HELMHOLTZ_CASES, ids=lambda c: c.name)
def test_helmholtz27_references_agree_on_exact_data(case):
    same(T.helmholtz_reference(case.name, "exact"), T.rounded_helmholtz27(case.layout, T.init_start(case), T.EGEOM_EQ, T.HCOEF, T.KSQ, *case.box))


def test_the_coefficients_tell_axes_signs_and_entries_apart():
    """No two planes of a reference are equal on the box, and no plane is symmetric under a flip of the box along an axis."""
    for ref, case in ((T.varcoeff_reference, T.VARCOEFF_CASES[0]), (T.helmholtz_reference, T.HELMHOLTZ_CASES[0])):
        for cls in ("exact", "rounded"):
            a, l = ref(case.name, cls), case.layout
            K = 7 if ref is T.varcoeff_reference else 27
            planes = [T.view(l, a[k * l.size:(k + 1) * l.size])[T.box_index(l, *case.box)] for k in range(K)]
            edge = [k for k in range(K) if K == 27 and sum(o != 0 for o in T.H27_ENTRIES[k]) == 1]      # kf = 0.0: all zero
            for k in range(K):
                if k in edge:
                    assert not planes[k].any()
                    continue
                assert all(not np.array_equal(planes[k], planes[j]) for j in range(k) if j not in edge), (cls, k)
                assert all(not np.array_equal(planes[k], np.flip(planes[k], ax)) for ax in range(3)), (cls, k)


# ---- the older restatements -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lname,kind,mask", T.BC_CASES)
def test_bc_cell_reference_equals_the_restatements(lname, kind, mask):
    l = T.BC_LAYOUTS[lname]
    orc = FluxOracleOps() if kind == T.NEGATE else CellOracleOps()
    expr = ExprC.from_program(T.BC_PROGRAM) if kind == T.DIRICHLET else None
    got = run(orc, T.bc_start(l), lambda x: orc.apply_bc_cell(l.c_struct(), x, T.EGEOM, kind, expr, mask))
    same(got, T.bc_cell_reference(lname, kind, mask))


def test_bc_cell_reference_writes_what_it_claims():
    """Ghost 2: only the first layer changes; one cell on an axis: both ghosts come from it; edge and corner ghosts keep their values."""
    l = T.BC_LAYOUTS["5x4x3_g2_a2"]
    start, after = T.bc_start(l), T.bc_cell_reference("5x4x3_g2_a2", T.NEUMANN, 63)
    changed = T.view(l, after != start)
    expect = sum(2 * l.inner[a] * l.inner[b] for a, b in ((0, 1), (0, 2), (1, 2)))
    assert 0 < changed.sum() <= expect
    inner = T.box_index(l, (-1, -1, -1), tuple(n + 1 for n in l.inner))
    outer = changed.copy()
    outer[inner] = False
    assert not outer.any()
    l1 = T.BC_LAYOUTS["6x1x3_g1"]
    a = T.view(l1, T.bc_cell_reference("6x1x3_g1", T.NEGATE, 0b1100))
    row = T.box_index(l1, (0, 0, 0), (6, 1, 3))
    assert np.array_equal(a[T.box_index(l1, (0, -1, 0), (6, 0, 3))], -a[row]) and np.array_equal(a[T.box_index(l1, (0, 1, 0), (6, 2, 3))], -a[row])


def test_the_cap_case_reference_equals_the_restatement():
    orc = CellOracleOps()
    start, want = T.cap_reference()
    got = run(orc, start, lambda x: orc.apply_bc_cell(T.CAP_LAYOUT.c_struct(), x, T.CAP_GEOM, T.DIRICHLET, ExprC.from_program(T.CAP_PROGRAM), T.CAP_MASK))
    same(got, want)
    assert np.count_nonzero(got != start) > T.CAP_THREADS * 0.9


@pytest.mark.parametrize("loc,nd", T.POS_CASES)
@pytest.mark.parametrize("pname", sorted(T.POS_PROGRAMS))
def test_position_references_equal_the_restatements(loc, nd, pname):
    l = T.pos_layout(loc, nd)
    b, e = T.ghost_box(l)
    expr = ExprC.from_program(T.POS_PROGRAMS[pname])
    orc = MacOracleOps()
    fill = {"node": lambda x: orc.fill_expr(l.c_struct(), x, T.EGEOM, expr, b, e),
            "cell": lambda x: orc.fill_expr_cell(l.c_struct(), x, T.EGEOM, expr, b, e)}.get(
                loc, lambda x: orc.fill_expr_face(T.LOCS.index(loc) - 2, l.c_struct(), x, T.EGEOM, expr, b, e))
    want = T.pos_reference(loc, nd, pname)
    same(run(orc, np.full(l.size, SENTINEL), fill), want)
    # the needle: a deviation of 3.0 at one point is the maximum, exactly
    for where in T.plants(b, e):
        x = orc.from_host(T.planted(l, want, where))
        err = {"node": lambda: orc.max_err_expr(l.c_struct(), x, T.EGEOM, expr, b, e),
               "cell": lambda: orc.max_err_expr_cell(l.c_struct(), x, T.EGEOM, expr, b, e)}.get(
                   loc, lambda: orc.max_err_expr_face(T.LOCS.index(loc) - 2, l.c_struct(), x, T.EGEOM, expr, b, e))()
        assert orc.scalar_value(err) == 3.0


def test_face_positions_differ_from_every_other_localization():
    """A reference that took another localization's positions would differ: the fills of x, y and z tell all five apart."""
    for nd in (3, 2):
        for pname in "xyz"[:nd]:
            per_loc = {}
            for loc in [c[0] for c in T.POS_CASES if c[1] == nd]:
                l = T.pos_layout(loc, nd)
                per_loc[loc] = T.view(l, T.pos_reference(loc, nd, pname))[T.box_index(l, (0, 0, 0), (1, 1, 1))].item()
            half = {loc: per_loc[loc] - per_loc["node"] for loc in per_loc}
            d = "xyz".index(pname)
            for loc, v in half.items():
                own = loc == "node" or loc == "face_" + pname
                assert v == (0.0 if own else T.EGEOM.h[d] / 2), (nd, pname, loc)


@pytest.mark.parametrize("nd,axis,lname,kind,mask", T.FACE_CASES)
def test_bc_face_reference_equals_the_restatement(nd, axis, lname, kind, mask):
    l = T.face_layouts(nd, axis)[lname]
    orc = MacOracleOps()
    expr = ExprC.from_program(T.BC_PROGRAM) if kind == T.DIRICHLET else None
    got = run(orc, T.bc_start(l), lambda x: orc.apply_bc_face(axis, l, x, T.EGEOM, kind, expr, mask))
    same(got, T.bc_face_reference(nd, axis, lname, kind, mask))


def test_bc_face_reference_takes_interior_from_the_node_rule():
    """With all walls in the mask the ghosts beside the two boundary faces do not depend on what those faces held."""
    l = T.face_layouts(3, 0)["g1"]
    start = T.bc_start(l)
    other = start.copy()
    v = T.view(l, other)
    v[T.box_index(l, (0, 0, 0), (1, 3, 5))] += 100.0
    v[T.box_index(l, (6, 0, 0), (7, 3, 5))] -= 100.0
    a = T.exact_bc_face(0, l, start, T.EGEOM, T.DIRICHLET, T.BC_PROGRAM, 63)
    b = T.exact_bc_face(0, l, other, T.EGEOM, T.DIRICHLET, T.BC_PROGRAM, 63)
    assert np.array_equal(a, b)
    c = T.exact_bc_face(0, l, other, T.EGEOM, T.DIRICHLET, T.BC_PROGRAM, 0b111100)      # without the normal walls: read from memory
    assert not np.array_equal(T.view(l, a)[T.box_index(l, (0, -1, 0), (7, 0, 5))], T.view(l, c)[T.box_index(l, (0, -1, 0), (7, 0, 5))])


def _grid(orc, tables, ghost):
    g, keep = GridC(), []
    for d, t in enumerate(tables):
        keep.append(orc.from_host(t.copy()))
        g.nodes[d], g.n[d] = orc.ptr(keep[-1]), len(t)
    g.ghost = ghost
    return g, keep


@pytest.mark.parametrize("pname", sorted(T.GRID_PROGRAMS))
def test_grid_references_equal_the_restatement(pname):
    orc = GridOracleOps()
    l, L = T.GRID_LAYOUT, T.GRID_LAYOUT.c_struct()
    g, keep = _grid(orc, T.grid_tables(), T.GRID_GHOST)
    expr = ExprC.from_program(T.GRID_PROGRAMS[pname])
    b, e = T.GRID_FILL_BOX
    want = T.grid_fill_reference(pname)
    same(run(orc, np.full(l.size, SENTINEL), lambda x: orc.fill_expr_grid(L, x, g, expr, b, e)), want)
    for mask in T.GRID_MASKS:
        same(run(orc, np.full(l.size, SENTINEL), lambda x: orc.apply_dirichlet_expr_grid(L, x, g, expr, mask)), T.grid_dirichlet_reference(pname, mask))
    for where in T.plants(b, e):
        p = T.plants(b, e)[where]
        a = want.copy()
        a[l.linear(*p)] += 3.0
        assert orc.scalar_value(orc.max_err_expr_grid(L, orc.from_host(a), g, expr, b, e)) == 3.0
    assert orc.scalar_value(orc.max_err_expr_grid(L, orc.from_host(want.copy()), g, expr, b, e)) == 0.0


def test_grid_tables_are_dyadic_and_differ_per_axis_and_cell():
    t = T.grid_tables()
    assert [len(x) for x in t] == [T.GRID_LAYOUT.inner[d] + 2 + 2 * T.GRID_GHOST for d in range(3)]
    for x in t:
        w = np.diff(x)
        assert np.all(w > 0) and len(set(w.tolist())) >= 4
    m = T.view(T.GRID_LAYOUT, T.grid_dirichlet_reference("poly", 0b100110) != SENTINEL)
    assert m.sum() > 0 and not m[T.box_index(T.GRID_LAYOUT, (1, 1, 1), (7, 5, 4))].any()
    assert np.all(T.grid_dirichlet_reference("poly", 0) == SENTINEL)
