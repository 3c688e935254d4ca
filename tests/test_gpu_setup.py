"""The kernels that turn an index into a position, through the product library, against the references of tests/setup_cases.py
(pinned on the CPU by tests/test_setup_exact.py): the stencil-field initialisers, `apply bc` of cell, vector-valued cell and face
fields, the point expressions of the five localizations and the _grid entry points.  Every comparison covers the whole allocation;
every refusal is asserted together with "nothing written"."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import setup_cases as T
from blas_cases import SENTINEL, geometry

from exastencils_amd.layout import FieldLayout
from exastencils_amd.lib import ExamgError, ExprC, GridC


@pytest.fixture(scope="module")
def hip():
    from exastencils_amd.ops import HipOps

    return HipOps(0)


def run(hip, start, call):
    x = hip.from_host(np.array(start))
    call(x)
    hip.synchronize()
    return hip.to_host(x)


def same(got, want):
    msg = T.differing(got, want)
    assert msg is None, msg


def refused(hip, start, call, match):
    """The call raises, and the array keeps every double."""
    x = hip.from_host(np.array(start))
    with pytest.raises(ExamgError, match=match):
        call(x)
    hip.synchronize()
    assert np.array_equal(hip.to_host(x), start)


def expr(program):
    return ExprC.from_program(program)


def value(hip, t):
    return float(hip.to_host(t)[0])


# ---- examg_init_varcoeff7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["exact", "rounded"])
@pytest.mark.parametrize("case", T.VARCOEFF_CASES, ids=lambda c: c.name)
def test_init_varcoeff7(hip, case, cls):
    geom, _, coef, _ = T.INIT_CLASSES[cls]
    got = run(hip, T.init_start(case), lambda x: hip.init_varcoeff7(case.layout.c_struct(), x, geom, expr(coef), (), *case.box))
    same(got, T.varcoeff_reference(case.name, cls))


@pytest.mark.parametrize("cls", ["exact", "rounded"])
def test_init_varcoeff7_under_the_colour_split(hip, cls):
    """The coefficient layout under `[x, y, z] => [x / 2, y, z, x % 2]`: every plane holds the plain plane's values where the split puts them."""
    case = T.VARCOEFF_CASES[0]
    geom, _, coef, _ = T.INIT_CLASSES[cls]
    l = case.layout.split_x()
    got = run(hip, np.full(7 * l.size, SENTINEL), lambda x: hip.init_varcoeff7(l.c_struct(), x, geom, expr(coef), (), *case.box))
    assert l.size >= case.layout.size
    same(got, T.split_planes(case.layout, T.varcoeff_reference(case.name, cls), 7))


def test_init_varcoeff7_past_the_thread_cap(hip):
    """2048 x 1025 points of a 2-D box: more than the 8192 x 256 threads of the launch, the grid-stride loop of k_init_varcoeff."""
    l = FieldLayout.node(2, (2047, 1024, 0), 0)
    b, e = l.loop_box()
    assert (e[0] - b[0]) * (e[1] - b[1]) > 8192 * 256
    start = np.full(5 * l.size, SENTINEL)
    got = run(hip, start, lambda x: hip.init_varcoeff7(l.c_struct(), x, T.RGEOM, expr(T.RCOEF), (), b, e))
    same(got, T.rounded_varcoeff7(l, start, T.RGEOM, T.RCOEF, b, e))


# ---- examg_init_helmholtz27 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["exact", "rounded"])
@pytest.mark.parametrize("case", T.HELMHOLTZ_CASES, ids=lambda c: c.name)
def test_init_helmholtz27(hip, case, cls):
    _, geom, _, coef = T.INIT_CLASSES[cls]
    got = run(hip, T.init_start(case), lambda x: hip.init_helmholtz27(case.layout.c_struct(), x, geom, expr(coef), (0.0, T.KSQ), *case.box))
    same(got, T.helmholtz_reference(case.name, cls))


def test_initialisers_refuse(hip):
    case = T.HELMHOLTZ_CASES[0]
    L, start = case.layout.c_struct(), T.init_start(case)
    b, e = case.box
    # unequal mesh widths: the error names the three
    refused(hip, start, lambda x: hip.init_helmholtz27(L, x, T.EGEOM, expr(T.HCOEF), (0.0, T.KSQ), b, e), r"unequal mesh widths.*0\.125.*0\.25.*0\.5")
    for d in (1, 2):
        g = geometry((0.0, 0.0, 0.0), tuple(0.25 if t != d else 0.25 * (1.0 + 2.0 ** -52) for t in range(3)))
        refused(hip, start, lambda x: hip.init_helmholtz27(L, x, g, expr(T.HCOEF), (0.0, T.KSQ), b, e), "unequal mesh widths")
    # a 2-D layout
    l2 = T.VARCOEFF_CASES[-1].layout
    refused(hip, np.full(27 * l2.size, SENTINEL), lambda x: hip.init_helmholtz27(l2.c_struct(), x, T.EGEOM_EQ, expr(T.HCOEF), (0.0, T.KSQ), *l2.loop_box()), "3-D only")
    # a box that leaves the allocation, below and above
    out_b, out_e = T.ghost_box(case.layout)
    for bb, ee in (((out_b[0] - case.layout.pad_l[0] - 1, 0, 0), e), (b, (e[0], e[1], out_e[2] + 1))):
        refused(hip, start, lambda x: hip.init_helmholtz27(L, x, T.EGEOM_EQ, expr(T.HCOEF), (0.0, T.KSQ), bb, ee), "box leaves the allocation")
    vcase = T.VARCOEFF_CASES[0]
    vb, ve = vcase.box
    out_b, out_e = T.ghost_box(vcase.layout)
    for bb, ee in (((out_b[0] - vcase.layout.pad_l[0] - 1, 0, 0), ve), (vb, (ve[0], out_e[1] + 1, ve[2]))):
        refused(hip, T.init_start(vcase), lambda x: hip.init_varcoeff7(vcase.layout.c_struct(), x, T.EGEOM, expr(T.ECOEF), (), bb, ee), "box leaves the allocation")
    # a width opcode in the program of an entry point that takes an examg_geom_t
    refused(hip, T.init_start(vcase), lambda x: hip.init_varcoeff7(vcase.layout.c_struct(), x, T.EGEOM, expr(T.gprog("x wx *")), (), vb, ve), "unknown opcode")


# ---- examg_apply_bc_cell ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lname,kind,mask", T.BC_CASES)
def test_apply_bc_cell(hip, lname, kind, mask):
    l = T.BC_LAYOUTS[lname]
    e = expr(T.BC_PROGRAM) if kind == T.DIRICHLET else None
    got = run(hip, T.bc_start(l), lambda x: hip.apply_bc_cell(l.c_struct(), x, T.EGEOM, kind, e, mask))
    same(got, T.bc_cell_reference(lname, kind, mask))


def test_apply_bc_cell_past_the_thread_cap(hip):
    """524400 boundary cells on the two y walls: more than the 2048 x 256 threads of the launch."""
    start, want = T.cap_reference()
    got = run(hip, start, lambda x: hip.apply_bc_cell(T.CAP_LAYOUT.c_struct(), x, T.CAP_GEOM, T.DIRICHLET, expr(T.CAP_PROGRAM), T.CAP_MASK))
    same(got, want)


def test_apply_bc_cell_refuses(hip):
    l = FieldLayout.cell(3, (5, 4, 3), 0)
    for kind in (T.DIRICHLET, T.NEUMANN, T.NEGATE):
        refused(hip, T.bc_start(l), lambda x: hip.apply_bc_cell(l.c_struct(), x, T.EGEOM, kind, expr(T.BC_PROGRAM), 1 << 3), "no ghost layer")
    l = T.BC_LAYOUTS["5x4x3_g1"]
    refused(hip, T.bc_start(l), lambda x: hip.apply_bc_cell(l.c_struct(), x, T.EGEOM, T.DIRICHLET, expr(T.gprog("x wy +")), 63), "unknown opcode")


# ---- examg_vec_apply_bc_cell ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lname,n,mask", T.VEC_CASES)
def test_vec_apply_bc_cell(hip, lname, n, mask):
    l = T.VEC_LAYOUTS[lname]
    start, want = T.vec_bc_reference(lname, n, mask)
    assert start.size == n * l.size + T.VEC_TAIL
    got = run(hip, start, lambda x: hip.vec_apply_bc_cell(n, l.c_struct(), x, T.EGEOM, T.NEUMANN, mask))
    same(got, want)


# ---- positions per localization ---------------------------------------------------------------------------------------------------------
def _fill(hip, loc, l, x, e, b_, e_):
    if loc == "node":
        return hip.fill_expr(l.c_struct(), x, T.EGEOM, e, b_, e_)
    if loc == "cell":
        return hip.fill_expr_cell(l.c_struct(), x, T.EGEOM, e, b_, e_)
    return hip.fill_expr_face(T.LOCS.index(loc) - 2, l.c_struct(), x, T.EGEOM, e, b_, e_)


def _max_err(hip, loc, l, x, e, b_, e_):
    if loc == "node":
        return value(hip, hip.max_err_expr(l.c_struct(), x, T.EGEOM, e, b_, e_))
    if loc == "cell":
        return value(hip, hip.max_err_expr_cell(l.c_struct(), x, T.EGEOM, e, b_, e_))
    return value(hip, hip.max_err_expr_face(T.LOCS.index(loc) - 2, l.c_struct(), x, T.EGEOM, e, b_, e_))


@pytest.mark.parametrize("pname", sorted(T.POS_PROGRAMS))
@pytest.mark.parametrize("loc,nd", T.POS_CASES)
def test_fill_expr_per_localization(hip, loc, nd, pname):
    l = T.pos_layout(loc, nd)
    b, e = T.ghost_box(l)
    got = run(hip, np.full(l.size, SENTINEL), lambda x: _fill(hip, loc, l, x, expr(T.POS_PROGRAMS[pname]), b, e))
    same(got, T.pos_reference(loc, nd, pname))


@pytest.mark.parametrize("pname", sorted(T.POS_PROGRAMS))
@pytest.mark.parametrize("loc,nd", T.POS_CASES)
def test_max_err_expr_per_localization(hip, loc, nd, pname):
    l = T.pos_layout(loc, nd)
    b, e = T.ghost_box(l)
    want, ex = T.pos_reference(loc, nd, pname), expr(T.POS_PROGRAMS[pname])
    assert _max_err(hip, loc, l, hip.from_host(np.array(want)), ex, b, e) == 0.0
    for where in T.plants(b, e):
        assert _max_err(hip, loc, l, hip.from_host(T.planted(l, want, where)), ex, b, e) == 3.0, where


def test_point_expressions_refuse_width_opcodes(hip):
    l = T.pos_layout("face_y", 3)
    b, e = T.ghost_box(l)
    start = np.full(l.size, SENTINEL)
    for loc in ("node", "cell", "face_y"):
        refused(hip, start, lambda x: _fill(hip, loc, l, x, expr(T.gprog("wz")), b, e), "unknown opcode")
        with pytest.raises(ExamgError, match="unknown opcode"):
            _max_err(hip, loc, l, hip.from_host(start.copy()), expr(T.gprog("x wx +")), b, e)


# ---- examg_apply_bc_face ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd,axis,lname,kind,mask", T.FACE_CASES)
def test_apply_bc_face(hip, nd, axis, lname, kind, mask):
    l = T.face_layouts(nd, axis)[lname]
    e = expr(T.BC_PROGRAM) if kind == T.DIRICHLET else None
    got = run(hip, T.bc_start(l), lambda x: hip.apply_bc_face(axis, l.c_struct(), x, T.EGEOM, kind, e, mask))
    same(got, T.bc_face_reference(nd, axis, lname, kind, mask))


def test_apply_bc_face_refuses(hip):
    l = T.face_layouts(3, 1)["g1"]
    L, start, e = l.c_struct(), T.bc_start(l), expr(T.BC_PROGRAM)
    refused(hip, start, lambda x: hip.apply_bc_face(1, L, x, T.EGEOM, T.NEGATE, e, 63), "face fields take")
    for side in (0, 1):
        refused(hip, start, lambda x: hip.apply_bc_face(1, L, x, T.EGEOM, T.NEUMANN, None, 0b110011 | 1 << (2 + side)), "Neumann wall normal")
    refused(hip, start, lambda x: hip.apply_bc_face(1, L, x, T.EGEOM, T.DIRICHLET, expr(T.gprog("wx")), 63), "unknown opcode")
    l0 = FieldLayout.face(3, (6, 3, 5), 1, 0)
    refused(hip, T.bc_start(l0), lambda x: hip.apply_bc_face(1, l0.c_struct(), x, T.EGEOM, T.DIRICHLET, e, 1), "no ghost layer")


# ---- the _grid entry points -------------------------------------------------------------------------------------------------------------
def _grid(hip, tables, ghost):
    g, keep = GridC(), []
    for d, t in enumerate(tables):
        keep.append(hip.from_host(np.array(t)))
        g.nodes[d], g.n[d] = hip.ptr(keep[-1]), len(t)
    g.ghost = ghost
    return g, keep


@pytest.mark.parametrize("pname", sorted(T.GRID_PROGRAMS))
def test_fill_and_max_err_expr_grid(hip, pname):
    l, L = T.GRID_LAYOUT, T.GRID_LAYOUT.c_struct()
    g, keep = _grid(hip, T.grid_tables(), T.GRID_GHOST)
    ex, (b, e) = expr(T.GRID_PROGRAMS[pname]), T.GRID_FILL_BOX
    want = T.grid_fill_reference(pname)
    same(run(hip, np.full(l.size, SENTINEL), lambda x: hip.fill_expr_grid(L, x, g, ex, b, e)), want)
    assert value(hip, hip.max_err_expr_grid(L, hip.from_host(np.array(want)), g, ex, b, e)) == 0.0
    for where, p in T.plants(b, e).items():
        a = np.array(want)
        a[l.linear(*p)] += 3.0
        assert value(hip, hip.max_err_expr_grid(L, hip.from_host(a), g, ex, b, e)) == 3.0, where


@pytest.mark.parametrize("mask", T.GRID_MASKS)
@pytest.mark.parametrize("pname", sorted(T.GRID_PROGRAMS))
def test_apply_dirichlet_expr_grid(hip, pname, mask):
    l, L = T.GRID_LAYOUT, T.GRID_LAYOUT.c_struct()
    g, keep = _grid(hip, T.grid_tables(), T.GRID_GHOST)
    got = run(hip, np.full(l.size, SENTINEL), lambda x: hip.apply_dirichlet_expr_grid(L, x, g, expr(T.GRID_PROGRAMS[pname]), mask))
    same(got, T.grid_dirichlet_reference(pname, mask))


def test_grid_entry_points_refuse_a_box_the_tables_do_not_cover(hip):
    l, L = T.GRID_LAYOUT, T.GRID_LAYOUT.c_struct()
    start, ex = np.full(l.size, SENTINEL), expr(T.GRID_PROGRAMS["poly"])
    b, e = T.GRID_FILL_BOX
    tables = T.grid_tables()
    # no ghost node in front of the lower ghost point; the upper node of the last point's cell missing
    for tabs, ghost in (([t[2:] for t in tables], 0), ([tables[0], tables[1][:-2], tables[2]], T.GRID_GHOST)):
        g, keep = _grid(hip, tabs, ghost)
        refused(hip, start, lambda x: hip.fill_expr_grid(L, x, g, ex, b, e), "node table of axis")
        refused(hip, start, lambda x: hip.apply_dirichlet_expr_grid(L, x, g, ex, 63), "node table of axis")
        with pytest.raises(ExamgError, match="node table of axis"):
            hip.max_err_expr_grid(L, hip.from_host(start.copy()), g, ex, b, e)
