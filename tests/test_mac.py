"""CPU checks of the staggered-grid layer on its numpy restatement (tests/mac_ops.py): face layouts, the three-field operator against an
independently assembled dense matrix, the box smoother against the equations it solves, the decoupling claim of the accepted
colourings, the transfer pair, the boundary rules; then the Stokes driver (exastencils_amd/stokes.py) on the restatement."""
import itertools
import os

import numpy as np
import pytest

from mac_cases import H, MacData, boxes, colouring, parity, row_boxes
from mac_ops import BC_DIRICHLET, BC_NEUMANN, SYS_APPLY, SYS_RESIDUAL, MacError, MacOracleOps

from exastencils_amd.field import Colouring, MacSystem, Stencil
from exastencils_amd.layout import FieldLayout
from exastencils_amd.lib import ExprC, GeomC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def orc():
    return MacOracleOps()


def _geom(h=H, pb=(0.25, -0.5, 1.0)):
    g = GeomC()
    for d in range(3):
        g.pos_begin[d], g.h[d] = pb[d], h[d]
    return g


# x * 3 + y * 5 - z * 7 + 1: every operation exact on the dyadic positions of _geom where h is a power of two; used with tolerance-free
# comparisons only between the restatement and hand-written numpy, which round alike
POLY = ExprC.from_program([("x", None), ("const", 3.0), ("*", None), ("y", None), ("const", 5.0), ("*", None), ("+", None), ("z", None),
                           ("const", 7.0), ("*", None), ("-", None), ("const", 1.0), ("+", None)])


def poly(x, y, z):
    return (((x * 3.0) + (y * 5.0)) - (z * 7.0)) + 1.0


# -- layouts ----------------------------------------------------------------------------------------------------------------------------
def test_face_layouts_follow_the_reference_declaration():
    l = FieldLayout.face(3, (6, 4, 5), 1, 2)
    assert l.localization == "face_y" and l.is_face and l.face_axis == 1 and not l.is_cell
    assert l.dup == (0, 1, 0) and l.inner == (6, 3, 5) and l.ghost == (2, 2, 2) and l.ncells == (6, 4, 5)
    assert l.loop_box() == ([0, 0, 0], [6, 5, 5])      # [0, n + 1) on the own axis, [0, n) on the others
    assert l.idx("DLB", 1) == 0 and l.idx("DRE", 1) == 5 and l.idx("GLB", 0) == -2
    c = l.c_struct()
    assert list(c.dup_l) == [0, 1, 0] and list(c.dup_r) == [0, 1, 0] and list(c.inner) == [6, 3, 5]
    a = FieldLayout.face(2, (7, 3), 0, 1, align=2)
    assert (a.pad_l[0] + a.ghost[0]) % 2 == 0 and a.tot(0) % 2 == 0 and a.inner[:2] == (6, 3)
    assert FieldLayout.node(2, (4, 4), 1).face_axis is None and not FieldLayout.cell(2, (4, 4), 1).is_face
    with pytest.raises(ValueError):
        FieldLayout.face(2, (4, 4), 2, 1)


# -- the operator -----------------------------------------------------------------------------------------------------------------------
def _dense(sys, nd, rb, re):
    """Row r of the operator as a dense matrix over the concatenated arrays u_0 .., p (ghost layers and padding included), assembled
    point by point from the definition: independent of the slices of the restatement."""
    ls = list(sys.lu) + [sys.lp]
    base = np.cumsum([0] + [l.size for l in ls])
    rows = []
    for r in range(nd + 1):
        pts = list(itertools.product(range(rb[r][2], re[r][2]), range(rb[r][1], re[r][1]), range(rb[r][0], re[r][0])))
        M = np.zeros((len(pts), base[-1]))
        for k, (i2, i1, i0) in enumerate(pts):
            i = (i0, i1, i2)
            if r < nd:
                for o, c in zip(sys.A[r].offsets, sys.A[r].coefs):
                    M[k, base[r] + ls[r].linear(*[i[t] + o[t] for t in range(3)])] += c
                M[k, base[nd] + ls[nd].linear(*i)] += sys.bc[r]
                M[k, base[nd] + ls[nd].linear(*[i[t] - (t == r) for t in range(3)])] += sys.bm[r]
            else:
                for d in range(nd):
                    M[k, base[d] + ls[d].linear(*i)] += sys.cc[d]
                    M[k, base[d] + ls[d].linear(*[i[t] + (t == d) for t in range(3)])] += sys.cp[d]
        rows.append((pts, M))
    return rows


@pytest.mark.parametrize("nd,cells", [(2, (6, 3)), (2, (4, 5)), (3, (3, 3, 3)), (3, (4, 3, 2))])
@pytest.mark.parametrize("kind", ["asymmetric", "stokes", "few"])
def test_mac_op_equals_an_independent_dense_matrix(orc, nd, cells, kind):
    D = MacData(orc, nd, cells, ghost=1, kind=kind)
    y = D.sys
    rb, re = row_boxes(nd, cells, boxes(nd, cells)["whole"])
    x = np.concatenate([t.numpy().ravel() for t in y.u + [y.p]])
    f = [t.numpy().copy() for t in y.f + [y.fp]]
    rows = _dense(y, nd, rb, re)
    for mode in (SYS_APPLY, SYS_RESIDUAL):
        orc.mac_op(mode, y, (1 << (nd + 1)) - 1, rb, re)
        for r, (pts, M) in enumerate(rows):
            want = M @ x
            scale = np.abs(M) @ np.abs(x)
            ld, dst = (y.ld[r], y.dst[r]) if r < nd else (y.ldp, y.dstp)
            lf = y.lf[r] if r < nd else y.lfp
            got = np.array([dst.numpy()[ld.linear(i0, i1, i2)] for i2, i1, i0 in pts])
            if mode == SYS_RESIDUAL:
                fv = np.array([f[r][lf.linear(i0, i1, i2)] for i2, i1, i0 in pts])
                want, scale = fv - want, scale + np.abs(fv)
            assert np.all(np.abs(got - want) <= 1e-13 * scale), (r, mode)


def test_mac_op_writes_the_rows_of_the_mask_only(orc):
    nd, cells = 2, (6, 3)
    rb, re = row_boxes(nd, cells, boxes(nd, cells)["sub"])
    for mask in (1, 2, 4):
        D = MacData(orc, nd, cells)
        before = [t.numpy().copy() for t in D.arrays()]
        orc.mac_op(SYS_RESIDUAL, D.sys, mask, rb, re)
        changed = [k for k, (a, t) in enumerate(zip(before, D.arrays())) if not np.array_equal(a, t.numpy())]
        assert changed == [2 * (nd + 1) + mask.bit_length() - 1]


# -- the box smoother -------------------------------------------------------------------------------------------------------------------
def _abs_system(y):
    """The system with |coefficients| on |values|: its APPLY rows are the scale of the rows' rounding errors."""
    from torch import from_numpy

    ab = lambda t: from_numpy(np.abs(t.numpy()))
    A = [Stencil(s.offsets, [abs(c) for c in s.coefs]) for s in y.A]
    return MacSystem(nd=y.nd, lu=y.lu, u=[ab(t) for t in y.u], lp=y.lp, p=ab(y.p), A=A, bc=np.abs(y.bc), bm=np.abs(y.bm), cc=np.abs(y.cc),
                     cp=np.abs(y.cp), lf=y.lf, f=y.f, lfp=y.lfp, fp=y.fp, ld=y.ld, dst=[t.clone() for t in y.dst], ldp=y.ldp, dstp=y.dstp.clone())


def _colour_cells(col, b, e):
    return [c for c in itertools.product(*[range(b[d], e[d]) for d in range(3)])
            if all((shift + sum(c[d] for d in axes)) % mod == rem for (axes, shift, mod), rem in zip(col.exprs, col.rem))]


@pytest.mark.parametrize("nd,cells", [(2, (6, 3)), (2, (12, 9)), (3, (3, 3, 3)), (3, (6, 3, 6))])
@pytest.mark.parametrize("kind", ["asymmetric", "stokes", "few"])
def test_after_a_colour_the_equations_of_its_cells_hold(orc, nd, cells, kind):
    """relax = 1: the 2 * nd + 1 equations of every updated cell -- the rows of its faces that are not held and its continuity row -- have
    a residual of at most 1e-12 times the row's scale (sum of |coefficient * value| and |f|); held faces, the cells of the other colours
    and everything outside the box keep their bits."""
    b, e = boxes(nd, cells)["whole"]
    rb, re = row_boxes(nd, cells, (b, e))
    for col in colouring(nd).colours():
        D = MacData(orc, nd, cells, kind=kind)
        y = D.sys
        before = [t.numpy().copy() for t in y.u + [y.p]]
        orc.mac_relax(y, 1.0, col, b, e)
        orc.mac_op(SYS_RESIDUAL, y, (1 << (nd + 1)) - 1, rb, re)
        S = _abs_system(y)
        orc.mac_op(SYS_APPLY, S, (1 << (nd + 1)) - 1, rb, re)
        mine = _colour_cells(col, b, e)
        assert mine
        touched = [set() for _ in range(nd + 1)]
        for c in mine:
            rows = [(nd, c)]
            for d in range(nd):
                for s in (0, 1):
                    face = tuple(c[t] + (s if t == d else 0) for t in range(3))
                    if face[d] not in (0, cells[d]):
                        rows.append((d, face))
            for r, i in rows:
                touched[r].add(i)
                ld, lf = (y.ld[r], y.lf[r]) if r < nd else (y.ldp, y.lfp)
                res = (y.dst[r] if r < nd else y.dstp).numpy()[ld.linear(*i)]
                scale = (S.dst[r] if r < nd else S.dstp).numpy()[ld.linear(*i)] + abs((y.f[r] if r < nd else y.fp).numpy()[lf.linear(*i)])
                assert abs(res) <= 1e-12 * scale, (col.rem, r, i, res, scale)
        for r, (old, t) in enumerate(zip(before, y.u + [y.p])):
            l = y.lu[r] if r < nd else y.lp
            keep = np.ones(old.shape, dtype=bool)
            for i in touched[r]:
                keep[l.linear(*i)] = False
            assert np.array_equal(old[keep], t.numpy()[keep]), "row %d: a value outside the colour's boxes changed" % r
            assert not np.array_equal(old[~keep], t.numpy()[~keep])


@pytest.mark.parametrize("nd,cells", [(2, (6, 3)), (2, (7, 8)), (3, (6, 3, 6))])
def test_a_sweep_gives_the_same_bits_in_any_cell_order(orc, nd, cells):
    """The decoupling claim: the cells of a colour one at a time forwards, one at a time backwards, and all at once."""
    b, e = boxes(nd, cells)["whole"]

    def run(order):
        D = MacData(orc, nd, cells)
        for col in colouring(nd).colours():
            mine = _colour_cells(col, b, e)
            orc.mac_relax(D.sys, 0.8, col, b, e, cells=None if order is None else mine[::order])
        return [t.numpy().copy() for t in D.arrays()]

    whole, fwd, bwd = run(None), run(1), run(-1)
    for a, f_, r_ in zip(whole, fwd, bwd):
        assert np.array_equal(a, f_) and np.array_equal(a, r_)


def test_under_the_parity_colouring_the_order_would_matter_and_it_is_refused(orc):
    nd, cells = 2, (6, 3)
    b, e = boxes(nd, cells)["whole"]
    D = MacData(orc, nd, cells)
    before = [t.numpy().copy() for t in D.arrays()]
    for entry in (orc.mac_relax, orc.mac_sweep):
        with pytest.raises(MacError, match=r"does not decouple the boxes: cells i and i \+ \(-1, -1, 0\)"):
            entry(D.sys, 0.8, next(parity(nd).colours()), b, e)
    # `i0 % 2, i1 % 2` separates the neighbours but not the cells two apart, whose boxes share a face's star
    with pytest.raises(MacError, match=r"cells i and i \+ \(-2, 0, 0\)"):
        orc.mac_relax(D.sys, 0.8, next(Colouring.axis_parity(nd).colours()), b, e)
    # separating, but not of the form the kernel enumerates
    with pytest.raises(MacError, match="one expression"):
        orc.mac_relax(D.sys, 0.8, next(Colouring((((0,), 0, 3), ((0, 1), 0, 3))).colours()), b, e)
    assert all(np.array_equal(a, t.numpy()) for a, t in zip(before, D.arrays()))


def test_sweep_is_its_colours_in_the_reference_order(orc):
    nd, cells = 2, (7, 5)
    b, e = boxes(nd, cells)["whole"]
    A, B = MacData(orc, nd, cells), MacData(orc, nd, cells)
    orc.mac_sweep(A.sys, 0.8, colouring(nd), b, e)
    rems = []
    for col in colouring(nd).colours():
        rems.append(col.rem)
        orc.mac_relax(B.sys, 0.8, col, b, e)
    assert rems[:4] == [(0, 0), (1, 0), (2, 0), (0, 1)]      # the first expression fastest
    assert all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(A.arrays(), B.arrays()))


def test_restatement_refusals(orc):
    nd, cells = 2, (6, 3)
    b, e = boxes(nd, cells)["whole"]
    rb, re = row_boxes(nd, cells, (b, e))
    col = next(colouring(nd).colours())

    def fresh(**kw):
        D = MacData(orc, nd, cells)
        for k, v in kw.items():
            setattr(D.sys, k, v)
        return D.sys

    y = fresh()
    cases = [
        (fresh(lp=FieldLayout.node(nd, cells, 1)), "pressure layout is not a cell layout"),
        (fresh(lu=[y.lu[1], y.lu[1]]), "u_0 layout is not a face layout of axis 0"),
        (fresh(lp=FieldLayout.cell(nd, cells, 0)), "the pressure has no ghost layer"),
        (fresh(lu=[FieldLayout.face(nd, (5, 3), 0, 1), y.lu[1]]), "has 5 cells in dim 0, the pressure 6"),
        (fresh(A=[Stencil([(0, 0, 0), (2, 0, 0)], [1.0, 1.0]), y.A[1]]), "not the centre or an axis neighbour at distance 1"),
        (fresh(A=[Stencil([(0, 0, 0), (1, 1, 0)], [1.0, 1.0]), y.A[1]]), "not the centre or an axis neighbour"),
        (fresh(A=[Stencil([(0, 0, 0), (1, 0, 0), (1, 0, 0)], [1.0, 1.0, 1.0]), y.A[1]]), "repeats the offset"),
        (fresh(A=[Stencil([(1, 0, 0)], [1.0]), y.A[1]]), "has no centre entry"),
        (fresh(nd=4), "2-D or 3-D"),
        (fresh(lp=FieldLayout.cell(nd, cells, 1).split_x()), "layout transformation"),
    ]
    for sys, text in cases:
        with pytest.raises(MacError, match=text):
            orc.mac_op(SYS_RESIDUAL, sys, 7, rb, re)
        with pytest.raises(MacError, match=text):
            orc.mac_relax(sys, 1.0, col, b, e)
    with pytest.raises(MacError, match="destination 0 is unknown 0"):
        s = fresh()
        s.dst, s.ld = [s.u[0], s.dst[1]], [s.lu[0], s.ld[1]]
        orc.mac_op(SYS_APPLY, s, 1, rb, re)
    with pytest.raises(MacError, match="leaves the allocation of u_0"):
        orc.mac_op(SYS_APPLY, fresh(), 1, [[-1, 0, 0]] * 3, re)
    with pytest.raises(MacError, match="leaves the cells"):
        orc.mac_relax(fresh(), 1.0, col, [0, 0, 0], [7, 3, 1])
    with pytest.raises(MacError, match="determinant zero"):
        orc.mac_relax(fresh(A=[Stencil([(0, 0, 0), (1, 0, 0), (-1, 0, 0)], [1.0, 1.0, 1.0]), y.A[1]]), 1.0, col, b, e)
    with pytest.raises(MacError, match="Schur complement"):
        one = MacData(orc, 2, (1, 1))
        orc.mac_relax(one.sys, 1.0, col, [0, 0, 0], [1, 1, 1])
    with pytest.raises(ValueError, match="vector-valued"):
        orc.mac_op(SYS_APPLY, fresh(lp=FieldLayout.cell(nd, cells, 1).as_vector(2)), 7, rb, re)


# -- transfers ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd,coarse", [(2, (3, 2)), (2, (2, 3)), (3, (2, 2, 3))])
def test_prolongation_is_two_to_the_d_times_the_transposed_restriction(orc, nd, coarse):
    fine = tuple(2 * c for c in coarse)
    for axis in range(nd):
        lf, lc = FieldLayout.face(nd, fine, axis, 1), FieldLayout.face(nd, coarse, axis, 1)
        fb, fe = lf.loop_box()
        cb, ce = lc.loop_box()
        fpts = [lf.linear(*i[::-1]) for i in itertools.product(range(fb[2], fe[2]), range(fb[1], fe[1]), range(fb[0], fe[0]))]
        cpts = [lc.linear(*i[::-1]) for i in itertools.product(range(cb[2], ce[2]), range(cb[1], ce[1]), range(cb[0], ce[0]))]
        R = np.zeros((len(cpts), len(fpts)))
        P = np.zeros((len(fpts), len(cpts)))
        for k, f in enumerate(fpts):
            x, out = orc.new_array(lf.size), orc.new_array(lc.size)
            x.zero_()
            out.zero_()
            x[f] = 1.0
            orc.restrict_face(axis, lf, x, lc, out, 1.0, cb, ce)
            R[:, k] = out.numpy()[cpts]
        for k, c in enumerate(cpts):
            x, out = orc.new_array(lc.size), orc.new_array(lf.size)
            x.zero_()
            out.zero_()
            x[c] = 1.0
            orc.prolong_add_face(axis, lc, x, lf, out, fb, fe)
            P[:, k] = out.numpy()[fpts]
            assert np.count_nonzero(out.numpy()) == np.count_nonzero(P[:, k])      # nothing outside the box
        assert np.array_equal(P, (2.0 ** nd) * R.T)
        assert np.array_equal(P.sum(axis=1), np.ones(len(fpts)))      # constants are reproduced, boundary faces included


# -- boundary rules -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd,cells", [(2, (4, 3)), (3, (3, 4, 2))])
def test_boundary_rules_on_every_wall(orc, nd, cells):
    """Walls normal to the field's axis: the boundary face takes g at its position.  The other walls: ghost = 2 g(wall point) - interior,
    or the interior value.  Each wall alone, then all at once; everything else keeps its bits."""
    geom = _geom((0.125, 0.25, 0.5))
    n = list(cells) + [1] * (3 - nd)
    for axis in range(nd):
        l = FieldLayout.face(nd, cells, axis, 1)
        lo, hi = l.loop_box()

        def pos(i):
            return [i[d] * geom.h[d] + geom.pos_begin[d] + (0.0 if d == axis else 0.5 * geom.h[d]) for d in range(3)]

        for kind in (BC_DIRICHLET, BC_NEUMANN):
            walls = [(d, s) for d in range(nd) for s in (0, 1) if kind == BC_DIRICHLET or d != axis]
            for mask_walls in [[w] for w in walls] + [walls]:
                x = orc.new_array(l.size)
                orc.fill_random(x, 900 + axis)
                old = x.numpy().copy()
                want = old.copy()
                order = [w for w in mask_walls if w[0] == axis] + [w for w in mask_walls if w[0] != axis]
                for d, s in order:
                    for i in itertools.product(*[range(lo[t], hi[t]) for t in range(3)]):
                        if d == axis and i[d] == (n[d] if s else 0):
                            want[l.linear(*i)] = poly(*pos(i))
                        elif d != axis and i[d] == (n[d] - 1 if s else 0):
                            g = list(i)
                            g[d] += 1 if s else -1
                            wp = pos(i)
                            wp[d] = (n[d] if s else 0) * geom.h[d] + geom.pos_begin[d]
                            want[l.linear(*g)] = want[l.linear(*i)] if kind == BC_NEUMANN else 2.0 * poly(*wp) - want[l.linear(*i)]
                mask = sum(1 << (2 * d + s) for d, s in mask_walls)
                orc.apply_bc_face(axis, l, x, geom, kind, POLY if kind == BC_DIRICHLET else None, mask)
                assert np.array_equal(x.numpy(), want), (axis, kind, mask_walls)
                assert not np.array_equal(x.numpy(), old)
        with pytest.raises(MacError, match="Neumann wall normal"):
            orc.apply_bc_face(axis, l, x, geom, BC_NEUMANN, None, 1 << (2 * axis))
        with pytest.raises(MacError, match="not a face layout of axis"):
            orc.apply_bc_face(axis, FieldLayout.cell(nd, cells, 1), x, geom, BC_NEUMANN, None, 0)


def test_expressions_at_the_face_positions(orc):
    nd, cells, geom = 3, (3, 2, 4), _geom((0.125, 0.25, 0.5))
    for axis in range(nd):
        l = FieldLayout.face(nd, cells, axis, 1)
        b, e = l.loop_box()
        x = orc.new_array(l.size)
        x.zero_()
        orc.fill_expr_face(axis, l, x, geom, POLY, b, e)
        for i in itertools.product(*[range(b[t], e[t]) for t in range(3)]):
            p = [i[d] * geom.h[d] + geom.pos_begin[d] + (0.0 if d == axis else 0.5 * geom.h[d]) for d in range(3)]
            assert x.numpy()[l.linear(*i)] == poly(*p)
        assert np.count_nonzero(x.numpy()) <= (e[0] - b[0]) * (e[1] - b[1]) * (e[2] - b[2])
        assert orc.max_err_expr_face(axis, l, x, geom, POLY, b, e)[0] == 0.0
        x[l.linear(1, 1, 1)] += 0.375
        assert orc.max_err_expr_face(axis, l, x, geom, POLY, b, e)[0] == 0.375


# -- the Stokes driver on the restatement ---------------------------------------------------------------------------------------------------
from exastencils_amd.stokes import ConfigStokes, StokesSolver  # noqa: E402

FINEST = {2: 5, 3: 3}      # 96^2 and 24^3 cells
_SOLVED = {}


def solved(nd, hi, problem="trigonometric"):
    """One solve per size, shared by the tests and left unchanged."""
    key = (nd, hi, problem)
    if key not in _SOLVED:
        S = StokesSolver(MacOracleOps(), ConfigStokes(nd=nd, max_level=hi, problem=problem))
        S.Solve()
        _SOLVED[key] = S
    return _SOLVED[key]


@pytest.mark.parametrize("nd", [2, 3])
def test_driver_reaches_the_tolerance_within_the_cap_and_prints_the_golden(nd):
    S = solved(nd, FINEST[nd])
    print("cycles %d, residuals %s" % (S.iterations, ["%.3e" % r for r in S.res_history]))
    assert S.iterations <= 30 and S.res_history[-1] <= 1e-10 * S.res_history[0]
    with open(os.path.join(ROOT, "tests", "golden", "own", "stokes%dd.results" % nd)) as f:
        assert "\n".join(S.log) + "\n" == f.read()
    assert len(S.log) == 2 + S.iterations * (nd + 2) and S.log[-1] == str(S.iterations)


@pytest.mark.parametrize("nd", [2, 3])
def test_velocity_errors_fall_with_second_order(nd):
    """Between the two finest levels the maximum errors of the velocities fall by at least 3 (second order gives 4; the margin is for the
    pre-asymptotic range).  The pressure errors are printed, not bounded."""
    coarse, fine = solved(nd, FINEST[nd] - 1), solved(nd, FINEST[nd])
    ec, ef = coarse.err_history[-1], fine.err_history[-1]
    print("errors at level %d: %s, at level %d: %s, ratios %s" % (FINEST[nd] - 1, ec, FINEST[nd], ef, [a / b for a, b in zip(ec, ef)]))
    for d in range(nd):
        assert ec[d] / ef[d] >= 3.0


@pytest.mark.parametrize("nd", [2, 3])
def test_the_scheme_is_exact_for_the_quadratic_field(orc, nd):
    """The polynomial problem lies in the scheme's range: the exact solution on the grid, boundary values by `apply bc`, has a residual of
    rounding size in all rows -- operator, gradient, divergence, right-hand sides and the ghost rules agree with each other.  Bound: a row
    is at most 13 roundings (7 + 2 products, their sums, the subtraction) of at most eps / 2 each on partial sums below
    S = sum |c_k| max|u| + (|bc| + |bm|) max|p| + max|f|, and its inputs carry a few eps of their own (position, two or three operations
    of the program, the ghost rule): 32 eps S holds with room, and a wrong sign, weight or position misses it by twelve orders."""
    hi = 2
    S = StokesSolver(orc, ConfigStokes(nd=nd, max_level=hi, problem="polynomial"))
    L, y = S.levels[hi], S.levels[hi].sys
    for d in range(nd):
        orc.fill_expr_face(d, y.lu[d].c_struct(), y.u[d], L.geom, S.sol_u[d], *L.face_box[d])
    orc.fill_expr_cell(y.lp.c_struct(), y.p, L.geom, S.sol_p, *L.cell_box)
    S.apply_bc(hi)
    S.UpdateRes(hi)
    big = lambda ts: max(float(np.abs(t.numpy()).max()) for t in ts)
    scale = sum(abs(c) for c in y.A[0].coefs) * big(y.u) + (abs(y.bc[0]) + abs(y.bm[0])) * big([y.p]) + big(y.f + [y.fp])
    worst = big(y.dst + [y.dstp])
    print("largest residual %.3e, bound %.3e" % (worst, 32 * np.finfo(float).eps * scale))
    assert worst <= 32 * np.finfo(float).eps * scale
    assert big(y.u) > 1.0 and big([y.p]) > 0.5      # (the fields are not zero)


def test_every_cycle_statement_is_the_header_entry_point():
    """The cycle issues the library's entry points and nothing else: per level and sweep one mac_relax and nd + 1 `apply bc` per colour, the
    residual is ONE mac_op."""
    calls = []

    class Counting(MacOracleOps):
        def __getattribute__(self, name):
            v = MacOracleOps.__getattribute__(self, name)
            if callable(v) and not name.startswith("_") and name not in ("new_array", "new_scalar", "ptr", "to_host", "scalar_value"):
                calls.append(name)
            return v

    S = StokesSolver(Counting(), ConfigStokes(nd=2, max_level=2, coarse_sweeps=3))
    del calls[:]
    S.mgCycle(2)
    n = {k: calls.count(k) for k in set(calls)}
    assert n == {"mac_relax": 9 * (4 + 4 + 3), "apply_bc_face": 2 * (9 * 11 + 2), "apply_bc_cell": 9 * 11 + 2, "mac_op": 1, "restrict_face": 2,
                 "restrict_cell": 1, "set": 3, "prolong_add_face": 2, "prolong_add_cell": 1}
