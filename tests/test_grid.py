"""Axis-aligned non-uniform grids without a GPU: the node tables of `linearFct` against a second restatement of the three formulas, the
uniform fold of the virtual-field constructs (the reference's finite-volume programs run as constant stencils, one of them against its
checked-in results file), the separation of a stencil entry into per-axis tables against the entry evaluated as written, the
consistency of the example operator on a graded grid, the refusals by name, and the goldens of the two example programs.  Everything
runs on the numpy restatement of the new entry points (tests/grid_ops.py)."""
import os
import re

import numpy as np
import pytest

import grid_cases as G
from grid_ops import APPLY, GridOracleOps
from test_exa4 import REF

from exastencils_amd import exa4, knowledge
from exastencils_amd.exa4_parser import Exa4Unsupported, Parser, _classify_transfer
from exastencils_amd.grid import GHOST, AxisGrid, coarsen_nodes, linear_fct_nodes, uniform_nodes

REFDIR = os.path.join(REF, "Examples", "Poisson")
U = 2.0 ** -53


class Recording(GridOracleOps):
    """Records the name of every kernel-layer call."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def __getattribute__(self, name):
        a = object.__getattribute__(self, name)
        if callable(a) and not name.startswith("_") and name not in ("new_array", "new_scalar", "ptr", "to_host", "from_host", "scalar_value",
                                                                     "synchronize", "axis_coefficients"):
            calls = object.__getattribute__(self, "calls")

            def rec(*args, **kw):
                calls.append(name)
                return a(*args, **kw)

            return rec
        return a


NEW_OPS = ("axis_op", "axis_route", "fill_expr_grid", "apply_dirichlet_expr_grid", "max_err_expr_grid")


# -- 1, 2: the uniform fold ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir(REFDIR), reason="reference checkout not present")
def test_reference_fv_program_with_its_knowledge_file_reproduces_its_results_file():
    from oracle import mg

    k = knowledge.parse_file(os.path.join(REF, "Testing", "Poisson", "2D_FV_Poisson_fromL4.knowledge"))
    with open(os.path.join(REFDIR, "2D_FV_Poisson_fromL4.exa4")) as f:
        ops = Recording()
        P = exa4.Exa4Program(f.read(), k, ops=ops)
    out = P.run()
    with open(os.path.join(REF, "Testing", "Poisson", "2D_FV_Poisson_fromL4.results")) as f:
        want = f.read()
    assert len(want.split()) == 17
    assert mg.compare_with_golden(out, want) == []      # Testing/run_test.py:12-42
    assert not set(ops.calls) & set(NEW_OPS)


def constants_by_hand(text, nd):
    """The three constructs written as what they fold to on a uniform grid: widths -> vf_gridWidth_*, the cell volume -> the product of the
    widths, NodeRestrictionForRes -> 2^nd times the linear restriction."""
    text = re.sub(r"vf_cellWidth_([xyz])(@\[[^\]]*\])?", r"vf_gridWidth_\1", text)
    text = text.replace("vf_cellVolume", "( " + " * ".join("vf_gridWidth_" + a for a in "xyz"[:nd]) + " )")
    text = re.sub(r"Stencil NodeRestrictionForRes@all \{.*?\n\}", "Stencil NodeRestrictionForRes@all from default restriction on Node with 'linear'",
                  text, flags=re.S)
    text = text.replace("= NodeRestrictionForRes * Residual", "= %s * NodeRestrictionForRes * Residual" % float(2 ** nd))
    assert "vf_cellWidth" not in text and "@[" not in text
    return text


@pytest.mark.skipif(not os.path.isdir(REFDIR), reason="reference checkout not present")
def test_uniform_fold_equals_the_constant_stencil_written_by_hand():
    k = knowledge.parse_file(os.path.join(REFDIR, "3D_FV_Poisson_fromL4.knowledge"))
    k.update(minLevel=2, maxLevel=4)
    with open(os.path.join(REFDIR, "3D_FV_Poisson_fromL4.exa4")) as f:
        text = f.read()
    runs = []
    for t in (text, constants_by_hand(text, 3)):
        ops = Recording()
        P = exa4.Exa4Program(t, dict(k), ops=ops)
        runs.append(([line for line in P.run() if "Timer" not in line], list(ops.calls), P))      # wall-clock lines apart
    assert runs[0][0] == runs[1][0] and len(runs[0][0]) > 4
    assert runs[0][1] == runs[1][1]                      # call for call the same kernels ...
    assert not set(runs[0][1]) & set(NEW_OPS)            # ... and none of the new ones
    assert [float(v).hex() for v in runs[0][2].printed_values] == [float(v).hex() for v in runs[1][2].printed_values]
    A = runs[0][2].stencil("Laplace", 4)
    assert A.cfield is None and not getattr(A, "is_axis", False) and A.coefs == runs[1][2].stencil("Laplace", 4).coefs


def test_restriction_with_a_common_factor_is_classified_with_its_factor():
    lin = {-1.0: 0.25, 0.0: 0.5, 1.0: 0.25}
    for factor in (1.0, 4.0, 0.25):
        mapped = [([("bin", "+", ("bin", "*", ("num", 2.0), ("id", "i0", None)), ("num", a)),
                    ("bin", "+", ("bin", "*", ("num", 2.0), ("id", "i1", None)), ("num", b))], ("num", factor * lin[a] * lin[b]))
                  for a in (-1.0, 0.0, 1.0) for b in (-1.0, 0.0, 1.0)]
        assert _classify_transfer(mapped, with_factor=True) == ("restriction", factor)
        if factor != 1.0:
            with pytest.raises(Exa4Unsupported, match="not the linear restriction"):
                _classify_transfer(mapped)
    with pytest.raises(Exa4Unsupported, match="not the linear prolongation"):
        Parser("Stencil P@all {\n" + "\n".join("[i0] from [0.5 * ( i0 + %s )] with %s" % (o, w) for o, w in (("1.0", 1.0), ("0.0", 2.0), ("-1.0", 1.0))) + "\n}").parse()


# -- 3: the tables ------------------------------------------------------------------------------------------------------------------------
def literal_linear_fct(n, lo, hi):
    """IR_SetupNodePositions.scala:137-157, 222-231 once more, node by node, with Python floats."""
    xf, xs = n // 4 - 1, (n // 4) * 3
    a_coeff = -0.5 * xf * xf - 0.5 * xf + xf * n - 0.5 * n * n + 0.5 * n + n * xs - 0.5 * xs * xs - 0.5 * xs
    factor = (n // 4) / 8.0
    alpha = (hi - lo) / (a_coeff + n * factor)
    beta = factor * alpha
    out = []
    for i in range(n + 1):
        if i <= xf + 1:
            out.append(lo + 0.5 * alpha * i * i + (beta - 0.5 * alpha) * i)
        elif i <= xs + 1:
            out.append(lo - 0.5 * alpha * (xf * xf + xf) + (beta + alpha * xf) * i)
        else:
            out.append(lo - 0.5 * alpha * i * i + (alpha * xf + alpha * xs + 0.5 * alpha + beta) * i - 0.5 * alpha * (xf * xf + xf + xs * xs + xs))
    return out


@pytest.mark.parametrize("n", [8, 16, 64])
@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-1.0, 3.0)])
def test_linear_fct_tables(n, lo, hi):
    x = linear_fct_nodes(n, lo, hi)
    inner = x[GHOST:-GHOST]
    assert len(x) == n + 1 + 2 * GHOST
    assert [float(v).hex() for v in inner] == [float(v).hex() for v in literal_linear_fct(n, lo, hi)]
    assert inner[0] == lo
    w = inner[1:] - inner[:-1]
    assert np.all(w > 0.0)
    # every node is a handful of operations on numbers below 2 * max(|lo|, |hi|, hi - lo): its rounding error is below 16 u of that, a
    # width's and the difference of two widths' a small multiple; the end of the axis, the sum of all widths, carries the same
    tol = 64 * U * max(abs(lo), abs(hi), hi - lo)
    assert np.all(np.abs(w - w[::-1]) <= tol) and abs(inner[-1] - hi) <= tol
    print("n", n, "width ratio", w.max() / w.min())
    # ghost nodes: the extrapolation, the inner one first
    assert x[1] == 2.0 * x[2] - x[3] and x[0] == 2.0 * x[1] - x[2]
    assert x[-2] == 2.0 * x[-3] - x[-4] and x[-1] == 2.0 * x[-2] - x[-3]
    c = coarsen_nodes(x)
    assert np.array_equal(c[GHOST:-GHOST], inner[::2]) and len(c) == n // 2 + 1 + 2 * GHOST
    assert c[1] == 2.0 * c[2] - c[3] and c[0] == 2.0 * c[1] - c[2] and c[-2] == 2.0 * c[-3] - c[-4] and c[-1] == 2.0 * c[-2] - c[-3]


def test_grid_levels_and_uniform_model():
    g = AxisGrid(3, (0.0, -1.0, 0.0), (1.0, 3.0, 2.0), (32, 16, 64), 2, 4, "linearFct")
    for d, n in enumerate((32, 16, 64)):
        assert g.ncells(4, d) == n and g.ncells(3, d) == n // 2 and g.ncells(2, d) == n // 4
        assert np.array_equal(g.nodes(3, d), coarsen_nodes(g.nodes(4, d))) and np.array_equal(g.nodes(2, d), coarsen_nodes(g.nodes(3, d)))
        assert np.array_equal(g.widths(4, d), g.nodes(4, d)[1:] - g.nodes(4, d)[:-1])
    u = AxisGrid(2, (0.0, 0.0), (1.0, 1.0), (16, 16), 3, 4, "uniform")
    assert np.array_equal(u.nodes(4, 0), uniform_nodes(16, 0.0, 1.0)) and u.nodes(4, 0)[GHOST + 5] == 5 * (1.0 / 16) + 0.0


# -- 4: separation ------------------------------------------------------------------------------------------------------------------------
def direct_entries(kind, nd, grid, shape):
    """The entries of the FD / FV stencil evaluated as written, at every point: plain numpy on broadcast width arrays.  Returns
    (offset -> coefficient array (z, y, x)), and the number of roundings of a term on either side of the comparison."""
    n = [shape[d] + 1 if d < nd else 1 for d in range(3)]

    def w(d, o):          # vf_cellWidth_d@[o] over the node indices of the axis, broadcast
        v = grid.axis_values("cellWidth", G.LVL, d, o)
        s = [1, 1, 1]
        s[2 - d] = n[d]
        return v.reshape(s)

    full = np.zeros((n[2], n[1], n[0]))
    out = {}
    terms = []
    for d in range(nd):
        if kind == "fd":
            lo = 2.0 / (w(d, -1) * (w(d, 0) + w(d, -1)))
            up = 2.0 / (w(d, 0) * (w(d, 0) + w(d, -1)))
        else:
            others = [w(t, 0) for t in range(nd) if t != d]
            area = others[0] if nd == 2 else others[0] * others[1]
            lo = area / (0.5 * (w(d, 0) + w(d, -1)))
            up = area / (0.5 * (w(d, 1) + w(d, 0)))
        off = [0, 0, 0]
        off[d] = -1
        out[tuple(off)] = -lo + full
        off[d] = 1
        out[tuple(off)] = -up + full
        terms += [lo, up]
    c = terms[0]
    for t in terms[1:]:
        c = c + t
    out[(0, 0, 0)] = c + full
    # roundings of one term.  FD as written: the sum, the product, the quotient = 3; separated: the table 1.0 / (h * (h + h)) = 3, the
    # factor 2.0 and the absent tables are exact = 3.  FV as written: the area (3-D only), the sum, the quotient (0.5 * is exact) = 3;
    # separated: the table 1.0 / (0.5 * (h + h)) = 2, (s * Z) * Y = 1 (s = +-1 is exact), X * (..) = 1: 4.
    return out, (3 if kind == "fd" else 4)


@pytest.mark.parametrize("kind", ["fd", "fv"])
@pytest.mark.parametrize("nd", [2, 3])
def test_separated_coefficients_equal_the_entries_as_written(kind, nd):
    shape = (13, 9, 6) if nd == 3 else (21, 10, 0)
    grid = G.random_grid(nd, shape, 7 + nd)
    st = G.separated(G.fd_text(nd) if kind == "fd" else G.fv_text(nd), nd, grid)
    assert len(st.terms) == 4 * nd and all(len(set(t.tobytes() for t in tabs)) == len(tabs) for tabs in st.tables)      # duplicates shared
    b, e = [0, 0, 0], [shape[d] + 1 if d < nd else 1 for d in range(3)]
    ops = GridOracleOps()
    got = ops.axis_coefficients(st.c_struct(ops), b, e)
    want, m_term = direct_entries(kind, nd, grid, shape)
    worst = 0.0
    for k, off in enumerate(st.offsets):
        # the centre adds 2 nd positive terms: 2 nd - 1 more roundings, no cancellation
        m = m_term + (2 * nd - 1 if off == (0, 0, 0) else 0)
        bound = 2 * m * U / (1 - 2 * m * U)
        rel = np.abs(got[k] - want[off]) / np.abs(want[off])
        worst = max(worst, float(rel.max() / bound))
        assert np.all(rel <= bound), (off, float(rel.max()), bound)
    print(kind, nd, "largest difference / bound", worst)


def _program_with_stencil(entries_text, nd=2):
    text = G.own_text(nd)
    return re.sub(r"Stencil Laplace@all \{.*?\n\}", "Stencil Laplace@all {\n" + entries_text + "\n}", text, flags=re.S)


REFUSED_STENCILS = [
    ("[0, 0] => 1.0 / ( vf_cellWidth_x + vf_cellWidth_y )", "stencil Laplace: factor over x and y is not separable"),
    ("[0, 0] => vf_cellWidth_x\n[2, 0] => vf_cellWidth_x", "reaches above 1"),
    ("[0, 0] => vf_cellWidth_x@[2, 0]", "reach above 1"),
    ("[0, 0] => " + " + ".join(["vf_cellWidth_x"] * 33), "33 terms over the grid's virtual fields \\(at most 32\\)"),
    ("[0, 0] => vf_cellWidth_x * RHS", "field"),
    ("[0, 0] => vf_gridWidth_x * vf_cellWidth_y", "vf_gridWidth_x on a non-uniform grid"),
]


@pytest.mark.parametrize("entries_text,words", REFUSED_STENCILS)
def test_stencils_that_do_not_separate_are_refused_by_name(entries_text, words):
    P = exa4.Exa4Program(_program_with_stencil(entries_text), G.own_knowledge(2, maxLevel=3), ops=GridOracleOps())
    with pytest.raises(Exa4Unsupported, match=words):
        P.run()


REFUSED_GRIDS = [
    (dict(grid_spacingModel="diego"), "grid_spacingModel 'diego'"),
    (dict(grid_spacingModel="diego2"), "grid_spacingModel 'diego2'"),
    (dict(grid_spacingModel="blockstructured"), "grid_spacingModel 'blockstructured'"),
    (dict(grid_isAxisAligned=False), "grid_isAxisAligned = false"),
    (dict(domain_rect_periodic_x=True), "periodic axis"),
    (dict(minLevel=1, maxLevel=2), "at least 8 cells per axis"),
]


@pytest.mark.parametrize("over,words", REFUSED_GRIDS)
def test_grids_that_are_not_built_are_refused_by_name(over, words):
    with pytest.raises(Exa4Unsupported, match=words):
        exa4.Exa4Program(G.own_text(2), G.own_knowledge(2, **over), ops=GridOracleOps())


def test_non_uniform_grid_on_two_blocks_is_refused():
    from exastencils_amd.domain import RectDomain

    k = G.own_knowledge(2, domain_rect_numBlocks_x=2)
    with pytest.raises(Exa4Unsupported, match="non-uniform grid on 2 blocks"):
        exa4.Exa4Program(G.own_text(2), k, ops=GridOracleOps(), domain=RectDomain(2, (2, 1, 1), 0, (1, 1, 1)))
    # the merged single block of several fragments is fine
    P = exa4.Exa4Program(G.own_text(2), G.own_knowledge(2, maxLevel=3, domain_rect_numFragsPerBlock_x=2, domain_rect_numFragsPerBlock_y=2), ops=GridOracleOps())
    assert P.grid.ncells(3, 0) == 16


REFUSED_STATEMENTS = [
    ("Solution += 0.8 / diag ( Laplace ) * ( RHS - Laplace * Solution )", "Solution += 0.8 * ( RHS - Laplace * Solution )", "smoother weight on a stencil over the grid's virtual fields"),
    ("Residual = RHS - Laplace * Solution\n  }\n  apply bc to Residual\n\n  communicate Residual", "Residual = RHS - 2.0 * Laplace * Solution\n  }\n  apply bc to Residual\n\n  communicate Residual",
     "none of the recognised kernels"),
    ("fabs ( Solution - (", "fabs ( Solution - ( vf_cellWidth_x@[1, 0] + ", "offset access"),
]


@pytest.mark.parametrize("old,new,words", REFUSED_STATEMENTS)
def test_statements_outside_the_three_loop_forms_are_refused(old, new, words):
    text = G.own_text(2)
    assert old in text
    P = exa4.Exa4Program(text.replace(old, new), G.own_knowledge(2, maxLevel=3), ops=GridOracleOps())
    with pytest.raises(Exa4Unsupported, match=words):
        P.run()


def test_field_offset_access_is_still_refused_word_for_word():
    with pytest.raises(Exa4Unsupported, match=r"line 3: offset access Solution@\[\.\.\.\]"):
        Parser("Field Solution< global, L, None >@all\nFunction F@all {\n  loop over Solution { Solution = Solution@[1, 0] }\n}\n").parse()


# -- 5: consistency of the example operator -----------------------------------------------------------------------------------------------
def test_example_operator_is_exact_for_quadratics_on_a_graded_grid():
    from exastencils_amd.layout import FieldLayout

    ops = GridOracleOps()
    P = exa4.Exa4Program(G.own_text(3), G.own_knowledge(3, maxLevel=4), ops=ops)
    A, g, n = P.stencil("Laplace", 4), P.grid, 16
    assert A.is_axis and len(A.terms) == 12 and [g.ncells(4, d) for d in range(3)] == [n, n, n]
    lay = FieldLayout.node(3, (n, n, n), 0)
    x, y, z = [g.nodes(4, d)[GHOST:-GHOST] for d in range(3)]
    X, Y, Z = x[None, None, :], y[None, :, None], z[:, None, None]
    q = X * X + 2.0 * Y * Y + 3.0 * Z * Z + X * Y
    u, dst = ops.from_host(q.reshape(-1).copy()), ops.new_array(lay.size)
    b, e = [1, 1, 1], [n, n, n]
    ops.axis_op(APPLY, lay.c_struct(), u, None, None, lay.c_struct(), dst, A, 0.0, -1, b, e)
    got = ops.to_host(dst).reshape(n + 1, n + 1, n + 1)[1:n, 1:n, 1:n]
    coef = ops.axis_coefficients(A.c_struct(ops), b, e)
    mag = np.zeros_like(got)
    for k, o in enumerate(A.offsets):
        mag = mag + np.abs(coef[k] * q[1 + o[2]:n + o[2], 1 + o[1]:n + o[1], 1 + o[0]:n + o[0]])
    # A = -Laplace: -(2 + 4 + 6).  Every product c_e q_e carries the roundings of its coefficient (at most 8: 3 per term, 5 additions in
    # the centre), of the sample (at most 6) and its own; the fold adds 6: below 16 u of the sum of the magnitudes, and nothing else
    # remains, the three-point formula being exact for quadratics
    err = np.abs(got - (-12.0))
    print("largest error / bound", float((err / (16 * U * mag)).max()))
    assert np.all(err <= 16 * U * mag)


# -- 6: the example programs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [2, 3])
def test_example_programs_print_their_goldens_and_the_error_falls_with_the_level(nd):
    ops = Recording()
    P, out = G.run_own(nd, ops)
    assert out == G.own_results(nd)
    assert "stencil_op" not in ops.calls and "cg_coarse" not in ops.calls and "fill_expr" not in ops.calls and "apply_dirichlet" not in ops.calls
    assert ops.calls.count("axis_op") > 100 and "apply_dirichlet_expr_grid" in ops.calls and "max_err_expr_grid" in ops.calls
    P4, out4 = G.run_own(nd, GridOracleOps(), maxLevel=4)
    err4, err5 = P4.printed_values[-2], P.printed_values[-2]
    assert float(out4[-1]) <= 1e-6 and float(out[-1]) <= 1e-6          # both met the tolerance, an absolute one
    print("final maximum error at maxLevel 4:", err4, "at 5:", err5)
    assert err5 < err4


def test_example_cycle_replays_from_a_recording_with_equal_output():
    from graph_ops import DeferringOps

    ops = DeferringOps(GridOracleOps())
    P, out = G.run_own(2, ops, maxLevel=4, auto_graph=True)
    Q, want = G.run_own(2, GridOracleOps(), maxLevel=4)
    assert out == want and [float(v).hex() for v in P.printed_values] == [float(v).hex() for v in Q.printed_values]
    assert ops.replays > 0 and P.graph_replays > 0


# -- the restatement against an independent reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,colour,wform", [(0, -1, 0), (1, 0, 0), (2, -1, 0), (2, -1, 1), (2, 1, 1)])
def test_restatement_equals_the_oracle_on_a_stencil_field_with_the_same_coefficients(mode, colour, wform):
    """examg_axis_op is, from the coefficients on, examg_stencil_op on a stencil field in planes: the C oracle's loop over such a field,
    filled with the coefficients of the terms, gives the restatement's bits."""
    from exastencils_amd.field import Stencil
    from exastencils_amd.layout import FieldLayout

    n = (11, 7, 6)
    ops = GridOracleOps()
    st = G.separated(G.fv_text(3), 3, G.random_grid(3, n, 9)).with_wform(wform)
    lu, lf, ld = G.layouts(3, n)
    lc = FieldLayout.node(3, n, 0)
    coef = st.coefficients([0, 0, 0], [n[0] + 1, n[1] + 1, n[2] + 1])
    cf = ops.from_host(np.concatenate([c.reshape(-1) for c in coef]))
    field = Stencil(list(st.offsets), [], cf, lc, 0, wform)
    rng = np.random.default_rng(3)
    u, f = ops.from_host(rng.uniform(-1, 1, int(lu.size))), ops.from_host(rng.uniform(-1, 1, int(lf.size)))
    b, e = [1, 1, 1], list(n)
    outs = []
    for fn, A in ((ops.axis_op, st), (ops.stencil_op, field)):
        un, dst = u.clone(), ops.from_host(np.full(int(ld.size), -7.0e300))
        if mode == 2 and colour >= 0:
            fn(mode, lu.c_struct(), un, lf.c_struct(), f, lu.c_struct(), un, A, 0.8, colour, b, e)
            outs.append(un.numpy().copy())
        else:
            fn(mode, lu.c_struct(), un, lf.c_struct(), f, ld.c_struct(), dst, A, 0.8, colour, b, e)
            outs.append(dst.numpy().copy())
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64)) and np.count_nonzero(outs[0] != -7.0e300) > 0
