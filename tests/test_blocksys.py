"""Block systems of node fields without a GPU: the interpreter's stencil arithmetic (factor folding, merging of the terms on one
unknown, d indices), one launch per recognised loop and per colour, every refusal by its text, the two elasticity programs on the
numpy restatement (tests/blocksys_ops.py) against their goldens, and the decoupling claim: the restatement's vectorised colour sweeps
equal a plain sequential loop over the points in the reference's nest order."""
import os
import re

import numpy as np
import pytest

from blocksys_cases import SHAPES, BsysData, blocks, boxes, colouring, layouts
from blocksys_ops import SYS_RESIDUAL, BlockSysOracleOps, centre
from system_ops import solve2, solve3

from exastencils_amd import exa4
from exastencils_amd.domain import RectDomain
from exastencils_amd.exa4_parser import Exa4Unsupported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RecordingOps(BlockSysOracleOps):
    """The restatement, and a record of the block-system calls."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def bsys_op(self, mode, lu, u, lf, f, ld, dst, A, row_mask, begin, end):
        self.calls.append(("op", mode, row_mask, A, [x.data_ptr() for x in u], [None if x is None else x.data_ptr() for x in dst]))
        super().bsys_op(mode, lu, u, lf, f, ld, dst, A, row_mask, begin, end)

    def bsys_relax(self, lu, u, lf, f, A, relax, col, begin, end):
        self.calls.append(("relax", relax, col, A, [x.data_ptr() for x in u]))
        super().bsys_relax(lu, u, lf, f, A, relax, col, begin, end)


def _text(nd=2):
    with open(os.path.join(ROOT, "examples", "exa4", "elasticity%dd.exa4" % nd)) as f:
        return f.read()


def _program(text, nd=2, hi=3, ops=None, **kw):
    return exa4.Exa4Program(text, dict(dimensionality=nd, minLevel=1, maxLevel=hi), ops=ops or RecordingOps(), **kw)


def _entries(st):
    return list(zip(st.offsets, st.coefs))


# -- the host's stencil arithmetic -----------------------------------------------------------------------------------------------
def test_rows_are_merged_in_order_of_appearance_with_the_factor_folded_in():
    """Level 2 (h = 1/4): 1 / h^2 = 16, 1 / (4 h^2) = 4, lambda + mu = 325.  `( lambda + mu ) * dxx` and `lambda * Laplace` on u are
    ONE block: the entries of dxx in its order with the Laplacian's added where the offsets meet, the Laplacian's y neighbours
    appended.  Every product and sum below is exact in binary, so the expected coefficients are literals."""
    P = _program(_text())
    P.call("Defect", 2)
    (kind, mode, mask, A, u, dst), = P.ops.calls
    assert (kind, mode, mask) == ("op", SYS_RESIDUAL, 3)
    assert u == [P.fields[(n, 2)].data(0).data_ptr() for n in ("u", "v")] and dst == [P.fields[(n, 2)].data(0).data_ptr() for n in ("r_u", "r_v")]
    assert _entries(A[0][0]) == [((0, 0, 0), 325.0 * -32.0 + 195.0 * -64.0), ((-1, 0, 0), 8320.0), ((1, 0, 0), 8320.0), ((0, -1, 0), 3120.0),
                                 ((0, 1, 0), 3120.0)]
    assert _entries(A[0][1]) == [((-1, 1, 0), -1300.0), ((1, 1, 0), 1300.0), ((-1, -1, 0), 1300.0), ((1, -1, 0), -1300.0)]
    assert _entries(A[1][0]) == _entries(A[0][1])
    assert _entries(A[1][1]) == [((0, 0, 0), -22880.0), ((0, -1, 0), 8320.0), ((0, 1, 0), 8320.0), ((-1, 0, 0), 3120.0), ((1, 0, 0), 3120.0)]


def test_factors_fold_left_to_right_and_d_follows_first_appearance():
    """`lambda * ( dxy * v + 0.7 * 0.7 * ( dxx * u ) )`: the coefficients of dxx take ((lambda * 0.7) * 0.7) * c -- the outer factor first,
    then the inner ones as written -- and those of dxy lambda * c.  The first row of the loop names v before u: v is unknown 0 of BOTH rows."""
    t = _text().replace("    r_u = f_u - ( ( lambda + mu ) * ( dxx * u + dxy * v ) + lambda * ( Laplace * u ) )\n",
                        "    r_u = f_u - ( lambda * ( dxy * v + 0.7 * 0.7 * ( dxx * u ) ) )\n")
    assert t != _text()
    P = _program(t)
    P.call("Defect", 2)
    (_, _, mask, A, u, _), = P.ops.calls
    assert mask == 3 and u == [P.fields[(n, 2)].data(0).data_ptr() for n in ("v", "u")]
    s = (195.0 * 0.7) * 0.7
    assert s != 195.0 * (0.7 * 0.7)      # (the other association rounds differently: the order is observable)
    assert _entries(A[0][1]) == [((0, 0, 0), s * -32.0), ((-1, 0, 0), s * 16.0), ((1, 0, 0), s * 16.0)]
    assert [c for _, c in _entries(A[0][0])] == [195.0 * -4.0, 195.0 * 4.0, 195.0 * 4.0, 195.0 * -4.0]
    assert _entries(A[1][0])[0] == ((0, 0, 0), -22880.0) and len(A[1][1].offsets) == 4      # row v: dyy + Laplace on v (d = 0), dxy on u (d = 1)


def test_rows_apart_are_one_launch_each_with_a_one_row_mask():
    t = _text().replace("    r_v = f_v - (", "  }\n  loop over r_v {\n    r_v = f_v - (")
    P = _program(t)
    P.call("Defect", 2)
    assert [(c[0], c[2]) for c in P.ops.calls] == [("op", 1), ("op", 1)]
    assert [c[5] for c in P.ops.calls] == [[P.fields[(n, 2)].data(0).data_ptr(), None] for n in ("r_u", "r_v")]
    Q = _program(_text())
    Q.call("Defect", 2)
    for n in ("r_u", "r_v"):
        assert np.array_equal(P.fields[(n, 2)].data(0).numpy(), Q.fields[(n, 2)].data(0).numpy())


def test_launches_of_one_cycle():
    """Levels 1..3, statement by statement: a sweep is 4 colours of (1 relax + 2 `apply bc`), a level that is not the coarsest runs 6
    sweeps, the defect (1 op for both rows + 2 `apply bc`), 2 restrictions, 2 set + 2 `apply bc`, 2 corrections + 2 `apply bc`; the
    coarsest level 16 sweeps."""
    P = _program(_text(), fuse=False)
    l0 = P.launches
    P.call("VCycle", 3)
    ops = [c for c in P.ops.calls if c[0] == "op"]
    relax = [c for c in P.ops.calls if c[0] == "relax"]
    assert len(ops) == 2 and all(c[2] == 3 for c in ops)
    assert len(relax) == 4 * (6 + 6 + 16) and {c[1] for c in relax} == {0.8}
    assert [c[2].rem for c in relax[:4]] == [(0, 0), (1, 0), (0, 1), (1, 1)]      # the first expression varies fastest
    assert P.launches - l0 == 2 * (6 * 12 + 3 + 10) + 16 * 12


# -- the programs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [2, 3])
def test_elasticity_prints_its_golden_within_20_cycles(nd):
    name = os.path.join(ROOT, "examples", "exa4", "elasticity%dd" % nd)
    out = exa4.load(name + ".exa4", name + ".knowledge", ops=BlockSysOracleOps()).run()
    with open(os.path.join(ROOT, "tests", "golden", "own", "elasticity%dd.results" % nd)) as f:
        assert "\n".join(out) + "\n" == f.read()
    cycles = int(out[-1])
    assert cycles <= 20 and len(out) == cycles + 2
    assert float(out[-2]) <= 1e-10 * float(out[0]) * (1.0 + 1e-3)      # (four printed digits of both)


# -- refusals --------------------------------------------------------------------------------------------------------------------
ROW_U = "u => ( lambda + mu ) * ( dxx * u + dxy * v ) + lambda * ( Laplace * u ) == f_u"
ROW_V = "v => ( lambda + mu ) * ( dxy * u + dyy * v ) + lambda * ( Laplace * v ) == f_v"
SPLIT = "LayoutTransformations {\n  transform u@finest with [x, y] => [x / 2, y, x % 2]\n}\n\n"
REFUSALS = [
    ("red-black does not decouple dxy", lambda t: t.replace("    i0 % 2,\n    i1 % 2,\n", "    ( i0 + i1 ) % 2,\n"),
     "does not decouple the system: block (u, v) reads v at offset [-1, 1], a point of the row's own colour -- the generated loop would depend on its order"),
    ("repeat with colour conditions do not either", lambda t: t.replace("  color with {\n    i0 % 2,\n    i1 % 2,\n", "  repeat with {\n    ( 0 == ( ( i0 + i1 ) % 2 ) ),\n    ( 1 == ( ( i0 + i1 ) % 2 ) ),\n"),
     "does not decouple the system: block (u, v)"),
    ("jacobi", lambda t: t.replace("solve locally relax 0.8", "solve locally with jacobi relax 0.8"), "solve locally with jacobi"),
    ("uncoloured", lambda t: t.replace("  color with {\n    i0 % 2,\n    i1 % 2,\n", "  repeat 1 times {\n"), "solve locally in an uncoloured loop"),
    ("unknown with offset", lambda t: t.replace(ROW_U, "u@[1, 0] => " + ROW_U[5:]), "offset access"),
    ("four unknowns", lambda t: t.replace(ROW_U, ROW_U + "\n        r_u => dxx * r_u + dxy * u == f_u\n        r_v => dxx * r_v + dxy * u == f_u"), "more unknowns than 3 (4)"),
    ("unknown missing from the rows", lambda t: t.replace(ROW_U, ROW_U.replace("dxy * v", "dxy * u")).replace(ROW_V, ROW_V.replace("dyy * v", "dyy * u").replace("Laplace * v", "Laplace * u")),
     "unknown v is missing from the rows"),
    ("row over another field", lambda t: t.replace("u => ( lambda + mu ) * ( dxx * u + dxy * v )", "u => ( lambda + mu ) * ( dxx * u + dxy * r_v )"),
     "the unknowns must be exactly the fields of the rows (r_v is none)"),
    ("fields of different layouts", lambda t: t.replace("Field v< global, Halo, 0.0 >@(all but finest)", "Field v< global, Plain, 0.0 >@(all but finest)"),
     "solve locally: u and v have different layouts"),
    ("stencil field as a block", lambda t: t.replace("Stencil Fine from", "Layout Five< ColumnVector<Real, 5>, Node >@all {\n  ghostLayers = [0, 0]\n  duplicateLayers = [1, 1]\n}\n"
                                                     "Field five< global, Five, None >@all\nStencilField LapField< five => Laplace >@all\nStencil Fine from")
     .replace("lambda * ( Laplace * u ) == f_u", "lambda * ( LapField * u ) == f_u"), "a stencil field (LapField) as a block of a system"),
    ("reach 2", lambda t: t.replace("Stencil dyy@all {\n  [ 0,  0]", "Stencil dyy@all {\n  [ 0,  2] => 1.0\n  [ 0,  0]"), "stencil dyy reaches further than one point (reach 2)"),
    ("where on the loop", lambda t: t.replace("    loop over u {\n      solve", "    loop over u where ( i0 > 0 ) {\n      solve"), "`only`, `where` or under contraction"),
    ("row in a coloured loop outside solve locally", lambda t: t.replace("    loop over u {\n      solve locally relax 0.8 {\n        " + ROW_U, "    loop over r_u {\n      r_u = f_u - ( dxx * u + dxy * v )\n    }\n    loop over u {\n      solve locally relax 0.8 {\n        " + ROW_U),
     "system row in a coloured loop outside solve locally"),
    ("row in a red-black loop", lambda t: t.replace("  loop over r_u {\n    r_u = f_u", "  loop over r_u where ( 0 == ( ( i0 + i1 ) % 2 ) ) {\n    r_u = f_u"),
     "system row in a coloured loop outside solve locally"),
    ("row in a loop with where", lambda t: t.replace("  loop over r_u {\n    r_u = f_u", "  loop over r_u where ( i0 > 0 ) {\n    r_u = f_u"),
     "system row in a loop with `only`, `where` or under contraction"),
    ("row under contraction", lambda t: t.replace("  loop over r_u {\n    r_u = f_u", "  repeat 1 times with contraction [1, 1] {\n  loop over r_u {\n    r_u = f_u")
     .replace("  apply bc to r_u\n  apply bc to r_v\n}", "  }\n  apply bc to r_u\n  apply bc to r_v\n}"), "under contraction"),
]


@pytest.mark.parametrize("what,change,text", REFUSALS, ids=[r[0].replace(" ", "-") for r in REFUSALS])
def test_refusals_by_name(what, change, text):
    t = change(_text())
    assert t != _text(), "the substitution found nothing to change"
    with pytest.raises(Exa4Unsupported, match=re.escape(text)):
        _program(t, ops=BlockSysOracleOps()).run()


@pytest.mark.parametrize("what,kw,text", [
    ("two blocks", dict(domain=RectDomain(2, (2, 1, 1), 0, (1, 2, 1))), "on more than one block or with a periodic axis"),
    ("a periodic axis", dict(domain=RectDomain(2, (1, 1, 1), 0, (2, 2, 1), periodic=(True, False, False))), "on more than one block or with a periodic axis"),
], ids=["two-blocks", "periodic-axis"])
def test_refusals_of_the_decomposition(what, kw, text):
    class NoComm:      # (the refusal comes before anything is exchanged)
        def exchange(self, *a, **k):
            pass

    with pytest.raises(Exa4Unsupported, match=re.escape(text)):
        _program(_text(), ops=BlockSysOracleOps(), comm=NoComm(), **kw).call("Defect", 2)


def test_colour_split_fields_are_refused():
    """(The CPU stand-in only records layout transformations; one that claims to have transformed layouts makes the interpreter apply them.)"""
    class SplitOps(BlockSysOracleOps):
        transform_field = None

    P = _program(SPLIT + _text(), ops=SplitOps())
    assert P.fields[("u", 3)].layout.transform == 1
    with pytest.raises(Exa4Unsupported, match="solve locally over colour-split field u"):
        P.call("Sweep", 3)
    with pytest.raises(Exa4Unsupported, match="system row over colour-split field u"):
        P.call("Defect", 3)


def test_stencils_over_grid_tables_and_complex_entries_are_no_blocks():
    """On a non-uniform grid the stencils over vf_gridWidth_* become per-axis tables; an entry over a complex global makes a complex stencil."""
    k = dict(dimensionality=2, minLevel=1, maxLevel=3, grid_isUniform=False, grid_isAxisAligned=True, grid_spacingModel="linearFct")
    from grid_ops import GridOracleOps

    with pytest.raises(Exa4Unsupported, match="as a block of a system"):
        exa4.Exa4Program(_text().replace("vf_gridWidth_x", "vf_cellWidth_x").replace("vf_gridWidth_y", "vf_cellWidth_y"), k, ops=GridOracleOps()).call("Defect", 2)
    t = _text().replace("  Val mu : Real = 130.0\n", "  Val mu : Real = 130.0\n  Val shift : Complex<Real> = (1.0+0.5j)\n").replace(
        "Stencil dyy@all {\n  [ 0,  0] => -2.0 /", "Stencil dyy@all {\n  [ 0,  0] => shift - 2.0 /")
    with pytest.raises(Exa4Unsupported, match=re.escape("a stencil with complex entries (dyy) as a block of a system")):
        _program(t, ops=BlockSysOracleOps()).call("Defect", 2)


def test_a_point_wise_coefficient_stencil_on_node_fields_keeps_its_refusal():
    t = _text().replace("Stencil Fine from", "Stencil Cu@all {\n  [0, 0] => f_u\n}\nStencil Fine from").replace(
        "u => ( lambda + mu ) * ( dxx * u + dxy * v ) + lambda * ( Laplace * u ) == f_u", "u => ( Cu * u + Cu * v + Laplace * u ) == f_u").replace(
        "v => ( lambda + mu ) * ( dxy * u + dyy * v ) + lambda * ( Laplace * v ) == f_v", "v => ( Cu * u + Cu * v + Laplace * v ) == f_v").replace(
        "    i0 % 2,\n    i1 % 2,\n", "    ( i0 + i1 ) % 2,\n")
    with pytest.raises(Exa4Unsupported, match="solve locally on node field u"):
        _program(t, ops=BlockSysOracleOps()).run()


# -- the decoupling claim --------------------------------------------------------------------------------------------------------
def _sequential_sweep(lu, lo, u, f, A, relax, col, b, e):
    """All colours in the reference's order, each a plain nest over the box (z outermost, x innermost), in place, one Python float
    operation at a time in the header's order."""
    n = len(u)
    U = [x.numpy() for x in u]
    F = [x.numpy() for x in f]
    for c in col.colours():
        for i2 in range(b[2], e[2]):
            for i1 in range(b[1], e[1]):
                for i0 in range(b[0], e[0]):
                    if any((shift + sum((i0, i1, i2)[d] for d in axes)) % mod != rem for (axes, shift, mod), rem in zip(c.exprs, c.rem)):
                        continue
                    rhs = []
                    for r in range(n):
                        row = None
                        for d in range(n):
                            s = None
                            for o, co in (zip(A[r][d].offsets, A[r][d].coefs) if A[r][d] is not None else ()):
                                if not any(o):
                                    continue
                                t = float(co) * float(U[d][lu.linear(i0 + o[0], i1 + o[1], i2 + o[2])])
                                s = t if s is None else s + t
                            if s is not None:
                                row = s if row is None else row + s
                        fv = float(F[r][lo.linear(i0, i1, i2)])
                        rhs.append(fv if row is None else fv - row)
                    m = [[centre(A[r][d]) for d in range(n)] for r in range(n)]
                    xs = solve2(m, rhs) if n == 2 else solve3(m, rhs)
                    for r in range(n):
                        k = lu.linear(i0, i1, i2)
                        U[r][k] = xs[r] if relax == 1.0 else float(U[r][k]) + relax * (xs[r] - float(U[r][k]))


@pytest.mark.parametrize("pattern", ["elasticity", "dense", "sparse"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=["5x3", "5x4x3"])
@pytest.mark.parametrize("relax", [1.0, 0.7])
def test_colour_sweeps_equal_the_sequential_loop(shape, pattern, relax):
    nd, n, inner = shape
    ops = BlockSysOracleOps()
    lu, lo = layouts(nd, inner, 0)
    A = blocks(pattern, nd, n)
    col = colouring(nd, "axes")
    b, e = boxes(nd, inner)["inner"]
    vec, seq = BsysData(ops, n, lu, lo), BsysData(ops, n, lu, lo)
    before = [x.numpy().copy() for x in vec.u]
    for c in col.colours():
        ops.bsys_relax(lu.c_struct(), vec.u, lo.c_struct(), vec.f, A, relax, c, b, e)
    _sequential_sweep(lu, lo, seq.u, seq.f, A, relax, col, b, e)
    for k, (x, y) in enumerate(zip(vec.arrays(), seq.arrays())):
        assert np.array_equal(x.numpy(), y.numpy()), "array %d" % k
    assert not any(np.array_equal(x.numpy(), y) for x, y in zip(vec.u, before))
