"""GPU parity of the block-system entry points (include/examg.h: examg_bsys_op, examg_bsys_relax, examg_bsys_route) against their
numpy restatement (tests/blocksys_ops.py): point-wise kernels, bit-identical over the WHOLE of every array -- a stray write outside
the box, to a row outside the mask, to another colour or to an input shows.  Then the two elasticity programs on HipOps."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from blocksys_cases import PATTERNS, SHAPES, BsysData, blocks, boxes, colouring, layouts
from blocksys_ops import SYS_APPLY, SYS_RESIDUAL, BlockSysOracleOps

from exastencils_amd import exa4, lib
from exastencils_amd.field import Colouring, Stencil
from exastencils_amd.layout import FieldLayout
from exastencils_amd.lib import ExamgError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    from exastencils_amd.ops import HipOps

    return HipOps(0)


@pytest.fixture(scope="module")
def orc():
    return BlockSysOracleOps()


def same(a, b, what):
    if not np.array_equal(a, b):
        d = np.abs(a - b)
        raise AssertionError("%s: %d of %d values differ, max abs %.3e" % (what, int((d > 0).sum()), d.size, d.max()))


def compare(hip, orc, fn, what):
    """fn(ops) -> list of BsysData, one per call sequence; every array of every system is compared whole."""
    g = fn(hip)
    hip.synchronize()
    c = fn(orc)
    assert len(g) == len(c) and g
    for k, (sg, sc) in enumerate(zip(g, c)):
        for j, (x, y) in enumerate(zip(sg.arrays(), sc.arrays())):
            same(hip.to_host(x), orc.to_host(y), "%s, sequence %d, array %d" % (what, k, j))


CASES = [(nd, n, inner, ghost) for nd, n, inner in SHAPES for ghost in (1, 0)]
IDS = ["%dd-n%d-%s-g%d" % (nd, n, "x".join(map(str, inner)), ghost) for nd, n, inner, ghost in CASES]


def op_all(ops, nd, n, inner, ghost, pattern, routes=None):
    """Every single row and all rows, APPLY and RESIDUAL, on all three boxes, each call on fresh data."""
    lu, lo = layouts(nd, inner, ghost)
    A = blocks(pattern, nd, n)
    out = []
    for b, e in boxes(nd, inner).values():
        for mode in (SYS_APPLY, SYS_RESIDUAL):
            for mask in [1 << c for c in range(n)] + [(1 << n) - 1]:
                s = BsysData(ops, n, lu, lo)
                if routes is not None:
                    routes.append((mask, ops.bsys_route(mode, lu.c_struct(), s.u, lo.c_struct(), s.f, lo.c_struct(), s.dst, A, mask, b, e)))
                ops.bsys_op(mode, lu.c_struct(), s.u, lo.c_struct(), s.f, lo.c_struct(), s.dst, A, mask, b, e)
                out.append(s)
    return out


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nd,n,inner,ghost", CASES, ids=IDS)
def test_bsys_op_bitwise(hip, orc, nd, n, inner, ghost, pattern):
    routes = []
    compare(hip, orc, lambda ops: op_all(ops, nd, n, inner, ghost, pattern, routes if ops is hip else None), "bsys_op %s" % pattern)
    assert routes and all(r == lib.BSYS_GATHER for _, r in routes)      # the one route there is: it ran, and the answers above are its bits


def relax_all(ops, nd, n, inner, ghost, pattern, kind):
    """Single colours and the full sweep in the reference's order, relax 1.0 and 0.7, on all three boxes."""
    lu, lo = layouts(nd, inner, ghost)
    A = blocks(pattern, nd, n)
    cols = list(colouring(nd, kind).colours())
    out = []
    for b, e in boxes(nd, inner).values():
        for relax in (1.0, 0.7):
            for seq in [(c,) for c in cols] + [tuple(cols)]:
                s = BsysData(ops, n, lu, lo)
                for col in seq:
                    ops.bsys_relax(lu.c_struct(), s.u, lo.c_struct(), s.f, A, relax, col, b, e)
                out.append(s)
    return out


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nd,n,inner,ghost", CASES, ids=IDS)
def test_bsys_relax_bitwise_under_the_axis_parities(hip, orc, nd, n, inner, ghost, pattern):
    """The 4-colouring `i0 % 2, i1 % 2` in 2-D, the 8-colouring in 3-D: they decouple every block of reach 1."""
    compare(hip, orc, lambda ops: relax_all(ops, nd, n, inner, ghost, pattern, "axes"), "bsys_relax %s" % pattern)


@pytest.mark.parametrize("nd,n,inner,ghost", CASES, ids=IDS)
def test_bsys_relax_bitwise_under_the_parity_of_all_indices(hip, orc, nd, n, inner, ghost):
    """A system whose blocks are all stars, which red-black decouples."""
    compare(hip, orc, lambda ops: relax_all(ops, nd, n, inner, ghost, "stars", "all"), "bsys_relax stars")


def test_a_shifted_colouring_with_mod_3(hip, orc):
    """`(1 + i0) % 3, i1 % 2`: a lattice with a stride other than 2 and a shift; it decouples stars and the xy diagonals."""
    nd, n, inner = SHAPES[1]
    col = Colouring((((0,), 1, 3), ((1,), 0, 2)))
    lu, lo = layouts(nd, inner, 0)
    A = blocks("asymmetric", nd, n)
    b, e = boxes(nd, inner)["interior"]

    def run(ops):
        s = BsysData(ops, n, lu, lo)
        for c in col.colours():
            ops.bsys_relax(lu.c_struct(), s.u, lo.c_struct(), s.f, A, 0.7, c, b, e)
        return [s]

    compare(hip, orc, run, "mod-3 colouring")


def test_empty_box_is_a_no_op_and_routes_to_nothing(hip, orc):
    nd, n, inner = SHAPES[0]
    lu, lo = layouts(nd, inner, 1)
    A = blocks("elasticity", nd, n)

    def run(ops):
        s = BsysData(ops, n, lu, lo)
        assert ops.bsys_route(SYS_RESIDUAL, lu.c_struct(), s.u, lo.c_struct(), s.f, lo.c_struct(), s.dst, A, 3, [3, 2, 0], [3, 4, 1]) == 0
        ops.bsys_op(SYS_RESIDUAL, lu.c_struct(), s.u, lo.c_struct(), s.f, lo.c_struct(), s.dst, A, 3, [3, 2, 0], [3, 4, 1])
        ops.bsys_relax(lu.c_struct(), s.u, lo.c_struct(), s.f, A, 1.0, next(colouring(nd, "axes").colours()), [1, 3, 0], [6, 3, 1])
        return [s]

    compare(hip, orc, run, "empty box")


# -- refusals ----------------------------------------------------------------------------------------------------------------------
def _refusals():
    nd, inner = 2, (8, 6)
    lu, lo = layouts(nd, inner, 0)
    A = blocks("elasticity", nd, 2)
    axes = next(colouring(nd, "axes").colours())
    good = dict(n=2, lu=lu, lf=lo, ld=lo, A=A, col=axes, b=[1, 1, 0], e=[9, 7, 1], alias=False)
    split = lo.c_struct()
    split.transform = 1          # EXAMG_LAYOUT_SPLIT_X
    one_d = FieldLayout.node(1, (9,), 1).c_struct()
    field_block = Stencil([(0, 0, 0)], [1.0], cfield="self", clayout=lo)

    def table(c, d, st):
        T = [list(r) for r in A]
        T[c][d] = st
        return T

    neg = Colouring((((0,), -5, 2), ((1,), 0, 2)), (0, 0))
    bad_mod = axes.c_struct()
    bad_mod.mod[1] = 0
    bad_rem = axes.c_struct()
    bad_rem.rem[0] = 2
    bad_nexpr = axes.c_struct()
    bad_nexpr.nexpr = 4
    return [
        ("n = 1", dict(good, n=1), "2 or 3", "both"),
        ("n = 4", dict(good, n=4), "2 or 3", "both"),
        ("cell layout", dict(good, lf=FieldLayout.cell(nd, (10, 8), 0)), "is a cell layout", "both"),
        ("colour-split layout", dict(good, lf=split), "colour-split", "both"),
        ("1-D layout", dict(good, lu=one_d), "2-D or 3-D", "both"),
        ("rhs layout of another size", dict(good, lf=FieldLayout.node(nd, (11, 7), 1)), "rhs layout has", "both"),
        ("dst layout of another dimensionality", dict(good, ld=FieldLayout.node(3, (9, 7, 3), 1)), "dst layout has 3 dimensions", "op"),
        ("stencil field as a block", dict(good, A=table(0, 1, field_block)), "is a stencil field", "both"),
        ("reach 2", dict(good, A=table(1, 0, Stencil([(0, 0, 0), (2, 0, 0)], [1.0, 1.0]))), "reaches further than one point", "both"),
        ("an entry off the layout's axes", dict(good, A=table(1, 0, Stencil([(0, 0, 1)], [1.0]))), "reaches further than one point", "both"),
        ("repeated offset", dict(good, A=table(0, 0, Stencil([(0, 0, 0), (1, 0, 0), (1, 0, 0)], [4.0, 1.0, 1.0]))), "repeats the offset", "both"),
        ("row without blocks", dict(good, A=[A[0], [None, None]]), "row 1 has no block", "both"),
        ("zero a_cc", dict(good, A=table(1, 1, Stencil([(1, 0, 0), (-1, 0, 0)], [1.0, 1.0]))), "a_11.*is zero", "relax"),
        ("dst is an unknown", dict(good, lf=lu, ld=lu, alias=True), "destination 0 is unknown 1", "op"),
        ("dst is a right-hand side", dict(good, alias="f"), "destination 0 is right-hand side 1", "op"),
        ("shell leaves the unknowns", dict(good, lu=lo, b=[0, 1, 0]), "box \\+ one point leaves the allocation of the unknowns", "both"),
        ("box leaves the rhs", dict(good, lu=FieldLayout.node(nd, [i + 1 for i in inner], 2), b=[-1, 1, 0]), "box leaves the rhs allocation", "both"),
        ("parity of all indices does not decouple dxy", dict(good, col=next(colouring(nd, "all").colours())), "does not decouple block \\(0, 1\\)", "relax"),
        ("negative colour expression", dict(good, col=neg), "can be negative", "relax"),
        ("mod 0", dict(good, col=bad_mod), "mod must be positive", "relax"),
        ("rem outside [0, mod)", dict(good, col=bad_rem), "rem must lie", "relax"),
        ("nexpr 4", dict(good, col=bad_nexpr), "nexpr must be", "relax"),
    ]


class _RawColouring:
    """A colouring struct the value type would not build."""

    def __init__(self, c):
        self.c = c

    def c_struct(self):
        return self.c


REFUSALS = [(name, args, text, entry) for name, args, text, which in _refusals() for entry in ("op", "relax") if which in ("both", entry)]


@pytest.mark.parametrize("name,args,text,entry", REFUSALS, ids=["%s-%s" % (r[3], r[0].replace(" ", "-")) for r in REFUSALS])
def test_refusals_launch_nothing(hip, name, args, text, entry):
    """Each refusal returns its error through examg_last_error and leaves every array as it was; examg_bsys_route answers -1."""
    n, big = args["n"], FieldLayout.node(3, (12, 9, 4), 1)
    t = [hip.new_array(big.size) for _ in range(4 * 3)]      # every array large enough for any of the layouts
    for k, a in enumerate(t):
        hip.fill_random(a, 70 + k)
    before = [hip.to_host(a).copy() for a in t]
    u, f, dst = t[0:n], t[4:4 + n], t[8:8 + n]
    if args["alias"]:
        dst = [f[1] if args["alias"] == "f" else u[1]] + dst[1:]
    A = [[(Stencil(s.offsets, s.coefs, cfield=t[0], clayout=s.clayout) if s is not None and s.cfield == "self" else s) for s in row] for row in args["A"]]
    A = [row + [None] * (n - len(row)) for row in A] + [[None] * n] * (n - len(A))
    cs = lambda l: l if not hasattr(l, "c_struct") else l.c_struct()
    col = args["col"] if hasattr(args["col"], "exprs") else _RawColouring(args["col"])
    with pytest.raises(ExamgError, match=text):
        if entry == "op":
            assert hip.bsys_route(SYS_RESIDUAL, cs(args["lu"]), u, cs(args["lf"]), f, cs(args["ld"]), dst, A, 3, args["b"], args["e"]) == -1
            hip.bsys_op(SYS_RESIDUAL, cs(args["lu"]), u, cs(args["lf"]), f, cs(args["ld"]), dst, A, 3, args["b"], args["e"])
        else:
            hip.bsys_relax(cs(args["lu"]), u, cs(args["lf"]), f, A, 0.7, col, args["b"], args["e"])
    hip.synchronize()
    for k, a in enumerate(t):
        same(hip.to_host(a), before[k], "array %d after the refused call" % k)


# -- the interpreted example programs on the HIP kernels --------------------------------------------------------------------------
def _program(nd, ops, **kw):
    name = os.path.join(ROOT, "examples", "exa4", "elasticity%dd" % nd)
    return exa4.load(name + ".exa4", name + ".knowledge", ops=ops, **kw)


@pytest.mark.parametrize("nd", [2, 3])
def test_elasticity_on_the_gpu_prints_the_golden_within_20_cycles(hip, nd):
    """Levels 1..6 (65^2 nodes) and 1..5 (33^3 nodes): the lines of the numpy-layer run, four digits each; the second call of the
    cycle is recorded and every later one replays from the graph."""
    with open(os.path.join(ROOT, "tests", "golden", "own", "elasticity%dd.results" % nd)) as f:
        golden = f.read()
    P = _program(nd, hip)
    got = P.run()
    assert "\n".join(got) + "\n" == golden
    assert int(got[-1]) <= 20 and len(got) == int(got[-1]) + 2
    assert P.auto_graph and P.graph_replays > 0 and isinstance(P._auto_graphs.get(("VCycle", P.max_level)), dict)


@pytest.mark.parametrize("nd", [2, 3])
def test_fields_after_one_cycle_equal_the_numpy_layer(hip, orc, nd):
    """Every kernel of the cycle is point-wise (no reduction): after the defect and one V-cycle, every field of every level has the bits
    of the numpy restatement.  Both programs start from the SAME boundary values, the restatement's: the boundary expression calls sin,
    which the C library and the device library need not round alike (the difference is printed and bounded: a few ulps, on the faces
    where the expression is not zero), and `apply bc` writes them only once
    (the planes stay valid through the cycle)."""
    names = ("u", "v", "w")[:nd]

    def start(ops):
        P = _program(nd, ops)
        for F in names:
            P._apply_bc(P.fields[(F, P.max_level)], 0)
        return P

    def cycle(P):
        l0 = P.launches
        P.call("Defect", P.max_level)
        P.call("VCycle", P.max_level)
        P.call("Defect", P.max_level)
        return P.launches - l0

    G, C = start(hip), start(orc)
    for F in names:
        g, c = G.fields[(F, G.max_level)], C.fields[(F, C.max_level)]
        x, y = g.host_array(hip), c.host_array(orc)
        differ = x != y
        print("boundary values of %s: %d differ between the layers" % (F, int(differ.sum())))
        # sin of the two libraries, each within an ulp of the true value, then three exact-to-half-an-ulp products: a handful of ulps
        # at the most, and only where the boundary expression is not zero (one face of 65 points in 2-D, three faces of 33^2 in 3-D)
        assert np.all(np.abs(x - y)[differ] <= 8 * np.spacing(np.abs(y[differ]))) and int(differ.sum()) <= (65 if nd == 2 else 3 * 33 ** 2)
        g.set_host_array(hip, c.host_array(orc))
    assert cycle(G) == cycle(C)
    hip.synchronize()
    for key, f in C.fields.items():
        same(hip.to_host(G.fields[key].data(0)), orc.to_host(f.data(0)), "field %s@%d" % key)
