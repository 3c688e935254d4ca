"""The 5-point benchmark on the CPU: the ghost-loop rule `F = E - F@[-d]` (the EXAMG_BC_VALUE_MINUS kind of examg_apply_bc_cell), the node
position in its value, the faces of a boundary function merged into ONE examg_apply_bc_cell_faces call, every refusal by its words --
in the interpreter on the numpy kernel layer (tests/star2d_ops.py).  The reference's benchmark program runs as it is where the
reference checkout is present, against a plain loop nest written here from its statements; examples/exa4/jacobi2d_cell.exa4 prints
its golden."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from star2d_ops import BC_DIRICHLET, BC_NEGATE, BC_NEUMANN, BC_VALUE_MINUS, Star2dOracleOps  # noqa: E402

from exastencils_amd import exa4, knowledge  # noqa: E402
from exastencils_amd.exa4_parser import Exa4Unsupported  # noqa: E402
from exastencils_amd.layout import FieldLayout  # noqa: E402
from exastencils_amd.lib import ExprC, GeomC  # noqa: E402

EX = os.path.join(ROOT, "examples", "exa4")
REF = "/root/reference/Benchmark/FivePointStencil"


class Counting(Star2dOracleOps):
    """Counts the kernel-layer calls by name."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def apply_bc_cell(self, *a):
        self.calls.append("apply_bc_cell")
        return super().apply_bc_cell(*a)

    def apply_bc_cell_faces(self, l, x, geom, faces, mask):
        self.calls.append(("apply_bc_cell_faces", mask))
        return super().apply_bc_cell_faces(l, x, geom, faces, mask)

    def stencil_op(self, *a):
        self.calls.append("stencil_op")
        return super().stencil_op(*a)


# -- the reference's program as it is ---------------------------------------------------------------------------------------------------
def _benchmark_by_hand(n0, n1, iters):
    """Benchmark/FivePointStencil/5pt_Jac_Cell.exa4 statement by statement on (n1 + 2) x (n0 + 2) arrays [y][x] with one ghost layer: the
    rows in an explicit loop, every operation one IEEE operation on a row.  Returns Solution (active slot) and Residual."""
    hx, hy = (2.0 - 0.0) / n0, (1.0 - 0.0) / n1
    pi = math.pi
    c0 = (2.0 / (hx * hx)) + (2.0 / (hy * hy))
    cxp = cxm = -1.0 / (hx * hx)
    cyp = cym = -1.0 / (hy * hy)
    w = (1.0 / c0) * 0.8
    i = np.arange(n0)
    xc = (i * hx + 0.0) + 0.5 * hx
    xn = i * hx + 0.0
    rhs = np.zeros((n1, n0))
    for j in range(n1):
        yc = (j * hy + 0.0) + 0.5 * hy
        rhs[j] = ((4. * pi * pi) * np.sin((2. * pi) * xc)) * np.sinh(np.full(n0, (2. * pi) * yc))
    top = np.sin((2. * pi) * xn) * math.sinh(2. * pi)
    sol = [np.zeros((n1 + 2, n0 + 2)), np.zeros((n1 + 2, n0 + 2))]
    res = np.zeros((n1 + 2, n0 + 2))
    act = 0

    def apply_bc(u):
        for j in range(1, n1 + 1):
            u[j, 0] = 0. - u[j, 1]              # ghost [-1, 0] = 0. - interior@[1, 0]
            u[j, n0 + 1] = 0. - u[j, n0]        # ghost [ 1, 0]
        u[0, 1:n0 + 1] = 0. - u[1, 1:n0 + 1]    # ghost [0, -1]
        u[n1 + 1, 1:n0 + 1] = top - u[n1, 1:n0 + 1]      # ghost [0, 1]: the value at the ghost cell's own node position

    def conv(u, j):
        a = c0 * u[j, 1:n0 + 1]
        a = a + cxp * u[j, 2:n0 + 2]
        a = a + cxm * u[j, 0:n0]
        a = a + cyp * u[j + 1, 1:n0 + 1]
        a = a + cym * u[j - 1, 1:n0 + 1]
        return a

    def up_residual():
        u = sol[act]
        apply_bc(u)
        for j in range(1, n1 + 1):
            res[j, 1:n0 + 1] = rhs[j - 1] - conv(u, j)

    apply_bc(sol[act])
    up_residual()
    for _ in range(iters):
        u, un = sol[act], sol[1 - act]
        apply_bc(u)
        for j in range(1, n1 + 1):
            un[j, 1:n0 + 1] = u[j, 1:n0 + 1] + w * (rhs[j - 1] - conv(u, j))
        act = 1 - act
        up_residual()
    return sol[act], res


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference checkout is not on this machine")
def test_reference_benchmark_program_runs_as_it_is(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)      # printJSON writes results.json
    k = knowledge.parse_file(os.path.join(REF, "5pt_Jac_Cell.knowledge"))
    k["minLevel"] = k["maxLevel"] = 5
    ops = Counting()
    with open(os.path.join(REF, "5pt_Jac_Cell.exa4")) as f:
        P = exa4.Exa4Program(f.read(), k, ops=ops)
    P.json_dir = str(tmp_path)
    out = P.run()
    timers = [line for line in out if "Timer" in line]
    assert len(timers) == 5 and all(any(name in line for line in timers) for name in ("applyBC", "setup", "communication", "kernel", "solve"))
    # one apply bc at set-up, one per residual (101) and one per smoother step (100): each exactly one call, of all four faces
    bc = [c for c in ops.calls if c != "stencil_op"]
    assert bc == [("apply_bc_cell_faces", 15)] * 202, bc[:6]
    assert ops.calls.count("stencil_op") == 201
    S, R = P.fields[("Solution", 5)], P.fields[("Residual", 5)]
    assert S.layout.inner[:2] == (64, 64)      # 2 x 2 fragments of 32 x 32 cells, merged into one block
    want_s, want_r = _benchmark_by_hand(64, 64, 100)
    got_s = np.asarray(ops.to_host(S.data(S.active))).reshape(66, 66)
    got_r = np.asarray(ops.to_host(R.data(0))).reshape(66, 66)
    # edge and corner ghosts are never written, by either side
    assert np.array_equal(got_s, want_s)
    assert np.array_equal(got_r[1:65, 1:65], want_r[1:65, 1:65])


# -- the own program ------------------------------------------------------------------------------------------------------------------------
def test_own_program_prints_its_golden():
    from oracle import mg

    ops = Counting()
    P = exa4.load(os.path.join(EX, "jacobi2d_cell.exa4"), os.path.join(EX, "jacobi2d_cell.knowledge"), ops=ops)
    out = P.run()
    with open(os.path.join(ROOT, "tests", "golden", "own", "jacobi2d_cell.results")) as f:
        assert mg.compare_with_golden(out, f.read()) == []
    assert out[-1] == "100" and len(out) == 12
    assert [c for c in ops.calls if c != "stencil_op"] == [("apply_bc_cell_faces", 15)] * 201
    Q = exa4.load(os.path.join(EX, "jacobi2d_cell.exa4"), os.path.join(EX, "jacobi2d_cell.knowledge"), ops=Counting(), fuse=False)
    assert Q.run() == out and Q.ops.calls.count("apply_bc_cell") == 4 * 201      # the separate launches: the same values


# -- the kind against hand-computed ghosts ------------------------------------------------------------------------------------------------
def _geom(h=(0.5, 0.25, 1.0), pb=(-1.0, 2.0, 0.0)):
    g = GeomC()
    for d in range(3):
        g.pos_begin[d], g.h[d] = pb[d], h[d]
    return g


def _field43(ops, vals=None):
    """A 4 x 3 cell layout with one ghost layer: (5, 6) rows [y][x]; interior values 1 .. 12 (or `vals`), 99 everywhere else."""
    l = FieldLayout.cell(2, (4, 3), 1)
    a = np.full((5, 6), 99.0)
    a[1:4, 1:5] = np.arange(1.0, 13.0).reshape(3, 4) if vals is None else vals
    return l, ops.from_host(a.reshape(-1).copy()), a


def test_value_minus_interior_against_hand_computed_ghosts():
    ops = Star2dOracleOps()
    g = _geom()
    # a constant: ghost = 7.5 - interior on all four faces
    l, x, a = _field43(ops)
    ops.apply_bc_cell(l.c_struct(), x, g, BC_VALUE_MINUS, ExprC.from_program([("const", 7.5)]), 15)
    got = np.asarray(ops.to_host(x)).reshape(5, 6)
    want = a.copy()
    want[1:4, 0] = 7.5 - a[1:4, 1]
    want[1:4, 5] = 7.5 - a[1:4, 4]
    want[0, 1:5] = 7.5 - a[1, 1:5]
    want[4, 1:5] = 7.5 - a[3, 1:5]
    assert np.array_equal(got, want)      # the interior, the edge and the corner ghosts (99) untouched
    # x_node + 10 * y_centre AT THE GHOST CELL: node i * 0.5 - 1.0, centre (j * 0.25 + 2.0) + 0.125
    prog = ExprC.from_program([("nx", None), ("const", 10.0), ("y", None), ("*", None), ("+", None)])
    l, x, a = _field43(ops)
    ops.apply_bc_cell(l.c_struct(), x, g, BC_VALUE_MINUS, prog, 15)
    got = np.asarray(ops.to_host(x)).reshape(5, 6)
    want = a.copy()
    xn = lambda i: i * 0.5 - 1.0
    yc = lambda j: (j * 0.25 + 2.0) + 0.125
    for j in range(3):
        want[1 + j, 0] = (xn(-1) + 10.0 * yc(j)) - a[1 + j, 1]
        want[1 + j, 5] = (xn(4) + 10.0 * yc(j)) - a[1 + j, 4]
    for i in range(4):
        want[0, 1 + i] = (xn(i) + 10.0 * yc(-1)) - a[1, 1 + i]
        want[4, 1 + i] = (xn(i) + 10.0 * yc(3)) - a[3, 1 + i]
    assert np.array_equal(got, want)
    assert want[0, 1] == (-1.0 + 10.0 * 1.875) - 1.0 and want[2, 5] == (1.0 + 10.0 * 2.375) - 8.0      # two of them by hand


def test_value_minus_keeps_the_sign_of_zero_where_negate_flips_it():
    ops = Star2dOracleOps()
    zero = ExprC.from_program([("const", 0.0)])
    l, x, _ = _field43(ops, np.zeros((3, 4)))
    ops.apply_bc_cell(l.c_struct(), x, _geom(), BC_VALUE_MINUS, zero, 15)
    got = np.asarray(ops.to_host(x)).reshape(5, 6)
    assert got[2, 0] == 0.0 and not np.signbit(got[2, 0]) and not np.signbit(got[0, 1:5]).any()      # 0.0 - (+0.0) = +0.0
    l, y, _ = _field43(ops, np.zeros((3, 4)))
    ops.apply_bc_cell(l.c_struct(), y, _geom(), BC_NEGATE, None, 15)
    neg = np.asarray(ops.to_host(y)).reshape(5, 6)
    assert neg[2, 0] == 0.0 and np.signbit(neg[2, 0]) and np.signbit(neg[0, 1:5]).all()                # -(+0.0) = -0.0


def test_faces_call_equals_the_single_face_calls_in_both_orders():
    ops = Star2dOracleOps()
    g = _geom()
    poly = ExprC.from_program([("x", None), ("ny", None), ("*", None), ("const", 0.5), ("-", None)])
    dpoly = ExprC.from_program([("x", None), ("const", 3.0), ("y", None), ("*", None), ("+", None)])
    faces = [(BC_VALUE_MINUS, poly), (BC_NEGATE, None), (BC_DIRICHLET, dpoly), (BC_NEUMANN, None)]
    l, x, _ = _field43(ops)
    ops.apply_bc_cell_faces(l.c_struct(), x, g, faces, 15)
    one = np.asarray(ops.to_host(x)).copy()
    for order in ((0, 1, 2, 3), (3, 2, 1, 0)):
        l, y, _ = _field43(ops)
        for f in order:
            ops.apply_bc_cell(l.c_struct(), y, g, faces[f][0], faces[f][1], 1 << f)
        assert np.array_equal(np.asarray(ops.to_host(y)), one), order
    l, z, a = _field43(ops)
    ops.apply_bc_cell_faces(l.c_struct(), z, g, [None, faces[1], None, faces[3]], 0b1010)      # a partial mask: the other faces untouched
    got = np.asarray(ops.to_host(z)).reshape(5, 6)
    assert np.array_equal(got[1:4, 0], a[1:4, 0]) and np.array_equal(got[0], a[0]) and np.array_equal(got[1:4, 5], -a[1:4, 4])


# -- the interpreter: merging and refusals ------------------------------------------------------------------------------------------------
HEAD = """
Domain global< [0.0, 0.0] to [1.0, 1.0] >
Layout H< Real, Cell >@all {
  ghostLayers = [1, 1] with communication
  duplicateLayers = [0, 0] with communication
}
Globals {
  Var top : Real = 2.5
}
Field c< global, H, wall ( ) >@finest
Field e< global, H, %s >@finest
Function wall@finest ( ) : Unit {
%s
}
Function Application {
  loop over c@finest {
    c@finest = 1.0 + vf_cellCenter_x
  }
  loop over e@finest {
    e@finest = 2.0
  }
  apply bc to c@finest
}
"""
WEST = "  loop over c only ghost [-1, 0] on boundary {\n    c = 0. - c@[1, 0]\n  }\n"
EAST = "  loop over c only ghost [1, 0] on boundary {\n    c = top - c@[-1, 0]\n  }\n"
SOUTH = "  loop over c only ghost [0, -1] on boundary {\n    c = -c@[0, 1]\n  }\n"
NORTH = "  loop over c only ghost [0, 1] on boundary {\n    c = vf_nodePosition_x * top - c@[0, -1]\n  }\n"
K2 = dict(dimensionality=2, minLevel=2, maxLevel=2)


def _run(body, ebc="None", **kw):
    ops = Counting()
    P = exa4.Exa4Program(HEAD % (ebc, body), dict(K2), ops=ops, **kw)
    P.run()
    return P, [c for c in ops.calls if c != "stencil_op"]


def test_ghost_loops_of_one_function_merge_into_one_faces_call():
    P, calls = _run(WEST + EAST + SOUTH + NORTH)
    assert calls == [("apply_bc_cell_faces", 15)]
    Q, sep = _run(WEST + EAST + SOUTH + NORTH, fuse=False)
    assert sep == ["apply_bc_cell"] * 4
    c, d = P.fields[("c", 2)], Q.fields[("c", 2)]
    got = np.asarray(P.ops.to_host(c.data(0))).reshape(6, 6)
    assert np.array_equal(got, np.asarray(Q.ops.to_host(d.data(0))).reshape(6, 6))
    # the values: the global through its value, the node position of the ghost cell itself (h = 0.25)
    assert got[2, 5] == 2.5 - got[2, 4] and got[2, 0] == 0. - got[2, 1] and got[0, 2] == -got[1, 2]
    assert got[5, 3] == (2 * 0.25 + 0.0) * 2.5 - got[4, 3]
    # timers of one name between the loops do not end the group
    timed = "  startTimer ( 'bc' )\n" + WEST + "  stopTimer ( 'bc' )\n  startTimer ( 'bc' )\n" + EAST + SOUTH + "  stopTimer ( 'bc' )\n"
    assert _run(timed)[1] == [("apply_bc_cell_faces", 0b0111)]


def test_merging_ends_at_a_repeated_face_and_at_a_foreign_statement():
    assert _run(WEST + EAST + WEST + SOUTH)[1] == [("apply_bc_cell_faces", 0b0011), ("apply_bc_cell_faces", 0b0101)]
    foreign = "  loop over e {\n    e = 3.0\n  }\n"
    assert _run(WEST + EAST + foreign + SOUTH)[1] == [("apply_bc_cell_faces", 0b0011), "apply_bc_cell"]
    other = "  loop over e only ghost [0, -1] on boundary {\n    e = -e@[0, 1]\n  }\n"
    assert _run(WEST + other + SOUTH)[1] == ["apply_bc_cell"] * 3      # another field
    two = "  stopTimer ( 'a' )\n  startTimer ( 'b' )\n"
    assert _run("  startTimer ( 'a' )\n" + WEST + two + EAST + "  stopTimer ( 'b' )\n")[1] == ["apply_bc_cell"] * 2      # two timers between


REFUSALS = [
    ("field in E", WEST.replace("0. - c", "e - c"), "a field access inside the value E"),
    ("offset in E", WEST.replace("0. - c", "vf_cellCenter_x@[1, 0] - c"), "offset"),
    ("wrong side", WEST.replace("c@[1, 0]", "c@[-1, 0]"), "not the one inside the face"),
    ("swapped", WEST.replace("0. - c@[1, 0]", "c@[1, 0] - 0."), "the body of a ghost loop must be"),
    ("scaled", WEST.replace("0. - c@[1, 0]", "0. - 2.0 * c@[1, 0]"), r"or `c = E - c@\[\.\.\]`"),
]


@pytest.mark.parametrize("what,body,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_ghost_loop_refusals_by_their_words(what, body, words):
    with pytest.raises(Exa4Unsupported, match=words):
        _run(body)


def test_node_position_stays_refused_in_cell_loops_and_dirichlet_values():
    with pytest.raises(Exa4Unsupported, match="vf_nodePosition_x in a loop over cell fields"):
        _run(WEST.replace("c = 0. - c@[1, 0]", "c = 0. - c@[1, 0]") + "  loop over e {\n    e = vf_nodePosition_x\n  }\n")
    with pytest.raises(Exa4Unsupported, match="vf_nodePosition_x in an expression of a cell field"):
        _run(WEST, ebc="vf_nodePosition_x")
    ops = Star2dOracleOps()
    l, x, _ = _field43(ops)
    with pytest.raises(ValueError, match="unknown opcode"):      # the kernel layer: the opcodes are operands of the new kind alone
        ops.apply_bc_cell(l.c_struct(), x, _geom(), BC_DIRICHLET, ExprC.from_program([("nx", None)]), 1)
