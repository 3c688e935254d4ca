"""Coupled systems of cell fields without a GPU.  The numpy restatement of the system entry points (tests/system_ops.py) is a solver
for its own operator, and the library exports them; the interpreter parses `repeat with`, `solve locally` and coefficient stencils,
issues one launch per system loop without deferring or fusing it, refuses what it does not build by name, scopes variables of a
repeat body to one pass, runs the reference's optical-flow benchmark program against its results file and prints the results files'
lines from the own examples, on one block and on two over gloo."""
import numpy as np
import pytest

from system_cases import SHAPES, SysData, boxes, laplace, layouts
from system_ops import SYS_APPLY, SYS_RESIDUAL, SystemOracleOps, solve3


@pytest.fixture(scope="module")
def orc():
    return SystemOracleOps()


def _colour_mask(l, b, e, colour):
    """Boolean array over the whole allocation: the cells of the box with (i0 + i1 + i2) % 2 == colour."""
    ref = [l.pad_l[d] + l.ghost[d] for d in range(3)]
    tot = [l.tot(d) for d in range(3)]
    m = np.zeros((tot[2], tot[1], tot[0]), dtype=bool)
    i2, i1, i0 = np.meshgrid(np.arange(b[2], e[2]), np.arange(b[1], e[1]), np.arange(b[0], e[0]), indexing="ij")
    m[tuple(slice(b[d] + ref[d], e[d] + ref[d]) for d in (2, 1, 0))] = ((i0 + i1 + i2) % 2) == colour
    return m.reshape(-1)


@pytest.mark.parametrize("nd,n,cells", SHAPES, ids=["%dd-n%d" % (s[0], s[1]) for s in SHAPES])
@pytest.mark.parametrize("box", ["full", "interior"])
@pytest.mark.parametrize("pattern", ["full", "alias", "null"])
@pytest.mark.parametrize("colour", [0, 1])
def test_local_solve_is_exact_for_its_cell(orc, nd, n, cells, box, pattern, colour):
    """After one sys_relax of a colour with relax = 1.0 the sys_op residual at the cells of that colour is zero to 1e-12 relative to
    |f| (the operator's diagonal is ~2e2, |f| < 1: a few roundings of products of that size); the other colour and everything
    outside the box keep their bits."""
    lu, lo = layouts(nd, cells, 2)
    b, e = boxes(nd, cells)[box]
    L = laplace(nd, order=colour)
    s = SysData(orc, n, lu, lo, pattern)
    before = [t.numpy().copy() for t in s.u]
    frozen = [t.numpy().copy() for t in s.f + [x for row in s.g for x in row if x is not None]]
    orc.sys_relax(lu.c_struct(), s.u, lo.c_struct(), s.f, lo.c_struct(), s.g, L, 1.0, colour, b, e)
    sel = _colour_mask(lu, b, e, colour)
    for c in range(n):
        assert np.array_equal(s.u[c].numpy()[~sel], before[c][~sel]), "unknown %d changed off the colour's cells" % c
        assert not np.array_equal(s.u[c].numpy()[sel], before[c][sel])
    for got, want in zip(s.f + [x for row in s.g for x in row if x is not None], frozen):
        assert np.array_equal(got.numpy(), want)
    for t in s.dst:
        t.zero_()
    orc.sys_op(SYS_RESIDUAL, lu.c_struct(), s.u, lo.c_struct(), s.f, lo.c_struct(), s.g, lo.c_struct(), s.dst, L, (1 << n) - 1, b, e)
    selo = _colour_mask(lo, b, e, colour)
    fmax = max(float(np.abs(t.numpy()).max()) for t in s.f)
    for c in range(n):
        r = float(np.abs(s.dst[c].numpy()[selo]).max())
        assert r <= 1e-12 * fmax, "row %d: residual %.3e at the relaxed cells" % (c, r)


def test_residual_is_rhs_minus_apply_and_rows_outside_the_mask_stay(orc):
    nd, n, cells = SHAPES[2]
    lu, lo = layouts(nd, cells, 0)
    b, e = boxes(nd, cells)["interior"]
    L = laplace(nd, 1)
    s = SysData(orc, n, lu, lo, "alias")
    keep = [t.numpy().copy() for t in s.dst]
    orc.sys_op(SYS_APPLY, lu.c_struct(), s.u, lo.c_struct(), s.f, lo.c_struct(), s.g, lo.c_struct(), s.dst, L, 0b010, b, e)
    assert np.array_equal(s.dst[0].numpy(), keep[0]) and np.array_equal(s.dst[2].numpy(), keep[2])
    au = s.dst[1].numpy().copy()
    orc.sys_op(SYS_RESIDUAL, lu.c_struct(), s.u, lo.c_struct(), s.f, lo.c_struct(), s.g, lo.c_struct(), s.dst, L, 0b010, b, e)
    inside = _colour_mask(lo, b, e, 0) | _colour_mask(lo, b, e, 1)
    assert np.array_equal(s.dst[1].numpy()[inside], (s.f[1].numpy() - au)[inside])
    assert np.array_equal(s.dst[1].numpy()[~inside], keep[1][~inside])


def test_cramer3_solves_a_known_system():
    a = [[np.array(v) for v in row] for row in ((4.0, 1.0, -2.0), (0.5, 5.0, 1.0), (-1.0, 2.0, 6.0))]
    x = np.array([1.0, -2.0, 3.0])
    b = [sum(a[c][d] * x[d] for d in range(3)) for c in range(3)]
    got = solve3(a, b)
    assert np.allclose([float(v) for v in got], x, rtol=1e-14)


def test_pointwise_mul_is_negate_then_multiply(orc):
    from exastencils_amd.layout import FieldLayout

    l = FieldLayout.cell(2, (6, 4), 1)
    x, y, d = (orc.new_array(l.size) for _ in range(3))
    orc.fill_random(x, 1)
    orc.fill_random(y, 2)
    orc.fill_random(d, 3)
    keep = d.numpy().copy()
    orc.pointwise_mul(l.c_struct(), x, l.c_struct(), y, l.c_struct(), d, -1.0, [0, 0, 0], [6, 4, 1])
    inside = _colour_mask(l, [0, 0, 0], [6, 4, 1], 0) | _colour_mask(l, [0, 0, 0], [6, 4, 1], 1)
    assert np.array_equal(d.numpy()[inside], ((-x.numpy()) * y.numpy())[inside])
    assert np.array_equal(d.numpy()[~inside], keep[~inside])


def test_library_declares_the_system_entry_points():
    """Header, exported symbols and ctypes mirror: the struct is the header's (4 + 4 x 92 bytes of layouts, padded to 8, then 18 pointers)."""
    import ctypes as C

    from exastencils_amd import lib

    for name in ("examg_sys_op", "examg_sys_relax", "examg_pointwise_mul"):
        assert name in lib.SYMBOLS
    assert lib.SysC.u.offset == 376 and C.sizeof(lib.SysC) == 376 + 8 * 18


# -- the interpreter: repeat with, coefficient stencils, system rows, solve locally ----------------------------------------------
import os  # noqa: E402
import re  # noqa: E402
import socket  # noqa: E402

from test_exa4 import REF  # noqa: E402

from exastencils_amd import exa4, knowledge  # noqa: E402
from exastencils_amd.domain import RectDomain  # noqa: E402
from exastencils_amd.exa4_parser import Exa4Unsupported, Parser  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples", "exa4")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _text(name):
    with open(os.path.join(EX, name)) as f:
        return f.read()


def _golden(nd):
    with open(os.path.join(GOLDEN, "Application_OpticalFlow%dD.results" % nd)) as f:
        return f.read()


def _run(text, nd, hi, ops=None, **kw):
    P = exa4.Exa4Program(text, dict(dimensionality=nd, minLevel=2, maxLevel=hi), ops=ops or SystemOracleOps(), **kw)
    return P, P.run()


def test_parser_repeat_with_and_solve_locally():
    a = Parser(_text("optflow2d.exa4")).parse()
    smooth = [f for f in a.functions if f.name == "Smooth"][0]
    rw = smooth.body[0][3][0]
    assert rw[0] == "repeatwith" and len(rw[1]) == 2 and [s[0] for s in rw[2]] == ["comm", "comm", "loop", "applybc", "applybc"]
    solve = rw[2][2][5][0]
    assert solve[0] == "solve" and solve[1] is False and solve[2] == ("num", 1.0)
    assert [r[0][1] for r in solve[3]] == ["u", "v"] and [r[2][1] for r in solve[3]] == ["f_u", "f_v"]
    cuv = [s for s in a.stencils if s.name == "Cuv"][0]
    assert cuv.entries == [((0, 0), ("fld", "Jxy", None, None))]
    assert [f.name for f in Parser("Field It< g, L, None >@finest\nField It< g, L, None >@finest\n").parse().fields] == ["It", "It"]


class Recording(SystemOracleOps):
    """Records the name of every kernel-layer call."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def __getattribute__(self, name):
        a = object.__getattribute__(self, name)
        if callable(a) and not name.startswith("_") and name not in ("new_array", "new_scalar", "ptr", "to_host", "from_host", "scalar_value", "synchronize"):
            calls = object.__getattribute__(self, "calls")

            def rec(*args, **kw):
                calls.append(name)
                return a(*args, **kw)

            return rec
        return a


def test_system_loops_are_one_launch_each_and_never_deferred_or_fused():
    """`fuse=True` and `fuse=False` issue the same calls: the system loops run where they stand (cell fields are never deferred, and
    no one-pass form takes them); every residual / apply loop is one sys_op, every coloured solve one sys_relax."""
    runs = []
    for fuse in (True, False):
        ops = Recording()
        P, out = _run(_text("optflow2d.exa4"), 2, 4, ops=ops, fuse=fuse)
        runs.append((out, ops.calls, P.launches))
    assert runs[0] == runs[1]
    calls = runs[0][1]
    assert calls.count("pointwise_mul") == 5 and "sys_relax" in calls and "sys_op" in calls
    assert not {"rbgs_sweep_fused", "residual_restrict", "cg_coarse", "jacobi2"} & set(calls)
    # V(3,3) with two colours on levels 4 and 3: 24 relaxations per cycle
    assert calls.count("sys_relax") == 24 * (len(runs[0][0]) - 1)


@pytest.mark.parametrize("nd,hi", [(2, 8), (3, 6)])
def test_own_example_prints_the_reference_results(nd, hi):
    """256^2 and 64^3 cells, the sizes of the reference's result files; the norm is a reduction loop with one `+=` product per
    component, accumulated statement by statement.  The 64^3 run takes about eight seconds on the numpy restatement: kept at the
    golden's size."""
    _, out = _run(_text("optflow%dd.exa4" % nd), nd, hi)
    assert "\n".join(out) + "\n" == _golden(nd)


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference checkout not present")
def test_reference_benchmark_program_against_the_results_file():
    """Benchmark/OptFlow2D/2D_FD_OptFlow.exa4 as it is, with Testing/Application/OpticalFlow2D.knowledge: start residual and the four
    cycles agree with the results file of the vector-field form to one unit of its fourth significant digit."""
    k = knowledge.parse_file(os.path.join(REF, "Testing", "Application", "OpticalFlow2D.knowledge"))
    with open(os.path.join(REF, "Benchmark", "OptFlow2D", "2D_FD_OptFlow.exa4")) as f:
        P = exa4.Exa4Program(f.read(), k, ops=SystemOracleOps())
    out = P.run()
    got = [float(out[0].split()[-1])] + [float(re.match(r"Residual after \d+ iterations is (\S+)", l).group(1)) for l in out[1:] if l.startswith("Residual after")]
    want = [float(l) for l in _golden(2).split()]
    assert len(got) == len(want) == 5
    for g, w in zip(got, want):
        unit = 10.0 ** (int(np.floor(np.log10(w))) - 3)
        assert abs(g - w) <= unit


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference checkout not present")
def test_fixtures_are_the_reference_results_files():
    for nd in (2, 3):
        with open(os.path.join(REF, "Testing", "Application", "OpticalFlow%dD.results" % nd)) as f:
            assert f.read() == _golden(nd)


SOLVE2 = "solve locally relax 1.0 {"
REFUSALS = [
    ("with jacobi", 2, lambda t: t.replace(SOLVE2, "solve locally with jacobi relax 1.0 {"), "with jacobi"),
    ("uncoloured loop", 2, lambda t: re.sub(r"repeat with \{\n\s*\( 0 == .*\n\s*\( 1 == .*\n", "repeat 1 times {\n", t), "uncoloured loop"),
    ("another condition", 2, lambda t: t.replace("( 0 == ( ( i0 + i1 ) % 2 ) ),", "( 0 == ( i0 % 2 ) ),"), "repeat with: a condition other than"),
    ("unknown with offset", 2, lambda t: t.replace("          u => (", "          u@[1, 0] => ("), "offset access"),
    ("four unknowns", 3, lambda t: t.replace("          u => (", "          r_u => ( Cuu * r_u + weight * weight * Lap * r_u ) == f_u\n          u => ("), "more unknowns than 3"),
    ("Laplacians differ", 2, lambda t: t.replace("          v => ( Cvu * u + Cvv * v + weight * weight * Lap * v )", "          v => ( Cvu * u + Cvv * v + 2.0 * Lap * v )"),
     "Laplacians differ"),
    ("coefficient entry off the centre", 2, lambda t: t.replace("Stencil Cuu@all {\n  [0, 0] => Jxx", "Stencil Cuu@all {\n  [1, 0] => Jxx"), "off the centre"),
    ("coefficient stencil with two entries", 2, lambda t: t.replace("Stencil Cuu@all {\n  [0, 0] => Jxx", "Stencil Cuu@all {\n  [0, 0] => Jxx\n  [1, 0] => 1.0"), "more than one entry"),
    ("unknown that is no field of the rows", 2, lambda t: t.replace("          v => ( Cvu * u + Cvv * v +", "          v => ( Cvu * r_u + Cvv * v +"), "exactly the fields of the rows"),
    ("right-hand side that is no field", 2, lambda t: t.replace(") == f_v\n        }", ") == 0.0\n        }"), "right-hand side of a row must be a field"),
    ("coefficient stencil outside a system row", 2, lambda t: t.replace("      q_u = ( Cuu * p_u ) + ( Cuv * p_v ) + ( weight * weight * Lap * p_u )", "      q_u = Cuu * p_u"),
     "point-wise coefficient stencil"),
]


MINI = """
Domain global< [0.0, 0.0] to [1.0, 1.0] >
Layout Halo< Real, %(loc)s >@all {
  ghostLayers = [1, 1] with communication
  duplicateLayers = [%(dup)s, %(dup)s] with communication
}
Layout Five< ColumnVector<Real, 5>, Node >@all {
  ghostLayers = [0, 0]
  duplicateLayers = [1, 1]
}
Field u< global, Halo, %(bc)s >@all
Field v< global, Halo, %(bc)s >@all
Field f_u< global, Halo, None >@all
Field f_v< global, Halo, None >@all
Field J< global, Halo, None >@all
Field five< global, Five, None >@all
Stencil Lap@all {
  [0, 0] => 4.0
  [-1, 0] => -1.0
  [1, 0] => -1.0
  [0, -1] => -1.0
  [0, 1] => -1.0
}
StencilField LapField< five => Lap >@all
Stencil C@all {
  [0, 0] => J
}
Function Application {
  repeat with {
    ( 0 == ( ( i0 + i1 ) %% 2 ) ),
    ( 1 == ( ( i0 + i1 ) %% 2 ) ),
    loop over u@finest {
      solve locally {
        u@finest => ( C@finest * u@finest + C@finest * v@finest + %(lap)s@finest * u@finest ) == f_u@finest
        v@finest => ( C@finest * u@finest + C@finest * v@finest + %(lap)s@finest * v@finest ) == f_v@finest
      }
    }
  }
}
"""


@pytest.mark.parametrize("what,subst,text", [
    ("node fields", dict(loc="Node", dup="1", bc="0.0", lap="Lap"), "solve locally on node field u"),
    ("stencil field as L", dict(loc="Cell", dup="0", bc="Neumann", lap="LapField"), "a stencil field (LapField) as the constant stencil of a system"),
], ids=["node-fields", "stencil-field-as-L"])
def test_refusals_of_node_fields_and_stencil_fields(what, subst, text):
    with pytest.raises(Exa4Unsupported, match=re.escape(text)):
        _run(MINI % subst, 2, 3)
    if subst["lap"] == "Lap" and subst["loc"] == "Node":
        return
    # the same program with the constant stencil runs: the refusal above is the stencil field's, nothing else's
    _run(MINI % dict(subst, lap="Lap"), 2, 3)


def test_variable_declared_in_a_repeat_body_lives_for_one_pass():
    """The generated code declares it in the loop's block: the next pass's first statements see the global of that name again (the
    coarse-grid CG of the optical-flow benchmark declares `Var alpha` at the end of a pass that starts with `alpha * alpha * Laplace`)."""
    text = """
Domain global< [0.0, 0.0] to [1.0, 1.0] >
Globals {
  Val alpha : Real = 3.0
}
Function Application {
  Var outer : Real = 1.0
  repeat 2 times {
    print ( alpha )
    Var alpha : Real = 7.0
    Var outer : Real = 5.0
    print ( alpha )
  }
  print ( alpha )
  print ( outer )
}
"""
    P = exa4.Exa4Program(text, dict(dimensionality=2, minLevel=2, maxLevel=2), ops=SystemOracleOps())
    P.run()
    assert P.printed_values == [3.0, 7.0, 3.0, 7.0, 3.0, 1.0]


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference checkout not present")
@pytest.mark.parametrize("kfile,start", [("2D_FD_OptFlow.knowledge", "0.218783"), ("2D_FD_OptFlow_CUDA.knowledge", "0.445561")])
def test_reference_benchmark_program_with_its_own_knowledge_files_at_a_reduced_size(kfile, start):
    """The benchmark's own knowledge files ask for levels 2..11 (4096^2 cells); everything else as they say, maxLevel reduced to 4.
    One fragment gives the 16^2 cells and the start residual of Testing/Application/OpticalFlow2D.knowledge at that size; the CUDA
    file's 2 x 2 fragments per block give 32^2 cells (the start residual of one fragment at level 5).  Both converge in four cycles."""
    base = os.path.join(REF, "Benchmark", "OptFlow2D")
    k = knowledge.parse_file(os.path.join(base, kfile))
    k["maxLevel"] = 4
    with open(os.path.join(base, "2D_FD_OptFlow.exa4")) as f:
        out = exa4.Exa4Program(f.read(), k, ops=SystemOracleOps()).run()
    res = [l for l in out if l.startswith("Residual after")]
    assert out[0].split()[-1] == start and len(res) == 4
    assert float(res[-1].split()[5]) <= 1.0e-5 * float(start)


@pytest.mark.parametrize("name,nd,edit,text", REFUSALS, ids=[r[0].replace(" ", "-") for r in REFUSALS])
def test_refusals_by_name(name, nd, edit, text):
    src = _text("optflow%dd.exa4" % nd)
    bad = edit(src)
    assert bad != src, "the edit did not apply"
    with pytest.raises(Exa4Unsupported, match=re.escape(text)):
        _run(bad, nd, 3)


# -- two blocks over gloo ---------------------------------------------------------------------------------------------------------
K2 = dict(dimensionality=2, minLevel=2, maxLevel=4, domain_fragmentLength_x=2, domain_fragmentLength_y=2)


def _worker(rank, world, port, out_dir):
    import json

    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from exastencils_amd.comm import Communicator

    ops = SystemOracleOps()
    dom = RectDomain(2, (2, 1, 1), rank, (1, 2, 1))
    P = exa4.Exa4Program(_text("optflow2d.exa4"), dict(K2), ops=ops, domain=dom, comm=Communicator(dom, ops))
    out = P.run()
    json.dump({"lines": out, "values": P.printed_values, "messages": P.comm.stats["messages"]}, open(os.path.join(out_dir, "r%d.json" % rank), "w"))
    dist.barrier()
    dist.destroy_process_group()


def test_optflow2d_on_two_blocks_in_x_prints_the_same_lines(tmp_path):
    import json

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    single = exa4.Exa4Program(_text("optflow2d.exa4"), dict(K2), ops=SystemOracleOps())
    lines = single.run()
    for r in range(2):
        meta = json.load(open(tmp_path / ("r%d.json" % r)))
        assert meta["messages"] > 0
        assert meta["lines"] == lines
