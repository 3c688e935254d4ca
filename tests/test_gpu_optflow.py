"""GPU parity of the coupled-system entry points (include/examg.h: examg_sys_op, examg_sys_relax, examg_pointwise_mul) against
their numpy restatement (tests/system_ops.py): point-wise kernels, bit-identical over the WHOLE arrays -- a stray write outside
the box, or to the other colour, shows.  Both access widths: the product library takes 16-byte pairs wherever the arguments'
pairs are aligned, the debug library is told to take 8-byte accesses."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from system_cases import SHAPES, SysData, boxes, laplace, layouts
from system_ops import SYS_APPLY, SYS_RESIDUAL, SystemOracleOps

from exastencils_amd import lib
from exastencils_amd.field import Stencil
from exastencils_amd.layout import FieldLayout
from exastencils_amd.lib import ExamgError


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
    return SystemOracleOps()


@pytest.fixture(params=["pairs", "narrow"])
def gpu(request, hip, hipd):
    if request.param == "pairs":
        yield hip
        return
    hipd.L.examg_debug_sys_narrow(1)
    try:
        yield hipd
    finally:
        hipd.L.examg_debug_sys_narrow(0)


def same(a, b, what):
    if not np.array_equal(a, b):
        d = np.abs(a - b)
        raise AssertionError("%s: %d of %d values differ, max abs %.3e" % (what, int((d > 0).sum()), d.size, d.max()))


def compare(gpu, orc, fn, what):
    """fn(ops) -> SysData after the calls under test; every array of the system is compared whole."""
    g = fn(gpu)
    gpu.synchronize()
    c = fn(orc)
    for k, (x, y) in enumerate(zip(g.arrays(), c.arrays())):
        same(gpu.to_host(x), orc.to_host(y), "%s, array %d" % (what, k))


CASES = [(nd, n, cells, align, box) for nd, n, cells in SHAPES for align in (0, 2) for box in ("full", "interior")]
IDS = ["%dd-n%d-%s-a%d-%s" % (nd, n, "x".join(map(str, cells)), align, box) for nd, n, cells, align, box in CASES]


def sys_op_all(ops, nd, n, cells, align, box, pattern="full", ghost_other=1, order=0):
    """Every single row and all rows, APPLY and RESIDUAL, one after the other into the same destinations (the last writer of a row is
    the all-rows RESIDUAL; the arrays are compared after each call by running the sequence to that point)."""
    lu, lo = layouts(nd, cells, align, ghost_other)
    b, e = boxes(nd, cells)[box]
    L = laplace(nd, order)
    out = []
    for mode in (SYS_APPLY, SYS_RESIDUAL):
        for mask in [1 << c for c in range(n)] + [(1 << n) - 1]:
            s = SysData(ops, n, lu, lo, pattern)
            ops.sys_op(mode, lu.c_struct(), s.u, lo.c_struct(), s.f, lo.c_struct(), s.g, lo.c_struct(), s.dst, L, mask, b, e)
            out.append(s)
    return out


@pytest.mark.parametrize("nd,n,cells,align,box", CASES, ids=IDS)
def test_sys_op_bitwise(gpu, orc, nd, n, cells, align, box):
    g = sys_op_all(gpu, nd, n, cells, align, box)
    gpu.synchronize()
    c = sys_op_all(orc, nd, n, cells, align, box)
    for k, (sg, sc) in enumerate(zip(g, c)):
        for j, (x, y) in enumerate(zip(sg.arrays(), sc.arrays())):
            same(gpu.to_host(x), orc.to_host(y), "sys_op call %d, array %d" % (k, j))


def sys_relax_all(ops, nd, n, cells, align, box, pattern="full", ghost_other=1, order=0):
    lu, lo = layouts(nd, cells, align, ghost_other)
    b, e = boxes(nd, cells)[box]
    L = laplace(nd, order)
    out = []
    for relax in (1.0, 0.7):
        for colours in ((0,), (1,), (0, 1)):
            s = SysData(ops, n, lu, lo, pattern)
            for colour in colours:
                ops.sys_relax(lu.c_struct(), s.u, lo.c_struct(), s.f, lo.c_struct(), s.g, L, relax, colour, b, e)
            out.append(s)
    return out


@pytest.mark.parametrize("nd,n,cells,align,box", CASES, ids=IDS)
def test_sys_relax_bitwise(gpu, orc, nd, n, cells, align, box):
    g = sys_relax_all(gpu, nd, n, cells, align, box)
    gpu.synchronize()
    c = sys_relax_all(orc, nd, n, cells, align, box)
    for k, (sg, sc) in enumerate(zip(g, c)):
        for j, (x, y) in enumerate(zip(sg.arrays(), sc.arrays())):
            same(gpu.to_host(x), orc.to_host(y), "sys_relax sequence %d, array %d" % (k, j))


@pytest.mark.parametrize("pattern,ghost_other,order", [("alias", 1, 0), ("null", 1, 1), ("full", 0, 1), ("alias", 0, 0)])
@pytest.mark.parametrize("nd,n,cells", SHAPES[::2] + [SHAPES[3]], ids=["2d-n2", "3d-n3", "3d-n2"])
def test_aliased_null_and_own_layouts(gpu, orc, nd, n, cells, pattern, ghost_other, order):
    """Aliased off-diagonal pointers, null entries off and on the diagonal, rhs / coefficients / destinations in a layout without ghost
    layers (other origin parity: without alignment padding the pairs of the arguments do not line up), the second entry order."""
    for align in (0, 2):
        for fn in (sys_op_all, sys_relax_all):
            g = fn(gpu, nd, n, cells, align, "interior", pattern, ghost_other, order)
            gpu.synchronize()
            c = fn(orc, nd, n, cells, align, "interior", pattern, ghost_other, order)
            for k, (sg, sc) in enumerate(zip(g, c)):
                for j, (x, y) in enumerate(zip(sg.arrays(), sc.arrays())):
                    same(gpu.to_host(x), orc.to_host(y), "%s align %d call %d, array %d" % (fn.__name__, align, k, j))


def test_empty_box_is_a_no_op(hip, orc):
    nd, n, cells = SHAPES[0]
    lu, lo = layouts(nd, cells, 2)

    def run(ops):
        s = SysData(ops, n, lu, lo)
        L = laplace(nd)
        ops.sys_op(SYS_RESIDUAL, lu.c_struct(), s.u, lo.c_struct(), s.f, lo.c_struct(), s.g, lo.c_struct(), s.dst, L, 3, [3, 2, 0], [3, 5, 1])
        ops.sys_relax(lu.c_struct(), s.u, lo.c_struct(), s.f, lo.c_struct(), s.g, L, 1.0, 0, [0, 4, 0], [9, 4, 1])
        ops.pointwise_mul(lo.c_struct(), s.f[0], lo.c_struct(), s.f[1], lo.c_struct(), s.dst[0], 1.0, [5, 0, 0], [5, 6, 1])
        return s

    compare(hip, orc, run, "empty box")


@pytest.mark.parametrize("nd,cells", [(2, (130, 6)), (3, (66, 5, 3))])
@pytest.mark.parametrize("s", [1.0, -1.0])
def test_pointwise_mul_bitwise(hip, orc, nd, cells, s):
    """dst = (s * x) * y with every argument in a layout of its own; then in place on x."""
    lx, ly, ld = FieldLayout.cell(nd, cells, 1), FieldLayout.cell(nd, cells, 0), FieldLayout.cell(nd, cells, 1, align=2)
    b, e = boxes(nd, cells)["interior"]

    def run(ops):
        t = [ops.new_array(l.size) for l in (lx, ly, ld)]
        for k, a in enumerate(t):
            ops.fill_random(a, 40 + k)
        ops.pointwise_mul(lx.c_struct(), t[0], ly.c_struct(), t[1], ld.c_struct(), t[2], s, b, e)
        ops.pointwise_mul(lx.c_struct(), t[0], ly.c_struct(), t[1], lx.c_struct(), t[0], s, b, e)
        return t

    g = run(hip)
    hip.synchronize()
    c = run(orc)
    for k in range(3):
        same(hip.to_host(g[k]), orc.to_host(c[k]), "pointwise_mul array %d" % k)


class NoCentre(Stencil):
    """A stencil without a (0, 0, 0) entry: `diag` names entry 0, as a caller of the C ABI could."""
    diag_index = property(lambda self: 0)


def _refusals():
    nd, cells = 2, (8, 6)
    lu, lo = layouts(nd, cells, 0)
    good = dict(n=2, lu=lu, lf=lo, lg=lo, ld=lo, L=laplace(nd))
    split = lo.c_struct()
    split.transform = 1          # EXAMG_LAYOUT_SPLIT_X
    other = FieldLayout.cell(nd, (10, 6), 1)
    off_axis = Stencil([(0, 0, 0), (1, 1, 0)], [4.0, -1.0])
    no_centre = NoCentre([(-1, 0, 0), (1, 0, 0)], [-1.0, -1.0])
    return [
        ("n = 1", dict(good, n=1), "2 or 3"),
        ("n = 4", dict(good, n=4), "2 or 3"),
        ("node layout", dict(good, lg=FieldLayout.node(nd, cells, 0)), "not a cell layout"),
        ("colour-split layout", dict(good, lf=split), "colour-split"),
        ("coefficient layout of another size", dict(good, lg=other), "coefficient layout has"),
        ("rhs layout of another size", dict(good, lf=other), "rhs layout has"),
        ("off-axis entry", dict(good, L=off_axis), "not an axis entry"),
        ("no centre entry", dict(good, L=no_centre), "no centre entry"),
        ("u without ghost layer", dict(good, lu=FieldLayout.cell(nd, cells, 0)), "ghost layer"),
    ]


@pytest.mark.parametrize("name,args,text", _refusals(), ids=[r[0].replace(" ", "-") for r in _refusals()])
@pytest.mark.parametrize("entry", ["op", "relax"])
def test_refusals_launch_nothing(hip, name, args, text, entry):
    """Each refusal returns its error and leaves every array as it was."""
    n, big = args["n"], FieldLayout.cell(2, (10, 6), 1)
    t = [hip.new_array(big.size) for _ in range(4 * 4 + 3 * 4)]      # every array large enough for any of the layouts
    for k, a in enumerate(t):
        hip.fill_random(a, 70 + k)
    before = [hip.to_host(a).copy() for a in t]
    u, f, dst = t[0:n], t[4:4 + n], t[8:8 + n]
    g = [[t[12 + c * 4 + d] for d in range(n)] for c in range(n)]
    cs = lambda l: l if not hasattr(l, "c_struct") else l.c_struct()
    b, e = [0, 0, 0], [8, 6, 1]
    with pytest.raises(ExamgError, match=text):
        if entry == "op":
            hip.sys_op(SYS_RESIDUAL, cs(args["lu"]), u, cs(args["lf"]), f, cs(args["lg"]), g, cs(args["ld"]), dst, args["L"], 1, b, e)
        else:
            hip.sys_relax(cs(args["lu"]), u, cs(args["lf"]), f, cs(args["lg"]), g, args["L"], 1.0, 0, b, e)
    hip.synchronize()
    for k, a in enumerate(t):
        same(hip.to_host(a), before[k], "array %d after the refused call" % k)


# -- the interpreted example programs on the HIP kernels --------------------------------------------------------------------------
import os  # noqa: E402

from exastencils_amd import exa4  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {2: 8, 3: 6}          # 256^2 and 64^3 cells: the sizes of the reference's result files


def _program(nd, ops, hi=None, **kw):
    with open(os.path.join(ROOT, "examples", "exa4", "optflow%dd.exa4" % nd)) as f:
        return exa4.Exa4Program(f.read(), dict(dimensionality=nd, minLevel=2, maxLevel=hi or SIZES[nd]), ops=ops, **kw)


@pytest.mark.parametrize("nd", [2, 3])
def test_own_example_on_the_gpu_prints_the_reference_results(hip, orc, nd):
    """Both examples on HipOps print exactly the lines of the reference's result files, and the lines of the restatement run."""
    with open(os.path.join(ROOT, "tests", "golden", "Application_OpticalFlow%dD.results" % nd)) as f:
        golden = f.read()
    got = _program(nd, hip).run()
    assert "\n".join(got) + "\n" == golden
    assert got == _program(nd, orc).run()


def test_graph_replay_of_the_interpreted_cycle_is_bit_identical(hip):
    """`Smooth@level` and `Defect@level` of optflow2d.exa4 are free of host round trips (`repeat with`, `solve locally` loops, system
    rows, `apply bc`): under auto_graph they are recorded at their second call and replayed afterwards, guarded by the existing
    replay-equals-interpretation check.  Every field of every level ends with the bits of statement-by-statement execution."""
    plain = _program(2, hip, auto_graph=False)
    a = plain.run()
    P = _program(2, hip)
    assert P.auto_graph
    b = P.run()
    assert a == b and P.printed_values == plain.printed_values
    assert P.graph_replays > 0 and isinstance(P._auto_graphs.get(("Smooth", 8)), dict)
    hip.synchronize()
    for key, f in plain.fields.items():
        for s in range(f.num_slots):
            same(hip.to_host(P.fields[key].data(s)), hip.to_host(f.data(s)), "field %s@%d" % key)
