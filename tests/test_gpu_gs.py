"""Lexicographic Gauss-Seidel on the MI355X: examg_gs_sweep on its three routes (one workgroup, tiles, one launch per point hyperplane),
its schedule point by point, its refusals, and the two host drivers on top of it.

Reference (tests/gs_cases.py): FoldGS -- for t ascending the out-of-place loop of FoldOps, then exactly the points of the box with
i0 + a * i1 + b * i2 == t copied back; tests/test_gs.py pins it against the literal loop nest.  WHOLE allocations are compared with
np.array_equal: padding, ghost layers and boundary planes of u, the right-hand side and the coefficient array included.

Layouts: u with one ghost layer and rows padded to a multiple of 4, rhs and coefficients with no ghost layer -- an index formed with
another argument's layout reads or writes another point.
Shapes: node grids of 72 x 28 x 28 cells, 71 x 27 x 27 inner points.  A tile of the kernel is 32 times by 8 skewed rows by 8 planes,
not the 4 x 2 rows and planes the 72 x 20 x 12 grid of the feature's description assumes, so y and z are enlarged to give three tiles
and a remainder in every tiled direction for every stencil (rows: 27 for star stencils, 27 + 26 skewed rows for the others; planes:
27; times: 71 + 26 + 26 and 71 + 2 * 26 + 4 * 26).  Boxes: the whole interior; the sub-box [3, 1, 2) .. (70, 26, 25); the thin boxes
71 x 1 x 1, 1 x 27 x 27 and 71 x 27 x 1; an empty box.  2-D: 72 x 200 cells (a 2-D tile is 64 rows), the whole interior and a sub-box.
Each case runs on the product library as it routes and on the debug library with each route forced, twice from the same input.
Stencil fields: 7 entries in both weight forms, 27 entries, and entry counts no kernel is compiled for (6 in 3-D, 4 in 2-D); 5 entries in 2-D."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import gs_cases as G  # noqa: E402
import stencil_cases as S  # noqa: E402
from test_gpu_kernels import hip, hipd  # noqa: E402,F401  (fixtures)

from exastencils_amd import lib  # noqa: E402
from exastencils_amd.field import Stencil  # noqa: E402
from exastencils_amd.layout import FieldLayout  # noqa: E402
from exastencils_amd.lib import ExamgError  # noqa: E402

pytestmark = pytest.mark.gpu

FOLD = G.FoldGS()
CELLS3, CELLS2 = (72, 28, 28), (72, 200, 0)
BOXES3 = {
    "interior": ([1, 1, 1], [72, 28, 28]),
    "sub": ([3, 1, 2], [70, 26, 25]),
    "line": ([1, 5, 7], [72, 6, 8]),
    "slab_x": ([9, 1, 1], [10, 28, 28]),
    "plane_z": ([1, 1, 6], [72, 28, 7]),
    "empty": ([3, 1, 1], [3, 28, 28]),
}
BOXES2 = {"interior": ([1, 1, 0], [72, 200, 1]), "sub": ([3, 2, 0], [70, 197, 1])}
ROUTES = (lib.GS_ONE_WORKGROUP, lib.GS_TILED, lib.GS_PER_HYPERPLANE)


def layouts(nd):
    cells = CELLS3 if nd == 3 else CELLS2
    return FieldLayout.node(nd, cells, 1, align=4), FieldLayout.node(nd, cells, 0, True, False)


class Case:
    """Host data of one (stencil, box): u and rhs over their whole allocations, the stencil (constant or a coefficient field in planes)
    and, computed once, the reference result."""

    _cache = {}

    def __init__(self, nd, kind, box):
        self.nd, self.kind = nd, kind
        self.lu, self.lf = layouts(nd)
        self.b, self.e = (BOXES3 if nd == 3 else BOXES2)[box]
        rng = np.random.default_rng(900 + nd)
        self.u, self.f = rng.uniform(-1.0, 1.0, self.lu.size), rng.uniform(-1.0, 1.0, self.lf.size)
        self.cf = None
        if kind.startswith("field"):
            # field_inv_times / field_divide: 7 entries, the diagonal third; field27: 27 entries (the prefetching kernels); field6, field4:
            # the asymmetric entry lists, no kernel compiled for their entry count; field5: 2-D, the centre last
            lists = {"field27": lambda: G.twentyseven_point().offsets, "field6": lambda: G.upwind(3).offsets,
                     "field4": lambda: G.upwind(2).offsets, "field5": lambda: G.five_point(True).offsets}
            if kind in lists:
                proto = G.field_of(FOLD, lists[kind](), self.lf, len(kind) % 2)
            else:
                proto = G.coefficient_field(FOLD, self.lf, 1 if kind == "field_divide" else 0)
            self.cf, self.offsets, self.wform = np.array(proto.cfield, copy=True), list(proto.offsets), proto.wform
            self.w = 0.713
        else:
            self.st = {"seven": G.seven_point, "twentyseven": G.twentyseven_point, "five": G.five_point, "nine": G.nine_point,
                       "upwind": lambda: G.upwind(nd), "centre": G.centre_only}[kind.replace("_centre_last", "")](*([True] if kind.endswith("centre_last") else []))
            self.w = S.free_weight(self.st)

    @classmethod
    def get(cls, nd, kind, box):
        key = (nd, kind, box)
        if key not in cls._cache:
            c = cls._cache[key] = cls(nd, kind, box)
            c.want = c.run(FOLD)
        return cls._cache[key]

    def on(self, ops):
        u, f = ops.from_host(self.u.copy()), ops.from_host(self.f.copy())
        if self.cf is None:
            return u, f, self.st
        return u, f, Stencil(list(self.offsets), [], ops.from_host(self.cf.copy()), self.lf, 0, self.wform)

    def run(self, ops):
        u, f, st = self.on(ops)
        ops.gs_sweep(self.lu.c_struct(), u, self.lf.c_struct(), f, st, self.w, self.b, self.e)
        ops.synchronize()
        out = [np.array(ops.to_host(t), dtype=np.float64, copy=True) for t in (u, f)]
        if st.cfield is not None:
            out.append(np.array(ops.to_host(st.cfield), dtype=np.float64, copy=True))
        return out


def assert_same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            dd = np.abs(g - w)
            raise AssertionError("%s[%d]: %d of %d values differ, max abs %.3e" % (what, i, int((dd > 0).sum()), dd.size, np.nanmax(dd)))


class forced:
    """The debug library with one route of examg_gs_sweep forced (per host thread), restored on exit."""

    def __init__(self, hipd, route):
        self.L, self.route = hipd.L, route

    def __enter__(self):
        self.old = self.L.examg_debug_gs_route(self.route)

    def __exit__(self, *a):
        self.L.examg_debug_gs_route(self.old)


def schedule(hipd, case, st):
    """(route, launch, step) of examg_debug_gs_schedule for the case's box, arrays shaped (n2, n1, n0)."""
    n = [case.e[d] - case.b[d] for d in range(3)]
    launch = np.full(n[0] * n[1] * n[2], -1, dtype=np.int32)
    step = np.full(n[0] * n[1] * n[2], -1, dtype=np.int32)
    sc, lu, lf = st.c_struct(hipd.ptr), case.lu.c_struct(), case.lf.c_struct()
    r = hipd.L.examg_debug_gs_schedule(C.byref(lu), C.byref(lf), C.byref(sc), lib.ivec(case.b), lib.ivec(case.e), launch.ctypes.data,
                                       step.ctypes.data)
    count = hipd.L.examg_debug_gs_launches(C.byref(lu), C.byref(lf), C.byref(sc), lib.ivec(case.b), lib.ivec(case.e))
    return r, count, launch.reshape(n[2], n[1], n[0]), step.reshape(n[2], n[1], n[0])


def check_schedule(hipd, case, route):
    """The hook enumerates the sweep as the kernels do (launches, blocks, lanes, steps) and marks what it visits: every point of the
    box exactly once (-1: never, -2: more than once); (launch, step) of an earlier neighbour inside the box is smaller, of a later one
    larger -- so two dependent points never share a (launch, step)."""
    _, _, st = case.on(hipd)
    with forced(hipd, route):
        r, count, launch, step = schedule(hipd, case, st)
    assert r == route
    assert int((launch == -1).sum()) == 0, "route %d: %d points are visited by no lane" % (route, int((launch == -1).sum()))
    assert int((launch == -2).sum()) == 0, "route %d: %d points are visited more than once" % (route, int((launch == -2).sum()))
    assert step.min() >= 0 and launch.max() < count
    key = launch.astype(np.int64) * (int(step.max()) + 1) + step
    n2, n1, n0 = key.shape
    for o in st.offsets:
        if not any(o):
            continue
        src = tuple(slice(max(0, -o[d]), min(n, n - o[d])) for d, n in ((2, n2), (1, n1), (0, n0)))
        dst = tuple(slice(max(0, o[d]), min(n, n + o[d])) for d, n in ((2, n2), (1, n1), (0, n0)))
        p, q = key[src], key[dst]           # q: the point p + o
        if p.size == 0:
            continue
        if G.later(o):
            assert np.all(q > p), "route %d offset %r: a later neighbour is not scheduled later" % (route, o)
        else:
            assert np.all(q < p), "route %d offset %r: an earlier neighbour is not scheduled earlier" % (route, o)


def check_case(hip, hipd, nd, kind, box):
    case = Case.get(nd, kind, box)
    empty = any(case.e[d] <= case.b[d] for d in range(3))
    _, _, st = case.on(hip)
    routed = hip.gs_route(case.lu.c_struct(), case.lf.c_struct(), st, case.b, case.e)
    assert routed == lib.GS_EMPTY if empty else routed in (lib.GS_ONE_WORKGROUP, lib.GS_TILED)      # the cases are below the bound of the large stencil fields
    assert_same(case.run(hip), case.want, "%s %s as routed (%d)" % (kind, box, routed))
    assert_same(case.run(hip), case.want, "%s %s as routed, second run" % (kind, box))
    for route in ROUTES:
        if not empty:
            check_schedule(hipd, case, route)
        with forced(hipd, route):
            assert hipd.gs_route(case.lu.c_struct(), case.lf.c_struct(), st, case.b, case.e) == (lib.GS_EMPTY if empty else route)
            assert_same(case.run(hipd), case.want, "%s %s route %d" % (kind, box, route))
            assert_same(case.run(hipd), case.want, "%s %s route %d, second run" % (kind, box, route))
    if empty:
        assert_same(case.want, [case.u, case.f], "an empty box writes nothing")


@pytest.mark.parametrize("box", list(BOXES3))
@pytest.mark.parametrize("kind", ["seven", "twentyseven"])
def test_constant_stencils_3d(hip, hipd, kind, box):
    check_case(hip, hipd, 3, kind, box)


@pytest.mark.parametrize("box", ["interior", "sub"])
@pytest.mark.parametrize("kind", ["field_inv_times", "field_divide", "field6", "field27", "twentyseven_centre_last", "upwind", "centre"])
def test_coefficient_fields_entry_orders_and_asymmetric_stencils_3d(hip, hipd, kind, box):
    check_case(hip, hipd, 3, kind, box)


@pytest.mark.parametrize("box", list(BOXES2))
@pytest.mark.parametrize("kind", ["five", "nine", "five_centre_last", "upwind", "field5", "field4"])
def test_stencils_2d(hip, hipd, kind, box):
    check_case(hip, hipd, 2, kind, box)


def test_tiled_route_on_a_box_of_several_tiles_is_what_the_product_takes(hip):
    """The product library takes the tiled route for the whole interior without a hook, and one workgroup for a small box."""
    case = Case.get(3, "seven", "interior")
    _, _, st = case.on(hip)
    assert hip.gs_route(case.lu.c_struct(), case.lf.c_struct(), st, case.b, case.e) == lib.GS_TILED
    assert hip.gs_route(case.lu.c_struct(), case.lf.c_struct(), st, [1, 1, 1], [6, 6, 6]) == lib.GS_ONE_WORKGROUP
    # a 27-entry stencil field on more than 128^3 points: one launch per point hyperplane (the route is decided from the layouts alone;
    # the coefficient array is never read)
    big, bigf = FieldLayout.node(3, (160, 160, 160), 1), FieldLayout.node(3, (160, 160, 160), 0, True, False)
    f27 = Stencil(list(G.twentyseven_point().offsets), [], hip.new_array(8), bigf, 0, 0)
    f7 = Stencil(list(G.seven_point().offsets), [], hip.new_array(8), bigf, 0, 0)
    assert hip.gs_route(big.c_struct(), bigf.c_struct(), f27, [1, 1, 1], [160, 160, 160]) == lib.GS_PER_HYPERPLANE
    assert hip.gs_route(big.c_struct(), bigf.c_struct(), f27, [1, 1, 1], [129, 129, 129]) == lib.GS_TILED
    assert hip.gs_route(big.c_struct(), bigf.c_struct(), f7, [1, 1, 1], [160, 160, 160]) == lib.GS_TILED
    assert hip.gs_route(big.c_struct(), bigf.c_struct(), G.twentyseven_point(), [1, 1, 1], [160, 160, 160]) == lib.GS_TILED


# -- eligibility: refused before anything is launched ----------------------------------------------------------------------------------------
def test_refusals(hip):
    case = Case.get(3, "seven", "sub")
    lu, lf = case.lu.c_struct(), case.lf.c_struct()
    b, e = case.b, case.e
    u, f, st = case.on(hip)

    def refused(what, lu_, lf_, st_, u_=u, f_=f):
        assert hip.gs_route(lu_, lf_, st_, b, e) == lib.GS_REFUSED
        assert what in hip.L.examg_last_error().decode()
        with pytest.raises(ExamgError, match=what):
            hip.gs_sweep(lu_, u_, lf_, f_, st_, case.w, b, e)

    # offsets of reach 2 (the u layout has one ghost layer: the reach, not the allocation, must be what is refused)
    refused("reach 2", lu, lf, Stencil([(0, 0, 0), (-2, 0, 0), (1, 0, 0)], [3.0, -1.0, -1.0]))
    # entry-fastest coefficient records
    fcase = Case.get(3, "field_divide", "sub")
    _, _, planes = fcase.on(hip)
    refused("entry-fastest", lu, lf, planes.entry_fastest(hip))
    # a colour-split layout, for u and for the right-hand side
    split = case.lu.split_x()
    refused("colour-split", split.c_struct(), lf, st, u_=hip.new_array(split.size))
    refused("colour-split", lu, case.lf.split_x().c_struct(), st, f_=hip.new_array(case.lf.split_x().size))
    # a cell layout
    cu, cf = FieldLayout.cell(3, CELLS3, 1), FieldLayout.cell(3, CELLS3, 0)
    refused("cell layout", cu.c_struct(), cf.c_struct(), st, u_=hip.new_array(cu.size), f_=hip.new_array(cf.size))
    # a centre-only stencil (reach 0) on the whole allocation of a layout without ghost layers: the tile kernel loads the one-point
    # shell of the box whatever the stencil reaches, so the shell must be allocated
    bare = FieldLayout.node(3, CELLS3, 0)
    whole = [CELLS3[d] + 1 for d in range(3)]
    ub = hip.new_array(bare.size)
    assert hip.gs_route(bare.c_struct(), lf, G.centre_only(), [0, 0, 0], whole) == lib.GS_REFUSED
    with pytest.raises(ExamgError, match="one-point shell of the box leaves the u allocation"):
        hip.gs_sweep(bare.c_struct(), ub, lf, f, G.centre_only(), 0.4, [0, 0, 0], whole)
    assert hip.gs_route(bare.c_struct(), lf, G.centre_only(), [1, 1, 1], CELLS3) == lib.GS_TILED      # its interior has the shell
    assert float(ub.abs().max()) == 0.0
    # a box whose shell leaves the allocation
    assert hip.gs_route(lu, lf, st, [1, 1, 1], [80, 5, 5]) == lib.GS_REFUSED
    with pytest.raises(ExamgError, match="leaves the u allocation"):
        hip.gs_sweep(lu, u, lf, f, st, case.w, [1, 1, 1], [80, 5, 5])
    hip.synchronize()
    assert_same([hip.to_host(u), hip.to_host(f)], [case.u, case.f], "after the refused calls")
    assert hip.gs_route(lu, lf, st, b, e) == lib.GS_TILED


# -- the drivers ---------------------------------------------------------------------------------------------------------------------------
def _hip_helper(hip):
    """The helper layer on the device: GsMixin over the HIP kernel layer -- every statement but the sweep is the product's own kernel
    (reductions included, so the coarse solver takes the same steps), the sweep is the out-of-place loop of examg_stencil_op
    hyperplane by hyperplane with a masked copy."""
    torch = hip.torch

    class HipGS(G.GsMixin, type(hip)):
        def gs_sweep(self, lu, u, lf, rhs, st, w, begin, end):
            self.gs_calls = getattr(self, "gs_calls", 0) + 1
            a, b = G.skew(st.offsets)
            t_lo = begin[0] + a * begin[1] + b * begin[2]
            t_hi = (end[0] - 1) + a * (end[1] - 1) + b * (end[2] - 1)
            L = S.Lay(lu)
            i2, i1, i0 = np.meshgrid(*[np.arange(begin[d], end[d]) for d in (2, 1, 0)], indexing="ij")
            times = np.full(L.shape, -1, dtype=np.int64)
            times[L.box(begin, end)] = i0 + a * i1 + b * i2
            times = torch.from_numpy(times.reshape(-1)).to(u.device)
            for t in range(t_lo, t_hi + 1):
                scratch = u.clone()
                self.stencil_op(S.SMOOTH, lu, u, lf, rhs, lu, scratch, st, w, -1, begin, end)
                u.copy_(torch.where(times == t, scratch, u))

    H = HipGS.__new__(HipGS)
    H.__dict__.update(hip.__dict__)
    return H


@pytest.mark.parametrize("nd", [2, 3])
def test_solver_with_the_lexicographic_smoother(hip, nd):
    """SolverFromL3(smoother="gs"), levels 2..5: after three cycles the fields are those of the helper-layer run on the device bit for
    bit; the residual norms agree with the oracle-backed helper run within 1e-10 (test_gpu_solver's rule for reduction values)."""
    from test_gpu_solver import _close
    from test_gs import solver_run

    P = solver_run(hip, nd, 2, 5, cycles=3)
    Hh = _hip_helper(hip)
    Q = solver_run(Hh, nd, 2, 5, cycles=3)
    O = solver_run(G.oracle_gs(), nd, 2, 5, cycles=3)
    print("gs history gpu", P.res_history, "helper on the device", Q.res_history, "oracle helper", O.res_history)
    assert Hh.gs_calls == 3 * 6 * 3
    for l in P.levels:
        assert np.array_equal(hip.to_host(P.Solution[l].data()), hip.to_host(Q.Solution[l].data())), "Solution@%d" % l
    assert P.res_history == Q.res_history
    _close(P.res_history, O.res_history)
    for l in P.levels:      # ... and against the helper on the CPU oracle, which shares no kernel: within the tolerance of the norms
        got, want = hip.to_host(P.Solution[l].data()), O.ops.to_host(O.Solution[l].data())
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max(), "Solution@%d against the oracle-backed helper" % l
    assert P.res_history[-1] < 1e-2 * P.res_history[0]


def test_example_program_on_gpu(hip):
    """examples/exa4/poisson3d_gs.exa4, levels 2..5: interpreted, and with `Cycle@finest` replayed from its hipGraph, it prints the same
    values and leaves the same field, bit for bit; these are the values of the helper-layer run on the device and, within the
    tolerance of reduction values, of the oracle-backed helper."""
    from test_gpu_exa4 import _close
    from test_gs import run_example

    plain = run_example(hip, 2, 5, auto_graph=False)
    P = run_example(hip, 2, 5)
    assert P.auto_graph and P.graph_replays > 0 and plain.graph_replays == 0
    print("gs example gpu", P.printed_values)
    assert P.printed_values == plain.printed_values
    assert np.array_equal(hip.to_host(P.fields[("u", 5)].data()), hip.to_host(plain.fields[("u", 5)].data()))
    H = run_example(_hip_helper(hip), 2, 5, auto_graph=False)
    assert H.printed_values == plain.printed_values
    assert np.array_equal(hip.to_host(H.fields[("u", 5)].data()), hip.to_host(plain.fields[("u", 5)].data()))
    O = run_example(G.oracle_gs(), 2, 5)
    _close(P.printed_values, O.printed_values, O.printed_values[0])
    got, want = hip.to_host(P.fields[("u", 5)].data()), O.ops.to_host(O.fields[("u", 5)].data())
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
