"""The C path a block with neighbours takes (exastencils_amd/csrc/examg_comm.hip: examg_exchange, examg_jacobi2_blocks,
examg_rbgs_sweep_blocks, examg_residual_restrict_blocks, examg_prolong_add_blocks) on ONE GPU against the torus reference of
tests/torus_cases.py: a lone block with periodic axes is its own neighbour, so index ranges, pack / unpack, message pairing, the side
stream with its fork / join events, the thin shell launches and the box splitting all run for real, and what they must compute is
the same statement on a torus -- numpy index arithmetic and FoldOps' loops, pinned on the CPU by tests/test_torus.py, nothing of it
going through exchange index ranges.

Every comparison is bit for bit over WHOLE allocations (uint64 views): the outputs hold the reference's bits on the box and the bits
from before the call everywhere else, the right-hand side and the other inputs come back unchanged, the exchanged input differs in
its ghost layers at periodic faces only, and those hold their torus images.  Stale data cannot pass for good data: before each call
every ghost layer at a periodic face, all of the scratch arrays and the outputs are NaN (tagged with their own index where they
must survive), so a value read before its exchange or its first stage reaches the output as NaN.  Both self-transports run: direct
self-messages and, with EXAMG_COMM_SELF_RCCL=1, ncclSend / ncclRecv to self.  Which route a case took (one pass beside the shell
work, or everything in sequence) is asked of the library with the boxes the entry points form and asserted, and both routes must
occur among the cases of every entry point."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import torus_cases as TC
from torus_cases import bits

from exastencils_amd.comm import Communicator
from exastencils_amd.domain import RectDomain, shrink
from exastencils_amd.field import Field

pytestmark = pytest.mark.gpu

TRANSPORT_IDS = ["direct", "rccl-to-self"]
OUTPUT = {"jacobi2": "u_out", "rbgs": "u_out", "rr": "fc", "prolong": "uf"}


@pytest.fixture(scope="module")
def hip():
    from exastencils_amd.ops import HipOps

    return HipOps(0)


@pytest.fixture(scope="module")
def comm_cache(hip):
    """One communicator per (self-transport, dimensionality, periodic set, consistent_duplicates) for the whole module: creating an
    RCCL communicator costs more than all the calls made through it."""
    made = {}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture
def comm_for(hip, comm_cache, monkeypatch):
    def get(rccl, nd, per, consistent):
        key = (bool(rccl), nd, tuple(per), bool(consistent))
        if key not in comm_cache:
            if rccl:
                monkeypatch.setenv("EXAMG_COMM_SELF_RCCL", "1")          # read when the communicator is created
            else:
                monkeypatch.delenv("EXAMG_COMM_SELF_RCCL", raising=False)
            dom = RectDomain(nd, (1, 1, 1), 0, (1, 1, 1), periodic=per)
            comm_cache[key] = Communicator(dom, hip, concurrent_ghost_axes=True, consistent_duplicates=consistent, transport="c")
            assert comm_cache[key]._c is not None and comm_cache[key].transport == "c"
        return comm_cache[key]

    return get


def field(hip, name, layout, a):
    f = Field(name, 0, layout, hip, 1, None)
    f.slots[0] = hip.from_host(np.array(a, dtype=np.float64, copy=True))
    return f


def assert_bits(got, want, what, keep=None):
    g, w = bits(got), bits(want)
    bad = g != w
    if keep is not None:
        bad &= keep
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: %d points differ, the first at %d: %r, expected %r" % (what, int(bad.sum()), k, float(np.asarray(got).reshape(-1)[k]),
                                                                                          float(np.asarray(want).reshape(-1)[k])))


# -- examg_exchange ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rccl", [False, True], ids=TRANSPORT_IDS)
@pytest.mark.parametrize("what,one_batch", TC.MODES, ids=["all", "ghost", "dup", "ghost-one-batch"])
@pytest.mark.parametrize("nd,per", [(3, p) for p in TC.PER3] + [(2, p) for p in TC.PER2], ids=lambda v: TC.per_id(v) if isinstance(v, tuple) else None)
def test_exchange_equals_the_torus_images(hip, comm_for, nd, per, what, one_batch, rccl):
    """Node layouts (ghost 1 and 2; align 0, 2 and 16; 72x12x10 and 9x5x3 cells), cell layouts (ghost 1 and 2, with and without
    align = 2: no duplicate layer, the dup phase leaves the array alone) and the 2-D layouts, the allocation filled with its own
    linear index, compared over the whole allocation; the one-batch mode leaves the ghosts across two periodic axes unspecified, and
    only they are masked."""
    comm = comm_for(rccl, nd, per, False)
    for name, lay in TC.exchange_layouts(nd):
        a = TC.linear_index_field(lay)
        f = field(hip, "U", lay, a)
        comm.exchange(f, None, what, axis_only=one_batch)
        hip.synchronize()
        got = hip.to_host(f.data())
        keep = ~TC.unspecified(lay, per) if one_batch else None
        assert_bits(got, TC.images(lay, per, a, what, one_batch), "%s, %s" % (name, what), keep)
        if what == "dup" and lay.is_cell:
            assert_bits(got, a, "%s: a cell layout has no duplicate layer" % name)


# -- the block-face passes -------------------------------------------------------------------------------------------------------------------
def faces_of(per):
    return [(d, side) for d in range(3) if per[d] for side in (-1, 1)]


def route(hip, case, s):
    """(has an interior, the interior runs as one pass, runs beside the shell work) as the entry point decides them: the library's
    route functions on the boxes the entry points form -- begin / end moved by 1 and 2 at interior faces."""
    faces = faces_of(case.per)
    if case.kind in ("jacobi2", "rbgs"):
        b1, e1 = shrink(s.b, s.e, faces, 1)
        b2, e2 = shrink(s.b, s.e, faces, 2)
        has = all(e2[d] > b2[d] for d in range(3))
        one = has and hip.two_stage_eligible(s.lu.c_struct(), s.lf.c_struct(), s.A, b1, e1, b2, e2)
    elif case.kind == "rr":
        cb1, ce1 = shrink(s.cb, s.ce, faces, 1)
        has = all(ce1[d] > cb1[d] for d in range(3))
        one = has and hip.residual_restrict_one_pass(s.lu.c_struct(), s.lf.c_struct(), s.A, s.lcf.c_struct(), s.b, s.e, cb1, ce1)
    else:
        has = one = True          # the interpolation reads no ghost value: `overlap` alone decides
    return has, bool(one), bool(case.overlap and one)


def expected_route(case):
    """What each shape is in the list for.  72 cells in x: rows of 69 .. 73 points, coarse rows of 35 .. 37 -- the one-pass kernels,
    for the Laplacian (they decline the asymmetric stencil's entry order).  40 cells: rows too short for the two-stage kernel, the
    smoother interior falls back through tmp; the restriction (coarse rows of 19 .. 21 points) takes the small-level one-pass kernel,
    which takes any 7-point star.  4 cells across z: a single interior plane.  2 cells across z: no interior."""
    has = case.cells[2] > 2
    if case.kind in ("jacobi2", "rbgs"):
        return has, has and case.cells[0] == 72 and case.stencil == "laplace"
    if case.kind == "rr":
        return has, has and (case.cells[0] == 40 or case.stencil == "laplace")
    return True, True


def prepare(hip, comm, case, s, dev):
    """The fields of one call around the device arrays `dev`; returns the function that makes the library call."""
    S_, F_ = Field("S", 0, s.lu, hip, 1, None), Field("F", 0, s.lf, hip, 1, None)
    F_.slots[0] = dev["rhs"]
    if case.kind in ("jacobi2", "rbgs"):
        S_.slots[0] = dev["u"]
        return lambda: comm.c_pass(case.kind, S_, dev["u"], dev["u_out"], dev["tmp"], F_, s.A, s.w, case.first, s.b, s.e, axis_only=case.batch,
                                   overlap=case.overlap, tmp_planes_valid=case.tpv)
    if case.kind == "rr":
        R_, Fc_ = Field("R", 0, s.lu, hip, 1, None), Field("Fc", 0, s.lcf, hip, 1, None)
        S_.slots[0], R_.slots[0], Fc_.slots[0] = dev["u"], dev["res"], dev["fc"]
        return lambda: comm.c_residual_restrict(S_, F_, R_, s.A, Fc_, s.scale, s.b, s.e, s.cb, s.ce, axis_only=case.batch, overlap=case.overlap)
    Sc_ = Field("Sc", 0, s.lc, hip, 1, None)
    Sc_.slots[0], S_.slots[0] = dev["uc"], dev["uf"]
    return lambda: comm.c_prolong_add(Sc_, S_, s.b, s.e, overlap=case.overlap)


def host_inputs(case, s):
    inp = dict(s.inputs)
    if case.kind in ("jacobi2", "rbgs"):
        inp["tmp"] = TC.tmp_input(case, s)
    return inp


def check(hip, case, s, inp, dev):
    """The assertions of one call; tmp and res are scratch and are not compared."""
    got = {k: hip.to_host(v) for k, v in dev.items()}
    out = OUTPUT[case.kind]
    exchanged, lay = ("uc", s.lc) if case.kind == "prolong" else ("u", s.lu)
    box_lay, bb, ee = (s.lcf, s.cb, s.ce) if case.kind == "rr" else (s.lu, s.b, s.e)
    inside = TC.S.box_mask(box_lay, bb, ee)
    # the output: the torus reference on the box, the bits from before the call everywhere else
    assert_bits(got[out], s.want[out], "%s on the box" % out, inside)
    assert_bits(got[out], inp[out], "%s outside the box" % out, ~inside)
    assert np.isfinite(got[out][inside]).all()
    # the right-hand side: unchanged over the whole array
    assert_bits(got["rhs"], inp["rhs"], "rhs")
    # the exchanged input: unchanged except the ghost layers at periodic faces (and, with the duplicate part of the communicate, the
    # scrambled lower duplicate planes); those hold their images -- the faces only in the one-batch mode
    ghosts = TC.periodic_ghosts(lay, case.per)
    written = ghosts | (TC.lower_dups(lay, case.per) if case.dup else False)
    assert_bits(got[exchanged], inp[exchanged], "%s outside the exchanged layers" % exchanged, ~written)
    assert_bits(got[exchanged], s.want[exchanged], "%s after the exchange" % exchanged, TC.compare_mask(case, lay))
    assert np.isfinite(got[exchanged][ghosts & TC.compare_mask(case, lay)]).all()


def run(hip, comm_for, case, seed=0):
    s = TC.setup(case, seed)
    has, one, beside = route(hip, case, s)
    assert (has, one) == expected_route(case), "the case does not take the route it is in the list for"
    inp = host_inputs(case, s)
    dev = {k: hip.from_host(np.array(v, copy=True)) for k, v in inp.items()}
    assert prepare(hip, comm_for(case.rccl, 3, case.per, not case.dup), case, s, dev)()          # True: the library call was made
    hip.synchronize()
    check(hip, case, s, inp, dev)


def _params(kind):
    cs = TC.cases(kind)
    return pytest.mark.parametrize("case", cs, ids=[c.id for c in cs])


@_params("jacobi2")
def test_jacobi2_blocks_equals_two_steps_on_the_torus(hip, comm_for, case):
    run(hip, comm_for, case)


@_params("rbgs")
def test_rbgs_sweep_blocks_equals_a_sweep_on_the_torus(hip, comm_for, case):
    run(hip, comm_for, case)


@_params("rr")
def test_residual_restrict_blocks_equals_the_statements_on_the_torus(hip, comm_for, case):
    """The last case runs with consistent_duplicates=False and scrambled lower duplicate planes: EXAMG_EXCH_DUP restores them (the
    reference's result is that of the consistent input: tests/test_torus.py)."""
    run(hip, comm_for, case)


@_params("prolong")
def test_prolong_add_blocks_equals_the_statements_on_the_torus(hip, comm_for, case):
    run(hip, comm_for, case)


@pytest.mark.parametrize("kind", TC.KINDS)
def test_both_routes_occur(hip, kind):
    """For every entry point: cases that run one pass beside the shell work and cases that run in sequence, cases with and without an
    interior, and -- where the library chooses -- both of its answers."""
    routes = [route(hip, c, TC.setup(c)) for c in TC.cases(kind)]
    assert {r[2] for r in routes} == {True, False}
    if kind != "prolong":
        assert {r[0] for r in routes} == {True, False}
        assert {r[1] for r in routes if r[0]} == {True, False}
        # ... and the flag alone does not decide: overlap asked for, but the interior not a single pass
        assert any(c.overlap and not r[1] for c, r in zip(TC.cases(kind), routes))


@pytest.mark.parametrize("case", TC.GRAPH_CASES, ids=[c.kind for c in TC.GRAPH_CASES])
def test_a_captured_call_replays_to_the_torus_result(hip, comm_for, case):
    """The call captured into a graph after one eager call, as the cycle captures it, and replayed once on fresh inputs (direct
    self-messages: RCCL point-to-point groups are not for stream capture)."""
    torch = hip.torch
    s0, s1 = TC.setup(case, 0), TC.setup(case, 1)
    assert route(hip, case, s0) == (True, True, True)
    comm = comm_for(False, 3, case.per, True)
    inp0, inp1 = host_inputs(case, s0), host_inputs(case, s1)
    assert not np.array_equal(inp0["rhs"], inp1["rhs"])
    dev = {k: hip.from_host(np.array(v, copy=True)) for k, v in inp0.items()}
    launch = prepare(hip, comm, case, s0, dev)
    assert launch()
    hip.synchronize()
    check(hip, case, s0, inp0, dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert launch()
    for k, v in inp1.items():
        dev[k].copy_(hip.from_host(np.array(v, copy=True)))
    g.replay()
    hip.synchronize()
    check(hip, case, s1, inp1, dev)
