"""`auto_graph` of the ExaSlang-4 interpreter (exastencils_amd/exa4.py) on the CPU: a replayed function must equal its interpretation.

A recording freezes the launches the interpreter decided to issue and the scalars it had evaluated when it issued them.  The programs
of tests/graph_cases.py change, between two calls of a recorded function, what those decisions were made from -- a global the
smoother reads (A, E), a global the function itself assigns (B) or branches on (C), the boundary bookkeeping (D: `loop over .. only`,
G: readField), the coefficient planes behind an entry-fastest stencil field (F) -- on ONE iteration or on every one, and the replayed
run must leave what the interpreted run leaves, bit for bit.  The kernel layer is the recording stand-in of tests/graph_ops.py over the
CPU oracle: it defers calls the way a stream capture does (numbers by value, arrays by reference), so a stale replay computes stale
numbers here exactly as it does on the device.  The same programs run through hipGraphs in tests/test_gpu_exa4_graph.py.

F runs on `PlanesOps`: the oracle reads coefficient planes, so the "entry-fastest" copy of this layer is a copy in plane order -- the
interpreter's path (`Exa4Program.stencil`: a second array, re-laid out when `_sf_dirty` says so) is the one the HIP layer takes.

H (`Exa4Program.capture`, the explicit form) needs HIP streams: its test is in the GPU module.

The stand-in's `PlanesOps` has two traits of the HIP layer that the plain oracle layer lacks: a "transformed" copy of a stencil
field's coefficients (F), and a residual + restriction pass that never stores the residual -- so a recording that splits the pass in
two leaves another, dead, array than interpretation, which the comparison of every array sees.

Against the interpreter before the guard (recordings checked for array roles only), on this stand-in: A, B, C, C', D, E, F and G fail.
Printed values differ in A, C', E, F (B: the printed count; D and G: the stale iteration runs on until the oracle's coarse solver
divides by a norm that has underflowed).  C gives the interpreted run's printed values there too -- its recorded call of Cycle smooths
nine times, which leaves the arrays of u in exchanged roles, and such a recording was refused already -- and differs in a dead residual
array only: Defect, recorded on its own, stored what the one-pass form of interpretation never stores.  The stock program passes."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import graph_cases as gc  # noqa: E402
from graph_ops import DeferringOps, PlanesOps  # noqa: E402
from oracle_ops import OracleOps  # noqa: E402

from exastencils_amd import exa4  # noqa: E402

HI = gc.HI


def _pair(case, tmp_path=None, inner=None):
    ops = DeferringOps(inner)
    G, P = gc.run_pair(case(tmp_path), ops)
    gc.assert_same_run(G, P)
    return G, P, ops


def test_stock_program_still_records_the_cycle_and_replays_it_from_the_third_call_on():
    """The guard must not work by turning the feature off: the unmodified red-black program records Cycle@finest at the second call and
    replays it on every later one; Norm returns to the host and is never recorded, Defect leaves its loop pending for its caller's next
    statement (a one-pass form may take both) and is interpreted."""
    G, P, ops = _pair(gc.stock)
    cycles = len(G.printed_values) - 1
    assert cycles >= 5
    assert gc.recorded(G) == {("Cycle", HI): cycles - 1}
    assert G._auto_graphs[("Defect", HI)] is False
    assert ("Norm", HI) not in G._auto_graphs
    assert G.graph_replays >= len(G.printed_values) - 2
    assert abs(G.launches - P.launches) <= len(G.printed_values)
    assert ops.replays == G.graph_replays


def test_stand_in_defers_by_value_and_refuses_host_reads():
    """The stand-in itself: a recorded call runs at replay, with the number it was given and the array as it is then; reading a value
    back while recording raises."""
    from exastencils_amd.domain import RectDomain
    from exastencils_amd.layout import FieldLayout

    ops = DeferringOps()
    lay = FieldLayout.node(3, RectDomain(3, (1, 1, 1), 0).ncells(2), 0)          # 5 x 5 x 5 points, no ghost layers
    x, begin, end = ops.new_array(lay.size), [0, 0, 0], [5, 5, 5]
    rec = ops.graph_begin()
    assert ops.graph_capturing()
    ops.set(lay.c_struct(), x, 2.0, begin, end)
    end[0] = 1               # the caller's list changes after the call: the recording keeps the box it was given
    with pytest.raises(RuntimeError):
        ops.to_host(x)
    with pytest.raises(RuntimeError):
        ops.scalar_value(x[:1])
    ops.graph_end(rec)
    assert not ops.graph_capturing() and int((x != 0.0).sum()) == 0          # nothing ran
    x += 1.0                 # ... and the array is the one of replay time
    ops.graph_replay(rec)
    assert int((x == 2.0).sum()) == 125 and int((x == 1.0).sum()) == x.numel() - 125
    assert not hasattr(ops, "no_such_kernel") and hasattr(ops, "rbgs_sweep_fused_zero")


def test_a_global_changed_between_calls_is_not_stale_in_a_replay():
    """A: omega = 1.3 - 0.1 * it before every cycle.  Cycle is recorded (second call: one replay) and never meets that guard again."""
    G, P, _ = _pair(gc.stale_global)
    assert round(P.printed_values[1], 1) == 327.8           # (the stock program: 2944.98)
    assert gc.recorded(G) == {("Cycle", HI): 1} and G.graph_replays == 1


def test_a_function_that_assigns_a_global_is_never_recorded():
    """B: Sweeps counts its calls in a global.  A replay would not count: Sweeps, and Cycle above it, are not recordable (decided
    from the text: nothing of them is in _auto_graphs, not even a refusal).  The correct handling of this program is to record NOTHING:
    the one other candidate, Defect, leaves its loop pending for the caller's next statement and is interpreted for that reason."""
    G, P, _ = _pair(gc.global_assigned_inside)
    assert P.out[-1] == "sweeps 36" and G.globals["nsweep"] == 36
    assert not any(k[0] in ("Cycle", "Sweeps") for k in G._auto_graphs)
    assert not G._is_host_free("Cycle", HI) and not G._is_host_free("Sweeps", HI) and G._is_host_free("Defect", HI)
    assert gc.recorded(G) == {} and G.graph_replays == 0


def test_a_branch_on_a_global_is_not_frozen():
    """C: Cycle smooths once more while nsweep, which Application sets to the iteration count, is even.  The correct handling of this
    program is to record NOTHING: the second call of Cycle, the one that would be recorded, smooths nine times, which leaves the arrays
    of u in exchanged roles, and a recording that does is refused (before the guard too: C' below is the program that tells a frozen
    branch from a refused recording); Sweeps changes the roles, Defect leaves its loop pending."""
    G, P, _ = _pair(gc.branch_on_global)
    assert round(P.printed_values[2], 1) == 121.8
    assert gc.recorded(G) == {} and G.graph_replays == 0 and G._auto_graphs[("Cycle", HI)] is False


def test_a_branch_on_a_global_is_not_frozen_when_the_recorded_branch_keeps_the_roles():
    """C': nsweep = it + 1.  The recorded call (second: nsweep 3) smooths six times and leaves every array in its role, so Cycle IS
    recorded -- and every later call meets another nsweep: interpreted, with the branch of its own."""
    G, P, _ = _pair(gc.branch_on_global_shifted)
    assert gc.recorded(G)[("Cycle", HI)] == 1 and G._auto_graphs[("Cycle", HI)]["guard"][1] == ((int, 3), (float, 0.8))          # nsweep, omega


def test_boundary_planes_rewritten_once_are_applied_again():
    """D: `loop over u@finest only dup ..` after the third cycle only.  The fourth call of Cycle meets bookkeeping the recording was
    not made under (u's planes no longer valid) and is interpreted, boundary values and all; the fifth meets the state the program then
    stays in, the sixth meets it again and is recorded anew: replays from there on."""
    G, P, ops = _pair(gc.boundary_rewritten_once)
    cycles = len(G.printed_values) - 1
    assert cycles == 10 and P.printed_values[4] > 100 * P.printed_values[3]          # the residual jumps after iteration 3
    assert gc.recorded(G)[("Cycle", HI)] == cycles - 1 - 2                              # all but the first and the two interpreted after the change
    assert G._auto_graphs[("Cycle", HI)]["guard"][3] == {("u", HI): 1}                   # recorded under the new boundary epoch


def test_a_global_that_returns_to_its_recorded_value_replays_again():
    """E: omega is 1.0 on even iterations, 0.8 on odd ones.  Cycle is recorded on the second call (1.0); the ONE recording is reused on
    every even iteration and the odd ones are interpreted (two calls in a row never meet the same other guard: no re-recording)."""
    G, P, ops = _pair(gc.alternating_global)
    cycles = len(G.printed_values) - 1
    assert gc.recorded(G)[("Cycle", HI)] == cycles // 2
    assert G._auto_graphs[("Cycle", HI)]["guard"][1] == ((float, 1.0),)


def test_rewritten_coefficient_planes_are_laid_out_again():
    """F: the finest level's coefficient planes are rewritten after the third cycle only.  The fourth call of Cycle meets a stencil
    field whose entry-fastest copy is out of date, which the recording was not made under: interpreted, re-layout included."""
    G, P, ops = _pair(gc.coefficients_rewritten_once, inner=PlanesOps())
    assert G._sf_rec and ("A", HI) in G._sf_rec and not any(G._sf_dirty.values())
    assert gc.recorded(G)[("Cycle", HI)] >= 3 and P.out[-1] == "8"
    plain = gc.program(gc.coefficients_rewritten_once().replace("it == 3", "it == 300"), DeferringOps(PlanesOps()), False)
    plain.run()
    assert plain.printed_values[:7] == P.printed_values[:7] and plain.printed_values[7:9] != P.printed_values[7:9]      # the rewrite matters


def test_a_field_read_from_a_file_gets_its_boundary_values_again(tmp_path):
    """G: readField replaces u@finest, boundary planes included, after the third cycle only (exa4_builtins.py: the entry leaves
    _bc_valid, the boundary epoch advances).  As D."""
    G, P, ops = _pair(gc.field_read_once, tmp_path)
    assert P.printed_values[4] > 100 * P.printed_values[3]
    assert gc.recorded(G)[("Cycle", HI)] == len(G.printed_values) - 1 - 1 - 2


# -- the decision itself ------------------------------------------------------------------------------------------------------------

DECISION = """
Domain global< [0.0, 0.0, 0.0] to [1.0, 1.0, 1.0] >
Layout L< Real, Node >@all {
  duplicateLayers = [1, 1, 1]
  ghostLayers = [1, 1, 1]
}
Field u< global, L, 0.0 >@all
Field v< global, L, None >@all
Globals {
  Var w : Real = 0.5
  Var n : Int = 0
  Var unused : Real = 1.0
}
Function ReadsW@all {
  loop over v {
    v += w * u
  }
}
Function Deep@all {
  ReadsW ( )
}
Function Counts@all {
  n += 1
}
Function F@all {
%s
}
Function Application {
}
"""

LOOP = "  loop over v {\n    v = 2.0 * u\n  }\n"
# (body of F, recordable, globals a recording depends on)
BODIES = [
    ("reads a global", "  loop over v {\n    v = w * u\n  }\n", True, ("w",)),
    ("assigns a global", "  n = 3\n" + LOOP, False, None),
    ("adds to a global", "  n += 1\n" + LOOP, False, None),
    ("assigns a local of its own", "  Var k : Int = 1\n  k += n\n" + LOOP, True, ("n",)),
    ("if on a global", "  if ( n % 2 == 0 ) {\n" + LOOP + "  }\n", True, ("n",)),
    ("if on a literal", "  if ( 1 < 2 ) {\n" + LOOP + "  }\n", True, ()),
    ("only loops with literal scalars", LOOP + "  apply bc to u\n", True, ()),
    ("calls a function that reads a global", "  ReadsW ( )\n", True, ("w",)),
    ("calls a function that calls one that reads a global", LOOP + "  Deep ( )\n", True, ("w",)),
    ("calls a function that assigns a global", LOOP + "  Counts ( )\n", False, None),
    ("a reduction returns to the host", "  Var s : Real = 0.0\n  loop over u with reduction ( + : s ) {\n    s += u * u\n  }\n", False, None),
    ("a print returns to the host", LOOP + '  print ( "x" )\n', False, None),
]


@pytest.mark.parametrize("what,body,recordable,reads", BODIES, ids=[b[0] for b in BODIES])
def test_what_is_recordable_and_what_a_recording_depends_on(what, body, recordable, reads):
    """The decision, from the program text alone: a function is recordable if nothing below it returns to the host or assigns a global;
    a recording depends on the globals named anywhere below it (through calls too), and on no other."""
    P = exa4.Exa4Program(DECISION % body.rstrip("\n"), dict(dimensionality=3, minLevel=1, maxLevel=2), ops=DeferringOps(), auto_graph=True)
    assert P.auto_graph
    assert P._graph_deps("F", 2) == reads
    assert P._is_host_free("F", 2) == recordable
    if not recordable:
        return
    # the guard: a host function of the globals read and of the interpreter's bookkeeping
    g0 = P._graph_guard(("F", 2))
    assert g0 == P._graph_guard(("F", 2))
    P.globals["unused"] = 2.0
    assert P._graph_guard(("F", 2)) == g0
    for name in reads:
        saved = P.globals[name]
        P.globals[name] = saved + 1
        assert P._graph_guard(("F", 2)) != g0, name
        P.globals[name] = saved
        assert P._graph_guard(("F", 2)) == g0, name
    if "n" in reads:
        P.globals["n"] = 0.0          # 0 and 0.0 are equal and divide differently: another guard
        assert P._graph_guard(("F", 2)) != g0


@pytest.mark.parametrize("change", ["bc_valid", "bc_epoch", "alt_shell", "sf_dirty", "sf_clean", "pair_tmp", "slot", "switch", "site"])
def test_guard_sees_the_bookkeeping(change):
    """Every piece of host state a launch decision reads is in the guard (exa4.py: _apply_bc, stencil; exa4_peepholes.py: _try_fused_sweep,
    _try_jacobi_pairs, _contract_pair_plan; exa4_fusion.py: _try_defer, _dead_after) -- and a stencil field marked clean is no change."""
    P = exa4.Exa4Program(DECISION % LOOP.rstrip("\n"), dict(dimensionality=3, minLevel=1, maxLevel=2), ops=DeferringOps(), auto_graph=True)
    assert P._is_host_free("F", 2)
    g0 = P._graph_guard(("F", 2))
    if change == "bc_valid":
        P._bc_valid.add(("u", 2, 0))
    elif change == "bc_epoch":
        P._bc_epoch[("u", 2)] = 1
    elif change == "alt_shell":
        P._alt_shell[("u", 2, 0)] = 0
    elif change == "sf_dirty":
        P._sf_dirty[("A", 2)] = True
    elif change == "sf_clean":
        P._sf_dirty[("A", 2)] = False
    elif change == "pair_tmp":
        P._pair_tmp[("u", 2)] = P.fields[("u", 2)]
    elif change == "slot":
        P.fields[("v", 2)].slots[0] = P.ops.new_array(P.fields[("v", 2)].layout.size)
    elif change == "switch":
        P.fused_prolong_min_points = 0
    elif change == "site":
        P._cont.append([P.functions["Application"][0].body, 0, None, False, True])
    assert (P._graph_guard(("F", 2)) == g0) == (change == "sf_clean")


def test_auto_graph_needs_a_kernel_layer_that_records():
    """`auto_graph=True` on a kernel layer without the graph operations stays off (nothing to record with): no error, interpretation."""
    P = gc.program(gc.stock(), OracleOps(), True)
    assert not P.auto_graph
    assert gc.program(gc.stock(), DeferringOps(), None).auto_graph is False      # the default is on for the HIP layer only
