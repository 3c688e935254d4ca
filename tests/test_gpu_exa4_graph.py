"""`auto_graph` of the ExaSlang-4 interpreter on the MI355X: a function replayed from a hipGraph must equal its interpretation.

The programs of tests/graph_cases.py (what each changes between two calls of a recorded function is said there and in
tests/test_exa4_graph.py, which runs them on the CPU stand-in) on the HIP kernel layer, minLevel 2, maxLevel 5: the run with
auto_graph=True against the run with auto_graph=False, printed values, printed lines, every array of every field and the globals
bit for bit, and what was recorded and replayed.  Then the explicit form, `Exa4Program.capture` (H), which checks nothing at a replay:
its docstring's condition -- nothing the recorded call was decided from has changed -- is the only one, a global the function reads
may be there as long as it keeps its value."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from exastencils_amd.ops import HipOps

    return HipOps(0)


def _stock(G, P, cyc, rec):
    # the guard does not work by turning the feature off: recorded at the second call, replayed on every later one
    assert rec == {("Cycle", 5): cyc - 1} and ("Norm", 5) not in G._auto_graphs
    assert G.graph_replays >= len(G.printed_values) - 2 and abs(G.launches - P.launches) <= len(G.printed_values)


def _assigned(G, P, cyc, rec):
    # NEVER RECORD: a replay of Sweeps, or of Cycle above it, would not count the calls (decided from the text, so there is not even a
    # refused recording), and Defect leaves its loop pending for its caller's next statement
    assert P.out[-1] == "sweeps 36" and not any(k[0] in ("Cycle", "Sweeps") for k in G._auto_graphs) and rec == {} and G.graph_replays == 0


CASES = {
    "stock": _stock,
    # A: Cycle recorded at the second call, every later call under another omega
    "stale_global": lambda G, P, cyc, rec: rec == {("Cycle", 5): 1},
    "global_assigned_inside": _assigned,
    # C: NEVER RECORD -- the call of Cycle that would be recorded smooths nine times: arrays in exchanged roles, refused; C' records
    "branch_on_global": lambda G, P, cyc, rec: rec == {} and G.graph_replays == 0 and G._auto_graphs[("Cycle", 5)] is False,
    "branch_on_global_shifted": lambda G, P, cyc, rec: rec[("Cycle", 5)] == 1,
    # D, G: interpreted twice after the change (the state after it, then the state the program stays in), recorded anew at the third
    "boundary_rewritten_once": lambda G, P, cyc, rec: cyc == 10 and rec[("Cycle", 5)] == cyc - 3 and P.printed_values[4] > 100 * P.printed_values[3],
    # E: the one recording (omega 1.0, second call) reused on every even iteration
    "alternating_global": lambda G, P, cyc, rec: rec[("Cycle", 5)] == cyc // 2,
    # F: the entry-fastest copy of A@finest re-laid out by the interpreted fourth call (8 cycles, two values printed per cycle)
    "coefficients_rewritten_once": lambda G, P, cyc, rec: P.out[-1] == "8" and rec[("Cycle", 5)] >= 3 and G._sf_rec[("A", 5)].ctransform == 1,
    "field_read_once": lambda G, P, cyc, rec: rec[("Cycle", 5)] == cyc - 3 and P.printed_values[4] > 100 * P.printed_values[3],
}


@pytest.mark.parametrize("case", list(CASES))
def test_replayed_run_equals_interpreted_run(hip, case, tmp_path):
    import graph_cases as gc

    G, P = gc.run_pair(getattr(gc, case)(tmp_path), hip)
    rec = gc.recorded(G)
    print(case, "printed", G.printed_values, "interpreted", P.printed_values, "recorded", rec, "replays", G.graph_replays)
    gc.assert_same_run(G, P)
    assert (bool(rec) and G.graph_replays > 0) or case in ("global_assigned_inside", "branch_on_global")
    cycles = len([l for l in P.out if l.startswith(("cycle", "residual"))]) - (case == "coefficients_rewritten_once")
    assert CASES[case](G, P, cycles, rec) is not False


def test_captured_cycle_with_a_constant_global_replays_like_direct_calls(hip):
    """H: `capture()` records the scalars of the call, so the caller re-captures after changing a global -- and only then: with omega a
    global that keeps its value, replays of the captured Cycle@finest reproduce direct calls bit for bit (the program of
    test_captured_cycle_replays_like_direct_calls with the smoother weight in a global)."""
    import numpy as np

    import graph_cases as gc

    def residuals(use_graph):
        P = gc.program(gc._with_globals(gc.stock()), hip, False)
        assert "omega" in P.globals and not P.auto_graph
        P._apply_bc(P.fields[("u", 5)], 0)
        out = []
        if use_graph:
            g = P.capture("Cycle", 5)           # two cycles have run when this returns (recording executes nothing)
        else:
            for _ in range(2):
                P.call("Cycle", 5)
        for _ in range(3):
            g.replay() if use_graph else P.call("Cycle", 5)
            P.call("Defect", 5)
            out.append(P.call("Norm", 5))
        return out, hip.to_host(P.fields[("u", 5)].data()).copy()

    (a, ua), (b, ub) = residuals(False), residuals(True)
    assert a == b and np.array_equal(ua.view(np.uint64), ub.view(np.uint64))
    assert a[2] < 2e-2 * a[0]
