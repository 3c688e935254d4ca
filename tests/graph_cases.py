"""Programs whose host state changes between two calls of a function that `auto_graph` records (exastencils_amd/exa4.py), and the
comparison every one of them must pass: the run with auto_graph=True equals the interpreted run (auto_graph=False) on the same kernel
layer, bit for bit.  Shared by the CPU tests (tests/test_exa4_graph.py: the recording stand-in of tests/graph_ops.py) and the GPU
tests (tests/test_gpu_exa4_graph.py: hipGraphs).  All programs run with minLevel = 2, maxLevel = 5."""
import os

import numpy as np

from exastencils_amd import exa4

EX = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "exa4")
LO, HI = 2, 5

GLOBALS = "Globals {\n  Var omega : Real = 0.8\n  Var nsweep : Int = 0\n}\n\n"
SMOOTHER = "u += 0.8 / diag ( A ) * ( f - A * u )"
PRINT = '    print ( "cycle", it, "residual", res )\n'


def _edit(text, *pairs):
    for old, new in pairs:
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    return text


def _rbgs():
    with open(os.path.join(EX, "poisson3d_rbgs.exa4")) as f:
        return f.read()


def _with_globals(text):
    return _edit(text, ("Function Defect@all {", GLOBALS + "Function Defect@all {"), (SMOOTHER, SMOOTHER.replace("0.8", "omega")))


def stock(tmp=None):
    return _rbgs()


def stale_global(tmp=None):
    """A: the smoother weight is a global that Application changes before every cycle."""
    return _edit(_with_globals(_rbgs()), ("    it += 1\n", "    it += 1\n    omega = 1.3 - 0.1 * it\n"))


def global_assigned_inside(tmp=None):
    """B: a function below the cycle counts its calls in a global."""
    return _edit(_with_globals(_rbgs()), ("Function Sweeps@(all but coarsest) {\n", "Function Sweeps@(all but coarsest) {\n  nsweep += 1\n"),
                 ('  stopTimer ( "solve" )', '  print ( "sweeps", nsweep )\n  stopTimer ( "solve" )'))


def branch_on_global(tmp=None):
    """C: the cycle smooths once more while a global that Application sets is even."""
    return _edit(_with_globals(_rbgs()), ("Function Cycle@(all but coarsest) {\n", "Function Cycle@(all but coarsest) {\n  if ( nsweep % 2 == 0 ) {\n    Sweeps ( )\n  }\n"),
                 ("    it += 1\n", "    it += 1\n    nsweep = it\n"))


def branch_on_global_shifted(tmp=None):
    """C': as C with nsweep = it + 1, so that the second call of Cycle -- the one that is recorded -- takes the branch without the extra
    sweeps.  (In C it takes the other: nine sweeps leave the arrays of u in exchanged roles, and a recording that does is refused
    whatever else is checked -- C alone cannot tell a frozen branch from a refused recording.)"""
    return _edit(branch_on_global(), ("    nsweep = it\n", "    nsweep = it + 1\n"))


def boundary_rewritten_once(tmp=None):
    """D: after the third cycle, and only then, a loop writes the boundary planes of u: the next cycle has to apply bc again."""
    return _edit(_rbgs(), (PRINT, PRINT + "    if ( it == 3 ) {\n      loop over u@finest only dup [0, 0, 0] {\n        u@finest = 1.0\n      }\n    }\n"))


def alternating_global(tmp=None):
    """E: the smoother weight alternates between two values, so it keeps coming back to the recorded one."""
    return _edit(_with_globals(_rbgs()), ("    it += 1\n", "    it += 1\n    if ( it % 2 == 0 ) {\n      omega = 1.0\n    } else {\n      omega = 0.8\n    }\n"))


REASSEMBLE = """Function b ( x : Real, y : Real, z : Real ) : Real {
  return 1.5 * exp ( kappa * ( ( ( x - ( x ** 2 ) ) * ( y - ( y ** 2 ) ) ) * ( z - ( z ** 2 ) ) ) )
}

Function Reassemble@finest {
  loop over coeff {
%s  }
}

"""


def coefficients_rewritten_once(tmp=None):
    """F: examples/exa4/varcoeff3d.exa4 with its coefficient field under the entry-fastest layout transformation; after the third cycle,
    and only then, the finest level's coefficient planes are rewritten (1.5 times the operator): the next loop over A has to re-lay
    them out.  At most 8 cycles (the coarse levels keep the old operator: the iteration need not converge, and need not)."""
    from test_exa4 import TRANSFORMED

    with open(os.path.join(EX, "varcoeff3d.exa4")) as f:
        text = f.read()
    entries = text[text.index("    A:[0, 0, 0] ="):text.index("  }\n}\n\nFunction Relax")]
    assert entries.count("\n") == 7
    return TRANSFORMED + _edit(text, ("Function Application {", REASSEMBLE % entries.replace(" a (", " b (") + "Function Application {"),
                               ("it >= 100", "it >= 8"),
                               ('    print ( "residual", res, "error", Error@finest ( ) )\n',
                                '    print ( "residual", res, "error", Error@finest ( ) )\n    if ( it == 3 ) {\n      Reassemble@finest ( )\n    }\n'))


def field_read_once(tmp):
    """G: after the third cycle, and only then, readField replaces u -- boundary planes included -- by the zero field written at the
    start: the next cycle has to apply bc again."""
    name = os.path.join(str(tmp), "zero.txt")
    return _edit(_rbgs(), ("  apply bc to u@finest\n  startTimer", '  writeField ( "%s", u@finest )\n  apply bc to u@finest\n  startTimer' % name),
                 (PRINT, PRINT + '    if ( it == 3 ) {\n      readField ( "%s", u@finest )\n    }\n' % name))


def program(text, ops, auto_graph):
    return exa4.Exa4Program(text, dict(dimensionality=3, minLevel=LO, maxLevel=HI), ops=ops, auto_graph=auto_graph)


def run_pair(text, ops):
    """The program replayed (auto_graph=True) and interpreted on the same kernel layer, both run to their end."""
    G, P = program(text, ops, True), program(text, ops, False)
    assert G.auto_graph and not P.auto_graph
    G.run()
    P.run()
    return G, P


def assert_same_run(G, P):
    """Printed values and lines, every array of every field on every level and slot, and the globals: equal bit for bit."""
    assert len(P.printed_values) > 4
    assert G.printed_values == P.printed_values, (G.printed_values, P.printed_values)
    assert G.out == P.out
    assert G.globals == P.globals and [type(v) for v in G.globals.values()] == [type(v) for v in P.globals.values()]
    assert sorted(G.fields) == sorted(P.fields)
    for key in sorted(P.fields):
        g, p = G.fields[key], P.fields[key]
        assert g.current_slot == p.current_slot and len(g.slots) == len(p.slots), key
        for s in range(len(p.slots)):
            a, b = G.ops.to_host(g.slots[s]), P.ops.to_host(p.slots[s])
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (key, s)
    assert P.graph_replays == 0 and not P._auto_graphs


def recorded(G):
    """{(function, level): number of replays} of the functions `G` has a recording of."""
    return {k: r["replays"] for k, r in G._auto_graphs.items() if isinstance(r, dict)}
