#!/usr/bin/env python
"""Record which kernel-layer calls the ExaSlang-4 interpreter (exastencils_amd/exa4*.py) issues for a program, in which order, on which
boxes and arrays -- the property a change of how loop statements are recognised and launched must keep, and that the interpreter tests
cannot see: they compare printed values and `launches` totals, which a pass issued twice, or a loop launched once where it stands and
once more when a pending loop is flushed, leaves alone.

The kernel layer of an `Exa4Program` is wrapped in the proxy of tools/record_choreography.py: every call that is no plumbing is logged
with its method name, integers, boxes and scalars as they are, and every array under the role `Field@level[slot]` it got right after
construction (arrays created later -- second arrays of the one-pass sweeps, scratch fields -- keep the recorder's `anonN`).  The
communicator is not wrapped: every scenario runs on one block.  Beside the calls a trace holds `launches`, `fusions` and
`printed_values` of the run.

`python tools/record_exa4_calls.py [--gpu]` writes tests/traces/exa4_cpu.json (exa4_gpu.json); tests/test_exa4_calls.py replays the
scenarios and demands the committed traces."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from record_choreography import TRACES, Recorder, plain  # noqa: E402

from exastencils_amd import exa4  # noqa: E402

EX = os.path.join(ROOT, "examples", "exa4")
FUSIONS = ("residual_restrict", "residual_norm", "zero_start", "folded_correction")
# a statement that READS the residual after the restriction: the pending residual loop must run as the statement it is
RESTRICTION = "  loop over f@coarser {\n    f@coarser = R * r\n  }\n"
LIVE_RESIDUAL = RESTRICTION + "  Var chk : Real = 0.0\n  loop over r with reduction ( + : chk ) {\n    chk += r * r\n  }\n"
# the operations of a recording kernel layer: no launch of the interpreter's, so outside the count that `launches` is compared with
GRAPH_OPS = ("graph_begin", "graph_end", "graph_replay", "graph_capturing")


def _nonlinear():
    from nonlinear_ops import NonlinearOracleOps

    return NonlinearOracleOps()


def _multicolour():
    from multicolour_cases import oracle_mc

    return oracle_mc()


def _deferring():
    from graph_ops import DeferringOps

    return DeferringOps()


def _rbgs_knobs(P):
    P.fuse_min_row, P.fused_prolong_min_points, P.fuse_residual_norm = 8, 0, True


def _all_fusions(P):
    assert all(P.fusions[k] > 0 for k in FUSIONS), "the deferred paths are not in the trace: %r" % (P.fusions,)


def _live(src):
    assert RESTRICTION in src
    return src.replace(RESTRICTION, LIVE_RESIDUAL)


def run(rec, ops, name, nd, lo, hi, setup=None, check=None, edit=None, knowledge=None, **kw):
    """Run examples/exa4/<name> on the wrapped kernel layer; the trace's entry without its calls."""
    with open(os.path.join(EX, name)) as f:
        src = f.read()
    P = exa4.Exa4Program(edit(src) if edit else src, dict(knowledge or {}, dimensionality=nd, minLevel=lo, maxLevel=hi), ops=rec.wrap(ops, "ops"), **kw)
    for (fname, lvl), F in sorted(P.fields.items()):
        for i, t in enumerate(F.slots):
            rec.name(t, "%s@%d[%d]" % (fname, lvl, i))
    if setup:
        setup(P)
    P.run()
    if check:
        check(P)
    return {"launches": P.launches, "fusions": dict(sorted(P.fusions.items())), "printed_values": list(P.printed_values)}


# name -> (kernel layer, program, nd, min level, max level, keywords of `run`); "+fuse": once with fuse=True and once with fuse=False
_PLAIN = [("jacobi3d_slots", 3, 1, 4), ("jacobi3d_contraction", 3, 1, 3), ("varcoeff3d", 3, 1, 4), ("cell2d_dirichlet", 2, 0, 4),
          ("cell3d_neumann", 3, 0, 3), ("optflow2d", 2, 0, 4), ("bratu2d_fas", 2, 1, 4), ("bratu3d_rbgs_fas", 3, 1, 3)]
# the pure Neumann problem on the one cell that level 0 of a unit fragment is has no solution the coarse solver could reach: its loop runs
# out 350 000 launches later.  As in tests/test_cell.py the fragment is 4 cells long, the coarsest grid 4^3
_KNOWLEDGE = {"cell3d_neumann": dict(domain_fragmentLength_x=4, domain_fragmentLength_y=4, domain_fragmentLength_z=4)}
CPU = {}
for _fuse in (True, False):
    _tag = "fuse" if _fuse else "plain"
    CPU["poisson3d_rbgs_" + _tag] = (_nonlinear, "poisson3d_rbgs.exa4", 3, 2, 5, dict(setup=_rbgs_knobs, check=_all_fusions if _fuse else None, fuse=_fuse))
    for _n, _nd, _lo, _hi in _PLAIN:
        CPU["%s_%s" % (_n, _tag)] = (_nonlinear, _n + ".exa4", _nd, _lo, _hi, dict(fuse=_fuse, knowledge=_KNOWLEDGE.get(_n)))
    # levels 1..2: the smallest range the program runs on (its cycle needs a coarser level)
    CPU["helmholtz3d_gs8_" + _tag] = (_multicolour, "helmholtz3d_gs8.exa4", 3, 1, 2, dict(fuse=_fuse))
CPU["poisson3d_rbgs_live_residual"] = (_nonlinear, "poisson3d_rbgs.exa4", 3, 2, 5, dict(setup=_rbgs_knobs, edit=_live, fuse=True))
CPU["poisson3d_rbgs_auto_graph"] = (_deferring, "poisson3d_rbgs.exa4", 3, 2, 4, dict(auto_graph=True))

# the HIP kernel layer has entry points the CPU layers lack (rbgs_sweep_fused_zero, rbgs_sweep_fused_prolong, mcgs_sweep, residual_norm2,
# jacobi3): the interpreter asks for them with hasattr and takes other routes there
GPU = {}
for _fuse in (True, False):
    _tag = "fuse" if _fuse else "plain"
    GPU["poisson3d_rbgs_" + _tag] = (None, "poisson3d_rbgs.exa4", 3, 2, 5, dict(setup=_rbgs_knobs, check=_all_fusions if _fuse else None, fuse=_fuse))
    GPU["jacobi3d_slots_" + _tag] = (None, "jacobi3d_slots.exa4", 3, 1, 4, dict(fuse=_fuse))
    GPU["helmholtz3d_gs8_" + _tag] = (None, "helmholtz3d_gs8.exa4", 3, 1, 2, dict(fuse=_fuse))


def record(name, hip=None):
    """(calls, the rest of the trace's entry) of one scenario; `hip`: the HIP kernel layer of the GPU scenarios."""
    make, prog, nd, lo, hi, kw = (GPU if hip is not None else CPU)[name]
    rec = Recorder()
    rest = run(rec, hip if hip is not None else make(), prog, nd, lo, hi, **kw)
    if hip is not None:
        hip.synchronize()
    return plain(rec.events), plain(rest)


def launches_logged(calls):
    """How many of the calls are launches of the interpreter's: all but the operations of a recording."""
    return sum(1 for ev in calls if ev["c"].split(".")[-1] not in GRAPH_OPS)


def path_of(kind, out=TRACES):
    return os.path.join(out, "exa4_%s.json" % kind)


def dump(traces, path):
    """{scenario: (calls, rest)} as one file: per scenario every distinct call once (`events`) and the numbers of the calls in order
    (`order`), beside launches, fusions and printed values.  `--show NAME` prints one in full."""
    out = []
    for name, (calls, rest) in traces.items():
        texts = [json.dumps(ev, sort_keys=True, separators=(",", ":")) for ev in calls]
        number = {}
        order = [number.setdefault(t, len(number)) for t in texts]
        out.append('"%s":{"events":[\n%s\n],\n"order":%s,\n"rest":%s}' % (
            name, ",\n".join(number), json.dumps(order, separators=(",", ":")), json.dumps(rest, sort_keys=True, separators=(",", ":"))))
    with open(path, "w") as f:
        f.write("{\n%s\n}\n" % ",\n".join(out))


def load(path):
    """{scenario: (calls, rest)} of a file written by `dump`."""
    with open(path) as f:
        d = json.load(f)
    return {name: ([t["events"][i] for i in t["order"]], t["rest"]) for name, t in d.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gpu", action="store_true", help="record the GPU scenarios (needs the built library and a GPU) instead of the CPU ones")
    ap.add_argument("--out", default=TRACES)
    ap.add_argument("--show", metavar="NAME", help="print the recorded trace of one scenario, a call per line, and stop")
    args = ap.parse_args()
    kind = "gpu" if args.gpu else "cpu"
    if args.show:
        calls, rest = load(path_of(kind, args.out))[args.show]
        for ev in calls:
            print(json.dumps(ev, separators=(",", ":")))
        print(json.dumps(rest))
        return
    os.makedirs(args.out, exist_ok=True)
    hip = None
    if args.gpu:
        from exastencils_amd.ops import HipOps

        hip = HipOps(0)
    got = {name: record(name, hip) for name in (GPU if args.gpu else CPU)}
    dump(got, path_of(kind, args.out))
    for name, (calls, rest) in got.items():
        print("%-40s %6d calls %6d distinct %6d launches" % (name, len(calls), len({json.dumps(e, sort_keys=True) for e in calls}), rest["launches"]))


if __name__ == "__main__":
    main()
