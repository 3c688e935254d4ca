#!/usr/bin/env python
"""The flux-form kernels (examg_flux_step, examg_reduce_expr_cell) in one process, by the protocol of tools/axis_bench.py:

  one Lax-Friedrichs step of the shallow-water equations (tests/flux_cases.py: swe_spec -- three components, six programs, eight
  terms) on n^2 cells, n = 4096 and 1024, hipEvent-timed after a settle, the variants alternating in every round:
    march      examg_flux_step on the row-marching kernel (every program once per cell)
    gather     examg_flux_step on the one-lane-per-cell kernel (every term evaluates its program at both of its cells)
  forced through the debug library (examg_debug_flux_route); both must give the same bits (checked at every size before anything is
  timed).  The compulsory traffic is 56 B per cell: four fields read, three written.
    wave_speed the CFL reduction, max over the cells of max(|hu / h|, |hv / h|) + sqrt(g h): three fields read, 24 B per cell
  --solve: the interpreted examples/exa4/swe2d.exa4 at 256^2 on the product library (652 steps): wall time, launches per step.

Writes one JSON document (default profiles/flux_bench.json) and prints it: the median, the smallest and the largest time of every
variant and the bytes per second the compulsory traffic amounts to."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(torch, cases, rounds, reps):
    for _ in range(3):            # settle: code objects loaded, clocks up
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k, _ in cases}
    for _ in range(rounds):
        for k, fn in cases:
            out[k].append(timed(torch, fn, reps))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in out.items()}


def run_size(torch, ops, n, rounds, reps):
    import numpy as np

    import flux_cases as K
    from exastencils_amd import lib
    from exastencils_amd.flux import field_program
    from exastencils_amd.layout import FieldLayout

    lay = FieldLayout.cell(2, (n, n), 1, align=2)
    L = lay.c_struct()
    rng = np.random.default_rng(n)
    ins = [ops.from_host(a) for a in K.swe_data(rng, lay)]
    outs = [ops.new_array(lay.size) for _ in range(3)]
    spec = K.swe_spec()
    b, e = [0, 0, 0], [n, n, 1]
    fx = spec.c_struct(ops.ptr, L, ins, L, outs)      # bound once: the timed loop is the library call alone
    import ctypes as C

    def step(route):
        def fn():
            ops.L.examg_debug_flux_route(route)
            lib.check(ops.L.examg_flux_step(C.byref(fx), lib.ivec(b), lib.ivec(e), ops._stream()), "examg_flux_step")
        return fn

    prog = field_program(K.WAVE_SPEED)
    red = ops.new_scalar()
    got = []
    for route in (lib.FLUX_MARCH, lib.FLUX_GATHER):
        for t in outs:
            t.zero_()
        step(route)()
        torch.cuda.synchronize()
        got.append([t.clone() for t in outs])
    same = all(bool(torch.equal(x, y)) for x, y in zip(*got))
    t = measure(torch, [("march", step(lib.FLUX_MARCH)), ("gather", step(lib.FLUX_GATHER)),
                        ("wave_speed", lambda: ops.reduce_expr_cell(lib.REDUCE_MAX, L, ins[:3], prog, b, e, red))], rounds, reps)
    ops.L.examg_debug_flux_route(0)
    for k, v in t.items():
        v["GB_per_s"] = round(n * n * (24 if k == "wave_speed" else 56) / (v["median_ms"] * 1e-3) / 1e9, 1)
    t["march_over_gather"] = round(t["march"]["median_ms"] / t["gather"]["median_ms"], 4)
    # outside the spread of the two: the slowest march timing against the fastest gather timing
    t["march_beats_gather_outside_the_spread"] = bool(t["march"]["max_ms"] < t["gather"]["min_ms"])
    t["same_bits_march_gather"] = same
    return dict(cells=n, **t)


def run_solve(torch):
    from exastencils_amd import exa4
    from exastencils_amd.ops import HipOps

    d = os.path.join(ROOT, "examples", "exa4")
    out = {}
    for graphs in (False, True):
        P = exa4.load(os.path.join(d, "swe2d.exa4"), os.path.join(d, "swe2d.knowledge"), ops=HipOps(0), auto_graph=graphs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P.run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        steps = int([l for l in P.out if l.startswith("Total number of iterations:")][0].split()[-1])
        out["auto_graph" if graphs else "interpreted"] = {"seconds": round(dt, 3), "steps": steps, "launches": P.launches,
                                                           "launches_per_step": round(P.launches / steps, 2), "graph_replays": P.graph_replays}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 1024])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flux_bench.json"))
    a = ap.parse_args()
    import torch

    from exastencils_amd import lib
    from exastencils_amd.ops import HipOps

    ops = HipOps(0, lib.DBG_LIB_PATH)           # raises without a GPU: nothing here is measured on a CPU
    doc = {"tool": "tools/flux_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps_per_timing": a.reps,
           "bytes_per_cell": {"march": 56, "gather": 56, "wave_speed": 24},
           "sizes": [run_size(torch, ops, n, a.rounds, a.reps) for n in a.sizes]}
    if a.solve:
        doc["swe2d_256"] = run_solve(torch)
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
