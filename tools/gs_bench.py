#!/usr/bin/env python
"""The lexicographic Gauss-Seidel sweep (examg_gs_sweep) against its alternatives, in one process, on the debug library (the product's
kernels plus the hook that forces a route):

  per sweep -- 7-point constant stencil at 512^3 and 256^3 cells, 27-entry stencil field (planes) at 64^3 .. 256^3 -- hipEvent-timed after a
  settle, the variants alternating in every round:
    (a) one gs_sweep on the tiled route                              (k_gs_tile, one launch per tile hyperplane)
    (b) the same sweep as one launch per point hyperplane            (k_gs_planes: the simplest correct schedule)
    (c) one red-black sweep, two examg_rbgs_colour loops in place
    (d) one Jacobi step
  with the launches per sweep of (a) and (b);
  small boxes, n^3 cells for n in 8 .. 64: the one-workgroup route against the tiled one, for the 7-point and a constant 27-point
  stencil -- the size bound of the one-workgroup route (GS_ONE_WG_MAX in csrc/kernels_gs.hip) is read off this table;
  solver: ConfigL3(smoother="gs") against smoother="rbgs" (plain colour loops), unit 7-point stencil, finest levels 4 .. 9, the cycle
  replayed from its hipGraph: cycles to the tolerance and time to solution.

Writes one JSON document (default profiles/gs_bench.json) and prints it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ONE_WG, TILED, PLANES = 1, 2, 3


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(torch, cases, rounds):
    """cases: (key, fn, reps).  Median of `rounds` timings each, the cases alternating."""
    for _ in range(2):            # settle: code objects loaded, clocks up
        for _, fn, _ in cases:
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k, _, _ in cases}
    for _ in range(rounds):
        for k, fn, reps in cases:
            out[k].append(timed(torch, fn, reps))
    res = {}
    for k, _, _ in cases:
        res[k] = statistics.median(out[k])
        res[k.replace("_ms", "_all_ms")] = [round(v, 4) for v in out[k]]
    return res


def stencil_for(ops, kind, lf):
    from exastencils_amd.field import Stencil, helmholtz27_offsets, laplace_unit

    if kind == "const7":
        return laplace_unit(3), 0.8 / 6.0
    offs = helmholtz27_offsets()
    if kind == "const27":
        return Stencil(offs, [26.0 * 1.1] + [-1.0 - 0.01 * k for k in range(26)]), 0.8 / 28.6
    cf = ops.new_array(27 * lf.size)
    ops.fill_random(cf, 3)
    cf[:lf.size] += 30.0          # a dominant diagonal: repeated sweeps stay bounded
    return Stencil(offs, [], cf, lf), 0.8


def forced(ops, route, fn):
    def run():
        old = ops.L.examg_debug_gs_route(route)
        try:
            fn()
        finally:
            ops.L.examg_debug_gs_route(old)
    return run


def launches(ops, route, Ls, Fs, st, b, e):
    from exastencils_amd.lib import ivec

    sc = st.c_struct(ops.ptr)
    old = ops.L.examg_debug_gs_route(route)
    try:
        return int(ops.L.examg_debug_gs_launches(C.byref(Ls), C.byref(Fs), C.byref(sc), ivec(b), ivec(e)))
    finally:
        ops.L.examg_debug_gs_route(old)


def sweep_times(ops, n, kind, rounds, reps):
    import torch

    from exastencils_amd.layout import FieldLayout

    lu, lf = FieldLayout.node(3, (n, n, n), 1), FieldLayout.node(3, (n, n, n), 0)
    u, un, f = ops.new_array(lu.size), ops.new_array(lu.size), ops.new_array(lf.size)
    ops.fill_random(u, 1)
    ops.fill_random(f, 2)
    st, w = stencil_for(ops, kind, lf)
    Ls, Fs = lu.c_struct(), lf.c_struct()
    b, e = [1, 1, 1], [n, n, n]
    gs = lambda: ops.gs_sweep(Ls, u, Fs, f, st, w, b, e)      # noqa: E731

    def red_black():
        for c in (0, 1):
            ops.stencil_op(2, Ls, u, Fs, f, Ls, u, st, w, c, b, e)

    cases = [("a_gs_tiled_ms", forced(ops, TILED, gs), reps), ("b_gs_per_hyperplane_ms", forced(ops, PLANES, gs), max(1, reps // 5)),
             ("d_jacobi_step_ms", lambda: ops.stencil_op(2, Ls, u, Fs, f, Ls, un, st, w, -1, b, e), reps)]
    if kind != "field27":         # the parity colouring does not decouple a 27-point stencil: no red-black sweep to compare with
        cases.insert(2, ("c_red_black_sweep_ms", red_black, reps))
    res = {"n": n, "stencil": kind, "points": (n - 1) ** 3, "rounds": rounds, "sweeps_per_timing": reps,
           "a_launches_per_sweep": launches(ops, TILED, Ls, Fs, st, b, e), "b_launches_per_sweep": launches(ops, PLANES, Ls, Fs, st, b, e)}
    res.update(measure(torch, cases, rounds))
    res["a_over_b"] = res["a_gs_tiled_ms"] / res["b_gs_per_hyperplane_ms"]
    if "c_red_black_sweep_ms" in res:
        res["a_over_c"] = res["a_gs_tiled_ms"] / res["c_red_black_sweep_ms"]
    res["a_over_d"] = res["a_gs_tiled_ms"] / res["d_jacobi_step_ms"]
    res["a_us_per_launch"] = 1e3 * res["a_gs_tiled_ms"] / res["a_launches_per_sweep"]
    res["b_us_per_launch"] = 1e3 * res["b_gs_per_hyperplane_ms"] / res["b_launches_per_sweep"]
    del u, un, f, st
    torch.cuda.empty_cache()
    return res


def small_times(ops, n, kind, rounds, reps):
    import torch

    from exastencils_amd.layout import FieldLayout

    lu, lf = FieldLayout.node(3, (n, n, n), 1), FieldLayout.node(3, (n, n, n), 0)
    u, f = ops.new_array(lu.size), ops.new_array(lf.size)
    ops.fill_random(u, 1)
    ops.fill_random(f, 2)
    st, w = stencil_for(ops, kind, lf)
    Ls, Fs = lu.c_struct(), lf.c_struct()
    b, e = [1, 1, 1], [n, n, n]
    gs = lambda: ops.gs_sweep(Ls, u, Fs, f, st, w, b, e)      # noqa: E731
    res = {"n": n, "stencil": kind, "points": (n - 1) ** 3, "tiled_launches": launches(ops, TILED, Ls, Fs, st, b, e)}
    res.update(measure(torch, [("one_workgroup_ms", forced(ops, ONE_WG, gs), reps), ("tiled_ms", forced(ops, TILED, gs), reps)], rounds))
    res["one_workgroup_over_tiled"] = res["one_workgroup_ms"] / res["tiled_ms"]
    return res


def solve(ops, level, smoother):
    import torch

    from exastencils_amd.solver import ConfigL3, SolverFromL3

    P = SolverFromL3(ConfigL3(nd=3, min_level=2, max_level=level, smoother=smoother, tol=1e-8, fused_coarse=True), ops)
    P.setup()
    P.capture()
    P.Solve(use_graph=True)          # settle
    times = []
    for _ in range(3):
        P.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P.Solve(use_graph=True)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    out = {"smoother": smoother, "level": level, "cells_per_dim": 1 << level, "cycles_to_tol": P.iterations, "tol": 1e-8,
           "time_to_solution_ms": statistics.median(times), "time_to_solution_all_ms": [round(t, 3) for t in times],
           "last_reduction": P.res_history[-1] / P.res_history[-2]}
    del P
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", type=int, nargs="*", default=[8, 12, 16, 24, 32, 48, 64])
    ap.add_argument("--levels", type=int, nargs="*", default=[4, 5, 6, 7, 8, 9])
    ap.add_argument("--sweeps", nargs="*", default=["256:const7", "512:const7", "64:field27", "128:field27", "256:field27"], help="large sweeps as cells:stencil (const7 | const27 | field27)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gs_bench.json"))
    a = ap.parse_args()
    import torch

    from exastencils_amd import lib
    from exastencils_amd.ops import HipOps

    ops = HipOps(0, lib.DBG_LIB_PATH)
    doc = {"device": torch.cuda.get_device_name(0), "sweeps": [], "small": [], "solver": []}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    for n in a.small:
        for kind in ("const7", "const27"):
            doc["small"].append(small_times(ops, n, kind, a.rounds, a.reps))
            print(json.dumps(doc["small"][-1]), flush=True)
    save()
    for item in a.sweeps:
        n, kind = item.split(":")
        doc["sweeps"].append(sweep_times(ops, int(n), kind, a.rounds, a.reps))
        print(json.dumps(doc["sweeps"][-1]), flush=True)
        save()
    for level in a.levels:
        for sm in ("gs", "rbgs"):
            doc["solver"].append(solve(ops, level, sm))
            print(json.dumps(doc["solver"][-1]), flush=True)
        save()
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
