#!/usr/bin/env python
"""The 8-colour Gauss-Seidel sweep of a 27-entry record field against its alternatives, in one process:

  per sweep, at n^3 cells (default 512 and 256), hipEvent-timed after a settle, the three variants alternating in every round:
    (a) one sweep as eight examg_stencil_op_coloured launches       (k_stencil_coloured)
    (b) examg_mcgs_sweep on its row-pair path, four launches        (k_mcgs_rowpair27; examg_mcgs_one_pass_eligible is asserted)
    (c) one Jacobi step on the same field                           (k_stencilfield27_rec)
  solver: the 27-entry Helmholtz solve (BASELINE configs[3]'s operator as bench.py sets it up: records, pairs of Jacobi steps,
    step + residual in one pass, cycle replayed from its hipGraph) with smoother="jacobi" against smoother="mcgs": cycles to the
    tolerance and time to solution.

Writes one JSON document (default profiles/mcgs_bench.json) and prints it.  The row-pair path is worth its kernel when (b) beats (a) of
the same run at both sizes by more than the box-to-box spread of 3 %; `verdict` says so."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sweep_times(ops, n, rounds, reps):
    import torch

    from exastencils_amd.field import Colouring, Stencil, helmholtz27_offsets
    from exastencils_amd.layout import FieldLayout

    lu, lf = FieldLayout.node(3, (n, n, n), 1), FieldLayout.node(3, (n, n, n), 0)
    u, un, f = ops.new_array(lu.size), ops.new_array(lu.size), ops.new_array(lf.size)
    ops.fill_random(u, 1)
    ops.fill_random(f, 2)
    cf = ops.new_array(27 * lf.size)
    ops.fill_random(cf, 3)
    cf[:lf.size] += 30.0          # a dominant diagonal: repeated sweeps stay bounded
    rec = Stencil(helmholtz27_offsets(), [], cf, lf).entry_fastest(ops)
    del cf
    torch.cuda.empty_cache()
    Ls, Fs = lu.c_struct(), lf.c_struct()
    b, e = [1, 1, 1], [n, n, n]
    col = Colouring.axis_parity(3)
    colours = list(col.colours())
    if not ops.mcgs_one_pass_eligible(Ls, Fs, rec, col, b, e):
        raise RuntimeError("examg_mcgs_sweep does not take the row-pair kernel for this case")

    def eight():
        for c in colours:
            ops.stencil_op_coloured(2, Ls, u, Fs, f, Ls, u, rec, 0.8, c, b, e)

    cases = [("a_eight_coloured_launches_ms", eight),
             ("b_row_pair_sweep_ms", lambda: ops.mcgs_sweep(Ls, u, Fs, f, rec, 0.8, col, b, e)),
             ("c_jacobi_step_ms", lambda: ops.stencil_op(2, Ls, u, Fs, f, Ls, un, rec, 0.8, -1, b, e))]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for _ in range(3):            # settle: code objects loaded, clocks up
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k, _ in cases}
    for _ in range(rounds):
        for k, fn in cases:
            out[k].append(timed(fn))
    res = {"n": n, "points": (n - 1) ** 3, "rounds": rounds, "launches_per_timing": reps}
    for k, _ in cases:
        res[k] = statistics.median(out[k])
        res[k.replace("_ms", "_all_ms")] = [round(v, 4) for v in out[k]]
    res["b_over_a"] = res["b_row_pair_sweep_ms"] / res["a_eight_coloured_launches_ms"]
    res["b_over_c"] = res["b_row_pair_sweep_ms"] / res["c_jacobi_step_ms"]
    # compulsory traffic of a sweep: 216 B of coefficients + rhs + u read + u written per point (neighbours from cache)
    res["b_gbs_of_240B_per_point"] = 240.0 * res["points"] / res["b_row_pair_sweep_ms"] / 1e6
    return res


def solve(ops, level, smoother):
    import torch

    from exastencils_amd.solver import ConfigL3, SolverFromL3

    kw = dict(nd=3, min_level=1, max_level=level, frag_len=(2, 2, 2), stencil="helmholtz27", restrict_scale=1.0, tol=1e-8, cg_max=512, bc_fn=0,
              sol_fn=9, coef_fn=7, kappa=10.0, ksq=2.0, rhs_from_solution=True, fused_coarse=True, coef_entry_fastest=True)
    if smoother == "jacobi":
        kw.update(smoother="jacobi", omega=0.8, temporal_blocking=True, fused_smooth_residual=True)
    else:
        kw.update(smoother="mcgs", omega=1.0)
    P = SolverFromL3(ConfigL3(**kw), ops)
    P.setup()
    P.capture()
    P.Solve(use_graph=True)          # settle
    times = []
    for _ in range(3):
        P.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        its = P.Solve(use_graph=True)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    out = {"smoother": smoother, "omega": kw["omega"], "cells_per_dim": 2 << level, "cycles_to_tol": its, "tol": kw["tol"],
           "time_to_solution_ms": statistics.median(times), "time_to_solution_all_ms": [round(t, 3) for t in times],
           "residuals": P.res_history, "final_error": P.err_history[-1] if P.err_history else None}
    del P
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[512, 256])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--solve-level", type=int, default=8, help="finest level of the solver comparison (2^(level + 1) cells per dimension); 0: skip")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcgs_bench.json"))
    a = ap.parse_args()
    import torch

    from exastencils_amd.ops import HipOps

    ops = HipOps(0)
    doc = {"device": torch.cuda.get_device_name(0), "sweeps": [], "solver": []}
    for n in a.sizes:
        doc["sweeps"].append(sweep_times(ops, n, a.rounds, a.reps))
        print(json.dumps(doc["sweeps"][-1]), flush=True)
    wins = [s["b_over_a"] < 0.97 for s in doc["sweeps"]]
    doc["verdict"] = ("row-pair path beats the eight launches by more than 3 %% at %s" % ("every size" if all(wins) else
                      "some sizes" if any(wins) else "no size")) if wins else "not measured"
    if a.solve_level:
        for sm in ("jacobi", "mcgs"):
            doc["solver"].append(solve(ops, a.solve_level, sm))
            print(json.dumps(doc["solver"][-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
