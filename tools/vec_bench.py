#!/usr/bin/env python
"""The kernels of vector-valued cell fields (examg_vec_op, examg_vec_smooth) on the optical-flow operator, against the coupled-system
kernels (examg_sys_op, examg_sys_relax) on the SAME arrays, in one process:

  n = 2 components on cells^2 cells (default 4096), n = 3 components on cells^3 cells (default 256); the operator is the Laplacian
  on every component plus a symmetric point-wise n x n matrix of coefficient fields (the off-diagonal fields aliased, as IxIy is).
  The vector field is one array of n planes; the system entry points get the planes as their n unknowns.  hipEvent-timed after a
  settle, the variants alternating in every round:
    vec_residual / sys_residual   f - M u, all rows in one launch (reads n unknowns, n right-hand sides and n (n + 1) / 2 coefficient
                                  fields, writes n residuals: 8 * (3 n + n (n + 1) / 2) compulsory bytes per cell)
    vec_smooth / sys_relax        one colour, relax 1.0, in place (the same traffic per UPDATED cell, half of the cells; the two
                                  smoothers are different formulas over the same bytes: include/examg.h)

Writes one JSON document (default profiles/vec_bench.json) and prints it: the median, the smallest and the largest time of every
variant, the bytes per second that the compulsory bytes amount to, and vec / sys.

  interpreted_cycle: one `Cycle@finest` of examples/exa4/optflow{2,3}d_vec.exa4 (one vector field) against the same call of the
  scalar-component program optflow{2,3}d.exa4, both statement by statement (no one-pass fusions, no graph replay: what the vector
  program runs with), after each program has run to its end: kernel-layer launches of the call and its wall time, host included,
  median of the same alternating rounds; `scalar_graph` is the scalar program with its defaults (fusions and graph replay where they engage: a cycle with host reductions is not replayed), for scale."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SYS_RESIDUAL = 1


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


def run_size(torch, ops, nd, cells, rounds, reps):
    from exastencils_amd.field import MatrixStencil, Stencil
    from exastencils_amd.layout import FieldLayout

    n = nd
    lu, lo = FieldLayout.cell(nd, (cells,) * nd, 1, align=2), FieldLayout.cell(nd, (cells,) * nd, 0, align=2)
    h = 1.0 / cells
    offs = [(0, 0, 0)] + [tuple((s if t == d else 0) for t in range(3)) for d in range(nd) for s in (-1, 1)]
    L = Stencil(offs, [2.0 * nd / (h * h)] + [-1.0 / (h * h)] * (2 * nd))
    u, f, r = ops.new_array(n * lu.size), ops.new_array(n * lo.size), ops.new_array(n * lo.size)
    ops.fill_random(u, 500)
    ops.fill_random(f, 501)
    g = [[None] * n for _ in range(n)]
    for c in range(n):
        for d in range(c, n):
            g[c][d] = g[d][c] = ops.new_array(lo.size)
            ops.fill_random(g[c][d], 510 + c * n + d)
    elems = []
    for k, o in enumerate(offs):
        m = [[None] * n for _ in range(n)]
        for c in range(n):
            if k == 0:
                for d in range(n):
                    m[c][d] = (L.coefs[0] if c == d else None, g[c][d])
            else:
                m[c][c] = (L.coefs[k], None)
        elems.append(m)
    M = MatrixStencil(n, offs, elems, lo)
    L_u, L_o = lu.c_struct(), lo.c_struct()
    b, e = [0, 0, 0], [cells if t < nd else 1 for t in range(3)]
    planes = lambda x, l: [x[c * l.size:(c + 1) * l.size] for c in range(n)]
    us, fs, rs = planes(u, lu), planes(f, lo), planes(r, lo)
    points = cells ** nd
    per_cell = 8 * (3 * n + n * (n + 1) // 2)

    cases = [("vec_residual", lambda: ops.vec_op(SYS_RESIDUAL, n, L_u, u, L_o, f, L_o, r, M, b, e)),
             ("sys_residual", lambda: ops.sys_op(SYS_RESIDUAL, L_u, us, L_o, fs, L_o, g, L_o, rs, L, (1 << n) - 1, b, e)),
             ("vec_smooth", lambda: ops.vec_smooth(n, L_u, u, L_o, f, M, 1.0, 0, b, e)),
             ("sys_relax", lambda: ops.sys_relax(L_u, us, L_o, fs, L_o, g, L, 1.0, 0, b, e))]
    u0 = u.clone()
    t = measure(torch, cases, rounds, reps)
    u.copy_(u0)                   # (the smoothers ran in place, again and again)
    for k in ("vec_residual", "sys_residual"):
        t[k]["GB_per_s"] = round(points * per_cell / (t[k]["median_ms"] * 1e-3) / 1e9, 1)
    for k in ("vec_smooth", "sys_relax"):
        t[k]["GB_per_s"] = round(points // 2 * per_cell / (t[k]["median_ms"] * 1e-3) / 1e9, 1)
    t["vec_residual_over_sys_residual"] = round(t["vec_residual"]["median_ms"] / t["sys_residual"]["median_ms"], 4)
    t["vec_smooth_over_sys_relax"] = round(t["vec_smooth"]["median_ms"] / t["sys_relax"]["median_ms"], 4)
    return dict({"nd": nd, "n": n, "cells": cells, "points": points, "compulsory_bytes_per_cell": per_cell}, **t)


def interpreted_cycle(torch, nd, hi, rounds):
    import time

    from exastencils_amd import exa4

    def load(name, **kw):
        with open(os.path.join(ROOT, "examples", "exa4", name)) as f:
            P = exa4.Exa4Program(f.read(), dict(dimensionality=nd, minLevel=2, maxLevel=hi), **kw)
        P.run()
        return P

    progs = [("vector", load("optflow%dd_vec.exa4" % nd)), ("scalar", load("optflow%dd.exa4" % nd, fuse=False, auto_graph=False)),
             ("scalar_graph", load("optflow%dd.exa4" % nd))]
    out = {}
    for k, P in progs:
        n0 = P.launches
        P.call("Cycle", hi)
        torch.cuda.synchronize()
        out[k] = {"launches": P.launches - n0, "ms": []}
    for _ in range(rounds):
        for k, P in progs:
            torch.cuda.synchronize()
            t = time.perf_counter()
            P.call("Cycle", hi)
            torch.cuda.synchronize()
            out[k]["ms"].append((time.perf_counter() - t) * 1e3)
    for k in out:
        v = out[k].pop("ms")
        out[k].update({"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)})
    out["vector_over_scalar_launches"] = round(out["vector"]["launches"] / out["scalar"]["launches"], 4)
    out["vector_over_scalar_time"] = round(out["vector"]["median_ms"] / out["scalar"]["median_ms"], 4)
    return dict({"nd": nd, "levels": [2, hi]}, **out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes2d", type=int, nargs="*", default=[4096])
    ap.add_argument("--sizes3d", type=int, nargs="*", default=[256])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vec_bench.json"))
    a = ap.parse_args()
    import torch

    from exastencils_amd.ops import HipOps

    ops = HipOps(0)           # raises without a GPU: nothing here is measured on a CPU
    doc = {"tool": "tools/vec_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps_per_timing": a.reps,
           "sizes": [run_size(torch, ops, 2, c, a.rounds, a.reps) for c in a.sizes2d] + [run_size(torch, ops, 3, c, a.rounds, a.reps) for c in a.sizes3d],
           "interpreted_cycle": [interpreted_cycle(torch, 2, 8, a.rounds), interpreted_cycle(torch, 3, 6, a.rounds)]}
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
