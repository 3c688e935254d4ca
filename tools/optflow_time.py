#!/usr/bin/env python
"""Device times of the coupled-system kernels (include/examg.h: examg_sys_relax, examg_sys_op): n = 2 unknowns on 4096^2 cells
(the optical-flow system: three distinct coefficient fields, the off-diagonal one named twice) and n = 3 on 256^3 (six distinct
ones), ghost 1, x-aligned layouts: one colour of the relaxation, the residual of all rows, the residual of one row.  Yardstick, same
process and sizes: n scalar coloured SMOOTH launches of examg_stencil_op (one colour of one cell field each) -- the work the n
unknowns of one colour would take as uncoupled scalar problems.

Bytes.  `value_bytes` are the compulsory ones: the values the arithmetic needs, each once.  Relaxation of one colour: the other
colour's half of the n unknowns (the neighbours), the colour's half of the m coefficient fields and of the n right-hand sides read,
the colour's half of the n unknowns written: 4 B per cell and array.  Residual of all rows: the same arrays, all cells, 8 B.
Residual of row 0: the unknowns it reads, its coefficient fields, one right-hand side, one result.  Scalar coloured launch: the
neighbours' half and the colour's own half of the unknown, half the right-hand side read, half the unknown written.  `line_bytes`
is what HBM moves at the least: a colour touches every 128-byte line of every array it reads or writes (stride 2), so whole arrays
count, 8 B per cell and array.  Fractions are of 8 TB/s (the datasheet peak; a streaming copy reaches 6.3 TB/s).  The relaxation is
judged on the compulsory bytes: its time over the yardstick's against 1.15 times the ratio of the value bytes.

Every number: median and spread (min, max) of REPS timings, each the mean of ITERS calls between two device events, after warm-up.
Prints one JSON object (profiles/optflow_kernels.json), the solve time of the interpreted example program at the benchmark's size
(levels 2..11, 4096^2 cells) with and without graph replay among it."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from exastencils_amd import lib
from exastencils_amd.field import Stencil
from exastencils_amd.layout import FieldLayout
from exastencils_amd.ops import HipOps

REPS, ITERS = int(os.environ.get("REPS", 7)), int(os.environ.get("ITERS", 20))
BW = 8.0e12
ops = HipOps(0)


def timed(fn, iters=ITERS, reps=REPS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def with_bytes(t, line_bytes, value_bytes):
    t["line_GB"], t["value_GB"] = line_bytes / 1e9, value_bytes / 1e9
    t["fraction_of_8TBs_line_bytes"] = line_bytes / BW * 1e3 / t["median_ms"]
    t["fraction_of_8TBs_value_bytes"] = value_bytes / BW * 1e3 / t["median_ms"]
    return t


def laplace(nd, h):
    off, coef = [(0, 0, 0)], [2.0 * nd / (h * h)]
    for d in range(nd):
        for s in (-1, 1):
            o = [0, 0, 0]
            o[d] = s
            off.append(tuple(o))
            coef.append(-1.0 / (h * h))
    return Stencil(off, coef)


def case(nd, n, cells):
    N = 1
    for c in cells:
        N *= c
    lu, lo = FieldLayout.cell(nd, cells, 1, align=2), FieldLayout.cell(nd, cells, 0, align=2)
    seed = [0]

    def arr(l):
        seed[0] += 1
        t = ops.new_array(l.size)
        ops.fill_random(t, seed[0])
        return t

    u, f, dst = [arr(lu) for _ in range(n)], [arr(lo) for _ in range(n)], [arr(lo) for _ in range(n)]
    g = [[None] * n for _ in range(n)]
    for c in range(n):
        for d in range(c, n):
            g[c][d] = g[d][c] = arr(lo)          # symmetric: n (n + 1) / 2 distinct coefficient fields
    m = n * (n + 1) // 2
    L = laplace(nd, 1.0 / cells[0])
    cu, co = lu.c_struct(), lo.c_struct()
    b, e = [0, 0, 0], list(cells) + [1] * (3 - nd)
    res = {"nd": nd, "n": n, "cells": list(cells), "distinct_coefficient_fields": m}
    res["relax_one_colour"] = with_bytes(timed(lambda: ops.sys_relax(cu, u, co, f, co, g, L, 1.0, 0, b, e)), 8 * N * (3 * n + m), 4 * N * (3 * n + m))
    res["residual_all_rows"] = with_bytes(timed(lambda: ops.sys_op(lib.SYS_RESIDUAL, cu, u, co, f, co, g, co, dst, L, (1 << n) - 1, b, e)),
                                          8 * N * (3 * n + m), 8 * N * (3 * n + m))
    res["residual_one_row"] = with_bytes(timed(lambda: ops.sys_op(lib.SYS_RESIDUAL, cu, u, co, f, co, g, co, dst, L, 1, b, e)),
                                         8 * N * (2 * n + 2), 8 * N * (2 * n + 2))
    w = 1.0 / L.coefs[0]

    def scalar():
        for c in range(n):
            ops.stencil_op(2, cu, u[c], co, f[c], cu, u[c], L, w, 0, b, e)

    res["yardstick_scalar_coloured_smooth_x%d" % n] = with_bytes(timed(scalar), 8 * N * 3 * n, 4 * N * 4 * n)
    y = res["yardstick_scalar_coloured_smooth_x%d" % n]
    res["relax_over_yardstick"] = res["relax_one_colour"]["median_ms"] / y["median_ms"]
    res["value_bytes_ratio"] = (3 * n + m) / (4.0 * n)
    res["line_bytes_ratio"] = (3 * n + m) / (3.0 * n)
    res["relax_bound_1.15_x_value_bytes_ratio"] = 1.15 * res["value_bytes_ratio"]
    res["relax_within_bound"] = res["relax_over_yardstick"] <= res["relax_bound_1.15_x_value_bytes_ratio"]
    return res


out = {"reps": REPS, "iters": ITERS, "device": torch.cuda.get_device_name(0)}
out["n2_4096x4096"] = case(2, 2, (4096, 4096))
torch.cuda.empty_cache()
out["n3_256x256x256"] = case(3, 3, (256, 256, 256))
torch.cuda.empty_cache()

# the interpreted program at the benchmark's size: levels 2..11, one block of 4096^2 cells.  examples/exa4/optflow2d.exa4 is the
# repository's form of Benchmark/OptFlow2D/2D_FD_OptFlow.exa4 (no timers of its own): host clock around the solve loop -- everything
# after the set-up of images, products and right-hand sides -- ended by a device synchronise; second of two runs in this process
import time

from exastencils_amd import exa4

with open(os.path.join(ROOT, "examples", "exa4", "optflow2d.exa4")) as fh:
    TEXT = fh.read()
SOLVE = TEXT[TEXT.index("  Defect@finest ( )\n  Var r0"):TEXT.rindex("}")]
SETUP = TEXT[:TEXT.index("  Defect@finest ( )\n  Var r0")] + "}\nFunction Solve {\n" + SOLVE + "}\n"


def interpreted(auto_graph):
    best = None
    for _ in range(2):
        P = exa4.Exa4Program(SETUP, dict(dimensionality=2, minLevel=2, maxLevel=11), ops=ops, auto_graph=auto_graph)
        P.run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P.call("Solve")
        torch.cuda.synchronize()
        best = {"solve_ms": (time.perf_counter() - t0) * 1e3, "cycles": len(P.printed_values) - 1, "launches": P.launches, "graph_replays": P.graph_replays,
                "residuals": P.printed_values}
        del P
        torch.cuda.empty_cache()
    return best


out["interpreted_optflow2d_levels_2_11_4096x4096"] = {"statement_by_statement": interpreted(False), "graph_replay": interpreted(True)}
print(json.dumps(out, indent=1))
