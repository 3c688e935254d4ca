#!/usr/bin/env python
"""The y-marching 2-D 5-point star (route `ymarch` of examg_stencil_op, csrc/kernels_star2d.hip) against the generic kernel of the same
library -- the kernel these loops took before the route existed -- and the 5-point benchmark program.

One process on the debug build (examg_debug_star2d selects the kernel per call), device events, every number the median and the spread
(min, max) of REPS rounds of ITERS launches; the variants alternate within each round.  Layouts of the benchmark: a cell field with one
ghost layer, the right-hand side without ghost layers, the reference layout (no padding).

  profiles/star2d_bench_sizes.json   Jacobi step, residual and one red-black colour at 256^2 .. 4096^2 cells, both kernels; the fraction
                                     of 8 TB/s on 24 B per point; chunk lengths at 4096^2
  profiles/star2d_bench.json         examples/exa4/jacobi2d_cell.exa4 at level 11 (4096^2 cells, 100 steps): the `kernel` and `applyBC`
                                     timers and the solve time with the route on / off and the faces of the boundary function merged / separate

Usage: python tools/star2d_bench.py [--out DIR] [--sizes 256,512,...] [--level 11] [--skip-program]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from exastencils_amd import exa4, knowledge, lib  # noqa: E402
from exastencils_amd.field import Stencil  # noqa: E402
from exastencils_amd.layout import FieldLayout  # noqa: E402
from exastencils_amd.ops import HipOps  # noqa: E402

REPS, ITERS = int(os.environ.get("REPS", 7)), int(os.environ.get("ITERS", 20))
BW = 8.0e12
EX = os.path.join(ROOT, "examples", "exa4")


def alternating(variants, iters=ITERS, reps=REPS):
    """variants: {name: (select, launch)}.  Every round times every variant once, in turn: ITERS launches between two device events."""
    for select, launch in variants.values():
        select()
        for _ in range(3):
            launch()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, (select, launch) in variants.items():
            select()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                launch()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / iters)
    return {name: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for name, t in times.items()}


def size_sweep(ops, sizes):
    L = ops.L
    out = {"reps": REPS, "iters": ITERS, "bytes_per_point": 24, "bandwidth_TBs": 8.0, "sizes": {}}
    for n in sizes:
        lu, lf = FieldLayout.cell(2, (n, n), 1), FieldLayout.cell(2, (n, n), 0)
        h = (2.0 / n, 1.0 / n)
        A = Stencil([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0)],
                    [2.0 / (h[0] * h[0]) + 2.0 / (h[1] * h[1]), -1.0 / (h[0] * h[0]), -1.0 / (h[0] * h[0]), -1.0 / (h[1] * h[1]), -1.0 / (h[1] * h[1])])
        w = (1.0 / A.coefs[0]) * 0.8
        u, v, f = ops.new_array(lu.size), ops.new_array(lu.size), ops.new_array(lf.size)
        ops.fill_random(u, 1)
        ops.fill_random(f, 2)
        cu, cf = lu.c_struct(), lf.c_struct()
        b, e = [0, 0, 0], [n, n, 1]
        loops = {"jacobi": lambda: ops.stencil_op(2, cu, u, cf, f, cu, v, A, w, -1, b, e),
                 "residual": lambda: ops.stencil_op(1, cu, u, cf, f, cu, v, A, 0.0, -1, b, e),
                 "rb_colour": lambda: ops.stencil_op(2, cu, u, cf, f, cu, u, A, w, 0, b, e)}
        roof = 24.0 * n * n / BW * 1e3
        rec = {"points": n * n, "roofline_ms": roof}
        for name, launch in loops.items():
            variants = {"generic": (lambda: L.examg_debug_star2d(0, 0), launch), "ymarch": (lambda: L.examg_debug_star2d(1, 0), launch)}
            if n == 4096 and name == "jacobi":
                for c in (16, 64, 128, 512):
                    variants["ymarch_chunk%d" % c] = (lambda c=c: L.examg_debug_star2d(1, c), launch)
            t = alternating(variants)
            for r in t.values():
                r["fraction_of_roofline"] = roof / r["median_ms"]
            t["ymarch_over_generic"] = t["ymarch"]["median_ms"] / t["generic"]["median_ms"]
            rec[name] = t
            print("%5d^2 %-10s generic %.4f ms (%.2f)  ymarch %.4f ms (%.2f)  ratio %.3f" % (
                n, name, t["generic"]["median_ms"], t["generic"]["fraction_of_roofline"], t["ymarch"]["median_ms"],
                t["ymarch"]["fraction_of_roofline"], t["ymarch_over_generic"]), flush=True)
        out["sizes"][str(n)] = rec
        L.examg_debug_star2d(-1, 0)
        del u, v, f
        torch.cuda.empty_cache()
    return out


def program(ops, level):
    """The own program at `level`, four ways; every run after one warm-up run of the same kind."""
    k = knowledge.parse_file(os.path.join(EX, "jacobi2d_cell.knowledge"))
    k["minLevel"] = k["maxLevel"] = level
    with open(os.path.join(EX, "jacobi2d_cell.exa4")) as fh:
        src = fh.read()
    out = {"level": level, "cells": [2 << level, 2 << level], "runs": {}}
    for on in (1, 0):
        for fuse in (True, False):
            name = "route_%s_faces_%s" % ("on" if on else "off", "merged" if fuse else "separate")
            recs = []
            for _ in range(3):
                ops.L.examg_debug_star2d(on, 0)
                P = exa4.Exa4Program(src, dict(k), ops=ops, fuse=fuse, auto_graph=False)
                printed = P.run()
                recs.append({t: P.timers.get(t, 0.0) * 1e3 for t in ("kernel", "applyBC", "solve")})
                del P
                torch.cuda.empty_cache()
            recs = recs[1:]
            out["runs"][name] = {"kernel_ms": [r["kernel"] for r in recs], "applyBC_ms": [r["applyBC"] for r in recs],
                                 "solve_ms": [r["solve"] for r in recs], "launches_printed": printed[-1], "last_residual": printed[-2]}
            print(name, out["runs"][name], flush=True)
    ops.L.examg_debug_star2d(-1, 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--sizes", default="256,512,1024,2048,4096")
    ap.add_argument("--level", type=int, default=11)
    ap.add_argument("--skip-program", action="store_true")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    ops = HipOps(0, lib.DBG_LIB_PATH)
    sizes = size_sweep(ops, [int(s) for s in args.sizes.split(",") if s])
    with open(os.path.join(args.out, "star2d_bench_sizes.json"), "w") as fh:
        json.dump(sizes, fh, indent=1)
    if not args.skip_program:
        with open(os.path.join(args.out, "star2d_bench.json"), "w") as fh:
            json.dump(program(ops, args.level), fh, indent=1)


if __name__ == "__main__":
    main()
