#!/usr/bin/env python
"""The two kernels of examg_cstencil_op (complex node fields) against each other and against the real loop, in one process:

  one residual (EXAMG_RESIDUAL), one Jacobi step (EXAMG_SMOOTH, colour -1, out of place) and one colour of the local solve (EXAMG_CRELAX,
  colour 0, in place) of the complex shifted Laplacian -Laplace - (1 + 0.5j) k^2, k = 80, on n^2 points (5-point) and n^3 points (7-point),
  hipEvent-timed after a settle, the variants alternating in every round:
    march      examg_cstencil_op on the marching kernel           (u, rhs, dst: 48 B per point; a colour in place: half the points)
    gather     examg_cstencil_op on the one-lane-per-point kernel
  forced through the debug library (examg_debug_cstencil_route); both must give the same bits (checked before anything is timed).
    real       examg_stencil_op on the real parts of the same stencil (24 B per point; the colour as one red-black half sweep): the
               reference point -- a complex loop moves twice the bytes

Writes one JSON document (default profiles/complex_bench.json) and prints it: the median, the smallest and the largest time of every
variant, the bytes per second that 48 B (24 B) per updated point amount to, and march / gather.  --sizes2d / --sizes3d choose the sizes
(profiles/complex_bench_sizes.json: where the default route changes), --chunks adds a sweep of the rows per wave of the marching kernel
(profiles/complex_bench_chunks.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RESIDUAL, SMOOTH, CRELAX = 1, 2, 3


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


def shifted_laplace(nd, n, k=80.0, shift=1.0 + 0.5j):
    from exastencils_amd.field import Stencil

    h2 = float(n) ** 2
    offs = [(0, 0, 0)]
    for d in range(nd):
        for s in (-1, 1):
            o = [0, 0, 0]
            o[d] = s
            offs.append(tuple(o))
    return Stencil(offs, [complex(2 * nd * h2, 0.0) - shift * k * k] + [complex(-h2, 0.0)] * (2 * nd))


def run_size(torch, ops, nd, n, rounds, reps, chunk=0):
    from exastencils_amd import lib
    from exastencils_amd.field import Stencil
    from exastencils_amd.layout import FieldLayout

    cells = (n,) * nd
    lu, lf = FieldLayout.node(nd, cells, 1), FieldLayout.node(nd, cells, 0)
    st = shifted_laplace(nd, n)
    real = Stencil(st.offsets, [c.real for c in st.coefs])
    u, f, d = ops.new_complex_array(lu.size), ops.new_complex_array(lf.size), ops.new_complex_array(lu.size)
    ops.fill_random(u, 1234)
    ops.fill_random(f, 77)
    ru, rf, rd = ops.new_array(lu.size), ops.new_array(lf.size), ops.new_array(lu.size)
    ops.fill_random(ru, 1234)
    ops.fill_random(rf, 77)
    L_u, L_f = lu.c_struct(), lf.c_struct()
    b = [1 if t < nd else 0 for t in range(3)]
    e = [n if t < nd else 1 for t in range(3)]
    w = 0.8 / st.coefs[0]
    points = (n - 1) ** nd

    def complex_loop(route, mode):
        def fn():
            ops.L.examg_debug_cstencil_route(route, chunk)
            if mode == CRELAX:
                ops.cstencil_op(CRELAX, L_u, u, L_f, f, None, None, st, 0.6, 0, b, e)
            else:
                ops.cstencil_op(mode, L_u, u, L_f, f, L_u, d, st, w, -1, b, e)
        return fn

    def real_loop(mode):
        if mode == CRELAX:
            return lambda: ops.stencil_op(SMOOTH, L_u, ru, L_f, rf, L_u, ru, real, 0.6 / real.diag, 0, b, e)
        return lambda: ops.stencil_op(mode, L_u, ru, L_f, rf, L_u, rd, real, 0.8 / real.diag, -1, b, e)

    res = {"nd": nd, "cells": n, "points": points}
    if chunk:
        res["march_rows_per_wave"] = chunk
    for mode, name in ((RESIDUAL, "residual"), (SMOOTH, "jacobi"), (CRELAX, "crelax_colour")):
        outs = []
        u0 = u.clone()
        for route in (lib.CSTENCIL_MARCH, lib.CSTENCIL_GATHER):      # the same bits, before anything is timed
            u.copy_(u0)
            d.zero_()
            complex_loop(route, mode)()
            torch.cuda.synchronize()
            outs.append((u.clone(), d.clone()))
        u.copy_(u0)
        same = bool(torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]))
        t = measure(torch, [("march", complex_loop(lib.CSTENCIL_MARCH, mode)), ("gather", complex_loop(lib.CSTENCIL_GATHER, mode)),
                            ("real", real_loop(mode))], rounds, reps)
        upd = points // 2 if mode == CRELAX else points
        for k, v in t.items():
            v["GB_per_s"] = round(upd * (24 if k == "real" else 48) / (v["median_ms"] * 1e-3) / 1e9, 1)
        t["march_over_gather"] = round(t["march"]["median_ms"] / t["gather"]["median_ms"], 4)
        t["march_over_real"] = round(t["march"]["median_ms"] / t["real"]["median_ms"], 4)
        t["march_beats_gather_outside_the_spread"] = bool(t["march"]["max_ms"] < t["gather"]["min_ms"])
        t["same_bits_march_gather"] = same
        res[name] = t
        u.copy_(u0)
    ops.L.examg_debug_cstencil_route(0, 0)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes2d", type=int, nargs="*", default=[4096])
    ap.add_argument("--sizes3d", type=int, nargs="*", default=[256])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=0, help="rows (planes) per wave of the marching kernel; 0: the library's choice")
    ap.add_argument("--chunks", type=int, nargs="*", default=[], help="a sweep: every size once more with each of these rows per wave (chunk_sweep)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "complex_bench.json"))
    a = ap.parse_args()
    import torch

    from exastencils_amd import lib
    from exastencils_amd.ops import HipOps

    ops = HipOps(0, lib.DBG_LIB_PATH)           # raises without a GPU: nothing here is measured on a CPU
    doc = {"tool": "tools/complex_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps_per_timing": a.reps,
           "bytes_per_updated_point": {"march": 48, "gather": 48, "real": 24},
           "sizes": [run_size(torch, ops, 2, n, a.rounds, a.reps, a.chunk) for n in a.sizes2d] + [run_size(torch, ops, 3, n, a.rounds, a.reps, a.chunk) for n in a.sizes3d]}
    if a.chunks:
        doc["chunk_sweep"] = [{"march_rows_per_wave": c, "sizes": [run_size(torch, ops, 2, n, a.rounds, a.reps, c) for n in a.sizes2d] +
                               [run_size(torch, ops, 3, n, a.rounds, a.reps, c) for n in a.sizes3d]} for c in a.chunks]
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
