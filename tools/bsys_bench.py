#!/usr/bin/env python
"""The block-system kernels (examg_bsys_op, examg_bsys_relax) on the linear-elasticity blocks, against the launches the library had
for the same arithmetic before them, in one process:

  n = 2 unknowns on cells^2 nodes (default 4096), n = 3 unknowns on cells^3 nodes (default 256); the blocks of row c are
  (lambda + mu) * d_cd on u_d and lambda * Laplace merged into the diagonal block (tests/blocksys_cases.py states the same table).
  hipEvent-timed after a settle, the variants alternating in every round:
    residual   one examg_bsys_op, EXAMG_SYS_RESIDUAL, all rows (reads n unknowns and n right-hand sides, writes n residuals:
               24 * n compulsory bytes per point)
    relax      one examg_bsys_relax of the first colour of `i0 % 2, i1 % 2 [, i2 % 2]`, relax 0.8, in place (the same 24 * n bytes
               per UPDATED point, a 2^nd-th of the points)
    stencil_ops  n * n examg_stencil_op launches, EXAMG_APPLY, one per block into n * n scratch arrays: what a caller could issue
               for the operator before these entry points existed (the n sums and subtractions that complete a residual not
               included: they would be n * (n + 1) examg_axpby launches more)

Writes one JSON document (default profiles/bsys_bench.json) and prints it: the median, the smallest and the largest time of every
variant, the bytes per second that the compulsory bytes amount to, and residual / stencil_ops.  --sizes2d / --sizes3d choose the sizes
(profiles/bsys_bench_sizes.json).  profiles/bsys_bench_routes.json is this tool's output while examg_bsys_op had a second, marching kernel:
the two alternated as `gather` and `march`; the marching kernel lost at every size and was deleted."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SYS_RESIDUAL, APPLY = 1, 0
LAMBDA, MU = 195.0, 130.0


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


def elasticity_blocks(nd, cells):
    """Row c: (lambda + mu) * d_cd on u_d, the diagonal block merged with lambda * Laplace -- the host's stencil arithmetic (include/examg.h)."""
    from exastencils_amd.exa4_blocksys import _merge
    from exastencils_amd.field import Stencil

    h = 1.0 / cells

    def axis(d, s):
        o = [0, 0, 0]
        o[d] = s
        return tuple(o)

    def second(d, s):
        return Stencil([(0, 0, 0), axis(d, -1), axis(d, 1)], [s * -2.0 / (h * h), s / (h * h), s / (h * h)])

    def mixed(d, e, s):
        offs, co = [], []
        for a, b, sign in ((-1, 1, -1.0), (1, 1, 1.0), (-1, -1, 1.0), (1, -1, -1.0)):
            o = [0, 0, 0]
            o[d], o[e] = a, b
            offs.append(tuple(o))
            co.append(s * sign / (4.0 * h * h))
        return Stencil(offs, co)

    lap = Stencil([(0, 0, 0)] + [axis(d, s) for d in range(nd) for s in (-1, 1)], [LAMBDA * -2.0 * nd / (h * h)] + [LAMBDA / (h * h)] * (2 * nd))
    return [[_merge(second(c, LAMBDA + MU), lap.offsets, lap.coefs) if c == d else mixed(min(c, d), max(c, d), LAMBDA + MU) for d in range(nd)]
            for c in range(nd)]


def run_size(torch, ops, nd, cells, rounds, reps):
    from exastencils_amd.field import Colouring, Stencil
    from exastencils_amd.layout import FieldLayout

    class NoCentre(Stencil):      # examg_stencil_op reads `diag` in EXAMG_SMOOTH only
        diag_index = property(lambda self: self.offsets.index((0, 0, 0)) if (0, 0, 0) in self.offsets else 0)

    n = nd
    lu, lf = FieldLayout.node(nd, (cells,) * nd, 1), FieldLayout.node(nd, (cells,) * nd, 0)
    A = elasticity_blocks(nd, cells)
    u = [ops.new_array(lu.size) for _ in range(n)]
    f = [ops.new_array(lf.size) for _ in range(n)]
    r = [ops.new_array(lf.size) for _ in range(n)]
    tmp = [ops.new_array(lf.size) for _ in range(n * n)]
    for k, t in enumerate(u + f):
        ops.fill_random(t, 500 + k)
    L_u, L_f = lu.c_struct(), lf.c_struct()
    b = [1 if t < nd else 0 for t in range(3)]
    e = [cells if t < nd else 1 for t in range(3)]
    col = next(Colouring.axis_parity(nd).colours())
    plain = [[NoCentre(S.offsets, S.coefs) for S in row] for row in A]
    points = (cells - 1) ** nd
    coloured = ((cells - 1) // 2) ** nd      # inner points 1 .. cells - 1 with every index even

    def residual():
        ops.bsys_op(SYS_RESIDUAL, L_u, u, L_f, f, L_f, r, A, (1 << n) - 1, b, e)

    def relax():
        ops.bsys_relax(L_u, u, L_f, f, A, 0.8, col, b, e)

    def stencil_ops():
        for c in range(n):
            for d in range(n):
                ops.stencil_op(APPLY, L_u, u[d], None, None, L_f, tmp[c * n + d], plain[c][d], 0.0, -1, b, e)

    u0 = [t.clone() for t in u]
    route = ops.bsys_route(SYS_RESIDUAL, L_u, u, L_f, f, L_f, r, A, (1 << n) - 1, b, e)
    t = measure(torch, [("residual", residual), ("relax", relax), ("stencil_ops", stencil_ops)], rounds, reps)
    for x, x0 in zip(u, u0):      # (the relaxation ran in place, again and again)
        x.copy_(x0)
    t["residual"]["GB_per_s"] = round(points * 24 * n / (t["residual"]["median_ms"] * 1e-3) / 1e9, 1)
    t["relax"]["GB_per_s"] = round(coloured * 24 * n / (t["relax"]["median_ms"] * 1e-3) / 1e9, 1)
    t["stencil_ops"]["GB_per_s_of_the_residual"] = round(points * 24 * n / (t["stencil_ops"]["median_ms"] * 1e-3) / 1e9, 1)
    t["residual_over_stencil_ops"] = round(t["residual"]["median_ms"] / t["stencil_ops"]["median_ms"], 4)
    return dict({"nd": nd, "n": n, "cells": cells, "points": points, "points_of_the_colour": coloured, "route_of_the_residual": route}, **t)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes2d", type=int, nargs="*", default=[4096])
    ap.add_argument("--sizes3d", type=int, nargs="*", default=[256])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bsys_bench.json"))
    a = ap.parse_args()
    import torch

    from exastencils_amd.ops import HipOps

    ops = HipOps(0)           # raises without a GPU: nothing here is measured on a CPU
    doc = {"tool": "tools/bsys_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps_per_timing": a.reps,
           "compulsory_bytes_per_point": "24 * n", "routes": {"1": "gather (the only route)"},
           "sizes": [run_size(torch, ops, 2, c, a.rounds, a.reps) for c in a.sizes2d] + [run_size(torch, ops, 3, c, a.rounds, a.reps) for c in a.sizes3d]}
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
