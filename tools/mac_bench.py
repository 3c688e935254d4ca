#!/usr/bin/env python
"""The staggered-grid kernels (examg_mac_op, examg_mac_relax / examg_mac_sweep) on the Stokes operator, beside the coupled cell-field
kernels of like traffic (examg_sys_op, examg_sys_relax, n = 3) on the same cell counts, in one process; then one V-cycle of the Stokes
driver (exastencils_amd/stokes.py), eager and replayed from its graph.

  2-D on cells^2 (default 3072), 3-D on cells^3 (default 192): -Laplace on every velocity component, the gradient and the divergence of
  a uniform grid.  hipEvent-timed after a settle, the variants alternating in every round, the median of the rounds:
    residual      one examg_mac_op, EXAMG_SYS_RESIDUAL, all nd + 1 rows: reads nd + 1 unknowns and nd + 1 right-hand sides, writes nd + 1
                  residuals -- 24 * (nd + 1) compulsory bytes per cell
    sweep         one examg_mac_sweep under `i0 % 3, i1 % 3 [, i2 % 3]`, relax 0.8, in place: every unknown and every right-hand side read
                  once, every unknown written once -- the same 24 * (nd + 1) bytes per cell, if a line were fetched once per sweep; the 3^nd
                  colour launches each touch nearly every line, which is what the figure shows
    colour        one examg_mac_relax of the first colour: its share of the sweep, 24 * (nd + 1) bytes per UPDATED cell (a 3^nd-th)
                  (each call builds the examg_mac_t anew on the host: where the kernel is shorter than that, the figure is the host's --
                  sweep / 3^nd, launched by the library, is the tighter bound on one colour)
    sys_residual  one examg_sys_op, EXAMG_SYS_RESIDUAL, n = 3 cell fields without coefficient fields: 24 * 3 bytes per cell
    sys_relax     one examg_sys_relax of colour 0 (half the cells): 24 * 3 bytes per updated cell
  and cycle_eager / cycle_replay: one mgCycle of StokesSolver on levels 1 .. log2(cells / 3), launched from Python and replayed from the
  captured graph (wall time of the call up to the end of the device work, median of `--cycle-rounds`).

Writes one JSON document (default profiles/mac_bench.json) and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

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


def run_size(torch, ops, nd, cells, rounds, reps, cycle_rounds):
    from exastencils_amd.field import Stencil
    from exastencils_amd.layout import FieldLayout
    from exastencils_amd.stokes import ConfigStokes, StokesSolver

    level = (cells // 3).bit_length() - 1
    if 3 * 2 ** level != cells:
        raise SystemExit("cells must be 3 * 2^level, not %d" % cells)
    S = StokesSolver(ops, ConfigStokes(nd=nd, min_level=1, max_level=level))
    L = S.levels[level]
    y = L.sys
    for k, t in enumerate(y.u + [y.p]):
        ops.fill_random(t, 700 + k)
    start = [t.clone() for t in y.u + [y.p]]
    b, e = L.cell_box
    mask = (1 << (nd + 1)) - 1

    # the yardstick: three cell fields coupled by one star, no coefficient fields
    lc, lo = FieldLayout.cell(nd, (cells,) * nd, 1, align=2), FieldLayout.cell(nd, (cells,) * nd, 0, align=2)
    su = [ops.new_array(lc.size) for _ in range(3)]
    sf = [ops.new_array(lo.size) for _ in range(3)]
    sr = [ops.new_array(lo.size) for _ in range(3)]
    for k, t in enumerate(su + sf):
        ops.fill_random(t, 800 + k)
    star = Stencil(list(y.A[0].offsets), list(y.A[0].coefs))
    none = [[None] * 3 for _ in range(3)]
    C_c, C_o = lc.c_struct(), lo.c_struct()

    cases = [
        ("residual", lambda: ops.mac_op(SYS_RESIDUAL, y, mask, L.row_begin, L.row_end)),
        ("sweep", lambda: ops.mac_sweep(y, 0.8, S.colouring, b, e)),
        ("colour", lambda: ops.mac_relax(y, 0.8, L.colours[0], b, e)),
        ("sys_residual", lambda: ops.sys_op(SYS_RESIDUAL, C_c, su, C_o, sf, C_o, none, C_o, sr, star, 7, b, e)),
        ("sys_relax", lambda: ops.sys_relax(C_c, su, C_o, sf, C_o, none, star, 0.8, 0, b, e)),
    ]
    t = measure(torch, cases, rounds, reps)
    ncell = cells ** nd
    per = 24 * (nd + 1)
    gbs = lambda nbytes, k: round(nbytes / (t[k]["median_ms"] * 1e-3) / 1e9, 1)
    t["residual"]["GB_per_s"] = gbs(ncell * per, "residual")
    t["sweep"]["GB_per_s"] = gbs(ncell * per, "sweep")
    t["sweep"]["launches"] = 3 ** nd
    t["colour"]["GB_per_s"] = gbs(((cells + 2) // 3) ** nd * per, "colour")
    t["colour"]["share_of_the_sweep"] = round(t["colour"]["median_ms"] / t["sweep"]["median_ms"], 4)
    t["sys_residual"]["GB_per_s"] = gbs(ncell * 72, "sys_residual")
    t["sys_relax"]["GB_per_s"] = gbs((ncell + 1) // 2 * 72, "sys_relax")
    t["residual_per_cell_over_sys_residual"] = round(t["residual"]["median_ms"] / t["sys_residual"]["median_ms"], 4)
    t["sweep_over_two_sys_relax"] = round(t["sweep"]["median_ms"] / (2.0 * t["sys_relax"]["median_ms"]), 4)

    # one V-cycle, eager and replayed
    for x, x0 in zip(y.u + [y.p], start):
        x.copy_(x0)
    S.setup()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    S.mgCycle(level)
    eager = [wall(lambda: S.mgCycle(level)) for _ in range(cycle_rounds)]
    S.capture_cycle()
    S.replay_cycle()
    replay = [wall(S.replay_cycle) for _ in range(cycle_rounds)]
    t["cycle_eager"] = {"median_ms": round(statistics.median(eager), 3), "min_ms": round(min(eager), 3), "max_ms": round(max(eager), 3)}
    t["cycle_replay"] = {"median_ms": round(statistics.median(replay), 3), "min_ms": round(min(replay), 3), "max_ms": round(max(replay), 3)}
    return dict({"nd": nd, "cells": cells, "levels": [1, level], "compulsory_bytes_per_cell": per}, **t)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes2d", type=int, nargs="*", default=[3072])
    ap.add_argument("--sizes3d", type=int, nargs="*", default=[192])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cycle-rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mac_bench.json"))
    a = ap.parse_args()
    import torch

    from exastencils_amd.ops import HipOps

    ops = HipOps(0)           # raises without a GPU: nothing here is measured on a CPU
    doc = {"tool": "tools/mac_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps_per_timing": a.reps,
           "cycle_rounds": a.cycle_rounds,
           "sizes": [run_size(torch, ops, 2, c, a.rounds, a.reps, a.cycle_rounds) for c in a.sizes2d] +
                    [run_size(torch, ops, 3, c, a.rounds, a.reps, a.cycle_rounds) for c in a.sizes3d]}
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
