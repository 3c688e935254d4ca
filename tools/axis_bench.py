#!/usr/bin/env python
"""The table-coefficient stencil kernels (examg_axis_op) against the route the library had before them, in one process:

  one Jacobi step (EXAMG_SMOOTH, colour -1) and one residual of the finite-difference Laplacian of examples/exa4/poisson3d_nonuniform.exa4
  on a `linearFct` grid of n^3 cells, n = 256 and 512 -- hipEvent-timed after a settle, the variants alternating in every round:
    star       examg_axis_op on the z-marching star kernel        (u, rhs, dst: 24 B per point)
    generic    examg_axis_op on the one-lane-per-point kernel
    field      examg_stencil_op on a 7-entry stencil field in planes that holds the same coefficients (80 B per point): what a
               program had to do for this operator before -- the yardstick
    constant   examg_stencil_op on the constant 7-point stencil of the uniform grid: the floor
  The four compute the same operator; star, generic and field must give the same bits (checked at every size before anything is timed).

Writes one JSON document (default profiles/axis_bench.json) and prints it: the median, the smallest and the largest time of every
variant, the ratios to `field`, and the bytes per second the 24 B (80 B) per point amount to."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SMOOTH, RESIDUAL = 2, 1


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


def laplace_entries():
    from exastencils_amd.exa4_parser import Parser

    with open(os.path.join(ROOT, "examples", "exa4", "poisson3d_nonuniform.exa4")) as f:
        return [s for s in Parser(f.read()).parse().stencils if s.name == "Laplace"][0].entries


def coefficient_field(torch, ops, st, lay):
    """The coefficients of `st` on every point the tables cover, as a stencil field in planes: the terms multiplied and added on the device
    in the order of examg_axis_op (one IEEE operation per torch kernel)."""
    from exastencils_amd.field import Stencil

    size = int(lay.size)
    cf = ops.new_array(len(st.offsets) * size)
    tz, ty, tx = lay.shape_zyx
    ref = [lay.ref(d) for d in range(3)]
    dev = [[ops.from_host(t.copy()) for t in st.tables[d]] for d in range(3)]
    n = [len(st.tables[d][0]) for d in range(3)]
    planes = [None] * len(st.offsets)
    for e, s, tab in st.terms:
        X = dev[0][tab[0]] if tab[0] >= 0 else torch.ones(n[0], dtype=torch.float64, device=ops.device)
        Y = dev[1][tab[1]] if tab[1] >= 0 else torch.ones(n[1], dtype=torch.float64, device=ops.device)
        Z = dev[2][tab[2]] if tab[2] >= 0 else torch.ones(n[2], dtype=torch.float64, device=ops.device)
        c = X[None, None, :] * ((float(s) * Z)[:, None, None] * Y[None, :, None])
        planes[e] = c if planes[e] is None else planes[e] + c
    for k, c in enumerate(planes):
        cf[k * size:(k + 1) * size].view(tz, ty, tx)[ref[2]:ref[2] + n[2], ref[1]:ref[1] + n[1], ref[0]:ref[0] + n[0]] = c
    return Stencil(list(st.offsets), [], cf, lay, 0, 1)


def run_size(torch, ops, n, rounds, reps):
    from exastencils_amd.exa4_parser import _const_value
    from exastencils_amd.field import laplace_fd
    from exastencils_amd.grid import AxisGrid, separate
    from exastencils_amd.layout import FieldLayout
    from exastencils_amd.lib import AXIS_GENERIC, AXIS_STAR

    grid = AxisGrid(3, (0.0,) * 3, (1.0,) * 3, (n, n, n), 0, 0, "linearFct")
    st = separate("Laplace", laplace_entries(), 3, 0, grid, _const_value).with_wform(1)
    lu, lf = FieldLayout.node(3, (n, n, n), 1), FieldLayout.node(3, (n, n, n), 0)
    field = coefficient_field(torch, ops, st, lf)
    const = laplace_fd(3, (1.0 / n,) * 3)
    u, f, d = ops.new_array(lu.size), ops.new_array(lf.size), ops.new_array(lu.size)
    ops.fill_random(u, 1234)
    ops.fill_random(f, 77)
    L_u, L_f = lu.c_struct(), lf.c_struct()
    b, e = [1, 1, 1], [n, n, n]
    w = 0.8

    def star(mode):
        return lambda: ops.axis_op(mode, L_u, u, L_f, f, L_u, d, st, w, -1, b, e, route=AXIS_STAR)

    def generic(mode):
        return lambda: ops.axis_op(mode, L_u, u, L_f, f, L_u, d, st, w, -1, b, e, route=AXIS_GENERIC)

    def sfield(mode):
        return lambda: ops.stencil_op(mode, L_u, u, L_f, f, L_u, d, field, w, -1, b, e)

    def constant(mode):
        return lambda: ops.stencil_op(mode, L_u, u, L_f, f, L_u, d, const, w / const.diag, -1, b, e)

    res = {"cells": n, "points": (n - 1) ** 3}
    for mode, name in ((SMOOTH, "smooth"), (RESIDUAL, "residual")):
        outs = []
        for fn in (star(mode), generic(mode), sfield(mode)):      # the same bits, before anything is timed
            d.zero_()
            fn()
            torch.cuda.synchronize()
            outs.append(d.clone())
        same = bool(torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]))
        t = measure(torch, [("star", star(mode)), ("generic", generic(mode)), ("field", sfield(mode)), ("constant", constant(mode))], rounds, reps)
        pts = res["points"]
        for k, v in t.items():
            v["GB_per_s"] = round(pts * (80 if k == "field" else 24) / (v["median_ms"] * 1e-3) / 1e9, 1)
            v["ratio_to_field"] = round(v["median_ms"] / t["field"]["median_ms"], 4)
        # outside the spread of the two: the slowest star timing against the fastest field timing
        t["star_beats_field_outside_the_spread"] = bool(t["star"]["max_ms"] < t["field"]["min_ms"])
        t["same_bits_star_generic_field"] = same
        res[name] = t
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "axis_bench.json"))
    a = ap.parse_args()
    import torch

    from exastencils_amd.ops import HipOps

    ops = HipOps(0)           # raises without a GPU: nothing here is measured on a CPU
    doc = {"tool": "tools/axis_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps_per_timing": a.reps,
           "bytes_per_point": {"star": 24, "generic": 24, "constant": 24, "field": 80},
           "sizes": [run_size(torch, ops, n, a.rounds, a.reps) for n in a.sizes]}
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
