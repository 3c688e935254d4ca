#!/usr/bin/env python
"""Device times of the semilinear kernels (include/examg.h: examg_nl_smooth, examg_nl_op): the 2-D 5-point Laplacian on 4096^2 cells
and the 3-D 7-point one on 256^3, ghost 1 -- a Jacobi step, one colour in place and the residual, each with a program of the exact
class (c = (gamma u) u, d = ((3 gamma) u) u: five and seven multiplications) and with the Bratu programs (c = gamma exp(u),
d = (gamma (1 + u)) exp(u): two fp64 exp per point in the smoother, one in the residual).  Yardstick, same process, boxes and
stencils: examg_stencil_op (EXAMG_SMOOTH, all points and one colour; EXAMG_RESIDUAL), the linear kernels, which move the same
compulsory bytes -- u read, rhs read, result written: 24 B per point (a colour touches every 128-byte line of the three arrays: the same
24 B per point of the box at half the updates).  Fractions are of 8 TB/s (the datasheet peak; a streaming copy reaches 6.3 TB/s).

The Jacobi step and the residual run twice on the same inputs: on the row-marching star kernel (what the library does) and, through
the debug build's examg_debug_nl_gather_only, on the gather kernel; `star_over_gather_*` is the ratio that decides whether the star
path stays (kept only if it is below 0.97: the box-to-box spread is 3 %).

Every number: median and spread (min, max) of REPS timings, each the mean of ITERS calls between two device events, after warm-up of
that very call.  Prints one JSON object (profiles/nl_kernels.json), the solve time of the interpreted examples/exa4/bratu2d_fas.exa4
(levels 0 .. 7, 1152^2 cells) with and without graph replay among it."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from exastencils_amd import exa4, lib
from exastencils_amd.field import Stencil
from exastencils_amd.layout import FieldLayout
from exastencils_amd.ops import HipOps

REPS, ITERS = int(os.environ.get("REPS", 7)), int(os.environ.get("ITERS", 20))
BW = 8.0e12
GAMMA = 0.3
PROGRAMS = {
    "exact": ([("const", GAMMA), ("u", None), ("*", None), ("u", None), ("*", None)],
              [("const", 3.0), ("const", GAMMA), ("*", None), ("u", None), ("*", None), ("u", None), ("*", None)]),
    "exp": ([("const", GAMMA), ("u", None), ("exp", None), ("*", None)],
            [("const", GAMMA), ("const", 1.0), ("u", None), ("+", None), ("*", None), ("u", None), ("exp", None), ("*", None)]),
}
ops = HipOps(0, lib.DBG_LIB_PATH)      # the debug build: the same kernels, and the switch that sends star stencils to the gather kernel


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


def with_bytes(t, nbytes):
    t["GB"] = nbytes / 1e9
    t["fraction_of_8TBs"] = nbytes / BW * 1e3 / t["median_ms"]
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


def case(nd, cells):
    lu, lf = FieldLayout.node(nd, cells, 1), FieldLayout.node(nd, cells, 0, True, False)
    b = [1] * nd + [0] * (3 - nd)
    e = list(cells) + [1] * (3 - nd)
    pts = 1
    for d in range(nd):
        pts *= e[d] - b[d]
    u, un, r = (ops.new_array(lu.size) for _ in range(3))
    f = ops.new_array(lf.size)
    ops.fill_random(u, 1)
    ops.fill_random(f, 2)
    cu, cf = lu.c_struct(), lf.c_struct()
    A = laplace(nd, 1.0 / cells[0])
    w = 0.8 / A.diag
    res = {"nd": nd, "cells": list(cells), "points": pts}

    def finite(t, what, bound=None):
        # the in-place loops iterate on their own output some 150 times: the timed inputs must stay ordinary numbers
        assert bool(torch.isfinite(t).all()) and (bound is None or float(t.abs().max()) < bound), what + ": the values ran away"

    ops.fill_random(un, 3)
    lin = res["linear_stencil_op"] = {
        "jacobi": with_bytes(timed(lambda: ops.stencil_op(2, cu, u, cf, f, cu, r, A, w, -1, b, e)), 24 * pts),
        "colour": with_bytes(timed(lambda: ops.stencil_op(2, cu, un, cf, f, cu, un, A, w, 0, b, e)), 24 * pts),
        "residual": with_bytes(timed(lambda: ops.stencil_op(1, cu, u, cf, f, cu, r, A, 0.0, -1, b, e)), 24 * pts),
    }
    finite(un, "linear colour", 1.0e3)
    for name, (pc, pd) in PROGRAMS.items():
        c, d = lib.NlExprC.from_program(pc), lib.NlExprC.from_program(pd)
        cur = res["semilinear_" + name] = {}
        for path, gather in (("star_path", 0), ("gather_path", 1)):      # the same calls on the same inputs, the star stencil on either kernel
            ops.L.examg_debug_nl_gather_only(gather)
            cur[path] = {
                "jacobi": with_bytes(timed(lambda: ops.nl_smooth(cu, u, cu, r, cf, f, A, c, d, 0.8, -1, b, e)), 24 * pts),
                "residual": with_bytes(timed(lambda: ops.nl_op(lib.NL_RESIDUAL, cu, u, cu, u, cf, f, cu, r, A, c, b, e)), 24 * pts),
            }
            finite(r, name + " " + path)
        ops.L.examg_debug_nl_gather_only(0)
        for k in ("jacobi", "residual"):
            cur["star_over_gather_" + k] = cur["star_path"][k]["median_ms"] / cur["gather_path"][k]["median_ms"]
            cur["star_path"][k]["over_linear"] = cur["star_path"][k]["median_ms"] / lin[k]["median_ms"]
            cur["gather_path"][k]["over_linear"] = cur["gather_path"][k]["median_ms"] / lin[k]["median_ms"]
        ops.fill_random(un, 3)      # the coloured loop runs in place on un (the gather kernel: the star path takes all points only)
        cur["colour"] = with_bytes(timed(lambda: ops.nl_smooth(cu, un, cu, un, cf, f, A, c, d, 0.8, 0, b, e)), 24 * pts)
        finite(un, name + " colour", 1.0e3)
        cur["colour"]["over_linear"] = cur["colour"]["median_ms"] / lin["colour"]["median_ms"]
    return res


out = {"reps": REPS, "iters": ITERS, "device": torch.cuda.get_device_name(0)}
out["2d_5pt_4096x4096"] = case(2, (4096, 4096))
torch.cuda.empty_cache()
out["3d_7pt_256x256x256"] = case(3, (256, 256, 256))
torch.cuda.empty_cache()

# the interpreted program: host clock around run(), ended by a device synchronise; second of two runs in this process
with open(os.path.join(ROOT, "examples", "exa4", "bratu2d_fas.exa4")) as fh:
    TEXT = fh.read()
K = dict(dimensionality=2, minLevel=0, maxLevel=7, domain_rect_generate=True, domain_rect_numBlocks_x=3, domain_rect_numBlocks_y=3, domain_rect_numBlocks_z=1,
         domain_rect_numFragsPerBlock_x=3, domain_rect_numFragsPerBlock_y=3, domain_rect_numFragsPerBlock_z=1)


def interpreted(auto_graph):
    best = None
    for _ in range(2):
        P = exa4.Exa4Program(TEXT, dict(K), ops=ops, auto_graph=auto_graph)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lines = P.run()
        torch.cuda.synchronize()
        best = {"seconds": time.perf_counter() - t0, "launches": P.launches, "graph_replays": P.graph_replays, "cycles": int(lines[-1])}
    return best


out["bratu2d_fas_1152x1152"] = {"interpreted": interpreted(False), "graph_replay": interpreted(True)}
print(json.dumps(out, indent=1))
