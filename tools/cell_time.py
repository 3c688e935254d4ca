#!/usr/bin/env python
"""Device times of the cell-centred kernels at 512^3 fine cells (ghost 1, x-aligned layouts): examg_restrict_cell,
examg_prolong_add_cell and examg_apply_bc_cell, a Jacobi step on the cell layout next to the same step on the 511^3 node
layout, and the interpreted V(3,3) cycle of examples/exa4/cell3d_dirichlet.exa4 at 512^3 cells (fragment length 4, levels
0..7) after its graph recording.  Every number: median and spread (min, max) of REPS timings, each the mean of ITERS calls
between two device events, after warm-up.  Prints one JSON object (profiles/cell_kernels.json)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from exastencils_amd import exa4, lib
from exastencils_amd.field import Stencil
from exastencils_amd.layout import FieldLayout
from exastencils_amd.lib import ExprC, GeomC
from exastencils_amd.ops import HipOps

REPS, ITERS = int(os.environ.get("REPS", 7)), int(os.environ.get("ITERS", 20))
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


N = 512
lf, lc = FieldLayout.cell(3, (N,) * 3, 1, align=2), FieldLayout.cell(3, (N // 2,) * 3, 1, align=2)
rf, fc, uf = ops.new_array(lf.size), ops.new_array(lc.size), ops.new_array(lf.size)
ops.fill_random(rf, 1)
ops.fill_random(uf, 2)
cf, cc = lf.c_struct(), lc.c_struct()
res = {"fine_cells": [N] * 3, "reps": REPS, "iters": ITERS}
BW = 8.0e12
for name, fn, nbytes in [
        ("restrict_cell", lambda: ops.restrict_cell(cf, rf, cc, fc, 1.0, [0, 0, 0], [N // 2] * 3), 8 * (N ** 3 + (N // 2) ** 3)),
        ("prolong_add_cell", lambda: ops.prolong_add_cell(cc, fc, cf, uf, [0, 0, 0], [N] * 3), 8 * (2 * N ** 3 + (N // 2) ** 3))]:
    t = timed(fn)
    t["compulsory_GB"] = nbytes / 1e9
    t["roofline_ms_8TBs"] = nbytes / BW * 1e3
    t["fraction_of_roofline"] = t["roofline_ms_8TBs"] / t["median_ms"]
    res[name] = t

g = GeomC()
for d in range(3):
    g.pos_begin[d], g.h[d] = 0.0, 1.0 / N
trig = ExprC.from_program([("const", 3.141592653589793), ("x", None), ("*", None), ("sin", None), ("const", 3.141592653589793), ("y", None),
                           ("*", None), ("sin", None), ("*", None), ("const", 4.442882938158366), ("z", None), ("*", None), ("sinh", None),
                           ("*", None)])
res["apply_bc_cell_dirichlet_expr"] = timed(lambda: ops.apply_bc_cell(cf, uf, g, lib.BC_DIRICHLET, trig, 63))
res["apply_bc_cell_neumann"] = timed(lambda: ops.apply_bc_cell(cf, uf, g, lib.BC_NEUMANN, None, 63))

# Jacobi step: cell 512^3 against node 511^3 (inner points), same stencil form, same process
h = 1.0 / N
A = Stencil([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)],
            [6.0 / (h * h)] + [-1.0 / (h * h)] * 6)
w = 0.8 / A.coefs[0]
lfc = FieldLayout.cell(3, (N,) * 3, 0, align=2)
ln, lnf = FieldLayout.node(3, (N,) * 3, 1, align=2), FieldLayout.node(3, (N,) * 3, 0, align=2)
u0, u1, f0 = ops.new_array(lf.size), ops.new_array(lf.size), ops.new_array(lfc.size)
n0, n1, nf = ops.new_array(ln.size), ops.new_array(ln.size), ops.new_array(lnf.size)
for t_, s in ((u0, 3), (f0, 4), (n0, 5), (nf, 6)):
    ops.fill_random(t_, s)
res["jacobi_cell_512"] = timed(lambda: ops.stencil_op(2, cf, u0, lfc.c_struct(), f0, cf, u1, A, w, -1, [0, 0, 0], [N] * 3))
res["jacobi_node_511"] = timed(lambda: ops.stencil_op(2, ln.c_struct(), n0, lnf.c_struct(), nf, ln.c_struct(), n1, A, w, -1, [1, 1, 1], [N] * 3))
res["jacobi_cell_over_node"] = res["jacobi_cell_512"]["median_ms"] / res["jacobi_node_511"]["median_ms"]
del rf, fc, uf, u0, u1, f0, n0, n1, nf
torch.cuda.empty_cache()

# the interpreted cycle of the example program at 512^3 cells: interpreted once, recorded at the second call, replayed after
with open(os.path.join(ROOT, "examples", "exa4", "cell3d_dirichlet.exa4")) as fh:
    P = exa4.Exa4Program(fh.read(), dict(dimensionality=3, minLevel=0, maxLevel=7, domain_fragmentLength_x=4, domain_fragmentLength_y=4,
                                         domain_fragmentLength_z=4), ops=ops)
P.call("Defect", 7)
for _ in range(3):
    P.call("Cycle", 7)
res["vcycle_cell3d_dirichlet_512"] = timed(lambda: P.call("Cycle", 7), iters=5, reps=5)
res["vcycle_graph_replays"] = P.graph_replays
print(json.dumps(res, indent=1))
