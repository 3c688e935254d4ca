#!/usr/bin/env python
"""Launch plans of the three-step pass (csrc/ts3_plan.h) against each other at n^3 (default 512 and 256), debug build, one process:

    python3 tools/time_three_stage_plans.py [512] [256]           medians of interleaved rounds after a run-in, ms per pass
    rocprofv3 --pmc FETCH_SIZE ... -- python3 tools/time_three_stage_plans.py --pmc [--only a,b,..] 512
                                                                  three launches per case, cases separated by a k_fill_random launch
    python3 tools/time_three_stage_plans.py --reduce TIMES.json CASES.json FETCH_DIR WRITE_DIR [HITMISS_DIR]
                                                                  the counter passes as a table (FETCH_SIZE doubled as in pmc_reduce.py)

Cases: the launcher's rule; the uniform grid with forced chunks of 16 / 28 / 48 / 64 planes; whole-round plans with m layers per round
(the rule's m for the box: 2 at 512^3, 7 at 256^3) and R rounds in both layer orders.  --colour: the pass of three colour loops
(examg_rbgs_colours3) instead of three Jacobi steps.  --out FILE writes the times (or, with --pmc, the case names in launch order) as JSON."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def case_list(n):
    cs = [("rule", None, None)]
    for zc in (16, 28, 48, 64):
        cs.append(("uniform %d planes" % zc, zc, None))
    m, rounds = (2, (1, 2, 4, 6, 8)) if n >= 512 else (7, (1, 2))
    for r in rounds:
        for order in (0, 1):
            cs.append(("%d x %d layers, %s" % (m, r, "interleaved" if order else "natural"), None, (m, r, order)))
    return cs


def reduce_(argv):
    import pmc_reduce

    times, names = json.load(open(argv[0])), json.load(open(argv[1]))
    argv = argv[1:]
    fetch = pmc_reduce.segments(pmc_reduce.dispatches(argv[1], "FETCH_SIZE"))
    write = pmc_reduce.segments(pmc_reduce.dispatches(argv[2], "WRITE_SIZE"))
    hit = miss = None
    if len(argv) > 3:
        hit = pmc_reduce.segments(pmc_reduce.dispatches(argv[3], "TCC_HIT_sum"))
        miss = pmc_reduce.segments(pmc_reduce.dispatches(argv[3], "TCC_MISS_sum"))

    def avg(segs, i):
        vals = [v for name, v in segs[i] if "k_three_stage7_lds" in name]
        return sum(vals) / len(vals)

    fetch, write = fetch[-len(names):], write[-len(names):]
    print("| plan | ms | fetch GB | write GB | traffic GB | TB/s | L2 hit |")
    print("|---|---|---|---|---|---|---|")
    for i, name in enumerate(names):
        fb, wb, ms = 2.0 * avg(fetch, i), avg(write, i), times[name]
        hr = ""
        if hit:
            h, m_ = avg(hit[-len(names):], i), avg(miss[-len(names):], i)
            hr = "%.3f" % (h / (h + m_))
        print("| %s | %.4f | %.3f | %.3f | %.3f | %.2f | %s |" % (name, ms, fb / 1e9, wb / 1e9, (fb + wb) / 1e9, (fb + wb) / (ms * 1e-3) / 1e12, hr))


def main():
    if "--reduce" in sys.argv:
        return reduce_(sys.argv[sys.argv.index("--reduce") + 1:])
    import torch
    from exastencils_amd import lib
    from exastencils_amd.field import laplace_fd
    from exastencils_amd.layout import FieldLayout
    from exastencils_amd.ops import HipOps

    pmc, colour = "--pmc" in sys.argv, "--colour" in sys.argv
    only = sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else None
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    ops = HipOps(0, lib.DBG_LIB_PATH)
    L = ops.L
    L.examg_debug_three_stage.argtypes = [C.c_int] * 2
    L.examg_debug_three_stage_plan.argtypes = [C.c_int] * 4
    sizes = [int(a) for a in sys.argv[1:] if a.isdigit()] or [512, 256]

    def select(zc, plan):
        L.examg_debug_three_stage(0, zc if zc else -1)
        if plan:
            L.examg_debug_three_stage_plan(plan[0], plan[1], plan[2], 0)
        else:
            L.examg_debug_three_stage_plan(0, 0, -1, 0)

    def timed(fn, reps=30):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    record, pmc_names = {}, []
    for n in sizes:
        lu, lf = FieldLayout.node(3, (n, n, n), 1), FieldLayout.node(3, (n, n, n), 0, True, False)
        u, un, f = ops.new_array(lu.size), ops.new_array(lu.size), ops.new_array(lf.size)
        ops.fill_random(u, 1)
        ops.fill_random(f, 2)
        un.copy_(u)
        A = laplace_fd(3, (1.0 / n,) * 3)
        w = 0.8 / A.diag
        b, e = [1, 1, 1], [n, n, n]
        Ls, Fs = lu.c_struct(), lf.c_struct()
        state = [u, un]

        def run():
            if colour:      # three colour loops per pass, the first colour alternating as in three sweeps
                ops.rbgs_colours3(Ls, state[0], state[1], Fs, f, A, w, state[0] is un, b, e)
            else:
                ops.jacobi3(Ls, state[0], state[1], None, Fs, f, A, w, b, e)
            state.reverse()

        cases = [("%d^3 %s" % (n, name), zc, plan) for name, zc, plan in case_list(n)]
        if only:
            cases = [c for c in cases if any(c[0].endswith(o) for o in only)]
        if pmc:
            scratch = ops.new_array(1024)
            for name, zc, plan in cases:
                select(zc, plan)
                for _ in range(3):
                    run()
                ops.fill_random(scratch, 3)      # the separator pmc_reduce.segments looks for
                pmc_names.append(name)
                print("pmc case", name, flush=True)
            torch.cuda.synchronize()
            select(None, None)
            continue
        for _ in range(20):
            for _, zc, plan in cases:
                select(zc, plan)
                run()
        res = {name: [] for name, _, _ in cases}
        for _ in range(5):
            for name, zc, plan in cases:
                select(zc, plan)
                run()
                res[name].append(timed(run))
        select(None, None)
        for name, _, _ in cases:
            ms = statistics.median(res[name])
            record[name] = ms
            print("%-40s %.4f ms per pass (min %.4f, max %.4f), %.3e LU/s" % (name, ms, min(res[name]), max(res[name]), 3 * (n - 1) ** 3 / (ms * 1e-3)), flush=True)
    if out_path:
        json.dump(pmc_names if pmc else record, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
