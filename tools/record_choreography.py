#!/usr/bin/env python
"""Record which kernel-layer and communicator calls the host layer (exastencils_amd/smoothers.py, solver.py) issues, in which order,
on which boxes and arrays -- the property a change of the choreography must keep and that bit-for-bit tests of the results cannot see
(a pass issued twice gives the same bits).

A kernel layer and a communicator are wrapped in proxies that log every call: method, integer / box / scalar arguments, every array as
the role name the scenario gave it (never a pointer), the result of a yes/no probe and, on a GPU, whether the call was issued while the
kernel layer's side stream was the current one.  The fork and join of the two streams (`wait_stream`) are calls of torch, not of the
kernel layer, and are NOT logged: that the streams wait for each other is left to the bit-for-bit tests of the results.

`python tools/record_choreography.py [--gpu]` writes the traces of every scenario to tests/traces/cpu.json (gpu.json);
tests/test_choreography_trace.py replays the scenarios and demands the committed traces."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from exastencils_amd.comm import Communicator  # noqa: E402
from exastencils_amd.domain import RectDomain  # noqa: E402
from exastencils_amd.field import Colouring, Field, Stencil, laplace_fd  # noqa: E402
from exastencils_amd.layout import FieldLayout  # noqa: E402
from exastencils_amd import smoothers  # noqa: E402
from exastencils_amd.solver import ConfigL3, ConfigL4, SolverFromL3, SolverFromL4  # noqa: E402

TRACES = os.path.join(ROOT, "tests", "traces")
# plumbing of the kernel layer: no launch, nothing a choreography is made of
PLUMBING = {"new_array", "new_scalar", "ptr", "synchronize", "side_stream", "to_host", "from_host", "scalar_value"}


class Recorder:
    def __init__(self, on_side=None):
        self.events, self._names, self._keep, self.on_side = [], {}, [], on_side

    def name(self, t, role):
        """Register array `t` under `role` (the first name an array gets stays); the array is kept alive, so no later one takes its address."""
        if t.data_ptr() not in self._names:
            self._names[t.data_ptr()] = role
            self._keep.append(t)

    def name_field(self, f, role):
        for i, t in enumerate(f.slots):
            self.name(t, role if len(f.slots) == 1 else "%s%d" % (role, i))

    def _enc(self, v):
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        if isinstance(v, (list, tuple, ctypes.Array)):
            return [self._enc(x) for x in v]
        if hasattr(v, "data_ptr"):
            if v.numel() == 1:
                return "scalar"
            self.name(v, "anon%d" % sum(1 for n in self._names.values() if n.startswith("anon")))
            return self._names[v.data_ptr()]
        if isinstance(v, ctypes.Structure) and hasattr(v, "inner"):
            s = "lay n%s g%s d%s" % tuple(".".join(str(x) for x in getattr(v, k)) for k in ("inner", "ghost_l", "dup_l"))
            if any(v.pad_l) or any(v.pad_r):
                s += " p%s/%s" % tuple(".".join(str(x) for x in getattr(v, k)) for k in ("pad_l", "pad_r"))
            return s + (" t%d" % v.transform if v.transform else "")
        if isinstance(v, Field):
            return "%s@%d" % (v.name, v.level)
        if isinstance(v, Stencil):
            return "stencil%d%s" % (len(v.offsets), "f" if v.cfield is not None else "")
        if isinstance(v, Colouring):
            return "colour%s" % (list(v.rem),)
        return type(v).__name__

    def log(self, what, args=(), kwargs=None, ret=None):
        ev = {"c": what, "a": self._enc(list(args))}
        if kwargs:
            ev["k"] = {k: self._enc(v) for k, v in sorted(kwargs.items())}
        if isinstance(ret, bool):
            ev["r"] = ret
        if self.on_side is not None and self.on_side():
            ev["side"] = True
        self.events.append(ev)

    def wrap(self, inner, prefix):
        return _Traced(inner, self, prefix)


class _Traced:
    """Every attribute of `inner`, absent ones included (hasattr answers as for `inner`); calls of its methods are logged."""

    def __init__(self, inner, rec, prefix):
        self.__dict__.update(_inner=inner, _rec=rec, _prefix=prefix)

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if not callable(attr) or name in PLUMBING or name.startswith("_") or isinstance(attr, type) or name == "torch":
            return attr

        def call(*args, **kwargs):
            ret = attr(*args, **kwargs)
            self._rec.log("%s.%s" % (self._prefix, name), args, kwargs, ret)
            return ret
        return call

    def __setattr__(self, name, value):
        setattr(self._inner, name, value)


class LoopbackComm:
    """Stands in for the block neighbours on one device: every interior face receives this block's own opposite inner planes.  No
    `c_pass`: the Python form of the choreography runs."""

    def __init__(self, domain, ops):
        self.domain, self.ops = domain, ops

    def exchange(self, f, slot=None, what="all", axis_only=False):
        nd, x = self.domain.nd, f.data(slot)
        for d in range(nd):
            for side in (-1, 1):
                if self.domain.neighbor(d, side) is None or f.layout.ghost[d] == 0:
                    continue
                sbox, rbox = Communicator.ghost_ranges(f.layout, nd, d, side)
                buf = self.ops.new_array(Communicator._count(sbox))
                self.ops.pack(f.lc, x, buf, sbox[0], sbox[1])
                self.ops.unpack(f.lc, x, buf, rbox[0], rbox[1])


def _oracle(eligible=None):
    from oracle_ops import OracleOps

    if eligible is None:
        return OracleOps()

    class Probed(OracleOps):
        def two_stage_eligible(self, lu, lf, st, begin1, end1, begin2, end2):
            return eligible

        def rbgs_sweep_fused_boxes(self, lu, u_in, u_out, tmp, *rest):      # the one-pass kernel takes no scratch array
            return OracleOps.rbgs_sweep_fused_boxes(self, lu, u_in, u_out, u_in.clone() if tmp is None else tmp, *rest)

    return Probed()


# -- the passes of smoothers.py ------------------------------------------------------------------------------------------------------

def passes(rec, ops, dom, L, overlaps=(True,), ghost=1, rhs_ghost=0):
    """jacobi_pair, rbgs_sweep (tmp_planes_valid both ways) and overlapped_loop on one block, two calls each so that the change of roles
    shows; what each returns is logged beside the calls."""
    tops, comm = rec.wrap(ops, "ops"), rec.wrap(LoopbackComm(dom, ops), "comm")
    lay = FieldLayout.node(3, dom.ncells(L), ghost)
    layf = FieldLayout.node(3, dom.ncells(L), rhs_ghost, True, rhs_ghost > 0)
    A = laplace_fd(3, dom.h(L))
    w = 0.8 / A.diag
    S, S1, F, T = Field("S", L, lay, ops, 2, None), Field("R", L, lay, ops, 1, None), Field("F", L, layf, ops, 1, None), Field("T", L, lay, ops, 1, None)
    alt = ops.new_array(lay.size)
    ops.fill_random(S.data(0), 1)
    ops.fill_random(F.data(), 3)
    for t in (S.data(1), S1.data(), T.data(), alt):
        t.copy_(S.data(0))
    rec.name_field(S, "S")
    rec.name_field(S1, "R")
    rec.name_field(F, "F")
    rec.name_field(T, "tmp")
    rec.name(alt, "alt")
    if ghost > 1:
        b, e = dom.loop_bounds(lay)
        # by hand, not dom.interior_faces(): the tool also records from older commits of the package, which have no such method
        faces = [(d, s) for d in range(3) for s in (-1, 1) if dom.neighbor(d, s) is not None]
        rec.log("deep_halo_boxes returns", [smoothers.deep_halo_boxes(tops, dom, S, F, A, b, e, faces)])
    for overlap in overlaps:
        for _ in range(2):
            smoothers.jacobi_pair(tops, comm, dom, S, F, A, w, T, overlap=overlap)
            rec.log("jacobi_pair returns", [S.active])
        for valid in (False, True):
            for first in (0, 1):
                alt = smoothers.rbgs_sweep(tops, comm, dom, S1, F, A, w, alt, T, first, overlap=overlap, tmp_planes_valid=valid)
                rec.log("rbgs_sweep returns", [alt, S1.data()])
        b, e = dom.loop_bounds(lay)
        smoothers.overlapped_loop(tops, dom, b, e, lambda: comm.exchange(S, None, "ghost", True),
                                  lambda bb, ee: tops.axpby(S.lc, S.data(), T.lc, T.data(), 1.0, 1.0, bb, ee), overlap=overlap)


def single_block(rec, ops):
    """jacobi_pair with and without the folded correction, and jacobi_triple, on a block without neighbours; jacobi_triple on a block
    with neighbours does nothing."""
    L, dom = 3, RectDomain(3, (1, 1, 1), 0)
    tops, comm = rec.wrap(ops, "ops"), rec.wrap(LoopbackComm(dom, ops), "comm")
    lay, layf = FieldLayout.node(3, dom.ncells(L), 1), FieldLayout.node(3, dom.ncells(L), 0, False, False)
    A = laplace_fd(3, dom.h(L))
    w = 0.8 / A.diag
    S, F, T = Field("S", L, lay, ops, 2, None), Field("F", L, layf, ops, 1, None), Field("T", L, lay, ops, 1, None)
    Sc = Field("Sc", L - 1, FieldLayout.node(3, dom.ncells(L - 1), 1), ops, 1, None)
    ops.fill_random(S.data(0), 1)
    ops.fill_random(F.data(), 3)
    ops.fill_random(Sc.data(), 5)
    for f, role in ((S, "S"), (F, "F"), (T, "tmp"), (Sc, "Sc")):
        rec.name_field(f, role)
    smoothers.jacobi_pair(tops, comm, dom, S, F, A, w, T)
    rec.log("jacobi_pair returns", [S.active])
    smoothers.jacobi_pair(tops, comm, dom, S, F, A, w, T, correction_from=Sc)
    rec.log("jacobi_pair returns", [S.active])
    rec.log("jacobi_triple returns", [smoothers.jacobi_triple(tops, comm, dom, S, F, A, w, T), S.active])
    nb = RectDomain(3, (2, 2, 2), 5)
    rec.log("jacobi_triple returns", [smoothers.jacobi_triple(tops, rec.wrap(LoopbackComm(nb, ops), "comm"), nb, S, F, A, w, T), S.active])


# -- the solvers ---------------------------------------------------------------------------------------------------------------------

def _name_solver(rec, P):
    for attr in ("Solution", "RHS", "Residual", "_sweep_tmp", "_rb_tmp", "_pair_tmp"):
        for l, f in sorted(getattr(P, attr, {}).items()):
            rec.name_field(f, "%s%d" % (f.name, l))
    for attr in ("_sol_alt", "_rb_alt"):
        for l, t in sorted(getattr(P, attr, {}).items()):
            rec.name(t, "alt%d" % l)
    for attr in ("cgTmp0", "cgTmp1", "VecP", "VecGradP"):
        if hasattr(P, attr):
            rec.name_field(getattr(P, attr), attr)
    rec.name(P._cg_info, "cg_info")


def solver(rec, ops, cls, cfg):
    dom = RectDomain(cfg.nd, (1, 1, 1), 0, cfg.frag_len)
    P = cls(cfg, rec.wrap(ops, "ops"), dom, rec.wrap(Communicator(dom, ops), "comm"))
    _name_solver(rec, P)
    P.setup()
    _name_solver(rec, P)
    rec.log("Solve returns", [P.Solve(), P.log])


L4_FUSED = dict(fused_rbgs=True, fused_rbgs3=True, fused_prolong_min_points=1, fused_zero_start=True, fused_residual_restrict=True,
                fused_residual_norm=True)
L3 = dict(nd=3, min_level=1, max_level=4)

CPU = {}
for _tag, _el in (("", None), ("_eligible", True), ("_ineligible", False)):
    for _dname, _dom, _L in (("2x2x2_rank0", ((2, 2, 2), 0), 3), ("2x2x2_rank5", ((2, 2, 2), 5), 3), ("1x1x2_rank0", ((1, 1, 2), 0), 3),
                             ("thin_level1", ((2, 2, 2), 0), 1), ("thin_level0", ((2, 2, 2), 0), 0)):
        CPU["passes_%s%s" % (_dname, _tag)] = lambda rec, d=_dom, L=_L, el=_el: passes(rec, _oracle(el), RectDomain(3, *d), L)
    for _dname, _dom in (("2x2x2_rank5", ((2, 2, 2), 5)), ("1x1x2_rank0", ((1, 1, 2), 0))):
        CPU["deep_halo_%s%s" % (_dname, _tag)] = lambda rec, d=_dom, el=_el: passes(rec, _oracle(el), RectDomain(3, *d), 3, ghost=2, rhs_ghost=1)
CPU["single_block"] = lambda rec: single_block(rec, _oracle())
CPU["solver_l4_fused"] = lambda rec: solver(rec, _oracle(), SolverFromL4, ConfigL4(nd=3, min_level=2, max_level=5, **L4_FUSED))
CPU["solver_l4_plain"] = lambda rec: solver(rec, _oracle(), SolverFromL4, ConfigL4(nd=3, min_level=2, max_level=5, **{k: type(v)(0) for k, v in L4_FUSED.items()}))
CPU["solver_l3_rbgs_fmg"] = lambda rec: solver(rec, _oracle(), SolverFromL3, ConfigL3(
    smoother="rbgs", fused_rbgs=True, fmg=True, fused_prolong_min_points=1, fused_zero_start=True, stencil="scaled", restrict_scale=1.0, omega=1.0, bc_fn=4, rhs_fn=5, **L3))
CPU["solver_l3_jacobi"] = lambda rec: solver(rec, _oracle(), SolverFromL3, ConfigL3(
    smoother="jacobi", temporal_blocking=True, fused_smooth_residual=True, fused_coarse=True, **L3))
CPU["solver_l3_mcgs"] = lambda rec: solver(rec, __import__("multicolour_cases").oracle_mc(), SolverFromL3, ConfigL3(smoother="mcgs", **L3))

# level 7 of a 2 x 2 x 2 decomposition: 64-point rows, the shortest the one-pass kernels take -- the side-stream branch is what runs
GPU = {"passes_2x2x2_rank%d" % r: (lambda rec, hip, r=r: passes(rec, hip, RectDomain(3, (2, 2, 2), r), 7, overlaps=(True, False))) for r in (0, 5)}


def record_cpu(name):
    rec = Recorder()
    CPU[name](rec)
    return rec.events


def record_gpu(name, hip):
    import torch

    rec = Recorder(lambda: torch.cuda.current_stream(hip.device) == hip.side_stream())
    GPU[name](rec, hip)
    hip.synchronize()
    return rec.events


def path_of(kind, out=TRACES):
    return os.path.join(out, "%s.json" % kind)


def dump(traces, path):
    """{scenario: events} as one compact file, since the scenarios repeat most of each other's calls and the calls most of each other's
    arguments: `args` holds every distinct method name and argument once, `calls` every distinct call once as [method, [arguments], the
    rest of the event] in numbers of `args`, `scenarios` the numbers of each scenario's calls in order.  `--show NAME` prints one in full."""
    args, calls, seqs = {}, {}, {}

    def arg(v):
        return args.setdefault(json.dumps(v, separators=(",", ":")), len(args))      # by its text: 1 and true are two arguments

    for name, events in traces.items():
        seqs[name] = []
        for ev in plain(events):
            rest = {k: v for k, v in ev.items() if k not in "ca"}
            call = json.dumps([arg(ev["c"]), [arg(a) for a in ev["a"]]] + ([rest] if rest else []), separators=(",", ":"))
            seqs[name].append(calls.setdefault(call, len(calls)))
    calls = list(calls)
    with open(path, "w") as f:
        f.write('{"args":%s,\n"calls":[\n%s\n],\n"scenarios":{\n%s\n}}\n' % (
            "[%s]" % ",".join(args), ",\n".join(",".join(calls[i:i + 12]) for i in range(0, len(calls), 12)),
            ",\n".join('"%s":%s' % (n, json.dumps(q, separators=(",", ":"))) for n, q in seqs.items())))


def load(path):
    """{scenario: events} of a file written by `dump`."""
    with open(path) as f:
        d = json.load(f)
    calls = [dict({"c": d["args"][c[0]], "a": [d["args"][a] for a in c[1]]}, **(c[2] if len(c) > 2 else {})) for c in d["calls"]]
    return {name: [calls[i] for i in seq] for name, seq in d["scenarios"].items()}


def plain(events):
    """`events` of a recorder as `load` returns them (lists for tuples)."""
    return json.loads(json.dumps(events))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gpu", action="store_true", help="record the GPU scenarios (needs the built library and a GPU) instead of the CPU ones")
    ap.add_argument("--out", default=TRACES)
    ap.add_argument("--show", metavar="NAME", help="print the recorded trace of one scenario, a call per line, and stop")
    args = ap.parse_args()
    if args.show:
        for ev in load(path_of("gpu" if args.gpu else "cpu", args.out))[args.show]:
            print(json.dumps(ev, separators=(",", ":")))
        return
    os.makedirs(args.out, exist_ok=True)
    if args.gpu:
        from exastencils_amd.ops import HipOps

        hip = HipOps(0)
        got = {name: record_gpu(name, hip) for name in GPU}
    else:
        got = {name: record_cpu(name) for name in CPU}
    dump(got, path_of("gpu" if args.gpu else "cpu", args.out))
    for name, events in got.items():
        print("%-40s %6d events" % (name, len(events)))


if __name__ == "__main__":
    main()
