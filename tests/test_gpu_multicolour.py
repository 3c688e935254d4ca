"""Multi-colour loops on the MI355X: examg_stencil_op_coloured (k_stencil_coloured), examg_mcgs_sweep (k_mcgs_rowpair27 and the
colour loops one by one), their argument checks, and the two host drivers (SolverFromL3 with smoother="mcgs", the ExaSlang-4
interpreter) on top of them.

References (tests/multicolour_cases.py): the uncoloured loop of FoldOps / ExactOps out of place, then exactly the colour's points of
the box copied -- whole arrays are compared, inputs and coefficient arrays included, so a write outside the colour or the box fails.
Random data is compared bit for bit with FoldOps (it separates entry order, diagonal index and weight form); integer / dyadic data
with equality against ExactOps, for single loops: a chain of eight dependent loops leaves the exactly representable range (every
loop adds up to 10 fractional bits and a factor of ~80 in magnitude), so whole sweeps are compared on random data, with FoldOps and
with the eight coloured calls on the GPU.

Layouts: u with one ghost layer, rhs and coefficients with none, the destination with two ghost layers and rows padded to a multiple
of 4 -- an index formed with another argument's layout reads or writes another point.
Shapes: inner sizes (n0, 5, 6) with n0 in {3, 8, 63, 64, 65, 127, 129, 255}: odd and even row counts per (y, z) parity, lattice rows
from one point to just past one, two and four waves of the row-pair kernel's 64-point tiles (129 and 255 inner points: 65 and 128
points of a colour); 2-D (65, 9).  Boxes [1, 1, 1) .. inner and [2, 1, 3) .. inner - 1: odd and even starts in x and z; an empty box
and a box of one row."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import multicolour_cases as M  # noqa: E402
import stencil_cases as S  # noqa: E402
from stencil_cases import APPLY, RESIDUAL, SMOOTH  # noqa: E402
from test_gpu_kernels import hip, hipd  # noqa: E402,F401  (fixtures)

from exastencils_amd.field import Colouring, Stencil  # noqa: E402
from exastencils_amd.layout import FieldLayout  # noqa: E402
from exastencils_amd.lib import ExamgError  # noqa: E402

pytestmark = pytest.mark.gpu

N0 = [3, 8, 63, 64, 65, 127, 129, 255]
DATA = ["random", "exact"]
OMEGA = 0.713
FOLD, EXACT = M.FoldMC(), M.ExactMC()


def ref_ops(data):
    return EXACT if data == "exact" else FOLD


def layouts(nd, inner):
    """(u, rhs, destination, coefficient) layouts of a block with `inner` inner points per dimension."""
    cells = tuple(inner[d] + 1 if d < nd else 0 for d in range(3))
    return (FieldLayout.node(nd, cells, 1), FieldLayout.node(nd, cells, 0, True, False), FieldLayout.node(nd, cells, 2, align=4),
            FieldLayout.node(nd, cells, 0, True, False))


def boxes(nd, inner, extra=False):
    """[1, 1, 1) .. inner, [2, 1, 3) .. inner - 1 (2-D: [2, 3) .. inner - 1); with `extra` an empty box and a box of one row."""
    z = nd == 3
    hi = [inner[d] + 1 if d < nd else 1 for d in range(3)]
    out = [([1, 1, 1 if z else 0], list(hi)),
           ([2, 1, 3] if z else [2, 3, 0], [hi[0] - 1, hi[1] - 1, hi[2] - 1 if z else 1])]
    if extra:
        out.append(([3, 1, 1 if z else 0], [3, hi[1], hi[2]]))
        out.append(([1, 2, 3 if z else 0], [hi[0], 3, 4 if z else 1]))
    return out


def host_data(size, data, seed):
    if data == "exact":
        return S.int_field(size, seed)
    return np.random.default_rng(seed).uniform(-1.0, 1.0, int(size))


class Case:
    """The host data of one case: u, rhs, destination over their whole allocations and the stencil (constant, or a coefficient field in
    planes); `on(ops, records)` puts it on a kernel layer -- the library gets the coefficient field in planes or, transformed by
    examg_transform_stencilfield, in records."""

    def __init__(self, nd, inner, kind, data, wform=0, seed=500):
        self.nd, self.data, self.kind = nd, data, kind
        self.lu, self.lf, self.ld, self.lc = layouts(nd, inner)
        self.u, self.f, self.d = (host_data(l.size, data, seed + i) for i, l in enumerate((self.lu, self.lf, self.ld)))
        self.cf = None
        if kind == "const27":
            self.st = S.exact27() if data == "exact" else S.random27()
        elif kind == "const27perm":
            self.st = S.exact27("perm") if data == "exact" else S.random27("perm")
        elif kind == "nine":
            self.st = M.nine_point(data)
        elif kind == "star7":
            self.st = S.exact7("pm") if data == "exact" else S.convdiff7(tuple(i + 1 for i in inner), "pm")
        else:
            if kind == "h27_shuffled":      # the centre first, the other 26 entries in another order than examg_init_helmholtz27's
                rest = S.field_offsets("h27")[1:]
                self.offsets = [(0, 0, 0)] + [rest[i] for i in np.random.default_rng(26).permutation(26)]
            else:
                self.offsets = S.field_offsets(kind)
            self.cf = S.coefficient_array(self.offsets, self.lc, data, seed + 7)
            self.wform = wform
        self.w = S.EXACT_W if data == "exact" else (OMEGA if self.cf is not None else S.free_weight(self.st))

    def on(self, ops, records=False):
        u, f, d = (ops.from_host(a.copy()) for a in (self.u, self.f, self.d))
        if self.cf is None:
            return u, f, d, self.st
        st = Stencil(list(self.offsets), [], ops.from_host(self.cf.copy()), self.lc, 0, self.wform)
        if records:
            planes, st = st, st.entry_fastest(ops)
            assert st.ctransform == 1 and st.cfield is not planes.cfield
        return u, f, d, st


def arrays(ops, u, f, d, st):
    ops.synchronize()
    out = [np.array(ops.to_host(t), dtype=np.float64, copy=True) for t in (u, f, d)]
    if st.cfield is not None:
        c = np.array(ops.to_host(st.cfield), dtype=np.float64, copy=True)
        if st.ctransform == 1:          # `[x, y, z, i] => [i, x, y, z]` of the same values
            c = c.reshape(-1, len(st.offsets)).T.reshape(-1)
        out.append(c)
    return out


def assert_same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            dd = np.abs(g - w)
            raise AssertionError("%s[%d]: %d of %d values differ, max abs %.3e" % (what, i, int((dd > 0).sum()), dd.size, np.nanmax(dd)))


def coloured(ops, case, mode, col, b, e, records=False, in_place=None):
    """One coloured loop from fresh data; SMOOTH in place when the colouring decouples the stencil, everything else into d."""
    u, f, d, st = case.on(ops, records)
    if in_place is None:
        in_place = mode == SMOOTH and col.decouples(st.offsets)
    lu, lf, ld = case.lu.c_struct(), case.lf.c_struct(), case.ld.c_struct()
    if in_place:
        ops.stencil_op_coloured(mode, lu, u, lf, f, lu, u, st, case.w, col, b, e)
    else:
        ops.stencil_op_coloured(mode, lu, u, lf, f, ld, d, st, case.w, col, b, e)
    return arrays(ops, u, f, d, st)


def check_colouring(gpu, case, colouring, bxs, records=False, what=""):
    R = ref_ops(case.data)
    for b, e in bxs:
        for mode in (APPLY, RESIDUAL, SMOOTH):
            for col in M.colours_in_order(colouring):
                got = coloured(gpu, case, mode, col, b, e, records)
                want = coloured(R, case, mode, col, b, e)
                assert_same(got, want, "%s %s %s mode %d colour %r box %r..%r" % (what, case.kind, case.data, mode, col.rem, b, e))


# -- examg_stencil_op_coloured: the generic coloured kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("kind", ["const27", "h27-planes", "h27-records", "h27_perm-records"])
@pytest.mark.parametrize("n0", N0)
def test_eight_colours_of_27_point_loops(hip, n0, kind, data):
    """pins k_stencil_coloured under `i0 % 2, i1 % 2, i2 % 2`: the three loop kinds, constant stencils and stencil fields in planes
    and in records (the diagonal first, and elsewhere in the entry list), every colour from fresh data."""
    inner = (n0, 5, 6)
    name, _, lay = kind.partition("-")
    case = Case(3, inner, name, data, wform=(n0 % 2))
    check_colouring(hip, case, M.AXIS8, boxes(3, inner, extra=(n0 == 65)), records=(lay == "records"), what="8 colours")


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("colouring", [M.AXIS4, M.AXIS9], ids=["i0%2,i1%2", "i0%3,i1%3"])
def test_nine_point_loops_in_2d(hip, colouring, data):
    inner = (65, 9, 1)
    check_colouring(hip, Case(2, inner, "nine", data), colouring, boxes(2, inner, extra=True), what="2-D")
    check_colouring(hip, Case(2, inner, "vc5", data, wform=1), colouring, boxes(2, inner), what="2-D field")


@pytest.mark.parametrize("data", DATA)
def test_mixed_colouring_row_start_and_stride(hip, data):
    """`(1 + i0 + i1) % 3, (1 + i2) % 2`: an expression over two axes that include x (a start and a stride per row), a lattice in z,
    shifts; it decouples the 7-point star (in place) and not the 27-point stencil (out of place)."""
    for n0 in (8, 65):
        inner = (n0, 5, 6)
        check_colouring(hip, Case(3, inner, "star7", data), M.MIXED, boxes(3, inner), what="mixed")
        check_colouring(hip, Case(3, inner, "const27perm", data), M.MIXED, boxes(3, inner)[1:], what="mixed")
    # expressions that are predicates only: (i1 + i2) % 2 has no x; a second expression on the x axis after the first made the lattice
    col = Colouring((((1, 2), 0, 2), ((0,), 1, 2), ((0,), 0, 3)))
    check_colouring(hip, Case(3, (65, 5, 6), "const27", data), col, boxes(3, (65, 5, 6))[:1], what="predicates")


@pytest.mark.parametrize("n0", [8, 63, 64, 65, 129])
def test_parity_colouring_equals_stencil_op(hip, n0):
    """nexpr == 1, all axes, mod 2: the bits of examg_stencil_op(colour) -- on rows of 64 points and more that is the z-marching
    kernel, which the coloured entry point reaches by forwarding."""
    inner = (n0, 5, 6)
    case = Case(3, inner, "star7", "random")
    lu, lf = case.lu.c_struct(), case.lf.c_struct()
    for b, e in boxes(3, inner):
        for shift in (0, 1):
            for rem in (0, 1):
                u, f, d, st = case.on(hip)
                hip.stencil_op_coloured(SMOOTH, lu, u, lf, f, lu, u, st, case.w, Colouring((((0, 1, 2), shift, 2),), (rem,)), b, e)
                got = arrays(hip, u, f, d, st)
                u, f, d, st = case.on(hip)
                hip.stencil_op(SMOOTH, lu, u, lf, f, lu, u, st, case.w, (rem - shift) % 2, b, e)
                assert_same(got, arrays(hip, u, f, d, st), "parity shift %d rem %d" % (shift, rem))
                want = coloured(FOLD, case, SMOOTH, Colouring((((0, 1, 2), shift, 2),), (rem,)), b, e)
                assert_same(got, want, "parity against the definition, shift %d rem %d" % (shift, rem))


@pytest.mark.parametrize("data", DATA)
def test_out_of_place_apply_under_a_colouring_that_does_not_decouple(hip, data):
    inner = (65, 5, 6)
    case = Case(3, inner, "const27", data)
    assert not M.PARITY3.decouples(case.st.offsets)
    for b, e in boxes(3, inner):
        for col in M.colours_in_order(M.PARITY3) + M.colours_in_order(Colouring((((0,), 0, 2),))):
            got = coloured(hip, case, APPLY, col, b, e)
            assert_same(got, coloured(ref_ops(data), case, APPLY, col, b, e), "apply %r" % (col,))


# -- examg_mcgs_sweep --------------------------------------------------------------------------------------------------------------------
def sweep(ops, case, colouring, b, e, records, loops=False):
    u, f, d, st = case.on(ops, records)
    lu, lf = case.lu.c_struct(), case.lf.c_struct()
    if loops:
        for col in M.colours_in_order(colouring):
            ops.stencil_op_coloured(SMOOTH, lu, u, lf, f, lu, u, st, case.w, col, b, e)
    else:
        ops.mcgs_sweep(lu, u, lf, f, st, case.w, colouring, b, e)
    return arrays(ops, u, f, d, st)


@pytest.mark.parametrize("wform", [0, 1], ids=["inv_times", "divide"])
@pytest.mark.parametrize("kind", ["h27", "h27_shuffled"])
@pytest.mark.parametrize("n0", N0)
def test_row_pair_sweep(hip, hipd, n0, kind, wform):
    """pins k_mcgs_rowpair27 (the entry order of examg_init_helmholtz27, and another order with the centre first): the product
    library takes it for the record layout (examg_mcgs_one_pass_eligible == 1) and not for
    planes; its result is that of the eight coloured calls and of FoldOps, bit for bit; the debug build's per-colour path gives the
    same bits; two runs from the same input give identical arrays."""
    inner = (n0, 5, 6)
    case = Case(3, inner, kind, "random", wform=wform)
    lu, lf = case.lu.c_struct(), case.lf.c_struct()
    for b, e in boxes(3, inner, extra=(n0 == 65)):
        empty = any(e[k] <= b[k] for k in range(3))
        _, _, _, rec = case.on(hip, True)
        _, _, _, planes = case.on(hip, False)
        assert hip.mcgs_one_pass_eligible(lu, lf, rec, M.AXIS8, b, e) == (not empty)
        assert not hip.mcgs_one_pass_eligible(lu, lf, planes, M.AXIS8, b, e)
        assert not hip.mcgs_one_pass_eligible(lu, lf, rec, M.MIXED, b, e)
        got = sweep(hip, case, M.AXIS8, b, e, True)
        want = sweep(FOLD, case, M.AXIS8, b, e, False)
        assert_same(got, want, "row pairs against FoldOps, box %r..%r" % (b, e))
        assert_same(got, sweep(hip, case, M.AXIS8, b, e, True, loops=True), "row pairs against the eight coloured calls")
        assert_same(got, sweep(hip, case, M.AXIS8, b, e, True), "second run")
        assert_same(sweep(hip, case, M.AXIS8, b, e, False), want, "planes: the colour loops one by one")
        old = hipd.L.examg_debug_mcgs_per_colour(1)
        try:
            assert not hipd.mcgs_one_pass_eligible(lu, lf, rec, M.AXIS8, b, e)
            assert_same(sweep(hipd, case, M.AXIS8, b, e, True), want, "per-colour path of the debug build")
        finally:
            hipd.L.examg_debug_mcgs_per_colour(old)
        assert hipd.mcgs_one_pass_eligible(lu, lf, rec, M.AXIS8, b, e) == (not empty)
        assert_same(sweep(hipd, case, M.AXIS8, b, e, True), want, "row pairs, debug build")
    # shifted parities: the colours start on other points, the pairs stay pairs
    col = Colouring((((0,), 1, 2), ((1,), 0, 2), ((2,), 3, 2)))
    b, e = boxes(3, inner)[1]
    _, _, _, rec = case.on(hip, True)
    assert hip.mcgs_one_pass_eligible(lu, lf, rec, col, b, e)
    assert_same(sweep(hip, case, col, b, e, True), sweep(FOLD, case, col, b, e, False), "shifted parities")


@pytest.mark.parametrize("kind,colouring,nd,inner", [("const27", M.AXIS8, 3, (65, 5, 6)), ("h27_perm", M.AXIS8, 3, (64, 5, 6)),
                                                     ("nine", M.AXIS9, 2, (65, 9, 1)), ("nine", M.AXIS4, 2, (65, 9, 1)),
                                                     ("star7", M.PARITY3, 3, (65, 5, 6)), ("star7", M.MIXED, 3, (65, 5, 6))],
                         ids=["const27", "h27_perm-records", "nine-9", "nine-4", "star7-parity", "star7-mixed"])
def test_sweeps_without_the_row_pair_kernel(hip, kind, colouring, nd, inner):
    """Constant stencils, a record field whose diagonal is not the first entry, 2-D and other colourings: the colour loops one by one
    in the reference's order, the result FoldOps' bit for bit."""
    case = Case(nd, inner, kind, "random")
    lu, lf = case.lu.c_struct(), case.lf.c_struct()
    for b, e in boxes(nd, inner):
        _, _, _, st = case.on(hip, True)
        assert not hip.mcgs_one_pass_eligible(lu, lf, st, colouring, b, e)
        got = sweep(hip, case, colouring, b, e, True)
        assert_same(got, sweep(FOLD, case, colouring, b, e, False), "%s sweep" % kind)
        assert_same(got, sweep(hip, case, colouring, b, e, True, loops=True), "%s sweep against its loops" % kind)


# -- argument checks: all of them return before any launch (the arrays are compared afterwards) -----------------------------------------
def test_argument_checks(hip):
    from exastencils_amd import lib

    inner = (8, 5, 6)
    case = Case(3, inner, "const27", "random")
    u, f, d, st = case.on(hip)
    before = arrays(hip, u, f, d, st)
    lu, lf, ld = case.lu.c_struct(), case.lf.c_struct(), case.ld.c_struct()
    b, e = boxes(3, inner)[0]

    def raw(nexpr, axes, shift, mod, rem):
        c = lib.ColouringC()
        c.nexpr = nexpr
        for k in range(3):
            c.axes[k], c.shift[k], c.mod[k], c.rem[k] = axes[k], shift[k], mod[k], rem[k]

        class Raw:
            @staticmethod
            def c_struct():
                return c

        return Raw

    good = dict(axes=(1, 2, 4), shift=(0, 0, 0), mod=(2, 2, 2), rem=(0, 0, 0))
    bad = [
        ("nexpr", raw(0, **good)), ("nexpr", raw(4, **good)),
        ("mod must be positive", raw(3, **dict(good, mod=(2, 0, 2)))), ("mod must be positive", raw(3, **dict(good, mod=(2, 2, -2)))),
        ("rem must lie", raw(3, **dict(good, rem=(0, 2, 0)))), ("rem must lie", raw(3, **dict(good, rem=(-1, 0, 0)))),
        ("axes", raw(3, **dict(good, axes=(1, 0, 4)))), ("axes", raw(3, **dict(good, axes=(1, 2, 8)))),
        ("can be negative", raw(3, **dict(good, shift=(0, -2, 0)))),
    ]
    for what, col in bad:
        with pytest.raises(ExamgError, match=what):
            hip.stencil_op_coloured(SMOOTH, lu, u, lf, f, ld, d, st, case.w, col, b, e)
        if "rem" not in what:
            with pytest.raises(ExamgError, match=what):
                hip.mcgs_sweep(lu, u, lf, f, st, case.w, col, b, e)
    # a negative start of the box itself: a layout with two ghost layers has room for it, the remainder has no meaning there
    l2 = FieldLayout.node(3, (9, 6, 7), 2)
    with pytest.raises(ExamgError, match="can be negative"):
        hip.stencil_op_coloured(APPLY, l2.c_struct(), hip.new_array(l2.size), None, None, ld, d, st, 0.0, next(M.AXIS8.colours()), [-1, 0, 0], [4, 4, 4])
    # aliasing without decoupling: the parity of all indices and a 27-point stencil; i0 % 2, i1 % 2 in 3-D
    for col in (M.PARITY3, M.AXIS4):
        with pytest.raises(ExamgError, match="does not decouple"):
            hip.stencil_op_coloured(SMOOTH, lu, u, lf, f, lu, u, st, case.w, next(col.colours()), b, e)
        with pytest.raises(ExamgError, match="does not decouple"):
            hip.mcgs_sweep(lu, u, lf, f, st, case.w, col, b, e)
    # a colour-split layout
    split = case.lu.split_x().c_struct()
    us = hip.new_array(case.lu.split_x().size)
    with pytest.raises(ExamgError, match="colour-split"):
        hip.stencil_op_coloured(APPLY, split, us, None, None, ld, d, st, 0.0, next(M.AXIS8.colours()), b, e)
    with pytest.raises(ExamgError, match="colour-split"):
        hip.mcgs_sweep(split, us, lf, f, st, case.w, M.AXIS8, b, e)
    # a box that leaves an allocation
    with pytest.raises(ExamgError, match="leaves the u allocation"):
        hip.stencil_op_coloured(APPLY, lu, u, None, None, ld, d, st, 0.0, next(M.AXIS8.colours()), [0, 0, 0], [12, 4, 4])
    assert_same(arrays(hip, u, f, d, st), before, "after the refused calls")
    assert not hip.mcgs_one_pass_eligible(lu, lf, st, raw(0, **good), b, e)


# -- the drivers ----------------------------------------------------------------------------------------------------------------------
def test_solver_with_the_multicolour_smoother_eager_and_from_its_graph(hip):
    """SolverFromL3(smoother="mcgs") on the 27-entry Helmholtz record field: the residual history of the oracle-backed run of the same
    configuration (1e-10 relative, test_gpu_solver's rule), eager and replayed from the captured hipGraph; the sweeps of the levels
    with a stencil field are row-pair sweeps."""
    from test_gpu_solver import _close
    from test_multicolour import MCGS27

    from exastencils_amd.solver import ConfigL3, SolverFromL3

    kw = dict(MCGS27, max_level=4, coef_entry_fastest=True, fused_coarse=True)
    O = SolverFromL3(ConfigL3(frag_len=(2, 2, 2), **kw), M.oracle_mc())
    O.setup()
    O.Solve()
    P = SolverFromL3(ConfigL3(frag_len=(2, 2, 2), **kw), hip)
    P.setup()
    P.Solve()
    S4, F4 = P.Solution[4], P.RHS[4]
    b, e = P.bounds(S4)
    assert hip.mcgs_one_pass_eligible(S4.lc, F4.lc, P.Laplace[4], Colouring.axis_parity(3), b, e)
    print("mcgs history gpu", P.res_history, "oracle", O.res_history)
    assert P.iterations == O.iterations
    _close(P.res_history, O.res_history)
    assert P.err_history[-1] < 1e-8
    G = SolverFromL3(ConfigL3(frag_len=(2, 2, 2), **kw), hip)
    G.setup()
    G.capture()
    G.Solve(use_graph=True)
    assert G.res_history == P.res_history
    assert np.array_equal(hip.to_host(G.Solution[4].data()), hip.to_host(P.Solution[4].data()))
    _close(G.res_history, O.res_history)


def test_example_program_on_gpu(hip):
    """examples/exa4/helmholtz3d_gs8.exa4 prints on the GPU what it prints on the oracle-backed kernel layer (norms: the device
    reduction tree sums in another order -- test_gpu_exa4's rule), with and without the one-call sweep bit for bit."""
    from test_gpu_exa4 import _close
    from test_multicolour import run_example

    O = run_example(M.oracle_mc(), 1, 4)
    P = run_example(hip, 1, 4)
    print("gs8 gpu", P.printed_values, "oracle", O.printed_values)
    assert P.fusions.get("mcgs_sweep", 0) > 0 and len(P.printed_values) > 3
    _close(P.printed_values, O.printed_values, O.printed_values[0])
    Q = run_example(hip, 1, 4, fuse=False, fuse_coarse_solver=True)
    assert Q.fusions.get("mcgs_sweep", 0) == 0 and Q.printed_values == P.printed_values


# -- transport: mcgs with a z neighbour ---------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


PEER_CASE = dict(nd=3, min_level=1, max_level=4, smoother="mcgs", omega=0.9, stencil="helmholtz27", restrict_scale=1.0, tol=1e-8, cg_max=512, bc_fn=0,
                 sol_fn=9, coef_fn=7, kappa=10.0, ksq=2.0, rhs_from_solution=True, coef_entry_fastest=True)


def test_sweeps_on_two_blocks_are_the_single_block_bit_for_bit(hip, tmp_path):
    """Two processes on the one device, a z neighbour each, peer-write transport: four sweeps of SolverFromL3(smoother="mcgs") on the
    finest level -- `communicate` before every colour loop, the generic coloured kernel -- leave the bits of the single block's four
    examg_mcgs_sweep calls (row pairs).  The grid widths are powers of two, so both decompositions compute the same coefficients."""
    from exastencils_amd.solver import ConfigL3, SolverFromL3

    hi = PEER_CASE["max_level"]
    P = SolverFromL3(ConfigL3(frag_len=(2, 2, 2), **PEER_CASE), hip)
    P.setup()
    for _ in range(4):
        P.Smoother(hi)
    S_ = P.Solution[hi]
    lay, n = S_.layout, 2 << hi
    a = hip.to_host(S_.data()).reshape(lay.shape_zyx)
    want = a[tuple(slice(lay.ref(k), lay.ref(k) + n + 1) for k in (2, 1, 0))].copy()
    assert np.abs(want).max() > 0

    d = str(tmp_path)
    json.dump({"mcgs": PEER_CASE, "sweeps": 4}, open(os.path.join(d, "cases.json"), "w"))
    port = _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", EXAMG_PEER_TIMEOUT_MS="30000")
    env.pop("EXAMG_TRANSPORT", None)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "mcgs_peer_worker.py"), str(r), "2", "1,1,2", str(port), d, "mcgs"],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, cwd=ROOT) for r in range(2)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=240)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("mcgs peer workers timed out")
    for r, (p, log) in enumerate(zip(procs, logs)):
        assert p.returncode == 0, "rank %d:\n%s" % (r, log[-3000:])
    for r in range(2):
        o = json.load(open(os.path.join(d, "mcgs_%d.json" % r)))
        assert o["transport"] == "peer" and o["exchanges"] > 0
        got = np.load(os.path.join(d, "mcgs_%d.npy" % r))
        piece = want[r * (n // 2): r * (n // 2) + n // 2 + 1]
        assert got.shape == piece.shape
        assert np.array_equal(got, piece), "rank %d differs from the single block (max abs %.3e)" % (r, np.abs(got - piece).max())
