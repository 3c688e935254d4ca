"""Multi-colour `color with` (several colour expressions, or one that is not the parity of all indices) on the CPU: parser, colour
order, the decoupling predicate, the refusals, and the two host drivers -- the ExaSlang-4 interpreter on
examples/exa4/helmholtz3d_gs8.exa4 and SolverFromL3(smoother="mcgs") -- against hand-written drivers that issue the colour loops one
by one through the same kernel layer (the oracle's loops behind tests/multicolour_cases.py's mixin)."""
import math
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import multicolour_cases as M  # noqa: E402
import stencil_cases as S  # noqa: E402

from exastencils_amd import exa4  # noqa: E402
from exastencils_amd.exa4_parser import _colour_expr  # noqa: E402
from exastencils_amd.field import Colouring, laplace_fd  # noqa: E402
from exastencils_amd.lib import ExprC  # noqa: E402

EX = os.path.join(ROOT, "examples", "exa4")


# -- parser -----------------------------------------------------------------------------------------------------------------------
def test_parser_accepts_the_written_forms():
    pr = exa4.Parser("Function F { color with { i0 % 2, ( i0 + i1 ) % 3, ( 1 + i2 ) % 2, loop over u { } } }").parse()
    kind, exprs, body = pr.functions[0].body[0]
    assert kind == "color" and len(exprs) == 3 and body[0][0] == "loop"
    assert [_colour_expr(e, 3) for e in exprs] == [((0,), 0, 2), ((0, 1), 0, 3), ((2,), 1, 2)]
    # the axes must exist, every index at most once, the modulus a positive integer constant
    assert _colour_expr(exprs[2], 2) is None
    for text in ("( i0 + i0 ) % 2", "( 2 * i0 ) % 2", "i0 % 0", "i0 % n", "3 % 2", "i0 + i1"):
        e = exa4.Parser("Function F { color with { %s, loop over u { } } }" % text).parse().functions[0].body[0][1][0]
        assert _colour_expr(e, 3) is None, text


# -- programs -----------------------------------------------------------------------------------------------------------------------
HEADER2 = """
Domain global< [0.0, 0.0] to [1.0, 1.0] >
Layout L< Real, Node >@all { duplicateLayers = [1, 1] with communication
 ghostLayers = [1, 1] with communication }
Field u< global, L, 0.0 >@all
Field f< global, L, None >@all
Stencil A@all { [0, 0] => 4.0
 [1, 0] => -1.0
 [-1, 0] => -1.0
 [0, 1] => -1.0
 [0, -1] => -1.0 }
Stencil B@all { [0, 0] => 8.0
 [1, 0] => -1.0
 [-1, 0] => -1.0
 [0, 1] => -1.0
 [0, -1] => -1.0
 [1, 1] => -1.0
 [-1, 1] => -1.0
 [1, -1] => -1.0
 [-1, -1] => -1.0 }
"""
SMOOTH_A = "loop over u@finest { u@finest += 0.8 / diag ( A@finest ) * ( f@finest - A@finest * u@finest ) }"
SMOOTH_B = "loop over u@finest { u@finest += 0.8 / diag ( B@finest ) * ( f@finest - B@finest * u@finest ) }"


class _Recorder:
    """The oracle-backed layer, recording every coloured call."""

    def __new__(cls):
        base = type(M.oracle_mc())

        class Rec(base):
            def __init__(self):
                super().__init__()
                self.calls = []

            def stencil_op_coloured(self, mode, lu, u, lf, rhs, ld, dst, st, w, col, begin, end):
                self.calls.append((mode, col.exprs, col.rem))
                super().stencil_op_coloured(mode, lu, u, lf, rhs, ld, dst, st, w, col, begin, end)

        return Rec()


def test_colour_loops_run_in_the_reference_order():
    """`color with { i0 % 2, i1 % 3, .. }`: the first expression varies fastest (L4_ColorLoops.toRepeatLoops)."""
    ops = _Recorder()
    text = HEADER2 + "Function Application { color with { i0 %% 2, i1 %% 3, communicate u@finest\n %s\n apply bc to u@finest } }" % SMOOTH_A
    exa4.Exa4Program(text, dict(dimensionality=2, minLevel=0, maxLevel=3), ops=ops, fuse=False).run()
    assert [c[2] for c in ops.calls] == [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2)]
    assert all(c[0] == S.SMOOTH and c[1] == (((0,), 0, 2), ((1,), 0, 3)) for c in ops.calls)
    # the value type and the test helper agree on it
    col = Colouring((((0,), 0, 2), ((1,), 0, 3)))
    assert [c.rem for c in col.colours()] == [c.rem for c in M.colours_in_order(col)] == [c[2] for c in ops.calls]
    assert [c.rem for c in M.AXIS8.colours()][:5] == [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1)]


def test_one_block_sweep_is_one_call_and_the_same_bits():
    """The peephole: the whole `color with` as one mcgs_sweep; same field as the colour loops one by one."""
    import numpy as np

    text = HEADER2 + ("Function Application { loop over f@finest { f@finest = vf_nodePos_x + ( 2.0 * vf_nodePos_y ) }\n apply bc to u@finest\n"
                      "repeat 2 times { color with { i0 %% 2, i1 %% 2, communicate u@finest\n %s\n apply bc to u@finest } } }" % SMOOTH_B)
    out = []
    for fuse in (True, False):
        ops = _Recorder()
        P = exa4.Exa4Program(text, dict(dimensionality=2, minLevel=0, maxLevel=3), ops=ops, fuse=fuse)
        P.run()
        assert P.fusions.get("mcgs_sweep", 0) == (2 if fuse else 0) and len(ops.calls) == 8
        out.append(ops.to_host(P.fields[("u", 3)].data()).copy())
    assert np.array_equal(out[0], out[1]) and np.abs(out[0]).max() > 0


# -- decoupling -------------------------------------------------------------------------------------------------------------------
def test_decoupling_predicate():
    star7, star5 = laplace_fd(3, (0.1, 0.1, 0.1)), laplace_fd(2, (0.1, 0.1))
    cases = [
        (M.PARITY3, star7.offsets, True), (M.AXIS8, star7.offsets, True), (M.PARITY2, star5.offsets, True),
        (M.PARITY3, S.random27().offsets, False), (M.AXIS8, S.random27().offsets, True), (M.AXIS8, S.random27("perm").offsets, True),
        (M.AXIS4, M.nine_point().offsets, True), (M.AXIS9, M.nine_point().offsets, True), (M.PARITY2, M.nine_point().offsets, False),
        (M.AXIS4, S.random27().offsets, False),                       # (0, 0, 1) changes neither i0 % 2 nor i1 % 2
        (Colouring((((0,), 0, 2),)), star5.offsets, False),           # i0 % 2 alone: (0, 1) stays in its colour
        (M.MIXED, star7.offsets, True), (M.MIXED, S.random27().offsets, False),      # (1, -1, 0): i0 + i1 unchanged, i2 unchanged
        (Colouring((((0,), 0, 3), ((1,), 0, 3))), [(0, 0, 0), (3, 0, 0)], False),   # reach 3 under mod 3
    ]
    for col, offs, want in cases:
        assert col.decouples(offs) is want, (col, want)
        assert M.decouples(col.exprs, offs) is want


def test_colouring_value_type():
    c = Colouring((((0, 2), 5, 3), ((1,), 0, 2)), (2, 1)).c_struct()
    assert (c.nexpr, list(c.axes)[:2], list(c.shift)[:2], list(c.mod)[:2], list(c.rem)[:2]) == (2, [5, 2], [5, 0], [3, 2], [2, 1])
    assert Colouring.axis_parity(3) == M.AXIS8 and Colouring.axis_parity(2) == M.AXIS4
    assert Colouring((((0, 1, 2), 1, 2),), (0,)).parity_colour(3) == 1 and M.AXIS8.parity_colour(3) is None
    for bad in ((), (((0,), 0, 2),) * 4, (((), 0, 2),), (((0, 0), 0, 2),), (((3,), 0, 2),), (((0,), 0, 0),)):
        with pytest.raises(ValueError):
            Colouring(bad)
    with pytest.raises(ValueError):
        Colouring((((0,), 0, 2),), (2,))


# -- refusals ---------------------------------------------------------------------------------------------------------------------
CELL_HEADER = """
Domain global< [0.0, 0.0] to [1.0, 1.0] >
Layout C< Real, Cell >@all { duplicateLayers = [0, 0]
 ghostLayers = [1, 1] with communication }
Field c< global, C, 0.0 >@all
Field b< global, C, None >@all
Stencil K@all { [0, 0] => 4.0
 [1, 0] => -1.0
 [-1, 0] => -1.0
 [0, 1] => -1.0
 [0, -1] => -1.0 }
"""
SPLIT = "LayoutTransformations {\n  transform u@finest with [x, y] => [x / 2, y, x % 2]\n}\n\n"


@pytest.mark.parametrize("header,colours,body,what", [
    (HEADER2, "i0 % 2, i1 % 2", "loop over u@finest { u@finest = 0.0 }", "only stencil loops"),
    (HEADER2, "i0 % 2, i1 % 2", "loop over u@finest { u@finest += f@finest }", "only stencil loops"),
    (HEADER2, "i0 % 2, i1 % 2", "Var s : Real = 0.0\n loop over u@finest with reduction ( + : s ) { s += u@finest * u@finest }", "reduction loop"),
    (HEADER2, "i0 % 2, i1 % 2", "loop over u@finest only dup [1, 0] on boundary { u@finest = f@finest - A@finest * u@finest }", "only <region>"),
    (HEADER2, "i0 % 2, i1 % 2", "loop over u@finest where 0 == ( ( i0 + i1 ) % 2 ) { u@finest = f@finest - A@finest * u@finest }", "`where` colour test"),
    (CELL_HEADER, "i0 % 2, i1 % 2", "loop over c@finest { c@finest += 0.8 / diag ( K@finest ) * ( b@finest - K@finest * c@finest ) }", "cell fields"),
    (SPLIT + HEADER2, "i0 % 2, i1 % 2", SMOOTH_A, "colour-split field u"),
    (SPLIT + HEADER2, "i0 % 2, i1 % 2", "loop over f@finest { f@finest = A@finest * u@finest }", "colour-split field u"),
    (HEADER2, "i0 % 2", SMOOTH_A, "in-place smoother .* does not decouple"),
    (HEADER2, "( i0 + i1 ) % 3", "loop over u@finest { u@finest = f@finest - B@finest * u@finest }", "in-place residual loop .* does not decouple"),
    (HEADER2, "i0 % 2", "loop over u@finest { u@finest = A@finest * u@finest }", "in-place stencil application .* does not decouple"),
    (HEADER2, "( i0 + i1 ) % 2, i1 % 1", SMOOTH_B, "does not decouple"),
    (HEADER2, "( i0 + i1 ) % 3", SMOOTH_B, "does not decouple"),
    (HEADER2, "( 2 * i0 ) % 2, i1 % 2", SMOOTH_A, "colour expression other than"),
    (HEADER2, "i0 % 2, i2 % 2", SMOOTH_A, "colour expression other than"),
    (HEADER2, "i0 % 2, i1 % 2, i0 % 3, i1 % 3", SMOOTH_A, "more than three colour expressions"),
    (HEADER2, "i0 % 2, i1 % 2", "color with { i0 %% 3, i1 %% 3,\n %s }" % SMOOTH_A, "color with inside color with"),
])
def test_constructs_without_a_coloured_kernel_are_refused_by_name(header, colours, body, what):
    ops = M.oracle_mc()
    ops.transform_field = lambda *a: None      # a kernel layer with transformed layouts: the colour split is applied (no call is reached)
    text = header + "Function Application { color with { %s,\n %s } }" % (colours, body)
    for fuse in (True, False):
        with pytest.raises(exa4.Exa4Unsupported, match=what):
            exa4.Exa4Program(text, dict(dimensionality=2, minLevel=0, maxLevel=2), ops=ops, fuse=fuse).run()


def test_out_of_place_loops_run_under_any_colouring():
    """A * u and f - A * u into another field need no decoupling: nothing is read that the loop writes.  Every colour runs, and the
    colours together leave what the uncoloured loops leave."""
    import numpy as np

    fill = "loop over u@finest { u@finest = vf_nodePos_x + ( 2.0 * vf_nodePos_y ) }\n"
    loops = "loop over f@finest { f@finest = B@finest * u@finest }\n loop over f@finest { f@finest = f@finest - B@finest * u@finest }\n"
    out = []
    for coloured in (True, False):
        ops = _Recorder()
        body = "color with { ( i0 + i1 ) % 3,\n" + loops + "}" if coloured else loops
        P = exa4.Exa4Program(HEADER2 + "Function Application { " + fill + body + " }", dict(dimensionality=2, minLevel=0, maxLevel=3), ops=ops)
        P.run()
        if coloured:
            assert not Colouring((((0, 1), 0, 3),)).decouples(P.stencil("B", 3).offsets)
            assert [(c[0], c[2]) for c in ops.calls] == [(S.APPLY, (0,)), (S.RESIDUAL, (0,)), (S.APPLY, (1,)), (S.RESIDUAL, (1,)), (S.APPLY, (2,)),
                                                         (S.RESIDUAL, (2,))]
        out.append(ops.to_host(P.fields[("f", 3)].data()).copy())
    # per point: f = B u, then f = f - B u = 0 exactly, whatever the colour order; the uncoloured program gives the same zeros
    assert np.array_equal(out[0], out[1])


def test_peephole_takes_the_documented_statement_order_only():
    """`[communicate u] loop over u { .. } [apply bc to u]` is one sweep; the same statements in another order run one by one."""
    for body, fused in (("communicate u@finest\n %s\n apply bc to u@finest", True), ("%s", True), ("%s\n apply bc to u@finest", True),
                        ("apply bc to u@finest\n %s", False), ("%s\n communicate u@finest", False), ("%s\n %s", False),
                        ("communicate f@finest\n %s", False)):
        ops = _Recorder()
        text = HEADER2 + "Function Application { apply bc to u@finest\n color with { i0 %% 2, i1 %% 2,\n" + body.replace("%s", SMOOTH_B.replace("%", "%%")) + " } }"
        P = exa4.Exa4Program(text % (), dict(dimensionality=2, minLevel=0, maxLevel=2), ops=ops)
        P.run()
        assert (P.fusions.get("mcgs_sweep", 0) == 1) is fused, body


def test_parity_colouring_keeps_its_path():
    """One expression, all axes, % 2: the frame keeps the int colour and the loops go to stencil_op -- no coloured call."""
    ops = _Recorder()
    text = HEADER2 + "Function Application { color with { ( 1 + i0 + i1 ) %% 2, communicate u@finest\n %s } }" % SMOOTH_A
    P = exa4.Exa4Program(text, dict(dimensionality=2, minLevel=0, maxLevel=2), ops=ops, fuse=False)
    P.run()
    assert ops.calls == [] and P.launches == 2


# -- the example program against a hand-written driver ---------------------------------------------------------------------------------
RHS_PROGRAM = [("const", 4.0), ("x", None), ("x", None), ("*", None), ("const", 0.5), ("y", None), ("y", None), ("*", None), ("*", None),
               ("-", None), ("const", 0.5), ("z", None), ("z", None), ("*", None), ("*", None), ("-", None), ("*", None)]


def gs8_driver(ops, lo, hi, loop_by_loop=True):
    """examples/exa4/helmholtz3d_gs8.exa4 written out as kernel-layer calls: the declarations (fields, layouts, stencil values,
    boundary expressions) come from an interpreter instance that never runs; every statement of the program is issued here by
    hand -- the 8-colour sweep as its eight loops in the reference's order."""
    with open(os.path.join(EX, "helmholtz3d_gs8.exa4")) as f:
        Q = exa4.Exa4Program(f.read(), dict(dimensionality=3, minLevel=lo, maxLevel=hi), ops=ops, fuse=False)
    dom = Q.domain
    fld = lambda name, l: Q.fields[(name, l)]      # noqa: E731
    H = {l: Q.stencil("H", l) for l in range(lo, hi + 1)}
    printed = []

    def bounds(f, reduction=False):
        return dom.loop_bounds(f.layout, reduction)

    def defect(l):
        v, g, d = fld("v", l), fld("g", l), fld("d", l)
        b, e = bounds(d)
        ops.stencil_op(S.RESIDUAL, v.lc, v.data(), g.lc, g.data(), d.lc, d.data(), H[l], 0.0, -1, b, e)
        Q._apply_bc(d, d.active)

    def dot(x, y, over):
        b, e = bounds(over, True)
        return 0.0 + (0.0 + ops.scalar_value(ops.dot(x.lc, x.data(), y.lc, y.data(), b, e)))

    def norm(l):
        d = fld("d", l)
        return math.sqrt(dot(d, d, d))

    def sweeps(l):
        v, g = fld("v", l), fld("g", l)
        b, e = bounds(v)
        w = 0.9 / H[l].diag
        for _ in range(2):
            for r2 in (0, 1):
                for r1 in (0, 1):
                    for r0 in (0, 1):
                        col = Colouring((((0,), 0, 2), ((1,), 0, 2), ((2,), 0, 2)), (r0, r1, r2))
                        ops.stencil_op_coloured(S.SMOOTH, v.lc, v.data(), g.lc, g.data(), v.lc, v.data(), H[l], w, col, b, e)
                        Q._apply_bc(v, v.active)

    def cycle(l):
        if l == lo:
            return coarse(l)
        sweeps(l)
        defect(l)
        d, gc, vc, v = fld("d", l), fld("g", l - 1), fld("v", l - 1), fld("v", l)
        b, e = bounds(gc)
        ops.restrict(d.lc, d.data(), gc.lc, gc.data(), 1.0, b, e)
        b, e = bounds(vc)
        ops.set(vc.lc, vc.data(), 0.0, b, e)
        Q._apply_bc(vc, vc.active)
        cycle(l - 1)
        b, e = bounds(v)
        ops.prolong_add(vc.lc, vc.data(), v.lc, v.data(), b, e)
        Q._apply_bc(v, v.active)
        sweeps(l)

    def coarse(l):
        v, d, s, t = fld("v", l), fld("d", l), fld("s", l), fld("t", l)
        defect(l)
        rho = rho0 = norm(l)
        b, e = bounds(s)
        ops.axpby(d.lc, d.data(), s.lc, s.data(), 1.0, 0.0, b, e)
        Q._apply_bc(s, s.active)
        for _ in range(96):
            b, e = bounds(t)
            ops.stencil_op(S.APPLY, s.lc, s.data(), None, None, t.lc, t.data(), H[l], 0.0, -1, b, e)
            top = dot(d, d, d)
            bottom = dot(s, t, s)
            step = top / bottom
            b, e = bounds(v)
            ops.axpby(s.lc, s.data(), v.lc, v.data(), step, 1.0, b, e)
            Q._apply_bc(v, v.active)
            b, e = bounds(d)
            ops.axpby(t.lc, t.data(), d.lc, d.data(), -1.0 * step, 1.0, b, e)
            Q._apply_bc(d, d.active)
            rho_new = norm(l)
            if rho_new <= 0.0001 * rho0:
                return
            ratio = (rho_new * rho_new) / (rho * rho)
            b, e = bounds(s)
            ops.axpby(d.lc, d.data(), s.lc, s.data(), 1.0, ratio, b, e)
            Q._apply_bc(s, s.active)
            rho = rho_new
        raise AssertionError("coarse grid solver: iteration limit reached")

    g, v = fld("g", hi), fld("v", hi)
    b, e = bounds(g)
    ops.fill_expr(g.lc, g.data(), dom.geom(hi), ExprC.from_program(RHS_PROGRAM), b, e)
    Q._apply_bc(v, v.active)
    defect(hi)
    first = now = norm(hi)
    printed.append(first)
    n = 0
    while not (n >= 30 or now <= 1.0e-8 * first):
        n += 1
        cycle(hi)
        defect(hi)
        now = norm(hi)
        printed.append(now)
    return printed


def run_example(ops, lo, hi, **kw):
    with open(os.path.join(EX, "helmholtz3d_gs8.exa4")) as f:
        P = exa4.Exa4Program(f.read(), dict(dimensionality=3, minLevel=lo, maxLevel=hi), ops=ops, **kw)
    P.run()
    return P


def test_example_program_equals_the_hand_written_driver():
    """The interpreter (peephole: one mcgs_sweep per `color with`; and statement by statement) prints what the hand-written driver
    computes, bit for bit, and the cycle converges: the 27-point operator is exact on the harmonic polynomial."""
    want = gs8_driver(M.oracle_mc(), 1, 3)
    P = run_example(M.oracle_mc(), 1, 3, fuse_coarse_solver=False)
    assert P.fusions.get("mcgs_sweep", 0) > 0
    assert P.printed_values == want
    Q = run_example(M.oracle_mc(), 1, 3, fuse=False)
    assert Q.fusions.get("mcgs_sweep", 0) == 0 and Q.printed_values == want
    res = want[1:]
    assert want[0] > 100.0 and len(res) <= 10 and res[-1] <= 1e-8 * want[0] and all(b_ < 0.2 * a for a, b_ in zip([want[0]] + res, res))


# -- SolverFromL3(smoother="mcgs") ---------------------------------------------------------------------------------------------------
MCGS27 = dict(nd=3, min_level=1, max_level=3, smoother="mcgs", omega=0.9, stencil="helmholtz27", restrict_scale=1.0, tol=1e-8, cg_max=512, bc_fn=0,
              sol_fn=9, coef_fn=7, kappa=10.0, ksq=2.0, rhs_from_solution=True)


def loop_by_loop_solver(cfg, ops):
    """SolverFromL3 with the sweep written out: eight coloured loops, each after its `communicate`."""
    from exastencils_amd.solver import SolverFromL3

    class LoopByLoop(SolverFromL3):
        def Smoother(self, l, correction_from=None, zero_input=False):
            assert correction_from is None and not zero_input
            Sol, F, A = self.Solution[l], self.RHS[l], self.Laplace[l]
            b, e = self.bounds(Sol)
            for r2 in (0, 1):
                for r1 in (0, 1):
                    for r0 in (0, 1):
                        col = Colouring((((0,), 0, 2), ((1,), 0, 2), ((2,), 0, 2)), (r0, r1, r2))
                        self.communicate(Sol, Sol.active)
                        self.ops.stencil_op_coloured(S.SMOOTH, Sol.lc, Sol.data(), F.lc, F.data(), Sol.lc, Sol.data(), A, self._w(l), col, b, e)

    return LoopByLoop(cfg, ops)


def test_solver_with_the_multicolour_smoother():
    from exastencils_amd.solver import ConfigL3, SolverFromL3

    cfg = ConfigL3(frag_len=(2, 2, 2), **MCGS27)
    P = SolverFromL3(cfg, M.oracle_mc())
    P.setup()
    P.Solve()
    Q = loop_by_loop_solver(cfg, M.oracle_mc())
    Q.setup()
    Q.Solve()
    assert P.res_history == Q.res_history and P.err_history == Q.err_history
    assert 2 <= P.iterations <= 8 and P.err_history[-1] < 1e-8
    # it smooths better than damped Jacobi: fewer cycles to the same tolerance
    J = SolverFromL3(ConfigL3(frag_len=(2, 2, 2), **dict(MCGS27, smoother="jacobi", omega=0.8)), M.oracle_mc())
    J.setup()
    J.Solve()
    assert P.iterations < J.iterations
    # the one-pass options of the other smoothers are refused, not ignored
    for opt in (dict(temporal_blocking=True), dict(fused_rbgs=True), dict(fused_smooth_residual=True)):
        with pytest.raises(AssertionError, match="mcgs"):
            SolverFromL3(ConfigL3(frag_len=(2, 2, 2), **dict(MCGS27, **opt)), M.oracle_mc())
    with pytest.raises(ValueError):
        SolverFromL3(ConfigL3(**dict(MCGS27, smoother="sor")), M.oracle_mc())
