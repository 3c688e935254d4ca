"""Semilinear operators and FAS cycles without a GPU.  The numpy restatement of examg_nl_op / examg_nl_smooth (tests/nonlinear_ops.py)
runs the reference's Testing/NonLinear/FAS_2D_Basic.exa4 as it is and the two own example programs through the interpreter; a second,
straight-line numpy FAS that uses neither the interpreter nor a kernel layer prints the same lines, so the restatement is not its own
judge.  The interpreter issues one launch per operator loop, refuses by name what it does not build, keeps routing the optical-flow
coefficient stencils to the system kernels, replays the FAS cycle from a recording like any host-free function and gives the same
answer on two blocks over gloo.  The library refuses malformed calls before it launches anything (no GPU is needed to see that)."""
import ctypes as C
import os
import re
import socket

import numpy as np
import pytest

import nonlinear_cases as N
from nonlinear_ops import NL_ADD, NL_APPLY, NL_RESIDUAL, NonlinearOracleOps, check_program, eval_program
from test_exa4 import REF

from exastencils_amd import exa4, knowledge
from exastencils_amd.domain import RectDomain
from exastencils_amd.exa4_parser import Exa4Unsupported
from exastencils_amd.layout import FieldLayout

REFDIR = os.path.join(REF, "Testing", "NonLinear")


@pytest.fixture(scope="module")
def bratu2d():
    """(program, printed lines) of examples/exa4/bratu2d_fas.exa4 on the restatement, run once."""
    return N.run("bratu2d_fas.exa4", N.K_BRATU2D, NonlinearOracleOps())


# -- the programs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir(REFDIR), reason="reference checkout not present")
def test_reference_program_with_its_knowledge_file_reproduces_its_results_file():
    from oracle import mg

    k = knowledge.parse_file(os.path.join(REFDIR, "FAS_2D_Basic.knowledge"))
    k["testing_enabled"] = True
    with open(os.path.join(REFDIR, "FAS_2D_Basic.exa4")) as f:
        P = exa4.Exa4Program(f.read(), k, ops=NonlinearOracleOps())
    out = P.run()
    with open(os.path.join(N.GOLDEN, "NonLinear_FAS_2D_Basic.results")) as f:
        want = f.read()
    assert mg.compare_with_golden(out, want) == []      # Testing/run_test.py:12-42
    assert out == want.split()


@pytest.mark.skipif(not os.path.isdir(REFDIR), reason="reference checkout not present")
def test_fixture_is_the_reference_results_file():
    with open(os.path.join(REFDIR, "FAS_2D_Basic.results")) as f, open(os.path.join(N.GOLDEN, "NonLinear_FAS_2D_Basic.results")) as g:
        assert f.read() == g.read()


def test_bratu2d_prints_the_lines_of_the_results_file(bratu2d):
    P, out = bratu2d
    assert out == N.results_lines()
    g = N.own_golden("bratu2d_fas")
    assert out == g["lines"]
    for got, want in zip(P.printed_values, [float.fromhex(v) for v in g["values"]]):
        assert abs(got - want) <= 1e-10 * abs(want)


def test_bratu2d_operator_loops_are_one_launch_each(bratu2d):
    """Per cycle and level above the coarsest: 6 smoothing steps, one residual, one `+=`; 30 steps on the coarsest; one residual per
    norm.  Nothing of the linear stencil kernels runs."""
    calls = Recording()
    P, out = N.run("bratu2d_fas.exa4", dict(N.K_BRATU2D, maxLevel=3), calls)
    cycles = int(out[-1])
    names = calls.calls
    assert names.count("nl_smooth") == cycles * (6 * 3 + 30)
    assert names.count("nl_op") == cycles * (2 * 3) + cycles + 1
    assert "stencil_op" not in names and "sys_op" not in names


def test_bratu3d_prints_its_golden_and_is_second_order():
    """The manufactured solution is smooth: the maximum error at convergence falls by a factor of four per level, between 3 and 5 on
    three successive finest levels (measured on the restatement: 4.00 and 4.00)."""
    g = N.own_golden("bratu3d_rbgs_fas")
    errs = []
    for hi in (3, 4, 5):
        P, out = N.run("bratu3d_rbgs_fas.exa4", dict(N.K_BRATU3D, maxLevel=hi), NonlinearOracleOps())
        errs.append(P.printed_values[-1])
        assert P.printed_values[-2] < 1e-8 * P.printed_values[0]        # converged: the error is the discretisation's
    assert out == g["lines"]
    for got, want in zip(P.printed_values, [float.fromhex(v) for v in g["values"]]):
        assert abs(got - want) <= 1e-10 * abs(want)
    print("errors", errs)
    for coarse, fine in zip(errs, errs[1:]):
        assert 3.0 < coarse / fine < 5.0


def straight_line_fas():
    """-lap(u) + 10 u exp(u) = f on 1152^2 cells, levels 0 .. 7, FAS V(3,3) with the damped Newton-Jacobi smoother: plain numpy on whole
    arrays, written from the mathematics (full weighting, bilinear interpolation, interior points only).  The printed lines."""
    gam, w = 10.0, 0.8

    def nonlin(u, h):
        out = np.zeros_like(u)
        c = u[1:-1, 1:-1]
        out[1:-1, 1:-1] = (4.0 * c - u[1:-1, :-2] - u[1:-1, 2:] - u[:-2, 1:-1] - u[2:, 1:-1]) / (h * h) + gam * np.exp(c) * c
        return out

    def smooth(u, f, h, n):
        for _ in range(n):
            c = u[1:-1, 1:-1]
            new = u.copy()
            new[1:-1, 1:-1] = c + w * (f - nonlin(u, h))[1:-1, 1:-1] / (4.0 / (h * h) + gam * (1.0 + c) * np.exp(c))
            u = new
        return u

    def restrict(x):
        out = np.zeros(((x.shape[0] - 1) // 2 + 1,) * 2)
        out[1:-1, 1:-1] = (4.0 * x[2:-2:2, 2:-2:2] + 2.0 * (x[1:-3:2, 2:-2:2] + x[3:-1:2, 2:-2:2] + x[2:-2:2, 1:-3:2] + x[2:-2:2, 3:-1:2])
                           + x[1:-3:2, 1:-3:2] + x[1:-3:2, 3:-1:2] + x[3:-1:2, 1:-3:2] + x[3:-1:2, 3:-1:2]) / 16.0
        return out

    def prolong(x):
        out = np.zeros((2 * (x.shape[0] - 1) + 1,) * 2)
        out[::2, ::2] = x
        out[1::2, ::2] = 0.5 * (x[:-1, :] + x[1:, :])
        out[::2, 1::2] = 0.5 * (x[:, :-1] + x[:, 1:])
        out[1::2, 1::2] = 0.25 * (x[:-1, :-1] + x[1:, :-1] + x[:-1, 1:] + x[1:, 1:])
        return out

    def cycle(l, u, f):
        h = 1.0 / (9 * 2 ** l)
        if l == 0:
            return smooth(u, f, h, 30)
        u = smooth(u, f, h, 3)
        r = np.zeros_like(u)
        r[1:-1, 1:-1] = (f - nonlin(u, h))[1:-1, 1:-1]
        v = restrict(u)
        fc = restrict(r) + nonlin(v, 2.0 * h)
        uc = cycle(l - 1, v.copy(), fc)
        e = prolong(uc - v)
        u[1:-1, 1:-1] += e[1:-1, 1:-1]
        return smooth(u, f, h, 3)

    n = 9 * 2 ** 7
    h = 1.0 / n
    y, x = np.meshgrid(np.arange(n + 1) * h, np.arange(n + 1) * h, indexing="ij")
    sol = (x ** 2 - x ** 3) * np.sin(3.0 * np.pi * y)
    f = ((9.0 * np.pi ** 2 + gam * np.exp(sol)) * (x ** 2 - x ** 3) + 6.0 * x - 2.0) * np.sin(3.0 * np.pi * y)
    u = np.zeros_like(f)

    def resnorm():
        return float(np.sqrt(np.sum((f - nonlin(u, h))[1:-1, 1:-1] ** 2)))

    res0 = res = resnorm()
    lines = ["%.4g" % res0]
    it = 0
    while not (res < 1.0e-5 * res0 or it >= 100):
        it += 1
        u = cycle(7, u, f)
        res = resnorm()
        lines.append("%.4g" % float(np.max(np.abs(u - sol)[1:-1, 1:-1])))
    return lines + ["%d" % it]


def test_a_straight_line_numpy_fas_prints_the_same_lines():
    assert straight_line_fas() == N.results_lines()


# -- the restatement on its own -----------------------------------------------------------------------------------------------------------
def test_restatement_smoother_is_a_newton_step_for_its_point():
    """With w = 1 and a stencil of the centre entry alone the smoother is Newton's method for a u + gamma u exp(u) = f at every point:
    five steps from 0 solve it to 1e-14 relative (quadratic convergence), and nl_op's residual of the result says so."""
    from exastencils_amd.field import Stencil

    orc = NonlinearOracleOps()
    l = FieldLayout.node(2, (6, 5), 1)
    L = l.c_struct()
    st = Stencil([(0, 0, 0)], [3.0])
    c = [("const", 2.0), ("u", None), ("exp", None), ("*", None)]
    d = [("const", 2.0), ("const", 1.0), ("u", None), ("+", None), ("*", None), ("u", None), ("exp", None), ("*", None)]
    u, un, f, r = (orc.new_array(l.size) for _ in range(4))
    f.copy_(orc.from_host(np.random.default_rng(5).uniform(0.5, 4.0, l.size)))
    b, e = [1, 1, 0], [6, 5, 1]
    for _ in range(5):
        orc.nl_smooth(L, u, L, un, L, f, st, c, d, 1.0, -1, b, e)
        u, un = un, u
    orc.nl_op(NL_RESIDUAL, L, u, L, u, L, f, L, r, st, c, b, e)
    assert float(np.abs(r.numpy()).max()) <= 1e-14 * 4.0 * 10
    assert float(np.abs(u.numpy()).max()) > 0.1


def test_restatement_modes_agree_and_write_the_box_only():
    orc = NonlinearOracleOps()
    shape, b, e = N.geometry(3, (7, 5, 3), (1, 1, 1))
    lu, lq, lf, ld = N.layouts(3, shape)
    st = N.stencil(7, "middle")
    u, q, f, d = N.arrays(orc, (lu, lq, lf, ld), 11)
    keep = d.numpy().copy()
    C_ = [x.c_struct() for x in (lu, lq, lf, ld)]
    orc.nl_op(NL_APPLY, C_[0], u, C_[1], q, None, None, C_[3], d, st, N.EXACT_C, b, e)
    n = d.numpy().copy()
    import stencil_cases as S

    inside = S.box_mask(ld, b, e)
    assert np.array_equal(n[~inside], keep[~inside]) and not np.array_equal(n[inside], keep[inside])
    orc.nl_op(NL_ADD, C_[0], u, C_[1], q, None, None, C_[3], d, st, N.EXACT_C, b, e)
    assert np.array_equal(d.numpy()[inside], (n + n)[inside])
    orc.nl_op(NL_RESIDUAL, C_[0], u, C_[1], q, C_[2], f, C_[3], d, st, N.EXACT_C, b, e)
    fi = S.box_mask(lf, b, e)
    assert np.array_equal(d.numpy()[inside], f.numpy()[fi] - n[inside])


def test_program_rules_of_the_restatement():
    check_program(N.deep_program(8))
    check_program(N.long_program(31))
    for bad, text in ((N.deep_program(9), "deeper"), (N.long_program(33), "33 instructions"), ([("x", None)], "'x'"), ([("u", None), ("+", None)], "underflows"),
                      ([("u", None), ("u", None)], "exactly one")):
        with pytest.raises(ValueError, match=text):
            check_program(bad)
    v = np.array([0.5, 1.25])
    assert np.array_equal(eval_program(N.LIBM_D, v), (N.GAMMA * (1.0 + v)) * np.exp(v))


# -- the library's refusals: decided on the host before anything is launched -----------------------------------------------------------------
def _abi():
    import __graft_entry__ as ge

    ge.build_examg()
    from exastencils_amd import lib

    return lib, C.CDLL(lib.LIB_PATH)


def test_library_declares_the_semilinear_entry_points():
    lib, L = _abi()
    for name in ("examg_nl_op", "examg_nl_smooth"):
        assert name in lib.SYMBOLS and hasattr(L, name)
    assert C.sizeof(lib.NlExprC) == 392 and lib.NlExprC.c.offset == 136
    assert lib.NL_OPS["u"] == 22 and "x" not in lib.NL_OPS and (lib.NL_APPLY, lib.NL_RESIDUAL, lib.NL_ADD) == (0, 1, 2)


def _nl_call(lib, st=None, mutate=None, c=None, d=None, lu=None, lq=None, ld=None, lf=None, colour=None, same=False, begin=(1, 1, 0), end=(1, 4, 1), mode=1):
    """examg_nl_op (colour None) or examg_nl_smooth with made-up non-null pointers and an EMPTY box: the library checks stencil,
    layouts, programs and aliasing before it looks at the box, so every case is refused, and a call that were accepted would return
    0 without a launch (tests/test_blas_exact.py does the same).  The refusals that need a box -- it leaves an allocation -- are in
    tests/test_gpu_nonlinear.py, on real allocations.  Returns the error text."""
    from exastencils_amd.lib import NlExprC, ivec

    Lh = lib.load()
    base = FieldLayout.node(2, (6, 5), 1)
    lu, lq, ld, lf = [(x or base).c_struct() for x in (lu, lq, ld, lf)]
    st = st or N.stencil(5, "first")
    sc = st.c_struct(lambda t: t)
    if mutate is not None:
        mutate(sc)
    cc = c if c is not None else NlExprC.from_program(N.EXACT_C)
    dd = d if d is not None else NlExprC.from_program(N.EXACT_D)
    pu, pq, pf, pd = 0x1000, 0x2000, 0x3000, 0x4000
    if colour is None:
        rc = Lh.examg_nl_op(mode, C.byref(lu), pu, C.byref(lq), pq, C.byref(lf), pf, C.byref(ld), pu if same else pd, C.byref(sc), C.byref(cc),
                            ivec(begin), ivec(end), None)
    else:
        rc = Lh.examg_nl_smooth(C.byref(lu), pu, C.byref(ld), pu if same else pd, C.byref(lf), pf, C.byref(sc), C.byref(cc), C.byref(dd), 0.8, colour,
                                ivec(begin), ivec(end), None)
    assert rc != 0, "the call was not refused"
    return Lh.examg_last_error().decode()


def _raw_program(ops, consts=None):
    from exastencils_amd.lib import NlExprC

    e = NlExprC()
    e.n = len(ops)
    for i, o in enumerate(ops):
        e.op[i] = o
    return e


def test_library_refuses_before_launching():
    from exastencils_amd.field import Stencil

    lib, _ = _abi()
    base = FieldLayout.node(2, (6, 5), 1)
    cell = FieldLayout.cell(2, (6, 5), 1)
    sf = Stencil([(0, 0, 0), (1, 0, 0)], [], 0x5000, base, 0, 0)
    nine = N.stencil(9, "first")
    for colour in (None, -1):
        assert "stencil field" in _nl_call(lib, st=sf, colour=colour)
        def off_centre(sc):         # the entry `diag` names is not (0, 0, 0)
            sc.off[sc.diag][1] = 1

        assert "no centre entry" in _nl_call(lib, mutate=off_centre, colour=colour)
        assert "colour-split" in _nl_call(lib, lu=base.split_x(), colour=colour)
        assert "colour-split" in _nl_call(lib, ld=base.split_x(), colour=colour)
        assert "cell layout" in _nl_call(lib, lu=cell, colour=colour)
        assert "cell layout" in _nl_call(lib, lf=cell, colour=colour)
        assert "reads the node position" in _nl_call(lib, c=_raw_program([1]), colour=colour)
        assert "unknown opcode" in _nl_call(lib, c=_raw_program([23]), colour=colour)
        assert "underflows" in _nl_call(lib, c=_raw_program([22, 4]), colour=colour)
        assert "exactly one value" in _nl_call(lib, c=_raw_program([22, 22]), colour=colour)
        assert "deeper than 8" in _nl_call(lib, c=_raw_program([22] * 9 + [4] * 8), colour=colour)
        assert "is empty" in _nl_call(lib, c=_raw_program([]), colour=colour)
        long = _raw_program([22])
        long.n = 33
        assert "33 instructions" in _nl_call(lib, c=long, colour=colour)
    assert "reads the node position" in _nl_call(lib, d=_raw_program([2]), colour=-1)
    assert "out of place" in _nl_call(lib, colour=-1, same=True)
    assert "in place" in _nl_call(lib, colour=0, same=False)
    assert "does not decouple" in _nl_call(lib, st=nine, colour=1, same=True)
    assert "the layout of u_out is not that of u_in" in _nl_call(lib, colour=1, same=True, ld=FieldLayout.node(2, (6, 5), 2))
    assert "colour must be" in _nl_call(lib, colour=2, same=True)
    assert "dst is u" in _nl_call(lib, same=True)
    assert "bad mode" in _nl_call(lib, mode=3)
    # an empty box is a no-op that returns 0, and the existing expression entry points keep refusing EXAMG_OP_U
    from exastencils_amd.lib import ExprC, NlExprC, ivec

    Lh = lib.load()
    l = base.c_struct()
    sc = N.stencil(5, "first").c_struct(lambda t: t)
    assert Lh.examg_nl_op(0, C.byref(l), 0x1000, C.byref(l), 0x1000, None, None, C.byref(l), 0x2000, C.byref(sc), C.byref(NlExprC.from_program(N.EXACT_C)),
                          ivec((1, 1, 0)), ivec((1, 4, 1)), None) == 0
    e = ExprC()
    e.n, e.op[0] = 1, 22
    from exastencils_amd.lib import GeomC

    assert Lh.examg_fill_expr(C.byref(l), 0x1000, C.byref(GeomC()), C.byref(e), ivec((1, 1, 0)), ivec((2, 2, 1)), None) != 0
    assert b"unknown opcode" in Lh.examg_last_error()


# -- the interpreter: recognition, routing, refusals ------------------------------------------------------------------------------------------
class Recording(NonlinearOracleOps):
    """Records the name of every kernel-layer call."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def __getattribute__(self, name):
        a = object.__getattribute__(self, name)
        if callable(a) and not name.startswith("_") and name not in ("new_array", "new_scalar", "ptr", "to_host", "from_host", "scalar_value", "synchronize"):
            calls = object.__getattribute__(self, "calls")

            def rec(*args, **kw):
                calls.append(name)
                return a(*args, **kw)

            return rec
        return a


def test_optical_flow_coefficient_stencils_still_route_to_the_system_kernels():
    ops = Recording()
    P = exa4.Exa4Program(N.text("optflow2d.exa4"), dict(dimensionality=2, minLevel=2, maxLevel=4), ops=ops)
    P.run()
    assert "sys_op" in ops.calls and "sys_relax" in ops.calls and ops.calls.count("pointwise_mul") == 5
    assert "nl_op" not in ops.calls and "nl_smooth" not in ops.calls
    assert P._coef_field("Cuu") is not None and P._coef_expr("Cuu") is None


def test_coefficient_expression_reads_its_own_field_not_the_operand():
    """`G@coarser * v@coarser` reads u inside the stencil and multiplies v: q and u are different arrays in the `+=` loop."""
    seen = []

    class Spy(NonlinearOracleOps):
        def nl_op(self, mode, lu, u, lq, q, *a):
            seen.append((mode, u.data_ptr() == q.data_ptr()))
            return super().nl_op(mode, lu, u, lq, q, *a)

    N.run("bratu2d_fas.exa4", dict(N.K_BRATU2D, maxLevel=2), Spy())
    assert (NL_ADD, False) in seen and (NL_RESIDUAL, True) in seen and all(same for mode, same in seen if mode != NL_ADD)


def _edit(text, *pairs):
    for old, new in pairs:
        assert text.count(old) >= 1, old
        text = text.replace(old, new, 1)
    return text


G2 = "gamma * exp ( u<active> )"
SM2 = "( 1.0 + u<active> ) * exp ( u<active> ) ) )"
RES2 = "r = f - ( A * u<active> + G * u<active> )"
FIVE = ("Layout Five< ColumnVector<Real, 5>, Node >@all {\n  ghostLayers = [0, 0]\n  duplicateLayers = [1, 1]\n}\nField five< global, Five, None >@all\n"
        "StencilField AF< five => A >@all\n")
CELL = ("Layout Cells< Real, Cell >@all {\n  ghostLayers = [1, 1] with communication\n  duplicateLayers = [0, 0]\n}\n"
        "Field cu< global, Cells, Neumann >@all\nField cf< global, Cells, None >@all\nField cr< global, Cells, None >@all\n"
        "Stencil GC@all {\n  [0, 0] => gamma * exp ( cu )\n}\n")

REFUSALS = [
    ("two fields", 2, lambda t: _edit(t, (G2, G2 + " * v")), "stencil G: a coefficient expression over 2 fields"),
    ("offset access", 2, lambda t: _edit(t, (G2, "gamma * exp ( u<active>@[1, 0] )")), "offset access"),
    ("beside other entries", 2, lambda t: _edit(t, ("  [0, 0] => " + G2, "  [0, 0] => " + G2 + "\n  [1, 0] => 1.0")), "stencil G: a coefficient expression beside other entries"),
    ("off the centre", 2, lambda t: _edit(t, ("  [0, 0] => " + G2, "  [1, 0] => " + G2)), "stencil G: a coefficient expression off the centre"),
    ("stencil field as A", 2, lambda t: _edit(t, ("Stencil R from", FIVE + "Stencil R from"), (RES2, "r = f - ( AF * u<active> + G * u<active> )")),
     "a stencil field (AF) as the constant stencil of a semilinear operator"),
    ("cell fields", 2, lambda t: _edit(t, ("Stencil R from", CELL + "Stencil R from"), ("Function Application {\n", "Function Application {\n  loop over cr@finest {\n    cr@finest = cf@finest - ( A@finest * cu@finest + GC@finest * cu@finest )\n  }\n")),
     "semilinear operator on cell field"),
    ("multi-colouring", 3, lambda t: _edit(t, ("( i0 + i1 + i2 ) % 2,", "i0 % 2, i1 % 2, i2 % 2,")), "semilinear operator (coefficient-expression stencil) under a multi-colouring"),
    ("only region", 2, lambda t: _edit(t, ("  loop over r {\n    r = f - (", "  loop over r only dup [0, 0] {\n    r = f - (")), "semilinear operator in a loop with an `only` region or under contraction"),
    ("contraction", 2, lambda t: _edit(t, ("  loop over r {\n    r = f - ( A * u<active> + G * u<active> )\n  }", "  repeat 1 times with contraction [1, 1] {\n    loop over r {\n      r = f - ( A * u<active> + G * u<active> )\n    }\n  }")),
     "semilinear operator in a loop with an `only` region or under contraction"),
    ("denominator of another field", 2, lambda t: _edit(t, (SM2, "( 1.0 + v ) * exp ( v ) ) )")), "nonlinear smoother: a denominator whose field is not u"),
    ("diag of another stencil", 2, lambda t: _edit(t, ("Stencil R from", "Stencil B@all {\n  [0, 0] => 1.0\n}\nStencil R from"), ("diag ( A )", "diag ( B )")), "diag of another stencil than A"),
    ("program longer than the bound", 2, lambda t: _edit(t, (G2, G2 + " + 1.0" * 15)), "is longer than the bound (32)"),
    ("stack deeper than the bound", 2, lambda t: _edit(t, (G2, "u<active> + ( " * 8 + "u<active>" + " )" * 8)), "is longer than the bound (8)"),
    ("position in the expression", 2, lambda t: _edit(t, (G2, G2 + " * vf_nodePosition_x")), "a coefficient expression over the node position"),
    ("outside the forms", 2, lambda t: _edit(t, (RES2, "r = G * u<active>")), "coefficient-expression stencil G outside the forms"),
    ("scaled operator", 2, lambda t: _edit(t, (RES2, "r = f - 2.0 * ( A * u<active> + G * u<active> )")), "coefficient-expression stencil G outside the forms"),
    ("operator in a coloured loop", 3, lambda t: _edit(t, ("      u += 1.0 * ( ( f - ( A * u + G * u ) ) / ( diag ( A ) + gamma * ( 1.0 + u ) * exp ( u ) ) )", "      r = f - ( A * u + G * u )")),
     "semilinear operator in a coloured loop outside the smoother"),
    ("in place without colouring", 2, lambda t: _edit(t, ("u<next> = u<active> + omega", "u<active> = u<active> + omega")), "in-place nonlinear smoother without colouring"),
]


@pytest.mark.parametrize("name,nd,edit,text", REFUSALS, ids=[r[0].replace(" ", "-") for r in REFUSALS])
def test_refusals_by_name(name, nd, edit, text):
    src = N.text("bratu2d_fas.exa4" if nd == 2 else "bratu3d_rbgs_fas.exa4")
    bad = edit(src)
    assert bad != src
    with pytest.raises(Exa4Unsupported, match=re.escape(text)):
        exa4.Exa4Program(bad, dict(dimensionality=nd, minLevel=1, maxLevel=3), ops=NonlinearOracleOps()).run()


def test_a_global_assigned_between_two_launches_reaches_the_kernel():
    """Globals are folded into the constants of a point program: a `Var` that the program assigns between two loops must give another
    program (parameter continuation in gamma is what a Bratu solver is used for).  With u = 0.5 and f = 0 on a 3 x 3 grid of inner
    points the residual is -(A u + gamma exp(u) u); its change between gamma = 10 and gamma = 1000 is 990 exp(0.5) 0.5 per point,
    both for the operator and -- through d -- for the smoother."""
    src = _edit(N.text("bratu2d_fas.exa4"), ("  Val gamma : Real = 10.0", "  Var gamma : Real = 10.0"))
    src = src[:src.index("Function Application {")] + """Function Application {
  loop over u@finest {
    u<active>@finest = 0.5
  }
  loop over f@finest {
    f@finest = 0.0
  }
  Defect@finest ( )
  print ( DefectNorm@finest ( ) )
  Relax@finest ( )
  print ( ErrorNorm@finest ( ) )
  gamma = 1000.0
  Defect@finest ( )
  print ( DefectNorm@finest ( ) )
  Relax@finest ( )
  print ( ErrorNorm@finest ( ) )
}
"""
    outs = {}
    for auto_graph in (False, True):
        P = exa4.Exa4Program(src, dict(dimensionality=2, minLevel=1, maxLevel=2), ops=NonlinearOracleOps(), auto_graph=auto_graph)
        P.run()
        outs[auto_graph] = list(P.printed_values)
    r10, e10, r1000, e1000 = outs[False]
    assert outs[True] == outs[False]
    assert r1000 > 20.0 * r10 and e1000 != e10
    # the first state from a program that never changes gamma
    fixed = _edit(src, ("  gamma = 1000.0\n", ""))
    P = exa4.Exa4Program(fixed, dict(dimensionality=2, minLevel=1, maxLevel=2), ops=NonlinearOracleOps())
    P.run()
    assert P.printed_values[:2] == [r10, e10] and P.printed_values[2] != r1000


# -- graph replay ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("bratu2d_fas.exa4", dict(N.K_BRATU2D, maxLevel=3)), ("bratu3d_rbgs_fas.exa4", dict(N.K_BRATU3D, maxLevel=3))],
                         ids=["bratu2d", "bratu3d"])
def test_fas_cycle_replayed_from_a_recording_equals_its_interpretation(name, k):
    """`auto_graph` records Cycle@finest at its second call and replays it afterwards, like any host-free leveled function: printed
    values, lines and every array of every field bit for bit (tests/graph_cases.py on the recording stand-in of tests/graph_ops.py)."""
    import graph_cases as gc
    from graph_ops import DeferringOps

    ops = DeferringOps(NonlinearOracleOps())
    G = exa4.Exa4Program(N.text(name), dict(k), ops=ops, auto_graph=True)
    P = exa4.Exa4Program(N.text(name), dict(k), ops=ops, auto_graph=False)
    G.run()
    P.run()
    gc.assert_same_run(G, P)
    rec = gc.recorded(G)
    cycles = int(P.out[-1].split()[-1])
    assert rec[("Cycle", 3)] == cycles - 1 and G.graph_replays >= cycles - 1
    assert "gamma" in G._graph_deps("Cycle", 3)


# -- two blocks over gloo ---------------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, out_dir):
    import json

    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from exastencils_amd.comm import Communicator

    ops = NonlinearOracleOps()
    dom = RectDomain(2, (2, 1, 1), rank, (1, 1, 1))
    P = exa4.Exa4Program(N.text("bratu2d_fas.exa4"), dict(N.K_BRATU2D_TWO), ops=ops, domain=dom, comm=Communicator(dom, ops))
    out = P.run()
    lay = P.fields[("u", 4)].layout
    u = ops.to_host(P.fields[("u", 4)].data()).reshape(lay.tot(1), lay.tot(0))
    np.save(os.path.join(out_dir, "u%d.npy" % rank), u[lay.ref(1):lay.ref(1) + 17, lay.ref(0):lay.ref(0) + 17])
    json.dump({"lines": out, "values": [float(v).hex() for v in P.printed_values], "messages": P.comm.stats["messages"]},
              open(os.path.join(out_dir, "r%d.json" % rank), "w"))
    dist.barrier()
    dist.destroy_process_group()


def test_bratu2d_on_two_blocks_in_x_equals_the_single_block(tmp_path):
    """The kernels are point-wise and the communication is the existing one: the solution of the two-block run is that of the single
    block bit for bit (so is the maximum error, a reduction whose order does not matter); the residual norms are sums over blocks and
    agree to rounding (1e-13 relative: some 250 points per block, each partial sum within 2^-53 times its length of the exact one)."""
    import json

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    single, lines = N.run("bratu2d_fas.exa4", N.K_BRATU2D_TWO, NonlinearOracleOps())
    lay = single.fields[("u", 4)].layout
    u = single.ops.to_host(single.fields[("u", 4)].data()).reshape(lay.tot(1), lay.tot(0))
    u = u[lay.ref(1):lay.ref(1) + 17, lay.ref(0):lay.ref(0) + 33]
    for r in range(2):
        meta = json.load(open(tmp_path / ("r%d.json" % r)))
        assert meta["messages"] > 0
        assert meta["lines"] == lines
        vals = [float.fromhex(v) for v in meta["values"]]
        assert len(vals) > 3 and vals[1:] == single.printed_values[1:]
        assert abs(vals[0] - single.printed_values[0]) <= 1e-13 * single.printed_values[0]
        part = np.load(tmp_path / ("u%d.npy" % r))
        assert np.array_equal(part.view(np.uint64), u[:, 16 * r:16 * r + 17].view(np.uint64))
