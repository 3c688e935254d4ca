"""Lexicographic Gauss-Seidel without a GPU: the hyperplane helper of tests/gs_cases.py against the literal loop nest, the two host
drivers (SolverFromL3 with smoother="gs", the ExaSlang-4 interpreter on examples/exa4/poisson3d_gs.exa4) on the helper layer, and
every refusal by name.  The GPU tests (tests/test_gpu_gs.py) compare the kernels with the same helper."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import gs_cases as G  # noqa: E402
import stencil_cases as S  # noqa: E402
from oracle_ops import OracleOps  # noqa: E402

from exastencils_amd import exa4  # noqa: E402
from exastencils_amd.layout import FieldLayout  # noqa: E402
from exastencils_amd.solver import ConfigL3, SolverFromL3  # noqa: E402

EX = os.path.join(ROOT, "examples", "exa4")
FOLD = G.FoldGS()


# -- the helper is the loop nest -----------------------------------------------------------------------------------------------------------
def test_skews_of_the_case_stencils():
    assert G.skew(G.seven_point().offsets) == (1, 1) and G.skew(G.five_point(True).offsets) == (1, 1)
    assert G.skew(G.twentyseven_point().offsets) == (2, 4) and G.skew(G.nine_point().offsets) == (2, 4)
    assert G.skew(G.upwind(2).offsets) == (2, 4) and G.skew(G.upwind(3).offsets) == (2, 4)
    assert G.skew([(0, 0, 0), (1, 0, 0), (0, -1, 0)]) == (1, 1)
    with pytest.raises(AssertionError):
        G.skew([(0, 0, 0), (-2, 1, 0)])


def _nest_case(nd, inner, st_of, begin=None, end=None):
    cells = tuple(inner[d] + 1 if d < nd else 0 for d in range(3))
    lu, lf = FieldLayout.node(nd, cells, 1, align=4), FieldLayout.node(nd, cells, 0, True, False)
    st = st_of(FOLD, lf) if callable(st_of) else st_of
    rng = np.random.default_rng(77)
    u0, f = rng.uniform(-1.0, 1.0, lu.size), rng.uniform(-1.0, 1.0, lf.size)
    b = begin or [1, 1, 1 if nd == 3 else 0]
    e = end or [inner[d] + 1 if d < nd else 1 for d in range(3)]
    w = 0.713 if st.cfield is not None else S.free_weight(st)
    want = u0.copy()
    G.gs_nest(lu, want, lf, f, st, w, b, e)
    got = u0.copy()
    fcopy = f.copy()
    FOLD.gs_sweep(lu, got, lf, f, st, w, b, e)
    assert np.array_equal(f, fcopy)
    assert np.array_equal(got, want), "%d values differ" % int((got != want).sum())
    changed = got != u0
    assert changed.sum() == np.prod([e[d] - b[d] for d in range(3)])      # every point of the box moved, nothing else
    return got


@pytest.mark.parametrize("name", ["twentyseven", "twentyseven_centre_last", "seven", "seven_centre_last", "upwind3", "field_inv_times", "field_divide"])
def test_helper_is_the_loop_nest_3d(name):
    """6 x 5 x 4 points: the hyperplane helper equals the literal triple loop over Python floats, bit for bit."""
    st = {"twentyseven": G.twentyseven_point(), "twentyseven_centre_last": G.twentyseven_point(True), "seven": G.seven_point(),
          "seven_centre_last": G.seven_point(True), "upwind3": G.upwind(3),
          "field_inv_times": lambda ops, lc: G.coefficient_field(ops, lc, 0), "field_divide": lambda ops, lc: G.coefficient_field(ops, lc, 1)}[name]
    _nest_case(3, (6, 5, 4), st)
    _nest_case(3, (6, 5, 4), st, [2, 1, 2], [6, 5, 4])


@pytest.mark.parametrize("name", ["nine", "nine_centre_last", "five", "upwind2"])
def test_helper_is_the_loop_nest_2d(name):
    st = {"nine": G.nine_point(), "nine_centre_last": G.nine_point(True), "five": G.five_point(), "upwind2": G.upwind(2)}[name]
    _nest_case(2, (7, 5, 1), st)


def test_sweep_differs_from_jacobi_and_from_red_black():
    """The cases can tell the orders apart: the nest's result is neither the out-of-place loop's nor the two colour loops'."""
    lu, lf = FieldLayout.node(3, (7, 6, 5), 1), FieldLayout.node(3, (7, 6, 5), 0, True, False)
    st = G.seven_point()
    rng = np.random.default_rng(3)
    u0, f = rng.uniform(-1.0, 1.0, lu.size), rng.uniform(-1.0, 1.0, lf.size)
    b, e, w = [1, 1, 1], [7, 6, 5], S.free_weight(st)
    gs, jac, rb = u0.copy(), u0.copy(), u0.copy()
    FOLD.gs_sweep(lu, gs, lf, f, st, w, b, e)
    FOLD.stencil_op(S.SMOOTH, lu, u0, lf, f, lu, jac, st, w, -1, b, e)
    for c in (0, 1):
        FOLD.stencil_op(S.SMOOTH, lu, rb, lf, f, lu, rb, st, w, c, b, e)
    assert not np.array_equal(gs, jac) and not np.array_equal(gs, rb)


# -- SolverFromL3(smoother="gs") against a hand-written driver ---------------------------------------------------------------------------
def gs_driver(ops, nd, lo, hi, cycles=None):
    """ConfigL3(smoother="gs") written out as kernel-layer calls: fields, layouts and stencils come from a solver instance whose
    cycle never runs; every statement of Solve / VCycle / VCycle_0 is issued here by hand, the smoother as `communicate Solution`
    (empty on one block) and one gs_sweep on the loop bounds.  Returns (residual history, Solution@finest)."""
    cfg = ConfigL3(nd=nd, min_level=lo, max_level=hi, smoother="gs")
    Q = SolverFromL3(cfg, ops)
    Q.setup()
    dom = Q.domain

    def bounds(f, reduction=False):
        return dom.loop_bounds(f.layout, reduction)

    def dot(x, y, over):
        b, e = bounds(over, True)
        return Q.comm.reduce_value(ops.dot(x.lc, x.data(), y.lc, y.data(), b, e), "sum")

    def residual(l):
        s, r, f = Q.Solution[l], Q.Residual[l], Q.RHS[l]
        b, e = bounds(r)
        ops.stencil_op(S.RESIDUAL, s.lc, s.data(), f.lc, f.data(), r.lc, r.data(), Q.Laplace[l], 0.0, -1, b, e)

    def norm(l):
        r = Q.Residual[l]
        return math.sqrt(dot(r, r, r))

    def smooth(l):
        s, f, A = Q.Solution[l], Q.RHS[l], Q.Laplace[l]
        b, e = bounds(s)
        for _ in range(3):
            ops.gs_sweep(s.lc, s.data(), f.lc, f.data(), A, (1.0 / A.diag) * 0.8, b, e)

    def coarse(l):
        s, r, p, q, A = Q.Solution[l], Q.Residual[l], Q.VecP, Q.VecGradP, Q.Laplace[l]
        residual(l)
        res = first = norm(l)
        b, e = bounds(p)
        ops.axpby(r.lc, r.data(), p.lc, p.data(), 1.0, 0.0, b, e)
        for _ in range(512):
            b, e = bounds(p)
            ops.stencil_op(S.APPLY, p.lc, p.data(), None, None, q.lc, q.data(), A, 0.0, -1, b, e)
            den = dot(p, q, p)
            alpha = (res * res) / den if den != 0.0 else float("nan")
            b, e = bounds(s)
            ops.axpby(p.lc, p.data(), s.lc, s.data(), alpha, 1.0, b, e)
            ops.axpby(q.lc, q.data(), r.lc, r.data(), -alpha, 1.0, b, e)
            nxt = norm(l)
            if nxt <= 0.001 * first:
                return
            beta = (nxt * nxt) / (res * res)
            b, e = bounds(p)
            ops.axpby(r.lc, r.data(), p.lc, p.data(), 1.0, beta, b, e)
            res = nxt
        raise AssertionError("coarse grid solver: iteration limit reached")

    def cycle(l):
        if l == lo:
            return coarse(l)
        smooth(l)
        residual(l)
        r, fc, sc, s = Q.Residual[l], Q.RHS[l - 1], Q.Solution[l - 1], Q.Solution[l]
        b, e = bounds(fc)
        ops.restrict(r.lc, r.data(), fc.lc, fc.data(), 4.0, b, e)
        b, e = bounds(sc)
        ops.set(sc.lc, sc.data(), 0.0, b, e)
        cycle(l - 1)
        b, e = bounds(s)
        ops.prolong_add(sc.lc, sc.data(), s.lc, s.data(), b, e)
        smooth(l)

    residual(hi)
    first = now = norm(hi)
    hist = [first]
    n = 0
    while not (now < 1.0e-5 * first or n >= (100 if cycles is None else cycles)):
        n += 1
        cycle(hi)
        residual(hi)
        now = norm(hi)
        hist.append(now)
    return hist, np.array(ops.to_host(Q.Solution[hi].data()), copy=True)


def solver_run(ops, nd, lo, hi, cycles=None, **kw):
    P = SolverFromL3(ConfigL3(nd=nd, min_level=lo, max_level=hi, smoother="gs", **({} if cycles is None else dict(max_it=cycles, tol=0.0)), **kw), ops)
    P.setup()
    P.Solve()
    return P


@pytest.mark.parametrize("nd", [2, 3])
def test_solver_equals_the_hand_written_driver(nd):
    ops = G.oracle_gs()
    P = solver_run(ops, nd, 1, 3)
    hist, sol = gs_driver(G.oracle_gs(), nd, 1, 3)
    assert P.res_history == hist
    assert np.array_equal(ops.to_host(P.Solution[3].data()), sol)
    assert P.Solution[3].num_slots == 1
    assert ops.gs_calls == 6 * 2 * P.iterations       # V(3,3) on levels 2 and 3
    assert len(hist) > 2 and hist[-1] < 1e-5 * hist[0] and all(y < 0.5 * x for x, y in zip(hist, hist[1:]))


def test_solver_refusals():
    from exastencils_amd.domain import RectDomain

    with pytest.raises(AssertionError, match="smoother='gs'.*fused_rbgs"):
        SolverFromL3(ConfigL3(nd=3, min_level=1, max_level=2, smoother="gs", fused_rbgs=True), G.oracle_gs())
    with pytest.raises(AssertionError, match="temporal_blocking"):
        SolverFromL3(ConfigL3(nd=3, min_level=1, max_level=2, smoother="gs", temporal_blocking=True), G.oracle_gs())
    with pytest.raises(ValueError, match="world_size must be 1"):
        SolverFromL3(ConfigL3(nd=3, min_level=1, max_level=2, smoother="gs"), G.oracle_gs(), RectDomain(3, (1, 1, 2), 0, (1, 1, 1)), comm=object())
    with pytest.raises(ValueError, match="periodic"):
        SolverFromL3(ConfigL3(nd=3, min_level=1, max_level=2, smoother="gs"), G.oracle_gs(),
                     RectDomain(3, (1, 1, 1), 0, (1, 1, 1), (0.0,) * 3, (1.0,) * 3, (True, False, False)))
    with pytest.raises(ValueError, match="smoother"):
        SolverFromL3(ConfigL3(nd=3, min_level=1, max_level=2, smoother="sgs"), G.oracle_gs())


# -- the interpreter ------------------------------------------------------------------------------------------------------------------------
class Tracing:
    """Records the names of the kernel-layer calls of the wrapped layer, in order."""

    def __init__(self, ops):
        self._ops, self.calls = ops, []

    def __getattr__(self, name):
        v = getattr(self._ops, name)          # AttributeError for what the layer does not have: hasattr() sees the wrapped layer
        if not callable(v) or name in ("ptr", "to_host", "from_host", "new_array", "new_scalar", "scalar_value", "synchronize", "clone"):
            return v

        def call(*a, **k):
            self.calls.append(name)
            return v(*a, **k)

        return call


def run_example(ops, lo, hi, **kw):
    with open(os.path.join(EX, "poisson3d_gs.exa4")) as f:
        P = exa4.Exa4Program(f.read(), dict(dimensionality=3, minLevel=lo, maxLevel=hi), ops=ops, **kw)
    P.run()
    return P


def test_example_program_prints_what_the_solver_computes():
    want = solver_run(G.oracle_gs(), 3, 1, 3)
    ops = Tracing(G.oracle_gs())
    P = run_example(ops, 1, 3, fuse_coarse_solver=False)
    assert P.printed_values == want.res_history
    assert P.out[-1] == str(want.iterations)
    # one gs_sweep per loop: V(3,3) on two levels, and no other smoother call in the trace
    assert ops.calls.count("gs_sweep") == 12 * want.iterations
    assert not any(c in ops.calls for c in ("mcgs_sweep", "stencil_op_coloured", "rbgs_sweep_fused", "jacobi2"))
    smooths = [i for i, c in enumerate(ops.calls) if c == "gs_sweep"]
    assert ops.calls[smooths[0]:smooths[0] + 3] == ["gs_sweep"] * 3
    Q = run_example(G.oracle_gs(), 1, 3, fuse=False)
    assert Q.printed_values == P.printed_values


HEADER = """
Domain global< [0.0, 0.0, 0.0] to [1.0, 1.0, 1.0] >
Layout L< Real, Node >@all { ghostLayers = [1, 1, 1] with communication
 duplicateLayers = [1, 1, 1] with communication }
Field u< global, L, 0.0 >@all
Field f< global, L, None >@all
Field r< global, L, 0.0 >@all
Stencil A@all { [0, 0, 0] => 6.0
 [1, 0, 0] => -1.0
 [-1, 0, 0] => -1.0
 [0, 1, 0] => -1.0
 [0, -1, 0] => -1.0
 [0, 0, 1] => -1.0
 [0, 0, -1] => -1.0 }
"""
CELLS = """Layout C< Real, Cell >@all { ghostLayers = [1, 1, 1] with communication
 duplicateLayers = [0, 0, 0] }
Field cu< global, C, Neumann >@all
Field cf< global, C, None >@all
"""
GS_LOOP = "loop over u@finest %s { u@finest += 0.8 / diag ( A@finest ) * ( f@finest - A@finest * u@finest ) }"


def _program(body, knowledge=None, ops=None, header=HEADER, **kw):
    k = dict(dimensionality=3, minLevel=0, maxLevel=2)
    k.update(knowledge or {})
    return exa4.Exa4Program(header + "Function Application { %s }" % body, k, ops=ops or G.oracle_gs(), **kw)


def test_plain_loop_runs_and_counts_one_launch():
    ops = Tracing(G.oracle_gs())
    P = _program("apply bc to u@finest\n loop over f@finest { f@finest = 1.0 }\n" + GS_LOOP % "", ops=ops)
    P.run()
    Q = _program("apply bc to u@finest\n loop over f@finest { f@finest = 1.0 }")
    Q.run()
    assert ops.calls.count("gs_sweep") == 1 and P.launches == Q.launches + 1
    u = P.fields[("u", 2)]
    lu, lf = u.layout, P.fields[("f", 2)].layout
    ref = np.zeros(lu.size)
    fh = np.array(ops.to_host(P.fields[("f", 2)].data()), copy=True)
    b, e = P.domain.loop_bounds(lu)
    G.gs_nest(lu, ref, lf, fh, P.stencil("A", 2), 0.8 / 6.0, b, e)
    assert np.array_equal(ops.to_host(u.data()), ref) and np.abs(ref).max() > 0


@pytest.mark.parametrize("body,knowledge,what", [
    (GS_LOOP % "where i0 > 0", None, "`only` or `where`"),
    ("loop over u@finest only inner [0, 0, 0] { u@finest += 0.8 / diag ( A@finest ) * ( f@finest - A@finest * u@finest ) }", None, "`only` or `where`"),
    (GS_LOOP % "", dict(domain_rect_numFragsPerBlock_x=2), "2 fragments"),
    (GS_LOOP % "", dict(domain_rect_numBlocks_z=2), "2 fragments"),
    (GS_LOOP % "", dict(domain_rect_periodic_y=True), "periodic"),
])
def test_interpreter_refusals_by_name(body, knowledge, what):
    with pytest.raises(exa4.Exa4Unsupported, match="lexicographic Gauss-Seidel.*" + what):
        _program(body, knowledge).run()


def test_loop_under_color_with_is_unchanged():
    """Under `color with` the same statement is the red-black half sweep it always was."""
    ops = Tracing(G.oracle_gs())
    P = _program("color with { ( i0 + i1 + i2 ) % 2,\n" + GS_LOOP % "" + " }", ops=ops, fuse=False)
    P.run()
    assert "gs_sweep" not in ops.calls and ops.calls.count("stencil_op") == 2


def test_layer_without_gs_sweep_keeps_the_refusal():
    with pytest.raises(exa4.Exa4Unsupported, match="without colouring"):
        _program(GS_LOOP % "", ops=OracleOps()).run()


def test_two_blocks_are_refused():
    from exastencils_amd.domain import RectDomain

    class NoComm:
        def __init__(self, *a):
            pass

    dom = RectDomain(3, (1, 1, 2), 0, (1, 1, 1))
    P = exa4.Exa4Program(HEADER + "Function Application { %s }" % (GS_LOOP % ""), dict(dimensionality=3, minLevel=0, maxLevel=2),
                         ops=G.oracle_gs(), domain=dom, comm=NoComm())
    with pytest.raises(exa4.Exa4Unsupported, match="lexicographic Gauss-Seidel.*world_size"):
        P.run()


def test_cell_and_transformed_fields_are_refused():
    with pytest.raises(exa4.Exa4Unsupported, match="lexicographic Gauss-Seidel.*over cell field cu"):
        _program("loop over cu@finest { cu@finest += 0.8 / diag ( A@finest ) * ( cf@finest - A@finest * cu@finest ) }", header=HEADER + CELLS).run()
    # the colour split is applied where the kernel layer has transformed layouts: this one says it has
    ops = G.oracle_gs()
    ops.transform_field = lambda *a: None
    split = "LayoutTransformations {\n  transform u@finest with [x, y, z] => [x / 2, y, z, x % 2]\n}\n"
    with pytest.raises(exa4.Exa4Unsupported, match="lexicographic Gauss-Seidel.*colour-split field u"):
        _program(GS_LOOP % "", ops=ops, header=split + HEADER).run()
    # ... and the entry-fastest coefficient records where it has the transformation of stencil fields
    from test_exa4 import TRANSFORMED

    ops = G.oracle_gs()
    ops.transform_stencilfield = lambda *a: None
    with open(os.path.join(EX, "varcoeff3d.exa4")) as f:
        text = f.read()
    old = "u<next> = u<active> + ( ( 1.0 / diag ( A ) ) * 0.85 ) * ( g - A * u<active> )"
    assert text.count(old) == 1
    text = TRANSFORMED + text.replace(old, old.replace("u<next> =", "u<active> ="))
    with pytest.raises(exa4.Exa4Unsupported, match="lexicographic Gauss-Seidel.*entry-fastest coefficient field"):
        exa4.Exa4Program(text, dict(dimensionality=3, minLevel=1, maxLevel=3), ops=ops).run()


def test_nonlinear_loop_without_colouring_is_still_refused():
    """The semilinear in-place smoother without a colouring keeps its own refusal on a layer that has gs_sweep."""
    from nonlinear_ops import NonlinearOracleOps

    class Both(G.GsMixin, NonlinearOracleOps):
        pass

    with open(os.path.join(EX, "bratu2d_fas.exa4")) as f:
        text = f.read()
    assert text.count("u<next> = u<active> + omega") == 1
    bad = text.replace("u<next> = u<active> + omega", "u<active> = u<active> + omega")
    with pytest.raises(exa4.Exa4Unsupported, match="in-place nonlinear smoother without colouring"):
        exa4.Exa4Program(bad, dict(dimensionality=2, minLevel=1, maxLevel=3), ops=Both()).run()


def test_pending_loop_is_flushed_before_the_sweep():
    """`r = f - A * u` over the whole box stays pending for a restriction to absorb; the sweep that follows changes u, so the residual
    runs first -- with the u it was written for."""
    class Lazy(Tracing):
        pass

    ops = Lazy(G.oracle_gs())
    ops.residual_restrict = lambda *a, **k: (_ for _ in ()).throw(AssertionError("nothing to absorb here"))
    body = ("apply bc to u@finest\n loop over f@finest { f@finest = 1.0 }\n loop over r@finest { r@finest = f@finest - A@finest * u@finest }\n"
            + GS_LOOP % "" + "\n")
    P = _program(body, dict(maxLevel=3), ops=ops, fuse=True)
    P.run()
    assert [c for c in ops.calls if c in ("stencil_op", "gs_sweep")] == ["stencil_op", "gs_sweep"]
    r = np.array(ops.to_host(P.fields[("r", 3)].data()), copy=True)
    lay = P.fields[("r", 3)].layout
    b, e = P.domain.loop_bounds(lay)
    box = S.box_values(lay, r, b, e)
    assert np.all(box == 1.0)          # f - A * 0: the residual of the field before the sweep
