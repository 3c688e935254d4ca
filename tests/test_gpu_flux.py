"""The flux-form kernels (examg_flux_step on both routes, examg_reduce_expr_cell, the EXAMG_BC_NEGATE kind of examg_apply_bc_cell) on the
MI355X against the numpy restatement (tests/flux_ops.py), and the shallow-water example on the HIP kernel layer.

Comparisons are bitwise over the WHOLE arrays (sentinels outside the box, every input with its copy): the programs of the step cases use
+ - * / only, every instruction one IEEE rounding.  The wave-speed program adds fabs, max and sqrt, which are exact or correctly rounded
on both sides.  Shapes, boxes, layouts and data: tests/flux_cases.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import flux_cases as K  # noqa: E402
from flux_ops import BC_NEGATE, REDUCE_MAX, REDUCE_MIN, FluxOracleOps  # noqa: E402

from exastencils_amd import lib  # noqa: E402
from exastencils_amd.flux import field_program  # noqa: E402
from exastencils_amd.layout import FieldLayout  # noqa: E402
from exastencils_amd.lib import ExamgError  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from exastencils_amd.ops import HipOps

    return HipOps(0)


@pytest.fixture(scope="module")
def hipd():
    """The debug library: examg_debug_flux_route forces either kernel."""
    from exastencils_amd.ops import HipOps

    ops = HipOps(0, lib.DBG_LIB_PATH)
    yield ops
    ops.L.examg_debug_flux_route(0)


@pytest.fixture(scope="module")
def orc():
    return FluxOracleOps()


def host(ops, t):
    ops.synchronize()
    return np.array(ops.to_host(t), dtype=np.float64, copy=True)


def same_bits(got, want, what):
    if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
        bad = got.view(np.uint64) != want.view(np.uint64)
        raise AssertionError("%s: %d of %d values differ, max abs %.3e" % (what, int(bad.sum()), bad.size, float(np.nanmax(np.abs(got - want)[bad]))))


def step(ops, lin, lout, data, spec, b, e, call="flux_step"):
    """One call from host data; the inputs and outputs afterwards (and what the call returned)."""
    ins = [ops.from_host(a.copy()) for a in data]
    outs = [ops.from_host(np.full(int(lout.size), K.SENTINEL)) for _ in spec.comps]
    r = getattr(ops, call)(lin.c_struct(), ins, lout.c_struct(), outs, spec, b, e)
    return [host(ops, t) for t in ins], [host(ops, t) for t in outs], r


SPECS = [("swe", K.swe_spec, K.swe_data), ("asym1", lambda: K.asym_spec(1), K.asym_data), ("asym4", lambda: K.asym_spec(4), K.asym_data)]


@pytest.mark.parametrize("shape", K.SHAPES, ids=["%dx%d" % s for s in K.SHAPES])
def test_both_routes_give_numpys_bits(hip, hipd, orc, shape):
    runs = 0
    for align in (0, 2):
        lin, lout = K.layouts(shape, align)
        for sname, make, make_data in SPECS:
            spec = make()
            data = make_data(np.random.default_rng(shape[0] + 7 * align + len(sname)), lin)
            for bname, (b, e) in K.boxes(shape):
                what = "%dx%d align %d %s box %s" % (shape + (align, sname, bname))
                _, want, _ = step(orc, lin, lout, data, spec, b, e)
                inside = K.box_mask(lout, b, e)
                for route in (lib.FLUX_GATHER, lib.FLUX_MARCH, 0):
                    ops = hip if route == 0 else hipd
                    if route:
                        assert hipd.L.examg_debug_flux_route(route) == 0
                        assert step(hipd, lin, lout, data, spec, b, e, "flux_route")[2] == route, what
                    ins, got, _ = step(ops, lin, lout, data, spec, b, e)
                    for k, (x, x0) in enumerate(zip(ins, data)):
                        same_bits(x, x0, "%s route %d: input %d was written" % (what, route, k))
                    for c, (g, w) in enumerate(zip(got, want)):
                        same_bits(g, w, "%s route %d component %d" % (what, route, c))
                        assert np.all(g[~inside] == K.SENTINEL) and not np.any(g[inside] == K.SENTINEL), what
                    runs += 1
    assert runs == 2 * 3 * 3 * 3


def test_route_answers(hip, hipd):
    """examg_flux_route: the default of the product library, either kernel by name in the debug library, 0 for an empty box, -1 refused."""
    shape = (66, 5)
    lin, lout = K.layouts(shape, 0)
    data = K.swe_data(np.random.default_rng(1), lin)
    spec = K.swe_spec()
    b, e = K.boxes(shape)[0][1]
    assert step(hip, lin, lout, data, spec, b, e, "flux_route")[2] == lib.FLUX_DEFAULT
    for route in (lib.FLUX_GATHER, lib.FLUX_MARCH):
        hipd.L.examg_debug_flux_route(route)
        assert step(hipd, lin, lout, data, spec, b, e, "flux_route")[2] == route
    hipd.L.examg_debug_flux_route(0)
    assert step(hipd, lin, lout, data, spec, b, e, "flux_route")[2] == lib.FLUX_DEFAULT
    assert step(hip, lin, lout, data, spec, [3, 2, 0], [3, 4, 1], "flux_route")[2] == 0
    assert step(hip, lin, lout, data, spec, [0, 0, 0], [shape[0] + 1, shape[1], 1], "flux_route")[2] == -1
    assert hipd.L.examg_debug_flux_route(7) != 0


def _bad(spec, **kw):
    import copy

    s = copy.deepcopy(spec)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _refusals(shape):
    """(name, text of the library's refusal, lin, lout, spec, box, alias)"""
    lin, lout = K.layouts(shape, 0)
    full = K.boxes(shape)[0][1]
    base = K.swe_spec()
    c0 = base.comps[0]
    t0 = c0.terms[0]

    def comp0(**kw):
        import dataclasses

        return [dataclasses.replace(c0, **kw)] + base.comps[1:]

    def term0(**kw):
        import dataclasses

        return comp0(terms=(dataclasses.replace(t0, **kw),) + c0.terms[1:])

    def prog0(prog):
        return [prog] + base.programs[1:]

    node = FieldLayout.node(2, shape, 1)
    return [
        ("3-D", "not built", FieldLayout.cell(3, shape + (4,), 1), FieldLayout.cell(3, shape + (4,), 1), base, full, False),
        ("node layout", "duplicate layers", node, lout, base, ([0, 0, 0], [3, 3, 1]), False),
        ("colour split", "colour-split", FieldLayout.cell(2, shape, 1, align=2).split_x(), lout, base, full, False),
        ("box leaves lout", "leaves the output", lin, lout, base, ([-3, 0, 0], [4, 4, 1]), False),
        ("box + 1 leaves lin", "grown by one cell leaves the input", lin, lout, base, ([-1, 0, 0], [4, 4, 1]), False),
        ("out is in", "overlaps input", lin, lin, base, full, True),
        ("field index", "names field", lin, lout, _bad(base, comps=comp0(field=4)), full, False),
        ("program index", "names program", lin, lout, _bad(base, comps=term0(prog=6)), full, False),
        ("diagonal term", "unit axis offset", lin, lout, _bad(base, comps=term0(plus=(1, 1, 0))), full, False),
        ("reach 2 term", "unit axis offset", lin, lout, _bad(base, comps=term0(minus=(-2, 0, 0))), full, False),
        ("diagonal entry", "is not the centre or a unit axis offset", lin, lout, _bad(base, comps=comp0(offsets=(K.W, K.E, K.S, (1, 1, 0)))), full, False),
        ("reach 2 entry", "is not the centre or a unit axis offset", lin, lout, _bad(base, comps=comp0(offsets=(K.W, K.E, K.S, (0, 2, 0)))), full, False),
        ("empty stencil", "is empty", lin, lout, _bad(base, comps=comp0(offsets=(), coefs=())), full, False),
        ("empty program", "program 0 is empty", lin, lout, _bad(base, programs=prog0([])), full, False),
        ("long program", "instructions", lin, lout, _bad(base, programs=prog0(K.P_LONG[:-1] + [K.op("neg"), K.op("neg")])), full, False),
        ("deep program", "deeper than", lin, lout, _bad(base, programs=prog0([K.push(0)] * 9 + [K.op("+")] * 8)), full, False),
        ("underflow", "underflows", lin, lout, _bad(base, programs=prog0([K.push(0), K.op("+")])), full, False),
        ("two values", "exactly one value", lin, lout, _bad(base, programs=prog0([K.push(0), K.push(1)])), full, False),
        ("field operand out of range", "reads field", lin, lout, _bad(base, programs=prog0([K.push(5)])), full, False),
        ("EXAMG_OP_U", "EXAMG_OP_U", lin, lout, _bad(base, programs=prog0([("op", 22)])), full, False),
        ("position", "reads the position", lin, lout, _bad(base, programs=prog0([("op", 1)])), full, False),
        ("cell width", "reads a cell width", lin, lout, _bad(base, programs=prog0([("op", 23)])), full, False),
        ("too many terms", "terms", lin, lout, _bad(base, comps=comp0(terms=(t0,) * 5)), full, False),
        ("too many programs", "programs", lin, lout, _bad(base, programs=base.programs + [K.SWE_F0] * 3), full, False),
    ]


def test_refusals_launch_nothing(hip, hipd):
    shape = (8, 8)
    rng = np.random.default_rng(3)
    cases = _refusals(shape)
    for name, text, lin, lout, spec, (b, e), alias in cases:
        data = [rng.uniform(5.0, 15.0, int(lin.size)) for _ in range(4)]
        for ops, route in ((hip, 0), (hipd, lib.FLUX_GATHER), (hipd, lib.FLUX_MARCH)):
            if route:
                hipd.L.examg_debug_flux_route(route)
            ins = [ops.from_host(a.copy()) for a in data]
            outs = ins[:3] if alias else [ops.from_host(np.full(int(lout.size), K.SENTINEL)) for _ in range(3)]
            if alias:
                ins = [ins[3], ins[0], ins[1], ins[2]]      # out[0] is in[1]
            with pytest.raises(ExamgError, match=text):
                ops.flux_step(lin.c_struct(), ins, lout.c_struct(), outs, spec, b, e)
            assert ops.flux_route(lin.c_struct(), ins, lout.c_struct(), outs, spec, b, e) == -1, name
            if not alias:
                for t in outs:
                    assert np.all(host(ops, t) == K.SENTINEL), name
                for t, a in zip(ins, data):
                    same_bits(host(ops, t), a, name)
    assert len({c[1] for c in cases}) >= 18      # each refusal has a text of its own (the two offsets share one per kind)
    # EXAMG_OP_FIELD* is refused by the entry points that take the other program types
    from exastencils_amd.field import laplace_unit

    lay = FieldLayout.node(2, shape, 1)
    u, d = hip.new_array(lay.size), hip.new_array(lay.size)
    bad = field_program([K.push(0)])
    with pytest.raises(ExamgError, match="unknown opcode"):
        hip.nl_op(lib.NL_APPLY, lay.c_struct(), u, lay.c_struct(), u, None, None, lay.c_struct(), d, laplace_unit(2), bad, [1, 1, 0], [3, 3, 1])
    e256 = lib.ExprC()
    e256.n, e256.op[0] = 1, lib.OP_FIELD0
    with pytest.raises(ExamgError, match="unknown opcode"):
        hip.fill_expr(lay.c_struct(), u, _geom(shape), e256, [1, 1, 0], [3, 3, 1])


def _geom(shape):
    g = lib.GeomC()
    for d in range(3):
        g.pos_begin[d], g.h[d] = 0.0, 1.0 / shape[d] if d < 2 else 1.0
    return g


def test_empty_box_is_a_no_op(hip, orc):
    shape = (8, 8)
    lin, lout = K.layouts(shape, 0)
    data = K.swe_data(np.random.default_rng(4), lin)
    for ops in (hip, orc):
        ins, outs, _ = step(ops, lin, lout, data, K.swe_spec(), [2, 5, 0], [6, 5, 1])
        for t in outs:
            assert np.all(t == K.SENTINEL)
        for t, a in zip(ins, data):
            same_bits(t, a, "empty box")


@pytest.mark.parametrize("shape", K.SHAPES, ids=["%dx%d" % s for s in K.SHAPES])
def test_reductions_equal_numpy_exactly(hip, orc, shape):
    """max and min of the wave-speed program and of h + b.  Every ghost cell holds 1e300 (for the minima, -1e300 in b's): a read outside
    the box shows in the result."""
    progs = {"wave speed": field_program(K.WAVE_SPEED), "h + b": field_program(K.SURFACE)}
    for align in (0, 2):
        lin, _ = K.layouts(shape, align)
        ghost = ~K.box_mask(lin, [0, 0, 0], [shape[0], shape[1], 1])
        for op in (REDUCE_MAX, REDUCE_MIN):
            data = K.swe_data(np.random.default_rng(11 + shape[0] + align), lin)
            for k, a in enumerate(data):
                a[ghost] = -1e300 if (op == REDUCE_MIN and k == 3) else 1e300
            for bname, (b, e) in K.boxes(shape):
                for pname, prog in progs.items():
                    got = host(hip, hip.reduce_expr_cell(op, lin.c_struct(), [hip.from_host(a.copy()) for a in data], prog, b, e))
                    want = host(orc, orc.reduce_expr_cell(op, lin.c_struct(), [orc.from_host(a.copy()) for a in data], prog, b, e))
                    same_bits(got, want, "%s of %s, box %s, align %d" % ("max" if op == REDUCE_MAX else "min", pname, bname, align))
                    assert abs(got[0]) < 1e3
    # an empty box gives the identity, and a box that leaves the allocation is refused
    x = [hip.from_host(a) for a in K.swe_data(np.random.default_rng(1), lin)]
    assert host(hip, hip.reduce_expr_cell(REDUCE_MAX, lin.c_struct(), x, progs["h + b"], [1, 1, 0], [1, 2, 1]))[0] == -np.inf
    assert host(hip, hip.reduce_expr_cell(REDUCE_MIN, lin.c_struct(), x, progs["h + b"], [1, 1, 0], [1, 2, 1]))[0] == np.inf
    with pytest.raises(ExamgError, match="leaves the allocation"):
        hip.reduce_expr_cell(REDUCE_MAX, lin.c_struct(), x, progs["h + b"], [-5, 0, 0], [2, 2, 1])
    with pytest.raises(ExamgError, match="unknown reduction"):
        hip.reduce_expr_cell(5, lin.c_struct(), x, progs["h + b"], [0, 0, 0], [2, 2, 1])


def test_negate_boundary_kind(hip, orc):
    """ghost = -interior on every single-face mask and on the full mask, in 2-D and 3-D; edge and corner ghosts keep their sentinel (the
    whole array is compared).  The existing kinds go through the same kernel and keep their bits."""
    for nd, shape in ((2, (9, 6)), (3, (5, 4, 3))):
        lay = FieldLayout.cell(nd, shape, 1)
        a = np.random.default_rng(nd).uniform(-1.0, 1.0, int(lay.size))
        a[~_inner_mask(lay)] = K.SENTINEL
        masks = [1 << f for f in range(2 * nd)] + [(1 << (2 * nd)) - 1]
        for mask in masks:
            for kind in (BC_NEGATE, lib.BC_NEUMANN):
                got, want = hip.from_host(a.copy()), orc.from_host(a.copy())
                hip.apply_bc_cell(lay.c_struct(), got, _geom(shape + (1,) * (3 - nd)), kind, None, mask)
                orc.apply_bc_cell(lay.c_struct(), want, _geom(shape + (1,) * (3 - nd)), kind, None, mask)
                same_bits(host(hip, got), host(orc, want), "%d-D mask %d kind %d" % (nd, mask, kind))
                written = host(hip, got) != a
                assert int(written.sum()) == sum(np.prod([shape[t] for t in range(nd) if t != f // 2]) for f in range(2 * nd) if mask >> f & 1)
    with pytest.raises(ExamgError, match="unknown kind"):
        hip.apply_bc_cell(lay.c_struct(), hip.from_host(a.copy()), _geom(shape), 3, None, 1)


def _inner_mask(lay):
    return K.box_mask(lay, [0, 0, 0], [lay.inner[0], lay.inner[1], lay.inner[2]])


# -- the example on the HIP kernel layer ---------------------------------------------------------------------------------------------
def _swe(ops, **kw):
    from exastencils_amd import exa4

    d = os.path.join(ROOT, "examples", "exa4")
    P = exa4.load(os.path.join(d, "swe2d.exa4"), os.path.join(d, "swe2d.knowledge"), ops=ops, **kw)
    P.run()
    return P


def test_swe2d_prints_the_golden_lines_with_and_without_graph_replay(hip):
    """652 adaptive steps on 256^2 cells, about 7500 small launches per run.  The printed numbers pass through the device's sqrt and
    sin (start values) and six digits: the rule of tests/flux_cases.py: check_golden.  Replayed functions (the wall functions and
    AdvanceTimestep; Update reads dt and is interpreted) must print the text of the interpreted run."""
    plain = _swe(hip, auto_graph=False)
    K.check_golden(plain.out)
    graphs = _swe(hip, auto_graph=True)
    assert graphs.graph_replays > 0
    assert graphs.out == plain.out
