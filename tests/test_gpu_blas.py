"""The kernels of csrc/kernels_blas.hip and the expression interpreter (ExprEval, csrc/examg_common.h) on the GPU, through the product
library, against the references of tests/blas_cases.py -- which share no code with the library or the oracle and are themselves run
against the oracle in tests/test_blas_exact.py.  Whole allocations are compared, each argument in its own layout; an argument under
the colour split goes through examg_transform_field on the device and the reference stays on the plain layout.

  integer data   dot and sum == a Python integer; axpby, add_scalar, set equal integer arithmetic converted once;
  random data    elementwise kernels bit for bit against the one numpy expression of the form (form 4: two rounded products, then the
                 sum -- no fused multiply-add); reductions within (K + 1) * 2^-53 * fsum(|terms|) of math.fsum(terms), K the longest chain
                 of additions in the launch that blas_cases.reduction_plan restates (20 to 37 here).  This derived bound replaces the
                 undocumented 1e-13 of test_gpu_kernels.test_reductions;
  max_err        == Fraction arithmetic on dyadic data, the largest deviation planted at the first point, the last point and the end
                 of a row;
  programs       the exact class (const x y z + - * / neg fabs max min sqrt) == a Fraction evaluator; the libm class within the
                 per-function table blas_cases.LIBM_ULP of mpmath's correctly rounded value, in ulps of that value.

Measured on an MI355X: the random-data reductions lie at most 0.23 units of 2^-53 * fsum(|terms|) from math.fsum (37x5x3, dot; the
allowance is K + 1 >= 21 units; test_reductions prints every figure), the libm functions at most 1 ulp from the correctly rounded value
(cosh: 0).  Form 4 equals the two rounded products added: the library is built without contraction, as the header's "evaluated as the
reference statements are written" asks.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import blas_cases as B
from test_gpu_kernels import hip  # noqa: F401  (fixture)

from exastencils_amd.lib import ExamgError, ExprC, check

pytestmark = pytest.mark.gpu

BY_NAME = dict(ids=lambda c: c.name)
NAN = float("nan")


def dev(ops, a):
    return ops.from_host(np.array(a, dtype=np.float64, copy=True))


def host(ops, t):
    ops.synchronize()
    return ops.to_host(t).copy()


def to_split(ops, l, t):
    ts = dev(ops, np.full(l.split_x().size, B.SENTINEL))
    ops.transform_field(l.c_struct(), t, l.split_x().c_struct(), ts)
    return ts


def from_split(ops, l, ts):
    t = ops.new_array(l.size)
    ops.transform_field(l.split_x().c_struct(), ts, l.c_struct(), t)
    return t


class Arg:
    """A host array on the device in the layout the case asks for: plain, or under the colour split."""

    def __init__(self, ops, l, a, split):
        self.ops, self.l, self.split = ops, l, split
        t = dev(ops, a)
        self.t = to_split(ops, l, t) if split else t
        self.c = (l.split_x() if split else l).c_struct()

    def host(self):
        return host(self.ops, from_split(self.ops, self.l, self.t) if self.split else self.t)


def args(ops, case, x, y):
    lx, ly = B.layouts(case)
    sx, sy = B.split_of(case)
    return Arg(ops, lx, x, sx), Arg(ops, ly, y, sy)


# ---- elementwise ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", ["int", "random"])
@pytest.mark.parametrize("case", B.ELEMENTWISE, **BY_NAME)
def test_axpby_every_form(hip, case, data):
    lx, ly = B.layouts(case)
    box = B.box_of(case)
    x, y = B.field(lx.size, data, 5), B.field(ly.size, data, 6)
    for (a, b), form in zip(B.AXPBY_SCALARS, B.AXPBY_FORMS):
        X, Y = args(hip, case, x, y)
        hip.axpby(X.c, X.t, Y.c, Y.t, a, b, *box)
        want = B.ref_axpby(lx, x, ly, y, a, b, box, form=form, exact=data == "int")
        assert np.array_equal(Y.host(), want), (a, b, form)
        assert np.array_equal(X.host(), x)


@pytest.mark.parametrize("data", ["int", "random"])
@pytest.mark.parametrize("case", B.ELEMENTWISE, **BY_NAME)
def test_axpby_dev_every_reachable_form(hip, case, data):
    """a = sign * (num / den) resp. b = num / den with the inexact quotient 3.7 / 1.9, computed in that order."""
    lx, ly = B.layouts(case)
    box = B.box_of(case)
    x, y = B.field(lx.size, data, 5), B.field(ly.size, data, 6)
    num, den = dev(hip, [B.DEV_NUM]), dev(hip, [B.DEV_DEN])
    for which, a, b, sign, form in B.AXPBY_DEV:
        X, Y = args(hip, case, x, y)
        hip.axpby_dev(X.c, X.t, Y.c, Y.t, a, b, which, sign, num, den, *box)
        a2, b2 = B.dev_scalars(which, a, b, sign)
        assert np.array_equal(Y.host(), B.ref_axpby(lx, x, ly, y, a2, b2, box, form=form)), (which, form)
    assert host(hip, num)[0] == B.DEV_NUM and host(hip, den)[0] == B.DEV_DEN


@pytest.mark.parametrize("case", [B.ELEMENTWISE[0], B.ELEMENTWISE[6], B.ELEMENTWISE[7]], **BY_NAME)
def test_forms_that_ignore_y_do_not_read_it(hip, case):
    """"b==0: a*x" (include/examg.h): a y full of NaN leaves no NaN in the box, for b = 0.0 and b = -0.0, host and device scalars."""
    lx, ly = B.layouts(case)
    box = B.box_of(case)
    x, y = B.field(lx.size, "random", 5), np.full(ly.size, NAN)
    num, den = dev(hip, [B.DEV_NUM]), dev(hip, [B.DEV_DEN])
    zeros = np.zeros(ly.size)
    for a, b in [(2.5, 0.0), (1.0, 0.0), (0.5, -0.0), (1.0, -0.0), (None, 0.0)]:
        X, Y = args(hip, case, x, y)
        if a is None:
            hip.axpby_dev(X.c, X.t, Y.c, Y.t, 0.0, b, 0, -1.0, num, den, *box)
            a = B.dev_scalars(0, 0.0, b, -1.0)[0]
        else:
            hip.axpby(X.c, X.t, Y.c, Y.t, a, b, *box)
        want = B.ref_axpby(lx, x, ly, zeros, a, b, box)
        got = Y.host()
        inside = B.view(ly, got)[B.box_index(ly, *box)]
        assert not np.isnan(inside).any() and np.array_equal(inside, B.view(ly, want)[B.box_index(ly, *box)])
        assert np.isnan(got).sum() == ly.size - inside.size                      # and y is untouched outside the box


@pytest.mark.parametrize("data", ["int", "random"])
@pytest.mark.parametrize("case", B.ELEMENTWISE, **BY_NAME)
def test_set_and_add_scalar(hip, case, data):
    lx, ly = B.layouts(case)
    box = B.box_of(case)
    x, y = B.field(lx.size, data, 5), B.field(ly.size, data, 6)
    for v in (-2.75, 0.0):
        X, Y = args(hip, case, x, y)
        hip.set(X.c, X.t, v, *box)
        assert np.array_equal(X.host(), B.ref_set(lx, x, v, box))
    for c in (-0.375, 3.0):
        X, Y = args(hip, case, x, y)
        hip.add_scalar(Y.c, Y.t, c, *box)
        assert np.array_equal(Y.host(), B.ref_add_scalar(ly, y, c, box, exact=data == "int"))
    for b, e in B.EMPTY_BOXES:                                                    # an empty box writes nothing
        X, Y = args(hip, case, x, y)
        hip.set(X.c, X.t, 1.0, b, e)
        hip.add_scalar(Y.c, Y.t, 1.0, b, e)
        hip.axpby(X.c, X.t, Y.c, Y.t, 2.0, 3.0, b, e)
        assert np.array_equal(X.host(), x) and np.array_equal(Y.host(), y)


# ---- reductions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", ["int", "random"])
@pytest.mark.parametrize("case", B.REDUCTIONS, **BY_NAME)
def test_reductions(hip, case, data):
    """examg_dot and examg_sum on every route of the table: == the Python integer on integer data; on random data within
    (K + 1) * 2^-53 * fsum(|terms|) of math.fsum(terms) -- the derived bound that replaces the 1e-13 of test_gpu_kernels.test_reductions.
    The same call twice gives the same bits."""
    x, y = B.reduction_inputs(case.name, data)
    X, Y = args(hip, case, x, y)
    box = B.box_of(case)
    for sum_only in (False, True):
        plan = B.plan_of(case, sum_only)
        want, unit = B.reduction_reference(case.name, data, sum_only)
        run = (lambda: hip.sum(X.c, X.t, *box, out=dev(hip, [NAN]))) if sum_only else (lambda: hip.dot(X.c, X.t, Y.c, Y.t, *box, out=dev(hip, [NAN])))
        got, again = host(hip, run())[0], host(hip, run())[0]
        assert got == again and math.copysign(1.0, got) == math.copysign(1.0, again)
        if data == "int":
            assert got == want, (plan, got, want)
        else:
            print("%s %s: %s K=%d |got - fsum| = %.2f units" % (case.name, "sum" if sum_only else "dot", plan.kernel, plan.K, abs(got - want) / unit))
            assert abs(got - want) <= (plan.K + 1) * unit, (plan, got, want)


@pytest.mark.parametrize("name", B.NEEDLE_CASES)
def test_needles_sum_to_one(hip, name):
    """All zeros but a single 1 -- at the first and the last point of the first and of the last row, at the end of a row in the middle
    (the tail element of odd rows), in the outermost ghost layer with the box grown to it -- and 2^20 + 1 everywhere outside the box."""
    case = next(c for c in B.REDUCTIONS if c.name == name)
    lx, ly = B.layouts(case)
    for p, box in B.needle_points(case):
        X, Y = args(hip, case, B.needle_field(lx, box, p), B.needle_field(ly, box, p))
        assert host(hip, hip.dot(X.c, X.t, Y.c, Y.t, *box))[0] == 1.0, (p, box)
        assert host(hip, hip.sum(X.c, X.t, *box))[0] == 1.0, (p, box)
        assert host(hip, hip.sum(Y.c, Y.t, *box))[0] == 1.0, (p, box)


@pytest.mark.parametrize("lays", ["own", "split_x"])
def test_empty_boxes_give_plus_zero(hip, lays):
    """end == begin in one dimension, end < begin in two: +0.0 over the NaN that was there, the work buffer untouched."""
    case = next(c for c in B.REDUCTIONS if c.lays == lays)
    lx, ly = B.layouts(case)
    X, Y = args(hip, case, B.field(lx.size, "random", 1), B.field(ly.size, "random", 2))
    expr = ExprC.from_program(B.prog("x y *"))
    for b, e in B.EMPTY_BOXES:
        assert B.reduction_plan((b, e), lx, ly).kernel == "empty"
        hip._work.fill_(B.SENTINEL)
        outs = [hip.dot(X.c, X.t, Y.c, Y.t, b, e, out=dev(hip, [NAN])), hip.sum(X.c, X.t, b, e, out=dev(hip, [NAN])),
                hip.max_err_expr(X.c, X.t, B.MGEOM, expr, b, e, out=dev(hip, [NAN]))]
        for o in outs:
            v = host(hip, o)[0]
            assert v == 0.0 and math.copysign(1.0, v) == 1.0
        assert bool((hip._work == B.SENTINEL).all())


@pytest.mark.parametrize("case", B.MAXERR, **BY_NAME)
def test_max_err_is_exact_and_finds_the_planted_point(hip, case):
    l = B.layouts(case)[0]
    expr = ExprC.from_program(B.prog(case.program))
    box = B.box_of(case)
    f = hip.max_err_expr_cell if case.lays == "cell" else hip.max_err_expr
    base = B.maxerr_base(case.name)[0]
    X = Arg(hip, l, base, B.split_of(case)[0])
    small = host(hip, f(X.c, X.t, B.MGEOM, expr, *box))[0]
    assert 0.0 < small <= 0.25                                # without a planted point: the largest of the small deviations
    for where in B.maxerr_plants(case):
        a, want = B.maxerr_field(case, where)
        X = Arg(hip, l, a, B.split_of(case)[0])
        got = host(hip, f(X.c, X.t, B.MGEOM, expr, *box))[0]
        assert got == want == 3.0, (where, got)


def test_max_err_passes_over_nan_points(hip):
    """Pinned, not derived: the header says "max |x - e|" and no more.  A point whose deviation is NaN does not enter the maximum --
    fmax in the kernel, `if (e > m) m = e` in the oracle's loop (orc_max_err_fn), a comparison in the generated `reduction(max : err)`
    loop the kernel stands for.  The NaN sits in lane 0 of the first workgroup and at the end of a row; the maximum is the planted 3."""
    case = B.MAXERR[0]
    l = B.layouts(case)[0]
    b, e = B.box_of(case)
    a, want = B.maxerr_field(case, "last")
    for p in (b, B.maxerr_plants(case)["row_end"]):
        B.view(l, a)[B.box_index(l, p, tuple(v + 1 for v in p))] = NAN
    X = Arg(hip, l, a, False)
    assert host(hip, hip.max_err_expr(X.c, X.t, B.MGEOM, ExprC.from_program(B.prog(case.program)), b, e))[0] == want == 3.0


# ---- the interpreter ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(B.EXACT_PROGRAMS))
def test_exact_programs(hip, name):
    """== the Fraction evaluator, at node positions and (where the values stay fp64 numbers) at cell centres; the rest of the array
    keeps its sentinel.  examg_max_err_expr of the filled array is then exactly 0."""
    program, geom, (b, e) = B.EXACT_PROGRAMS[name]
    l = B.EXPR_LAYOUT
    expr = ExprC.from_program(program)
    t = dev(hip, np.full(l.size, B.SENTINEL))
    hip.fill_expr(l.c_struct(), t, geom, expr, b, e)
    exp = np.full(l.size, B.SENTINEL)
    B.view(l, exp)[B.box_index(l, b, e)] = B.exact_values(program, geom, b, e)
    got = host(hip, t)
    assert np.array_equal(got, exp), np.argwhere(B.view(l, got) != B.view(l, exp))[:4]
    assert host(hip, hip.max_err_expr(l.c_struct(), t, geom, expr, b, e))[0] == 0.0
    if name != "4_div_by_x":
        hip.fill_expr_cell(l.c_struct(), t, geom, expr, b, e)
        B.view(l, exp)[B.box_index(l, b, e)] = B.exact_values(program, geom, b, e, cell=True)
        assert np.array_equal(host(hip, t), exp)
        assert host(hip, hip.max_err_expr_cell(l.c_struct(), t, geom, expr, b, e))[0] == 0.0


def test_programs_past_the_limits_are_refused(hip):
    l = B.EXPR_LAYOUT
    t = dev(hip, np.full(l.size, B.SENTINEL))
    b, e = B.EBOX
    with pytest.raises(ValueError, match="257 instructions"):
        ExprC.from_program(B.long_program() + [("neg", None)])
    claims = ExprC.from_program(B.long_program())
    claims.n = 257
    for expr, text in ((claims, "too long"), (ExprC.from_program(B.deep_program(25)), "stack deeper than 24")):
        with pytest.raises(ExamgError, match=text):
            hip.fill_expr(l.c_struct(), t, B.EGEOM, expr, b, e)
        with pytest.raises(ExamgError, match=text):
            hip.max_err_expr(l.c_struct(), t, B.EGEOM, expr, b, e)
        with pytest.raises(ExamgError, match=text):
            hip.apply_dirichlet_expr(l.c_struct(), t, B.EGEOM, expr, 63)
    assert np.array_equal(host(hip, t), np.full(l.size, B.SENTINEL))


@pytest.mark.parametrize("fn", B.LIBM_OPS)
def test_libm_functions_within_the_table(hip, fn):
    """One function per program on 40 arguments in [0.25, 2.0] (pow: 3 exponents), against mpmath at 50 digits rounded once, in ulps of
    that value; the bound is the error measured on an MI355X plus one (blas_cases.LIBM_ULP)."""
    l = B.LIBM_LAYOUT
    t = dev(hip, np.zeros(l.size))
    hip.fill_expr(l.c_struct(), t, B.LGEOM, ExprC.from_program(B.libm_program(fn)), *B.LBOX)
    got = B.view(l, host(hip, t))[B.box_index(l, *B.LBOX)]
    err = B.ulp_error(got, B.libm_reference(fn))
    print("libm %s: %.0f ulp" % (fn, err))
    measured, bound = B.LIBM_ULP[fn]
    assert bound == measured + 1 and err <= bound


# ---- boundary fills ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lname", sorted(B.FILL_LAYOUTS))
def test_boundary_fills(hip, lname):
    """examg_apply_dirichlet_expr: the duplicate plane of each face of the mask, tangentially GLB..GRE; examg_fill_dup_faces_expr: the
    same plane, tangentially DLB..DRE.  Exact values; everything else keeps its sentinel."""
    l = B.FILL_LAYOUTS[lname]
    expr = ExprC.from_program(B.FILL_PROGRAM)
    for mask in B.fill_masks(l.nd):
        t = dev(hip, np.full(l.size, B.SENTINEL))
        hip.apply_dirichlet_expr(l.c_struct(), t, B.FGEOM, expr, mask)
        assert np.array_equal(host(hip, t), B.ref_boundary_fill(lname, mask, True)), mask
        t = dev(hip, np.full(l.size, B.SENTINEL))
        check(hip.L.examg_fill_dup_faces_expr(C.byref(l.c_struct()), hip.ptr(t), C.byref(B.FGEOM), C.byref(expr), mask, hip._stream()),
              "examg_fill_dup_faces_expr")
        assert np.array_equal(host(hip, t), B.ref_boundary_fill(lname, mask, False)), mask


# ---- data movers ----------------------------------------------------------------------------------------------------------------------
def test_pack_and_unpack_every_exchange_box(hip):
    l = B.PACK_LAYOUT
    x = np.arange(l.size, dtype=np.float64)
    X = dev(hip, x)
    for box in B.pack_boxes():
        want = B.ref_pack(l, x, box)
        buf = dev(hip, np.full(want.size + 3, B.SENTINEL))
        hip.pack(l.c_struct(), X, buf, *box)
        assert np.array_equal(host(hip, buf), np.concatenate([want, [B.SENTINEL] * 3])), box
        src = np.arange(want.size + 3, dtype=np.float64) + 0.5
        t = dev(hip, np.full(l.size, B.SENTINEL))
        hip.unpack(l.c_struct(), t, dev(hip, src), *box)
        assert np.array_equal(host(hip, t), B.ref_unpack(l, np.full(l.size, B.SENTINEL), src, box)), box
    assert np.array_equal(host(hip, X), x)


@pytest.mark.parametrize("gi,ge,align", B.EXTERNAL)
def test_external_copies(hip, gi, ge, align):
    li, le = B.external_layouts(gi, ge, align)
    xi, xe = np.arange(li.size, dtype=np.float64), np.arange(le.size, dtype=np.float64) + 0.5
    dest = dev(hip, np.full(le.size, B.SENTINEL))
    hip.copy_to_external(li.c_struct(), dev(hip, xi), le.c_struct(), dest)
    assert np.array_equal(host(hip, dest), B.ref_external(li, xi, le, np.full(le.size, B.SENTINEL)))
    dest = dev(hip, np.full(li.size, B.SENTINEL))
    hip.copy_from_external(le.c_struct(), dev(hip, xe), li.c_struct(), dest)
    assert np.array_equal(host(hip, dest), B.ref_external(le, xe, li, np.full(li.size, B.SENTINEL)))


@pytest.mark.parametrize("lname", sorted(B.TRANSFORM_LAYOUTS))
def test_transform_field(hip, lname):
    """Direct placement against the index map of the colour split, and the round trip; odd and even total x extent."""
    l = B.TRANSFORM_LAYOUTS[lname]
    x = np.arange(l.size, dtype=np.float64)
    ts = to_split(hip, l, dev(hip, x))
    assert np.array_equal(host(hip, ts), B.ref_split(l, x))
    back = dev(hip, np.full(l.size, B.SENTINEL))
    hip.transform_field(l.split_x().c_struct(), ts, l.c_struct(), back)
    assert np.array_equal(host(hip, back), x)
    s = np.arange(l.split_x().size, dtype=np.float64) + 0.5
    hip.transform_field(l.split_x().c_struct(), dev(hip, s), l.c_struct(), back)
    assert np.array_equal(host(hip, back), B.ref_unsplit(l, s))


@pytest.mark.parametrize("size", B.SF_SIZES)
@pytest.mark.parametrize("K", B.SF_ENTRIES)
def test_transform_stencilfield(hip, K, size):
    l = B.sf_layout(size)
    src = np.arange(K * size, dtype=np.float64)
    for to_aos in (True, False):
        dst = dev(hip, np.full(K * size + 5, B.SENTINEL))
        hip.transform_stencilfield(l.c_struct(), K, dev(hip, src), dst, to_aos)
        assert np.array_equal(host(hip, dst), np.concatenate([B.ref_transform_sf(src, size, K, to_aos), [B.SENTINEL] * 5])), to_aos


@pytest.mark.parametrize("n", B.RANDOM_SIZES)
def test_fill_random_is_the_restated_generator(hip, n):
    """Bit for bit, the array behind the last value untouched; the small sizes against the Python-integer form, the large one against
    its numpy form (equal to it: test_blas_exact)."""
    for seed in B.RANDOM_SEEDS:
        t = dev(hip, np.full(n + 2, B.SENTINEL))
        check(hip.L.examg_fill_random(hip.ptr(t), n, seed, hip._stream()), "examg_fill_random")
        got = host(hip, t)
        want = [B.random_value(seed, i) for i in range(n)] if n < 1000 else B.random_field(n, seed)
        assert np.array_equal(got[:n], want) and got[n] == got[n + 1] == B.SENTINEL, seed
