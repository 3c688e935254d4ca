"""The one-kernel coarse-grid CG on the GPU -- k_cg_coarse and k_cg_coarse_lds of csrc/kernels_coarse.hip, through
examg_cg_coarse_variant of the product library and of the debug build -- against the independent reference of tests/coarse_cases.py:
whole arrays, each argument in its own layout, anisotropic stencils, boxes on either side of each routing bound.

Every case first asks the debug build which kernel the call takes (examg_debug_cg_route; nothing is launched) and asserts the form
of the table in coarse_cases.CASES; examg_debug_cg(0) forces the global-memory form.  Then:

  random data    sol, res, p, ap, info[1] and info[2] within 64 * max(delta_ref, eps * max |field|) of R64 (never looser than 1e-10
                 of the field; delta_ref = max |R64 - RLD| from the two precisions of the reference, never from GPU output),
                 info[0] and info[3] equal, rhs and the coefficients untouched, every point outside the box equal to the
                 reference's bit for bit (the input's bits, or 0.0 on the planes `apply bc` writes);
  equalities     that no summation order can break: the LDS-resident form equals the global-memory form and the product library
                 equals the debug build, on all arrays and info; two runs give the same bits; EXAMG_CG_ZERO_START equals examg_set +
                 the solver; on integer data with the integer stencils r, alpha, and after one iteration sol, res, ap equal R64;
  limits         the info[3] count at max_it 0, 1, 2 and a generous limit; info == NULL; the empty box; every refusal of the
                 entry point, with all arrays unchanged.

Three behaviours the two forms must share, each pinned down here:
  - max_it = 0 leaves ap untouched: the solver computes the residual, its norm and the first search direction only
    (test_iteration_limits, test_exact_data_is_bit_for_bit);
  - under `apply bc`, a layout without duplicate planes (a cell layout) takes the global-memory form, which reads the ghost cells
    around the box as they are: the zero halo of the LDS form stands for planes that `apply bc` zeroes, and such a layout has none
    (include/examg.h; test_route_is_the_table_s, test_fixed_iterations_from_raw_data[cell_7x6x5]);
  - the LDS form loads no halo plane below or above the single plane of a 2-D field (the 2-D cases under EXAMG_CG_NO_BC).

The unit of a comparison is max(delta_ref, eps * max |field|) with the maximum over the box: at rel_tol 1e-8 the residual
is 1e-8 to 1e-4 there and its unit 1e-21 to 1e-16, whatever the data around the box holds.  Solves that end by exact termination (coarse_cases.EXACT_TERMINATION:
3x3x3 at 1e-8, 1x1x1) leave a residual and an info[2] that are rounding noise; they keep the 64 units of delta_ref, and only the
1e-10 cap is taken of the last search direction (coarse_cases.tolerance).

Largest |GPU - R64| / unit measured on an MI355X, per case, over all flags, tolerances, forms and the six compared outputs (the
allowance is 64, or 1e-10 of the field if that is less: 40 units at the least, 16x16x17):

  case                random data   3 iterations, raw data   integer data, max_it 1 (p, info[2])
  1x1x1                   0.00              -                       0.00
  3x3x3                   5.62             0.90                     0.00
  15x15x15               14.94             1.00                     0.59
  16x16x16                6.77             1.09                     0.00
  17x16x15               11.79             0.78                      -
  64x8x7                  4.78             0.55                     0.00
  200x4x4                 4.72             1.73                      -
  220x4x4                 8.14              -                       0.84
  16x16x17                4.84              -                       0.00
  31x31x31                3.56              -                       0.00
  31x31                   4.97             3.76                     0.00
  48x48                   5.21             1.46                     0.00
  49x49                   5.24              -                       0.00
  63x63                   9.15              -                       0.00
  part_of_11x11x11        2.81              -                        -
  vc7_planes_13x12x11     3.45              -                        -
  vc7_records_13x12x11    8.56              -                        -
  cell_7x6x5               -               0.77                      -

The factor 64 was a guess; nothing measured needs a quarter of it.  info[1] and alpha equal R64 bit for bit on the integer data: the
device's f64 sqrt and division are correctly rounded, nothing had to be relaxed to 1 ulp.
"""
import ctypes as C
import os
import sys
from collections import namedtuple
from contextlib import contextmanager

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import coarse_cases as CC
import stencil_cases as S
from coarse_cases import CASES, CELL_CASE, GENEROUS, INFO3, RAW_CASES, RAW_ITERATIONS, REL_TOLS
from test_gpu_kernels import hip, hipd  # noqa: F401  (fixtures)

from exastencils_amd.layout import FieldLayout
from exastencils_amd.lib import ivec

pytestmark = pytest.mark.gpu

ROUTES = {-1: "refused", 0: "empty", 1: "global", 2: "lds"}          # enum CgRoute
BY_ID = dict(ids=lambda c: c.name)
CONSTANT = [c for c in CASES if not c.cfield]
INTEGER = [c for c in CONSTANT if c.stencil in CC.INTEGER_STENCILS]

Out = namedtuple("Out", "sol rhs res p ap info coef rc error")


def route(hipd, case, flags, L=None, box=None, mask=None):
    """The kernel examg_cg_coarse_variant takes for these arguments under the hook that is set; nothing is launched."""
    L = L or CC.layouts(case)
    b, e = box or CC.box(case)
    dummy = hipd.new_array(1) if case.cfield else None
    sc = CC.stencil(case, dummy, L.coef).c_struct(hipd.ptr)
    r = hipd.L.examg_debug_cg_route(C.byref(L.sol.c_struct()), C.byref(L.rhs.c_struct()), C.byref(L.res.c_struct()), C.byref(L.p.c_struct()),
                                    C.byref(L.ap.c_struct()), C.byref(sc), CC.face_mask(case) if mask is None else mask, ivec(b), ivec(e), int(flags))
    return ROUTES[r]


@contextmanager
def forced_global(hipd, on=True):
    hipd.L.examg_debug_cg(0 if on else 1)
    try:
        yield
    finally:
        hipd.L.examg_debug_cg(1)


def solve(ops, case, inp, flags, max_it, rel_tol, L=None, box=None, mask=None, with_info=True, prepare=None):
    """One call of examg_cg_coarse_variant of the library behind `ops` on device copies of the host arrays `inp`; returns every
    array as it is afterwards, the return code and the library's error text.  prepare(ops, L, device arrays): work on the device
    before the call."""
    L = L or CC.layouts(case)
    b, e = box or CC.box(case)
    t = {k: ops.from_host(np.array(inp[k], dtype=np.float64, copy=True)) for k in CC.ARRAYS + ("info",)}
    coef = ops.from_host(inp["coef"].copy()) if inp.get("coef") is not None else None
    sc = CC.stencil(case, coef, L.coef).c_struct(ops.ptr)
    geom = CC.geometry(case)
    if prepare is not None:
        prepare(ops, L, t)
    rc = ops.L.examg_cg_coarse_variant(C.byref(L.sol.c_struct()), ops.ptr(t["sol"]), C.byref(L.rhs.c_struct()), ops.ptr(t["rhs"]),
                                       C.byref(L.res.c_struct()), ops.ptr(t["res"]), C.byref(L.p.c_struct()), ops.ptr(t["p"]),
                                       C.byref(L.ap.c_struct()), ops.ptr(t["ap"]), C.byref(sc), C.byref(geom),
                                       CC.face_mask(case) if mask is None else mask, int(max_it), float(rel_tol), ivec(b), ivec(e), int(flags),
                                       ops.ptr(t["info"]) if with_info else None, ops._stream())
    error = ops.L.examg_last_error().decode() if rc else ""
    ops.synchronize()
    host = {k: np.array(ops.to_host(t[k]), copy=True) for k in t}
    return Out(host["sol"], host["rhs"], host["res"], host["p"], host["ap"], host["info"],
               np.array(ops.to_host(coef), copy=True) if coef is not None else None, rc, error)


def assert_same_bits(got, want, what, names=CC.ARRAYS + ("info",)):
    assert got.rc == 0 and want.rc == 0, (what, got.error, want.error)
    for name in names:
        g, w = getattr(got, name), getattr(want, name)
        if not np.array_equal(g, w):
            d = np.abs(g - w)
            raise AssertionError("%s: %s differs in %d of %d values, max abs %.3e" % (what, name, int((d > 0).sum()), d.size, np.nanmax(d)))


def assert_inputs_untouched(got, inp, what, names=CC.ARRAYS + ("info",)):
    for name in names:
        assert np.array_equal(getattr(got, name), inp[name]), "%s: %s was written" % (what, name)
    if inp.get("coef") is not None:
        assert np.array_equal(got.coef, inp["coef"]), "%s: the coefficients were written" % what


def assert_matches_reference(got, r64, rld, case, inp, what, exact=(), noise=()):
    """The comparison with R64 (see the module docstring); `exact`: outputs that must equal R64 bit for bit; `noise`: outputs that
    are rounding noise (CC.noise_outputs).  Returns the largest |GPU - R64| / max(delta_ref, eps * max |field|) of the outputs
    compared within the tolerance, and prints it per output."""
    assert got.rc == 0, (what, got.error)
    L, (b, e) = CC.layouts(case), CC.box(case)
    assert got.info[0] == r64.info[0] and got.info[3] == r64.info[3], (what, got.info, r64.info)
    assert_inputs_untouched(got, inp, what, ("rhs",))
    worst, figures = 0.0, []
    for name in CC.OUTPUTS + (("info", 1), ("info", 2)):
        if isinstance(name, tuple):
            g, w = got.info[name[1]], r64.info[name[1]]
            d = abs(g - w)
        else:
            g, w = getattr(got, name), getattr(r64, name)
            outside = ~S.box_mask(getattr(L, name), b, e)
            assert np.array_equal(g[outside], w[outside]), "%s: %s outside the box" % (what, name)
            d = float(np.max(np.abs(g - w)))
        if name in exact:
            assert np.array_equal(g, w), "%s: %s is not the exact value (max abs %.3e)" % (what, name, d)
            continue
        u = CC.unit(case, r64, rld, name)            # 0.0: the output is 0.0 in both precisions, and d must be
        ratio = d / u if u else (0.0 if d == 0.0 else np.inf)
        figures.append("%s %.2f" % (name if isinstance(name, str) else "info%d" % name[1], ratio))
        worst = max(worst, ratio)
        assert d <= CC.tolerance(case, r64, rld, name, noise), \
            "%s: %s is %.1f units from R64 (allowed 64, and 1e-10 of the field in the box)" % (what, name, ratio)
    print("UNITS %s: %s" % (what, ", ".join(figures)))
    return worst


def forms_of(hipd, hip, case, flags):
    """(name, ops, forced global) of the runs of one call: the product library, the debug build as it routes, and -- where that is
    the LDS form -- the debug build with the global-memory form forced."""
    runs = [("product", hip, False), ("debug", hipd, False)]
    if route(hipd, case, flags) == "lds":
        runs.append(("debug, global forced", hipd, True))
    return runs


# -- route ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + [CELL_CASE], **BY_ID)
def test_route_is_the_table_s(hipd, case):
    for flags in CC.case_flags(case):
        assert route(hipd, case, flags) == CC.expected_form(case, flags), flags
        with forced_global(hipd):
            assert route(hipd, case, flags) == "global", flags
    assert route(hipd, case, 0) == case.form
    b, e = CC.box(case)
    assert route(hipd, case, 0, box=(b, b)) == "empty"


# -- random data against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, **BY_ID)
def test_random_data_against_the_reference(hip, hipd, case):
    worst = 0.0
    for flags in CC.case_flags(case):
        assert route(hipd, case, flags) == case.form
        for rel_tol in REL_TOLS:
            inp = CC.case_inputs(case, flags=flags)
            r64, rld = (CC.reference(case, p, flags, GENEROUS, rel_tol) for p in ("R64", "RLD"))
            first = None
            for name, ops, glob in forms_of(hipd, hip, case, flags):
                what = "%s flags %d rel_tol %g (%s)" % (case.name, flags, rel_tol, name)
                with forced_global(hipd, glob):
                    got = solve(ops, case, inp, flags, GENEROUS, rel_tol)
                if first is None:
                    first = got
                    worst = max(worst, assert_matches_reference(got, r64, rld, case, inp, what, noise=CC.noise_outputs(case, rel_tol, r64)))
                else:
                    assert_same_bits(got, first, what + " against the product library")
                assert_inputs_untouched(got, inp, what, ("rhs",))
    print("MARGIN %s %.2f" % (case.name, worst))


@pytest.mark.parametrize("case", RAW_CASES, **BY_ID)
def test_fixed_iterations_from_raw_data(hip, hipd, case):
    """Three iterations from nothing but random data: non-zero planes and ghost points around the box, which the mat-vec of the
    search direction reads wherever `apply bc` does not zero them -- EXAMG_CG_NO_BC (the LDS form loads its halo from memory), and
    the cell layout under `apply bc`, which has no plane to zero and must take the global-memory form."""
    inp = CC.case_inputs(case)
    worst = 0.0
    for flags in (0, CC.CG_ALPHA_FROM_NORM | CC.CG_NO_BC):
        assert route(hipd, case, flags) == ("global" if case.cell and flags == 0 else "lds")
        r64, rld = (CC.reference(case, p, flags, RAW_ITERATIONS, 1e-8, raw=True) for p in ("R64", "RLD"))
        first = None
        for name, ops, glob in forms_of(hipd, hip, case, flags):
            what = "%s flags %d (%s)" % (case.name, flags, name)
            with forced_global(hipd, glob):
                got = solve(ops, case, inp, flags, RAW_ITERATIONS, 1e-8)
            if first is None:
                first = got
                worst = max(worst, assert_matches_reference(got, r64, rld, case, inp, what))
            else:
                assert_same_bits(got, first, what + " against the product library")
    print("MARGIN raw:%s %.2f" % (case.name, worst))


# -- equality that no summation order can break --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CC.BY_NAME[n] for n in ("16x16x16", "17x16x15", "16x16x17", "48x48", "vc7_records_13x12x11")], **BY_ID)
def test_two_runs_give_the_same_bits(hipd, case):
    for flags in (0, CC.CG_ALPHA_FROM_NORM | CC.CG_NO_BC):
        inp = CC.case_inputs(case, flags=flags)
        a, b = (solve(hipd, case, inp, flags, GENEROUS, 1e-8) for _ in range(2))
        assert_same_bits(a, b, "%s flags %d, second run" % (case.name, flags))
        assert a.info[0] >= 1


@pytest.mark.parametrize("case", CONSTANT, **BY_ID)
def test_zero_start_equals_set_then_solve(hipd, case):
    """EXAMG_CG_ZERO_START against examg_set(sol, 0) on the box + the solver without the flag, from the state include/examg.h
    names: Solution's planes around the box hold 0, its points in the box hold anything.  Every array and info, in both forms."""
    L, (b, e) = CC.layouts(case), CC.box(case)

    def zero_box(ops, L, t):
        ops.set(L.sol.c_struct(), t["sol"], 0.0, b, e)

    for base in (0, CC.CG_ALPHA_FROM_NORM | CC.CG_NO_BC):
        inp = CC.case_inputs(case, flags=base | CC.CG_ZERO_START)
        assert np.any(S.box_values(L.sol, inp["sol"], b, e))
        for glob in ((False, True) if case.form == "lds" else (False,)):
            with forced_global(hipd, glob):
                flagged = solve(hipd, case, inp, base | CC.CG_ZERO_START, GENEROUS, 1e-8)
                plain = solve(hipd, case, inp, base, GENEROUS, 1e-8, prepare=zero_box)
            assert_same_bits(flagged, plain, "%s flags %d, global forced %s" % (case.name, base, glob))
            assert flagged.info[0] >= 1


@pytest.mark.parametrize("case", INTEGER, **BY_ID)
def test_exact_data_is_bit_for_bit(hip, hipd, case):
    """Integer fields in [-8, 8] over the whole allocations with the integer stencils: every partial sum of r^2 and of p * Ap is an
    integer below 2^53 (tests/test_coarse_exact.py), so the sums are exact in any order, and with a correctly rounded sqrt and
    division so are info[1] and alpha.  max_it = 0: everything equals R64; max_it = 1: sol, res, ap, info[0], info[1] and info[3]
    equal R64 bit for bit, p and info[2] (from the sum of the squares of the new, no longer integer residual) within the tolerance.
    Both forms, the product library, both alpha rules, with and without `apply bc` (without: non-zero integers in the halo)."""
    inp = CC.case_inputs(case, "exact")
    worst = 0.0
    for flags in (0, CC.CG_ALPHA_FROM_NORM, CC.CG_ALPHA_FROM_NORM | CC.CG_NO_BC):
        for max_it in (0, 1):
            r64, rld = (CC.reference(case, p, flags, max_it, 1e-3, "exact", raw=True) for p in ("R64", "RLD"))
            exact = CC.OUTPUTS + (("info", 1), ("info", 2)) if max_it == 0 else ("sol", "res", "ap", ("info", 1))
            for name, ops, glob in forms_of(hipd, hip, case, flags):
                what = "%s flags %d max_it %d (%s)" % (case.name, flags, max_it, name)
                with forced_global(hipd, glob):
                    got = solve(ops, case, inp, flags, max_it, 1e-3)
                worst = max(worst, assert_matches_reference(got, r64, rld, case, inp, what, exact))
                if max_it == 0:
                    assert_inputs_untouched(got, inp, what, ("ap",))
    print("MARGIN exact:%s %.2f" % (case.name, worst))


# -- limits and refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CC.BY_NAME[n] for n in ("16x16x16", "16x16x17", "31x31", "vc7_planes_13x12x11")], **BY_ID)
def test_iteration_limits(hip, hipd, case):
    """info[3] counts the solves whose loop ran out: at max_it 0, 1 and 2 it is incremented, at a generous limit it is not.  With
    max_it = 0 the solver computes the residual, its norm and the first search direction and leaves ap alone, in both forms."""
    inp = CC.case_inputs(case, flags=0)
    for max_it in (0, 1, 2, GENEROUS):
        r64, rld = (CC.reference(case, p, 0, max_it, 1e-3) for p in ("R64", "RLD"))
        assert r64.info[3] == (INFO3 if max_it == GENEROUS else INFO3 + 1) and r64.info[0] == min(max_it, r64.info[0])
        first = None
        for name, ops, glob in forms_of(hipd, hip, case, 0):
            what = "%s max_it %d (%s)" % (case.name, max_it, name)
            with forced_global(hipd, glob):
                got = solve(ops, case, inp, 0, max_it, 1e-3)
            assert_matches_reference(got, r64, rld, case, inp, what)
            if max_it == 0:
                assert_inputs_untouched(got, inp, what, ("ap",))
                assert got.info[0] == 0 and got.info[2] == got.info[1]
            if first is not None:
                assert_same_bits(got, first, what)
            first = got


@pytest.mark.parametrize("case", [CC.BY_NAME[n] for n in ("15x15x15", "16x16x17")], **BY_ID)
def test_info_may_be_null(hip, hipd, case):
    inp = CC.case_inputs(case, flags=0)
    for name, ops, glob in forms_of(hipd, hip, case, 0):
        with forced_global(hipd, glob):
            with_info = solve(ops, case, inp, 0, GENEROUS, 1e-3)
            without = solve(ops, case, inp, 0, GENEROUS, 1e-3, with_info=False)
        assert_same_bits(without, with_info, "%s without info (%s)" % (case.name, name), CC.ARRAYS)
        assert np.array_equal(without.info, inp["info"])


@pytest.mark.parametrize("case", [CC.BY_NAME[n] for n in ("15x15x15", "48x48", "vc7_planes_13x12x11")], **BY_ID)
def test_empty_box_is_a_solve_of_nothing(hip, hipd, case):
    inp = CC.case_inputs(case)
    b, e = CC.box(case)
    for empty in ((b, b), (b, [e[0], b[1], e[2]])):
        assert route(hipd, case, 0, box=empty) == "empty"
        for ops in (hip, hipd):
            got = solve(ops, case, inp, 0, GENEROUS, 1e-3, box=empty)
            assert got.rc == 0, got.error
            assert_inputs_untouched(got, inp, "%s, empty box" % case.name, CC.ARRAYS)
            assert list(got.info) == [0.0, 0.0, 0.0, INFO3]


def _refusals():
    small, vc = CC.BY_NAME["3x3x3"], CC.BY_NAME["vc7_planes_13x12x11"]
    L = CC.layouts(small)
    b, e = CC.box(small)
    cells = tuple(v + 1 for v in small.n)
    return [
        ("unknown flag", small, dict(flags=8), "unknown flag"),
        ("colour-split layout", small, dict(L=L._replace(sol=L.sol.split_x(), p=L.p.split_x())), "layout transformation"),
        ("colour-split residual", small, dict(L=L._replace(res=L.res.split_x())), "layout transformation"),
        ("incomplete face mask", small, dict(mask=63 & ~4), "every face"),
        ("zero start with a coefficient field", vc, dict(flags=CC.CG_ZERO_START), "constant coefficients"),
        # 2^22 + 2^16 points in arrays of a few hundred: refused by the arguments alone, before anything is launched
        ("box of more than 2^22 points", small, dict(box=([1, 1, 1], [257, 257, 66])), "too large"),
        ("box leaving Solution's allocation", small, dict(box=(b, [e[0] + 4, e[1], e[2]])), "leaves an allocation"),
        ("box leaving the right-hand side's allocation", small, dict(box=([b[0] - 2, b[1], b[2]], e)), "leaves an allocation"),
        ("box leaving the coefficient field's layout", vc, dict(L=CC.layouts(vc)._replace(coef=FieldLayout.node(3, (8, 8, 8), 1, align=2))), "leaves an allocation"),
        ("strides of Solution and the search direction disagree", small, dict(L=L._replace(p=FieldLayout.node(3, cells, 1, align=16))), "must agree"),
    ]


@pytest.mark.parametrize("what,case,change,message", _refusals(), ids=[r[0].replace(" ", "_") for r in _refusals()])
def test_refusals_leave_every_array_alone(hip, hipd, what, case, change, message):
    inp = CC.case_inputs(case)
    flags = change.get("flags", 0)
    kw = {k: v for k, v in change.items() if k != "flags"}
    assert route(hipd, case, flags, **kw) == "refused"
    for ops in (hip, hipd):
        got = solve(ops, case, inp, flags, GENEROUS, 1e-3, **kw)
        assert got.rc != 0 and message in got.error, (what, got.rc, got.error)
        assert_inputs_untouched(got, inp, what)
    # the library still works after a refusal
    ok = solve(hip, case, CC.case_inputs(case, flags=0), 0, GENEROUS, 1e-3)
    assert ok.rc == 0 and ok.info[0] >= 1
