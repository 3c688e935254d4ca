"""The reference of the one-kernel coarse CG (tests/coarse_cases.py) on its own, without a GPU: the conditions the GPU comparison of
tests/test_gpu_coarse.py rests on.  For every case, flag set and tolerance the two precisions of the reference (R64: float64 with
correctly rounded sums; RLD: long double throughout) must take the same number of iterations, no exit test may come within 1e-6 of
its threshold (rounding can then not flip it, on the device either), the two must agree to 1e-11 of every output's maximum over
the box -- the four arrays, info[1] and info[2]; only the residual and info[2] of the solves that end by exact termination
(coarse_cases.EXACT_TERMINATION) are exempt, and must be rounding noise -- and R64 must agree with the oracle's loops -- the
reference the project already trusts -- within the tolerance the GPU tests use."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import coarse_cases as CC
import stencil_cases as S
from coarse_cases import CASES, CELL_CASE, GENEROUS, RAW_CASES, RAW_ITERATIONS, REL_TOLS

ALL = CASES + [CELL_CASE]
IDS = [c.name for c in ALL]


def combos(case):
    return [(f, t) for f in CC.case_flags(case) for t in REL_TOLS]


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_routing_table_follows_the_rule(case):
    """The form the table names for each case is what the routing rule gives (with `apply bc`; the cell case is the one whose form
    depends on the flag), and the boxes sit where the table says: on either side of each bound."""
    assert CC.expected_form(case, 0) == case.form
    assert CC.expected_form(case, CC.CG_NO_BC) == ("lds" if case.cell else case.form)
    L = CC.layouts(case)
    assert L.sol == L.p and len({L.sol, L.rhs, L.res, L.ap}) == 4           # every argument in its own layout
    assert L.rhs.ghost == (0, 0, 0) and L.ap.ghost == (0, 0, 0) and L.res.ghost[0] == 2


def test_bounds_are_met_from_both_sides():
    n = {c.name: c.n for c in CASES}
    pts = lambda v: v[0] * v[1] * v[2]
    lds = lambda v: (v[0] + 2) * (v[1] + 2) * (v[2] + 2) * 8
    assert pts(n["16x16x16"]) == CC.LDS_POINTS and pts(n["17x16x15"]) < CC.LDS_POINTS < pts(n["16x16x17"])
    assert lds(n["16x16x17"]) <= CC.LDS_BYTES                                  # fails the point bound only
    assert lds(n["200x4x4"]) <= CC.LDS_BYTES < lds(n["220x4x4"]) and pts(n["220x4x4"]) <= CC.LDS_POINTS
    assert lds(n["48x48"]) <= CC.LDS_BYTES < lds(n["49x49"])


@pytest.mark.parametrize("name", sorted(CC.STENCILS))
def test_stencils_are_symmetric_definite_and_anisotropic(name):
    orders = {"s7": S.ORDERS7, "s5": S.ORDERS5, "s27": S.ORDERS27, "lap": ("mp", "pm", "perm")}[name]
    used = {c.order for c in CASES if c.stencil == name}
    assert len(used) >= 2 and any("perm" in o for o in used) and used <= set(orders)
    for order in orders:
        st = CC.STENCILS[name](order)
        c = dict(zip(st.offsets, st.coefs))
        assert len(c) == len(st.offsets)
        assert all(c[o] == c[tuple(-v for v in o)] for o in c)                                   # symmetric
        assert c[(0, 0, 0)] >= sum(abs(v) for o, v in c.items() if any(o)) and all(v < 0 for o, v in c.items() if any(o))
        axes = [c[o] for o in ((1, 0, 0), (0, 1, 0), (0, 0, 1)) if o in c]
        assert len(set(axes)) == len(axes)                                                       # x, y, z distinguishable
    if name in CC.INTEGER_STENCILS:
        assert all(float(v).is_integer() for v in CC.STENCILS[name](sorted(used)[0]).coefs)


@pytest.mark.parametrize("case", CASES, ids=IDS[:-1])
def test_the_two_precisions_agree_and_no_exit_is_close(case):
    worst = 0.0
    for flags, rel_tol in combos(case):
        r64 = CC.reference(case, "R64", flags, GENEROUS, rel_tol)
        rld = CC.reference(case, "RLD", flags, GENEROUS, rel_tol)
        what = (case.name, flags, rel_tol)
        assert r64.info[0] == rld.info[0] and 1 <= r64.info[0] < GENEROUS, what
        assert r64.info[3] == CC.INFO3 and rld.info[3] == CC.INFO3, what
        assert len(rld.ratios) == int(rld.info[0]) and min(abs(r - 1.0) for r in rld.ratios + r64.ratios) >= 1e-6, what
        # every output; only a solve that ends by exact termination (CC.EXACT_TERMINATION, by name) leaves a residual and a final
        # norm that are rounding noise: there they must be just that, below one rounding of the initial residual
        noise = CC.noise_outputs(case, rel_tol, r64)
        assert bool(noise) == ((case.name, rel_tol) in CC.EXACT_TERMINATION), what
        for name in CC.OUTPUTS + (("info", 1), ("info", 2)):
            d, s = CC.delta_ref(r64, rld, name), CC.scale_of(case, r64, name)
            if name in noise:
                assert max(s, d) <= CC.EPS * r64.info[1] / 64, (what, name, s, d)
                continue
            assert d <= 1e-11 * s, (what, name, d, s)
            worst = max(worst, d / s if s else 0.0)
        # what the solver must not touch: rhs, and everything outside the box and the `apply bc` planes
        inp = CC.case_inputs(case, flags=flags)
        L, (b, e) = CC.layouts(case), CC.box(case)
        assert np.array_equal(r64.rhs, inp["rhs"])
        for name in ("sol", "res", "p", "ap"):
            l = getattr(L, name)
            keep = ~S.box_mask(l, b, e)
            if name != "ap" and not flags & CC.CG_NO_BC:
                faces = CC.face_mask_of(l, case.nd)
                assert not np.any(getattr(r64, name)[faces]), (what, name)
                keep &= ~faces
            assert np.array_equal(getattr(r64, name)[keep], inp[name][keep]), (what, name)
    print("%s: delta_ref <= %.2e of the field maximum" % (case.name, worst))


@pytest.fixture(scope="module")
def orc():
    from oracle_ops import OracleOps

    return OracleOps()


@pytest.mark.parametrize("case", CASES, ids=IDS[:-1])
def test_r64_agrees_with_the_oracle_loops(case, orc):
    """The oracle's loops sum their dots in their own order; its stencil fields are in the planes order."""
    L, (b, e) = CC.layouts(case), CC.box(case)
    for flags, rel_tol in combos(case):
        inp = CC.case_inputs(case, flags=flags)
        r64 = CC.reference(case, "R64", flags, GENEROUS, rel_tol)
        rld = CC.reference(case, "RLD", flags, GENEROUS, rel_tol)
        t = {k: orc.from_host(inp[k].copy()) for k in CC.ARRAYS + ("info",)}
        coef = inp["coef"]
        if case.cfield == "records":
            coef = np.ascontiguousarray(coef.reshape(L.coef.size, 7).T).reshape(-1)
        st = CC.stencil(case, orc.from_host(coef.copy()) if coef is not None else None)
        st.ctransform = 0
        orc.cg_coarse(L.sol.c_struct(), t["sol"], L.rhs.c_struct(), t["rhs"], L.res.c_struct(), t["res"], L.p.c_struct(), t["p"],
                      L.ap.c_struct(), t["ap"], st, CC.geometry(case), CC.face_mask(case), GENEROUS, rel_tol, b, e, t["info"], flags=flags)
        what = (case.name, flags, rel_tol)
        assert float(t["info"][0]) == r64.info[0] and float(t["info"][3]) == CC.INFO3, what
        for name in CC.OUTPUTS:
            d = float(np.max(np.abs(orc.to_host(t[name]) - getattr(r64, name))))
            u = CC.unit(case, r64, rld, name)
            assert d <= CC.tolerance(case, r64, rld, name, CC.noise_outputs(case, rel_tol, r64)), (what, name, d / u if u else d)
        assert np.array_equal(orc.to_host(t["rhs"]), inp["rhs"])


@pytest.mark.parametrize("case", [c for c in CASES if c.stencil in CC.INTEGER_STENCILS], ids=lambda c: c.name)
def test_exact_data_has_exact_sums(case):
    """Integer fields in [-8, 8] with the integer stencils: the first residual, the first search direction and A p are integers,
    and the sums of r^2 and p * Ap stay below 2^53 in magnitude term by term -- no summation order can change them.  The data is
    random integers around the box too: without `apply bc` the halo of the search direction holds non-zero integers."""
    inp = CC.case_inputs(case, "exact")
    L, (b, e) = CC.layouts(case), CC.box(case)
    for flags in (0, CC.CG_ALPHA_FROM_NORM, CC.CG_ALPHA_FROM_NORM | CC.CG_NO_BC):
        r0 = CC.reference(case, "R64", flags, 0, 1e-3, "exact", raw=True)
        r1 = CC.reference(case, "R64", flags, 1, 1e-3, "exact", raw=True)
        r = S.box_values(L.res, r0.res, b, e)
        p, q = S.box_values(L.p, r0.p, b, e), S.box_values(L.ap, r1.ap, b, e)
        for v in (r, p, q):
            assert np.array_equal(v, np.round(v))
        assert np.array_equal(r, p) and float(np.sum(r * r)) < 2.0 ** 53 and float(np.sum(np.abs(p * q))) < 2.0 ** 53
        assert r0.info[1] == np.sqrt(np.sum(r * r)) and r0.info[0] == 0 and r0.info[3] == CC.INFO3 + 1
        assert np.array_equal(r0.ap, inp["ap"])                                # no iteration: cgTmp1 is not written
        ld = CC.reference(case, "RLD", flags, 1, 1e-3, "exact", raw=True)
        assert r1.info[1] == float(ld.info[1]) and r1.info[0] == 1


@pytest.mark.parametrize("case", RAW_CASES, ids=lambda c: c.name)
def test_fixed_iteration_runs_from_raw_data(case, orc):
    """Three iterations from nothing but random data -- non-zero planes and ghost points around the box, which the mat-vec of the
    search direction reads wherever `apply bc` does not zero them (EXAMG_CG_NO_BC; the cell layout, which has no plane to zero).
    No convergence is asked of such a run: the loop must end at the limit in both precisions, far from the exit test, and R64 must
    agree with the oracle's loops, which read those points from memory."""
    L, (b, e) = CC.layouts(case), CC.box(case)
    inp = CC.case_inputs(case)
    for flags in (0, CC.CG_ALPHA_FROM_NORM | CC.CG_NO_BC):
        r64 = CC.reference(case, "R64", flags, RAW_ITERATIONS, 1e-8, raw=True)
        rld = CC.reference(case, "RLD", flags, RAW_ITERATIONS, 1e-8, raw=True)
        assert r64.info[0] == rld.info[0] == RAW_ITERATIONS and r64.info[3] == rld.info[3] == CC.INFO3 + 1
        assert min(r64.ratios + rld.ratios) > 1.0 + 1e-6
        t = {k: orc.from_host(inp[k].copy()) for k in CC.ARRAYS + ("info",)}
        orc.cg_coarse(L.sol.c_struct(), t["sol"], L.rhs.c_struct(), t["rhs"], L.res.c_struct(), t["res"], L.p.c_struct(), t["p"],
                      L.ap.c_struct(), t["ap"], CC.stencil(case), CC.geometry(case), CC.face_mask(case), RAW_ITERATIONS, 1e-8, b, e,
                      t["info"], flags=flags)
        assert float(t["info"][0]) == RAW_ITERATIONS and float(t["info"][3]) == CC.INFO3 + 1
        for name in CC.OUTPUTS:
            assert CC.delta_ref(r64, rld, name) <= 1e-11 * CC.scale_of(case, r64, name)
            d = float(np.max(np.abs(orc.to_host(t[name]) - getattr(r64, name))))
            assert d <= CC.tolerance(case, r64, rld, name), (case.name, flags, name, d / CC.unit(case, r64, rld, name))
        if case.cell and flags == 0:
            # the ghost cells matter: with zeros there (what a zero halo amounts to) the answer is another one
            zeroed = dict(inp)
            zeroed["p"] = inp["p"].copy()
            zeroed["p"][S.shell_mask(L.p, b, e)] = 0.0
            other = CC.cg_reference("R64", L, case.nd, zeroed, CC.stencil(case), None, False, flags, RAW_ITERATIONS, 1e-8, b, e)
            assert float(np.max(np.abs(other.ap - r64.ap))) > 1e-3
