"""The semilinear kernels (examg_nl_op, examg_nl_smooth) on the MI355X against the numpy restatement (tests/nonlinear_ops.py), and the FAS
programs on the HIP kernel layer.

  exact class   programs of + - * / and constants on random (not dyadic) data: every operation is one IEEE rounding, so the device must
                give the restatement's bits -- all three modes of nl_op, Jacobi and both colours, asymmetric stencils with 5 / 9 (2-D)
                and 7 / 27 (3-D) distinct entries and the centre first, in the middle and last, every argument in a layout of its own,
                q the same array as u and another one, boxes with rows below, at and over a wave and odd begins.  The whole output array
                is compared (sentinels outside the box), and every input with its copy.
  libm class    c = gamma exp(u), d = (gamma (1 + u)) exp(u): the device's exp is within blas_cases.LIBM_ULP["exp"] ulps of the correctly
                rounded value (mpmath) on [0.25, 2]; that bound is carried through the remaining operations of the statement per point
                (derivation at _libm_bound), one ulp added per rounded operation downstream.  The largest observed / allowed ratio is printed.
  refusals      an error, and nothing is written.
  programs      bratu2d_fas prints the lines of the reference's results file; both examples follow the restatement's residual history
                within 1e-10 relative per iterate under the rule of tests/test_gpu_solver.py:25 (the data pass through the device's
                libm: 1e-13 of the starting residual is the perturbation converged iterates carry) and its error history under the rule
                of tests/test_gpu_solver.py:46-50; the FAS cycle replayed from a hipGraph equals its interpretation bit for bit
                (tests/graph_cases.py).

Measured on an MI355X: exact class equal in every case, star and gather kernel equal; libm class at most 0.68 of the derived allowance
(27-point apply; 5-point 0.52); residuals of bratu3d_rbgs_fas within 3.0e-12 absolute of the restatement's over a reduction from 2.1e3 to 1.6e-5 (relative 8.5e-8 at
the last iterate, 4.0e-10 at 1.9e-3: the floor of the rule, 2.1e-10 absolute, is what admits them); maximum errors within 5.5e-15."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import nonlinear_cases as N  # noqa: E402
import stencil_cases as S  # noqa: E402
from nonlinear_ops import NL_ADD, NL_APPLY, NL_RESIDUAL, NonlinearOracleOps  # noqa: E402
from system_ops import _fold  # noqa: E402

from exastencils_amd.layout import FieldLayout  # noqa: E402
from exastencils_amd.lib import NlExprC, ivec  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from exastencils_amd.ops import HipOps

    return HipOps(0)


@pytest.fixture(scope="module")
def orc():
    return NonlinearOracleOps()


def host(ops, t):
    ops.synchronize()
    return np.array(ops.to_host(t), dtype=np.float64, copy=True)


def same_bits(got, want, what):
    if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
        bad = got.view(np.uint64) != want.view(np.uint64)
        raise AssertionError("%s: %d of %d values differ, max abs %.3e" % (what, int(bad.sum()), bad.size, float(np.nanmax(np.abs(got - want)[bad]))))


def _run(ops, kind, data, lays, st, c, d, b, e, alias):
    """One call on kernel layer `ops` from the host arrays `data` = (u, q, f, dst); returns the host copies of (u, q, f, dst) afterwards.
    kind: an nl_op mode, 'jacobi' or ('colour', k).  alias: q is u."""
    lu, lq, lf, ld = [x.c_struct() for x in lays]
    u, q, f, dst = [ops.from_host(a.copy()) for a in data]
    if alias:
        lq, q = lu, u
    if kind in (NL_APPLY, NL_RESIDUAL, NL_ADD):
        ops.nl_op(kind, lu, u, lq, q, lf, f, ld, dst, st, c, b, e)
    elif kind == "jacobi":
        ops.nl_smooth(lu, u, ld, dst, lf, f, st, c, d, 0.713, -1, b, e)
    else:
        ops.nl_smooth(lu, u, lu, u, lf, f, st, c, d, 0.713, kind[1], b, e)
    return [host(ops, t) for t in (u, q, f, dst)]


# -- exact class -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nd,ext,begin", N.BOXES, ids=[x[0] for x in N.BOXES])
def test_exact_class_bit_for_bit(hip, orc, name, nd, ext, begin):
    shape, b, e = N.geometry(nd, ext, begin)
    lays = N.layouts(nd, shape)
    c, d = NlExprC.from_program(N.EXACT_C), NlExprC.from_program(N.EXACT_D)
    rng = np.random.default_rng(sum(ext) + 100 * nd)
    runs = 0
    for skind in ((5, 9) if nd == 2 else (7, 27)):
        for where in ("first", "middle", "last"):
            st = N.stencil(skind, where)
            u, q, f = [rng.uniform(-1.0, 1.0, int(l.size)) for l in lays[:3]]
            calls = [(m, alias) for m in (NL_APPLY, NL_RESIDUAL, NL_ADD) for alias in (False, True)] + [("jacobi", True)]
            if S.is_star(st):
                calls += [(("colour", 0), True), (("colour", 1), True)]
            for kind, alias in calls:
                # dst: sentinels where the call must write the box and nothing else; data where it adds to what is there
                dst = rng.uniform(-1.0, 1.0, int(lays[3].size)) if kind == NL_ADD else np.full(int(lays[3].size), N.SENTINEL)
                data = (u, q, f, dst)
                got = _run(hip, kind, data, lays, st, c, d, b, e, alias)
                want = _run(orc, kind, data, lays, st, c, d, b, e, alias)
                what = "%s stencil %d centre %s call %r alias %r" % (name, skind, where, kind, alias)
                for i, arr in enumerate("uqf"):
                    if not (arr == "u" and isinstance(kind, tuple)) and not (arr == "q" and alias):      # (q is u then)
                        same_bits(got[i], data[i], what + ": input " + arr + " was written")
                out = 0 if isinstance(kind, tuple) else 3
                same_bits(got[out], want[out], what)
                inside = S.box_mask(lays[0] if isinstance(kind, tuple) else lays[3], b, e)
                if kind != NL_ADD and not isinstance(kind, tuple):
                    assert np.all(got[3][~inside] == N.SENTINEL) and not np.any(got[3][inside] == N.SENTINEL), what
                if isinstance(kind, tuple):      # the other colour and everything outside the box keep their bits
                    i2, i1, i0 = np.meshgrid(*[np.arange(b[k], e[k]) for k in (2, 1, 0)], indexing="ij")
                    sel = np.zeros(inside.shape, dtype=bool)
                    sel[inside] = (((i0 + i1 + i2) % 2) == kind[1]).reshape(-1)
                    same_bits(got[0][~sel], u[~sel], what + ": points off the colour")
                    assert not np.any(got[0][sel] == u[sel]), what
                runs += 1
    assert runs == 2 * 3 * 7 + 3 * 2


def test_star_path_and_gather_path_give_the_same_bits(hip):
    """Star stencils of reach 1 take the row-marching kernel on all points; the debug build can send them to the gather kernel
    (examg_debug_nl_gather_only).  Both fold the entries in declared order: the same bits, with programs of either class, on rows
    below and over a wave, an odd number of rows (the last row group half empty) and in 3-D."""
    from exastencils_amd import lib
    from exastencils_amd.ops import HipOps

    hipd = HipOps(0, lib.DBG_LIB_PATH)
    progs = [(NlExprC.from_program(N.EXACT_C), NlExprC.from_program(N.EXACT_D)), (NlExprC.from_program(N.LIBM_C), NlExprC.from_program(N.LIBM_D))]
    for name, nd, ext, begin in [x for x in N.BOXES if x[0] in ("3x2", "65x5", "130x4", "7x5x3", "130x3x2")]:
        shape, b, e = N.geometry(nd, ext, begin)
        lays = N.layouts(nd, shape)
        rng = np.random.default_rng(5 + sum(ext))
        data = [rng.uniform(-1.0, 1.0, int(l.size)) for l in lays]
        for where in ("first", "last"):
            st = N.stencil(5 if nd == 2 else 7, where)
            for c, d in progs:
                for kind in (NL_APPLY, NL_RESIDUAL, NL_ADD, "jacobi"):
                    outs = []
                    for gather in (0, 1):
                        hipd.L.examg_debug_nl_gather_only(gather)
                        try:
                            outs.append(_run(hipd, kind, data, lays, st, c, d, b, e, kind == "jacobi")[3])
                        finally:
                            hipd.L.examg_debug_nl_gather_only(0)
                    same_bits(outs[0], outs[1], "%s centre %s call %r" % (name, where, kind))
                    assert not np.array_equal(outs[0], data[3])


# -- libm class ----------------------------------------------------------------------------------------------------------------------------
def _exp_correctly_rounded(x):
    import mpmath

    with mpmath.workdps(50):
        return np.array([float(mpmath.exp(mpmath.mpf(float(v)))) for v in x.reshape(-1)]).reshape(x.shape)


def _ulp(x):
    """One ulp of fp64 at x: the spacing of the doubles there."""
    return np.spacing(np.abs(x))


def _libm_bound(kind, lays, st, u, f, dst0, b, e, w):
    """(reference result on the box, allowed difference per point) with exp correctly rounded.  E = LIBM_ULP['exp'] ulps of exp(u) is
    the device's distance from it (measured on [0.25, 2], where u lies).  First-order propagation, one _ulp per rounded operation:
      cv = gamma * ex              err <= gamma E + ulp(cv)
      p  = cv * u                  err <= |u| err(cv) + ulp(p)
      n  = conv + p                err <= err(p) + ulp(n)                       (conv is exact-class: the same bits on both sides)
      residual f - n, add dst + n  err <= err(n) + ulp(result)
      smoother: dv = (gamma (1 + u)) * ex   err <= |gamma (1 + u)| E + ulp(dv);   den = diag + dv   err <= err(dv) + ulp(den)
                num = f - n                err <= err(n) + ulp(num)
                qt = num / den             err <= err(num) / |den| + |num| err(den) / den^2 + ulp(qt)        (the quotient rule)
                out = u + w * qt           err <= |w| err(qt) + ulp(w qt) + ulp(out)
    The terms of second order in 2^-52 are covered by the factor 1 + 2^-20 on the whole."""
    from blas_cases import LIBM_ULP
    from cell_ops import _sl, _view

    import torch

    lu, lq, lf, ld = lays
    ua, uref = _view(lu.c_struct(), torch.from_numpy(u))
    uc = ua[_sl(uref, b, e)]
    conv = _fold(st, ua, uref, b, e, False)
    ex = _exp_correctly_rounded(uc)
    E = LIBM_ULP["exp"][1] * np.spacing(ex)
    cv = N.GAMMA * ex
    e_cv = N.GAMMA * E + _ulp(cv)
    p = cv * uc
    e_p = np.abs(uc) * e_cv + _ulp(p)
    n = conv + p
    e_n = e_p + _ulp(n)
    fa, fref = _view(lf.c_struct(), torch.from_numpy(f))
    fv = fa[_sl(fref, b, e)]
    if kind == NL_APPLY:
        return n, e_n * (1.0 + 2.0 ** -20)
    if kind == NL_RESIDUAL:
        r = fv - n
        return r, (e_n + _ulp(r)) * (1.0 + 2.0 ** -20)
    if kind == NL_ADD:
        da, dref = _view(ld.c_struct(), torch.from_numpy(dst0))
        r = da[_sl(dref, b, e)] + n
        return r, (e_n + _ulp(r)) * (1.0 + 2.0 ** -20)
    g1 = N.GAMMA * (1.0 + uc)
    dv = g1 * ex
    e_dv = np.abs(g1) * E + _ulp(dv)
    den = float(st.coefs[st.diag_index]) + dv
    e_den = e_dv + _ulp(den)
    num = fv - n
    e_num = e_n + _ulp(num)
    qt = num / den
    e_qt = e_num / np.abs(den) + np.abs(num) * e_den / (den * den) + _ulp(qt)
    out = uc + w * qt
    e_out = abs(w) * e_qt + _ulp(w * qt) + _ulp(out)
    return out, e_out * (1.0 + 2.0 ** -20)


@pytest.mark.parametrize("name,nd,ext,begin,skind", [("65x5", 2, (65, 5, 1), (3, 1, 0), 5), ("7x5x3", 3, (7, 5, 3), (1, 1, 1), 7), ("9x4x3", 3, (9, 4, 3), (2, 1, 1), 27)],
                         ids=["65x5-5pt", "7x5x3-7pt", "9x4x3-27pt"])
def test_libm_class_within_the_derived_bound(hip, name, nd, ext, begin, skind):
    shape, b, e = N.geometry(nd, ext, begin)
    lays = N.layouts(nd, shape)
    st = N.stencil(skind, "middle")
    c, d = NlExprC.from_program(N.LIBM_C), NlExprC.from_program(N.LIBM_D)
    rng = np.random.default_rng(7 + skind)
    u = rng.uniform(0.25, 2.0, int(lays[0].size))       # the range blas_cases.LIBM_ULP was measured on
    q = rng.uniform(-1.0, 1.0, int(lays[1].size))
    f, dst0 = rng.uniform(-1.0, 1.0, int(lays[2].size)), rng.uniform(-1.0, 1.0, int(lays[3].size))
    kinds = [NL_APPLY, NL_RESIDUAL, NL_ADD, "jacobi"] + ([("colour", 1)] if S.is_star(st) else [])
    worst = 0.0
    for kind in kinds:
        got = _run(hip, kind, (u, q, f, dst0), lays, st, c, d, b, e, True)
        want, allowed = _libm_bound(kind, lays, st, u, f, dst0, b, e, 0.713)
        lay_out = lays[0] if isinstance(kind, tuple) else lays[3]
        g = got[0 if isinstance(kind, tuple) else 3][S.box_mask(lay_out, b, e)].reshape(want.shape)
        diff = np.abs(g - want)
        if isinstance(kind, tuple):
            i2, i1, i0 = np.meshgrid(*[np.arange(b[k], e[k]) for k in (2, 1, 0)], indexing="ij")
            sel = ((i0 + i1 + i2) % 2) == kind[1]
            same_bits(g[~sel], u[S.box_mask(lays[0], b, e)].reshape(want.shape)[~sel], "points off the colour")
            diff, allowed = diff[sel], allowed[sel]
        ratio = float(np.max(diff / allowed))
        print("libm class %s call %r: largest observed / allowed = %.3f (largest difference %.3e)" % (name, kind, ratio, float(diff.max())))
        worst = max(worst, ratio)
        assert ratio <= 1.0
    print("libm class %s: worst ratio %.3f" % (name, worst))


# -- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_an_error_and_write_nothing(hip):
    from exastencils_amd.field import Stencil

    base = FieldLayout.node(2, (6, 5), 1)
    cell = FieldLayout.cell(2, (6, 5), 1)
    u, q, f, dst = [hip.from_host(np.full(int(base.size) * 2, N.SENTINEL)) for _ in range(4)]
    good = N.stencil(5, "first")
    sf = Stencil([(0, 0, 0), (1, 0, 0)], [], u, base, 0, 0)

    def raw(ops, n=None):
        p = NlExprC()
        p.n = len(ops) if n is None else n
        for i, o in enumerate(ops):
            p.op[i] = o
        return p

    ok_c, ok_d = NlExprC.from_program(N.EXACT_C), NlExprC.from_program(N.EXACT_D)
    b, e = ivec((1, 1, 0)), ivec((5, 4, 1))
    cases = [
        ("stencil field", dict(st=sf)), ("colour-split", dict(lu=base.split_x())), ("cell layout", dict(ld=cell)), ("33 instructions", dict(c=raw([22], 33))),
        ("reads the node position", dict(c=raw([1]))), ("deeper than 8", dict(c=raw([22] * 9 + [4] * 8))), ("unknown opcode", dict(d=raw([40]))),
        ("leaves the u allocation", dict(b=(-1, 1, 0))), ("leaves the u allocation", dict(e=(8, 4, 1))),      # one point past the ghost layer
    ]
    for text, kw in cases:
        st = kw.get("st", good).c_struct(hip.ptr)
        lu, ld = kw.get("lu", base).c_struct(), kw.get("ld", base).c_struct()
        l = base.c_struct()
        cc, dd = kw.get("c", ok_c), kw.get("d", ok_d)
        b, e = ivec(kw.get("b", (1, 1, 0))), ivec(kw.get("e", (5, 4, 1)))
        rcs = []
        if "d" not in kw:
            rcs.append(hip.L.examg_nl_op(NL_RESIDUAL, C.byref(lu), hip.ptr(u), C.byref(l), hip.ptr(q), C.byref(l), hip.ptr(f), C.byref(ld), hip.ptr(dst),
                                         C.byref(st), C.byref(cc), b, e, hip._stream()))
            assert text in hip.L.examg_last_error().decode()
        rcs.append(hip.L.examg_nl_smooth(C.byref(lu), hip.ptr(u), C.byref(ld), hip.ptr(dst), C.byref(l), hip.ptr(f), C.byref(st), C.byref(cc), C.byref(dd),
                                         0.8, -1, b, e, hip._stream()))
        assert text in hip.L.examg_last_error().decode()
        assert all(rc != 0 for rc in rcs), text
    for t in (u, q, f, dst):
        assert np.all(host(hip, t) == N.SENTINEL)


def test_interpreter_refuses_colour_split_fields(hip):
    """On the HIP layer the `LayoutTransformations` directive is applied (the CPU stand-in records it only): the smoother on a
    colour-split field is refused by name."""
    from exastencils_amd import exa4
    from exastencils_amd.exa4_parser import Exa4Unsupported

    split = "LayoutTransformations {\n  transform u@finest with [x, y, z] => [x / 2, y, z, x % 2]\n}\n\n"
    with pytest.raises(Exa4Unsupported, match="colour-split field u"):
        exa4.Exa4Program(split + N.text("bratu3d_rbgs_fas.exa4"), dict(N.K_BRATU3D, maxLevel=3), ops=hip).run()


# -- whole programs ------------------------------------------------------------------------------------------------------------------------
def _follows(P, golden, kinds):
    """kinds: 'r' (a residual norm) or 'e' (a maximum error) per printed value.  The residuals under the rule of
    tests/test_gpu_solver.py:25 (_close): 1e-10 relative per iterate, and -- the coefficient exp(u) passes through the device's libm in
    every launch -- the perturbation the converged iterates carry, 1e-13 of the starting residual.  The maximum errors under the rule
    of tests/test_gpu_solver.py:46-50 for error histories: differences of nearly equal numbers, compared absolutely against the
    solution's magnitude (1e-9 relative + 1e-12)."""
    from test_gpu_solver import _close

    want = [float.fromhex(v) for v in golden["values"]]
    got = list(P.printed_values)
    assert len(got) == len(want) == len(kinds)
    for i, (g, w) in enumerate(zip(got, want)):
        print("value %d (%s): device %.17g restatement %.17g difference %.3e relative %.3e" % (i, kinds[i], g, w, abs(g - w), abs(g - w) / abs(w)))
    _close([g for g, k in zip(got, kinds) if k == "r"], [w for w, k in zip(want, kinds) if k == "r"])
    for g, w, k in zip(got, want, kinds):
        if k == "e":
            assert abs(g - w) <= 1e-9 * abs(w) + 1e-12


def test_bratu2d_prints_the_lines_of_the_results_file(hip):
    P, out = N.run("bratu2d_fas.exa4", N.K_BRATU2D, hip)
    assert out == N.results_lines()
    _follows(P, N.own_golden("bratu2d_fas"), "r" + "e" * 5)      # the start residual, then the error after every cycle


def test_bratu3d_follows_the_restatement(hip):
    g = N.own_golden("bratu3d_rbgs_fas")
    P, out = N.run("bratu3d_rbgs_fas.exa4", N.K_BRATU3D, hip)
    assert out[-1] == g["lines"][-1]
    _follows(P, g, "r" + "re" * 8)


@pytest.mark.parametrize("name,k", [("bratu2d_fas.exa4", dict(N.K_BRATU2D, maxLevel=3)), ("bratu3d_rbgs_fas.exa4", dict(N.K_BRATU3D, maxLevel=4))],
                         ids=["bratu2d", "bratu3d"])
def test_fas_cycle_replayed_from_a_hipgraph_equals_its_interpretation(hip, name, k):
    import graph_cases as gc

    from exastencils_amd import exa4

    G = exa4.Exa4Program(N.text(name), dict(k), ops=hip, auto_graph=True)
    P = exa4.Exa4Program(N.text(name), dict(k), ops=hip, auto_graph=False)
    G.run()
    P.run()
    gc.assert_same_run(G, P)
    rec = gc.recorded(G)
    cycles = int(P.out[-1].split()[-1])
    print(name, "recorded", rec, "replays", G.graph_replays)
    assert rec[("Cycle", k["maxLevel"])] == cycles - 1 and G.graph_replays >= cycles - 1
