"""The CPU oracle (oracle/examg_oracle.c) against the exact reference of tests/stencil_cases.py, on asymmetric constant stencils in
several entry orders and on exact data: every loop and every composition that the GPU parity tests use as their yardstick must
return exactly the mathematical value.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import stencil_cases as S
from oracle_ops import OracleOps
from stencil_cases import APPLY, RESIDUAL, SMOOTH, ExactOps

from exastencils_amd.layout import FieldLayout


@pytest.fixture(scope="module")
def orc():
    return OracleOps()


@pytest.fixture(scope="module")
def ex():
    return ExactOps()


def _stencil(kind, order):
    return {"7": S.exact7, "5": S.exact5, "27": S.exact27}[kind](order)


KINDS = [("7", o) for o in S.ORDERS7] + [("5", o) for o in S.ORDERS5] + [("27", o) for o in S.ORDERS27]


def _geometry(kind, variant):
    """(nd, cells, u layout, rhs layout, box): a non-cube fragment; `variant`: plain, padded (align 2 / 16), two ghost layers, a
    box over the duplicate planes, a box inside the inner points with odd origins."""
    nd = 2 if kind == "5" else 3
    shape = (13, 10, 8) if nd == 3 else (17, 12, 0)
    ghost, align = 1, 0
    if variant == "align2":
        align = 2
    elif variant == "align16":
        align = 16
    elif variant == "ghost2":
        ghost = 2
    lu = FieldLayout.node(nd, shape, ghost, align=align)
    lf = FieldLayout.node(nd, shape, 1 if variant == "ghost2" else 0, align=align)
    if variant == "dup":
        b, e = [0, 0, 0], [shape[0] + 1, shape[1] + 1, shape[2] + 1 if nd == 3 else 1]
    elif variant == "inside":
        b, e = [3, 1, 3 if nd == 3 else 0], [shape[0] - 2, shape[1] - 1, shape[2] - 1 if nd == 3 else 1]
    else:
        b, e = [1, 1, 1 if nd == 3 else 0], [shape[0], shape[1], shape[2] if nd == 3 else 1]
    return nd, shape, lu, lf, b, e


def _fields(ops, lays, seed):
    return [ops.from_host(S.int_field(l.size, seed + i)) for i, l in enumerate(lays)]


def _host(ops, ts):
    return [np.array(ops.to_host(t), dtype=np.float64, copy=True) for t in ts]


def _assert_equal(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            d = np.abs(g - w)
            raise AssertionError("%s[%d]: %d of %d values differ, max abs %.3e" % (what, i, int((d > 0).sum()), d.size, d.max()))


def test_the_stencils_are_asymmetric():
    """Mirror coefficients differ in every stencil kind, also in magnitude for the stars; the weights are not 0.8 / diag."""
    for st in [S.exact7(), S.exact5(), S.convdiff7((130, 120, 110)), S.convdiff5((257, 200, 0)), S.exact7(coefs=S.INT7)]:
        c = dict(zip(st.offsets, st.coefs))
        for d in range(3 if len(c) == 7 else 2):
            m = [0, 0, 0]
            m[d] = 1
            assert abs(c[tuple(m)]) != abs(c[tuple(-v for v in m)])
        assert len(set(abs(v) for v in c.values())) == len(c)
    for st in (S.exact27(), S.random27()):
        c = dict(zip(st.offsets, st.coefs))
        assert all(c[o] != c[tuple(-v for v in o)] for o in c if o != (0, 0, 0))
    assert S.EXACT_W != 0.8 / S.exact7().diag and S.free_weight(S.convdiff7((64, 64, 64))) != 0.8 / S.convdiff7((64, 64, 64)).diag
    for k, o in KINDS:
        st = _stencil(k, o)
        if o.startswith("perm"):
            assert st.offsets[0] != (0, 0, 0)


def test_exact_reference_refuses_what_it_cannot_do_exactly(ex):
    """Non-dyadic coefficients and in-place colour loops of a 27-point stencil (loop-order dependent) are refused, not rounded."""
    lu = FieldLayout.node(3, (6, 6, 6), 1)
    u, f = ex.from_host(S.int_field(lu.size, 1)), ex.from_host(S.int_field(lu.size, 2))
    with pytest.raises(ValueError):
        ex.stencil_op(SMOOTH, lu, u, lu, f, lu, ex.clone(u), S.convdiff7((6, 6, 6)), 0.1, -1, [1, 1, 1], [6, 6, 6])
    with pytest.raises(ValueError):
        ex.stencil_op(SMOOTH, lu, u, lu, f, lu, u, S.exact27(), S.EXACT_W, 0, [1, 1, 1], [6, 6, 6])
    with pytest.raises(AssertionError):      # values out of the exactly representable range
        big = ex.from_host(np.full(lu.size, 2.0 ** 19))
        ex.stencil_op(APPLY, lu, big, None, None, lu, ex.clone(u), S.exact27(), 0.0, -1, [1, 1, 1], [6, 6, 6])


@pytest.mark.parametrize("kind,order", KINDS)
@pytest.mark.parametrize("variant", ["plain", "align2", "align16", "ghost2", "dup", "inside"])
def test_oracle_stencil_loop_is_exact(orc, ex, kind, order, variant):
    """orc_stencil_op in APPLY, RESIDUAL and SMOOTH, colour -1, 0 and 1, over the whole destination array (outside the box it keeps
    what it held).  The 27-point stencil's colour loops run out of place: in place they depend on the loop order."""
    st = _stencil(kind, order)
    nd, shape, lu, lf, b, e = _geometry(kind, variant)
    for mode in (APPLY, RESIDUAL, SMOOTH):
        for colour in ((-1, 0, 1) if mode == SMOOTH else (-1,)):
            in_place = colour >= 0 and kind != "27"

            def run(ops):
                u, f, d = _fields(ops, (lu, lf, lu), 10)
                dst = u if in_place else d
                ops.stencil_op(mode, lu.c_struct(), u, lf.c_struct(), f, lu.c_struct(), dst, st, S.EXACT_W, colour, b, e)
                return _host(ops, (u, f, d))

            _assert_equal(run(orc), run(ex), "%s-point %s, %s, mode %d colour %d" % (kind, order, variant, mode, colour))


@pytest.mark.parametrize("nd,shape,scale,box", [
    (3, (14, 10, 12), 1.0, "inner"), (3, (14, 10, 12), 4.0, "dup"), (3, (18, 12, 10), 4.0, "inside"), (2, (18, 14, 0), 1.0, "inner"),
    (2, (18, 14, 0), 4.0, "dup")])
@pytest.mark.parametrize("align", [0, 2])
def test_oracle_transfers_are_exact(orc, ex, nd, shape, scale, box, align):
    """orc_restrict (full weighting, scale 1 and 4) and orc_prolong_add (trilinear interpolation added), whole arrays."""
    cs = tuple(s // 2 for s in shape)
    lfi, lco, lrh = FieldLayout.node(nd, shape, 1, align=align), FieldLayout.node(nd, cs, 1, align=align), FieldLayout.node(nd, cs, 0, align=align)
    z = 1 if nd == 3 else 0
    if box == "inner":
        cb, ce, fb, fe = [1, 1, z], [cs[0], cs[1], cs[2] if nd == 3 else 1], [1, 1, z], [shape[0], shape[1], shape[2] if nd == 3 else 1]
    elif box == "dup":
        cb, ce, fb, fe = [0, 1, 0], [cs[0] + 1, cs[1], cs[2] + 1 if nd == 3 else 1], [0, 0, 0], [shape[0] + 1, shape[1] + 1, shape[2] + 1 if nd == 3 else 1]
    else:
        cb, ce, fb, fe = [2, 1, 3 if nd == 3 else 0], [cs[0] - 1, cs[1] - 2, cs[2] - 1 if nd == 3 else 1], [3, 1, 3 if nd == 3 else 0], [shape[0] - 2, shape[1] - 3, shape[2] - 1 if nd == 3 else 1]

    def run(ops):
        r, fc, uc, uf = _fields(ops, (lfi, lrh, lco, lfi), 20)
        ops.restrict(lfi.c_struct(), r, lrh.c_struct(), fc, scale, cb, ce)
        ops.prolong_add(lco.c_struct(), uc, lfi.c_struct(), uf, fb, fe)
        return _host(ops, (r, fc, uc, uf))

    _assert_equal(run(orc), run(ex), "transfers")


def _comp_geometry(kind):
    nd = 2 if kind == "5" else 3
    shape = (14, 12, 10) if nd == 3 else (18, 14, 0)
    lu, lf = FieldLayout.node(nd, shape, 1), FieldLayout.node(nd, shape, 0)
    lc = FieldLayout.node(nd, tuple(s // 2 for s in shape), 1)
    b, e = [1, 1, 1 if nd == 3 else 0], [shape[0], shape[1], shape[2] if nd == 3 else 1]
    b2, e2 = [2, 1, 2 if nd == 3 else 0], [shape[0] - 1, shape[1], shape[2] - 1 if nd == 3 else 1]
    return nd, shape, lu, lf, lc, b, e, b2, e2


COMPOSITIONS = ["jacobi2", "jacobi3", "rbgs_sweep_fused", "rbgs_sweep_fused_zero", "rbgs_sweep_fused_prolong", "rbgs_sweep_fused_boxes",
                "rbgs_colours3", "jacobi2_prolong", "jacobi2_boxes", "jacobi_residual", "residual_restrict"]


@pytest.mark.parametrize("kind,order,name", [(k, o, n) for k, o in KINDS if k != "27" for n in COMPOSITIONS] +
                         [("27", "perm", n) for n in COMPOSITIONS if "rbgs" not in n and "colours" not in n])
def test_oracle_compositions_are_exact(orc, ex, kind, order, name):
    """The compositions of OracleOps that the GPU parity tests use as their reference, against the exact loops: the box of the
    output (their writes outside it differ by design), the inputs untouched.  The 27-point stencil only where no colour loop runs in
    place."""
    st = _stencil(kind, order)
    nd, shape, lu, lf, lc, b, e, b2, e2 = _comp_geometry(kind)
    if nd == 2 and "prolong" in name:
        lc = FieldLayout.node(2, tuple(s // 2 for s in shape), 1)
    L, F, Lc = lu.c_struct(), lf.c_struct(), lc.c_struct()
    w = S.EXACT_W
    ob, oe = (b2, e2) if name.endswith("_boxes") else (b, e)

    def run(ops, exact):
        u, f, out, res, uc = _fields(ops, (lu, lf, lu, lu, lc), 30)
        if name == "residual_restrict":
            cs = tuple(s // 2 for s in shape)
            lr = FieldLayout.node(nd, cs, 0)
            fc = ops.from_host(S.int_field(lr.size, 77))
            cb, ce = [1, 1, 1 if nd == 3 else 0], [cs[0], cs[1], cs[2] if nd == 3 else 1]
            if exact:
                S.residual_restrict(ops, L, u, F, f, st, lr.c_struct(), fc, 4.0, b, e, cb, ce)
            else:
                r = ops.new_array(lu.size)
                ops.residual_restrict(L, u, F, f, L, r, st, lr.c_struct(), fc, 4.0, b, e, cb, ce)
            return _host(ops, (fc, u, f)), None
        if name == "jacobi_residual":
            out = ops.clone(u) if exact else u.clone()       # u_out holds u_in's values on the box's shell
            if exact:
                S.jacobi_residual(ops, L, u, out, F, f, L, res, st, w, b, e)
            else:
                ops.jacobi_residual(L, u, out, F, f, L, res, st, w, b, e)
            return _host(ops, (out, res, u, f)), None
        tmp = None if exact else u.clone()        # OracleOps.jacobi2 reads the box's shell from tmp
        if exact:
            call = {"jacobi2": lambda: S.jacobi2(ops, L, u, out, F, f, st, w, b, e),
                    "jacobi3": lambda: S.jacobi3(ops, L, u, out, F, f, st, w, b, e),
                    "rbgs_sweep_fused": lambda: S.rbgs_sweep(ops, L, u, out, F, f, st, w, 1, b, e),
                    "rbgs_sweep_fused_zero": lambda: S.rbgs_sweep_zero(ops, L, out, F, f, st, w, 0, b, e),
                    "rbgs_sweep_fused_prolong": lambda: S.rbgs_sweep_prolong(ops, L, u, out, F, f, st, w, 1, b, e, Lc, uc),
                    "rbgs_sweep_fused_boxes": lambda: S.rbgs_sweep_boxes(ops, L, u, out, F, f, st, w, 0, b, e, b2, e2),
                    "rbgs_colours3": lambda: S.rbgs_colours3(ops, L, u, out, F, f, st, w, 1, b, e),
                    "jacobi2_prolong": lambda: S.jacobi2_prolong(ops, L, u, out, F, f, st, w, b, e, Lc, uc),
                    "jacobi2_boxes": lambda: S.jacobi2_boxes(ops, L, u, out, F, f, st, w, b, e, b2, e2)}[name]
        else:
            call = {"jacobi2": lambda: ops.jacobi2(L, u, out, tmp, F, f, st, w, b, e),
                    "jacobi3": lambda: ops.jacobi3(L, u, out, tmp, F, f, st, w, b, e),
                    "rbgs_sweep_fused": lambda: ops.rbgs_sweep_fused(L, u, out, F, f, st, w, 1, b, e),
                    "rbgs_sweep_fused_zero": lambda: ops.rbgs_sweep_fused_zero(L, out, F, f, st, w, 0, b, e),
                    "rbgs_sweep_fused_prolong": lambda: ops.rbgs_sweep_fused_prolong(L, u, out, F, f, st, w, 1, b, e, Lc, uc),
                    "rbgs_sweep_fused_boxes": lambda: ops.rbgs_sweep_fused_boxes(L, u, out, tmp, F, f, st, w, 0, b, e, b2, e2),
                    "rbgs_colours3": lambda: ops.rbgs_colours3(L, u, out, F, f, st, w, 1, b, e),
                    "jacobi2_prolong": lambda: ops.jacobi2_prolong(L, u, out, tmp, F, f, st, w, b, e, Lc, uc),
                    "jacobi2_boxes": lambda: ops.jacobi2_boxes(L, u, out, tmp, F, f, st, w, b, e, b2, e2)}[name]
        call()
        return _host(ops, (out, u, f, uc)), S.box_mask(lu, ob, oe)

    got, m = run(orc, False)
    want, _ = run(ex, True)
    if m is not None:
        got[0], want[0] = got[0][m], want[0][m]
    _assert_equal(got, want, "%s, %s-point %s" % (name, kind, order))


def test_three_steps_stay_exact_on_the_deepest_composition(ex):
    """The deepest composition of the GPU suite -- three Jacobi steps, the residual of the result and its restriction -- on the
    largest exact values the fields take: the reference itself asserts that every value stays exactly representable."""
    shape = (20, 16, 12)
    lu, lf, lr = FieldLayout.node(3, shape, 1), FieldLayout.node(3, shape, 0), FieldLayout.node(3, tuple(s // 2 for s in shape), 0)
    for st in (S.exact7("perm_b"), S.exact27("perm")):
        u = ex.from_host(np.full(lu.size, 16.0) * np.where(np.arange(lu.size) % 2, 1, -1))
        f = ex.from_host(np.full(lf.size, -16.0))
        out, fc = ex.clone(u), ex.new_array(lr.size)
        S.jacobi3(ex, lu, u, out, lf, f, st, S.EXACT_W, [1, 1, 1], list(shape))
        S.residual_restrict(ex, lu, out, lf, f, st, lr, fc, 4.0, [1, 1, 1], list(shape), [1, 1, 1], [s // 2 for s in shape])
        assert np.all(np.isfinite(ex.to_host(fc)))


# -- one interpreter run with an asymmetric constant stencil ----------------------------------------------------------------------
CONVDIFF_EXA4 = """
Domain global< [0.0, 0.0, 0.0] to [1.0, 1.0, 1.0] >

Layout Halo< Real, Node >@all {
  duplicateLayers = [1, 1, 1] with communication
  ghostLayers     = [1, 1, 1] with communication
}
Layout Plain< Real, Node >@all {
  duplicateLayers = [1, 1, 1] with communication
  ghostLayers     = [0, 0, 0]
}

Field u< global, Halo, 0.0 >@(all but finest)
Field u< global, Halo, vf_boundaryPosition_x ** 2 - 0.5 * vf_boundaryPosition_y ** 2 - 0.5 * vf_boundaryPosition_z ** 2 >@finest
Field f< global, Plain, None >@all
Field r< global, Halo, 0.0 >@all

Stencil A@all {
  [ 0,  0,  0] =>  2.0 / ( vf_gridWidth_x ** 2 ) + 1.2 / ( vf_gridWidth_y ** 2 ) + 2.8 / ( vf_gridWidth_z ** 2 ) + 3.0 / vf_gridWidth_x + 2.0 / vf_gridWidth_y + 1.0 / vf_gridWidth_z
  [-1,  0,  0] => -1.0 / ( vf_gridWidth_x ** 2 ) - 3.0 / vf_gridWidth_x
  [ 1,  0,  0] => -1.0 / ( vf_gridWidth_x ** 2 )
  [ 0, -1,  0] => -0.6 / ( vf_gridWidth_y ** 2 )
  [ 0,  1,  0] => -0.6 / ( vf_gridWidth_y ** 2 ) - 2.0 / vf_gridWidth_y
  [ 0,  0, -1] => -1.4 / ( vf_gridWidth_z ** 2 ) - 1.0 / vf_gridWidth_z
  [ 0,  0,  1] => -1.4 / ( vf_gridWidth_z ** 2 )
}
Stencil R from default restriction on Node with "linear"
Stencil P from default prolongation on Node with "linear"

Function Defect@all {
  communicate u
  loop over r {
    r = f - A * u
  }
  apply bc to r
}

Function Norm@finest : Real {
  Var s : Real = 0.0
  loop over r with reduction ( + : s ) {
    s += r * r
  }
  return sqrt ( s )
}

Function Sweeps@all {
  repeat 3 times {
    color with {
      ( i0 + i1 + i2 ) % 2,
      communicate u
      loop over u {
        u += 0.8 / diag ( A ) * ( f - A * u )
      }
      apply bc to u
    }
  }
}

Function Cycle@(all but coarsest) {
  Sweeps ( )
  Defect ( )
  communicate r
  loop over f@coarser {
    f@coarser = R * r
  }
  loop over u@coarser {
    u@coarser = 0.0
  }
  apply bc to u@coarser
  Cycle@coarser ( )
  communicate u@coarser
  loop over u {
    u += P@coarser * u@coarser
  }
  apply bc to u
  Sweeps ( )
}

Function Cycle@coarsest {
  repeat 16 times {
    Sweeps ( )
  }
}

Function Application {
  apply bc to u@finest
  Defect@finest ( )
  Var res0 : Real = Norm@finest ( )
  Var res : Real = res0
  print ( "initial residual", res0 )
  Var it : Int = 0
  repeat until it >= 5 || res <= 1.0E-9 * res0 {
    it += 1
    Cycle@finest ( )
    Defect@finest ( )
    res = Norm@finest ( )
    print ( "cycle", it, "residual", res )
  }
}
"""


def convdiff_program(ops, fuse=True, lo=2, hi=6):
    from exastencils_amd import exa4

    return exa4.Exa4Program(CONVDIFF_EXA4, dict(dimensionality=3, minLevel=lo, maxLevel=hi), ops=ops, fuse=fuse)


def test_convection_diffusion_program_fused_equals_unfused():
    """An ExaSlang-4 V-cycle with a mild convection-diffusion stencil (no two coefficients equal; smoother sweeps on the coarsest
    level, CG needs a symmetric operator) through the interpreter on the oracle: the one-pass forms and the cross-statement fusions
    change no bit of the printed residuals or the solution, and the residual goes down."""
    P = convdiff_program(OracleOps())
    P.run()
    Q = convdiff_program(OracleOps(), fuse=False)
    Q.run()
    assert P.printed_values == Q.printed_values and len(P.printed_values) >= 4
    assert sum(P.fusions.values()) > 0 and P.launches < Q.launches
    assert np.array_equal(P.fields[("u", 6)].data().numpy(), Q.fields[("u", 6)].data().numpy())
    assert P.printed_values[-1] < 0.1 * P.printed_values[0]


# -- stencil fields (variable coefficients) -------------------------------------------------------------------------------------------
from stencil_cases import FoldOps  # noqa: E402

FIELD_KINDS = ["vc7", "vc7_perm_a", "vc7_perm_b", "vc5", "vc5_perm", "h27", "h27_perm"]


@pytest.fixture(scope="module")
def fold():
    return FoldOps()


def _field_geometry(kind, variant):
    """(nd, u layout, rhs layout, destination layout, coefficient layout, box).  'own': every argument in a layout of its own (ghost
    widths 2 / 0 / 1 / 1, alignments 0 / 2 / 4 / 16); 'same': destination = u layout and coefficients in the rhs layout object (what
    the older tests pass); 'dup' / 'inside': own layouts, a box over the duplicate planes / inside the inner points."""
    nd = 2 if kind.startswith("vc5") else 3
    shape = (13, 10, 8) if nd == 3 else (17, 12, 0)
    if variant == "same":
        lu, lf = FieldLayout.node(nd, shape, 1), FieldLayout.node(nd, shape, 0)
        ld, lc = lu, lf
    else:
        lu, lf = FieldLayout.node(nd, shape, 2), FieldLayout.node(nd, shape, 0, align=2)
        ld, lc = FieldLayout.node(nd, shape, 1, align=4), FieldLayout.node(nd, shape, 1, align=16)
    z = nd == 3
    if variant == "dup":
        b, e = [0, 0, 0], [shape[0] + 1, shape[1] + 1, shape[2] + 1 if z else 1]
    elif variant == "inside":
        b, e = [3, 1, 3 if z else 0], [shape[0] - 2, shape[1] - 1, shape[2] - 1 if z else 1]
    else:
        b, e = [1, 1, 1 if z else 0], [shape[0], shape[1], shape[2] if z else 1]
    return nd, lu, lf, ld, lc, b, e


def _field_run(ops, kind, variant, data, mode, colour, wform, in_place):
    nd, lu, lf, ld, lc, b, e = _field_geometry(kind, variant)
    st = S.stencil_field(ops, S.field_offsets(kind), lc, data, 41, wform)
    u, f = S.data_field(ops, lu.size, data, 42), S.data_field(ops, lf.size, data, 43)
    d = S.data_field(ops, ld.size, data, 44)
    w = S.EXACT_W if data == "exact" else 0.713
    if in_place:
        ops.stencil_op(mode, lu.c_struct(), u, lf.c_struct(), f, lu.c_struct(), u, st, w, colour, b, e)
    else:
        ops.stencil_op(mode, lu.c_struct(), u, lf.c_struct(), f, ld.c_struct(), d, st, w, colour, b, e)
    return _host(ops, (u, f, d, st.cfield))


def test_the_stencil_field_data_is_what_the_tests_need(ex):
    """Entry lists: the reference's order and permutations with the centre elsewhere.  Exact coefficients: multiples of 1/4 of both
    signs over the whole allocation, no two entries of a point's neighbourhood systematically equal, the diagonal from {4, 8, 16}.
    The distinct layouts differ in size, reference offset and row length: an index formed with another argument's layout lands on
    another point."""
    from exastencils_amd.field import helmholtz27_offsets, stencil_field_offsets

    assert S.field_offsets("vc7") == stencil_field_offsets(3) and S.field_offsets("h27") == helmholtz27_offsets()
    for kind in FIELD_KINDS:
        offs = S.field_offsets(kind)
        nd, lu, lf, ld, lc, b, e = _field_geometry(kind, "own")
        a = S.coefficient_array(offs, lc, "exact", 41).reshape(len(offs), lc.size)
        d = offs.index((0, 0, 0))
        assert (d != 0) == ("perm" in kind)
        assert set(np.unique(a[d])) == set(S.EXACT_DIAGS)
        off = np.delete(a, d, axis=0)
        assert np.array_equal(off * 4, np.round(off * 4)) and (off > 0).any() and (off < 0).any() and not (off == 0).any()
        assert all(not np.array_equal(a[i], a[j]) for i in range(len(offs)) for j in range(i))
        r = S.coefficient_array(offs, lc, "random", 41).reshape(len(offs), lc.size)
        assert (np.delete(r, d, axis=0) < 0).any() and r[d].min() >= 2.0
        lays = [S._Lay(l) for l in (lu, lf, ld, lc)]
        assert len({(tuple(L.tot), tuple(L.ref)) for L in lays}) == 4 and len({L.tot[0] for L in lays}) == 4


@pytest.mark.parametrize("kind", FIELD_KINDS)
@pytest.mark.parametrize("variant", ["own", "same", "dup", "inside"])
def test_oracle_stencil_field_loop_is_exact(orc, ex, kind, variant):
    """orc_stencil_op on a stencil field, exact data, against the exact reference: APPLY, RESIDUAL and SMOOTH with colours -1, 0, 1 and
    both weight forms, over the whole u, rhs, destination and coefficient arrays.  The 27-entry fields' colour loops run out of place."""
    for mode in (APPLY, RESIDUAL, SMOOTH):
        for colour in ((-1, 0, 1) if mode == SMOOTH else (-1,)):
            for wform in ((0, 1) if mode == SMOOTH else (0,)):
                in_place = colour >= 0 and not kind.startswith("h27")
                got = _field_run(orc, kind, variant, "exact", mode, colour, wform, in_place)
                want = _field_run(ex, kind, variant, "exact", mode, colour, wform, in_place)
                _assert_equal(got, want, "%s %s, mode %d colour %d wform %d" % (kind, variant, mode, colour, wform))


@pytest.mark.parametrize("kind", FIELD_KINDS)
@pytest.mark.parametrize("variant", ["own", "same", "dup"])
def test_oracle_stencil_field_loop_folds_as_the_header_says(orc, fold, kind, variant):
    """The same on random data against the float64 restatement of the statement order, bit for bit; the two weight forms and a
    diagonal taken from entry 0 must differ from the right result somewhere (the data can tell them apart)."""
    for mode in (APPLY, RESIDUAL, SMOOTH):
        for colour in ((-1, 0, 1) if mode == SMOOTH else (-1,)):
            for wform in ((0, 1) if mode == SMOOTH else (0,)):
                in_place = colour >= 0 and not kind.startswith("h27")
                got = _field_run(orc, kind, variant, "random", mode, colour, wform, in_place)
                want = _field_run(fold, kind, variant, "random", mode, colour, wform, in_place)
                _assert_equal(got, want, "%s %s, mode %d colour %d wform %d" % (kind, variant, mode, colour, wform))
    a = _field_run(fold, kind, variant, "random", SMOOTH, -1, 0, False)
    b = _field_run(fold, kind, variant, "random", SMOOTH, -1, 1, False)
    assert not np.array_equal(a[2], b[2])


def test_fold_reference_equals_the_oracle_on_constant_stencils(orc, fold):
    """FoldOps on constant stencils (asymmetric, permuted orders): the bits of the oracle's loop."""
    for st, nd in ((S.convdiff7((13, 10, 8), "perm_b"), 3), (S.convdiff5((17, 12, 0), "perm_a"), 2), (S.random27("perm"), 3)):
        shape = (13, 10, 8) if nd == 3 else (17, 12, 0)
        lu, lf, ld = FieldLayout.node(nd, shape, 2), FieldLayout.node(nd, shape, 0, align=2), FieldLayout.node(nd, shape, 1, align=4)
        b, e = [1, 1, 1 if nd == 3 else 0], [shape[0], shape[1], shape[2] if nd == 3 else 1]
        for mode in (APPLY, RESIDUAL, SMOOTH):
            def run(ops):
                u, f, d = (S.data_field(ops, l.size, "random", 50 + i) for i, l in enumerate((lu, lf, ld)))
                ops.stencil_op(mode, lu.c_struct(), u, lf.c_struct(), f, ld.c_struct(), d, st, S.free_weight(st), -1, b, e)
                return _host(ops, (u, f, d))

            _assert_equal(run(orc), run(fold), "constant stencil, mode %d" % mode)


def test_exact_reference_refuses_stencil_fields_it_cannot_do_exactly(ex):
    """A transformed coefficient array, a diagonal that is no power of two and coefficients finer than 2^-8 are refused."""
    import dataclasses

    lu, lc = FieldLayout.node(3, (6, 6, 6), 1), FieldLayout.node(3, (6, 6, 6), 0)
    offs = S.field_offsets("vc7")
    u, f = ex.from_host(S.int_field(lu.size, 1)), ex.from_host(S.int_field(lc.size, 2))
    st = S.stencil_field(ex, offs, lc, "exact", 3)
    args = (lu, u, lc, f, lu, ex.clone(u))
    ex.stencil_op(SMOOTH, *args, st, S.EXACT_W, -1, [1, 1, 1], [6, 6, 6])
    with pytest.raises(ValueError):
        ex.stencil_op(SMOOTH, *args, dataclasses.replace(st, ctransform=1), S.EXACT_W, -1, [1, 1, 1], [6, 6, 6])
    a = S.coefficient_array(offs, lc, "exact", 3)
    a[:lc.size] = 6.0
    with pytest.raises(ValueError):
        ex.stencil_op(SMOOTH, *args, dataclasses.replace(st, cfield=ex.from_host(a)), S.EXACT_W, -1, [1, 1, 1], [6, 6, 6])
    a[:lc.size] = 8.0
    a[lc.size:2 * lc.size] = 2.0 ** -9
    with pytest.raises(ValueError):
        ex.stencil_op(APPLY, *args, dataclasses.replace(st, cfield=ex.from_host(a)), 0.0, -1, [1, 1, 1], [6, 6, 6])


@pytest.mark.parametrize("kind", ["vc7_perm_b", "h27", "h27_perm"])
def test_stencil_field_compositions_stay_exact(orc, ex, kind):
    """The deepest stencil-field compositions of the GPU suite on exact data -- two Jacobi steps and the residual of the result, a
    Jacobi step + residual, a red-black sweep, the residual of a smoothed field + its restriction -- with distinct layouts: the reference
    asserts that every value stays exactly representable, and the oracle's loops give the same values.  (Every step of a stencil-field
    smoother divides by up to 16 * 16: three steps in a row need more than the 32 fractional bits of the reference.)"""
    shape = (20, 16, 12)
    lu, lf, lr, lc = (FieldLayout.node(3, shape, 2), FieldLayout.node(3, shape, 0, align=2), FieldLayout.node(3, shape, 1, align=4),
                      FieldLayout.node(3, shape, 1, align=16))
    lco = FieldLayout.node(3, tuple(s // 2 for s in shape), 0)
    b, e = [1, 1, 1], list(shape)
    cb, ce = [1, 1, 1], [s // 2 for s in shape]

    def run(ops):
        st = S.stencil_field(ops, S.field_offsets(kind), lc, "exact", 61)
        u, f, res = (S.data_field(ops, l.size, "exact", 62 + i) for i, l in enumerate((lu, lf, lr)))
        out, out2, out3 = ops.clone(u) if hasattr(ops, "clone") else u.clone(), S._clone(ops, u), S._clone(ops, u)
        fc = S.data_field(ops, lco.size, "exact", 66)
        L, F = lu.c_struct(), lf.c_struct()
        S.jacobi2(ops, L, u, out, F, f, st, S.EXACT_W, b, e)
        ops.stencil_op(RESIDUAL, L, out, F, f, lr.c_struct(), res, st, 0.0, -1, b, e)
        res2 = S._clone(ops, res)
        S.jacobi_residual(ops, L, u, out2, F, f, lr.c_struct(), res2, st, S.EXACT_W, b, e)
        if not kind.startswith("h27"):
            S.rbgs_sweep(ops, L, u, out3, F, f, st, S.EXACT_W, 1, b, e)
        S.residual_restrict(ops, L, out2, F, f, st, lco.c_struct(), fc, 4.0, b, e, cb, ce)
        return _host(ops, (out, out2, res, res2, out3, fc, u, f))

    _assert_equal(run(orc), run(ex), "compositions on %s" % kind)


def test_residual_norm_of_a_stencil_field_is_exact(orc, ex):
    """Integer coefficients and integer data: integer residuals, whose squares sum exactly in any order."""
    shape = (14, 12, 10)
    lu, lf, lc = FieldLayout.node(3, shape, 2), FieldLayout.node(3, shape, 0, align=2), FieldLayout.node(3, shape, 1, align=16)
    b, e = [1, 1, 1], list(shape)
    for kind in ("vc7", "h27_perm"):
        def run(ops):
            st = S.stencil_field(ops, S.field_offsets(kind), lc, "exact", 71, unit=1.0)
            u, f = S.data_field(ops, lu.size, "exact", 72), S.data_field(ops, lf.size, "exact", 73)
            s = ops.residual_norm2(lu.c_struct(), u, lf.c_struct(), f, st, b, e)
            return s if isinstance(s, float) else ops.scalar_value(s)

        assert run(orc) == run(ex) > 0


# -- stencil-field initialisation --------------------------------------------------------------------------------------------------------
ORC_FN_ASYM3D = 17      # oracle/examg_oracle.c: ((1.0 + x) + ((2.0 * y) * y)) + (4.0 * z)


def _init_geometry(nd):
    """A coefficient layout with ghost layers and padding, a box off the array edges, a power-of-two mesh width (h * h, 0.5 * h and the
    positions are exact: the only roundings are those of the coefficient expressions) and a fragment that does not start at 0."""
    from exastencils_amd.lib import GeomC

    shape = (16, 12, 10) if nd == 3 else (16, 12, 0)
    lc = FieldLayout.node(nd, shape, 1, align=4)
    g = GeomC()
    for d in range(3):
        g.pos_begin[d] = (0.25, -0.5, 1.0)[d] if d < nd else 0.0
        g.h[d] = (1.0 / 16, 1.0 / 8, 1.0 / 32)[d] if d < nd else 0.0
    b, e = [1, 0, 2 if nd == 3 else 0], [shape[0] - 1, shape[1] + 1, shape[2] - 1 if nd == 3 else 1]
    return lc, g, b, e


def test_the_asymmetric_coefficient_separates_mirrorings_and_axis_permutations():
    """The 48 images of a point under the mirrorings about the centre of the unit cube and the permutations of the axes get 48
    different coefficients (the exp profile of the reference's program gets one)."""
    import itertools

    p = np.array([0.1234, 0.2718, 0.4142])          # offsets from the centre
    vals = set()
    for perm in itertools.permutations(range(3)):
        for sg in itertools.product((1, -1), repeat=3):
            vals.add(float(S.asym_coefficient(*[0.5 + sg[d] * p[perm[d]] for d in range(3)])))
    assert len(vals) == 48
    x, y, z = np.array([0.375]), np.array([-0.25]), np.array([1.125])
    assert OracleOps._eval_program(S.ASYM_PROGRAM, x, y, z)[0] == S.asym_coefficient(x, y, z)[0]


@pytest.mark.parametrize("nd", [3, 2])
def test_oracle_init_varcoeff7_equals_the_definition(orc, nd):
    """orc_init_varcoeff7 with the asymmetric +, * coefficient against the numpy restatement of include/examg.h, with equality, over
    the whole array (nothing outside the box is written)."""
    lc, g, b, e = _init_geometry(nd)
    K = 2 * nd + 1
    start = np.random.default_rng(5).uniform(-1.0, 1.0, K * lc.size)
    cf = orc.from_host(start.copy())
    orc.init_varcoeff7(lc.c_struct(), cf, g, ORC_FN_ASYM3D, (), b, e)
    want = start.copy()
    S.init_varcoeff7_ref(lc, want, g, S.asym_coefficient, b, e)
    assert np.array_equal(orc.to_host(cf), want)
    assert int((want != start).sum()) == K * int(np.prod([e[d] - b[d] for d in range(3)]))


def test_oracle_init_helmholtz27_equals_the_definition(orc):
    lc, g, b, e = _init_geometry(3)
    for d in range(3):
        g.h[d] = 1.0 / 16
    start = np.random.default_rng(6).uniform(-1.0, 1.0, 27 * lc.size)
    cf = orc.from_host(start.copy())
    orc.init_helmholtz27(lc.c_struct(), cf, g, ORC_FN_ASYM3D, (0.0, 2.5), b, e)
    want = start.copy()
    S.init_helmholtz27_ref(lc, want, g, S.asym_coefficient, 2.5, b, e)
    assert np.array_equal(orc.to_host(cf), want)
    # the entries of the plane dz = -1 differ from those of dz = +1, and likewise in x and y: the coefficient is not symmetric
    W = want.reshape(27, -1)
    from exastencils_amd.field import helmholtz27_offsets

    offs = helmholtz27_offsets()
    m = S.box_mask(lc, b, e)
    for o in ((1, 1, 0), (0, 1, 1), (1, 0, 1)):
        for d in range(3):
            if o[d]:
                mir = tuple(-v if i == d else v for i, v in enumerate(o))
                assert not np.array_equal(W[offs.index(o)][m], W[offs.index(mir)][m])


# -- inter-grid transfers: the cell restatement and the oracle against the exact reference, closed forms, adjointness ---------------
from cell_ops import CellOracleOps  # noqa: E402


@pytest.fixture(scope="module")
def cellorc():
    return CellOracleOps()


# (nd, fine cells, fine ghost, fine align, coarse ghost, coarse align): ghost widths 0 / 1 / 2, the two layouts never alike
CELL_LAYOUTS = [(3, (12, 10, 8), 1, 0, 0, 2), (3, (14, 8, 10), 2, 2, 1, 0), (3, (10, 12, 8), 0, 16, 2, 2), (2, (18, 12, 0), 1, 2, 2, 0),
                (2, (12, 14, 0), 2, 0, 0, 16), (2, (16, 10, 0), 0, 0, 1, 2)]


def _cell_pair(nd, n, gf, af, gc, ac):
    lf = FieldLayout.cell(nd, n[:nd], gf, align=af)
    lc = FieldLayout.cell(nd, [v // 2 for v in n[:nd]], gc, False, ac)
    return lf, lc


def _cell_boxes(nd, n, ghost, coarse):
    """Boxes with odd and even begins and ends in every dimension: the whole field, and two inside it (a fine box may begin in the
    ghost layer: negative indices)."""
    m = [v // 2 if coarse else v for v in n[:nd]]
    z = nd == 3
    out = [([0, 0, 0], [m[0], m[1], m[2] if z else 1]), ([1, 2, 1 if z else 0], [m[0] - 2, m[1] - 1, m[2] - 1 if z else 1]),
           ([2, 1, 2 if z else 0], [m[0] - 1, m[1] - 2, m[2] - 1 if z else 1])]
    if not coarse and ghost:
        g = ghost
        out.append(([-1, -g, -1 if z else 0], [m[0] + 1, m[1] - 1, m[2] + g if z else 1]))
    assert all(e[d] > b[d] for b, e in out for d in range(3))
    return out


@pytest.mark.parametrize("scale", [1.0, 4.0, 0.25])
@pytest.mark.parametrize("nd,n,gf,af,gc,ac", CELL_LAYOUTS)
def test_cell_restatement_is_exact(cellorc, ex, nd, n, gf, af, gc, ac, scale):
    """CellOracleOps.restrict_cell / prolong_add_cell (tests/cell_ops.py, the bitwise reference of the GPU tests) against the exact
    reference written from the definitions: whole arrays, the inputs included; fine and coarse layouts differ in ghost and
    alignment."""
    lf, lc = _cell_pair(nd, n, gf, af, gc, ac)
    for cb, ce in _cell_boxes(nd, n, gc, True):
        def run(ops):
            rf, fc = _fields(ops, (lf, lc), 30)
            ops.restrict_cell(lf.c_struct(), rf, lc.c_struct(), fc, scale, cb, ce)
            return _host(ops, (rf, fc))

        _assert_equal(run(cellorc), run(ex), "restrict_cell %r %r" % (cb, ce))
    for fb, fe in _cell_boxes(nd, n, min(gf, 2 * gc), False):
        def run(ops):
            uc, uf = _fields(ops, (lc, lf), 40)
            ops.prolong_add_cell(lc.c_struct(), uc, lf.c_struct(), uf, fb, fe)
            return _host(ops, (uc, uf))

        _assert_equal(run(cellorc), run(ex), "prolong_add_cell %r %r" % (fb, fe))


def test_exact_cell_transfers_refuse_what_leaves_the_allocation(ex):
    lf, lc = _cell_pair(3, (8, 8, 8), 1, 0, 0, 0)
    uc, uf = _fields(ex, (lc, lf), 1)
    with pytest.raises(IndexError):          # fine cell -1 has parent -1: the coarse layout has no ghost layer
        ex.prolong_add_cell(lc, uc, lf, uf, [-1, 0, 0], [8, 8, 8])
    with pytest.raises(IndexError):
        ex.restrict_cell(lf, uf, lc, uc, 1.0, [0, 0, 0], [5, 4, 4])


# fine / coarse-rhs / coarse-solution layouts, each with its own ghost width and alignment
NODE_LAYOUTS = [((2, 0), (0, 2), (1, 16)), ((1, 16), (2, 0), (0, 2)), ((1, 2), (1, 0), (2, 4))]


def _node_triple(nd, fs, cs, lay):
    (gf, af), (gr, ar), (gs, as_) = NODE_LAYOUTS[lay]
    return (FieldLayout.node(nd, fs, gf, align=af), FieldLayout.node(nd, cs, gr, True, False, ar), FieldLayout.node(nd, cs, gs, align=as_))


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("lay", [0, 1, 2])
@pytest.mark.parametrize("nd,n,kind", [(3, (9, 4, 6), "inner"), (3, (7, 5, 4), "faces"), (3, (6, 3, 5), "inside_odd"), (3, (5, 7, 3), "inside_even"),
                                       (2, (9, 5, 0), "inner"), (2, (6, 8, 0), "faces"), (2, (7, 4, 0), "inside_odd")])
def test_oracle_transfers_are_exact_on_anisotropic_shapes(orc, ex, nd, n, kind, lay, scale):
    """orc_restrict / orc_prolong_add on boxes whose extents differ in every dimension, the fine, coarse-rhs and coarse-solution
    arrays each in a layout of its own: whole arrays, inputs included."""
    fs, cs, cb, ce = S.restrict_geometry(nd, n, kind)
    lfi, lrh, lco = _node_triple(nd, fs, cs, lay)
    # the prolongation box: the fine points of the restriction's footprint that have non-negative indices
    fb = [max(2 * cb[d] - 1, 0) if d < nd else 0 for d in range(3)]
    fe = [min(2 * ce[d], fs[d] + 1) if d < nd else 1 for d in range(3)]

    def run(ops):
        r, fc, uc, uf = _fields(ops, (lfi, lrh, lco, lfi), 50)
        ops.restrict(lfi.c_struct(), r, lrh.c_struct(), fc, scale, cb, ce)
        ops.prolong_add(lco.c_struct(), uc, lfi.c_struct(), uf, fb, fe)
        return _host(ops, (r, fc, uc, uf))

    _assert_equal(run(orc), run(ex), "transfers %s" % kind)


def _layers(orc, cellorc, ex, cell):
    return [cellorc if cell else orc, ex]


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("nd,n,kind,lay", [(3, (9, 4, 6), "inner", 0), (3, (7, 5, 4), "faces", 1), (3, (5, 7, 3), "inside_even", 2),
                                           (2, (9, 5, 0), "inner", 1), (2, (6, 8, 0), "faces", 0)])
def test_node_transfers_of_linear_fields_have_closed_forms(orc, cellorc, ex, nd, n, kind, lay, scale):
    """v = 3 i + 7 j + 11 k + 5: full weighting gives scale * v(2I); interpolating uc(I) = v(2I) onto zeros gives v.  Plain float64
    numpy with equality, on the oracle and on the exact reference."""
    fs, cs, cb, ce = S.restrict_geometry(nd, n, kind)
    lfi, lrh, lco = _node_triple(nd, fs, cs, lay)
    fb = [max(2 * cb[d] - 1, 0) if d < nd else 0 for d in range(3)]
    fe = [min(2 * ce[d], fs[d] + 1) if d < nd else 1 for d in range(3)]
    for ops in _layers(orc, cellorc, ex, False):
        fc, uf = ops.from_host(np.zeros(lrh.size)), ops.from_host(np.zeros(lfi.size))
        ops.restrict(lfi.c_struct(), ops.from_host(S.linear_field(lfi, S.LINEAR, 5)), lrh.c_struct(), fc, scale, cb, ce)
        ops.prolong_add(lco.c_struct(), ops.from_host(S.linear_field(lco, S.LINEAR, 5, mul=2)), lfi.c_struct(), uf, fb, fe)
        assert np.array_equal(S.box_values(lrh, ops.to_host(fc), cb, ce), scale * S.box_values(lrh, S.linear_field(lrh, S.LINEAR, 5, mul=2), cb, ce))
        assert np.array_equal(S.box_values(lfi, ops.to_host(uf), fb, fe), S.box_values(lfi, S.linear_field(lfi, S.LINEAR, 5), fb, fe))


@pytest.mark.parametrize("scale", [1.0, 4.0, 0.25])
@pytest.mark.parametrize("nd,n,gf,af,gc,ac", CELL_LAYOUTS)
def test_cell_transfers_of_linear_fields_have_closed_forms(orc, cellorc, ex, nd, n, gf, af, gc, ac, scale):
    """Fine values 2 v at the cell centres (2 v(i + 1/2) = 3 (2 i + 1) + ..: integers): the mean of the children is 2 v at the
    parent's centre, 3 (4 I + 2) + ..; the prolongation of a linear coarse field onto zeros gives uc(i >> 1)."""
    lf, lc = _cell_pair(nd, n, gf, af, gc, ac)
    for ops in _layers(orc, cellorc, ex, True):
        for cb, ce in _cell_boxes(nd, n, gc, True):
            fc = ops.from_host(np.zeros(lc.size))
            ops.restrict_cell(lf.c_struct(), ops.from_host(S.linear_field(lf, S.LINEAR, 10, mul=2, add=1)), lc.c_struct(), fc, scale, cb, ce)
            assert np.array_equal(S.box_values(lc, ops.to_host(fc), cb, ce), scale * S.box_values(lc, S.linear_field(lc, S.LINEAR, 10, mul=4, add=2), cb, ce))
        for fb, fe in _cell_boxes(nd, n, min(gf, 2 * gc), False):
            uf = ops.from_host(np.zeros(lf.size))
            ops.prolong_add_cell(lc.c_struct(), ops.from_host(S.linear_field(lc, S.LINEAR, 4)), lf.c_struct(), uf, fb, fe)
            idx = np.meshgrid(*[np.arange(fb[d], fe[d]) >> (1 if d < nd else 0) for d in (2, 1, 0)], indexing="ij")
            want = 4 + sum(S.LINEAR[d] * idx[2 - d] for d in range(nd))
            assert np.array_equal(S.box_values(lf, ops.to_host(uf), fb, fe), want.astype(np.float64))


@pytest.mark.parametrize("scale", [1.0, 4.0])
def test_restriction_is_the_scaled_adjoint_of_the_prolongation(orc, cellorc, ex, scale):
    """sum(fc * w) * 2^d == scale * sum(r * P w) for integer fields that vanish outside the boxes, in int64."""
    for nd, n, kind, lay in [(3, (9, 4, 6), "inner", 0), (3, (7, 5, 4), "faces", 1), (2, (9, 5, 0), "inside_odd", 2)]:
        fs, cs, cb, ce = S.restrict_geometry(nd, n, kind)
        lfi, lrh, _ = _node_triple(nd, fs, cs, lay)
        fb = [max(2 * cb[d] - 1, 0) if d < nd else 0 for d in range(3)]
        fe = [min(2 * ce[d], fs[d] + 1) if d < nd else 1 for d in range(3)]
        for ops in (orc, ex):
            lhs, rhs = S.transfer_adjoint(ops, False, lfi, lrh, cb, ce, fb, fe, scale, 60)
            assert lhs == rhs
    for nd, n, gf, af, gc, ac in CELL_LAYOUTS:
        lf, lc = _cell_pair(nd, n, gf, af, gc, ac)
        cb, ce = _cell_boxes(nd, n, gc, True)[1]
        fb, fe = _cell_boxes(nd, n, min(gf, 2 * gc), False)[-1]
        for ops in (cellorc, ex):
            lhs, rhs = S.transfer_adjoint(ops, True, lf, lc, cb, ce, fb, fe, scale, 70)
            assert lhs == rhs
