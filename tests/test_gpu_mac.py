"""GPU parity of the staggered-grid entry points (include/examg.h: examg_mac_op, examg_mac_relax, examg_mac_sweep, examg_restrict_face,
examg_prolong_add_face, examg_apply_bc_face, examg_fill_expr_face, examg_max_err_expr_face) against their numpy restatement
(tests/mac_ops.py): point-wise kernels, bit-identical over the WHOLE of every array -- a stray write outside the box, to a row outside the
mask, to a held face, to another colour or to an input shows.  Then the Stokes driver on HipOps."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mac_cases import H, LAYOUT_KINDS, SHAPES, MacData, boxes, colouring, parity, row_boxes
from mac_ops import BC_DIRICHLET, BC_NEUMANN, SYS_APPLY, SYS_RESIDUAL, MacOracleOps

from exastencils_amd.field import Colouring, Stencil
from exastencils_amd.layout import FieldLayout
from exastencils_amd.lib import ExamgError, ExprC, GeomC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    from exastencils_amd.ops import HipOps

    return HipOps(0)


@pytest.fixture(scope="module")
def orc():
    return MacOracleOps()


def same(a, b, what):
    if not np.array_equal(a, b):
        d = np.abs(a - b)
        raise AssertionError("%s: %d of %d values differ, max abs %.3e" % (what, int((d > 0).sum()), d.size, d.max()))


def compare(hip, orc, fn, what):
    """fn(ops) -> list of lists of arrays, one per call sequence; every array is compared whole."""
    g = fn(hip)
    hip.synchronize()
    c = fn(orc)
    assert len(g) == len(c) and g
    for k, (sg, sc) in enumerate(zip(g, c)):
        for j, (x, y) in enumerate(zip(sg, sc)):
            same(hip.to_host(x), orc.to_host(y), "%s, sequence %d, array %d" % (what, k, j))


# the two smallest shapes in all four layout kinds (ghost, align), the two larger ones -- the last has a colour row longer than a wave -- in
# two kinds that between them hold both ghost widths and both alignments
CASES = [(nd, cells, g, a) for nd in (2, 3) for k, cells in enumerate(SHAPES[nd])
         for g, a in (LAYOUT_KINDS if k < 2 else [LAYOUT_KINDS[k], LAYOUT_KINDS[3 - k]])]
IDS = ["%dd-%s-g%d-a%d" % (nd, "x".join(map(str, c)), g, a) for nd, c, g, a in CASES]


def op_all(ops, nd, cells, ghost, align, kind):
    """Every single row and all rows, APPLY and RESIDUAL, on the three boxes, each call on fresh data."""
    out = []
    for box in boxes(nd, cells).values():
        rb, re = row_boxes(nd, cells, box)
        for mode in (SYS_APPLY, SYS_RESIDUAL):
            for mask in [1 << r for r in range(nd + 1)] + [(1 << (nd + 1)) - 1]:
                D = MacData(ops, nd, cells, ghost, align, kind)
                ops.mac_op(mode, D.sys, mask, rb, re)
                out.append(D.arrays())
    return out


@pytest.mark.parametrize("nd,cells,ghost,align", CASES, ids=IDS)
def test_mac_op_bitwise(hip, orc, nd, cells, ghost, align):
    compare(hip, orc, lambda ops: op_all(ops, nd, cells, ghost, align, "asymmetric"), "mac_op")


def test_mac_op_bitwise_with_folds_of_one_entry(hip, orc):
    compare(hip, orc, lambda ops: op_all(ops, 3, (6, 3, 6), 1, 0, "few"), "mac_op few")


def test_mac_op_rows_on_boxes_of_their_own(hip, orc):
    """One launch, a different box per row, an empty one among them."""
    nd, cells = 2, (12, 9)

    def run(ops):
        D = MacData(ops, nd, cells)
        ops.mac_op(SYS_RESIDUAL, D.sys, 7, [[1, 0, 0], [5, 5, 0], [0, 2, 0]], [[12, 9, 1], [5, 9, 1], [3, 9, 1]])
        return [D.arrays()]

    compare(hip, orc, run, "row boxes")


def relax_all(ops, nd, cells, ghost, align, kind):
    """Every colour alone on the whole block with relax 1.0 and 0.8 and on the sub-box with 0.8; the colours one after the other and the
    full sweep on all three boxes with both."""
    cols = list(colouring(nd).colours())
    out = []
    B = boxes(nd, cells)
    for name, (b, e) in B.items():
        for relax in (1.0, 0.8):
            seqs = [tuple(cols), "sweep"]
            if name == "whole" or (name == "sub" and relax == 0.8):
                seqs += [(c,) for c in cols]
            for seq in seqs:
                D = MacData(ops, nd, cells, ghost, align, kind)
                if seq == "sweep":
                    ops.mac_sweep(D.sys, relax, colouring(nd), b, e)
                else:
                    for col in seq:
                        ops.mac_relax(D.sys, relax, col, b, e)
                out.append(D.arrays()[:2 * (nd + 1)])      # the smoother has no destination
    return out


@pytest.mark.parametrize("nd,cells,ghost,align", CASES, ids=IDS)
def test_mac_relax_and_sweep_bitwise(hip, orc, nd, cells, ghost, align):
    compare(hip, orc, lambda ops: relax_all(ops, nd, cells, ghost, align, "asymmetric"), "mac_relax")


@pytest.mark.parametrize("kind", ["few", "stokes"])
def test_mac_relax_bitwise_with_other_operators(hip, orc, kind):
    compare(hip, orc, lambda ops: relax_all(ops, 2, (12, 9), 1, 0, kind), "mac_relax %s" % kind)


def test_a_shifted_colouring_with_mixed_moduli(hip, orc):
    """`(1 + i1) % 4, (2 + i0) % 3`: the expressions in another order than the axes, a modulus above 3, shifts."""
    nd, cells = 2, (12, 9)
    col = Colouring((((1,), 1, 4), ((0,), 2, 3)))

    def run(ops):
        D, S = MacData(ops, nd, cells), MacData(ops, nd, cells)
        for c in col.colours():
            ops.mac_relax(D.sys, 0.8, c, [1, 0, 0], [11, 9, 1])
        ops.mac_sweep(S.sys, 0.8, col, [1, 0, 0], [11, 9, 1])
        return [D.arrays(), S.arrays()]

    compare(hip, orc, run, "mixed moduli")
    D, S = run(hip)
    hip.synchronize()
    for x, y in zip(D, S):
        same(hip.to_host(x), hip.to_host(y), "sweep against its colours")


def test_empty_boxes_are_no_ops(hip, orc):
    nd, cells = 2, (6, 3)

    def run(ops):
        D = MacData(ops, nd, cells)
        ops.mac_op(SYS_RESIDUAL, D.sys, 7, [[3, 2, 0]] * 3, [[3, 3, 1]] * 3)
        ops.mac_relax(D.sys, 1.0, next(colouring(nd).colours()), [1, 2, 0], [6, 2, 1])
        ops.mac_sweep(D.sys, 1.0, colouring(nd), [4, 0, 0], [4, 3, 1])
        l = D.sys.lu[0]
        ops.restrict_face(0, l.c_struct(), D.sys.u[0], l.c_struct(), D.sys.dst[0], 1.0, [1, 1, 0], [1, 2, 1])
        return [D.arrays()]

    compare(hip, orc, run, "empty boxes")


# -- transfers ------------------------------------------------------------------------------------------------------------------------------
def transfers(ops, nd, coarse, ghost, align):
    fine = tuple(2 * c for c in coarse)
    out = []
    for axis in range(nd):
        lf, lc = FieldLayout.face(nd, fine, axis, ghost, align=align), FieldLayout.face(nd, coarse, axis, ghost + 1, align=align)
        cb, ce = lc.loop_box()
        fb, fe = lf.loop_box()
        ib, ie = list(cb), list(ce)
        ib[axis], ie[axis] = 1, ce[axis] - 1              # interior faces only
        sb = [min(1, ce[d] - 1) if d < nd else 0 for d in range(3)]
        for b, e in ((cb, ce), (ib, ie), (sb, ce)):
            rf, fc = ops.new_array(lf.size), ops.new_array(lc.size)
            ops.fill_random(rf, 31 + axis)
            ops.fill_random(fc, 41 + axis)
            ops.restrict_face(axis, lf.c_struct(), rf, lc.c_struct(), fc, 0.3, b, e)
            out.append([rf, fc])
        pb = [min(1, fe[d] - 1) if d < nd else 0 for d in range(3)]
        gb, ge = list(fb), list(fe)
        for d in range(nd):
            if d != axis:
                gb[d], ge[d] = -1, fe[d] + 1                  # the ghost cells beside the block: floor(-1 / 2) = -1
        for b, e in ((fb, fe), (pb, fe), (gb, ge)):
            uc, uf = ops.new_array(lc.size), ops.new_array(lf.size)
            ops.fill_random(uc, 51 + axis)
            ops.fill_random(uf, 61 + axis)
            ops.prolong_add_face(axis, lc.c_struct(), uc, lf.c_struct(), uf, b, e)
            out.append([uc, uf])
    return out


@pytest.mark.parametrize("nd,cells,ghost,align", CASES, ids=IDS)
def test_face_transfers_bitwise(hip, orc, nd, cells, ghost, align):
    compare(hip, orc, lambda ops: transfers(ops, nd, cells, ghost, align), "face transfers")


# -- boundary rules and expressions ----------------------------------------------------------------------------------------------------------
def _geom():
    g = GeomC()
    for d in range(3):
        g.pos_begin[d], g.h[d] = (0.25, -0.5, 1.0)[d], H[d]
    return g


# additions, subtractions and products only: the C library and the device round them alike
POLY = ExprC.from_program([("x", None), ("const", 3.0), ("*", None), ("y", None), ("y", None), ("*", None), ("+", None), ("z", None),
                           ("const", 7.0), ("*", None), ("-", None), ("const", 1.0), ("+", None)])


def boundary(ops, nd, cells, ghost, align):
    out = []
    for axis in range(nd):
        l = FieldLayout.face(nd, cells, axis, ghost, align=align)
        for kind in (BC_DIRICHLET, BC_NEUMANN):
            walls = [(d, s) for d in range(nd) for s in (0, 1) if kind == BC_DIRICHLET or d != axis]
            for mask in [1 << (2 * d + s) for d, s in walls] + [sum(1 << (2 * d + s) for d, s in walls)]:
                x = ops.new_array(l.size)
                ops.fill_random(x, 71 + axis)
                ops.apply_bc_face(axis, l.c_struct(), x, _geom(), kind, POLY if kind == BC_DIRICHLET else None, mask)
                out.append([x])
        b, e = l.loop_box()
        x, m = ops.new_array(l.size), ops.new_scalar()
        ops.fill_random(x, 81)
        ops.fill_expr_face(axis, l.c_struct(), x, _geom(), POLY, [1 if d < nd else 0 for d in range(3)], e)
        ops.max_err_expr_face(axis, l.c_struct(), x, _geom(), POLY, b, e, out=m)
        out.append([x, m])
    return out


@pytest.mark.parametrize("nd,cells,ghost,align", [c for c in CASES if c[1] in ((6, 3), (201, 6), (6, 3, 6), (69, 6, 3))],
                         ids=[i for c, i in zip(CASES, IDS) if c[1] in ((6, 3), (201, 6), (6, 3, 6), (69, 6, 3))])
def test_boundary_rules_and_face_expressions_bitwise(hip, orc, nd, cells, ghost, align):
    compare(hip, orc, lambda ops: boundary(ops, nd, cells, ghost, align), "apply_bc_face / fill / max_err")


# -- refusals ----------------------------------------------------------------------------------------------------------------------------
def _refusals():
    nd, cells = 2, (6, 3)
    col = next(colouring(nd).colours())
    face0, face1, cell = FieldLayout.face(nd, cells, 0, 1), FieldLayout.face(nd, cells, 1, 1), FieldLayout.cell(nd, cells, 1)
    bad_rem = _Raw(col.c_struct())
    bad_rem.c.rem[0] = 3
    bad_mod = _Raw(col.c_struct())
    bad_mod.c.mod[1] = 0
    star = lambda offs: Stencil(offs, [20.0 + k for k in range(len(offs))])
    return [
        ("nd = 1", dict(nd=1), "2-D or 3-D", "both"),
        ("nd = 4", dict(nd=4), "2-D or 3-D", "both"),
        ("pressure in a node layout", dict(lp=FieldLayout.node(nd, cells, 1)), "pressure layout is not a cell layout", "both"),
        ("u_0 in the layout of u_1", dict(lu=[face1, face1]), "u_0 layout is not a face layout of axis 0", "both"),
        ("u_1 in a cell layout", dict(lu=[face0, cell]), "u_1 layout is not a face layout of axis 1", "both"),
        ("rhs of the pressure in a face layout", dict(lfp=FieldLayout.face(nd, cells, 0, 0)), "rhs 2 layout is not a cell layout", "both"),
        ("dst in a 3-D layout", dict(ld=[FieldLayout.face(3, (6, 3, 2), 0, 1), face1]), "dst 0 layout has 3 dimensions", "op"),
        ("colour-split pressure", dict(lp=cell.split_x()), "layout transformation", "both"),
        ("unequal cell counts", dict(lu=[FieldLayout.face(nd, (5, 3), 0, 1), face1]), "has 5 cells in dim 0, the pressure 6", "both"),
        ("pressure without ghost layer", dict(lp=FieldLayout.cell(nd, cells, 0)), "the pressure has no ghost layer", "both"),
        ("u_1 without ghost layer", dict(lu=[face0, FieldLayout.face(nd, cells, 1, 0)]), "u_1 has no ghost layer", "both"),
        ("reach 2", dict(A0=star([(0, 0, 0), (2, 0, 0)])), "not the centre or an axis neighbour at distance 1", "both"),
        ("an entry off the axes", dict(A0=star([(0, 0, 0), (1, 1, 0)])), "not the centre or an axis neighbour", "both"),
        ("an entry off the layout's axes", dict(A0=star([(0, 0, 0), (0, 0, 1)])), "not the centre or an axis neighbour", "both"),
        ("repeated offset", dict(A0=star([(0, 0, 0), (1, 0, 0), (1, 0, 0)])), "repeats the offset", "both"),
        ("no centre", dict(A0=star([(1, 0, 0), (-1, 0, 0)])), "has no centre entry", "both"),
        ("stencil field", dict(A0="field"), "is a stencil field", "both"),
        ("zero determinant", dict(A0=Stencil([(0, 0, 0), (1, 0, 0), (-1, 0, 0)], [1.0, 1.0, 1.0])), "determinant zero", "relax"),
        ("dst is an unknown", dict(alias="u"), "destination 0 is unknown 0", "op"),
        ("dst is a right-hand side", dict(alias="f"), "destination 0 is right-hand side 0", "op"),
        ("two dst are one", dict(alias="dst"), "destinations 0 and 1 are one array", "op"),
        ("shell leaves u_0", dict(rb=[[-1, 0, 0], [0, 0, 0], [0, 0, 0]]), "leaves the allocation of u_0", "op"),
        ("gradient leaves the pressure", dict(rb=[[0, 0, 0], [0, -1, 0], [0, 0, 0]], lu=[face0, FieldLayout.face(nd, cells, 1, 3)]),
         "leaves the allocation of the pressure", "op"),
        ("divergence leaves u_0", dict(re=[[7, 3, 1], [6, 4, 1], [8, 3, 1]]), "divergence leaves the allocation of u_0", "op"),
        ("box leaves the dst", dict(ldp=FieldLayout.cell(nd, cells, 0), rb=[[0, 0, 0], [0, 0, 0], [0, -1, 0]]), "row 2: box leaves the dst allocation", "op"),
        ("box leaves the rhs", dict(lfp=FieldLayout.cell(nd, cells, 0), rb=[[0, 0, 0], [0, 0, 0], [0, -1, 0]]), "row 2: box leaves the rhs allocation", "op"),
        ("box leaves the cells", dict(e=[7, 3, 1]), "leaves the cells", "relax"),
        ("negative cells", dict(b=[-1, 0, 0]), "leaves the cells", "relax"),
        ("parity of all indices", dict(col=next(parity(nd).colours())), r"does not decouple the boxes: cells i and i \+ \(-1, -1, 0\)", "relax"),
        ("axis parities", dict(col=next(Colouring.axis_parity(nd).colours())), r"cells i and i \+ \(-2, 0, 0\)", "relax"),
        ("one expression only", dict(col=next(Colouring((((0,), 0, 3),)).colours())), r"cells i and i \+ \(0, -1, 0\)", "relax"),
        ("not one expression per axis", dict(col=next(Colouring((((0,), 0, 3), ((0, 1), 0, 3))).colours())), "one expression", "relax"),
        ("rem outside [0, mod)", dict(col=bad_rem), "rem must lie", "relax"),
        ("mod 0", dict(col=bad_mod), "mod must be positive", "relax"),
        ("negative colour expression", dict(col=Colouring((((0,), -5, 3), ((1,), 0, 3)), (0, 0)), b=[1, 0, 0]), "can be negative", "relax"),
    ]


class _Raw:
    """A colouring struct the value type would not build."""

    def __init__(self, c):
        self.c = c

    def c_struct(self):
        return self.c


REFUSALS = [(name, args, text, entry) for name, args, text, which in _refusals() for entry in ("op", "relax", "sweep")
            if which == "both" and entry != "sweep" or which == entry or (which == "relax" and entry == "sweep" and "rem" not in name)]


@pytest.mark.parametrize("name,args,text,entry", REFUSALS, ids=["%s-%s" % (r[3], r[0].replace(" ", "-")) for r in REFUSALS])
def test_refusals_launch_nothing(hip, name, args, text, entry):
    """Each refusal returns its error through examg_last_error and leaves every array as it was."""
    nd, cells = 2, (6, 3)
    D = MacData(hip, nd, cells, ghost=3)      # allocations large enough for every layout of the table
    y = D.sys
    arrs = D.arrays()
    before = [hip.to_host(a).copy() for a in arrs]
    rb, re = row_boxes(nd, cells, boxes(nd, cells)["whole"])
    b, e = boxes(nd, cells)["whole"]
    one = FieldLayout.face(nd, cells, 0, 1), FieldLayout.face(nd, cells, 1, 1), FieldLayout.cell(nd, cells, 1)
    y.lu, y.lp, y.lf, y.lfp, y.ld, y.ldp = [one[0], one[1]], one[2], [one[0], one[1]], one[2], [one[0], one[1]], one[2]
    col = next(colouring(nd).colours())
    for k, v in args.items():
        if k == "A0":
            y.A = [Stencil([(0, 0, 0)], [1.0], cfield=y.u[0], clayout=one[0]) if v == "field" else v, y.A[1]]
        elif k == "alias":
            y.dst = [y.u[0] if v == "u" else (y.f[0] if v == "f" else y.dst[0]), y.dst[0] if v == "dst" else y.dst[1]]
        elif k == "rb":
            rb = v
        elif k == "re":
            re = v
        elif k == "b":
            b = v
        elif k == "e":
            e = v
        elif k == "col":
            col = v
        else:
            setattr(y, k, v)
    with pytest.raises(ExamgError, match=text):
        if entry == "op":
            hip.mac_op(SYS_RESIDUAL, y, 7, rb, re)
        elif entry == "relax":
            hip.mac_relax(y, 0.8, col, b, e)
        else:
            hip.mac_sweep(y, 0.8, col, b, e)
    hip.synchronize()
    for k, a in enumerate(arrs):
        same(hip.to_host(a), before[k], "array %d after the refused call" % k)


@pytest.mark.parametrize("entry", ["relax", "sweep"])
@pytest.mark.parametrize("nd", [2, 3])
def test_a_block_of_one_cell_has_no_schur_complement(hip, nd, entry):
    """All 2 * nd faces of the one cell lie on the boundary and are held: the pressure's Schur complement is zero for constant input, and
    the smoother refuses before anything is launched."""
    cells = (1,) * nd
    D = MacData(hip, nd, cells)
    before = [hip.to_host(a).copy() for a in D.arrays()]
    b, e = boxes(nd, cells)["whole"]
    with pytest.raises(ExamgError, match="examg_mac_%s: the Schur complement of a cell's pressure is zero" % entry):
        if entry == "relax":
            hip.mac_relax(D.sys, 0.8, next(colouring(nd).colours()), b, e)
        else:
            hip.mac_sweep(D.sys, 0.8, colouring(nd), b, e)
    hip.synchronize()
    for k, a in enumerate(D.arrays()):
        same(hip.to_host(a), before[k], "array %d after the refused call" % k)


def test_complex_and_vector_layouts_are_refused_before_the_library(hip):
    """The C struct cannot carry the element kind: the kernel layer refuses such a system itself, whatever the entry point."""
    nd, cells = 2, (6, 3)
    D = MacData(hip, nd, cells)
    before = [hip.to_host(a).copy() for a in D.arrays()]
    rb, re = row_boxes(nd, cells, boxes(nd, cells)["whole"])
    b, e = boxes(nd, cells)["whole"]
    for attr, lay, text in (("lp", FieldLayout.cell(nd, cells, 1).as_vector(2), "vector-valued"),
                            ("lfp", FieldLayout.node(nd, cells, 1).as_complex(), "complex")):
        keep = getattr(D.sys, attr)
        setattr(D.sys, attr, lay)
        with pytest.raises(ValueError, match="examg_mac_op: the .* layout is %s" % text):
            hip.mac_op(SYS_RESIDUAL, D.sys, 7, rb, re)
        with pytest.raises(ValueError, match="examg_mac_sweep: the .* layout is %s" % text):
            hip.mac_sweep(D.sys, 0.8, colouring(nd), b, e)
        setattr(D.sys, attr, keep)
    hip.synchronize()
    for k, a in enumerate(D.arrays()):
        same(hip.to_host(a), before[k], "array %d after the refused calls" % k)


def test_single_field_refusals_launch_nothing(hip):
    nd, cells = 2, (6, 3)
    lf, lc = FieldLayout.face(nd, (12, 6), 0, 1), FieldLayout.face(nd, cells, 0, 1)
    node, other = FieldLayout.node(nd, cells, 1), FieldLayout.face(nd, cells, 1, 1)
    f, c = hip.new_array(lf.size), hip.new_array(lf.size)
    hip.fill_random(f, 5)
    hip.fill_random(c, 6)
    before = [hip.to_host(f).copy(), hip.to_host(c).copy()]
    cb, ce = lc.loop_box()
    fb, fe = lf.loop_box()
    g = _geom()
    calls = [
        (lambda: hip.restrict_face(0, lf.c_struct(), f, node.c_struct(), c, 1.0, cb, ce), "coarse layout is not a face layout of axis 0"),
        (lambda: hip.restrict_face(0, lf.c_struct(), f, other.c_struct(), c, 1.0, cb, ce), "coarse layout is not a face layout of axis 0"),
        (lambda: hip.restrict_face(2, lf.c_struct(), f, lc.c_struct(), c, 1.0, cb, ce), "axis 2 of a 2-D face field"),
        (lambda: hip.restrict_face(0, lf.c_struct(), f, lc.c_struct(), c, 1.0, [-1, 0, 0], ce), "box leaves an allocation"),
        (lambda: hip.restrict_face(0, lf.c_struct(), f, lc.c_struct(), c, 1.0, cb, [ce[0] + 1, ce[1], 1]), "box leaves an allocation"),
        (lambda: hip.restrict_face(0, lf.c_struct(), f, lc.c_struct(), f, 1.0, cb, ce), "the two arrays are one"),
        (lambda: hip.restrict_face(0, lf.split_x().c_struct(), f, lc.c_struct(), c, 1.0, cb, ce), "layout transformation"),
        (lambda: hip.restrict_face(0, lf.c_struct(), f, FieldLayout.face(3, (6, 3, 2), 0, 1).c_struct(), c, 1.0, cb, ce), "one dimensionality"),
        (lambda: hip.prolong_add_face(0, lc.c_struct(), c, lf.c_struct(), f, [-1, 0, 0], fe), "negative index on the field's own axis"),
        (lambda: hip.prolong_add_face(0, lc.c_struct(), c, lf.c_struct(), f, fb, [fe[0], fe[1] + 2, 1]), "box leaves an allocation"),
        (lambda: hip.prolong_add_face(0, lc.c_struct(), c, node.c_struct(), f, fb, fe), "fine layout is not a face layout"),
        (lambda: hip.prolong_add_face(0, lc.c_struct(), f, lf.c_struct(), f, fb, fe), "the two arrays are one"),
        (lambda: hip.apply_bc_face(0, lc.c_struct(), c, g, BC_NEUMANN, None, 1), "Neumann wall normal"),
        (lambda: hip.apply_bc_face(0, lc.c_struct(), c, g, 2, None, 4), "kind 2"),
        (lambda: hip.apply_bc_face(0, other.c_struct(), c, g, BC_NEUMANN, None, 4), "not a face layout of axis 0"),
        (lambda: hip.apply_bc_face(0, FieldLayout.face(nd, cells, 0, 0).c_struct(), c, g, BC_NEUMANN, None, 4), "has no ghost layer"),
        (lambda: hip.fill_expr_face(1, lc.c_struct(), c, g, POLY, cb, ce), "not a face layout of axis 1"),
        (lambda: hip.max_err_expr_face(0, node.c_struct(), c, g, POLY, cb, ce), "not a face layout of axis 0"),
        (lambda: hip.fill_expr_face(0, lc.c_struct(), c, g, POLY, [-2, 0, 0], ce), "box leaves the allocation"),
    ]
    for call, text in calls:
        with pytest.raises(ExamgError, match=text):
            call()
    hip.synchronize()
    same(hip.to_host(f), before[0], "fine array after the refused calls")
    same(hip.to_host(c), before[1], "coarse array after the refused calls")


# -- the Stokes driver on the HIP kernels ------------------------------------------------------------------------------------------------
from exastencils_amd.stokes import ConfigStokes, StokesSolver  # noqa: E402


@pytest.mark.parametrize("nd,hi", [(2, 3), (3, 2)])
def test_fields_after_one_cycle_equal_the_restatement(hip, orc, nd, hi):
    """Every kernel of the cycle is point-wise: after the residual, one V-cycle and the residual again, every array of every level has the
    restatement's bits.  On the polynomial problem, whose programs hold additions, subtractions and products only (the two layers' sin and
    cos need not round alike, and `apply bc` evaluates the boundary program after every colour)."""
    G, C = (StokesSolver(ops, ConfigStokes(nd=nd, max_level=hi, problem="polynomial")) for ops in (hip, orc))
    for S in (G, C):
        S.UpdateRes(hi)
        S.mgCycle(hi)
        S.UpdateRes(hi)
    hip.synchronize()
    for k, (x, y) in enumerate(zip(G.arrays(), C.arrays())):
        same(hip.to_host(x), orc.to_host(y), "array %d" % k)


@pytest.mark.parametrize("nd,hi", [(2, 3), (3, 2)])
def test_a_replayed_cycle_equals_the_eager_one(hip, nd, hi):
    E, R = (StokesSolver(hip, ConfigStokes(nd=nd, max_level=hi)) for _ in range(2))
    E.mgCycle(hi)
    E.mgCycle(hi)
    R.capture_cycle()      # records only: R's fields are still the start values
    R.replay_cycle()
    R.replay_cycle()
    hip.synchronize()
    for k, (x, y) in enumerate(zip(E.arrays(), R.arrays())):
        same(hip.to_host(x), hip.to_host(y), "array %d" % k)


@pytest.mark.parametrize("nd,hi", [(2, 5), (3, 3)])
def test_solve_prints_the_golden(hip, nd, hi):
    """96^2 and 24^3 cells: the lines of the restatement's run, four digits each; eager, then from the graph."""
    with open(os.path.join(ROOT, "tests", "golden", "own", "stokes%dd.results" % nd)) as f:
        golden = f.read()
    S = StokesSolver(hip, ConfigStokes(nd=nd, max_level=hi))
    S.Solve()
    assert "\n".join(S.log) + "\n" == golden
    assert S.iterations <= 30 and S.res_history[-1] <= 1e-10 * S.res_history[0]
    S.setup()
    S.Solve(use_graph=True)
    assert "\n".join(S.log) + "\n" == golden
