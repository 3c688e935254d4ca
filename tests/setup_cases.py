"""Cases and references for the kernels that turn an index into a position (test helper, no test functions): the stencil-field
initialisers examg_init_varcoeff7 / examg_init_helmholtz27, `apply bc` of cell, vector-valued cell and face fields, the point
expressions of every localization (examg_fill_expr* / examg_max_err_expr*) and the three _grid entry points.

Nothing here shares code with the library, the C oracle or the numpy restatements cell_ops / mac_ops / flux_ops / grid_ops: every
reference is written from the text of include/examg.h.  From blas_cases come the program syntax, the geometry struct, the views of whole
allocations and the exact positions.  tests/test_setup_exact.py pins the references (against the oracle, the older restatements and each
other) before tests/test_gpu_setup.py lets them judge the library.

Two classes of reference, as in blas_cases:
  exact    dyadic geometry (pos_begin of both signs, another power of two per axis as mesh width), programs over + - * and division by
           powers of two with dyadic literals, fields of small integers.  The reference is Fraction arithmetic; every value it stores
           is asserted to be an fp64 number, so a correct implementation returns it in any order of evaluation: np.array_equal.
           The one exception is examg_init_helmholtz27, which rounds in exactly one place, S * kf with kf = 1.0 / 3.0 or -1.0 / 12.0
           (neither is dyadic): the reference takes float(Fraction(S) * Fraction(kf)) -- the IEEE product of the two fp64 numbers --
           and asserts that / (h * h) (a power of two) and - ksq (dyadic) are exact.
  rounded  mesh widths 1/7, 1/5, 1/3, pos_begin not dyadic, a rational coefficient program (no libm).  The reference is numpy, one
           IEEE operation per numpy operation in the order the header gives: compared bit for bit.

Every reference returns the WHOLE allocation as it has to be afterwards: SENTINEL (or the start field, where the entry point reads
it) at every double the entry point may not write -- pads, ghost layers outside the box, edge and corner ghosts, the planes behind
the last entry of a stencil field, the doubles behind the last component of a vector field.
"""
import itertools
import operator
from collections import namedtuple
from fractions import Fraction
from functools import lru_cache

import numpy as np

import blas_cases as B
import stencil_cases as S
from blas_cases import SENTINEL, box_index, geometry, positions, prog, view

from exastencils_amd.layout import FieldLayout

DIRICHLET, NEUMANN, NEGATE = 0, 1, 2          # EXAMG_BC_* of include/examg.h
LOCS = ("node", "cell", "face_x", "face_y", "face_z")


# ---- programs ---------------------------------------------------------------------------------------------------------------------------
def gprog(text):
    """blas_cases.prog plus the width operands wx wy wz of the _grid entry points."""
    out = []
    for w in text.split():
        out += [(w, None)] if w in ("wx", "wy", "wz") else prog(w)
    return out


_BIN = {"+": operator.add, "-": operator.sub, "*": operator.mul, "/": operator.truediv}


def run_program(program, operands, const):
    """The postfix program on any number type: the operand pushed first is the left one; one operation per instruction."""
    st = []
    for name, c in program:
        if name == "const":
            st.append(const(c))
        elif name in operands:
            st.append(operands[name])
        elif name == "neg":
            st[-1] = -st[-1]
        else:
            r = st.pop()
            st[-1] = _BIN[name](st[-1], r)
    assert len(st) == 1
    return st[0]


def frac_fn(program):
    return lambda x, y, z, **w: run_program(program, dict(x=x, y=y, z=z, **w), Fraction)


def np_fn(program):
    def f(x, y, z, **w):
        with np.errstate(all="ignore"):
            r = run_program(program, dict(x=x, y=y, z=z, **w), np.float64)
        return np.broadcast_to(r, np.broadcast(x, y, z).shape).copy()          # a program may leave an axis out: the shape of the box
    return f


def fp64(v):
    """The Fraction v as a float; it must be one."""
    f = v.numerator / v.denominator
    assert Fraction(f) == v, "not exact in fp64: %r" % (v,)
    return f


def is_pow2(v):
    v = Fraction(v)
    return v > 0 and (v.numerator == 1 and v.denominator & (v.denominator - 1) == 0 or v.denominator == 1 and v.numerator & (v.numerator - 1) == 0)


def rounded_positions(geom, b, e, loc="node"):
    """Per dimension index * h + pos_begin (then + 0.5 * h off the own axes), each operation rounded, as (z, y, x)-broadcastable arrays."""
    own = {"node": (0, 1, 2), "cell": (), "face_x": (0,), "face_y": (1,), "face_z": (2,)}[loc]
    out = []
    for d in range(3):
        shape = [1, 1, 1]
        shape[2 - d] = e[d] - b[d]
        p = np.arange(b[d], e[d]).astype(np.float64) * np.float64(geom.h[d]) + np.float64(geom.pos_begin[d])
        if d not in own:
            p = p + np.float64(0.5) * np.float64(geom.h[d])
        out.append(p.reshape(shape))
    return out


def points(b, e):
    """(i0, i1, i2) of the box, x fastest."""
    return [(i0, i1, i2) for i2 in range(b[2], e[2]) for i1 in range(b[1], e[1]) for i0 in range(b[0], e[0])]


def at(l, i):
    """numpy index of the iterator point i in view(l, .)."""
    return (i[2] + l.ref(2), i[1] + l.ref(1), i[0] + l.ref(0))


def ghost_box(l):
    """GLB..GRE: the allocation without its pads."""
    return (tuple(l.idx("GLB", d) if d < l.nd else 0 for d in range(3)), tuple(l.idx("GRE", d) if d < l.nd else 1 for d in range(3)))


def differing(got, want):
    """None, or a message with the number of differing doubles (bit patterns) and the first few indices."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    bad = bad[(got[bad] != want[bad]) | np.isnan(got[bad]) | np.isnan(want[bad])]          # -0.0 and 0.0 count as equal
    if bad.size == 0:
        return None
    return "%d of %d doubles differ; first at %s: got %s, want %s" % (bad.size, got.size, bad[:6].tolist(), got[bad[:6]].tolist(), want[bad[:6]].tolist())


# ---- geometries and coefficient programs ------------------------------------------------------------------------------------------------
EGEOM = geometry((-0.75, 0.5, -0.25), (0.125, 0.25, 0.5))                 # exact class: another power of two per axis
EGEOM_EQ = geometry((-0.75, 0.5, -0.25), (0.25, 0.25, 0.25))              # ... with equal widths (examg_init_helmholtz27)
RGEOM = geometry((0.1, -0.3, 0.7), (1.0 / 7.0, 1.0 / 5.0, 1.0 / 3.0))     # rounded class
RGEOM_EQ = geometry((0.1, -0.3, 0.7), (1.0 / 7.0, 1.0 / 7.0, 1.0 / 7.0))
# 1 + x/2 + (y/4) * x + (z*z)/8: every axis, and both signs of a half step, change the value
ECOEF = prog("1 x 2 / + y 4 / x * + z z * 8 / +")
# (1 + x*y) / (2 + z*z) + x / (3 + y*y): rational, no libm
RCOEF = prog("1 x y * + 2 z z * + / x 3 y y * + / +")
# ECOEF with the constant 3, for examg_init_helmholtz27: the centre entry stays above ksq in magnitude, so that `- ksq` is exact
HCOEF = prog("3 x 2 / + y 4 / x * + z z * 8 / +")
KSQ = 2.5


# ---- examg_init_varcoeff7 ---------------------------------------------------------------------------------------------------------------
def exact_varcoeff7(lc, start, geom, program, b, e):
    """include/examg.h: entry 0 = the sum over d of (ap_d + am_d) / (h_d * h_d), entry 1 + 2d = (-1 * ap_d) / (h_d * h_d), entry 2 + 2d =
    (-1 * am_d) / (h_d * h_d), ap_d / am_d = a(position +- h_d / 2 in d), position = index * h + pos_begin on all three axes (in 2-D
    z = pos_begin[2]); planes of size(lc) doubles."""
    a, nd, out = frac_fn(program), lc.nd, start.copy()
    h, pb = [Fraction(geom.h[d]) for d in range(3)], [Fraction(geom.pos_begin[d]) for d in range(3)]
    planes = [view(lc, out[k * lc.size:(k + 1) * lc.size]) for k in range(2 * nd + 1)]
    for i in points(b, e):
        p = [i[d] * h[d] + pb[d] for d in range(3)]
        centre = Fraction(0)
        for d in range(nd):
            up, dn = list(p), list(p)
            up[d], dn[d] = p[d] + h[d] / 2, p[d] - h[d] / 2
            ap, am = a(*up), a(*dn)
            centre += (ap + am) / (h[d] * h[d])
            planes[1 + 2 * d][at(lc, i)] = fp64(-ap / (h[d] * h[d]))
            planes[2 + 2 * d][at(lc, i)] = fp64(-am / (h[d] * h[d]))
        planes[0][at(lc, i)] = fp64(centre)
    return out


def rounded_varcoeff7(lc, start, geom, program, b, e):
    """The same in fp64, one rounding per operation, in the order of the header's formulas."""
    a, nd, out = np_fn(program), lc.nd, start.copy()
    planes = [view(lc, out[k * lc.size:(k + 1) * lc.size]) for k in range(2 * nd + 1)]
    if B.empty(b, e):
        return out
    p = rounded_positions(geom, b, e)
    s, centre = box_index(lc, b, e), None
    for d in range(nd):
        h = np.float64(geom.h[d])
        up, dn = list(p), list(p)
        up[d], dn[d] = p[d] + (np.float64(0.5) * h), p[d] - (np.float64(0.5) * h)
        ap, am = a(*up), a(*dn)
        t = (ap + am) / (h * h)
        centre = t if centre is None else centre + t
        planes[1 + 2 * d][s] = (np.float64(-1.0) * ap) / (h * h)
        planes[2 + 2 * d][s] = (np.float64(-1.0) * am) / (h * h)
    planes[0][s] = centre
    return out


# ---- examg_init_helmholtz27 -------------------------------------------------------------------------------------------------------------
H27_ENTRIES = [(0, 0, 0)] + [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
H27_SIDES = list(itertools.product((0, 1), repeat=3))          # (sx, sy, sz): the x side outermost, the lower side first


def _h27_elements(off):
    """The elements that hold the node and its neighbour at `off`: those on the side of every non-zero component."""
    return [s for s in H27_SIDES if all(off[d] == 0 or (off[d] > 0) == (s[d] == 1) for d in range(3))]


def _h27_kf(off):
    nnz = sum(1 for o in off if o != 0)
    return 1.0 / 3.0 if nnz == 0 else (0.0 if nnz == 1 else -1.0 / 12.0)


def exact_helmholtz27(lc, start, geom, program, ksq, b, e):
    """include/examg.h: entry (dx, dy, dz) = (S * kf) / (h * h), S the sum of a(element centre) over the elements that hold both nodes;
    the centre entry then has ksq subtracted.  The one inexact step is S * kf."""
    assert geom.h[0] == geom.h[1] == geom.h[2]
    a, out = frac_fn(program), start.copy()
    h, pb = Fraction(geom.h[0]), [Fraction(geom.pos_begin[d]) for d in range(3)]
    assert is_pow2(h * h)
    planes = [view(lc, out[k * lc.size:(k + 1) * lc.size]) for k in range(27)]
    for i in points(b, e):
        p = [i[d] * h + pb[d] for d in range(3)]
        ae = {s: a(*[p[d] + (h / 2 if s[d] else -h / 2) for d in range(3)]) for s in H27_SIDES}
        for k, off in enumerate(H27_ENTRIES):
            ssum = fp64(sum(ae[s] for s in _h27_elements(off)))
            prod = float(Fraction(ssum) * Fraction(_h27_kf(off)))          # the correctly rounded product of two fp64 numbers
            c = Fraction(prod) / (h * h)
            fp64(c)                                                         # a power of two: exact
            if k == 0:
                c = c - Fraction(ksq)
            planes[k][at(lc, i)] = fp64(c)                                  # dyadic ksq: exact
    return out


def rounded_helmholtz27(lc, start, geom, program, ksq, b, e):
    a, out = np_fn(program), start.copy()
    planes = [view(lc, out[k * lc.size:(k + 1) * lc.size]) for k in range(27)]
    if B.empty(b, e):
        return out
    h = np.float64(geom.h[0])
    p = rounded_positions(geom, b, e)
    ae = {s: a(*[p[d] + np.float64(0.5 if s[d] else -0.5) * h for d in range(3)]) for s in H27_SIDES}
    sl = box_index(lc, b, e)
    for k, off in enumerate(H27_ENTRIES):
        ssum = None
        for s in _h27_elements(off):
            ssum = ae[s] if ssum is None else ssum + ae[s]
        c = (ssum * np.float64(_h27_kf(off))) / (h * h)
        planes[k][sl] = c - np.float64(ksq) if k == 0 else c
    return out


# layouts and boxes of the initialisers
InitCase = namedtuple("InitCase", "name layout box nalloc")


def _init_cases(cells3, with2d):
    g1 = FieldLayout.node(3, cells3, 1, align=2)
    plain = FieldLayout.node(3, cells3, 0)
    K = 7 if with2d else 27
    out = [InitCase("loop_box", g1, (tuple(g1.loop_box()[0]), tuple(g1.loop_box()[1])), K),
           InitCase("sub_box", g1, ((2, 1, 1), (cells3[0] - 1, cells3[1] - 1, cells3[2] - 1)), K),
           InitCase("into_ghost", g1, ((-1, -1, -1), ghost_box(g1)[1]), K),
           InitCase("plain_layout", plain, (tuple(plain.loop_box()[0]), tuple(plain.loop_box()[1])), K)]
    if with2d:
        l2 = FieldLayout.node(2, (11, 5, 0), 1, align=2)
        out += [InitCase("2d_loop_box", l2, (tuple(l2.loop_box()[0]), tuple(l2.loop_box()[1])), 7),        # planes 5 and 6 stay untouched
                InitCase("2d_into_ghost", l2, ((-1, -1, 0), ghost_box(l2)[1]), 7)]
    assert any(l.layout.pad_l[0] + l.layout.pad_r[0] > 0 for l in out)
    return out


VARCOEFF_CASES = _init_cases((9, 6, 4), True)
assert VARCOEFF_CASES[1].box == ((2, 1, 1), (8, 5, 3))
HELMHOLTZ_CASES = _init_cases((7, 5, 4), False)
INIT_CLASSES = {"exact": (EGEOM, EGEOM_EQ, ECOEF, HCOEF), "rounded": (RGEOM, RGEOM_EQ, RCOEF, RCOEF)}


def init_start(case):
    return np.full(case.nalloc * case.layout.size, SENTINEL)


@lru_cache(maxsize=None)
def varcoeff_reference(name, cls):
    case = next(c for c in VARCOEFF_CASES if c.name == name)
    geom, _, coef, _ = INIT_CLASSES[cls]
    out = (exact_varcoeff7 if cls == "exact" else rounded_varcoeff7)(case.layout, init_start(case), geom, coef, *case.box)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def helmholtz_reference(name, cls):
    case = next(c for c in HELMHOLTZ_CASES if c.name == name)
    _, geom, _, coef = INIT_CLASSES[cls]
    out = (exact_helmholtz27 if cls == "exact" else rounded_helmholtz27)(case.layout, init_start(case), geom, coef, KSQ, *case.box)
    out.setflags(write=False)
    return out


def split_planes(l, plain, nplanes):
    """`nplanes` planes of the plain layout l, each as l.split_x() holds it."""
    return np.concatenate([B.ref_split(l, plain[k * l.size:(k + 1) * l.size]) for k in range(nplanes)])


# ---- examg_apply_bc_cell ----------------------------------------------------------------------------------------------------------------
def exact_bc_cell(l, start, geom, kind, program, mask):
    """include/examg.h: per face of the mask the ghost one step outwards of every cell of the boundary row, tangentially [0, inner);
    Dirichlet (2 * g(face centre)) - interior, Neumann interior, negate -interior; the face centre is the cell centre tangentially and
    idx * h + pos_begin on the normal, idx = 0 below and inner above."""
    out, src = start.copy(), view(l, start)
    dst = view(l, out)
    g = frac_fn(program) if kind == DIRICHLET else None
    h, pb = [Fraction(geom.h[d]) for d in range(3)], [Fraction(geom.pos_begin[d]) for d in range(3)]
    for d in range(l.nd):
        for side in (0, 1):
            if not mask & (1 << (2 * d + side)):
                continue
            b = [0, 0, 0]
            e = [l.inner[t] if t < l.nd else 1 for t in range(3)]
            if side:
                b[d] = l.inner[d] - 1
            else:
                e[d] = 1
            for i in points(b, e):
                interior = Fraction(float(src[at(l, i)]))
                o = list(i)
                o[d] += 1 if side else -1
                if kind == NEUMANN:
                    v = interior
                elif kind == NEGATE:
                    v = -interior
                else:
                    p = [(i[t] * h[t] + pb[t]) + h[t] / 2 for t in range(3)]
                    p[d] = (l.inner[d] if side else 0) * h[d] + pb[d]
                    v = 2 * g(*p) - interior
                dst[at(l, o)] = fp64(v)
    return out


BC_PROGRAM = prog("x y * z 2 / + 0.75 -")                 # depends on all three coordinates
BC_LAYOUTS = {
    "5x4x3_g1": FieldLayout.cell(3, (5, 4, 3), 1),
    "5x4x3_g2_a2": FieldLayout.cell(3, (5, 4, 3), 2, align=2),           # only the first ghost layer changes
    "6x1x3_g1": FieldLayout.cell(3, (6, 1, 3), 1),                       # one cell: the boundary row of both y faces
    "2d_7x3_g1_a2": FieldLayout.cell(2, (7, 3), 1, align=2),
    "2d_1x1_g1": FieldLayout.cell(2, (1, 1), 1),
}


def bc_masks(nd):
    full = (1 << (2 * nd)) - 1
    return [1 << f for f in range(2 * nd)] + [full, 0b100110 & full, 0]


BC_CASES = [(ln, kind, m) for ln, l in BC_LAYOUTS.items() for kind in (DIRICHLET, NEUMANN, NEGATE) for m in bc_masks(l.nd)]


def bc_start(l, tail=0, ncomp=1):
    """Small integers over the whole allocation(s), `tail` SENTINELs behind."""
    return np.concatenate([S.int_field(ncomp * l.size, 41 + l.size), np.full(tail, SENTINEL)])


@lru_cache(maxsize=None)
def bc_cell_reference(lname, kind, mask):
    l = BC_LAYOUTS[lname]
    out = exact_bc_cell(l, bc_start(l), EGEOM, kind, BC_PROGRAM, mask)
    out.setflags(write=False)
    return out


# more boundary cells than the 2048 x 256 threads of the launch: the grid-stride loop of k_apply_bc_cell
CAP_LAYOUT = FieldLayout.cell(2, (262200, 2), 1)
CAP_MASK = 0b1100
CAP_GEOM = geometry((-64.0, -0.5, 0.25), (2.0 ** -9, 0.5, 0.5))
CAP_PROGRAM = prog("x y * z +")
CAP_THREADS = 2048 * 256


def cap_reference():
    """(start, afterwards) of the Dirichlet walls y = 0 and y = 2 cells: integer arithmetic in units of 2^-11, vectorised."""
    l = CAP_LAYOUT
    n = l.inner[0]
    assert 2 * n > CAP_THREADS and l.nd == 2
    start = bc_start(l)
    out = start.copy()
    src, dst = view(l, start), view(l, out)
    X = (2 * np.arange(n, dtype=np.int64) + 1) + int(CAP_GEOM.pos_begin[0] * 2 ** 10)        # cell centres in units of 2^-10
    assert np.array_equal(X / 2.0 ** 10, (np.arange(n) * CAP_GEOM.h[0] + CAP_GEOM.pos_begin[0]) + 0.5 * CAP_GEOM.h[0])
    Z = Fraction(CAP_GEOM.pos_begin[2]) + Fraction(CAP_GEOM.h[2]) / 2                         # (0 * h + pos_begin) + h / 2
    for side, row, ghost in ((0, 0, -1), (1, l.inner[1] - 1, l.inner[1])):
        Y2 = int(2 * ((l.inner[1] if side else 0) * Fraction(CAP_GEOM.h[1]) + Fraction(CAP_GEOM.pos_begin[1])))     # wall in units of 1/2
        G = X * Y2 + int(Z * 2 ** 11)                                                         # g = x * y + z in units of 2^-11
        interior = src[l.ref(2), row + l.ref(1), l.ref(0):l.ref(0) + n].astype(np.int64)
        V = 2 * G - interior * 2 ** 11
        assert int(np.abs(V).max()) < 2 ** 52
        dst[l.ref(2), ghost + l.ref(1), l.ref(0):l.ref(0) + n] = V.astype(np.float64) / 2.0 ** 11
    return start, out


# ---- examg_vec_apply_bc_cell ------------------------------------------------------------------------------------------------------------
VEC_LAYOUTS = {"5x4x3_g1": FieldLayout.cell(3, (5, 4, 3), 1), "2d_7x3_g1": FieldLayout.cell(2, (7, 3), 1)}
assert any(l.size % 2 == 1 for l in VEC_LAYOUTS.values())
VEC_TAIL = 5
VEC_CASES = [(ln, n, m) for ln, l in VEC_LAYOUTS.items() for n in (2, 3) for m in ((1 << (2 * l.nd)) - 1, 0b100110 & ((1 << (2 * l.nd)) - 1), 1, 0)]


def vec_bc_reference(lname, n, mask):
    """(start, afterwards): every component plane the scalar Neumann reference of that plane, the tail untouched."""
    l = VEC_LAYOUTS[lname]
    start = bc_start(l, VEC_TAIL, n)
    out = start.copy()
    for c in range(n):
        out[c * l.size:(c + 1) * l.size] = exact_bc_cell(l, start[c * l.size:(c + 1) * l.size], EGEOM, NEUMANN, None, mask)
    return start, out


# ---- positions per localization: examg_fill_expr[_cell|_face], examg_max_err_expr[_cell|_face] ----------------------------------------------
POS_PROGRAMS = {"x": prog("x"), "y": prog("y"), "z": prog("z"), "poly": prog("x x * 0.5 y * z * - 0.25 z * + y -")}


def pos_layout(loc, nd):
    cells = (6, 5, 4) if nd == 3 else (9, 4)
    if loc == "node":
        return FieldLayout.node(nd, tuple(cells) + (0,) * (3 - nd), 2, align=2)
    if loc == "cell":
        return FieldLayout.cell(nd, cells, 2, align=2)
    return FieldLayout.face(nd, cells, LOCS.index(loc) - 2, 2, align=2)


POS_CASES = [(loc, nd) for nd in (3, 2) for loc in LOCS if LOCS.index(loc) - 2 < nd]


def exact_fill(l, start, geom, program, b, e, loc):
    """x[box] = program(position), position as blas_cases.positions gives it for the localization."""
    out = start.copy()
    if B.empty(b, e):
        return out
    f = frac_fn(program)
    px, py, pz = positions(geom, b, e, loc=loc)
    vals = np.array([[[fp64(f(x, y, z)) for x in px] for y in py] for z in pz])
    view(l, out)[box_index(l, b, e)] = vals
    return out


@lru_cache(maxsize=None)
def pos_reference(loc, nd, pname):
    """The whole allocation after the fill of SENTINELs over the box GLB..GRE (negative indices; the upper duplicate face)."""
    l = pos_layout(loc, nd)
    b, e = ghost_box(l)
    assert all(b[d] == -2 for d in range(nd))
    out = exact_fill(l, np.full(l.size, SENTINEL), EGEOM, POS_PROGRAMS[pname], b, e, loc)
    out.setflags(write=False)
    return out


def plants(b, e):
    return {"first": tuple(b), "last": tuple(v - 1 for v in e), "row_end": (e[0] - 1, (b[1] + e[1]) // 2, (b[2] + e[2]) // 2)}


def planted(l, filled, where):
    """The filled field with a deviation of 3.0 at one point of the box GLB..GRE; exact: the values are dyadic and small."""
    a = filled.copy()
    p = plants(*ghost_box(l))[where]
    a[l.linear(*p)] = a[l.linear(*p)] + 3.0
    assert Fraction(float(a[l.linear(*p)])) - Fraction(float(filled[l.linear(*p)])) == 3
    return a


# ---- examg_apply_bc_face ----------------------------------------------------------------------------------------------------------------
def exact_bc_face(axis, l, start, geom, kind, program, mask):
    """include/examg.h, the paragraph of examg_apply_bc_face.  Walls normal to `axis` (node rule): the boundary face = g(its position).
    Other walls (cell rule): the ghost beside every face of the boundary row -- tangentially the cells [0, cells), on the own axis the
    faces [0, cells + 1) -- is (2 * g(wall point)) - interior resp. interior; where that face is a boundary face of a normal wall of the
    mask, `interior` is g(position of the face), whatever the array held."""
    nd, cells = l.nd, l.ncells
    out, src = start.copy(), view(l, start)
    dst = view(l, out)
    g = frac_fn(program) if program is not None else None
    h, pb = [Fraction(geom.h[d]) for d in range(3)], [Fraction(geom.pos_begin[d]) for d in range(3)]

    def face_position(i):
        return [i[t] * h[t] + pb[t] + (0 if t == axis else h[t] / 2) for t in range(3)]

    def extent(t):
        return (cells[t] + 1 if t == axis else cells[t]) if t < nd else 1

    for side in (0, 1):                                   # node rule
        if mask & (1 << (2 * axis + side)):
            assert kind == DIRICHLET
            b, e = [0, 0, 0], [extent(t) for t in range(3)]
            b[axis], e[axis] = (cells[axis], cells[axis] + 1) if side else (0, 1)
            for i in points(b, e):
                dst[at(l, i)] = fp64(g(*face_position(i)))
    for d in range(nd):                                   # cell rule
        if d == axis:
            continue
        for side in (0, 1):
            if not mask & (1 << (2 * d + side)):
                continue
            b, e = [0, 0, 0], [extent(t) for t in range(3)]
            b[d], e[d] = (cells[d] - 1, cells[d]) if side else (0, 1)
            for i in points(b, e):
                on_wall = (i[axis] == 0 and mask & (1 << (2 * axis))) or (i[axis] == cells[axis] and mask & (1 << (2 * axis + 1)))
                interior = g(*face_position(i)) if on_wall else Fraction(float(src[at(l, i)]))
                o = list(i)
                o[d] += 1 if side else -1
                if kind == NEUMANN:
                    v = interior
                else:
                    p = face_position(i)
                    p[d] = (cells[d] if side else 0) * h[d] + pb[d]
                    v = 2 * g(*p) - interior
                dst[at(l, o)] = fp64(v)
    return out


def face_layouts(nd, axis):
    cells = (6, 3) if nd == 2 else (6, 3, 5)
    return {"g1": FieldLayout.face(nd, cells, axis, 1), "g2_a2": FieldLayout.face(nd, cells, axis, 2, align=2)}


def face_masks(nd, axis, kind):
    full = (1 << (2 * nd)) - 1
    if kind == DIRICHLET:
        return [1 << f for f in range(2 * nd)] + [full]
    tang = full & ~(3 << (2 * axis))
    return [1 << f for f in range(2 * nd) if f // 2 != axis] + [tang]


FACE_CASES = [(nd, axis, ln, kind, m) for nd in (2, 3) for axis in range(nd) for ln in ("g1", "g2_a2") for kind in (DIRICHLET, NEUMANN)
              for m in face_masks(nd, axis, kind)]


@lru_cache(maxsize=None)
def bc_face_reference(nd, axis, lname, kind, mask):
    l = face_layouts(nd, axis)[lname]
    out = exact_bc_face(axis, l, bc_start(l), EGEOM, kind, BC_PROGRAM if kind == DIRICHLET else None, mask)
    out.setflags(write=False)
    return out


# ---- the _grid entry points -------------------------------------------------------------------------------------------------------------
GRID_LAYOUT = FieldLayout.node(3, (7, 5, 4), 1, align=16)
GRID_GHOST = 2
GRID_PROGRAMS = {"poly": gprog("x y * wx wz * + z -"), "wx": gprog("wx"), "wy": gprog("wy"), "wz": gprog("wz")}
GRID_MASKS = (63, 0b100110, 0)


def grid_tables(l=GRID_LAYOUT, ghost=GRID_GHOST):
    """Per axis the positions of the nodes -ghost .. cells + ghost: cumulated dyadic widths that differ per axis and per cell."""
    out = []
    for d in range(l.nd):
        cells = l.inner[d] + 1
        widths = [Fraction(1 + (3 * j + d) % 5, 8 << d) for j in range(cells + 2 * ghost)]
        assert len(set(widths[:5])) == 5
        x = [Fraction(-3 + d, 4)]
        for w in widths:
            x.append(x[-1] + w)
        out.append(np.array([fp64(v) for v in x]))
    assert len({tuple(np.diff(t)[:4]) for t in out}) == len(out)
    return out


def exact_fill_grid(l, start, tables, ghost, program, b, e):
    """Position of point i: table[i + ghost]; width of its cell: table[i + ghost + 1] - table[i + ghost]; 0 on an axis without table."""
    out = start.copy()
    if B.empty(b, e):
        return out
    f = frac_fn(program)
    dst = view(l, out)
    for i in points(b, e):
        p, w = [Fraction(0)] * 3, [Fraction(0)] * 3
        for d in range(l.nd):
            j = i[d] + ghost
            assert 0 <= j and j + 1 < len(tables[d])
            p[d], w[d] = Fraction(float(tables[d][j])), Fraction(float(tables[d][j + 1])) - Fraction(float(tables[d][j]))
        dst[at(l, i)] = fp64(f(p[0], p[1], p[2], wx=w[0], wy=w[1], wz=w[2]))
    return out


def face_boxes(l, mask):
    """`apply bc` of a node field: the duplicate plane of each face of the mask, tangentially GLB..GRE."""
    out = []
    for d in range(l.nd):
        for side in (0, 1):
            if mask & (1 << (2 * d + side)):
                b, e = [list(v) for v in ghost_box(l)]
                b[d], e[d] = (l.idx("DRB", d), l.idx("DRE", d)) if side else (l.idx("DLB", d), l.idx("DLE", d))
                out.append((tuple(b), tuple(e)))
    return out


GRID_FILL_BOX = ((-1, -1, -1), ghost_box(GRID_LAYOUT)[1])


@lru_cache(maxsize=None)
def grid_fill_reference(pname):
    out = exact_fill_grid(GRID_LAYOUT, np.full(GRID_LAYOUT.size, SENTINEL), grid_tables(), GRID_GHOST, GRID_PROGRAMS[pname], *GRID_FILL_BOX)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def grid_dirichlet_reference(pname, mask):
    out = np.full(GRID_LAYOUT.size, SENTINEL)
    for b, e in face_boxes(GRID_LAYOUT, mask):
        out = exact_fill_grid(GRID_LAYOUT, out, grid_tables(), GRID_GHOST, GRID_PROGRAMS[pname], b, e)
    out.setflags(write=False)
    return out
