"""Cases and references for the kernels of csrc/kernels_blas.hip and the expression interpreter of csrc/examg_common.h (ExprEval):
the BLAS-1 loops, the two-stage reductions, the boundary fills, the data movers and examg_fill_random.

Nothing here shares code with the library (exastencils_amd.ops is not imported) or with the oracle: the references are numpy index
arithmetic on views of whole allocations (stencil_cases.Lay), Python integers, fractions.Fraction, math.fsum and mpmath.  The
dispatch of the reductions is restated in reduction_plan, that of examg_axpby in axpby_form; tests/test_blas_exact.py runs every
reference against the oracle and asserts that the case tables reach what they claim to reach.

Exact data: fields of integers in [-16, 16] (stencil_cases.int_field) and dyadic scalars.  Every product is at most 256 in magnitude and
every sum over a box of at most 2^22 points below 2^31, so each is exact in fp64 whatever the order -- dot and sum are compared with ==
against a Python integer.  Random data: splitmix64 restated below.  Elementwise kernels are then compared bit for bit with numpy
evaluating the one expression of the form (one rounding per operation, no fused multiply-add); reductions against math.fsum of the
fp64 terms with the bound (K + 1) * 2^-53 * fsum(|terms|), K = the longest chain of additions a term passes through in the launch
that reduction_plan restates.
"""
import math
from collections import namedtuple
from fractions import Fraction
from functools import lru_cache

import numpy as np

import stencil_cases as S

from exastencils_amd.layout import FieldLayout
from exastencils_amd.lib import MAX_EXPR, GeomC

SENTINEL = -777.25                       # what an array holds where nothing may be written
OUTSIDE = float(2 ** 20 + 1)             # what a reduced field holds outside the box: a read there cannot cancel
U = 2.0 ** -53                           # unit roundoff of fp64

# ---- layouts: every argument its own ------------------------------------------------------------------------------------------------
# (ghost, align, communicates_dup, communicates_ghost) of x and of y
PAIRS = {
    "own": ("node", 3, (2, 0, True, True), (1, 16, True, False)),
    "own2": ("node", 3, (1, 2, False, True), (2, 16, True, True)),
    "2d": ("node", 2, (2, 2, True, True), (1, 0, True, False)),
    "cell": ("cell", 3, (2, 2, True, True), (1, 0, True, False)),
    "split_x": ("node", 3, (2, 0, True, True), (1, 16, True, False)),
    "split_y": ("node", 3, (2, 0, True, True), (1, 16, True, False)),
}


def box_of(case):
    b = tuple(case.begin)
    return b, tuple(b[d] + case.n[d] for d in range(3))


def layouts(case):
    """(lx, ly): the plain layouts of the two arguments, large enough for the box, no two extents alike.  Which of them the GPU side
    puts under the colour split: split_of."""
    kind, nd, sx, sy = PAIRS[case.lays]
    b, e = box_of(case)
    def make(cells):
        if kind == "cell":
            return [FieldLayout.cell(nd, [c + 1 for c in cells[:nd]], g, cghost, align) for g, align, cdup, cghost in (sx, sy)]
        return [FieldLayout.node(nd, cells, g, cdup, cghost, align) for g, align, cdup, cghost in (sx, sy)]

    cells = [max(e[d], 1) if d < nd else 0 for d in range(3)]
    for d in range(1, nd):                 # room behind the box, and more of it until no two extents of an allocation are alike
        cells[d] += d
        while any(len({l.tot(t) for t in range(d + 1)}) <= d for l in make(cells)):
            cells[d] += 1
    out = make(tuple(cells))
    for l in out:
        for d in range(nd):
            assert l.idx("GLB", d) <= b[d] and (e[d] <= l.idx("GRE", d) or e[d] <= b[d]), (case, d)
        assert all((b[d], e[d]) == (0, 1) for d in range(nd, 3))
    return tuple(out)


def split_of(case):
    return case.lays == "split_x", case.lays == "split_y"


def view(l, a):
    """The flat allocation `a` of the plain layout l as a (z, y, x) array."""
    return a.reshape(S.Lay(l).shape)


def box_index(l, b, e):
    return S.Lay(l).box(b, e)


def empty(b, e):
    return any(e[d] <= b[d] for d in range(3))


# ---- examg_fill_random: splitmix64 of seed + golden * (i + 1), top 53 bits, * 2^-52 - 1 ---------------------------------------------
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def random_value(seed, i):
    """Value i of the stream of `seed`, in Python integers."""
    z = (seed + GOLDEN * (i + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z = z ^ (z >> 31)
    return float(Fraction(z >> 11, 1 << 52) - 1)          # a multiple of 2^-52 in [-1, 1): exact in fp64


def random_field(n, seed):
    """The first n values of the stream as an array: the same steps on numpy's wrapping 64-bit integers (test_blas_exact compares
    it with random_value)."""
    with np.errstate(over="ignore"):
        i = np.arange(1, int(n) + 1, dtype=np.uint64)
        z = np.uint64(seed & M64) + np.uint64(GOLDEN) * i
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0     # < 2^53: the conversion and both operations are exact


RANDOM_SIZES = (1, 255, 256, 257, 8192 * 256 + 3)        # the last: the grid-stride loop past the cap of 8192 workgroups
RANDOM_SEEDS = (0, 1, 1 << 63, (1 << 64) - 1)


def field(size, data, seed):
    return S.int_field(size, seed) if data == "int" else random_field(size, seed)


# ---- elementwise kernels --------------------------------------------------------------------------------------------------------------
ECase = namedtuple("ECase", "name n begin lays")
ELEMENTWISE = [
    ECase("37x5x3_into_ghost", (37, 5, 3), (-1, 0, 1), "own"),
    ECase("1x1x1", (1, 1, 1), (1, 2, 0), "own"),
    ECase("127x130x131", (127, 130, 131), (0, 1, 0), "own"),          # 2162810 points: one trip past 8192 * 256 threads
    ECase("37x5x3_other_pads", (37, 5, 3), (-1, 0, 1), "own2"),
    ECase("2d_37x5", (37, 5, 1), (-1, 1, 0), "2d"),
    ECase("cell_37x5x3", (37, 5, 3), (-1, 0, 1), "cell"),
    ECase("splitx_37x5x3", (37, 5, 3), (-1, 0, 1), "split_x"),
    ECase("splity_37x5x3", (37, 5, 3), (-1, 0, 1), "split_y"),
]
ELEMENTWISE_CAP = 8192 * 256

# (a, b) -> the form of examg_axpby; the ties (1, 1), (1, 0) and b = -0.0 are decided by the order of the header's sentence:
# "b==0: a*x (copy for a==1);  b==1: y + a*x;  a==1: x + b*y"
AXPBY_SCALARS = [(2.5, 0.0), (1.0, 0.0), (-0.375, 1.0), (1.0, -0.75), (1.5, -0.25), (1.0, 1.0), (0.5, -0.0), (1.0, -0.0)]
AXPBY_FORMS = [0, 1, 2, 3, 4, 2, 0, 1]
# which, a, b, sign -> form; a (which 0) or b (which 1) comes from the device as sign * (num / den) resp. num / den
DEV_NUM, DEV_DEN = 3.7, 1.9
AXPBY_DEV = [(0, 0.0, 1.0, -1.0, 2), (0, 0.0, 0.0, 1.0, 0), (0, 0.0, -0.625, -1.0, 4), (1, 1.0, 0.0, 1.0, 3), (1, -1.75, 0.0, 1.0, 4)]


def axpby_form(a, b):
    if b == 0.0:
        return 1 if a == 1.0 else 0
    if b == 1.0:
        return 2
    return 3 if a == 1.0 else 4


def axpby_dev_form(which, a, b):
    if which == 0:
        return 2 if b == 1.0 else (0 if b == 0.0 else 4)
    return 3 if a == 1.0 else 4


def dev_scalars(which, a, b, sign):
    """The (a, b) examg_axpby_dev computes with: sign * (num / den) in that order."""
    q = np.float64(DEV_NUM) / np.float64(DEV_DEN)
    return (float(np.float64(sign) * q), b) if which == 0 else (a, float(q))


def form_values(form, a, b, x, y):
    """The one expression of the form on fp64 arrays, one rounding per operation."""
    a, b = np.float64(a), np.float64(b)
    if form == 0:
        return a * x
    if form == 1:
        return x.copy()
    if form == 2:
        return y + a * x
    if form == 3:
        return x + b * y
    p, q = a * x, b * y              # two products, each rounded, then one addition: no fused multiply-add
    return p + q


def exact_axpby_values(a, b, x, y):
    """a * x + b * y on integer fields with dyadic scalars in integer arithmetic, converted once."""
    fa, fb = Fraction(a), Fraction(b)
    den = max(fa.denominator, fb.denominator)
    assert den & (den - 1) == 0 and den <= 1 << 20
    r = int(fa * den) * x.astype(np.int64) + int(fb * den) * y.astype(np.int64)
    assert int(np.abs(r).max(initial=0)) < 1 << 52
    return r.astype(np.float64) / float(den)


def ref_axpby(lx, x, ly, y, a, b, box, form=None, exact=False):
    """y afterwards (the whole allocation): the form's expression in the box, untouched elsewhere."""
    out = y.copy()
    b_, e_ = box
    if empty(b_, e_):
        return out
    xs, ys = view(lx, x)[box_index(lx, b_, e_)], view(ly, out)[box_index(ly, b_, e_)]
    form = axpby_form(a, b) if form is None else form
    view(ly, out)[box_index(ly, b_, e_)] = exact_axpby_values(a, b, xs, ys) if exact else form_values(form, a, b, xs, ys)
    return out


def ref_set(l, x, v, box):
    out = x.copy()
    if not empty(*box):
        view(l, out)[box_index(l, *box)] = v
    return out


def ref_add_scalar(l, x, c, box, exact=False):
    out = x.copy()
    if not empty(*box):
        s = box_index(l, *box)
        view(l, out)[s] = exact_axpby_values(1.0, c, view(l, x)[s], np.ones_like(view(l, x)[s])) if exact else view(l, x)[s] + np.float64(c)
    return out


# ---- reductions -----------------------------------------------------------------------------------------------------------------------
RED_BLOCK, RED_MAX_BLOCKS, ROW_MIN = 256, 2048, 128
Plan = namedtuple("Plan", "kernel nb capped tail final serial K")


def reduction_plan(box, lx, ly=None):
    """The launch of examg_dot / examg_sum restated (lx, ly: FieldLayouts; ly None for examg_sum).
    kernel  "empty" (a memset), "partial" (k_dot_partial: one point per thread and trip) or "rows" (k_dot_rows: a wave per row, two
            points per lane and trip) -- rows of at least 128 points of untransformed layouts only: a colour-split argument forces
            "partial" however long the rows are;
    nb      workgroups = partial sums, min(2048, ceil(count / 1024));
    tail    k_dot_rows' single-element branch: "none" (even rows), "lane0" or "lane>0";
    final   k_reduce_final: "single" (at most one partial per thread) or "strided";
    K       the longest chain of additions a term passes through: the serial additions of its thread, 6 shuffle steps, up to 3
            additions in LDS, ceil(nb / 256) serial additions in the final kernel, 6 + 3 again."""
    b, e = box
    n = [e[d] - b[d] for d in range(3)]
    if min(n) <= 0:
        return Plan("empty", 0, False, "none", "none", 0, 0)
    count = n[0] * n[1] * n[2]
    want = -(-count // (RED_BLOCK * 4))
    nb = max(1, min(RED_MAX_BLOCKS, want))
    transformed = lx.transform != 0 or (ly is not None and ly.transform != 0)
    if n[0] >= ROW_MIN and not transformed:
        kernel = "rows"
        rows_per_wave = -(-(n[1] * n[2]) // (nb * (RED_BLOCK // 64)))
        serial = rows_per_wave * max(sum(min(2, n[0] - i) for i in range(2 * lane, n[0], 128)) for lane in range(64))
        tail = "none" if n[0] % 2 == 0 else ("lane0" if ((n[0] - 1) % 128) // 2 == 0 else "lane>0")
    else:
        kernel, tail = "partial", "none"
        serial = -(-count // (nb * RED_BLOCK))
    final_serial = -(-nb // RED_BLOCK)
    final = "single" if nb <= RED_BLOCK else "strided"
    return Plan(kernel, nb, want > RED_MAX_BLOCKS, tail, final, serial, serial + 6 + 3 + final_serial + 6 + 3)


def reachable_plans():
    """Every (kernel, tail, final) reduction_plan can return.  Written out by hand from the branches of reduction_plan: the coverage test
    proves the table against this list, not the list against reduction_plan -- a branch added there has to be added here too."""
    return ({("empty", "none", "none")} | {("partial", "none", f) for f in ("single", "strided")}
            | {("rows", t, f) for t in ("none", "lane0", "lane>0") for f in ("single", "strided")})


RCase = namedtuple("RCase", "name n begin lays kernel tail final")
REDUCTIONS = [
    RCase("1x1x1", (1, 1, 1), (1, 2, 0), "own", "partial", "none", "single"),
    RCase("37x5x3", (37, 5, 3), (1, 1, 1), "own", "partial", "none", "single"),            # one workgroup, most threads idle
    RCase("127x9x4", (127, 9, 4), (0, 1, 0), "own", "partial", "none", "single"),          # just under the row bound
    RCase("128x7x3_even", (128, 7, 3), (0, 1, 1), "own", "rows", "none", "single"),        # just over it
    RCase("128x7x3_odd", (128, 7, 3), (1, 0, 1), "own", "rows", "none", "single"),         # the other parity of the 16-byte load address
    RCase("129x5x4", (129, 5, 4), (0, 0, 1), "own", "rows", "lane0", "single"),            # single-element tail in lane 0 of the second trip
    RCase("131x3x2", (131, 3, 2), (1, 1, 0), "own", "rows", "lane>0", "single"),           # tail in lane 1
    RCase("257x3x2", (257, 3, 2), (0, 1, 1), "own", "rows", "lane0", "single"),            # third trip
    RCase("1030x3x2", (1030, 3, 2), (1, 0, 0), "own", "rows", "none", "single"),           # more waves than rows
    RCase("130x48x45", (130, 48, 45), (0, 1, 1), "own", "rows", "none", "strided"),        # nb = 275 > 256
    RCase("127x130x131", (127, 130, 131), (1, 0, 1), "own", "partial", "none", "strided"),  # nb capped, several trips per thread
    RCase("128x128x130", (128, 128, 130), (0, 1, 0), "own", "rows", "none", "strided"),    # k_dot_rows with nb capped
    # added to the issue's table: the two tail shapes under a strided final stage (the coverage test asks for every combination)
    RCase("129x47x46", (129, 47, 46), (1, 1, 0), "own2", "rows", "lane0", "strided"),
    RCase("131x46x45", (131, 46, 45), (0, 0, 1), "own2", "rows", "lane>0", "strided"),
    # the other kinds of layout pairs
    RCase("2d_131x7", (131, 7, 1), (1, -1, 0), "2d", "rows", "lane>0", "single"),
    RCase("2d_37x5", (37, 5, 1), (-1, 1, 0), "2d", "partial", "none", "single"),
    RCase("cell_129x5x4", (129, 5, 4), (-1, 0, 1), "cell", "rows", "lane0", "single"),
    RCase("splitx_257x3x2", (257, 3, 2), (0, 1, 1), "split_x", "partial", "none", "single"),   # long rows, yet k_dot_partial
    RCase("splity_257x3x2", (257, 3, 2), (0, 1, 1), "split_y", "partial", "none", "single"),
]
CAPPED = ("127x130x131", "128x128x130")
EMPTY_BOXES = [((1, 2, 1), (5, 2, 4)), ((3, 1, 2), (2, 5, 1))]      # end == begin in one dimension; end < begin in two


def plan_of(case, sum_only=False):
    """The plan of examg_dot (of examg_sum on x: sum_only) with the layouts the GPU test passes."""
    lx, ly = layouts(case)
    sx, sy = split_of(case)
    lx = lx.split_x() if sx else lx
    ly = ly.split_x() if sy else ly
    return reduction_plan(box_of(case), lx, None if sum_only else ly)


def reduced_field(l, box, data, seed):
    """A field that holds `data` in the box and OUTSIDE everywhere else."""
    a = np.full(l.size, OUTSIDE)
    view(l, a)[box_index(l, *box)] = view(l, field(l.size, data, seed))[box_index(l, *box)]
    return a


@lru_cache(maxsize=None)
def reduction_inputs(name, data):
    case = next(c for c in REDUCTIONS if c.name == name)
    lx, ly = layouts(case)
    x, y = reduced_field(lx, box_of(case), data, 11), reduced_field(ly, box_of(case), data, 12)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def ref_reduction(lx, x, ly, y, box, exact):
    """(value, allowance before the factor K + 1) of the dot product (ly, y None: of the sum): a Python integer and 0 on integer
    data; math.fsum of the fp64 terms and 2^-53 * fsum(|terms|) otherwise."""
    if empty(*box):
        return 0, 0.0
    t = view(lx, x)[box_index(lx, *box)]
    if exact:
        t = t.astype(np.int64)
        assert np.array_equal(t, view(lx, x)[box_index(lx, *box)])
        if y is not None:
            t = t * view(ly, y)[box_index(ly, *box)].astype(np.int64)
        return int(t.sum()), 0.0
    if y is not None:
        t = t * view(ly, y)[box_index(ly, *box)]          # the fp64 products
    t = t.ravel().tolist()
    return math.fsum(t), U * math.fsum(abs(v) for v in t)


@lru_cache(maxsize=None)
def reduction_reference(name, data, sum_only):
    case = next(c for c in REDUCTIONS if c.name == name)
    lx, ly = layouts(case)
    x, y = reduction_inputs(name, data)
    return ref_reduction(lx, x, None if sum_only else ly, None if sum_only else y, box_of(case), data == "int")


def needle_points(case):
    """Where the single 1 of a needle field goes, with the box of each run: the first and the last point of the first and of the last
    row, the last point of a row in the middle (the tail element where the rows are odd), and a point of the outermost ghost layer
    that both layouts have, with the box grown to hold it."""
    b, e = box_of(case)
    lx, ly = layouts(case)
    pts = [((x0, x1, x2), (b, e)) for (x1, x2) in ((b[1], b[2]), (e[1] - 1, e[2] - 1)) for x0 in (b[0], e[0] - 1)]
    pts.append(((e[0] - 1, (b[1] + e[1]) // 2, (b[2] + e[2]) // 2), (b, e)))
    g = min(lx.ghost[0], ly.ghost[0])
    gb = (-g, b[1], b[2])
    pts.append(((-g, (b[1] + e[1]) // 2, e[2] - 1), (gb, e)))
    return pts


def needle_field(l, box, point):
    a = np.full(l.size, OUTSIDE)
    v = view(l, a)
    v[box_index(l, *box)] = 0.0
    v[box_index(l, point, tuple(p + 1 for p in point))] = 1.0
    return a


NEEDLE_CASES = ("37x5x3", "129x5x4", "131x3x2", "2d_131x7", "splitx_257x3x2")

# ---- expression programs ----------------------------------------------------------------------------------------------------------------
EXACT_OPS = ("const", "x", "y", "z", "+", "-", "*", "/", "neg", "fabs", "max", "min", "sqrt")
LIBM_OPS = ("sin", "cos", "tan", "exp", "log", "sinh", "cosh", "tanh", "pow")


def prog(text):
    """A postfix program from words: x y z, operator names, anything else a literal."""
    out = []
    for w in text.split():
        out.append((w, None) if w in ("x", "y", "z", "+", "-", "*", "/", "neg", "fabs", "max", "min", "sqrt") + LIBM_OPS else ("const", float(w)))
    return out


def geometry(pos_begin, h):
    g = GeomC()
    for d in range(3):
        g.pos_begin[d], g.h[d] = pos_begin[d], h[d]
    return g


def _fsqrt(v):
    n, d = math.isqrt(v.numerator), math.isqrt(v.denominator)
    assert v >= 0 and n * n == v.numerator and d * d == v.denominator, "sqrt of %r is not rational" % (v,)
    return Fraction(n, d)


def eval_exact(program, x, y, z):
    """The postfix program on Fractions: the operand pushed first is the left one."""
    st = []
    for name, c in program:
        if name == "const":
            st.append(Fraction(c))
        elif name in ("x", "y", "z"):
            st.append({"x": x, "y": y, "z": z}[name])
        elif name == "neg":
            st[-1] = -st[-1]
        elif name == "fabs":
            st[-1] = abs(st[-1])
        elif name == "sqrt":
            st[-1] = _fsqrt(st[-1])
        else:
            r = st.pop()
            l = st.pop()
            st.append({"+": lambda: l + r, "-": lambda: l - r, "*": lambda: l * r, "/": lambda: l / r, "max": lambda: max(l, r),
                       "min": lambda: min(l, r)}[name]())
    assert len(st) == 1
    return st[0]


def stack_depth(program):
    sp = deepest = 0
    for name, _ in program:
        sp += 1 if name in ("const", "x", "y", "z") else (-1 if name in ("+", "-", "*", "/", "pow", "max", "min") else 0)
        deepest = max(deepest, sp)
    return deepest


def positions(geom, b, e, cell=False, loc=None):
    """Per dimension the exact positions index * h + pos_begin (+ h / 2 for cell centres) of the indices [b, e), as Fractions.
    loc ("node", "cell", "face_x", "face_y", "face_z") overrides `cell`: a face of axis a is a node on a and a cell centre elsewhere."""
    loc = ("cell" if cell else "node") if loc is None else loc
    own = {"node": (0, 1, 2), "cell": (), "face_x": (0,), "face_y": (1,), "face_z": (2,)}[loc]
    out = []
    for d in range(3):
        h, pb = Fraction(geom.h[d]), Fraction(geom.pos_begin[d])
        out.append([i * h + pb + (0 if d in own else h / 2) for i in range(b[d], e[d])])
    return out


def exact_values(program, geom, b, e, cell=False):
    """The program at every point of the box as a (z, y, x) fp64 array; every value must be an fp64 number (and with dyadic geometry,
    dyadic constants, divisors that are powers of two and square roots of perfect squares every intermediate is one too)."""
    px, py, pz = positions(geom, b, e, cell)
    out = np.empty((len(pz), len(py), len(px)))
    for k, z in enumerate(pz):
        for j, y in enumerate(py):
            for i, x in enumerate(px):
                v = eval_exact(program, x, y, z)
                f = v.numerator / v.denominator
                assert Fraction(f) == v, "not exact in fp64: %r" % (v,)
                out[k, j, i] = f
    return out


def long_program():
    """256 instructions, every literal different: x, then 127 times (literal, + or -), then neg."""
    p = [("x", None)]
    for i in range(1, 128):
        p += [("const", i + (i * i % 7) / 8.0), ("+" if i % 3 else "-", None)]
    p.append(("neg", None))
    assert len(p) == MAX_EXPR and len({c for n, c in p if n == "const"}) == 127
    return p


def deep_program(depth=24):
    """`depth` pushes, then depth - 1 non-commutative operations: one division by the literal 4 on top, then subtractions."""
    p = [("x", None), ("y", None), ("z", None)] + [("const", 1.0 + i / 4.0) for i in range(depth - 4)] + [("const", 4.0)]
    p += [("/", None)] + [("-", None)] * (depth - 2)
    assert stack_depth(p) == depth
    return p


EGEOM = geometry((-0.75, -0.25, -0.5), (0.125, 0.25, 0.5))        # dyadic, negative and positive positions, x < y and x > y
PGEOM = geometry((0.0, -0.25, -0.5), (0.125, 0.25, 0.5))          # x = 1/8, 1/4 at the indices 1, 2: powers of two
EBOX = ((-1, 0, 0), (12, 5, 3))
PBOX = ((1, 0, 0), (3, 5, 3))
EXACT_PROGRAMS = {                                                  # name: (program, geometry, box)
    "sub": (prog("x y -"), EGEOM, EBOX),
    "div_by_4": (prog("x 4 /"), EGEOM, EBOX),
    "4_div_by_x": (prog("4 x /"), PGEOM, PBOX),
    "max": (prog("x y max"), EGEOM, EBOX),
    "min": (prog("x y min"), EGEOM, EBOX),
    "neg_fabs": (prog("x neg y fabs * z fabs neg +"), EGEOM, EBOX),
    "sqrt": (prog("x x * y y * * sqrt z z * sqrt -"), EGEOM, EBOX),
    "poly": (prog("x x * 0.5 y * y * - 0.25 z * + 3 -"), EGEOM, EBOX),
    "all_exact_ops": (prog("x y max z min 2 / neg fabs x x * sqrt + y 8 * - 0.5 *"), EGEOM, EBOX),
    "256_instructions": (long_program(), EGEOM, EBOX),
    "depth_24": (deep_program(), EGEOM, EBOX),
}
EXPR_LAYOUT = FieldLayout.node(3, (13, 6, 4), 2, align=2)

# the libm class: one function per program on a 40-point row with arguments in [0.25, 2.0] (pow: x in the row, y in {0.5, 1.25, 2.0})
LGEOM = geometry((0.25, 0.5, 0.0), (11.0 / 256.0, 0.75, 0.0))
LBOX = ((0, 0, 0), (40, 3, 1))
LIBM_LAYOUT = FieldLayout.node(3, (41, 4, 2), 1)
# function: (largest error measured on an MI355X, bound = measured + 1), in ulps of the reference value (mpmath at 50 digits at the
# exact fp64 argument, rounded once).  The oracle's numpy has to stay within the same bounds.
LIBM_ULP = {
    "sin": (1, 2), "cos": (1, 2), "tan": (1, 2), "exp": (1, 2), "log": (1, 2), "sinh": (1, 2), "cosh": (0, 1), "tanh": (1, 2), "pow": (1, 2),
}


def libm_program(fn):
    return prog("x y pow") if fn == "pow" else prog("x " + fn)


@lru_cache(maxsize=None)
def libm_reference(fn):
    """The function at the exact arguments with 50 digits, rounded once to fp64: a (1, 3, 40) array."""
    import mpmath

    px, py, pz = positions(LGEOM, *LBOX)
    out = np.empty((1, len(py), len(px)))
    with mpmath.workdps(50):
        for j, y in enumerate(py):
            for i, x in enumerate(px):
                mx, my = mpmath.mpf(x.numerator) / x.denominator, mpmath.mpf(y.numerator) / y.denominator
                out[0, j, i] = float(mpmath.power(mx, my) if fn == "pow" else getattr(mpmath, fn)(mx))
    assert 0.25 <= float(px[0]) and float(px[-1]) <= 2.0
    return out


def ulp_error(got, ref):
    """The largest |got - ref| in units of the spacing of fp64 at ref."""
    return float(np.max(np.abs(got - ref) / np.spacing(np.abs(ref))))


# ---- max |x - e(position)| -----------------------------------------------------------------------------------------------------------
MCase = namedtuple("MCase", "name n begin lays program")
MAXERR = [
    MCase("37x5x3", (37, 5, 3), (-1, 0, 1), "own", "x x * 0.5 y * y * - 0.25 z * +"),
    MCase("129x5x4", (129, 5, 4), (0, 1, 0), "own2", "x y * z -"),
    MCase("131x17x16", (131, 17, 16), (0, 0, 1), "own", "x y - z +"),          # 35 partial maxima: lanes past 32 of the final stage
    MCase("2d_37x5", (37, 5, 1), (1, -1, 0), "2d", "x x * y -"),
    MCase("cell_37x5x3", (37, 5, 3), (-1, 0, 1), "cell", "x y * z -"),
    MCase("splitx_37x5x3", (37, 5, 3), (-1, 0, 1), "split_x", "x y * z -"),
]
MGEOM = geometry((-0.5, 0.25, -1.0), (2.0 ** -6, 2.0 ** -4, 2.0 ** -3))


def maxerr_plants(case):
    b, e = box_of(case)
    return {"first": b, "last": tuple(v - 1 for v in e), "row_end": (e[0] - 1, (b[1] + e[1]) // 2, (b[2] + e[2]) // 2)}


@lru_cache(maxsize=None)
def maxerr_base(name):
    """The field that equals the program on the box up to small dyadic deviations (at most 16 / 64), OUTSIDE elsewhere; with it the
    deviations, as Fractions."""
    case = next(c for c in MAXERR if c.name == name)
    l = layouts(case)[0]
    b, e = box_of(case)
    f = exact_values(prog(case.program), MGEOM, b, e, cell=case.lays == "cell")
    dev = S.int_field(f.size, 5).reshape(f.shape) / 64.0
    a = np.full(l.size, OUTSIDE)
    view(l, a)[box_index(l, b, e)] = f + dev                 # exact: dyadic values far from 2^53 ulps apart
    assert np.array_equal(view(l, a)[box_index(l, b, e)] - f, dev)
    a.setflags(write=False)
    return a, f, dev


def maxerr_field(case, where):
    """(field, expected maximum): the largest deviation, 3 or -3, planted at `where`."""
    a, f, dev = maxerr_base(case.name)
    l = layouts(case)[0]
    b, e = box_of(case)
    a = a.copy()
    p = maxerr_plants(case)[where]
    amp = -3.0 if where == "last" else 3.0
    rel = tuple(p[d] - b[d] for d in (2, 1, 0))
    view(l, a)[box_index(l, p, tuple(v + 1 for v in p))] = f[rel] + amp
    got = view(l, a)[box_index(l, b, e)].ravel().tolist()
    expected = max(abs(Fraction(u) - Fraction(v)) for u, v in zip(got, f.ravel().tolist()))
    assert expected == 3 and sum(abs(Fraction(u) - Fraction(v)) == 3 for u, v in zip(got, f.ravel().tolist())) == 1
    return a, float(expected)


# ---- boundary fills -------------------------------------------------------------------------------------------------------------------
FILL_LAYOUTS = {
    "3d_g1": FieldLayout.node(3, (12, 10, 8), 1),
    "3d_g2_a16": FieldLayout.node(3, (12, 10, 8), 2, align=16),
    "2d_g1_a16": FieldLayout.node(2, (20, 14, 0), 1, align=16),
    "2d_g2": FieldLayout.node(2, (20, 14, 0), 2),
}
FGEOM = geometry((-0.5, -0.25, 0.5), (0.125, 0.25, 0.0625))
FILL_PROGRAM = prog("x x * 0.5 y * y * - 0.25 z * + 3 -")


def fill_masks(nd):
    full = (1 << (2 * nd)) - 1
    return [full, 0] + [1 << f for f in range(2 * nd)] + [0b100110 & full]


def face_mask_array(l, face_mask, tangential_ghost):
    """Boolean (z, y, x) array of the points the fill writes: the duplicate plane of each face of the mask, tangentially GLB..GRE
    (`apply bc`) or DLB..DRE (`only dup on boundary`)."""
    L = S.Lay(l)
    m = np.zeros(L.shape, dtype=bool)
    for d in range(l.nd):
        for side in (0, 1):
            if not face_mask & (1 << (2 * d + side)):
                continue
            b, e = [0, 0, 0], [1, 1, 1]
            for t in range(l.nd):
                if t == d:
                    b[t], e[t] = (l.idx("DLB", t), l.idx("DLE", t)) if side == 0 else (l.idx("DRB", t), l.idx("DRE", t))
                else:
                    b[t], e[t] = (l.idx("GLB", t), l.idx("GRE", t)) if tangential_ghost else (l.idx("DLB", t), l.idx("DRE", t))
            if not empty(b, e):
                m[L.box(b, e)] = True
    return m


@lru_cache(maxsize=None)
def fill_values(lname):
    """FILL_PROGRAM at every point GLB..GRE of the layout (pads: SENTINEL), a (z, y, x) array."""
    l = FILL_LAYOUTS[lname]
    b = [l.idx("GLB", d) if d < l.nd else 0 for d in range(3)]
    e = [l.idx("GRE", d) if d < l.nd else 1 for d in range(3)]
    a = np.full(S.Lay(l).shape, SENTINEL)
    a[S.Lay(l).box(b, e)] = exact_values(FILL_PROGRAM, FGEOM, b, e)
    a.setflags(write=False)
    return a


def ref_boundary_fill(lname, face_mask, tangential_ghost):
    """The whole allocation after the fill of an array of SENTINELs."""
    m = face_mask_array(FILL_LAYOUTS[lname], face_mask, tangential_ghost)
    return np.where(m, fill_values(lname), SENTINEL).ravel()


# ---- data movers ----------------------------------------------------------------------------------------------------------------------
PACK_LAYOUT = FieldLayout.node(3, (11, 9, 6), 2, align=16)


def pack_boxes(l=PACK_LAYOUT):
    """Every duplicate and ghost send / receive box of a block (the ranges of the communicator)."""
    from exastencils_amd.comm import Communicator

    boxes = []
    for d in range(l.nd):
        boxes += list(Communicator.dup_ranges(l, l.nd, d))
        for side in (-1, 1):
            boxes += list(Communicator.ghost_ranges(l, l.nd, d, side))
    return [(tuple(b), tuple(e)) for b, e in boxes]


def ref_pack(l, x, box):
    return view(l, x)[box_index(l, *box)].ravel().copy()


def ref_unpack(l, x, buf, box):
    out = x.copy()
    s = box_index(l, *box)
    view(l, out)[s] = buf[:view(l, out)[s].size].reshape(view(l, out)[s].shape)
    return out


EXTERNAL = [(gi, ge, al) for gi in (1, 2) for ge in (0, 1, 2) for al in (0, 4)]
EXTERNAL_CELLS = (9, 7, 5)


def external_layouts(gi, ge, align):
    return FieldLayout.node(3, EXTERNAL_CELLS, gi, align=2), FieldLayout.node(3, EXTERNAL_CELLS, ge, align=align)


def ref_external(lsrc, src, ldst, dst):
    """dst afterwards: the copy over [DLB - min(ghosts), DRE + min(ghosts)) per dimension, iterator coordinates coincide."""
    g = [min(lsrc.ghost[d], ldst.ghost[d]) for d in range(3)]
    b = tuple(lsrc.idx("DLB", d) - g[d] for d in range(3))
    e = tuple(lsrc.idx("DRE", d) + g[d] for d in range(3))
    out = dst.copy()
    view(ldst, out)[box_index(ldst, b, e)] = view(lsrc, src)[box_index(lsrc, b, e)]
    return out


TRANSFORM_LAYOUTS = {"odd_x": FieldLayout.node(3, (8, 5, 3), 1), "even_x": FieldLayout.node(3, (9, 5, 3), 1),
                     "2d_odd_x": FieldLayout.node(2, (10, 5, 0), 2)}


def ref_split(l, plain, fill=SENTINEL):
    """The array of l.split_x(): `[x, y, z] => [x / 2, y, z, x % 2]` on array indices, first index fastest; extents ceil(TOTx / 2), TOTy,
    TOTz, 2.  Where the odd half has no point (odd TOTx) the array keeps `fill`."""
    v = view(l, plain)
    tz, ty, tx = v.shape
    out = np.full((2, tz, ty, (tx + 1) // 2), fill)
    out[0, :, :, :(tx + 1) // 2] = v[:, :, 0::2]
    out[1, :, :, :tx // 2] = v[:, :, 1::2]
    return out.ravel()


def ref_unsplit(l, split, fill=SENTINEL):
    tz, ty, tx = S.Lay(l).shape
    s = split.reshape(2, tz, ty, (tx + 1) // 2)
    out = np.full((tz, ty, tx), fill)
    out[:, :, 0::2] = s[0, :, :, :(tx + 1) // 2]
    out[:, :, 1::2] = s[1, :, :, :tx // 2]
    return out.ravel()


SF_ENTRIES = (1, 5, 7, 27)
SF_SIZES = (63, 64, 65, 64 * 3 + 1)


def sf_layout(size):
    """A layout whose allocation has exactly `size` points."""
    return FieldLayout(3, (size, 1, 1), (0, 0, 0), (0, 0, 0))


def ref_transform_sf(src, size, nent, to_entry_fastest):
    """dst[linear * nent + k] <-> src[k * size + linear]"""
    return (src.reshape(nent, size).T if to_entry_fastest else src.reshape(size, nent).T).ravel().copy()
