"""Cases shared by the CPU and GPU tests of the semilinear entry points (include/examg.h: examg_nl_op, examg_nl_smooth) and of the FAS
programs: stencils, point programs, layouts in which every argument has ghost and pad widths of its own, boxes, and the two example
programs with the knowledge they run under."""
import os

import numpy as np

import stencil_cases as S

from exastencils_amd.field import Stencil
from exastencils_amd.layout import FieldLayout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples", "exa4")
GOLDEN = os.path.join(ROOT, "tests", "golden")

# -- the programs -----------------------------------------------------------------------------------------------------------------
# the decomposition of Testing/NonLinear/FAS_2D_Basic.knowledge (settings only): 9 x 9 fragments of 128^2 cells on level 7, merged
K_BRATU2D = dict(dimensionality=2, minLevel=0, maxLevel=7, domain_rect_generate=True, domain_rect_numBlocks_x=3, domain_rect_numBlocks_y=3,
                 domain_rect_numBlocks_z=1, domain_rect_numFragsPerBlock_x=3, domain_rect_numFragsPerBlock_y=3, domain_rect_numFragsPerBlock_z=1)
K_BRATU3D = dict(dimensionality=3, minLevel=1, maxLevel=5)
# two blocks in x over gloo against one block: 2 x 1 fragments of 16^2 cells on level 4
K_BRATU2D_TWO = dict(dimensionality=2, minLevel=1, maxLevel=4, domain_fragmentLength_x=2, domain_fragmentLength_y=1)


def text(name):
    with open(os.path.join(EX, name)) as f:
        return f.read()


def results_lines():
    with open(os.path.join(GOLDEN, "NonLinear_FAS_2D_Basic.results")) as f:
        return f.read().split()


def own_golden(name):
    import json

    with open(os.path.join(GOLDEN, "own", name + ".json")) as f:
        return json.load(f)


def run(name, k, ops, **kw):
    from exastencils_amd import exa4

    P = exa4.Exa4Program(text(name), dict(k), ops=ops, **kw)
    return P, P.run()


# -- point programs -----------------------------------------------------------------------------------------------------------------
GAMMA = 0.3
# exact class (+ - * / and constants: every operation one IEEE rounding, the same on every machine): c = (gamma u) u, d = ((3 gamma) u) u
EXACT_C = [("const", GAMMA), ("u", None), ("*", None), ("u", None), ("*", None)]
EXACT_D = [("const", 3.0), ("const", GAMMA), ("*", None), ("u", None), ("*", None), ("u", None), ("*", None)]
# libm class: c = gamma exp(u), d = (gamma (1 + u)) exp(u) -- the programs of the Bratu smoother
LIBM_C = [("const", GAMMA), ("u", None), ("exp", None), ("*", None)]
LIBM_D = [("const", GAMMA), ("const", 1.0), ("u", None), ("+", None), ("*", None), ("u", None), ("exp", None), ("*", None)]


def deep_program(depth):
    """`depth` values pushed, then added up."""
    return [("u", None)] * depth + [("+", None)] * (depth - 1)


def long_program(n):
    """n instructions (n odd): u, then (const, +) pairs."""
    return [("u", None)] + [("const", 1.5), ("+", None)] * ((n - 1) // 2)


# -- stencils: asymmetric, all entries distinct and not dyadic, the centre first, in the middle and last ------------------------------
_ORD5 = {"first": ["c", "+x", "-x", "+y", "-y"], "middle": ["-x", "+y", "c", "-y", "+x"], "last": ["+y", "-x", "-y", "+x", "c"]}
_ORD7 = {"first": ["c", "-x", "+x", "-y", "+y", "-z", "+z"], "middle": ["+y", "-z", "+x", "c", "-x", "+z", "-y"],
         "last": ["-z", "+x", "-y", "+z", "+y", "-x", "c"]}
_C5 = {"c": 9.37, "-x": -2.61, "+x": -1.43, "-y": -3.19, "+y": -0.87}
_C7 = {"c": 13.91, "-x": -2.61, "+x": -1.43, "-y": -3.19, "+y": -0.87, "-z": -2.23, "+z": -1.71}


def _full(nd, where):
    """All 3^nd entries of reach 1 with distinct coefficients drawn once, the centre (dominant) at the place `where` names."""
    offs = [(a, b, c) for c in ((-1, 0, 1) if nd == 3 else (0,)) for b in (-1, 0, 1) for a in (-1, 0, 1)]
    rng = np.random.default_rng(90 + nd)
    coef = {o: -float(v) for o, v in zip(offs, rng.uniform(0.1, 1.3, len(offs)))}
    coef[(0, 0, 0)] = 1.1 * sum(-v for o, v in coef.items() if o != (0, 0, 0))
    rest = [offs[i] for i in rng.permutation(len(offs)) if offs[i] != (0, 0, 0)]
    k = {"first": 0, "middle": len(rest) // 2, "last": len(rest)}[where]
    order = rest[:k] + [(0, 0, 0)] + rest[k:]
    st = Stencil(order, [coef[o] for o in order])
    assert len(set(st.coefs)) == len(order) and st.diag_index == k
    return st


def stencil(kind, where):
    """kind: 5, 9 (2-D), 7, 27 (3-D); where: 'first', 'middle', 'last' -- the place of the centre entry."""
    if kind == 5:
        return S.star(_C5, where, _ORD5)
    if kind == 7:
        return S.star(_C7, where, _ORD7)
    return _full(2 if kind == 9 else 3, where)


# -- layouts and boxes ------------------------------------------------------------------------------------------------------------------
def layouts(nd, shape):
    """(lu, lq, lf, ld) on the grid of `shape` cells, each with ghost and pad widths of its own: u one ghost layer, q two and rows
    padded to 16 doubles, rhs none and rows padded to 2, dst one and rows padded to 16."""
    return (FieldLayout.node(nd, shape, 1), FieldLayout.node(nd, shape, 2, align=16), FieldLayout.node(nd, shape, 0, True, False, 2),
            FieldLayout.node(nd, shape, 1, align=16))


# (name, nd, box extents, begin): rows below, at and just over a wave (63, 64, 65) and a second x window with a remainder (130); odd
# begins flip the colour of the first point
BOXES = [
    ("1x1", 2, (1, 1, 1), (1, 1, 0)),
    ("3x2", 2, (3, 2, 1), (2, 1, 0)),
    ("63x3", 2, (63, 3, 1), (1, 1, 0)),
    ("64x3", 2, (64, 3, 1), (1, 2, 0)),
    ("65x5", 2, (65, 5, 1), (3, 1, 0)),
    ("130x4", 2, (130, 4, 1), (1, 1, 0)),
    ("7x5x3", 3, (7, 5, 3), (1, 1, 1)),
    ("65x4x3", 3, (65, 4, 3), (2, 1, 1)),
    ("130x3x2", 3, (130, 3, 2), (1, 3, 2)),
]


def geometry(nd, ext, begin):
    """(cells per dimension, begin, end): the box lies inside the inner points, at least one point from every face."""
    shape = tuple(begin[d] + ext[d] + 1 if d < nd else 0 for d in range(3))
    return shape, list(begin), [begin[d] + ext[d] for d in range(3)]


SENTINEL = -7.0e300


def arrays(ops, lays, seed, lo=-1.0, hi=1.0):
    """One array per layout over the whole allocation, U(lo, hi) from a seeded generator: the same values on every kernel layer."""
    rng = np.random.default_rng(seed)
    return [ops.from_host(rng.uniform(lo, hi, int(l.size))) for l in lays]
