"""Shapes, stencils and data of the complex-field tests (tests/test_complex.py on the CPU, tests/test_gpu_complex.py on the GPU): the smallest
at which the kernels can still go wrong -- rows shorter than a 64-lane window and rows of two full windows plus a remainder, an interior box
with an odd begin, u with a ghost layer and rhs / dst in layouts of their own with other padding, random data everywhere."""
import itertools

import numpy as np

from exastencils_amd.field import Stencil
from exastencils_amd.layout import FieldLayout

# inner sizes (points between the duplicate layers)
SHAPES = {
    "2d_7x5": (2, (7, 5, 1)),
    "2d_131x9": (2, (131, 9, 1)),      # two full 64-lane windows and a remainder
    "3d_5x4x3": (3, (5, 4, 3)),
    "3d_67x6x5": (3, (67, 6, 5)),
}


def layouts(nd, inner):
    """(u with one ghost layer, rhs and dst without ghost layers and with paddings of their own)."""
    ncells = tuple(inner[d] + 1 for d in range(nd))
    lu = FieldLayout.node(nd, ncells, 1)
    dup = tuple(1 if d < nd else 0 for d in range(3))
    zero = (0, 0, 0)
    lf = FieldLayout(nd, tuple(inner), zero, dup, (1, 0, 0), (2, 1, 0))
    ld = FieldLayout(nd, tuple(inner), zero, dup, (3, 2, 1 if nd == 3 else 0), (0, 0, 0))
    return lu, lf, ld


def boxes(nd, inner):
    """The whole field (duplicate points included) and the interior box, whose begin is odd in every dimension."""
    whole = ([0, 0, 0], [inner[d] + 2 if d < nd else 1 for d in range(3)])
    interior = ([1 if d < nd else 0 for d in range(3)], [inner[d] + 1 if d < nd else 1 for d in range(3)])
    return {"whole": whole, "interior": interior}


def _axis(d, s):
    o = [0, 0, 0]
    o[d] = s
    return tuple(o)


def star_offsets(nd, order):
    """Centre first, then per axis (-, +) for order 'mp' or (+, -) for 'pm'; 'mixed': the centre in the middle of the list."""
    signs = (-1, 1) if order != "pm" else (1, -1)
    offs = [(0, 0, 0)] + [_axis(d, s) for d in range(nd) for s in signs]
    if order == "mixed":
        offs = offs[1:3] + [offs[0]] + offs[3:][::-1]
    return offs


def star_stencils(nd):
    """Star stencils in three declared orders, each with the coefficients of the shifted Laplacian (a complex centre, real off-centres: the
    M of the Helmholtz program) and with all entries complex."""
    rng = np.random.default_rng(7 + nd)
    out = {}
    for order in ("mp", "pm", "mixed"):
        offs = star_offsets(nd, order)
        h2 = 1.0 / 0.03125 ** 2
        shifted = [complex(2 * nd * h2 - 400.0, -200.0) if o == (0, 0, 0) else complex(-h2, 0.0) for o in offs]
        allc = [complex(a, b) for a, b in rng.uniform(-2.0, 2.0, (len(offs), 2))]
        allc[offs.index((0, 0, 0))] += 6.0
        out["%s_shifted" % order] = Stencil(offs, shifted)
        out["%s_complex" % order] = Stencil(offs, allc)
    # a real centre: the division of CRELAX takes its real branch
    out["mp_real"] = Stencil(star_offsets(nd, "mp"), [complex(5.0 if o == (0, 0, 0) else -1.25, 0.0) for o in star_offsets(nd, "mp")])
    return out


def gather_stencils(nd):
    """An asymmetric 9-point (2-D) or 27-point (3-D) stencil with complex entries, and a star with an entry missing (no route but gather)."""
    rng = np.random.default_rng(11 + nd)
    offs = [o[::-1] for o in itertools.product((-1, 0, 1), repeat=nd)]
    offs = [tuple(o) + (0,) * (3 - nd) for o in offs]
    rng.shuffle(offs)
    offs = [tuple(int(v) for v in o) for o in offs]
    coefs = [complex(a, b if k % 3 else 0.0) for k, (a, b) in enumerate(rng.uniform(-1.0, 1.0, (len(offs), 2)))]
    coefs[offs.index((0, 0, 0))] += 8.0
    star = star_offsets(nd, "mp")[:-1]
    return {"full": Stencil(offs, coefs), "star_less_one": Stencil(star, [complex(4.0, 1.0)] + [complex(-1.0, 0.5)] * (len(star) - 1))}


def random_field(layout, seed):
    """2 * size doubles, random everywhere: ghost layers and padding included."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, 2 * layout.size)


def integer_field(layout, seed, lo=-7, hi=8):
    return np.random.default_rng(seed).integers(lo, hi, 2 * layout.size).astype(np.float64)


def transfer_layouts(nd, inner_coarse):
    """(fine, coarse) node layouts of a level pair, the fine one with a ghost layer, the coarse one with paddings of its own."""
    nc = tuple(inner_coarse[d] + 1 for d in range(nd))
    lfine = FieldLayout.node(nd, tuple(2 * c for c in nc), 1)
    dup = tuple(1 if d < nd else 0 for d in range(3))
    lc = FieldLayout(nd, tuple(inner_coarse[d] if d < nd else 1 for d in range(3)), (0, 0, 0), dup, (1, 1, 0), (2, 0, 0))
    return lfine, lc


def deinterleave(a):
    return np.ascontiguousarray(a[0::2]), np.ascontiguousarray(a[1::2])
