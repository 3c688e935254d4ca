"""Shapes, block patterns and data of the block-system tests (tests/test_blocksys.py on the CPU, tests/test_gpu_blocksys.py on the GPU)."""
import itertools
import math

from exastencils_amd.field import Colouring, Stencil
from exastencils_amd.layout import FieldLayout

# (nd, n, inner nodes): 2-D narrower than a wave with fewer rows than a wave's lanes wrap around; one wave plus a remainder of 3; two
# waves and a remainder in few rows; the same in 3-D with odd plane counts.  Inner nodes + 2 duplicate points per axis = the field.
SHAPES = [(2, 2, (5, 3)), (2, 2, (67, 9)), (2, 2, (130, 6)), (3, 3, (5, 4, 3)), (3, 3, (67, 5, 4)), (3, 3, (33, 9, 7))]
H = (1.0 / 8.0, 1.0 / 5.0, 1.0 / 3.0)       # unequal per axis: a swapped axis shows
LAMBDA, MU = 195.0, 130.0


def _axis(d, s):
    o = [0, 0, 0]
    o[d] = s
    return tuple(o)


def second(d, scale=1.0):
    """d^2/dx_d^2: centre, lower, upper."""
    return Stencil([(0, 0, 0), _axis(d, -1), _axis(d, 1)], [scale * -2.0 / (H[d] * H[d]), scale / (H[d] * H[d]), scale / (H[d] * H[d])])


def mixed(d, e, scale=1.0):
    """d^2/dx_d dx_e: the four diagonal neighbours in the (d, e) plane, no centre."""
    offs, co = [], []
    for s, t, sign in ((-1, 1, -1.0), (1, 1, 1.0), (-1, -1, 1.0), (1, -1, -1.0)):
        o = [0, 0, 0]
        o[d], o[e] = s, t
        offs.append(tuple(o))
        co.append(scale * sign / (4.0 * H[d] * H[e]))
    return Stencil(offs, co)


def laplace(nd, scale=1.0):
    offs, co = [(0, 0, 0)], [None]
    c = None
    for d in range(nd):
        t = -2.0 / (H[d] * H[d])
        c = t if c is None else c + t
        for s in (-1, 1):
            offs.append(_axis(d, s))
            co.append(scale * 1.0 / (H[d] * H[d]))
    co[0] = scale * c
    return Stencil(offs, co)


def merged(a, b):
    """Host stencil arithmetic (include/examg.h): b added into a, an offset already present gets c_old + c_new, a new one is appended."""
    offs, co = list(a.offsets), list(a.coefs)
    for o, c in zip(b.offsets, b.coefs):
        if o in offs:
            co[offs.index(o)] = co[offs.index(o)] + c
        else:
            offs.append(o)
            co.append(c)
    return Stencil(offs, co)


def full_stencil(nd, seed, centre_at=4, big=True):
    """Every offset of {-1, 0, 1}^nd with distinct irrational-looking coefficients, the centre (big on the diagonal of the table: the
    local systems stay regular) at position `centre_at` of the list."""
    offs = [o + (0,) * (3 - nd) for o in itertools.product((-1, 0, 1), repeat=nd)]
    offs = [tuple(reversed(o[:nd])) + o[nd:] for o in offs]
    offs.remove((0, 0, 0))
    offs.insert(centre_at, (0, 0, 0))
    co = [math.sin(1.0 + 0.37 * seed + 0.61 * k) * math.sqrt(2.0 + k) for k in range(len(offs))]
    co[centre_at] = (40.0 if big else 2.5) + 3.0 * math.sqrt(1.0 + seed)
    return Stencil(offs, co)


def star_stencil(nd, seed):
    """Centre in the middle, then the axis neighbours: what the parity of all indices decouples."""
    offs = [_axis(d, s) for d in range(nd) for s in (1, -1)]
    offs.insert(nd, (0, 0, 0))
    co = [math.cos(0.3 + 0.53 * seed + 0.71 * k) * math.sqrt(3.0 + k) for k in range(len(offs))]
    co[nd] = 30.0 + math.sqrt(2.0 + seed)
    return Stencil(offs, co)


def blocks(pattern, nd, n):
    """The n x n table of a block pattern (rows of n; None: no block)."""
    if pattern == "elasticity":          # row c: (lambda + mu) * sum_d d_cd * u_d + lambda * Laplace * u_c, the two terms on u_c merged
        assert n == nd
        A = [[None] * n for _ in range(n)]
        for c in range(n):
            for d in range(n):
                A[c][d] = mixed(min(c, d), max(c, d), LAMBDA + MU) if c != d else merged(second(c, LAMBDA + MU), laplace(nd, LAMBDA))
        return A
    if pattern == "dense":
        return [[full_stencil(nd, 7 * c + d, 4 if c == d else 2 + c + d, c == d) for d in range(n)] for c in range(n)]
    if pattern == "sparse":              # one off-diagonal block missing, one block without a centre
        A = [[full_stencil(nd, 3 * c + d, 3, c == d) for d in range(n)] for c in range(n)]
        A[0][1] = None
        A[n - 1][0] = mixed(0, 1, 0.5)
        return A
    if pattern == "asymmetric":          # A_01 != A_10: a transposed table shows
        A = [[star_stencil(nd, 5 * c + d) for d in range(n)] for c in range(n)]
        A[0][1] = mixed(0, 1, 2.0)
        A[1][0] = Stencil([(1, 0, 0), (0, 0, 0), (0, -1, 0)], [0.75, -1.25, math.sqrt(0.5)])
        return A
    if pattern == "stars":               # every block a star: the all-index parity decouples the system
        return [[star_stencil(nd, 11 * c + d) for d in range(n)] for c in range(n)]
    raise ValueError(pattern)


PATTERNS = ["elasticity", "dense", "sparse", "asymmetric"]


def layouts(nd, inner, ghost_other):
    """u with one ghost layer; rhs and destination in a layout of their own (ghost_other: 1 equal widths, 0 no ghost layers)."""
    cells = [i + 1 for i in inner]
    return FieldLayout.node(nd, cells, 1), FieldLayout.node(nd, cells, ghost_other)


def boxes(nd, inner):
    """All inner points (iterator coordinates 1 .. inner); an interior box shrunk by one on the low and two on the high side of every
    axis (where the field is too small for that: as far as one point is left); a single point."""
    n = list(inner) + [1] * (3 - nd)
    lo = [1 if d < nd else 0 for d in range(3)]
    hi = [1 + n[d] if d < nd else 1 for d in range(3)]
    ib = [lo[d] + 1 if d < nd else 0 for d in range(3)]
    ie = [max(hi[d] - 2, ib[d] + 1) if d < nd else 1 for d in range(3)]
    ie = [min(ie[d], hi[d]) for d in range(3)]
    ib = [min(ib[d], ie[d] - 1) for d in range(3)]
    pt = [lo[d] + (n[d] // 2 if d < nd else 0) for d in range(3)]
    return {"inner": (lo, hi), "interior": (ib, ie), "point": (pt, [p + 1 for p in pt])}


def colouring(nd, kind):
    if kind == "axes":
        return Colouring.axis_parity(nd)
    return Colouring(((tuple(range(nd)), 0, 2),))      # the parity of all indices


class BsysData:
    """Arrays of one system on a kernel layer: random doubles from a fixed seed everywhere, ghost layers and padding included."""

    def __init__(self, ops, n, lu, lo):
        self.n, self.lu, self.lo = n, lu, lo
        seed = [300]

        def arr(l):
            t = ops.new_array(l.size)
            seed[0] += 1
            ops.fill_random(t, seed[0])
            return t

        self.u = [arr(lu) for _ in range(n)]
        self.f = [arr(lo) for _ in range(n)]
        self.dst = [arr(lo) for _ in range(n)]

    def arrays(self):
        return self.u + self.f + self.dst
