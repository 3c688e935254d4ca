"""Shapes, stencils and data of the coupled-system tests (tests/test_optflow.py on the CPU, tests/test_gpu_optflow.py on the GPU)."""
from exastencils_amd.field import Stencil
from exastencils_amd.layout import FieldLayout

# (nd, n, cells): two tiles of 64 pairs and a partial one; one tile smaller than a pair run; 3 unknowns in 3-D with an odd row
# count (a workgroup's fifth row) and odd planes; n != nd
SHAPES = [(2, 2, (130, 6)), (2, 2, (4, 4)), (3, 3, (66, 5, 3)), (3, 2, (24, 6, 4))]
H = (1.0 / 8.0, 1.0 / 5.0, 1.0 / 3.0)       # unequal per axis: a swapped axis shows


def laplace(nd, order=0, scale=1.0):
    """5- / 7-point Laplacian with unequal h.  order 0: c, -x, +x, -y, +y [, -z, +z]; order 1: the centre in the middle and the
    axes from the last to the first, upper neighbour first -- the fold order is part of the result."""
    ent = [((0, 0, 0), sum(2.0 / (H[d] * H[d]) for d in range(nd)))]
    for d in range(nd):
        for sgn in (-1, 1):
            o = [0, 0, 0]
            o[d] = sgn
            ent.append((tuple(o), -1.0 / (H[d] * H[d])))
    if order == 1:
        rest = ent[1:][::-1]
        ent = rest[:nd] + [ent[0]] + rest[nd:]
    return Stencil([o for o, _ in ent], [scale * c for _, c in ent])


def boxes(nd, cells):
    """The whole field, and an interior box with odd begin in x and y: which cell of a pair carries the colour flips, and both ends
    of a row are partial pairs."""
    n = list(cells) + [1] * (3 - nd)
    full = ([0, 0, 0], n)
    inner = ([1, 1, 1 if nd == 3 else 0], [n[0] - 2, n[1] - 1, n[2] - 1 if nd == 3 else 1])
    return {"full": full, "interior": inner}


def layouts(nd, cells, align, ghost_other=1):
    """u with one ghost layer; rhs, coefficients and destination in a layout of their own (ghost_other)."""
    lu = FieldLayout.cell(nd, cells, 1, align=align)
    lo = FieldLayout.cell(nd, cells, ghost_other, align=align)
    return lu, lo


class SysData:
    """Arrays of one system on a kernel layer: random values everywhere, ghost layers and padding included.  The coefficient fields
    lie in (-1, 1) and the stencil centre (>= 178) is added to the diagonal: every cell's matrix is diagonally dominant."""

    def __init__(self, ops, n, lu, lo, pattern="full"):
        self.n, self.lu, self.lo = n, lu, lo
        seed = [100]

        def arr(l):
            t = ops.new_array(l.size)
            seed[0] += 1
            ops.fill_random(t, seed[0])
            return t

        self.u = [arr(lu) for _ in range(n)]
        self.f = [arr(lo) for _ in range(n)]
        self.dst = [arr(lo) for _ in range(n)]
        self.g = [[arr(lo) for _ in range(n)] for _ in range(n)]
        if pattern == "alias":           # uvSten and vuSten both name IxIy
            for c in range(n):
                for d in range(c):
                    self.g[c][d] = self.g[d][c]
        elif pattern == "null":          # no term off the diagonal in the first row, none on the diagonal of the last
            self.g[0][1] = None
            self.g[n - 1][n - 1] = None

    def arrays(self):
        return self.u + self.f + self.dst + [t for row in self.g for t in row if t is not None]
