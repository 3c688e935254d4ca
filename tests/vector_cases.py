"""Shapes, matrix stencils and data of the tests of vector-valued cell fields (tests/test_vector.py on the CPU, tests/test_gpu_vector.py
on the GPU).  Shapes, boxes and layouts are those of the coupled-system tests (tests/system_cases.py)."""
from exastencils_amd.field import MatrixStencil
from system_cases import SHAPES, boxes, laplace, layouts  # noqa: F401

# the centre matrix: every element a field; off-diagonal fields aliased (IxIy twice); constant + field on the diagonal, constants off
# it; an element absent (and a diagonal element of an off-centre entry, and a diagonal centre element without field)
PATTERNS = ["fields", "alias", "kplusg", "absent"]
ORDERS = [0, 1]


def comp_scale(c):
    """Off-centre and centre constants differ per component."""
    return 1.0 + 0.25 * c


class VecData:
    """Arrays of one vector problem on a kernel layer: random values everywhere, ghost layers and padding included.  Coefficient fields lie
    in (-1, 1); the diagonal of the centre matrix carries the Laplacian's centre (>= 178), as a constant or -- pattern "fields" -- added
    to the diagonal fields: every cell's matrix is diagonally dominant, its diagonal ~2e2."""

    def __init__(self, ops, nd, n, lu, lo, pattern="fields", order=0):
        self.n, self.lu, self.lo = n, lu, lo
        seed = [200]

        def arr(l, ncomp=1, shift=0.0):
            t = ops.new_array(ncomp * l.size)
            seed[0] += 1
            ops.fill_random(t, seed[0])
            if shift:
                t = ops.from_host(ops.to_host(t).copy() + shift)
            return t

        self.u = arr(lu, n)
        self.f = arr(lo, n)
        self.dst = arr(lo, n)
        L = laplace(nd, order)
        centre = float(L.coefs[L.diag_index])
        self.coef = []
        elems = []
        for off, cf in zip(L.offsets, L.coefs):
            m = [[None] * n for _ in range(n)]
            if tuple(off) != (0, 0, 0):
                for c in range(n):
                    m[c][c] = (float(cf) * comp_scale(c), None)
                if pattern == "absent" and len(elems) == 1:
                    m[0][0] = None                      # component 0 has no term at this neighbour
                elems.append(m)
                continue
            for c in range(n):
                for d in range(n):
                    if pattern == "fields":
                        g = arr(lo, 1, centre * comp_scale(c) if c == d else 0.0)
                        m[c][d] = (None, g)
                    elif c == d:
                        m[c][d] = (centre * comp_scale(c), arr(lo))
                    elif pattern == "kplusg":
                        m[c][d] = (0.25 * (c - d), None)
                    elif pattern == "alias" and d < c:
                        m[c][d] = m[d][c]
                    else:
                        m[c][d] = (None, arr(lo))
            if pattern == "absent":
                m[0][1] = None
                m[n - 1][n - 1] = (centre * comp_scale(n - 1), None)
            for row in m:
                self.coef += [el[1] for el in row if el is not None and el[1] is not None]
            elems.append(m)
        self.M = MatrixStencil(n, [tuple(o) for o in L.offsets], elems, lo)

    def arrays(self):
        seen, out = set(), []
        for t in [self.u, self.f, self.dst] + self.coef:
            if id(t) not in seen:
                seen.add(id(t))
                out.append(t)
        return out
