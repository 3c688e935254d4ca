"""TEST-ONLY restatement of what the 5-point benchmark adds to the cell entry points (include/examg.h: the EXAMG_BC_VALUE_MINUS kind of
examg_apply_bc_cell, examg_apply_bc_cell_faces, the EXAMG_OP_NODE_* operands) in numpy, on top of the cell restatement
(tests/cell_ops.py).  One IEEE operation per instruction; what the library refuses raises ValueError here."""
import numpy as np

from cell_ops import CellOracleOps, _sl, _view

BC_DIRICHLET, BC_NEUMANN, BC_NEGATE, BC_VALUE_MINUS = 0, 1, 2, 4      # EXAMG_BC_* of include/examg.h
_NODE = ("nx", "ny", "nz")


def eval_ghost_program(prog, centre, node):
    """A point program at cells with the centres `centre` and the nodes of their own index `node` (three arrays each)."""
    un = {"neg": np.negative, "sin": np.sin, "cos": np.cos, "exp": np.exp, "sinh": np.sinh, "cosh": np.cosh, "sqrt": np.sqrt,
          "tan": np.tan, "log": np.log, "fabs": np.abs, "tanh": np.tanh}
    bi = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide, "pow": np.power, "max": np.maximum, "min": np.minimum}
    st = []
    for name, c in prog:
        if name == "const":
            st.append(np.full(centre[0].shape, float(c)))
        elif name in ("x", "y", "z"):
            st.append(np.array(centre["xyz".index(name)], dtype=np.float64))
        elif name in _NODE:
            st.append(np.array(node[_NODE.index(name)], dtype=np.float64))
        elif name in un:
            st[-1] = un[name](st[-1])
        elif name in bi:
            b = st.pop()
            st[-1] = bi[name](st[-1], b)
        else:
            raise ValueError("examg expression: unknown opcode %r" % name)
    if len(st) != 1:
        raise ValueError("examg expression: must leave exactly one value")
    return st[0]


class Star2dOracleOps(CellOracleOps):
    name = "star2d-oracle"

    def _one_face(self, l, x, geom, kind, expr, d, side):
        if kind not in (BC_DIRICHLET, BC_NEUMANN, BC_NEGATE, BC_VALUE_MINUS):
            raise ValueError("unknown kind %d" % kind)
        if (l.ghost_r[d] if side else l.ghost_l[d]) < 1:
            raise ValueError("face %d of dim %d has no ghost layer" % (side, d))
        if kind in (BC_DIRICHLET, BC_NEUMANN):
            if kind == BC_DIRICHLET and any(name in _NODE for name, _ in expr.program):
                raise ValueError("examg expression: unknown opcode")
            return CellOracleOps.apply_bc_cell(self, l, x, geom, kind, expr, 1 << (2 * d + side))
        a, ref = _view(l, x)
        b, e = [0, 0, 0], [1, 1, 1]
        for t in range(l.nd):
            b[t], e[t] = 0, l.inner[t]
        if side == 0:
            e[d] = 1
        else:
            b[d] = l.inner[d] - 1
        gb, ge = list(b), list(e)
        gb[d] += 1 if side else -1
        ge[d] += 1 if side else -1
        interior = a[_sl(ref, b, e)].copy()
        if kind == BC_NEGATE:
            a[_sl(ref, gb, ge)] = -interior
            return
        # g at the ghost cell itself: its centre (i * h + pos_begin) + 0.5 * h, the node of its own index i * h + pos_begin
        i2, i1, i0 = np.meshgrid(np.arange(gb[2], ge[2]), np.arange(gb[1], ge[1]), np.arange(gb[0], ge[0]), indexing="ij")
        node = [i * geom.h[t] + geom.pos_begin[t] for t, i in enumerate((i0, i1, i2))]
        centre = [node[t] + 0.5 * geom.h[t] for t in range(3)]
        with np.errstate(all="ignore"):
            a[_sl(ref, gb, ge)] = eval_ghost_program(expr.program, centre, node) - interior

    def apply_bc_cell(self, l, x, geom, kind, expr, face_mask):
        for d in range(l.nd):
            for side in (0, 1):
                if face_mask & (1 << (2 * d + side)):
                    self._one_face(l, x, geom, kind, expr, d, side)

    def apply_bc_cell_faces(self, l, x, geom, faces, face_mask):
        """faces[2 * d + side] = (kind, expr): every face of the mask with its own kind and program."""
        for d in range(l.nd):
            for side in (0, 1):
                f = 2 * d + side
                if face_mask & (1 << f):
                    if f >= len(faces) or faces[f] is None:
                        raise ValueError("face %d of the mask has no entry" % f)
                    self._one_face(l, x, geom, faces[f][0], faces[f][1], d, side)
