"""Axis-aligned grids of one block: node-position tables per axis and level, and stencils written over the virtual fields of the grid.

Reference: Compiler/src/exastencils/grid/ -- `grid_isUniform`, `grid_isAxisAligned`, `grid_spacingModel` (config/Knowledge.scala); the
node positions of an axis-aligned grid are one array per axis (IR_VF_NodePositionPerDim), set up on the finest level by a spacing model
(grid/ir/IR_SetupNodePositions.scala:128-239, `linearFct`) and restricted to the coarser levels by taking every second node (:476-550);
two ghost nodes per side are linear extrapolations.  Cell widths, cell centres and cell volumes are evaluated from the node positions
(grid/ir/IR_VF_CellWidth.scala, IR_VF_CellCenter.scala, IR_VF_CellVolume.scala).

A stencil over these virtual fields (`vf_cellWidth_x@[-1, 0, 0]`, Examples/Poisson/3D_FV_Poisson_fromL4.exa4:39-58) depends on the
position through one-dimensional tables only.  `separate` splits every entry into terms X[i0] * ((s * Z[i2]) * Y[i1]) and returns an
AxisStencil, the host form of examg_axis_stencil_t (include/examg.h)."""
from __future__ import annotations

import re
from dataclasses import dataclass, field as _dcf
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .exa4_parser import Exa4Unsupported

GHOST = 2                       # ghost nodes per side of every node table
MAX_TERMS = 32                  # EXAMG_AXIS_MAX_TERMS
MIN_CELLS = 8                   # linearFct: N / 4 - 1 must not be negative, and every zone holds a cell
_REFUSED_MODELS = ("diego", "diego2", "blockstructured")

_VF_AXIS = re.compile(r"^vf_(cellWidth|nodePosition|nodePos|cellCenter|cellCentre|gridWidth)_([xyz])$")
CELL_VOLUME = "vf_cellVolume"


def extrapolate_ghosts(x: np.ndarray) -> np.ndarray:
    """x[GHOST .. -GHOST) are set; the two ghost nodes of each side by linear extrapolation, the inner one first:
    x[-1] = 2 * x[0] - x[1], then x[-2] = 2 * x[-1] - x[0] (IR_SetupNodePositions.scala:190-213)."""
    g = GHOST
    x[g - 1] = 2.0 * x[g] - x[g + 1]
    x[g - 2] = 2.0 * x[g - 1] - x[g]
    x[-g] = 2.0 * x[-g - 1] - x[-g - 2]
    x[-g + 1] = 2.0 * x[-g] - x[-g - 1]
    return x


def uniform_nodes(n: int, lo: float, hi: float) -> np.ndarray:
    """index * h + begin, h = (hi - lo) / n (grid/ir/IR_VF_NodePosition.scala:109-111), ghost nodes by the same formula."""
    h = (hi - lo) / n
    i = np.arange(-GHOST, n + GHOST + 1, dtype=np.float64)
    return i * h + lo


def linear_fct_nodes(n: int, lo: float, hi: float) -> np.ndarray:
    """`grid_spacingModel = "linearFct"` for an axis of n cells (all fragments together) on [lo, hi]: n + 1 nodes and GHOST ghost nodes
    per side; element j is node j - GHOST.  Three zones: the widths grow linearly up to node xf + 1, stay constant up to node xs + 1 and
    shrink linearly from there (IR_SetupNodePositions.scala:137-157, 222-231).  Every operation in double, in the order written here:
    products and sums left to right."""
    if n < MIN_CELLS:
        raise Exa4Unsupported("grid_spacingModel linearFct needs at least %d cells per axis on the finest level (%d)" % (MIN_CELLS, n))
    nf = float(n)
    xf = float(n // 4 - 1)
    xs = float((n // 4) * 3)
    a_coeff = -0.5 * xf * xf - 0.5 * xf + xf * nf - 0.5 * nf * nf + 0.5 * nf + nf * xs - 0.5 * xs * xs - 0.5 * xs
    factor = (n // 4) / 8.0
    alpha = (hi - lo) / (a_coeff + nf * factor)
    beta = factor * alpha
    x = np.zeros(n + 1 + 2 * GHOST)
    for i in range(n + 1):
        fi = float(i)
        if fi <= xf + 1:
            v = lo + 0.5 * alpha * fi * fi + (beta - 0.5 * alpha) * fi
        elif fi <= xs + 1:
            v = lo - 0.5 * alpha * (xf * xf + xf) + (beta + alpha * xf) * fi
        else:
            v = lo - 0.5 * alpha * fi * fi + (alpha * xf + alpha * xs + 0.5 * alpha + beta) * fi - 0.5 * alpha * (xf * xf + xf + xs * xs + xs)
        x[i + GHOST] = v
    return extrapolate_ghosts(x)


def coarsen_nodes(fine: np.ndarray) -> np.ndarray:
    """Every second node of the next finer level, then the ghost extrapolation (for_AA_restrictFromFiner, :476-550)."""
    n = (len(fine) - 1 - 2 * GHOST) // 2
    x = np.zeros(n + 1 + 2 * GHOST)
    x[GHOST:GHOST + n + 1] = fine[GHOST:len(fine) - GHOST:2]
    return extrapolate_ghosts(x)


class AxisGrid:
    """The node tables of one block: nodes(level, d)[j] is the position of node j - GHOST of axis d."""

    def __init__(self, nd: int, lo: Sequence[float], hi: Sequence[float], cells_finest: Sequence[int], min_level: int, max_level: int,
                 model: str = "uniform"):
        self.nd, self.model, self.min_level, self.max_level = nd, model, min_level, max_level
        self.uniform = model == "uniform"
        self._nodes: Dict[Tuple[int, int], np.ndarray] = {}
        self._dev: Dict[Tuple[int, int], object] = {}
        for d in range(nd):
            n = int(cells_finest[d])
            if n % (1 << (max_level - min_level)) != 0:
                raise Exa4Unsupported("axis %s: %d cells on level %d do not coarsen to level %d" % ("xyz"[d], n, max_level, min_level))
            x = uniform_nodes(n, float(lo[d]), float(hi[d])) if self.uniform else linear_fct_nodes(n, float(lo[d]), float(hi[d]))
            for lvl in range(max_level, min_level - 1, -1):
                if lvl < max_level:
                    n //= 2
                    x = uniform_nodes(n, float(lo[d]), float(hi[d])) if self.uniform else coarsen_nodes(x)
                self._nodes[(lvl, d)] = x

    @staticmethod
    def from_nodes(nd: int, nodes: Dict[Tuple[int, int], np.ndarray]) -> "AxisGrid":
        """A grid from given node tables, nodes[(level, axis)] with GHOST ghost nodes per side (tests, tools)."""
        g = AxisGrid.__new__(AxisGrid)
        g.nd, g.model, g.uniform, g._dev = nd, "tables", False, {}
        g._nodes = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in nodes.items()}
        g.min_level, g.max_level = min(k[0] for k in nodes), max(k[0] for k in nodes)
        return g

    @staticmethod
    def from_knowledge(k: Dict, nd: int, lo, hi, cells_finest, min_level: int, max_level: int, blocks: int = 1,
                       periodic: Sequence[bool] = (False, False, False)) -> Optional["AxisGrid"]:
        """The tables of the non-uniform grid the knowledge file describes, None for a uniform grid, or the refusal that names what is
        not built."""
        uniform = bool(k.get("grid_isUniform", True))
        model = str(k.get("grid_spacingModel", "uniform"))
        if not bool(k.get("grid_isAxisAligned", True)):
            raise Exa4Unsupported("grid_isAxisAligned = false: grids that are not axis-aligned")
        if model in _REFUSED_MODELS:
            raise Exa4Unsupported("grid_spacingModel %r" % model)
        if uniform or model == "uniform":
            return None           # today's positions: index * h + begin, no tables
        if model != "linearFct":
            raise Exa4Unsupported("grid_spacingModel %r" % model)
        if blocks != 1:
            raise Exa4Unsupported("a non-uniform grid on %d blocks (one block only)" % blocks)
        if any(periodic[:nd]):
            raise Exa4Unsupported("a non-uniform grid with a periodic axis")
        return AxisGrid(nd, lo, hi, cells_finest, min_level, max_level, "linearFct")

    def ncells(self, lvl: int, d: int) -> int:
        return len(self._nodes[(lvl, d)]) - 1 - 2 * GHOST

    def nodes(self, lvl: int, d: int) -> np.ndarray:
        return self._nodes[(lvl, d)]

    def widths(self, lvl: int, d: int) -> np.ndarray:
        """vf_cellWidth_d: element j is the width of cell j - GHOST, x[i + 1] - x[i]."""
        x = self._nodes[(lvl, d)]
        return x[1:] - x[:-1]

    def axis_values(self, kind: str, lvl: int, d: int, shift: int) -> np.ndarray:
        """The virtual field `kind` of axis d at the iterator indices shift .. ncells + shift: one value per node index of the level."""
        n, g = self.ncells(lvl, d), GHOST
        x = self._nodes[(lvl, d)]
        if abs(shift) > 1:
            raise Exa4Unsupported("offset %d on a virtual field of the grid (reach above 1)" % shift)
        lo = g + shift
        if kind == "cellWidth":
            return x[lo + 1:lo + n + 2] - x[lo:lo + n + 1]
        if kind in ("nodePosition", "nodePos"):
            return x[lo:lo + n + 1].copy()
        if kind in ("cellCenter", "cellCentre"):
            return 0.5 * (x[lo + 1:lo + n + 2] + x[lo:lo + n + 1])
        raise Exa4Unsupported("vf_%s_%s on a non-uniform grid" % (kind, "xyz"[d]))

    def device(self, ops, lvl: int):
        """examg_grid_t of a level: the three node tables on the device of the kernel layer `ops`, allocated once."""
        from .lib import GridC

        key = (id(ops), lvl)
        if key not in self._dev:
            g = GridC()
            keep = []
            for d in range(3):
                if d < self.nd:
                    t = ops.from_host(np.ascontiguousarray(self._nodes[(lvl, d)]))
                    keep.append(t)
                    g.nodes[d] = ops.ptr(t)
                    g.n[d] = len(self._nodes[(lvl, d)])
                else:
                    g.nodes[d] = None
                    g.n[d] = 0
            g.ghost = GHOST
            g._keep = keep
            self._dev[key] = g
        return self._dev[key]


# =====================================================================================================================
# stencils over the virtual fields: separation into per-axis tables
# =====================================================================================================================
@dataclass
class AxisStencil:
    """Host form of examg_axis_stencil_t.  terms: (entry, s, (tx, ty, tz)) sorted by entry; tables[d]: the distinct tables of axis d, each
    over the iterator indices tab_begin[d] .. tab_begin[d] + len."""
    offsets: List[Tuple[int, int, int]]
    terms: List[Tuple[int, float, Tuple[int, int, int]]]
    tables: List[List[np.ndarray]]
    tab_begin: Tuple[int, int, int] = (0, 0, 0)
    wform: int = 0
    _dev: Dict[int, object] = _dcf(default_factory=dict, repr=False, compare=False)

    cfield = None               # not a stencil field, and not a constant stencil either: is_axis says so
    is_axis = True

    @property
    def diag_index(self) -> int:
        return self.offsets.index((0, 0, 0))

    @property
    def faces_only(self) -> bool:
        return all(sum(1 for c in o if c != 0) <= 1 for o in self.offsets)

    def with_wform(self, wform: int) -> "AxisStencil":
        return AxisStencil(self.offsets, self.terms, self.tables, self.tab_begin, wform, self._dev)

    def table_array(self, d: int) -> np.ndarray:
        """The tables of axis d as one (ntab, len) array."""
        if not self.tables[d]:
            return np.zeros((0, 0))
        return np.ascontiguousarray(np.stack(self.tables[d]))

    def coefficients(self, begin, end) -> List[np.ndarray]:
        """The coefficient of every entry on the box, (z, y, x) arrays, in the arithmetic order of examg_axis_op."""
        out: List[Optional[np.ndarray]] = [None] * len(self.offsets)
        sl = [slice(begin[d] - self.tab_begin[d], end[d] - self.tab_begin[d]) for d in range(3)]
        for e, s, tab in self.terms:
            X = self.tables[0][tab[0]][sl[0]] if tab[0] >= 0 else np.ones(end[0] - begin[0])
            Y = self.tables[1][tab[1]][sl[1]] if tab[1] >= 0 else np.ones(end[1] - begin[1])
            Z = self.tables[2][tab[2]][sl[2]] if tab[2] >= 0 else np.ones(end[2] - begin[2])
            c = X[None, None, :] * ((float(s) * Z)[:, None, None] * Y[None, :, None])
            out[e] = c if out[e] is None else out[e] + c
        return out

    def c_struct(self, ops):
        """examg_axis_stencil_t with the tables on the device of `ops` (uploaded once per kernel layer)."""
        from .lib import AXIS_MAX_TERMS, AxisStencilC

        if len(self.terms) > AXIS_MAX_TERMS:
            raise ValueError("%d terms (limit %d)" % (len(self.terms), AXIS_MAX_TERMS))
        key = id(ops)
        if key not in self._dev:
            self._dev[key] = [ops.from_host(self.table_array(d).reshape(-1).copy()) if self.tables[d] else None for d in range(3)]
        dev = self._dev[key]
        s = AxisStencilC()
        s.nent = len(self.offsets)
        s.diag = self.diag_index if (0, 0, 0) in self.offsets else -1
        for k, o in enumerate(self.offsets):
            for d in range(3):
                s.off[k][d] = o[d]
        s.wform = int(self.wform)
        s.nterm = len(self.terms)
        for t, (e, sv, tab) in enumerate(self.terms):
            s.term[t].entry = int(e)
            s.term[t].s = float(sv)
            for d in range(3):
                s.term[t].tab[d] = int(tab[d])
        for d in range(3):
            s.tables[d] = ops.ptr(dev[d]) if dev[d] is not None else None
            s.ntab[d] = len(self.tables[d])
            s.tab_begin[d] = int(self.tab_begin[d])
            s.tab_len[d] = len(self.tables[d][0]) if self.tables[d] else 0
        s.route = 0
        return s


def _axes_of(e, nd: int, name: str) -> set:
    """The axes an expression depends on through the virtual fields of the grid; a field access is refused."""
    axes = set()
    stack = [e]
    while stack:
        n = stack.pop()
        if not isinstance(n, tuple) or not n:
            continue
        if n[0] in ("fld", "sten", "sentry"):
            raise Exa4Unsupported("stencil %s: a field in an entry of a stencil over the grid's virtual fields" % name)
        if n[0] in ("id", "vfo") and isinstance(n[1], str):
            m = _VF_AXIS.match(n[1])
            if m:
                axes.add("xyz".index(m.group(2)))
            elif n[1] == CELL_VOLUME:
                axes.update(range(nd))
        for c in n[1:]:
            if isinstance(c, tuple):
                stack.append(c)
            elif isinstance(c, list):
                stack.extend(x for x in c if isinstance(x, tuple))
    return axes


def _split_terms(e, sign: float, out: list):
    """The terms of an entry: split at its top-level `+` / `-`; (sign, expression)."""
    if e[0] == "bin" and e[1] in ("+", "-"):
        _split_terms(e[2], sign, out)
        _split_terms(e[3], sign if e[1] == "+" else -sign, out)
    else:
        out.append((sign, e))


def _flatten(e, den: bool, out: list, nd: int) -> float:
    """A term flattened over `*`, `/` and unary minus: (factor, in the denominator) in written order; returns the sign.  `vf_cellVolume` is
    the product of the widths of the point's cell and flattens into them."""
    if e[0] == "bin" and e[1] == "*":
        return _flatten(e[2], den, out, nd) * _flatten(e[3], den, out, nd)
    if e[0] == "bin" and e[1] == "/":
        sign = _flatten(e[2], den, out, nd)
        if len(_axes_of(e[3], nd, "")) <= 1:      # a divisor over one axis is one factor: `0.5 * ( w@[0] + w@[-1] )`
            out.append((e[3], not den))
            return sign
        return sign * _flatten(e[3], not den, out, nd)
    if e[0] == "neg":
        return -_flatten(e[1], den, out, nd)
    if e[0] in ("id", "vfo") and e[1] == CELL_VOLUME:
        off = e[3] if e[0] == "vfo" else None
        for d in range(nd):
            w = ("id", "vf_cellWidth_" + "xyz"[d], e[2])
            out.append((w if off is None else ("vfo",) + w[1:] + (off,), den))
        return 1.0
    out.append((e, den))
    return 1.0


def separate(name: str, entries, nd: int, lvl: int, grid: AxisGrid, eval_scalar: Callable) -> AxisStencil:
    """The stencil `name` (entries: (offset, expression) in declared order) on level lvl of a non-uniform grid as an AxisStencil.
    eval_scalar(expression) -> float evaluates a factor that depends on no axis (literals, globals, PI).
    Per term and axis: T = (the axis's numerator factors multiplied in written order) / (its denominator factors multiplied in written
    order), one value per iterator index, in double; scalar factors fold the same way into s, and the term's sign multiplies s last."""
    offsets = [tuple(o) + (0,) * (3 - len(o)) for o, _ in entries]
    for o in offsets:
        if any(abs(c) > 1 for c in o):
            raise Exa4Unsupported("stencil %s: entry %s over the grid's virtual fields reaches above 1" % (name, list(o)))
    tables: List[List[np.ndarray]] = [[], [], []]
    keys: List[Dict[bytes, int]] = [{}, {}, {}]
    terms = []
    for k, (_, expr) in enumerate(entries):
        split: list = []
        _split_terms(expr, 1.0, split)
        for sign, te in split:
            factors: list = []
            sign = sign * _flatten(te, False, factors, nd)
            num: List[Optional[object]] = [None] * 4      # axis 0 .. 2, 3: scalars
            den: List[Optional[object]] = [None] * 4
            for f, in_den in factors:
                axes = _axes_of(f, nd, name)
                if len(axes) > 1:
                    raise Exa4Unsupported("stencil %s: factor over %s is not separable" % (name, " and ".join("xyz"[a] for a in sorted(axes))))
                a = axes.pop() if axes else 3
                v = float(eval_scalar(f)) if a == 3 else _eval_axis(f, a, lvl, grid, eval_scalar, name)
                side = den if in_den else num
                side[a] = v if side[a] is None else side[a] * v
            tab = [-1, -1, -1]
            for a in range(3):
                if num[a] is None and den[a] is None:
                    continue
                t = (num[a] if num[a] is not None else 1.0) / den[a] if den[a] is not None else num[a]
                t = np.ascontiguousarray(np.broadcast_to(t, (grid.ncells(lvl, a) + 1,)), dtype=np.float64)
                key = t.tobytes()
                if key not in keys[a]:
                    keys[a][key] = len(tables[a])
                    tables[a].append(t)
                tab[a] = keys[a][key]
            s = (num[3] if num[3] is not None else 1.0) / den[3] if den[3] is not None else (num[3] if num[3] is not None else 1.0)
            terms.append((k, sign * s, tuple(tab)))
    if len(terms) > MAX_TERMS:
        raise Exa4Unsupported("stencil %s: %d terms over the grid's virtual fields (at most %d)" % (name, len(terms), MAX_TERMS))
    return AxisStencil(offsets, terms, tables)


def _eval_axis(e, a: int, lvl: int, grid: AxisGrid, eval_scalar: Callable, name: str):
    """A single-axis factor at every iterator index of axis a: numpy evaluates each operation of the tree in double, in its order."""
    k = e[0]
    if k == "num":
        return float(e[1])
    if k == "neg":
        return -_eval_axis(e[1], a, lvl, grid, eval_scalar, name)
    if k in ("id", "vfo"):
        m = _VF_AXIS.match(e[1]) if isinstance(e[1], str) else None
        if m:
            if m.group(1) == "gridWidth":
                raise Exa4Unsupported("%s on a non-uniform grid" % e[1])
            off = e[3] if k == "vfo" else ()
            return grid.axis_values(m.group(1), lvl, a, int(off[a]) if a < len(off) else 0)
        return float(eval_scalar(e))
    if k == "bin" and e[1] in ("+", "-", "*", "/"):
        x, y = _eval_axis(e[2], a, lvl, grid, eval_scalar, name), _eval_axis(e[3], a, lvl, grid, eval_scalar, name)
        return x + y if e[1] == "+" else (x - y if e[1] == "-" else (x * y if e[1] == "*" else x / y))
    if k == "bin" and e[1] == "**" and e[3][0] == "num" and float(e[3][1]) == 2.0:
        x = _eval_axis(e[2], a, lvl, grid, eval_scalar, name)
        return x * x
    if not _axes_of(e, 3, name):
        return float(eval_scalar(e))
    raise Exa4Unsupported("stencil %s: %s in a factor over the grid's virtual fields" % (name, k))
