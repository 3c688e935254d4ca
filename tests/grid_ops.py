"""TEST-ONLY restatement of the entry points of axis-aligned non-uniform grids (include/examg.h: examg_fill_expr_grid,
examg_apply_dirichlet_expr_grid, examg_max_err_expr_grid, examg_axis_op, examg_axis_route) in numpy, on top of the oracle-backed kernel
layer (tests/oracle_ops.py through tests/nonlinear_ops.py, so that one class runs every program of the suite).  Every operation in the
order the header fixes; numpy evaluates each operation in IEEE double, one at a time: no contraction.  The structs are read back as the
library reads them (through their pointers), so the packing of grid.AxisStencil.c_struct and AxisGrid.device is part of what runs."""
import ctypes as C

import numpy as np

from cell_ops import _empty, _sl, _view
from nonlinear_ops import NonlinearOracleOps, _colour_sel

APPLY, RESIDUAL, SMOOTH = 0, 1, 2
AXIS_AUTO, AXIS_GENERIC, AXIS_STAR = 0, 1, 2
AXIS_MAX_TERMS, AXIS_STAR_TERMS = 32, 12


def _table(ptr, n):
    """n doubles at the address ptr (host memory on this kernel layer)."""
    if not ptr or n <= 0:
        return np.zeros(0)
    return np.ctypeslib.as_array((C.c_double * int(n)).from_address(int(ptr)))


def _tot(l, d):
    return l.pad_l[d] + l.ghost_l[d] + l.dup_l[d] + l.inner[d] + l.dup_r[d] + l.ghost_r[d] + l.pad_r[d]


def _inside(l, begin, end, halo):
    for d in range(3):
        h = halo if d < l.nd else 0
        ref = l.pad_l[d] + l.ghost_l[d]
        if begin[d] - h + ref < 0 or end[d] + h + ref > _tot(l, d):
            return False
    return True


class AxisRefused(ValueError):
    """What examg_axis_op refuses before it launches anything."""


def axis_check(mode, lu, lf, ld, sc, colour, begin, end, in_place):
    """The header's refusals of examg_axis_op, and its route: 0 for an empty box, AXIS_GENERIC or AXIS_STAR."""
    nd = lu.nd
    if nd not in (2, 3) or ld.nd != nd or (mode != APPLY and lf.nd != nd):
        raise AxisRefused("2-D or 3-D layouts of one dimensionality")
    for l in (lu, ld) + ((lf,) if mode != APPLY else ()):
        if l.transform != 0:
            raise AxisRefused("a layout under a layout transformation")
    if not 1 <= sc.nent <= 27 or not sc.nent <= sc.nterm <= AXIS_MAX_TERMS:
        raise AxisRefused("entry or term count out of range")
    offs = [tuple(sc.off[k]) for k in range(sc.nent)]
    if not 0 <= sc.diag < sc.nent or offs[sc.diag] != (0, 0, 0):
        raise AxisRefused("no centre entry")
    if any(abs(o) > 1 for off in offs for o in off) or any(off[d] != 0 for off in offs for d in range(nd, 3)):
        raise AxisRefused("offsets outside {-1, 0, 1} or outside the layout's dimensions")
    used, prev = [False] * 3, 0
    for t in range(sc.nterm):
        e = sc.term[t].entry
        if not (prev <= e <= prev + 1) or (t == 0 and e != 0) or e >= sc.nent:
            raise AxisRefused("terms are not sorted by entry, or an entry has none")
        prev = e
        for d in range(3):
            tb = sc.term[t].tab[d]
            if tb < -1 or tb >= sc.ntab[d] or (tb >= 0 and d >= nd):
                raise AxisRefused("table index out of range")
            used[d] = used[d] or tb >= 0
    if prev != sc.nent - 1:
        raise AxisRefused("the last entry has no term")
    if colour not in (-1, 0, 1) or (in_place and colour < 0):
        raise AxisRefused("bad colour, or dst is u without a colour")
    if _empty(begin, end):
        return 0
    if not _inside(lu, begin, end, 1):
        raise AxisRefused("the one-point shell of the box leaves the u allocation")
    if not _inside(ld, begin, end, 0) or (mode != APPLY and not _inside(lf, begin, end, 0)):
        raise AxisRefused("box leaves the dst or rhs allocation")
    for d in range(nd):
        if used[d] and (begin[d] < sc.tab_begin[d] or end[d] > sc.tab_begin[d] + sc.tab_len[d]):
            raise AxisRefused("the tables of axis %d do not cover the box" % d)
    axis_nb = sorted(off for off in offs if off != (0, 0, 0))
    star = nd == 3 and sc.nent == 7 and sc.nterm <= AXIS_STAR_TERMS and \
        axis_nb == sorted([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)])
    if sc.route == AXIS_STAR and not star:
        raise AxisRefused("the star route takes 3-D stencils of the centre and the six axis neighbours")
    return AXIS_STAR if star and sc.route != AXIS_GENERIC else AXIS_GENERIC


def eval_grid_program(prog, p, w):
    """The program on the positions p = (x, y, z) and widths w = (wx, wy, wz) of the box's points, one IEEE operation per instruction."""
    ops, out = {"wx": w[0], "wy": w[1], "wz": w[2]}, []
    un = {"neg": np.negative, "sin": np.sin, "cos": np.cos, "exp": np.exp, "sinh": np.sinh, "cosh": np.cosh, "sqrt": np.sqrt, "tan": np.tan,
          "log": np.log, "fabs": np.abs, "tanh": np.tanh}
    bi = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide, "pow": np.power, "max": np.maximum, "min": np.minimum}
    zero =0.0 * (p[0] + p[1] + p[2])
    for name, c in prog:
        if name == "const":
            out.append(zero + float(c))
        elif name in ("x", "y", "z"):
            out.append(zero + p["xyz".index(name)])
        elif name in ops:
            out.append(zero + ops[name])
        elif name in un:
            out[-1] = un[name](out[-1])
        else:
            b = out.pop()
            out[-1] = bi[name](out[-1], b)
    return out[0]


class GridOracleOps(NonlinearOracleOps):
    name = "grid-oracle"

    # -- point expressions over the node tables (examg_fill_expr_grid, examg_apply_dirichlet_expr_grid, examg_max_err_expr_grid) ----
    @staticmethod
    def _grid_points(l, grid, begin, end):
        """Positions and widths of the box's points as broadcastable (z, y, x) arrays; refuses what the tables do not hold."""
        p, w = [], []
        for d in range(3):
            n = end[d] - begin[d]
            shape = [1, 1, 1]
            shape[2 - d] = n
            if d >= l.nd or not grid.nodes[d]:
                if d < l.nd:
                    raise ValueError("no node table of axis %d" % d)
                p.append(np.zeros(shape))
                w.append(np.zeros(shape))
                continue
            if begin[d] + grid.ghost < 0 or end[d] + grid.ghost + 1 > grid.n[d]:
                raise ValueError("the node table of axis %d does not cover the box" % d)
            x = _table(grid.nodes[d], grid.n[d])
            lo = begin[d] + grid.ghost
            p.append(x[lo:lo + n].reshape(shape).copy())
            w.append((x[lo + 1:lo + n + 1] - x[lo:lo + n]).reshape(shape))
        return p, w

    def fill_expr_grid(self, l, x, grid, expr, begin, end):
        if _empty(begin, end):
            return
        if l.transform != 0:
            raise ValueError("a layout under a layout transformation")
        p, w = self._grid_points(l, grid, begin, end)
        a, ref = _view(l, x)
        with np.errstate(all="ignore"):
            a[_sl(ref, begin, end)] = eval_grid_program(expr.program, p, w)

    def apply_dirichlet_expr_grid(self, l, x, grid, expr, face_mask):
        nd = l.nd
        for d in range(nd):
            for side in (0, 1):
                if not face_mask & (1 << (2 * d + side)):
                    continue
                b, e = [0, 0, 0], [1, 1, 1]
                for t in range(nd):
                    if t == d:
                        b[t], e[t] = (0, l.dup_l[t]) if side == 0 else (l.dup_l[t] + l.inner[t], l.dup_l[t] + l.inner[t] + l.dup_r[t])
                    else:
                        b[t], e[t] = -l.ghost_l[t], l.dup_l[t] + l.inner[t] + l.dup_r[t] + l.ghost_r[t]
                self.fill_expr_grid(l, x, grid, expr, b, e)

    def max_err_expr_grid(self, l, x, grid, expr, begin, end, out=None):
        out = self.new_scalar() if out is None else out
        out[0] = 0.0
        if not _empty(begin, end):
            p, w = self._grid_points(l, grid, begin, end)
            a, ref = _view(l, x)
            with np.errstate(all="ignore"):
                out[0] = float(np.max(np.abs(a[_sl(ref, begin, end)] - eval_grid_program(expr.program, p, w))))
        return out

    # -- table-coefficient stencils (examg_axis_op) ---------------------------------------------------------------------------------
    @staticmethod
    def axis_coefficients(sc, begin, end):
        """c_k on the box for every entry k: the terms X[i0] * ((s * Z[i2]) * Y[i1]) of the entry folded left to right."""
        n = [end[d] - begin[d] for d in range(3)]
        tabs = [_table(sc.tables[d], sc.ntab[d] * sc.tab_len[d]).reshape(sc.ntab[d], -1) if sc.ntab[d] else None for d in range(3)]

        def tab(t, d):
            k = sc.term[t].tab[d]
            if k < 0:
                return np.ones(n[d])
            lo = begin[d] - sc.tab_begin[d]
            return tabs[d][k][lo:lo + n[d]]

        coef = [None] * sc.nent
        for t in range(sc.nterm):
            X, Y, Z = tab(t, 0), tab(t, 1), tab(t, 2)
            c = X[None, None, :] * ((float(sc.term[t].s) * Z)[:, None, None] * Y[None, :, None])
            e = sc.term[t].entry
            coef[e] = c if coef[e] is None else coef[e] + c
        return coef

    def axis_route(self, mode, lu, lf, ld, st, colour, begin, end, route=None):
        sc = st.c_struct(self)
        sc.route = AXIS_AUTO if route is None else int(route)
        try:
            return axis_check(mode, lu, lf, ld, sc, colour, begin, end, False)
        except AxisRefused:
            return -1

    def axis_op(self, mode, lu, u, lf, rhs, ld, dst, st, w, colour, begin, end, route=None):
        sc = st.c_struct(self)
        sc.route = AXIS_AUTO if route is None else int(route)
        if axis_check(mode, lu, lf, ld, sc, colour, begin, end, u.data_ptr() == dst.data_ptr()) == 0:
            return
        coef = self.axis_coefficients(sc, begin, end)
        ua, uref = _view(lu, u)
        acc = None
        for k in range(sc.nent):
            off = tuple(sc.off[k])
            nb = ua[_sl(uref, [begin[d] + off[d] for d in range(3)], [end[d] + off[d] for d in range(3)])]
            t = coef[k] * nb
            acc = t if acc is None else acc + t
        da, dref = _view(ld, dst)
        s = _sl(dref, begin, end)
        if mode == APPLY:
            out = acc
        else:
            fa, fref = _view(lf, rhs)
            f = fa[_sl(fref, begin, end)]
            if mode == RESIDUAL:
                out = f - acc
            else:
                dg = coef[sc.diag]
                ww = float(w) / dg if sc.wform == 1 else (1.0 / dg) * float(w)
                out = ua[_sl(uref, begin, end)] + ww * (f - acc)
        da[s] = out if colour < 0 else np.where(_colour_sel(begin, end, colour), out, da[s])
