"""Staggered-grid Stokes as a hand-written driver on the library layer, the way SolverFromL4 is one for Poisson: the method of
Examples/Stokes/2D_FD_Stokes_fromL4.exa4 / 3D_FD_Stokes_fromL4.exa4 (finite differences on a uniform MAC grid: velocities on the faces,
pressure in the cells) with the box smoother under the colouring of 2D_FV_Stokes_fromL4.exa4:588-591, `i0 % 3, i1 % 3 [, i2 % 3]`, the
one under which the sweep does not depend on the loop order (include/examg.h: examg_mac_relax).

    -Laplace u + grad p = f,   div u = g   on [0, 1]^d,   u Dirichlet, p Neumann (order 1), p normalised to the mean of the exact one (0)

V(4, 4) cycles of box sweeps with relax 0.8, `apply bc` after every colour as the program has it; the residual of all three fields is
ONE examg_mac_op; the residuals are restricted (velocities over interior faces only), the coarse problem starts from zero, the three
corrections are prolongated; the coarsest level runs cfg.coarse_sweeps sweeps (Testing/Application/ExaStokes_2D.exa4:228-233) instead
of the programs' BiCGStab.  Levels: domain_fragmentLength = 3, i.e. 3 * 2^level cells per axis.  Single block."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List

from .field import Colouring, MacSystem, Stencil
from .layout import FieldLayout
from .lib import BC_DIRICHLET, BC_NEUMANN, SYS_RESIDUAL, ExprC, GeomC
from .solver import reduced_prec

PI = math.pi


class _X:
    """An expression tree over the position as a postfix program (include/examg.h: examg_expr_t): operands left to right, then the
    operation -- the order the tree prescribes.  Products of Python numbers fold before they meet the tree, as the generator folds constants."""

    def __init__(self, prog):
        self.prog = prog

    @staticmethod
    def of(v):
        return v if isinstance(v, _X) else _X([("const", float(v))])

    def _bin(self, o, op, swap=False):
        a, b = (_X.of(o), self) if swap else (self, _X.of(o))
        return _X(a.prog + b.prog + [(op, None)])

    def __add__(self, o):
        return self._bin(o, "+")

    def __sub__(self, o):
        return self._bin(o, "-")

    def __mul__(self, o):
        return self._bin(o, "*")

    def __rmul__(self, o):
        return self._bin(o, "*", True)

    def expr(self) -> ExprC:
        return ExprC.from_program(self.prog)


def _sin(a):
    return _X(a.prog + [("sin", None)])


def _cos(a):
    return _X(a.prog + [("cos", None)])


_POS = (_X([("x", None)]), _X([("y", None)]), _X([("z", None)]))


def manufactured(nd: int, problem: str = "trigonometric"):
    """(exact u_d, exact p, rhs of u_d, rhs of p).  trigonometric: 2D_FD_Stokes_fromL4.exa4:222-227, 645-655 and 3D_FD_Stokes_fromL4.exa4:345-352,
    870-879.  polynomial: a divergence-free quadratic field and a pressure of mean zero, which the second-order scheme represents exactly
    (the errors fall to rounding) and whose programs hold additions, subtractions and products only: every kernel layer rounds them alike."""
    x, y, z = _POS
    if problem == "polynomial":
        zero = _X.of(0.0)
        if nd == 2:
            u, p = [x * x - y, x - (2.0 * x) * y], x * y - 0.25
            f, g = [y - 2.0, x + 0.0], zero
        else:
            u, p = [x * x - z, x - (2.0 * x) * y, y + 0.0 * z], (x * y + z) - 0.75
            f, g = [y - 2.0, x + 0.0, zero + 1.0], zero
        return [e.expr() for e in u], p.expr(), [e.expr() for e in f], g.expr()
    if problem != "trigonometric":
        raise ValueError("problem %r" % (problem,))
    if nd == 2:
        u = [_sin(2.0 * PI * x) - _cos(PI * y), _cos(PI * x) - _sin(2.0 * PI * y)]
        p = _sin(4.0 * PI * x) + _sin(4.0 * PI * y)
        f = [4.0 * PI ** 2 * _sin(2.0 * PI * x) - PI ** 2 * _cos(PI * y) + 4.0 * PI * _cos(4.0 * PI * x),
             PI ** 2 * _cos(PI * x) - 4.0 * PI ** 2 * _sin(2.0 * PI * y) + 4.0 * PI * _cos(4.0 * PI * y)]
        g = 2.0 * PI * _cos(2.0 * PI * x) - 2.0 * PI * _cos(2.0 * PI * y)
    else:
        u = [_sin(2.0 * PI * x) - _cos(PI * z), _cos(PI * x) - _sin(2.0 * PI * y), _sin(2.0 * PI * z) - _cos(PI * y)]
        p = _sin(4.0 * PI * x) + _sin(4.0 * PI * y) + _sin(4.0 * PI * z)
        f = [4.0 * PI ** 2 * _sin(2.0 * PI * x) - PI ** 2 * _cos(PI * z) + 4.0 * PI * _cos(4.0 * PI * x),
             PI ** 2 * _cos(PI * x) - 4.0 * PI ** 2 * _sin(2.0 * PI * y) + 4.0 * PI * _cos(4.0 * PI * y),
             4.0 * PI ** 2 * _sin(2.0 * PI * z) - PI ** 2 * _cos(PI * y) + 4.0 * PI * _cos(4.0 * PI * z)]
        g = 2.0 * PI * _cos(2.0 * PI * x) - 2.0 * PI * _cos(2.0 * PI * y) + 2.0 * PI * _cos(2.0 * PI * z)
    return [e.expr() for e in u], p.expr(), [e.expr() for e in f], g.expr()


ZERO = ExprC.from_program([("const", 0.0)])


@dataclass
class ConfigStokes:
    nd: int = 2
    min_level: int = 1
    max_level: int = 5
    pre: int = 4
    post: int = 4
    relax: float = 0.8
    colour_mod: int = 3           # `i0 % 3, i1 % 3 [, i2 % 3]`
    coarse_sweeps: int = 9        # the smallest count beyond which the cycle count no longer falls
    max_it: int = 30              # the reference's cap (2D_FD_Stokes_fromL4.exa4:305)
    tol: float = 1.0e-10
    frag_len: int = 3             # domain_fragmentLength
    problem: str = "trigonometric"   # the programs' manufactured solution, or "polynomial" (manufactured)


class _Level:
    pass


class StokesSolver:
    def __init__(self, ops, cfg: ConfigStokes):
        if cfg.nd not in (2, 3):
            raise ValueError("Stokes in 2-D or 3-D")
        if not 0 <= cfg.min_level <= cfg.max_level:
            raise ValueError("levels %d .. %d" % (cfg.min_level, cfg.max_level))
        self.ops, self.cfg = ops, cfg
        nd = cfg.nd
        self.sol_u, self.sol_p, self.rhs_u, self.rhs_p = manufactured(nd, cfg.problem)
        self.colouring = Colouring(tuple(((d,), 0, cfg.colour_mod) for d in range(nd)))
        self.walls = (1 << (2 * nd)) - 1
        self.levels = {l: self._make_level(l) for l in range(cfg.min_level, cfg.max_level + 1)}
        self.log: List[str] = []
        self.res_history: List[float] = []
        self.err_history: List[tuple] = []
        self.iterations = 0
        self._graph = None
        self.setup()

    # -- fields and operator of a level -----------------------------------------------------------------------------------------------
    def _make_level(self, l: int) -> _Level:
        cfg, ops, nd = self.cfg, self.ops, self.cfg.nd
        n = cfg.frag_len * 2 ** l
        cells = (n,) * nd
        L = _Level()
        L.n, L.cells = n, cells
        L.geom = GeomC()
        for d in range(3):
            L.geom.pos_begin[d], L.geom.h[d] = 0.0, (1.0 / n if d < nd else 0.0)
        h = 1.0 / n
        lu = [FieldLayout.face(nd, cells, d, 1) for d in range(nd)]
        lp = FieldLayout.cell(nd, cells, 1)
        lf = [FieldLayout.face(nd, cells, d, 0) for d in range(nd)]
        lfp = FieldLayout.cell(nd, cells, 0)
        new = lambda lay: ops.new_array(lay.size)
        # Stencil A11 / A22 / A33: the centre, then -x, +x, -y, +y [, -z, +z]
        offs, co, centre = [(0, 0, 0)], [None], None
        for t in range(nd):
            centre = 2.0 / (h ** 2) if centre is None else centre + 2.0 / (h ** 2)
            for s in (-1, 1):
                o = [0, 0, 0]
                o[t] = s
                offs.append(tuple(o))
                co.append(-1.0 / (h ** 2))
        co[0] = centre
        A = [Stencil(list(offs), list(co)) for _ in range(nd)]
        L.sys = MacSystem(nd=nd, lu=lu, u=[new(x) for x in lu], lp=lp, p=new(lp), A=A, bc=[1.0 / h] * nd, bm=[-1.0 / h] * nd, cc=[-1.0 / h] * nd,
                          cp=[1.0 / h] * nd, lf=lf, f=[new(x) for x in lf], lfp=lfp, fp=new(lfp), ld=lu, dst=[new(x) for x in lu], ldp=lp,
                          dstp=new(lp))
        L.cell_box = ([0, 0, 0], [n if d < nd else 1 for d in range(3)])
        L.face_box = [lu[d].loop_box() for d in range(nd)]
        # the residual rows: the velocities over interior faces only (a boundary face is no unknown; its residual stays 0)
        rb, re = [], []
        for d in range(nd):
            b, e = [list(v) for v in L.face_box[d]]
            b[d], e[d] = 1, n
            rb.append(b)
            re.append(e)
        L.row_begin, L.row_end = rb + [L.cell_box[0]], re + [L.cell_box[1]]
        L.colours = list(self.colouring.colours())
        L.bc_u = self.sol_u if l == cfg.max_level else [ZERO] * nd
        return L

    # -- statements ---------------------------------------------------------------------------------------------------------------------
    def apply_bc(self, l: int):
        """apply bc to u, v [, w] (Dirichlet: the exact solution on the finest level, 0.0 below) and to p (Neumann)."""
        L, ops, y = self.levels[l], self.ops, self.levels[l].sys
        for d in range(self.cfg.nd):
            ops.apply_bc_face(d, y.lu[d].c_struct(), y.u[d], L.geom, BC_DIRICHLET, L.bc_u[d], self.walls)
        ops.apply_bc_cell(y.lp.c_struct(), y.p, L.geom, BC_NEUMANN, None, self.walls)

    def sweep(self, l: int):
        """color with { i0 % 3, i1 % 3 [, i2 % 3], loop over p { solve locally relax 0.8 { .. } }  apply bc to u, v, p }"""
        L = self.levels[l]
        for col in L.colours:
            self.ops.mac_relax(L.sys, self.cfg.relax, col, L.cell_box[0], L.cell_box[1])
            self.apply_bc(l)

    def UpdateRes(self, l: int):
        L = self.levels[l]
        self.ops.mac_op(SYS_RESIDUAL, L.sys, (1 << (self.cfg.nd + 1)) - 1, L.row_begin, L.row_end)

    def ResNorm(self, l: int) -> float:
        L, ops, y = self.levels[l], self.ops, self.levels[l].sys
        norm = 0.0
        for d in range(self.cfg.nd):
            b, e = L.face_box[d]
            norm += ops.scalar_value(ops.dot(y.ld[d].c_struct(), y.dst[d], y.ld[d].c_struct(), y.dst[d], b, e))
        norm += ops.scalar_value(ops.dot(y.ldp.c_struct(), y.dstp, y.ldp.c_struct(), y.dstp, L.cell_box[0], L.cell_box[1]))
        return math.sqrt(norm)

    def mgCycle(self, l: int):
        cfg, ops, nd = self.cfg, self.ops, self.cfg.nd
        if l == cfg.min_level:
            for _ in range(cfg.coarse_sweeps):
                self.sweep(l)
            return
        F, Cs = self.levels[l], self.levels[l - 1]
        y, c = F.sys, Cs.sys
        for _ in range(cfg.pre):
            self.sweep(l)
        self.UpdateRes(l)
        for d in range(nd):
            ops.restrict_face(d, y.ld[d].c_struct(), y.dst[d], c.lf[d].c_struct(), c.f[d], 1.0, Cs.row_begin[d], Cs.row_end[d])
        ops.restrict_cell(y.ldp.c_struct(), y.dstp, c.lfp.c_struct(), c.fp, 1.0, Cs.cell_box[0], Cs.cell_box[1])
        for d in range(nd):
            ops.set(c.lu[d].c_struct(), c.u[d], 0.0, Cs.face_box[d][0], Cs.face_box[d][1])
        ops.set(c.lp.c_struct(), c.p, 0.0, Cs.cell_box[0], Cs.cell_box[1])
        self.apply_bc(l - 1)
        self.mgCycle(l - 1)
        for d in range(nd):
            ops.prolong_add_face(d, c.lu[d].c_struct(), c.u[d], y.lu[d].c_struct(), y.u[d], F.face_box[d][0], F.face_box[d][1])
        ops.prolong_add_cell(c.lp.c_struct(), c.p, y.lp.c_struct(), y.p, F.cell_box[0], F.cell_box[1])
        self.apply_bc(l)
        for _ in range(cfg.post):
            self.sweep(l)

    def NormalizePressure(self):
        L, ops, y = self.levels[self.cfg.max_level], self.ops, self.levels[self.cfg.max_level].sys
        mean = ops.scalar_value(ops.sum(y.lp.c_struct(), y.p, L.cell_box[0], L.cell_box[1])) / float(L.n ** self.cfg.nd)
        ops.add_scalar(y.lp.c_struct(), y.p, -mean, L.cell_box[0], L.cell_box[1])
        ops.apply_bc_cell(y.lp.c_struct(), y.p, L.geom, BC_NEUMANN, None, self.walls)

    def PrintError(self):
        """The maximum errors of u, v [, w] and p after NormalizePressure."""
        self.NormalizePressure()
        L, ops, y = self.levels[self.cfg.max_level], self.ops, self.levels[self.cfg.max_level].sys
        errs = []
        for d in range(self.cfg.nd):
            b, e = L.face_box[d]
            errs.append(ops.scalar_value(ops.max_err_expr_face(d, y.lu[d].c_struct(), y.u[d], L.geom, self.sol_u[d], b, e)))
        errs.append(ops.scalar_value(ops.max_err_expr_cell(y.lp.c_struct(), y.p, L.geom, self.sol_p, L.cell_box[0], L.cell_box[1])))
        return tuple(errs)

    def arrays(self):
        """Every array of every level, coarsest level first: unknowns, right-hand sides, residuals."""
        out = []
        for l in sorted(self.levels):
            y = self.levels[l].sys
            out += y.u + [y.p] + y.f + [y.fp] + y.dst + [y.dstp]
        return out

    def setup(self):
        """InitFields@finest, every unknown 0, `apply bc` of the three fields on every level."""
        ops, nd = self.ops, self.cfg.nd
        for l, L in self.levels.items():
            y = L.sys
            for arrs in (y.u, [y.p], y.f, [y.fp], y.dst, [y.dstp]):
                for t in arrs:
                    t.zero_()
            if l == self.cfg.max_level:
                for d in range(nd):
                    ops.fill_expr_face(d, y.lf[d].c_struct(), y.f[d], L.geom, self.rhs_u[d], L.face_box[d][0], L.face_box[d][1])
                ops.fill_expr_cell(y.lfp.c_struct(), y.fp, L.geom, self.rhs_p, L.cell_box[0], L.cell_box[1])
            self.apply_bc(l)
        self.log, self.res_history, self.err_history, self.iterations = [], [], [], 0

    def Solve(self, use_graph: bool = False) -> int:
        """Function Solve@finest: the lines of printWithReducedPrec -- the starting residual, then per cycle the residual and the maximum
        errors of u, v [, w], p -- and the number of cycles."""
        cfg, hi = self.cfg, self.cfg.max_level
        self.UpdateRes(hi)
        initRes = curRes = self.ResNorm(hi)
        self.res_history.append(initRes)
        self.log.append(reduced_prec(initRes))
        curIt = 0
        while not (curIt >= cfg.max_it or curRes <= cfg.tol * initRes):
            curIt += 1
            if use_graph:
                self.replay_cycle()
            else:
                self.mgCycle(hi)
            self.UpdateRes(hi)
            curRes = self.ResNorm(hi)
            self.res_history.append(curRes)
            self.log.append(reduced_prec(curRes))
            errs = self.PrintError()
            self.err_history.append(errs)
            self.log.extend(reduced_prec(v) for v in errs)
        self.iterations = curIt
        self.log.append(str(curIt))
        return curIt

    # -- one cycle as a hipGraph, on one stream -----------------------------------------------------------------------------------------
    def capture_cycle(self):
        """Records one mgCycle@finest (no reduction, no host round trip inside it).  The recording runs no kernel: the fields are as before."""
        rec = self.ops.graph_begin()
        try:
            self.mgCycle(self.cfg.max_level)
        finally:
            self.ops.graph_end(rec)
        self._graph = rec
        return rec

    def replay_cycle(self):
        if self._graph is None:
            self.capture_cycle()
        self.ops.graph_replay(self._graph)
