"""ExaSlang-4 subset reader and interpreter: run the reference's own multigrid programs on libexamg.

The reference compiles an ExaSlang-4 program (`*.exa4`) plus a `.knowledge` file into C++/CUDA whose hot loops are
what libexamg implements.  This module reads the same two inputs and executes the program directly:
declarations become device fields and host stencils, leveled functions are interpreted, and every `loop over` body is
recognised as one of the emitted-loop kinds and issued as ONE library call on the current HIP stream -- there is no
per-point interpretation, no generated code and no CPU arithmetic on field data.

Grammar covered (Compiler/src/exastencils/parsers/l4/L4_Parser.scala): `Domain` (:286-296), `Layout` with
`ghostLayers` / `duplicateLayers [with communication]` (:378-396), `Field name< domain, layout, bc >[slots]@levels`
(:398-408), `Stencil` with offset entries, `from [...] with` mapping entries and `from default restriction|prolongation`
(:430-466), `StencilField` (:468-472), `Globals` (:227-233), leveled `Function`s (:235-260) with `Var`/`Val`,
assignments, `loop over f [only dup [..] on boundary] [where c] [with reduction (op : v)]` (:303-340),
`communicate [ghost|dup of]`, `apply bc to`, `advance`, `repeat n times [count v]`, `repeat until`, `if/else`,
`color with`, `return`, level scopes `@(...) { }` (:653-667), declaration level lists `@all`, `@(a to b)`, `@(a, b)`,
`@(a and b)`, `@(all but x)`, `coarsest + 1`, and access levels `@current|coarser|finer|finest|coarsest|<n>`.

Loop bodies recognised (anything else raises Exa4Unsupported -- nothing is silently approximated); the assignments among them by the
one recogniser of exa4_statements.py (`_recognise_assign` -> LoopStmt) and issued by its launcher (`_launch`, `_launch_coloured`), the
whole-loop forms (reductions, stencil-field initialisation, builtins, `solve locally`) by executors of their own:
  F = c | F = G | F = analytic(x,y,z) | F += a*G | F -= a*G | F = G + b*F            examg_set/fill_fn/axpby
  R = RHS - A*U | D = A*U                                                            examg_residual / stencil_op(APPLY)
  U<next> = U<active> + w(diag A) * (RHS - A*U<active>)                              examg_jacobi
  U += w(diag A) * (RHS - A*U)   inside `color with {(i0+i1+i2) % 2, ...}` or `where (c == (i0+i1+i2) % 2)`
                                                                                      examg_rbgs_colour
  RHS@coarser = [s *] Restriction * Residual | U += Prolongation@coarser * U@coarser  examg_restrict / examg_prolong_add
  s += F*G (reduction +) | s = max(s, fabs(F - analytic)) (reduction max)             examg_dot / examg_max_err_fn
  A:[o] = expr (every entry of a stencil field)                                      examg_init_varcoeff7 / examg_fill_expr
Analytic point functions (boundary values, right-hand sides, exact solutions) are matched numerically against the
built-in function ids of include/examg.h; any other expression over the node position -- user functions included -- is
compiled to a postfix program (examg_expr_t) that the device evaluates per point in the order of the expression tree
(examg_fill_expr / examg_apply_dirichlet_expr / examg_max_err_expr).  Stencil-field entries `A:[o] = expr` take
examg_init_varcoeff7 when they are -div(a grad) with a built-in `a`, else one expression program per coefficient plane.

Fewer passes than statements, where the statements allow it (`fuse=True`, bit-identical): a `color with` red-black
sweep is one out-of-place pass (examg_rbgs_sweep_fused), `repeat n times { Smoother ( ) }` with a slotted Jacobi body runs
as n/2 two-step passes (examg_jacobi2_boxes) -- both only while the boundary planes involved are known to hold the
field's Dirichlet values.  A coarsest-level function that is statement for statement the generated CG solver -- in the form of the
layer-4 benchmark program or in the one the layer-3 solver generator writes (_match_coarse_cg) -- becomes one persistent kernel
(examg_cg_coarse / examg_cg_coarse_variant; `fuse_coarse_solver`, agrees to reduction-order rounding); a cycle is then free of host
synchronisation and `capture()` records it into a hipGraph.

Two deliberate readings of printed-L4 files (Testing/Smoothers/Jac.exa4:43 declares the finest `Solution` without level
and slot count): a declaration never overrides an earlier one on the same level (the reference's collection lookup
returns the first match, knowledge/l4/L4_KnowledgeCollection.scala:78-79), and a field name has one slot count, the
maximum over its declarations.
"""
from __future__ import annotations

import math
import os
import random
import re
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

from . import knowledge as _knowledge
from .comm import Communicator
from .domain import RectDomain
from .field import Field, Stencil
from .grid import CELL_VOLUME, AxisGrid, separate
from .layout import FieldLayout
from .exa4_parser import (Exa4SyntaxError, Exa4Unsupported, FunctionDecl, Parser, _COORD, _GRIDW, _MATH, _arith,  # noqa: F401
                          _colour_cond, _colour_expr, _conjuncts, _const_value, _contains, _find_calls, _has_coord, _lower_cond, _parity_expr, _walk)

from .exa4_systems import Systems  # noqa: E402
from .exa4_blocksys import BlockSystems  # noqa: E402
from .exa4_nonlinear import Nonlinear  # noqa: E402
from .exa4_statements import Statements  # noqa: E402
from .exa4_common import (APPLY, RESIDUAL, SMOOTH, _FN_2D_ONLY, _FN_ANY_DIM, _FN_WITH_PARAM, _N_FN, _Frame, _Return, fn_eval)  # noqa: E402,F401
from .exa4_builtins import Builtins  # noqa: E402
from .exa4_fusion import LazyFusions  # noqa: E402
from .exa4_peepholes import Peepholes  # noqa: E402
from .exa4_conservation import Conservation, _EXPR, expand  # noqa: E402
from .exa4_complex import ComplexFields  # noqa: E402
from .exa4_vector import VectorFields  # noqa: E402


class Exa4Program(LazyFusions, Peepholes, Builtins, Statements, Systems, BlockSystems, Nonlinear, Conservation, ComplexFields, VectorFields):
    """One ExaSlang-4 program bound to a kernel layer (`ops`: HipOps on the GPU), a block decomposition and a
    communicator.  `run()` executes `Function Application`; printed lines are collected in `self.out`."""

    def __init__(self, text: str, knowledge: Optional[Dict] = None, ops=None, domain: Optional[RectDomain] = None, comm=None,
                 echo: bool = False, fuse: bool = True, fuse_coarse_solver: Optional[bool] = None, auto_graph: Optional[bool] = None):
        """fuse: run red-black sweeps and pairs of slotted Jacobi steps as single passes over HBM where the program's
        statements allow it (bit-identical results; `fuse=False` issues exactly one launch per loop statement).
        auto_graph: a leveled function without parameters whose statements never return to the host (no reductions, prints or
        builtins anywhere below it, no assignment to a `Globals` variable: typically the cycle function) is recorded into a hipGraph
        at its second call.  A later call is a replay only while interpreting it would issue the recorded launches with the recorded
        scalars: the recording keeps a guard (_graph_guard: the array roles, the values of every global the function can read, the
        boundary / second-array / stencil-field bookkeeping as it stood at entry, the call site) that is compared before every
        replay, and a replay leaves the bookkeeping as the recorded call left it; a call under another guard is interpreted, and the
        function recorded anew when two calls in a row meet the same other guard.
        Default: on with `fuse` on the HIP kernel layer, one block; `auto_graph=True` is honoured on every kernel layer that has the
        four graph operations (graph_begin / graph_end / graph_replay / graph_capturing)."""
        self.ast = Parser(text).parse()
        self.k = dict(knowledge or {})
        d = _knowledge.derive(self.k)
        self.nd = d["dimensionality"]
        self.min_level, self.max_level = d["min_level"], d["max_level"]
        if ops is None:
            from .ops import HipOps

            ops = HipOps()              # raises without libexamg.so / GPU: no fallback
        self.ops = ops
        lo, hi = (0.0,) * 3, (1.0,) * 3
        if self.ast.domain:
            lo = tuple(float(_const_value(e)) for e in self.ast.domain[1]) + (0.0,) * (3 - self.nd)
            hi = tuple(float(_const_value(e)) for e in self.ast.domain[2]) + (1.0,) * (3 - self.nd)
        self._merged_blocks = None
        self._fragments = d["frags_total"][0] * d["frags_total"][1] * d["frags_total"][2]      # of the knowledge file: what a per-fragment loop order depends on
        if domain is None:
            # one process: the reference's blocks x fragments become one fragment of the same global grid
            flen = tuple(d["frags_total"][i] * d["frag_len"][i] for i in range(3))
            domain = RectDomain(self.nd, (1, 1, 1), 0, flen, lo[:3], hi[:3], d["periodic"])
            if d["num_blocks"] != (1, 1, 1) and d["frags_per_block"] == (1, 1, 1):
                self._merged_blocks = (d["num_blocks"], d["frag_len"])      # what a per-process std::rand() needs to know (_exec_rand_fill)
        self.domain = domain
        # node tables of an axis-aligned non-uniform grid (grid_isUniform = false, grid_spacingModel = "linearFct"); None: uniform
        self.grid = AxisGrid.from_knowledge(self.k, self.nd, lo, hi, d["cells_per_dim_finest"], self.min_level, self.max_level,
                                            blocks=domain.world_size, periodic=domain.periodic)
        self.comm = comm or Communicator(domain, ops)
        self.echo = echo
        self.out: List[str] = []
        self.printed_values: List[float] = []     # every Real handed to print / printWithReducedPrec, unrounded
        self.json_results: Dict[str, Dict] = {}
        self.json_dir: Optional[str] = None       # where printJSON writes its file (None: keep it in json_results only)
        self.timers: Dict[str, float] = {}
        self._timer_start: Dict[str, float] = {}
        self.launches = 0
        self._precision = 6
        self.globals: Dict[str, object] = {}
        self.fields: Dict[Tuple[str, int], Field] = {}
        self.stencils: Dict[Tuple[str, int], Stencil] = {}
        self.transfer: Dict[str, str] = {}
        self.transfer_factor: Dict[str, float] = {}     # the common factor of a node restriction's weights: multiplies the statement's scale
        self._fn_cache: Dict[Tuple, Tuple] = {}
        self._rng = random.Random(20240229)
        self.fuse = fuse
        # a coarsest-level function that is exactly the generated conjugate-gradient solver runs as ONE persistent kernel
        # (examg_cg_coarse; single block).  Same algorithm and statement order; the in-kernel reductions sum in another
        # (fixed) order, so iterates agree with the statement-by-statement run to rounding, not bit for bit.
        self.fuse_coarse_solver = fuse if fuse_coarse_solver is None else fuse_coarse_solver
        self._cg_plans: Dict[Tuple[str, int], object] = {}
        # shortest row the one-pass forms are used on: the kernel layer has them for every row length (two-stage kernel from 64 points,
        # csrc/kernels_small.hip below), blocks with neighbours keep 64 (interior + shell split)
        self.fuse_min_row = 3
        self.fuse_min_row_blocks = 64
        on_gpu = hasattr(ops, "torch") and getattr(getattr(ops, "device", None), "type", "cpu") != "cpu"
        self.auto_graph = bool((fuse and on_gpu if auto_graph is None else auto_graph) and hasattr(ops, "graph_begin") and
                               domain.world_size == 1 and not any(domain.periodic))
        self._auto_graphs: Dict[Tuple[str, int], object] = {}     # (function, level) -> recorded graph | False (not capturable)
        self._auto_calls: Dict[Tuple[str, int], int] = {}
        self._host_free: Dict[Tuple[str, int], bool] = {}
        self._graph_reads: Dict[Tuple[str, int], Tuple[str, ...]] = {}     # (function, level) -> globals a recording of it depends on
        self._graph_depth = 0
        self.graph_replays = 0
        self._alt: Dict[Tuple[str, int, int], object] = {}
        self._alt_shell: Dict[Tuple[str, int, int], int] = {}
        self._bc_epoch: Dict[Tuple[str, int], int] = {}
        self._pair_tmp: Dict[Tuple[str, int], Field] = {}
        self._bc_valid = set()      # (field, level, slot) whose physical-boundary planes hold the field's Dirichlet values
        self._complex_names = set() # fields declared on a Complex<Real> layout (exa4_complex.py)
        self._complex_scratch: Dict[int, Field] = {}     # per level: the real field a `C = <real point expression>` loop fills first
        self._bc_depth = 0          # inside a boundary function that `apply bc` runs
        self._bc_taken = set()      # ghost loops of the function body being executed that the launch of an earlier one covered
        self._node_ops = False      # _compile_point_expr: vf_nodePosition_* as EXAMG_OP_NODE_* (the value of a ghost loop)
        self._cell_names = set()    # fields declared on a cell layout: never taken by a one-pass peephole or cross-statement fusion
        self._vector_names = set()  # fields declared on a vector-valued cell layout (exa4_vector.py)
        self._has_vector = False    # ... or a stencil whose entries are matrices: only then is a statement asked whether it names one
        self._lazy_init()           # pending loops of the cross-statement fusions (exastencils_amd/exa4_fusion.py)
        self._declare()

    # -- declarations -> objects --------------------------------------------------------------------------------------
    def levels_of(self, spec, cur: Optional[int] = None) -> List[int]:
        lo, hi = self.min_level, self.max_level
        if spec is None or spec[0] == "all":
            return list(range(lo, hi + 1))
        k = spec[0]
        if k == "single":
            base = spec[1]
            if isinstance(base, str):
                if base in ("current", "coarser", "finer") and cur is None:
                    raise Exa4SyntaxError("@%s outside a leveled function" % base)
                base = {"current": cur, "coarser": None if cur is None else cur - 1, "finer": None if cur is None else cur + 1,
                        "finest": hi, "coarsest": lo}[base]
            return [base + spec[2]]
        if k == "range":
            a, b = self.levels_of(spec[1], cur)[0], self.levels_of(spec[2], cur)[0]
            return list(range(min(a, b), max(a, b) + 1))
        if k == "list":
            out = []
            for s in spec[1]:
                out += self.levels_of(s, cur)
            return sorted(set(out))
        if k == "but":
            drop = set(self.levels_of(spec[2], cur))
            return [l for l in self.levels_of(spec[1], cur) if l not in drop]
        raise Exa4SyntaxError("level specification %r" % (spec,))

    def _declare(self):
        a, nd, dom = self.ast, self.nd, self.domain
        self.functions: Dict[str, List[FunctionDecl]] = {}
        for fn in a.functions:
            self.functions.setdefault(fn.name, []).append(fn)
        self._inline_global_exprs()       # `Expr` macros of the Globals blocks (exa4_conservation.py)
        for name, e in a.globals:
            if _contains(e, ("mat", "colvec")):
                raise Exa4Unsupported("global %s: matrix-typed Var / Val (vector-valued fields run, matrix values do not)" % name)
            self.globals[name] = self._eval(e, _Frame(None, {}))
        layouts = {l.name: l for l in a.layouts}
        nslots: Dict[str, int] = {}
        for fd in a.fields:
            nslots[fd.name] = max(nslots.get(fd.name, 1), fd.slots)
        self._sfield_of = {}
        sfield_fields = {s.field for s in a.sfields}
        for fd in a.fields:
            ld = layouts.get(fd.layout)
            if ld is None:
                raise Exa4SyntaxError("field %s uses the undeclared layout %s" % (fd.name, fd.layout))
            if ld.datatype == "Complex":
                self._declare_complex_field(fd, ld, nslots[fd.name], sfield_fields)
                continue
            vector = (ld.vec_len != 1 or ld.vec_cols != 1) and fd.name not in sfield_fields
            if vector and ld.localization != "Node":      # column vectors on cell fields run (exa4_vector.py); every other one is refused there
                self._declare_vector_field(fd, ld, nslots[fd.name])
                continue
            if ld.localization not in ("Node", "Cell"):
                raise Exa4Unsupported("layout %s: localization %s (node and cell fields only)" % (ld.name, ld.localization))
            if vector:
                raise Exa4Unsupported("vector-valued field %s outside a StencilField" % fd.name)
            if ld.localization == "Cell":
                if self.grid is not None:
                    raise Exa4Unsupported("field %s: cell-centred fields on a non-uniform grid" % fd.name)
                self._declare_cell_field(fd, ld, nslots[fd.name], sfield_fields)
                continue
            if self._bc_kind(fd.bc) is not None:
                raise Exa4Unsupported("field %s: Neumann boundary conditions on node fields" % fd.name)
            for lvl in self.levels_of(fd.levels):
                if (fd.name, lvl) in self.fields or not (self.min_level <= lvl <= self.max_level):
                    continue
                nc = dom.ncells(lvl)
                ghost = tuple(ld.ghost[i] if i < nd and i < len(ld.ghost) else 0 for i in range(3))
                dup = tuple((ld.dup[i] if i < len(ld.dup) else 1) if i < nd else 0 for i in range(3))
                if any(dup[i] != 1 for i in range(nd)):
                    raise Exa4Unsupported("layout %s: node fields need one duplicate layer" % ld.name)
                inner = tuple(nc[i] - 1 if i < nd else 1 for i in range(3))
                if ld.inner and tuple(ld.inner[:nd]) != inner[:nd]:
                    # an explicit size (fieldlike/l4/L4_FieldLikeLayoutDecl.scala:49-51: innerPoints replaces the default 2^level * fragLen
                    # - 1): the benchmark programs of Testing/PolyExpl put a 256^3 array on level 0.  Loops follow the layout; grid
                    # widths and node positions stay those of the level, as in the reference.  Only without inter-grid transfers
                    if self.min_level != self.max_level or dom.world_size != 1:
                        raise Exa4Unsupported("layout %s: innerPoints %s differ from the %s points level %d gives one fragment"
                                              % (ld.name, list(ld.inner[:nd]), list(inner[:nd]), lvl))
                    inner = tuple(int(ld.inner[i]) if i < nd else 1 for i in range(3))
                lay = FieldLayout(nd, inner, ghost, dup, (0, 0, 0), (0, 0, 0), ld.dup_comm, ld.ghost_comm)
                bc_fn, bc_par = None, ()
                if fd.bc is not None:
                    bc_fn, bc_par = self._analytic(fd.bc, lvl)
                if ld.vec_len != 1:
                    f = Field.__new__(Field)     # coefficient planes: allocated by the stencil field below
                    f.name, f.level, f.layout, f.num_slots, f.bc_fn, f.bc_params = fd.name, lvl, lay, 1, None, ()
                    f.lc, f.slots, f.current_slot, f.vec_len = lay.c_struct(), [self.ops.new_array(ld.vec_len * lay.size)], 0, ld.vec_len
                else:
                    f = Field(fd.name, lvl, lay, self.ops, nslots[fd.name], bc_fn, bc_par)
                self.fields[(fd.name, lvl)] = f
        for sd in a.stencils:
            if sd.transfer:
                self.transfer[sd.name] = sd.transfer
                self.transfer_factor[sd.name] = float(sd.transfer_factor)
        self._stencil_decls = {s.name: s for s in a.stencils if not s.transfer}
        self._has_vector = bool(self._vector_names) or any(self._is_matrix_stencil(n) for n in self._stencil_decls)
        # a name declared once per level (`Stencil A@3 {..}  Stencil A@4 {..}`: the layer-4 text generated from layer 3)
        self._stencil_decl_at = {}
        for sd in a.stencils:
            if not sd.transfer and sd.levels is not None:
                for lvl in self.levels_of(sd.levels):
                    self._stencil_decl_at.setdefault((sd.name, lvl), sd)
        for sf in a.sfields:
            sd = self._stencil_decls.get(sf.stencil)
            if sd is None:
                raise Exa4SyntaxError("stencil field %s: stencil %s is not declared" % (sf.name, sf.stencil))
            for lvl in self.levels_of(sf.levels):
                cf = self.fields.get((sf.field, lvl))
                if cf is None:
                    continue
                offs = [tuple(o) + (0,) * (3 - len(o)) for o, _ in sd.entries]
                if getattr(cf, "vec_len", 1) != len(offs):
                    raise Exa4SyntaxError("stencil field %s: %d entries but %d coefficients per point" % (sf.name, len(offs), getattr(cf, "vec_len", 1)))
                self.stencils[(sf.name, lvl)] = Stencil(offs, [], cf.slots[0], cf.layout)
        self._apply_layout_transformations()

    # -- cell-centred fields ------------------------------------------------------------------------------------------------
    @staticmethod
    def _bc_kind(bc):
        """The order of a `Neumann` / `Neumann(n)` boundary condition, None for Dirichlet values (or no condition)."""
        if bc is None:
            return None
        if bc[0] == "id" and bc[1] == "Neumann":
            return 1
        if bc[0] == "call" and bc[1] == "Neumann":
            return int(_const_value(bc[3][0])) if len(bc[3]) == 1 else -1
        return None

    def _declare_cell_field(self, fd, ld, nslots: int, sfield_fields):
        """`Layout X< Real, Cell >`: no duplicate layers, one value per cell (fragLen * 2^level per dimension), boundary
        conditions in the ghost layer (examg_apply_bc_cell)."""
        from .lib import BC_DIRICHLET, BC_NEUMANN

        nd, dom = self.nd, self.domain
        if ld.vec_len != 1 or fd.name in sfield_fields:
            raise Exa4Unsupported("layout %s: vector-valued cell fields" % ld.name)
        if any(dom.periodic[:nd]):
            raise Exa4Unsupported("field %s: cell fields on a periodic domain" % fd.name)
        if any((ld.dup[i] if i < len(ld.dup) else 0) != 0 for i in range(nd)):
            raise Exa4Unsupported("layout %s: a cell layout has no duplicate layers" % ld.name)
        if ld.inner:
            raise Exa4Unsupported("layout %s: innerPoints on a cell layout" % ld.name)
        for key in ("discr_defaultDirichletOrder", "discr_defaultNeumannOrder"):
            if int(self.k.get(key, 1)) != 1:
                raise Exa4Unsupported("%s = %s: boundary conditions of order 2 on cell fields" % (key, self.k[key]))
        order = self._bc_kind(fd.bc)
        if order is not None and order != 1:
            raise Exa4Unsupported("field %s: Neumann(%d) -- boundary conditions of order 2 on cell fields" % (fd.name, order))
        self._cell_names.add(fd.name)
        ghost = tuple(ld.ghost[i] if i < nd and i < len(ld.ghost) else 0 for i in range(3))
        for lvl in self.levels_of(fd.levels):
            if (fd.name, lvl) in self.fields or not (self.min_level <= lvl <= self.max_level):
                continue
            nc = dom.ncells(lvl)
            lay = FieldLayout(nd, tuple(nc[i] if i < nd else 1 for i in range(3)), ghost, (0, 0, 0), (0, 0, 0), (0, 0, 0), ld.dup_comm,
                              ld.ghost_comm, localization="cell")
            f = Field(fd.name, lvl, lay, self.ops, nslots, None, ())
            if order is not None:
                f.cell_bc = (BC_NEUMANN, None)
            elif fd.bc is not None and fd.bc[0] == "call" and fd.bc[1] in self.functions:
                # a boundary function (`Field hu< global, L, wall_hu@finest ( ) >`): `apply bc` runs it; its ghost loops are faces of
                # examg_apply_bc_cell (exa4_conservation.py: _recognise_ghost_loop)
                if fd.bc[3]:
                    raise Exa4Unsupported("field %s: a boundary function with arguments" % fd.name)
                f.cell_bc = ("function", fd.bc[1])
            elif fd.bc is not None:
                f.cell_bc = (BC_DIRICHLET, self._cell_program(fd.bc, lvl))
            else:
                f.cell_bc = None
            self.fields[(fd.name, lvl)] = f

    def _cell_program(self, e, lvl: Optional[int]):
        """Expression program (examg_expr_t) of a point expression of a cell field: the cell-centre kernels evaluate it at the cell
        centres (loops) or at the face centres (boundary values), so it may read vf_cellCenter_* / vf_boundaryCoord_* but not the
        node position."""
        from .lib import ExprC

        for n in _walk(e):
            if n and n[0] == "id" and isinstance(n[1], str) and re.match(r"^vf_(nodePosition|nodePos)_", n[1]):
                raise Exa4Unsupported("%s in an expression of a cell field" % n[1])
        key = ("cellexpr", repr(e), lvl)
        if key not in self._fn_cache:
            try:
                self._fn_cache[key] = ExprC.from_program(self._compile_point_expr(e, lvl))
            except ValueError as ex:
                raise Exa4Unsupported(str(ex))
        return self._fn_cache[key]

    def _touches_cell(self, stmts) -> bool:
        """Does any field access in these statements name a cell field?"""
        if not self._cell_names:
            return False
        return any(n and n[0] == "fld" and n[1] in self._cell_names for n in _walk(("block", list(stmts))))

    def _check_cell_body(self, body, fr: _Frame) -> bool:
        """One loop body over cell fields (True) or node fields (False): never both, no node positions in a cell body and no cell
        centres in a node body, and stencils with axis entries only beside cell fields (a cell stencil with entries off the axes
        would read edge and corner ghosts, which examg_apply_bc_cell does not write)."""
        nodes = [n for n in _walk(("block", list(body))) if n and isinstance(n[0], str)]
        locs = {self._field(n, fr)[0].layout.localization for n in nodes if n[0] == "fld" and n[1] in self._cell_names} | \
            {"node" for n in nodes if n[0] == "fld" and n[1] not in self._cell_names}
        if len(locs) > 1:
            raise Exa4Unsupported("cell and node fields mixed in one loop body")
        cell = locs == {"cell"}
        for n in nodes:
            if cell and n[0] == "sten" and n[1] not in self.transfer and not (n[1] in self._stencil_decls and (self._coef_field(n[1]) is not None or self._coef_expr(n[1]) is not None)):
                A = self.stencil(n[1], self._level_of(n[2], fr))
                if not A.faces_only:
                    raise Exa4Unsupported("stencil %s on a cell field has entries off the axes (edge / corner ghosts are not set)" % n[1])
            if n[0] == "id" and isinstance(n[1], str):
                if not cell and re.match(r"^vf_cellCent(er|re)_", n[1]):
                    raise Exa4Unsupported("%s in a loop over node fields" % n[1])
                if cell and re.match(r"^vf_(nodePosition|nodePos)_", n[1]):
                    raise Exa4Unsupported("%s in a loop over cell fields" % n[1])
        return cell

    def _apply_layout_transformations(self):
        """`LayoutTransformations { transform <field>@<levels> with [x, y, z, i] => [i, x, y, z] }` on the coefficient field of a
        stencil field (Compiler/src/exastencils/layoutTransformation/l4/L4_LayoutSection.scala; Testing/LayoutTrafo/*.exa4): the
        entries of a point become contiguous -- APPLIED: loops read the coefficients through the transformed index
        (EXAMG_CLAYOUT_ENTRY_FASTEST), one stream instead of one per entry.  `transform <field> with [x, y, z] => [x / 2, y, z, x % 2]`
        (the colour split of Testing/LayoutTrafo/rbgs.exa4:2; 2-D: `[x, y] => [x / 2, y, x % 2]`) on a scalar field -- APPLIED on the
        HIP kernel layer: the field's arrays are allocated under EXAMG_LAYOUT_SPLIT_X and every loop reaches it through the
        transformed index (the points of one red-black colour of a row are contiguous: 32 B per update for a half sweep instead
        of 48); one-pass peepholes keep to plain fields.  The other directives of the reference's test programs (axis permutations,
        concat / rename of scalar fields) change no value either and stay recorded only."""
        import re

        self._sf_entry_fastest, self._sf_rec, self._sf_dirty = set(), {}, {}
        nd = self.nd
        src = ",".join("xyz"[:nd]) + ",i"
        dst = "i," + ",".join("xyz"[:nd])
        coef_of = {}
        for sf in self.ast.sfields:
            coef_of.setdefault(sf.field, []).append(sf)
        axes = "xyz"[:nd]
        split_src = ",".join(axes)
        split_dst = ",".join(["x/2"] + list(axes[1:]) + ["x%2"])
        self._split_fields = set()
        for text in getattr(self.ast, "layout_transformations", []):
            m = re.match(r"^transform (.+?) with \[(.+?)\] => \[(.+?)\]$", text.strip())
            if m and m.group(2).replace(" ", "") == split_src and m.group(3).replace(" ", "") == split_dst:
                self._apply_colour_split(m.group(1))
                continue
            if not m or m.group(2).replace(" ", "") != src or m.group(3).replace(" ", "") != dst:
                continue
            items, depth, cur = [], 0, []
            for tok in m.group(1).split(" "):          # items are separated by commas outside level lists
                depth += tok == "("
                depth -= tok == ")"
                if tok == "," and depth == 0:
                    items.append(cur)
                    cur = []
                else:
                    cur.append(tok)
            items.append(cur)
            for it in items:
                if not it:
                    continue
                fname, spec = it[0], " ".join(it[2:]) if len(it) > 2 and it[1] == "@" else "all"
                for sf in coef_of.get(fname, []):
                    lvls = self.levels_of(self._parse_level_text(spec))
                    for lvl in lvls:
                        if (sf.name, lvl) in self.stencils:
                            self._sf_entry_fastest.add((sf.name, lvl))

    def _transform_items(self, text: str):
        """(field name, levels) of the items of a `transform a@(..), b with ..` directive (items are separated by commas outside level lists)."""
        items, depth, cur = [], 0, []
        for tok in text.split(" "):
            depth += tok == "("
            depth -= tok == ")"
            if tok == "," and depth == 0:
                items.append(cur)
                cur = []
            else:
                cur.append(tok)
        items.append(cur)
        for it in items:
            if it:
                yield it[0], self.levels_of(self._parse_level_text(" ".join(it[2:]) if len(it) > 2 and it[1] == "@" else "all"))

    def _apply_colour_split(self, items: str):
        """The named scalar fields under `[x, y, z] => [x / 2, y, z, x % 2]`: their (still zero) arrays are re-allocated in the split
        layout.  Only where the kernel layer has transformed layouts (HipOps: examg_transform_field); the CPU stand-in of the tests
        keeps the directive recorded."""
        for fname, lvls in self._transform_items(items):
            if fname in self._complex_names:      # whatever the kernel layer: the complex kernels take untransformed layouts
                raise Exa4Unsupported("field %s: the colour-split layout of a complex field" % fname)
        if not hasattr(self.ops, "transform_field"):
            return
        for fname, lvls in self._transform_items(items):
            for lvl in lvls:
                f = self.fields.get((fname, lvl))
                if f is None or f.layout.transform:
                    continue
                f.layout = f.layout.split_x()
                f.lc = f.layout.c_struct()
                f.slots = [self.ops.new_array(f.layout.size) for _ in range(f.num_slots)]
                self._split_fields.add((fname, lvl))

    def _parse_level_text(self, spec: str):
        """Level specification of a LayoutTransformations item (`all`, `finest`, `4`, `(4 to finest)`) as the parser's level node."""
        from .exa4_parser import Parser

        return Parser("@ " + spec).decl_levels()

    def stencil(self, name: str, lvl: int) -> Stencil:
        """The stencil as loops use it: a stencil field whose coefficient field is under the entry-fastest layout transformation is
        handed out in that layout (re-laid out from the planes the initialisation statements write, when they have changed)."""
        s = self._stencil_planes(name, lvl)
        key = (name, lvl)
        if key in getattr(self, "_sf_entry_fastest", ()) and s.cfield is not None and hasattr(self.ops, "transform_stencilfield"):
            t = self._sf_rec.get(key)
            if t is None:
                t = self._sf_rec[key] = s.entry_fastest(self.ops)
                self.launches += 1
            elif self._sf_dirty.get(key, False):
                self.ops.transform_stencilfield(s.clayout.c_struct(), len(s.offsets), s.cfield, t.cfield, True)
                self.launches += 1
            self._sf_dirty[key] = False
            return t
        return s

    def _stencil_planes(self, name: str, lvl: int) -> Stencil:
        s = self.stencils.get((name, lvl))
        if s is None:
            sd = self._stencil_decl_at.get((name, lvl)) or self._stencil_decls.get(name)
            if sd is None:
                raise Exa4SyntaxError("stencil %s is not declared" % name)
            if lvl not in self.levels_of(sd.levels):
                raise Exa4SyntaxError("stencil %s is not declared on level %d" % (name, lvl))
            if self._coef_field(name) is not None:
                raise Exa4Unsupported("stencil %s is a point-wise coefficient stencil: it stands only in a system row (P * F) + .. + (L * F)" % name)
            if self._coef_expr(name) is not None:
                from .exa4_nonlinear import _FORMS

                raise Exa4Unsupported("coefficient-expression stencil %s outside the forms %s" % (name, _FORMS))
            fr = _Frame(lvl, {})
            if self.grid is not None and any(self._reads_grid(e) for _, e in sd.entries):
                # entries over the virtual fields of a non-uniform grid: per-axis tables, allocated once per level (examg_axis_op)
                s = self.stencils[(name, lvl)] = separate(name, sd.entries, self.nd, lvl, self.grid, lambda x: self._eval(x, fr))
                s.c_struct(self.ops)      # the tables go to the device here, never inside a recording
                return s
            offs = [tuple(o) + (0,) * (3 - len(o)) for o, _ in sd.entries]
            vals = [self._eval(e, fr) for _, e in sd.entries]      # entries over complex globals stay complex (exa4_complex.py)
            s = self.stencils[(name, lvl)] = Stencil(offs, [v if isinstance(v, complex) and v.imag != 0.0 else float(complex(v).real) for v in vals])
            s.has_complex_entries = any(isinstance(c, complex) for c in s.coefs)
        return s

    @staticmethod
    def _reads_grid(e) -> bool:
        """Does the expression name a virtual field of the grid (a width, a position, the cell volume)?"""
        return any(n and n[0] in ("id", "vfo") and isinstance(n[1], str) and n[1].startswith("vf_") for n in _walk(e))

    # -- analytic function recognition ----------------------------------------------------------------------------------
    def _point_eval(self, e, lvl: Optional[int], x: float, y: float, z: float):
        fr = _Frame(lvl, {"__x": x, "__y": y, "__z": z})
        return float(self._eval(e, fr))

    def _recognise(self, e, lvl: Optional[int]) -> Tuple[int, Tuple[float, ...]]:
        """Function id and parameters of include/examg.h that reproduce the point expression `e`."""
        key = (repr(e), lvl)
        if key in self._fn_cache:
            return self._fn_cache[key]
        pts = [(self._rng.uniform(0.05, 0.95), self._rng.uniform(0.05, 0.95), self._rng.uniform(0.05, 0.95)) for _ in range(12)]
        vals = [self._point_eval(e, lvl, *p) for p in pts]
        cands = [float(v) for v in self.globals.values() if isinstance(v, (int, float)) and not isinstance(v, bool)]
        for fn in range(_N_FN):
            if (fn in _FN_2D_ONLY) != (self.nd == 2) and fn not in _FN_ANY_DIM:
                continue
            for par in (cands if fn in _FN_WITH_PARAM else [None]):
                p = (par,) if par is not None else ()
                if all(abs(fn_eval(fn, p, *pt) - v) <= 1e-12 * max(1.0, abs(v)) for pt, v in zip(pts, vals)):
                    self._fn_cache[key] = (fn, p)
                    return fn, p
        raise Exa4Unsupported("analytic expression is none of the built-in point functions (include/examg.h EXAMG_FN_*)")

    def _compile_point_expr(self, e, lvl: Optional[int], subst: Optional[Dict[str, list]] = None) -> list:
        """Postfix program (include/examg.h EXAMG_OP_*) of an expression over the node position: operands in the order of
        the expression tree, user functions inlined, everything that does not depend on the position folded to constants
        exactly where the tree has it."""
        k = e[0]
        fr = _Frame(lvl, {})
        if k == "num":
            return [("const", float(e[1]))]
        if k == "neg":
            return self._compile_point_expr(e[1], lvl, subst) + [("neg", None)]
        if k == "fld" and subst is not None and "__u" in subst:
            return [("u", None)]          # the one field access of a coefficient expression: EXAMG_OP_U (exa4_nonlinear.py)
        if k == "vfo":
            raise Exa4Unsupported("point expression with the offset access %s@[...]" % e[1])
        if k == "id":
            name = e[1]
            if subst is not None and name in subst:
                return list(subst[name])
            m = _COORD.match(name)
            if m:
                if self.grid is not None and m.group(1).startswith("cellCent"):
                    raise Exa4Unsupported("%s on a non-uniform grid" % name)
                if self._node_ops and m.group(1).startswith("nodePos"):
                    return [("n" + m.group(2), None)]
                return [(m.group(2), None)]
            if self.grid is not None and name == CELL_VOLUME:       # the product of the widths of the point's cell
                prog = [("wx", None), ("wy", None), ("*", None)]
                return prog + ([("wz", None), ("*", None)] if self.nd == 3 else [])
            m = _GRIDW.match(name) if self.grid is not None else None
            if m and m.group(1) == "cellWidth":
                return [("w" + m.group(2), None)]
            return [("const", float(self._eval(e, fr)))]        # globals, PI, vf_gridWidth_*
        if k == "bin" and e[1] in ("+", "-", "*", "/"):
            return self._compile_point_expr(e[2], lvl, subst) + self._compile_point_expr(e[3], lvl, subst) + [(e[1], None)]
        if k == "bin" and e[1] == "**":
            base = self._compile_point_expr(e[2], lvl, subst)
            if e[3][0] == "num" and float(e[3][1]) == 2.0:
                return base + base + [("*", None)]                # the generator expands integer powers into products
            return base + self._compile_point_expr(e[3], lvl, subst) + [("pow", None)]
        if k == "call":
            name, args = e[1], e[3]
            if name in self.functions:
                fn = self._resolve(name, self._level_of(e[2], fr) if e[2] is not None else lvl)
                if len(fn.body) != 1 or fn.body[0][0] != "return" or fn.body[0][1] is None or len(fn.params) != len(args):
                    raise Exa4Unsupported("function %s inside a point expression must be a single return statement" % name)
                inner = {p: self._compile_point_expr(a, lvl, subst) for p, a in zip(fn.params, args)}
                return self._compile_point_expr(fn.body[0][1], lvl, inner)
            un = {"sin": "sin", "cos": "cos", "exp": "exp", "sinh": "sinh", "cosh": "cosh", "sqrt": "sqrt", "tan": "tan", "log": "log",
                  "fabs": "fabs", "abs": "fabs", "tanh": "tanh"}
            if name in un and len(args) == 1:
                return self._compile_point_expr(args[0], lvl, subst) + [(un[name], None)]
            if name in ("pow", "max", "min") and len(args) == 2:
                return self._compile_point_expr(args[0], lvl, subst) + self._compile_point_expr(args[1], lvl, subst) + [(name, None)]
        raise Exa4Unsupported("point expression with %s %r" % (k, e[1] if len(e) > 1 else ""))

    def _analytic(self, e, lvl: Optional[int]):
        """(fn id, params) of a built-in point function when the expression is one, else an expression program (ExprC)."""
        try:
            if self.grid is None:         # the built-in point functions are functions of a uniform grid's positions
                return self._recognise(e, lvl)
        except Exa4Unsupported:
            pass
        key = ("expr", repr(e), lvl)
        if key not in self._fn_cache:
            from .lib import ExprC

            try:
                self._fn_cache[key] = (ExprC.from_program(self._compile_point_expr(e, lvl)), ())
            except ValueError as ex:
                raise Exa4Unsupported(str(ex))
        return self._fn_cache[key]

    # -- expression evaluation (host scalars) ---------------------------------------------------------------------------
    def _level_of(self, spec, fr: _Frame) -> int:
        if spec is None:
            if fr.level is None:
                raise Exa4SyntaxError("leveled access without level outside a leveled function")
            return fr.level
        lv = self.levels_of(spec, fr.level)
        if len(lv) != 1:
            raise Exa4SyntaxError("access needs a single level")
        return lv[0]

    def _eval(self, e, fr: _Frame):
        k = e[0]
        if k == "num" or k == "str":
            return e[1]
        if k == "neg":
            return -self._eval(e[1], fr)
        if k == "not":
            return not self._eval(e[1], fr)
        if k == "bin":
            return _arith(e[1], self._eval(e[2], fr), self._eval(e[3], fr))
        if k == "id":
            name = e[1]
            if name in fr.vars:
                return fr.vars[name]
            if name in self.globals:
                return self.globals[name]
            if name == "PI":
                return math.pi
            m = _GRIDW.match(name)
            if m:
                if self.grid is not None:
                    raise Exa4Unsupported("%s on a non-uniform grid%s" % (name, "" if m.group(1) == "gridWidth" else
                                                                           " outside a stencil entry or a point expression"))
                return self.domain.h(self._level_of(e[2], fr))["xyz".index(m.group(2))]
            if name == CELL_VOLUME:       # uniform grid: the constant it is, the widths multiplied in axis order
                if self.grid is not None:
                    raise Exa4Unsupported("%s on a non-uniform grid outside a stencil entry or a point expression" % name)
                h = self.domain.h(self._level_of(e[2], fr))
                return h[0] * h[1] * h[2] if self.nd == 3 else (h[0] * h[1] if self.nd == 2 else h[0])
            if _EXPR + name in fr.vars or name in self._global_exprs():      # a scalar `Expr`: evaluated where it is used
                return self._eval(expand(("id", name, None), dict(self._global_exprs(), **self._expr_defs(fr))), fr)
            m = _COORD.match(name)
            if m:
                v = fr.vars.get("__" + m.group(2))
                if v is None:
                    raise Exa4Unsupported("%s outside a point expression" % name)
                return v
            raise Exa4SyntaxError("unknown name %r" % name)
        if k == "call":
            return self._call(e, fr)
        if k == "vfo":
            # a virtual field of the grid at a neighbouring cell: on a uniform grid widths and volumes are the constants they are
            if self.grid is None and (e[1] == CELL_VOLUME or _GRIDW.match(e[1])):
                return self._eval(("id", e[1], e[2]), fr)
            raise Exa4Unsupported("%s@[...] outside an entry of a stencil over the grid's virtual fields" % e[1])
        if k in ("fld", "sten", "sentry"):
            raise Exa4Unsupported("field / stencil access %s outside a recognised loop body" % e[1])
        raise Exa4SyntaxError("expression %r" % (e,))

    def _call(self, e, fr: _Frame):
        name, lspec, args = e[1], e[2], e[3]
        if name == "diag":
            a = args[0]
            if a[0] != "sten":
                raise Exa4Unsupported("diag of a non-stencil")
            st = self.stencil(a[1], self._level_of(a[2], fr))
            if getattr(st, "is_axis", False):
                raise Exa4Unsupported("diag of a stencil over the grid's virtual fields outside the smoother forms ((1.0 / diag(A)) * omega), (omega / diag(A))")
            if st.cfield is not None:
                raise Exa4Unsupported("diag of a stencil field outside the smoother form ((1.0 / diag(A)) * omega)")
            return st.diag
        if name in _MATH and name not in self.functions:
            return _MATH[name](*[self._eval(a, fr) for a in args])
        if name.split("_")[0] in ("printField", "writeField", "readField") and name not in self.functions:
            if self._has_vector and any(self._touches_vector(x) for x in args):
                raise Exa4Unsupported("%s: field I/O of vector-valued fields" % name)
            return self._field_io(name, args, fr)
        if self._has_vector and name not in self.functions and any(self._touches_vector(x) for x in args):
            raise Exa4Unsupported("%s ( .. ) outside a recognised loop: values of vector-valued fields and matrix stencils live in loop bodies" % name)
        if name in ("startTimer", "stopTimer", "getTotalFromTimer", "getTotalTime", "getMeanFromTimer") and args and \
                args[0][0] == "id" and args[0][1] not in fr.vars and args[0][1] not in self.globals:
            # timers may be named by a bare identifier (Testing/PolyExpl/Jac3Dcc.exa4:49: startTimer(benchTimer))
            args = [("str", args[0][1])] + list(args[1:])
        if name == "getKnowledge":
            key = self._eval(args[0], fr)
            return self.k.get(key, {"testing_enabled": False, "testing_printRes": True, "testing_printErr": True}.get(key, False))
        if name in self.functions:
            lvl = None
            if lspec is not None:
                lvl = self._level_of(lspec, fr)
            return self.call(name, lvl if lvl is not None else fr.level, [self._eval(a, fr) for a in args], fr)
        return self._builtin(name, [self._eval(a, fr) for a in args], fr)

    # -- functions ------------------------------------------------------------------------------------------------------
    def _resolve(self, name: str, lvl: Optional[int]) -> FunctionDecl:
        for fn in self.functions[name]:
            if fn.levels is None:
                return fn
            if lvl is not None and lvl in self.levels_of(fn.levels):
                return fn
        raise Exa4SyntaxError("function %s is not declared on level %r" % (name, lvl))

    def call(self, name: str, lvl: Optional[int] = None, args: Sequence = (), caller: Optional[_Frame] = None):
        fn = self._resolve(name, lvl)
        if self.auto_graph and self._graph_depth == 0 and fn.levels is not None and not fn.params and not args and \
                self._is_host_free(name, lvl) and self._call_through_graph(name, lvl):
            return None
        if self.fuse_coarse_solver and fn.levels is not None and lvl == self.min_level and not fn.params:
            plan = self._coarse_cg_plan(fn, lvl)
            if plan is not None:
                self._flush_pending()
                return self._run_coarse_cg(plan)
        fr = _Frame(lvl if fn.levels is not None else None, dict(zip(fn.params, args)))
        if caller is not None and "__x" in caller.vars:      # point expression: coordinates stay visible in callees
            for c in ("__x", "__y", "__z"):
                fr.vars.setdefault(c, caller.vars[c])
        try:
            self._exec_block(fn.body, fr, fn=True)
        except _Return as r:
            return r.value
        finally:
            if not self._cont:
                self._flush_pending()     # back at the caller of the interpreter: every field holds what the program says
        return None

    # -- functions that never return to the host, replayed from a hipGraph (auto_graph) -----------------------------------------------
    def _is_host_free(self, name: str, lvl: int) -> bool:
        """Can a call of this leveled function be issued without ever looking at a device value or doing host-visible work?  Decided
        from the program text: loops without reductions, `communicate` / `apply bc` / `advance`, repeats with literal counts, colour
        blocks, conditions and scalar statements without calls or field accesses, calls of functions that qualify themselves -- and
        the coarsest-level function when it is the generated CG solver (one kernel).  No statement below it may assign to a global
        (a replay would not); the globals it can read are what _graph_deps returns."""
        return self._graph_deps(name, lvl) is not None

    def _graph_deps(self, name: str, lvl: int) -> Optional[Tuple[str, ...]]:
        """None if calls of this function are never recorded, else the names of the globals a recording of it depends on (sorted):
        every global named in the function or in a function reachable from it -- in scalar arguments of loops, conditions, local
        declarations, point expressions.  Host work on the program text only."""
        key = (name, lvl)
        if not self._host_free_text(name, lvl):
            return None
        if key not in self._graph_reads:
            reads, assigned = self._globals_below(("call", name, None, []), set())
            if assigned:
                self._host_free[key] = False
                return None
            self._graph_reads[key] = tuple(sorted(reads))
        return self._graph_reads[key]

    def _globals_below(self, node, seen) -> Tuple[set, set]:
        """(globals read, globals assigned) by the statements / expressions of `node` and by every function they can call, whatever
        its level (every declaration of a called name counts: more than a call reaches, never less)."""
        reads, assigned = set(), set()
        for n in _walk(node):
            if len(n) >= 2 and n[0] == "id" and n[1] in self.globals:
                reads.add(n[1])
            elif len(n) == 3 and n[0] == "sten" and n[1] in self._stencil_decls and n[1] not in seen and self._coef_expr(n[1]) is not None:
                seen.add(n[1])      # a coefficient expression is compiled into every launch: its globals are the recording's
                reads |= self._globals_below(self._coef_expr(n[1]), seen)[0]
            elif len(n) == 4 and n[0] == "assign" and isinstance(n[2], tuple) and n[2][0] == "id" and n[2][1] in self.globals:
                assigned.add(n[2][1])
            elif len(n) == 2 and n[0] == "applybc" and isinstance(n[1], tuple) and n[1][0] == "fld":
                for (fname, _), f in self.fields.items():      # `apply bc` of a field with a boundary function runs that function
                    bf = getattr(f, "bc_function", None)
                    if bf is None and getattr(f, "cell_bc", None) is not None and f.cell_bc[0] == "function":
                        bf = f.cell_bc[1]      # ... of a cell field: its ghost loops may name globals in their values
                    if fname == n[1][1] and bf is not None and bf not in seen:
                        seen.add(bf)
                        for fn in self.functions[bf]:
                            r, a = self._globals_below(("block", list(fn.body)), seen)
                            reads |= r
                            assigned |= a
            elif len(n) == 4 and n[0] == "call" and n[1] in self.functions and n[1] not in seen:
                seen.add(n[1])
                for fn in self.functions[n[1]]:
                    r, a = self._globals_below(("block", list(fn.body)), seen)
                    reads |= r
                    assigned |= a
        return reads, assigned

    def _host_free_text(self, name: str, lvl: int) -> bool:
        """The structural half of _is_host_free: no statement below the function returns to the host."""
        key = (name, lvl)
        if key in self._host_free:
            return self._host_free[key]
        self._host_free[key] = False          # recursion at the same level: no
        try:
            fn = self._resolve(name, lvl)
            ok = fn.levels is not None and not fn.params
            if ok and self.fuse_coarse_solver and lvl == self.min_level and self._coarse_cg_plan(fn, lvl) is not None:
                ok = True
            elif ok:
                ok = self._host_free_body(fn.body, lvl)
        except (Exa4SyntaxError, Exa4Unsupported, KeyError, IndexError, TypeError):
            ok = False
        self._host_free[key] = ok
        return ok

    def _host_free_body(self, stmts, lvl: int) -> bool:
        def pure(e) -> bool:      # an expression without calls and field accesses
            if isinstance(e, (list, tuple)):
                if len(e) >= 1 and e[0] in ("call", "fld") and len(e) >= 4:
                    return False
                return all(pure(x) for x in e)
            return True

        for s in stmts:
            k = s[0]
            if k == "loop":
                if s[4] is not None:
                    return False
            elif k == "applybc":
                if not self._bc_function_host_free(s[1]):
                    return False
            elif k in ("comm", "advance"):
                continue
            elif k == "repeat":
                if s[1][0] != "num" or s[2] is not None or not self._host_free_body(s[3], lvl):
                    return False
            elif k in ("color", "repeatwith"):
                if not self._host_free_body(s[2], lvl):
                    return False
            elif k == "levelscope":
                if lvl in self.levels_of(s[1], lvl) and not self._host_free_body(s[2], lvl):
                    return False
            elif k == "if":
                if not pure(s[1]) or not self._host_free_body(s[2], lvl) or not self._host_free_body(s[3] or [], lvl):
                    return False
            elif k in ("decl", "assign"):
                e = s[2] if k == "decl" else s[3]
                if e is not None and not pure(e):
                    return False
            elif k == "callstmt":
                c = s[1]
                if c[0] != "call" or c[1] not in self.functions or c[3]:
                    return False
                clvl = self._level_of(c[2], _Frame(lvl, {})) if c[2] is not None else lvl
                if not self._is_host_free(c[1], clvl):
                    return False
            else:
                return False
        return True

    def _bc_function_host_free(self, target) -> bool:
        """`apply bc` of a cell field with a boundary function runs that function: its statements (a timer around the ghost loops, a
        print) count like those of a called function."""
        for (fname, flvl), f in self.fields.items():
            bc = getattr(f, "cell_bc", None)
            if fname == target[1] and bc is not None and bc[0] == "function":
                if not all(self._host_free_body(fn.body, flvl) for fn in self.functions[bc[1]]):
                    return False
        return True

    def _host_state(self):
        """What executing statements changes on the HOST side (boundary bookkeeping, second arrays, slots): saved before a function is
        recorded, put back if the recording is discarded (its launches were never issued)."""
        return {"bc_valid": set(self._bc_valid), "bc_epoch": dict(self._bc_epoch), "alt": dict(self._alt), "alt_shell": dict(self._alt_shell),
                "pair_tmp": dict(self._pair_tmp), "sf_dirty": dict(self._sf_dirty), "sf_rec": dict(self._sf_rec),
                "fields": {k: (list(f.slots), f.current_slot) for k, f in self.fields.items()},
                "cg": (getattr(self, "_cg_tail", None), getattr(self, "_cg_info", None))}

    def _restore_host_state(self, st):
        """Impose a saved host state (copies: the saved one stays what it was)."""
        self._bc_valid, self._bc_epoch, self._alt, self._alt_shell = set(st["bc_valid"]), dict(st["bc_epoch"]), dict(st["alt"]), dict(st["alt_shell"])
        self._pair_tmp, self._sf_dirty, self._sf_rec = dict(st["pair_tmp"]), dict(st["sf_dirty"]), dict(st["sf_rec"])
        for k, (slots, cur) in st["fields"].items():
            self.fields[k].slots, self.fields[k].current_slot = list(slots), cur
        for attr, v in zip(("_cg_tail", "_cg_info"), st["cg"]):
            if v is None and hasattr(self, attr):
                delattr(self, attr)
            elif v is not None:
                setattr(self, attr, v)

    def _graph_guard(self, key: Tuple[str, int]):
        """What the launches of a call of the recordable function `key`, and their scalar arguments, are decided from, as it stands
        now: the array roles; type and value of every global the function can read (_graph_deps); the interpreter's bookkeeping --
        which boundary planes hold their Dirichlet values, the boundary epochs and the shells of the second arrays, the stencil
        fields whose entry-fastest copy is out of date, which scratch fields and transformed copies exist -- taken whole; the call
        site (the liveness scan of the cross-statement fusions reads on into the caller); the switches of the one-pass forms.  Two
        calls with equal guards issue the same launches.  Host work only, no kernel-layer call."""
        g = self.globals
        return (self._roles(), tuple((g[n].__class__, g[n]) for n in self._graph_reads[key]), set(self._bc_valid), dict(self._bc_epoch),
                dict(self._alt_shell), {k for k, v in self._sf_dirty.items() if v}, set(self._pair_tmp), set(self._sf_rec),
                [(id(body), i) for body, i, _fr, _loop, _fn in self._cont],
                (self.fuse, self.fuse_coarse_solver, self.fuse_residual_norm, self.fused_prolong_min_points, self.fuse_min_row,
                 self.fuse_min_row_blocks, id(getattr(self, "_cg_info", None))))

    def _call_through_graph(self, name: str, lvl: int) -> bool:
        """True if the call was issued as a graph replay -- never while a loop of the caller's is pending, and never for a function that
        leaves a loop pending: the launches of such a call are not the function's alone.  First call: interpreted (lazily created arrays
        come into being); second call: recorded -- the interpreter runs the function while the kernel layer records, nothing executes
        -- and replayed once; afterwards: replayed whenever the guard (_graph_guard) equals the one the recording was made under,
        interpreted otherwise -- and recorded anew when two calls in a row meet the same other guard.  After a replay the host state is
        the one the recorded call left."""
        ops = self.ops
        key = (name, lvl)
        rec = self._auto_graphs.get(key)
        if rec is False or self._pending is not None or ops.graph_capturing():
            return False                      # (a pending loop of the caller's: interpretation may absorb it into a pass of this function)
        guard = self._graph_guard(key) if rec is not None or self._auto_calls.get(key, 0) >= 1 else None
        fresh = rec is None
        if not fresh and guard != rec["guard"]:
            # interpreting this call would not issue what was recorded.  A guard seen for the first time: interpret; the guard the
            # call before was interpreted under: the program has settled in another state, which is recorded in place of the old one
            fresh, rec["missed"] = rec["missed"] == guard, guard
            if not fresh:
                return False
        if fresh:
            n = self._auto_calls[key] = self._auto_calls.get(key, 0) + 1
            if n < 2:
                return False
            l0, f0 = self.launches, dict(self.fusions)
            saved = self._host_state()
            self._graph_depth += 1
            try:
                g = ops.graph_begin()
                try:
                    fn = self._resolve(name, lvl)
                    self._exec_block(fn.body, _Frame(lvl, {}), fn=True)
                    # a loop the function leaves pending may end in a one-pass form with its caller's next statement (which need not
                    # store what the loop alone stores): such a function is interpreted, like one that leaves arrays in other roles
                    left_pending = self._pending is not None
                    self._flush_pending()     # (recorded all the same: a recording without a launch draws a warning from the runtime)
                finally:
                    ops.graph_end(g)
                ok = not left_pending and self._roles() == guard[0]
            except (RuntimeError, Exa4Unsupported, _Return):
                ok = False
            finally:
                self._graph_depth -= 1
            recorded, fused = self.launches - l0, {k: v - f0.get(k, 0) for k, v in self.fusions.items()}
            self.launches, self.fusions = l0, f0
            if not ok or recorded == 0:
                # nothing of the recording was issued: the interpreter's bookkeeping goes back to where it was, the real call follows
                self._pending = None
                self._restore_host_state(saved)
                self._auto_graphs[key] = False
                return False
            rec = self._auto_graphs[key] = {"graph": g, "guard": guard, "exit": self._host_state(), "launches": recorded, "fusions": fused,
                                            "missed": None, "replays": 0 if rec is None else rec["replays"]}
        ops.graph_replay(rec["graph"])
        if not fresh:
            self._restore_host_state(rec["exit"])
        rec["missed"] = None
        rec["replays"] += 1
        self.launches += rec["launches"]
        for k, v in rec["fusions"].items():
            self.fusions[k] = self.fusions.get(k, 0) + v
        self.graph_replays += 1
        return True

    # -- hipGraph capture of a function call ----------------------------------------------------------------------------------
    def _roles(self):
        st = [(k, tuple(t.data_ptr() for t in f.slots), f.current_slot) for k, f in sorted(self.fields.items())]
        return st, sorted((k, v.data_ptr()) for k, v in self._alt.items())

    def capture(self, name: str, lvl: Optional[int] = None, args: Sequence = ()):
        """Record one call of a function (typically the cycle function on the finest level) into a hipGraph and return it;
        `graph.replay()` then re-issues all its kernels without host work.  The call must be free of host-visible
        reductions (a generated coarse-grid CG qualifies through examg_cg_coarse) and must leave every array in the role
        it had before (an even number of out-of-place sweeps / slot advances).

        Unlike `auto_graph`, the explicit form checks nothing at a replay: the graph holds the launches and the scalar arguments of
        the recorded call.  The caller must capture again after changing a global the function reads, after rewriting boundary
        planes (`loop over .. only ..`, readField) or the coefficients of a stencil field, and after anything else that changes the
        roles of the arrays; while none of these happens a replay is the call, bit for bit."""
        torch = self.ops.torch
        dev = self.ops.device
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        # twice outside the capture: lazily created second arrays / scratch fields exist and carry their boundary planes
        for _ in range(2):
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self.call(name, lvl, args)
            cur.wait_stream(side)
        before = self._roles()
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g):
                self.call(name, lvl, args)
        except RuntimeError as ex:
            raise Exa4Unsupported("%s cannot be captured (host-visible reduction or allocation inside?): %s" % (name, ex))
        if self._roles() != before:
            raise Exa4Unsupported("%s leaves arrays in other roles than it found them: a replay would read stale data" % name)
        return g

    def run(self, name: str = "Application"):
        self.call(name)
        self._flush_cg_limit()
        self.comm.check()         # a wait of the peer-write transport that gave up is an error of the run, not silent garbage
        return self.out

    def _flush_cg_limit(self):
        """The one-call coarse solve counts on the device how often its loop ran out of iterations (info[3]); the statements the
        program has after that loop -- a print -- run that often when the program ends."""
        if not hasattr(self, "_cg_tail"):
            return
        tail, lvl = self._cg_tail
        n = int(self.ops.to_host(self._cg_info)[3])
        for _ in range(n - getattr(self, "_cg_limit_seen", 0)):
            self._exec_block(tail, _Frame(lvl, {}))
        self._cg_limit_seen = n

    # -- statements -----------------------------------------------------------------------------------------------------
    def _exec_block(self, body: list, fr: _Frame, loop: bool = False, fn: bool = False):
        """loop: the list is a loop body that may run again; fn: a function body (a `return` ends here).  The stack of active lists
        is what the liveness scan of the cross-statement fusions walks (exa4_fusion.py: _dead_after).  A variable declared in the
        body of a repeat loop lives for one pass, as in the generated block: the CG of Benchmark/OptFlow2D/2D_FD_OptFlow.exa4 declares
        `Var alpha` at the end of a pass whose first statements mean the global `alpha`."""
        entry = [body, 0, fr, loop, fn]
        self._cont.append(entry)
        outer = dict(fr.vars) if loop and any(st[0] == "decl" for st in body) else None
        try:
            i = 0
            while i < len(body):
                entry[1] = i
                self._exec(body[i], fr)
                i += 1
        finally:
            self._cont.pop()
            if outer is not None:
                declared = {st[1] for st in body if st[0] == "decl"}
                for name in declared:
                    if name in outer:
                        fr.vars[name] = outer[name]
                    else:
                        fr.vars.pop(name, None)

    def _field(self, e, fr: _Frame) -> Tuple[Field, int]:
        if e[0] != "fld":
            raise Exa4SyntaxError("field access expected, found %r" % (e,))
        lvl = self._level_of(e[3], fr)
        f = self.fields.get((e[1], lvl))
        if f is None:
            raise Exa4SyntaxError("field %s is not declared on level %d" % (e[1], lvl))
        s = e[2]
        if s is None or s in ("active", "activeSlot", "current", "currentSlot"):
            slot = f.active
        elif s in ("next", "nextSlot"):
            slot = f.next
        elif s in ("previous", "previousSlot"):
            slot = (f.current_slot - 1) % f.num_slots
        else:
            slot = int(s) % f.num_slots
        return f, slot

    def _exec(self, s, fr: _Frame):
        k = s[0]
        if self._pending is not None and self._gate(s, fr):
            return
        if k == "decl":
            if s[2] is not None and self._has_vector and self._touches_vector(s[2]):
                raise Exa4Unsupported("variable %s: matrix-typed Var / Val and values of vector-valued fields outside a loop" % s[1])
            fr.vars[s[1]] = self._eval(s[2], fr) if s[2] is not None else 0
        elif k == "exprdecl":
            fr.vars[_EXPR + s[1]] = s[3]      # a macro: substituted where it is used (exa4_conservation.py)
        elif k == "assign":
            op, lhs, rhs = s[1], s[2], s[3]
            if lhs[0] != "id":
                raise Exa4Unsupported("assignment to %s outside a loop" % lhs[0])
            v = self._eval(rhs, fr)
            tgt = fr.vars if lhs[1] in fr.vars or lhs[1] not in self.globals else self.globals
            tgt[lhs[1]] = v if op == "=" else _arith(op[0], tgt[lhs[1]], v)
        elif k == "callstmt":
            self._call(s[1], fr)
        elif k == "loop":
            self._exec_loop(s, fr)
        elif k == "comm":
            if s[1] == "finish":
                return
            f, slot = self._field(s[3], fr)
            if f.layout.is_complex or f.layout.is_vector:      # one block without periodic axes (checked where the field is declared): nothing to exchange
                return
            self.comm.exchange(f, slot, s[2])
        elif k == "applybc":
            f, slot = self._field(s[1], fr)
            self._apply_bc(f, slot)
        elif k == "advance":
            f, _ = self._field(s[1], fr)
            f.advance()
        elif k == "repeat":
            n = int(self._eval(s[1], fr))
            if self.fuse and s[2] is None and n >= 2 and self._try_jacobi_pairs(s[3], n, fr):
                return
            for it in range(n):
                if s[2]:
                    fr.vars[s[2]] = it
                self._exec_block(s[3], fr, loop=True)
            if s[2]:
                fr.vars[s[2]] = n
        elif k == "contract":
            if self._has_vector and self._touches_vector(("block", list(s[5]))):
                raise Exa4Unsupported("repeat ... with contraction over vector-valued fields")
            self._exec_contract(s, fr)
        elif k == "until":
            while not self._eval(s[1], fr):
                self._exec_block(s[2], fr, loop=True)
        elif k == "if":
            self._exec_block(s[2] if self._eval(s[1], fr) else s[3], fr)
        elif k == "color":
            shift = _parity_expr(s[1][0], self.nd) if len(s[1]) == 1 else None
            if shift is None:
                return self._exec_multicolour(s, fr)
            if self.fuse and self._try_fused_sweep(s[2], (0 - shift) % 2, fr):
                return
            saved = fr.colour
            for c in (0, 1):
                fr.colour = (c - shift) % 2
                self._exec_block(s[2], fr)
            fr.colour = saved
        elif k == "repeatwith":
            # `repeat with { cond, cond, <statements> }`: the statements once per condition; a colour test becomes the colour of the loops inside
            if fr.colour is not None or fr.mcolour is not None:
                raise Exa4Unsupported("repeat with inside a coloured block")
            cols = [_colour_cond(c, self.nd) for c in s[1]]
            if any(c is None for c in cols):
                raise Exa4Unsupported("repeat with: a condition other than c == ((i0 + i1 [+ i2]) % 2)")
            try:
                for c in cols:
                    fr.colour = c
                    self._exec_block(s[2], fr)
            finally:
                fr.colour = None
        elif k == "levelscope":
            if fr.level in self.levels_of(s[1], fr.level):
                self._exec_block(s[2], fr)
        elif k == "return":
            raise _Return(self._eval(s[1], fr) if s[1] is not None else None)
        else:
            raise Exa4SyntaxError("statement %r" % (k,))

    def _exec_multicolour(self, s, fr: _Frame):
        """`color with { e_0 [, e_1 [, e_2]], <statements> }` with anything but the one parity expression of all indices
        (baseExt/l4/L4_ColorLoops.scala:32-66): the statements run once per element of the cross product of the remainders, the
        first expression varying fastest; loops inside take the points of the current colour (examg_stencil_op_coloured)."""
        from .field import Colouring

        if len(s[1]) > 3:
            raise Exa4Unsupported("color with more than three colour expressions")
        exprs = []
        for e in s[1]:
            ce = _colour_expr(e, self.nd)
            if ce is None:
                raise Exa4Unsupported("colour expression other than (s + i_a [+ i_b [+ i_c]]) % n with a positive integer n")
            exprs.append(ce)
        if fr.colour is not None or fr.mcolour is not None:
            raise Exa4Unsupported("color with inside color with")
        col = Colouring(tuple(exprs))
        if self.fuse and self._try_mcgs_sweep(s[2], col, fr):
            return
        try:
            for c in col.colours():
                fr.mcolour = c
                self._exec_block(s[2], fr)
        finally:
            fr.mcolour = None

    def _exec_loop_multicolour(self, s, fr: _Frame):
        """A `loop over` inside a multi-colouring: the stencil loops (A * u, f - A * u, the damped-residual update) on the points of
        the current colour.  Everything else has no coloured kernel and is refused by name."""
        _, target, only, where, reduction, body = s
        f, _ = self._field(target, fr)
        if f.layout.is_cell or self._touches_cell(body):
            raise Exa4Unsupported("cell fields in a loop under a multi-colouring (color with several expressions)")
        if reduction is not None:
            raise Exa4Unsupported("reduction loop under a multi-colouring (color with several expressions)")
        if only is not None or fr.contract is not None:
            raise Exa4Unsupported("loop ... only <region> / contraction under a multi-colouring (color with several expressions)")
        if where is not None and any(_colour_cond(c, self.nd) is not None for c in _conjuncts(where)):
            raise Exa4Unsupported("`where` colour test in a loop under a multi-colouring (color with several expressions)")
        boxes, _ = self._loop_boxes(f, only, where, reduction, fr)
        if any(st[0] == "solve" for st in body):      # the collective smoother of a block system (exa4_blocksys.py): one launch per colour
            if len(body) != 1:
                raise Exa4Unsupported("solve locally beside other statements, in a reduction or in an `only` loop")
            return self._exec_solve_locally(body[0], boxes, None, fr, only, where)
        for st in body:
            if st[0] != "assign":
                raise Exa4Unsupported("statement %r inside a loop body" % st[0])
            for b, e in boxes:
                self._exec_point_assign_multicolour(st, b, e, fr)

    def _exec_point_assign_multicolour(self, st, b, e, fr: _Frame):
        what = "under a multi-colouring (color with several expressions)"
        if st[2][0] != "fld":
            self._recognise_assign(st, fr)      # names what the loop assigns to
        if self._names_coef_expr(st[3]):
            raise Exa4Unsupported("semilinear operator (coefficient-expression stencil) %s" % what)
        if st[1] == "=" and st[2][0] == "fld":
            self._recognise_block_row(*self._field(st[2], fr), st[3], None, fr)      # a system row here is refused by name
        k = self._recognise_or_none(st, fr)     # whatever the recogniser refuses has no coloured kernel either
        if k is None or not self._launch_coloured(k, b, e, fr.mcolour):
            raise Exa4Unsupported("loop body statement %s %s ... %s: only stencil loops (A * u, f - A * u, u + w * (f - A * u)) have a coloured kernel"
                                  % (st[2][1], st[1], what))

    def _apply_bc(self, f: Field, slot: int):
        if f.layout.is_vector:
            return self._apply_bc_vector(f, slot)
        if f.layout.is_cell:
            # a ghost value is a function of the interior: written every time, never assumed valid
            mask = self.domain.face_mask()
            if f.cell_bc is not None and f.cell_bc[0] == "function":
                if slot != f.active:
                    raise Exa4Unsupported("apply bc to a slot of %s other than the active one: its boundary function names the active slot" % f.name)
                self.call(f.cell_bc[1], f.level)
            elif f.cell_bc is not None and mask:
                self.launches += 1
                self.ops.apply_bc_cell(f.lc, f.data(slot), self.domain.geom(f.level), f.cell_bc[0], f.cell_bc[1], mask)
            return
        if getattr(f, "bc_function", None) is not None:      # a boundary function of a complex node field (exa4_complex.py)
            self._bc_depth += 1
            try:
                self.call(f.bc_function, f.level)
            finally:
                self._bc_depth -= 1
            return
        if f.bc_fn is None:
            return
        if self.fuse and (f.name, f.level, slot) in self._bc_valid:
            # Dirichlet values are functions of the position: the planes already hold exactly what this statement would write (every
            # writer of boundary planes -- `loop over .. only ..`, readField -- takes the entry out of _bc_valid) -- no launch, no bit changes
            return
        self._bc_valid.add((f.name, f.level, slot))
        mask = self.domain.face_mask()
        if mask:
            self.launches += 1
            if self.grid is not None:
                self.ops.apply_dirichlet_expr_grid(f.lc, f.data(slot), self.grid.device(self.ops, f.level), f.bc_fn, mask)
            elif isinstance(f.bc_fn, int):
                self.ops.apply_dirichlet(f.lc, f.data(slot), self.domain.geom(f.level), f.bc_fn, f.bc_params, mask)
            else:
                self.ops.apply_dirichlet_expr(f.lc, f.data(slot), self.domain.geom(f.level), f.bc_fn, mask)

    # -- loops ----------------------------------------------------------------------------------------------------------
    def _loop_boxes(self, f: Field, only, where, reduction, fr: _Frame):
        """Iteration boxes of the loop and the colour its condition selects (None: all points)."""
        dom, lay, nd = self.domain, f.layout, self.nd
        colour = fr.colour
        lower = [False] * 3
        if where is not None:
            for c in _conjuncts(where):
                par = _colour_cond(c, nd)
                d = _lower_cond(c)
                if par is not None:
                    colour = par
                elif d is not None:
                    lower[d] = True
                else:
                    raise Exa4Unsupported("loop condition other than a colour test or (i_d > 0)")
        if only is not None:
            # `only <region> [dir] [on boundary]` (baseExt/ir/IR_LoopOverPointsInOneFragment.scala:57-72, 293-299): per dimension the
            # region's whole extent <R>LB..<R>RE where dir is 0, its lower part <R>LB..<R>LE / upper part <R>RB..<R>RE where dir is
            # -1 / +1, no iteration offsets; `on boundary`: only where the block has no neighbour in that direction
            region, direction, on_boundary = only
            code = {"dup": "D", "ghost": "G", "inner": "I"}.get(region)
            if code is None:
                raise Exa4Unsupported("loop ... only %s" % region)
            direction = tuple(direction) + (0,) * (3 - len(direction))
            if on_boundary:
                nz = [d for d in range(nd) if direction[d] != 0]
                if len(nz) != 1:
                    raise Exa4Unsupported("loop only ... on boundary: axis directions only")
                if dom.neighbor(nz[0], direction[nz[0]]) is not None:
                    return [], colour
            b, e = [0, 0, 0], [1, 1, 1]
            for t in range(nd):
                if code == "I":
                    lo_b, lo_e, hi_b, hi_e = "IB", "IE", "IB", "IE"
                else:
                    lo_b, lo_e, hi_b, hi_e = code + "LB", code + "LE", code + "RB", code + "RE"
                if direction[t] == 0:
                    b[t], e[t] = lay.idx(lo_b, t), lay.idx(hi_e, t)
                elif direction[t] < 0:
                    b[t], e[t] = lay.idx(lo_b, t), lay.idx(lo_e, t)
                else:
                    b[t], e[t] = lay.idx(hi_b, t), lay.idx(hi_e, t)
            return [(b, e)], colour
        b, e = dom.loop_bounds(lay, reduction is not None)
        for d in range(nd):
            if lower[d]:
                b[d] = max(b[d], 1)
        if fr.contract is not None and reduction is None:
            b, e = self._contract_bounds(lay, b, e, *fr.contract)
        return [(b, e)], colour

    def _contract_bounds(self, lay, b, e, extent: int, pos, neg):
        """Loop bounds inside `repeat n times with contraction`: widened by `extent` x the contraction per side at interior faces
        (iteration offset 0), unchanged on physical boundaries (IR_ContractingLoop.extendBoundsBegin / End,
        Compiler/src/exastencils/baseExt/ir/IR_ContractingLoop.scala:45-87); the layers computed redundantly must exist."""
        b, e = list(b), list(e)
        for d in range(self.nd):
            if self.domain.neighbor(d, -1) is not None:
                b[d] -= extent * (neg[d] if d < len(neg) else 0)
            if self.domain.neighbor(d, +1) is not None:
                e[d] += extent * (pos[d] if d < len(pos) else 0)
            if b[d] - 1 < lay.idx("GLB", d) or e[d] + 1 > lay.idx("GRE", d):
                raise Exa4Unsupported("contraction by %d layers needs deeper ghost layers than the layout has" % extent)
        return b, e

    def _exec_loop(self, s, fr: _Frame):
        _, target, only, where, reduction, body = s
        f, _ = self._field(target, fr)
        if self._has_vector and (f.layout.is_vector or self._touches_vector(("block", list(body)))):
            return self._exec_vector_loop(s, f, fr)      # (exa4_vector.py)
        if id(s) in self._bc_taken:                       # a ghost loop that went into the launch of the one before it
            self._bc_taken.discard(id(s))
            return
        ghost = self._recognise_ghost_loop(s, f, fr)      # a boundary function's loop over one face (exa4_conservation.py)
        if ghost is not None:
            return self._launch_bc_faces(self._merge_bc_faces(ghost, fr))
        if f.layout.is_complex and only is not None:
            return self._exec_complex_only_loop(s, f, fr)
        if only is not None and not f.layout.is_cell and any(n and n[0] == "off" and n[1][0] == "fld" for n in _walk(("block", list(body)))):
            raise Exa4Unsupported("loop over %s only %s %s: an offset access in a loop over a region of a real node field (boundary functions "
                                  "exist for cell fields and complex node fields)" % (f.name, only[0], list(only[1])))
        if f.layout.is_complex and (where is not None or fr.mcolour is not None):
            raise Exa4Unsupported("loop over complex field %s %s" % (f.name, "with a `where` condition" if where is not None else
                                                                      "under a multi-colouring (color with several expressions)"))
        if self._check_cell_body(body, fr) and not f.layout.is_cell:
            raise Exa4Unsupported("loop over node field %s with a body over cell fields" % f.name)
        if f.layout.is_cell and (only is not None or fr.contract is not None):
            raise Exa4Unsupported("loop over cell field %s: `only` regions and contraction" % f.name)
        if fr.mcolour is not None:
            return self._exec_loop_multicolour(s, fr)
        boxes, colour = self._loop_boxes(f, only, where, reduction, fr)
        flux = self._recognise_flux_loop(body, f, only, where, reduction, colour, fr)      # the whole body as ONE explicit update
        if flux is not None:
            for b, e in boxes:
                self._launch(flux, b, e, None)
            return
        if any(st[0] == "solve" for st in body):
            if len(body) != 1 or reduction is not None or only is not None:
                raise Exa4Unsupported("solve locally beside other statements, in a reduction or in an `only` loop")
            return self._exec_solve_locally(body[0], boxes, colour, fr, only, where)
        if reduction is not None:
            return self._exec_reduction(f, boxes, reduction, body, fr)
        if body and all(st[0] == "assign" and st[2][0] == "sentry" for st in body):
            return self._exec_stencil_field_init(body, boxes, fr)
        if (body and colour is None and all(st[0] == "assign" and st[1] == "=" and st[2][0] == "fld" and self._is_std_rand(st[3])
                                            for st in body)):
            return self._exec_rand_fill([st[2] for st in body], boxes, fr)
        cmp_ = self._match_compare_loop(body, fr)
        if cmp_ is not None and colour is None:
            return self._exec_compare_loop(cmp_, boxes, fr)
        if colour is None and self._is_check_loop(body):
            return self._exec_check_loop(body, boxes, fr)
        if (len(body) == 1 and len(boxes) == 1 and colour is None and only is None and where is None and fr.contract is None
                and self._try_defer(body[0], f, boxes[0], fr)):
            return      # absorbed by a one-pass form later, or run when the next statement could tell the difference
        if (only is not None or fr.contract is not None) and self._names_coef_expr(("block", list(body))):
            raise Exa4Unsupported("semilinear operator in a loop with an `only` region or under contraction")
        folded = 0
        for i, st in enumerate(body):
            if folded:      # a system row that went into the launch of the row before it (exa4_blocksys.py)
                folded -= 1
                continue
            if st[0] != "assign":
                raise Exa4Unsupported("statement %r inside a loop body" % st[0])
            if only is not None and st[2][0] == "fld":      # boundary planes rewritten: second arrays of fused sweeps are stale
                tf = self._field(st[2], fr)[0]
                self._bc_epoch[(tf.name, tf.level)] = self._bc_epoch.get((tf.name, tf.level), 0) + 1
                self._bc_valid -= {(tf.name, tf.level, sl) for sl in range(tf.num_slots)}
            for b, e in boxes:
                k = self._recognise_assign(st, fr, colour)
                if self._is_lexicographic(k, colour):
                    self._check_lexicographic(k, only, where, fr)
                if k.kind == "bsys_row":
                    self._check_block_loop(only, where, fr)
                    k, folded = self._merge_block_rows(k, body[i + 1:], fr)
                self._launch(k, b, e, colour)

    def _exec_reduction(self, f: Field, boxes, reduction, body, fr: _Frame):
        op, var = reduction
        locals_: Dict[str, object] = {}
        for st in body:
            if st[0] == "decl":
                locals_[st[1]] = st[2]
                continue
            if st[0] != "assign" or st[2] != ("id", var, None):
                raise Exa4Unsupported("reduction loop body")
            rhs = st[3]
            if op == "+" and st[1] == "+=" and rhs[0] == "fld":           # s += F
                X, xs = self._field(rhs, fr)
                acc = 0.0
                for b, e in boxes:
                    self.launches += 1
                    acc += self.comm.reduce_value(self.ops.sum(X.lc, X.data(xs), b, e), "sum")
                fr.vars[var] = fr.vars[var] + acc
                continue
            if op == "+" and st[1] == "+=" and rhs[0] == "bin" and rhs[1] == "*" and rhs[2][0] == "fld" and rhs[3][0] == "fld":
                X, xs = self._field(rhs[2], fr)
                Y, ys = self._field(rhs[3], fr)
                if X.layout.is_complex or Y.layout.is_complex:
                    fr.vars[var] = fr.vars[var] + self._complex_dot(X, xs, Y, ys, boxes)
                    continue
                acc = 0.0
                for b, e in boxes:
                    self.launches += 1
                    t = self.ops.dot(X.lc, X.data(xs), Y.lc, Y.data(ys), b, e)
                    acc += self.comm.reduce_value(t, "sum")
                fr.vars[var] = fr.vars[var] + acc
                continue
            if op == "max" and st[1] == "=" and rhs[0] == "call" and rhs[1] == "max" and len(rhs[3]) == 2:
                other = [a for a in rhs[3] if a != ("id", var, None)]
                if len(other) == 1:
                    t = other[0]
                    if t[0] == "id" and t[1] in locals_:
                        t = locals_[t[1]]
                    if t[0] == "call" and t[1] in ("fabs", "abs") and t[3][0][0] == "bin" and t[3][0][1] == "-" and t[3][0][2][0] == "fld":
                        X, xs = self._field(t[3][0][2], fr)
                        acc = fr.vars[var]
                        if X.layout.is_cell:
                            prog = self._cell_program(t[3][0][3], X.level)
                            for b, e in boxes:
                                self.launches += 1
                                r = self.ops.max_err_expr_cell(X.lc, X.data(xs), self.domain.geom(X.level), prog, b, e)
                                acc = max(acc, self.comm.reduce_value(r, "max"))
                            fr.vars[var] = acc
                            continue
                        fn, par = self._analytic(t[3][0][3], X.level)
                        for b, e in boxes:
                            self.launches += 1
                            if self.grid is not None:
                                r = self.ops.max_err_expr_grid(X.lc, X.data(xs), self.grid.device(self.ops, X.level), fn, b, e)
                            elif isinstance(fn, int):
                                r = self.ops.max_err_fn(X.lc, X.data(xs), self.domain.geom(X.level), fn, par, b, e)
                            else:
                                r = self.ops.max_err_expr(X.lc, X.data(xs), self.domain.geom(X.level), fn, b, e)
                            acc = max(acc, self.comm.reduce_value(r, "max"))
                        fr.vars[var] = acc
                        continue
            k = self._recognise_reduce_expr(op, var, st, locals_, f, fr)      # max | min of a point expression over cell fields
            if k is not None:
                tgt = fr.vars if var in fr.vars or var not in self.globals else self.globals
                acc = tgt[var]
                for b, e in boxes:
                    r = self.comm.reduce_value(self._launch(k, b, e, None), op)
                    acc = max(acc, r) if op == "max" else min(acc, r)
                tgt[var] = acc
                continue
            raise Exa4Unsupported("reduction %s over this loop body" % op)

    def _exec_stencil_field_init(self, body, boxes, fr: _Frame):
        """`A:[o] = expr` for every entry of a 7/5-entry stencil field: -div(a grad) with a at the half points."""
        name = body[0][2][1]
        lvl = self._level_of(body[0][2][2], fr)
        if self.grid is not None:
            raise Exa4Unsupported("initialisation of stencil field %s on a non-uniform grid" % name)
        A = self._stencil_planes(name, lvl)       # initialisation statements write the planes; loops get the transformed copy
        if A.cfield is None:
            raise Exa4Unsupported("%s is not a stencil field" % name)
        if hasattr(self, "_sf_dirty"):
            self._sf_dirty[(name, lvl)] = True
        nd = self.nd
        want = [(0, 0, 0)]
        for d in range(nd):
            for sgn in (1, -1):
                o = [0, 0, 0]
                o[d] = sgn
                want.append(tuple(o))
        got = {tuple(st[2][3]) + (0,) * (3 - len(st[2][3])): st[3] for st in body}
        offs = [tuple(o) for o in A.offsets]
        if set(got) != set(offs) or len(got) != len(body) or any(st[1] != "=" for st in body):
            raise Exa4Unsupported("stencil field initialisation: one assignment per declared entry")
        try:
            if offs != want:
                raise Exa4Unsupported("not the 5/7-entry form of examg_init_varcoeff7")
            fn, par = self._varcoeff_function(got, want, lvl)
        except Exa4Unsupported:
            want = offs
            # any other discretisation / coefficient function: every entry is a point expression of its own, filled into
            # its coefficient plane by the expression kernel (one launch per entry)
            size = A.clayout.size
            for k, o in enumerate(want):
                prog, _ = self._analytic(got[o], lvl)
                plane = A.cfield[k * size:(k + 1) * size]
                for b, e in boxes:
                    self.launches += 1
                    if isinstance(prog, int):
                        self.ops.fill_fn(A.clayout.c_struct(), plane, self.domain.geom(lvl), prog, _, b, e)
                    else:
                        self.ops.fill_expr(A.clayout.c_struct(), plane, self.domain.geom(lvl), prog, b, e)
            return
        for b, e in boxes:
            self.launches += 1
            self.ops.init_varcoeff7(A.clayout.c_struct(), A.cfield, self.domain.geom(lvl), fn, par, b, e)

    def _varcoeff_function(self, got, want, lvl: int):
        """Coefficient function id if the entries are -div(a grad) with a built-in `a` at the half points, in the exact
        form of examg_init_varcoeff7."""
        nd = self.nd
        calls = [c for c in _find_calls(got[want[1]]) if c[1] in self.functions]
        if not calls:
            raise Exa4Unsupported("stencil field initialisation without a coefficient function")
        cfn = self.functions[calls[0][1]][0]
        coef_expr = ("call", cfn.name, None, [("id", "vf_nodePosition_" + "xyz"[i], None) for i in range(len(cfn.params))])
        fn, par = self._recognise(coef_expr, lvl)
        h = self.domain.h(lvl)
        for _ in range(6):      # check the seven expressions against the kernel's formula at random points
            x, y, z = (self._rng.uniform(0.1, 0.9) for _ in range(3))
            a = lambda dx, dy, dz: fn_eval(fn, par, x + dx, y + dy, z + dz)
            ref = {}
            diag = None
            for d in range(nd):
                off = [0.0, 0.0, 0.0]
                off[d] = 0.5 * h[d]
                ap, am = a(*off), a(*[-v for v in off])
                term = (ap + am) / (h[d] * h[d])
                diag = term if diag is None else diag + term
                ref[want[1 + 2 * d]] = (-1.0 * ap) / (h[d] * h[d])
                ref[want[2 + 2 * d]] = (-1.0 * am) / (h[d] * h[d])
            ref[want[0]] = diag
            for o in want:
                v = self._point_eval(got[o], lvl, x, y, z)
                if abs(v - ref[o]) > 1e-11 * max(1.0, abs(ref[o])):
                    raise Exa4Unsupported("stencil field entry %r is not -a(x +- h/2)/h^2" % (o,))
        return fn, par


# =====================================================================================================================
def load(exa4_path: str, knowledge_path: Optional[str] = None, **kw) -> Exa4Program:
    with open(exa4_path) as f:
        text = f.read()
    k = _knowledge.parse_file(knowledge_path) if knowledge_path else {}
    return Exa4Program(text, k, **kw)


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description="run an ExaSlang-4 multigrid program on libexamg (MI355X)")
    ap.add_argument("exa4")
    ap.add_argument("knowledge", nargs="?")
    ap.add_argument("--set", action="append", default=[], metavar="key=value", help="override a knowledge flag")
    args = ap.parse_args(argv)
    k = _knowledge.parse_file(args.knowledge) if args.knowledge else {}
    for kv in args.set:
        _knowledge.parse_text(kv, None, k)
    with open(args.exa4) as f:
        prog = Exa4Program(f.read(), k, echo=True)
    prog.json_dir = os.getcwd()
    prog.run()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
