"""Kernel-call layer: one method per emitted-loop kind, forwarding to the C ABI of libexamg.so.

PyTorch is plumbing here: device memory (float64 tensors), the current HIP stream (so launches can be
captured by torch.cuda.graph and timed by events on that stream) and torch.distributed.  All
arithmetic happens in the HIP kernels; there is no CPU fallback -- constructing HipOps without the
built library or without a GPU raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

from . import lib as _lib
from .field import Colouring, MacSystem, MatrixStencil, Stencil, fn_expr  # noqa: F401  (Colouring: the value type of the coloured entry points)
from .lib import NL_ADD, NL_APPLY, NL_RESIDUAL, ExamgError, check, ivec  # noqa: F401  (NL_*: the modes of nl_op)


class HipOps:
    name = "hip"

    def __init__(self, device: Optional[int] = None, lib_path: Optional[str] = None):
        import torch

        self.torch = torch
        self.L = _lib.load(lib_path)   # raises if libexamg.so is missing
        if not torch.cuda.is_available():
            raise ExamgError("HipOps needs a GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        if self.L.examg_device_count() < 1:
            raise ExamgError("libexamg sees no HIP device")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self._work = torch.empty(int(self.L.examg_reduce_work_bytes()) // 8, dtype=torch.float64, device=self.device)

    # -- plumbing ------------------------------------------------------------------------------
    def new_array(self, n: int):
        return self.torch.zeros(int(n), dtype=self.torch.float64, device=self.device)

    def new_scalar(self):
        return self.torch.zeros(1, dtype=self.torch.float64, device=self.device)

    @staticmethod
    def ptr(t) -> int:
        return t.data_ptr()

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def synchronize(self):
        self.torch.cuda.synchronize(self.device)

    def side_stream(self):
        """A second HIP stream for halo traffic that overlaps the interior kernels."""
        if getattr(self, "_side", None) is None:
            # high priority: short shell kernels beside a pass that fills the chip (csrc/examg_comm.hip: overlap_of)
            import os

            self._side = self.torch.cuda.Stream(self.device, priority=0 if os.environ.get("EXAMG_SIDE_PRIORITY") == "0" else -1)
        return self._side

    # -- recording launches into a hipGraph (what Exa4Program's auto_graph needs of a kernel layer) ------------------------------
    def graph_begin(self):
        """From here on the launches of this thread are recorded, not executed (torch.cuda.graph); returns the recording."""
        g = self.torch.cuda.CUDAGraph()
        ctx = self.torch.cuda.graph(g, capture_error_mode="thread_local")
        ctx.__enter__()
        return g, ctx

    def graph_end(self, rec):
        rec[1].__exit__(None, None, None)

    def graph_replay(self, rec):
        rec[0].replay()

    def graph_capturing(self) -> bool:
        return self.torch.cuda.is_current_stream_capturing()

    def to_host(self, t):
        return t.detach().cpu().numpy()

    def from_host(self, a):
        return self.torch.from_numpy(a).to(self.device)

    # -- stencil loops ----------------------------------------------------------------------------
    def stencil_op(self, mode: int, lu, u, lf, rhs, ld, dst, st: Stencil, w: float, colour: int, begin, end):
        sc = st.c_struct(self.ptr)
        check(self.L.examg_stencil_op(mode, C.byref(lu), self.ptr(u), C.byref(lf) if lf is not None else None,
                                      self.ptr(rhs) if rhs is not None else None, C.byref(ld), self.ptr(dst),
                                      C.byref(sc), float(w), int(colour), ivec(begin), ivec(end), self._stream()),
              "examg_stencil_op")

    def stencil_op_coloured(self, mode: int, lu, u, lf, rhs, ld, dst, st: Stencil, w: float, col: Colouring, begin, end):
        """A stencil loop on the points of one colour of a multi-colouring (examg_stencil_op_coloured)."""
        sc, cc = st.c_struct(self.ptr), col.c_struct()
        check(self.L.examg_stencil_op_coloured(mode, C.byref(lu), self.ptr(u), C.byref(lf) if lf is not None else None,
                                               self.ptr(rhs) if rhs is not None else None, C.byref(ld), self.ptr(dst), C.byref(sc), float(w),
                                               C.byref(cc), ivec(begin), ivec(end), self._stream()), "examg_stencil_op_coloured")

    def mcgs_sweep(self, lu, u, lf, rhs, st: Stencil, w: float, col: Colouring, begin, end):
        """All colour loops of an in-place smoother on a block without neighbours, in the reference's order (examg_mcgs_sweep)."""
        sc, cc = st.c_struct(self.ptr), col.c_struct()
        check(self.L.examg_mcgs_sweep(C.byref(lu), self.ptr(u), C.byref(lf), self.ptr(rhs), C.byref(sc), float(w), C.byref(cc), ivec(begin),
                                      ivec(end), self._stream()), "examg_mcgs_sweep")

    def mcgs_one_pass_eligible(self, lu, lf, st: Stencil, col: Colouring, begin, end) -> bool:
        """Will mcgs_sweep run its row-pair kernel (True) or the colour loops one by one?"""
        sc, cc = st.c_struct(self.ptr), col.c_struct()
        return bool(self.L.examg_mcgs_one_pass_eligible(C.byref(lu), C.byref(lf), C.byref(sc), C.byref(cc), ivec(begin), ivec(end)))

    def gs_sweep(self, lu, u, lf, rhs, st: Stencil, w: float, begin, end):
        """One lexicographic Gauss-Seidel sweep in place on u: the sequential nest of the loop, x fastest, bit for bit (examg_gs_sweep)."""
        sc = st.c_struct(self.ptr)
        check(self.L.examg_gs_sweep(C.byref(lu), self.ptr(u), C.byref(lf), self.ptr(rhs), C.byref(sc), float(w), ivec(begin), ivec(end),
                                    self._stream()), "examg_gs_sweep")

    def gs_route(self, lu, lf, st: Stencil, begin, end) -> int:
        """What gs_sweep does with these arguments: lib.GS_REFUSED (the reason in examg_last_error), GS_EMPTY, GS_ONE_WORKGROUP, GS_TILED, GS_PER_HYPERPLANE."""
        sc = st.c_struct(self.ptr)
        return int(self.L.examg_gs_route(C.byref(lu), C.byref(lf), C.byref(sc), ivec(begin), ivec(end)))

    # -- table-coefficient stencils (axis-aligned non-uniform grids) ---------------------------------------------------------------
    def axis_op(self, mode: int, lu, u, lf, rhs, ld, dst, st, w: float, colour: int, begin, end, route: Optional[int] = None):
        """A stencil loop whose coefficients come from per-axis tables (examg_axis_op); st: grid.AxisStencil.  route: lib.AXIS_GENERIC /
        lib.AXIS_STAR by name, None: the star kernel wherever the stencil's shape admits it (tools/axis_bench.py: within 2 % of the
        generic one at 256^3, 1 to 5 % faster at 512^3)."""
        sc = st.c_struct(self)
        sc.route = _lib.AXIS_AUTO if route is None else int(route)
        check(self.L.examg_axis_op(mode, C.byref(lu), self.ptr(u), C.byref(lf) if lf is not None else None,
                                   self.ptr(rhs) if rhs is not None else None, C.byref(ld), self.ptr(dst), C.byref(sc), float(w), int(colour),
                                   ivec(begin), ivec(end), self._stream()), "examg_axis_op")

    def axis_route(self, mode: int, lu, lf, ld, st, colour: int, begin, end, route: Optional[int] = None) -> int:
        """What axis_op does with these arguments: -1 refused (the reason in examg_last_error), 0 empty box, lib.AXIS_GENERIC, lib.AXIS_STAR."""
        sc = st.c_struct(self)
        sc.route = _lib.AXIS_AUTO if route is None else int(route)
        return int(self.L.examg_axis_route(mode, C.byref(lu), C.byref(lf) if lf is not None else None, C.byref(ld), C.byref(sc), int(colour),
                                           ivec(begin), ivec(end)))

    def rbgs_sweep_fused(self, lu, u_in, u_out, lf, rhs, st: Stencil, w: float, first: int, begin, end):
        sc = st.c_struct(self.ptr)
        check(self.L.examg_rbgs_sweep_fused(C.byref(lu), self.ptr(u_in), self.ptr(u_out), C.byref(lf), self.ptr(rhs),
                                            C.byref(sc), float(w), int(first), ivec(begin), ivec(end), self._stream()),
              "examg_rbgs_sweep_fused")

    def rbgs_sweep_fused_boxes(self, lu, u_in, u_out, tmp, lf, rhs, st: Stencil, w: float, first: int, begin1, end1, begin2, end2):
        sc = st.c_struct(self.ptr)
        check(self.L.examg_rbgs_sweep_fused_boxes(C.byref(lu), self.ptr(u_in), self.ptr(u_out), self.ptr(tmp) if tmp is not None else None,
                                                  C.byref(lf), self.ptr(rhs), C.byref(sc), float(w), int(first), ivec(begin1), ivec(end1),
                                                  ivec(begin2), ivec(end2), self._stream()), "examg_rbgs_sweep_fused_boxes")

    def jacobi2(self, lu, u_in, u_out, tmp, lf, rhs, st: Stencil, w: float, begin, end):
        sc = st.c_struct(self.ptr)
        check(self.L.examg_jacobi2(C.byref(lu), self.ptr(u_in), self.ptr(u_out), self.ptr(tmp) if tmp is not None else None,
                                   C.byref(lf), self.ptr(rhs), C.byref(sc), float(w), ivec(begin), ivec(end), self._stream()),
              "examg_jacobi2")

    def jacobi3(self, lu, u_in, u_out, tmp, lf, rhs, st: Stencil, w: float, begin, end):
        """Three Jacobi steps in one pass where the kernel applies (examg_jacobi3)."""
        sc = st.c_struct(self.ptr)
        check(self.L.examg_jacobi3(C.byref(lu), self.ptr(u_in), self.ptr(u_out), self.ptr(tmp) if tmp is not None else None,
                                   C.byref(lf), self.ptr(rhs), C.byref(sc), float(w), ivec(begin), ivec(end), self._stream()),
              "examg_jacobi3")

    def rbgs_colours3(self, lu, u_in, u_out, lf, rhs, st: Stencil, w: float, first: int, begin, end):
        """Three colour loops (first, other, first) in one pass where the kernel applies (examg_rbgs_colours3)."""
        sc = st.c_struct(self.ptr)
        check(self.L.examg_rbgs_colours3(C.byref(lu), self.ptr(u_in), self.ptr(u_out), C.byref(lf), self.ptr(rhs), C.byref(sc), float(w), int(first),
                                         ivec(begin), ivec(end), self._stream()), "examg_rbgs_colours3")

    def three_stage_eligible(self, lu, lf, st: Stencil, begin, end) -> bool:
        sc = st.c_struct(self.ptr)
        return bool(self.L.examg_three_stage_eligible(C.byref(lu), C.byref(lf), C.byref(sc), ivec(begin), ivec(end)))

    def pow2_fma_eligible(self, st: Stencil) -> bool:
        """Are the six off-centre coefficients +-2^e, e >= 0, so that the three-step Jacobi pass fuses their products into the sums?"""
        sc = st.c_struct(self.ptr)
        return bool(self.L.examg_pow2_fma_eligible(C.byref(sc)))

    def jacobi_residual(self, lu, u_in, u_out, lf, rhs, lr, res, st: Stencil, w: float, begin, end):
        """One Jacobi step and the residual of its result in one pass (examg_jacobi_residual)."""
        sc = st.c_struct(self.ptr)
        check(self.L.examg_jacobi_residual(C.byref(lu), self.ptr(u_in), self.ptr(u_out), C.byref(lf), self.ptr(rhs), C.byref(lr), self.ptr(res),
                                           C.byref(sc), float(w), ivec(begin), ivec(end), self._stream()), "examg_jacobi_residual")

    def jacobi2_boxes(self, lu, u_in, u_out, tmp, lf, rhs, st: Stencil, w: float, begin1, end1, begin2, end2):
        sc = st.c_struct(self.ptr)
        check(self.L.examg_jacobi2_boxes(C.byref(lu), self.ptr(u_in), self.ptr(u_out), self.ptr(tmp) if tmp is not None else None,
                                         C.byref(lf), self.ptr(rhs), C.byref(sc), float(w), ivec(begin1), ivec(end1),
                                         ivec(begin2), ivec(end2), self._stream()), "examg_jacobi2_boxes")

    def rbgs_sweep_fused_prolong(self, lu, u_in, u_out, lf, rhs, st: Stencil, w: float, first: int, begin, end, lc, uc):
        sc = st.c_struct(self.ptr)
        check(self.L.examg_rbgs_sweep_fused_prolong(C.byref(lu), self.ptr(u_in), self.ptr(u_out), C.byref(lf), self.ptr(rhs), C.byref(sc),
                                                    float(w), int(first), ivec(begin), ivec(end), C.byref(lc), self.ptr(uc), self._stream()),
              "examg_rbgs_sweep_fused_prolong")

    def rbgs_sweep_fused_zero(self, lu, u_out, lf, rhs, st: Stencil, w: float, first: int, begin, end):
        sc = st.c_struct(self.ptr)
        check(self.L.examg_rbgs_sweep_fused_zero(C.byref(lu), self.ptr(u_out), C.byref(lf), self.ptr(rhs), C.byref(sc), float(w),
                                                 int(first), ivec(begin), ivec(end), self._stream()), "examg_rbgs_sweep_fused_zero")

    def jacobi2_prolong(self, lu, u_in, u_out, tmp, lf, rhs, st: Stencil, w: float, begin, end, lc, uc):
        sc = st.c_struct(self.ptr)
        check(self.L.examg_jacobi2_prolong(C.byref(lu), self.ptr(u_in), self.ptr(u_out), self.ptr(tmp) if tmp is not None else None,
                                           C.byref(lf), self.ptr(rhs), C.byref(sc), float(w), ivec(begin), ivec(end), C.byref(lc),
                                           self.ptr(uc), self._stream()), "examg_jacobi2_prolong")

    def two_stage_eligible(self, lu, lf, st: Stencil, begin1, end1, begin2, end2) -> bool:
        """Will jacobi2_boxes / rbgs_sweep_fused_boxes run their one-pass kernel (True) or the fallback that writes `tmp`?"""
        sc = st.c_struct(self.ptr)
        return bool(self.L.examg_two_stage_eligible(C.byref(lu), C.byref(lf), C.byref(sc), ivec(begin1), ivec(end1), ivec(begin2), ivec(end2)))

    def residual_restrict_one_pass(self, lu, lf, st: Stencil, lc, fbegin, fend, cbegin, cend) -> bool:
        """Will residual_restrict run its one-pass kernel for these boxes (True) or residual + restriction through the residual array?"""
        sc = st.c_struct(self.ptr)
        return bool(self.L.examg_residual_restrict_one_pass(C.byref(lu), C.byref(lf), C.byref(sc), C.byref(lc), ivec(fbegin), ivec(fend), ivec(cbegin),
                                                            ivec(cend)))

    # -- inter-grid -------------------------------------------------------------------------------
    def restrict(self, lfine, rf, lc, fc, scale: float, begin, end):
        check(self.L.examg_restrict(C.byref(lfine), self.ptr(rf), C.byref(lc), self.ptr(fc), float(scale), ivec(begin),
                                    ivec(end), self._stream()), "examg_restrict")

    def residual_restrict(self, lu, u, lf, rhs, lr, res, st: Stencil, lc, fc, scale: float, fbegin, fend, cbegin, cend):
        sc = st.c_struct(self.ptr)
        check(self.L.examg_residual_restrict(C.byref(lu), self.ptr(u), C.byref(lf), self.ptr(rhs), C.byref(lr) if lr is not None else None,
                                             self.ptr(res) if res is not None else None, C.byref(sc), C.byref(lc), self.ptr(fc), float(scale),
                                             ivec(fbegin), ivec(fend), ivec(cbegin), ivec(cend), self._stream()), "examg_residual_restrict")

    def prolong_add(self, lc, uc, lfine, uf, begin, end):
        check(self.L.examg_prolong_add(C.byref(lc), self.ptr(uc), C.byref(lfine), self.ptr(uf), ivec(begin), ivec(end),
                                       self._stream()), "examg_prolong_add")

    # -- BLAS-1 -----------------------------------------------------------------------------------
    def set(self, l, x, v: float, begin, end):
        check(self.L.examg_set(C.byref(l), self.ptr(x), float(v), ivec(begin), ivec(end), self._stream()), "examg_set")

    def axpby(self, lx, x, ly, y, a: float, b: float, begin, end):
        check(self.L.examg_axpby(C.byref(lx), self.ptr(x), C.byref(ly), self.ptr(y), float(a), float(b), ivec(begin),
                                 ivec(end), self._stream()), "examg_axpby")

    def axpby_dev(self, lx, x, ly, y, a: float, b: float, which: int, sign: float, num, den, begin, end):
        check(self.L.examg_axpby_dev(C.byref(lx), self.ptr(x), C.byref(ly), self.ptr(y), float(a), float(b), int(which),
                                     float(sign), self.ptr(num), self.ptr(den), ivec(begin), ivec(end), self._stream()),
              "examg_axpby_dev")

    # -- reductions (result stays on the device) ---------------------------------------------------
    def dot(self, lx, x, ly, y, begin, end, out=None):
        out = self.new_scalar() if out is None else out
        check(self.L.examg_dot(C.byref(lx), self.ptr(x), C.byref(ly), self.ptr(y), ivec(begin), ivec(end), self.ptr(out),
                               self.ptr(self._work), self._stream()), "examg_dot")
        return out

    def residual_norm2(self, lu, u, lf, rhs, st: Stencil, begin, end, lr=None, res=None, out=None):
        """sum over the box of (rhs - A u)^2 on the device, the residual not stored (examg_residual_norm2)"""
        out = self.new_scalar() if out is None else out
        sc = st.c_struct(self.ptr)
        check(self.L.examg_residual_norm2(C.byref(lu), self.ptr(u), C.byref(lf), self.ptr(rhs), C.byref(sc), ivec(begin), ivec(end),
                                          C.byref(lr) if lr is not None else None, self.ptr(res) if res is not None else None,
                                          self.ptr(out), self.ptr(self._work), self._stream()), "examg_residual_norm2")
        return out

    def max_err_fn(self, l, x, geom, fn: int, params: Sequence[float], begin, end, out=None):
        out = self.new_scalar() if out is None else out
        return self.max_err_expr(l, x, geom, fn_expr(fn, params), begin, end, out)

    def max_err_expr(self, l, x, geom, expr, begin, end, out=None):
        out = self.new_scalar() if out is None else out
        check(self.L.examg_max_err_expr(C.byref(l), self.ptr(x), C.byref(geom), C.byref(expr), ivec(begin), ivec(end), self.ptr(out),
                                        self.ptr(self._work), self._stream()), "examg_max_err_expr")
        return out

    def fill_expr(self, l, x, geom, expr, begin, end):
        check(self.L.examg_fill_expr(C.byref(l), self.ptr(x), C.byref(geom), C.byref(expr), ivec(begin), ivec(end), self._stream()),
              "examg_fill_expr")

    def apply_dirichlet_expr(self, l, x, geom, expr, face_mask: int):
        check(self.L.examg_apply_dirichlet_expr(C.byref(l), self.ptr(x), C.byref(geom), C.byref(expr), int(face_mask), self._stream()),
              "examg_apply_dirichlet_expr")

    # -- the same over the node tables of a non-uniform grid (grid: lib.GridC, AxisGrid.device) ------------------------------------
    def fill_expr_grid(self, l, x, grid, expr, begin, end):
        check(self.L.examg_fill_expr_grid(C.byref(l), self.ptr(x), C.byref(grid), C.byref(expr), ivec(begin), ivec(end), self._stream()),
              "examg_fill_expr_grid")

    def apply_dirichlet_expr_grid(self, l, x, grid, expr, face_mask: int):
        check(self.L.examg_apply_dirichlet_expr_grid(C.byref(l), self.ptr(x), C.byref(grid), C.byref(expr), int(face_mask), self._stream()),
              "examg_apply_dirichlet_expr_grid")

    def max_err_expr_grid(self, l, x, grid, expr, begin, end, out=None):
        out = self.new_scalar() if out is None else out
        check(self.L.examg_max_err_expr_grid(C.byref(l), self.ptr(x), C.byref(grid), C.byref(expr), ivec(begin), ivec(end), self.ptr(out),
                                             self.ptr(self._work), self._stream()), "examg_max_err_expr_grid")
        return out

    def sum(self, l, x, begin, end, out=None):
        """sum of x over the box on the device (examg_sum: examg_dot's reduction tree)"""
        out = self.new_scalar() if out is None else out
        check(self.L.examg_sum(C.byref(l), self.ptr(x), ivec(begin), ivec(end), self.ptr(out), self.ptr(self._work), self._stream()), "examg_sum")
        return out

    def add_scalar(self, l, x, c: float, begin, end):
        check(self.L.examg_add_scalar(C.byref(l), self.ptr(x), float(c), ivec(begin), ivec(end), self._stream()), "examg_add_scalar")

    # -- cell-centred fields ------------------------------------------------------------------------
    def fill_expr_cell(self, l, x, geom, expr, begin, end):
        check(self.L.examg_fill_expr_cell(C.byref(l), self.ptr(x), C.byref(geom), C.byref(expr), ivec(begin), ivec(end), self._stream()),
              "examg_fill_expr_cell")

    def max_err_expr_cell(self, l, x, geom, expr, begin, end, out=None):
        out = self.new_scalar() if out is None else out
        check(self.L.examg_max_err_expr_cell(C.byref(l), self.ptr(x), C.byref(geom), C.byref(expr), ivec(begin), ivec(end), self.ptr(out),
                                             self.ptr(self._work), self._stream()), "examg_max_err_expr_cell")
        return out

    def apply_bc_cell(self, l, x, geom, kind: int, expr, face_mask: int):
        """kind: lib.BC_DIRICHLET (expr: the boundary value at the face centres), lib.BC_NEUMANN (ghost = interior), lib.BC_NEGATE
        (ghost = -interior: a reflecting wall) or lib.BC_VALUE_MINUS (ghost = expr(ghost cell) - interior); expr may be None for the
        two kinds without a value."""
        check(self.L.examg_apply_bc_cell(C.byref(l), self.ptr(x), C.byref(geom), int(kind), C.byref(expr) if expr is not None else None,
                                         int(face_mask), self._stream()), "examg_apply_bc_cell")

    def apply_bc_cell_faces(self, l, x, geom, faces, face_mask: int):
        """Every face of the mask in one launch (examg_apply_bc_cell_faces).  faces[2 * d + side]: (kind, expr) of the face, None
        for a face outside the mask; kind lib.BC_* -- lib.BC_VALUE_MINUS: ghost = expr(ghost cell) - interior."""
        from .lib import BcFaceC, ExprC

        tab = (BcFaceC * 6)()
        for f in range(6):
            kind, expr = faces[f] if f < len(faces) and faces[f] is not None else (0, None)
            tab[f].kind = int(kind)
            tab[f].expr = C.pointer(expr) if expr is not None else C.POINTER(ExprC)()
        check(self.L.examg_apply_bc_cell_faces(C.byref(l), self.ptr(x), C.byref(geom), tab, int(face_mask), self._stream()),
              "examg_apply_bc_cell_faces")

    def restrict_cell(self, lfine, rf, lc, fc, scale: float, begin, end):
        check(self.L.examg_restrict_cell(C.byref(lfine), self.ptr(rf), C.byref(lc), self.ptr(fc), float(scale), ivec(begin), ivec(end),
                                         self._stream()), "examg_restrict_cell")

    def prolong_add_cell(self, lc, uc, lfine, uf, begin, end):
        check(self.L.examg_prolong_add_cell(C.byref(lc), self.ptr(uc), C.byref(lfine), self.ptr(uf), ivec(begin), ivec(end), self._stream()),
              "examg_prolong_add_cell")

    # -- coupled systems of cell fields -------------------------------------------------------------
    def _sys(self, lu, u, lf, f, lg, g, ld=None, dst=None):
        """examg_sys_t of the unknowns u (layout lu), right-hand sides f (lf; None where not read), the n x n coefficient table g (lg; rows
        of n, None: no term) and the destinations dst (ld)."""
        n = len(u)
        y = _lib.SysC()
        y.n = n
        for name, l in (("lu", lu), ("lf", lf), ("lg", lg), ("ld", ld if ld is not None else lu)):
            C.memmove(C.byref(getattr(y, name)), C.byref(l), C.sizeof(_lib.LayoutC))
        m = min(n, _lib.SYS_MAX)       # an n the library refuses still reaches it
        for c in range(m):
            y.u[c] = self.ptr(u[c])
            y.f[c] = self.ptr(f[c]) if f is not None and f[c] is not None else None
            y.dst[c] = self.ptr(dst[c]) if dst is not None and dst[c] is not None else None
            for d in range(m):
                y.g[c * m + d] = self.ptr(g[c][d]) if g[c][d] is not None else None
        return y

    def sys_op(self, mode: int, lu, u, lf, f, lg, g, ld, dst, L: Stencil, row_mask: int, begin, end):
        """dst_c = A u (lib.SYS_APPLY) or f_c - A u (lib.SYS_RESIDUAL) for the rows of row_mask, A = L * I + g (examg_sys_op)."""
        y, sc = self._sys(lu, u, lf, f, lg, g, ld, dst), L.c_struct(self.ptr)
        check(self.L.examg_sys_op(int(mode), C.byref(y), C.byref(sc), int(row_mask), ivec(begin), ivec(end), self._stream()), "examg_sys_op")

    def sys_relax(self, lu, u, lf, f, lg, g, L: Stencil, relax: float, colour: int, begin, end):
        """The local solves of one colour of the red-black smoother of A = L * I + g, in place on u (examg_sys_relax)."""
        y, sc = self._sys(lu, u, lf, f, lg, g), L.c_struct(self.ptr)
        check(self.L.examg_sys_relax(C.byref(y), C.byref(sc), float(relax), int(colour), ivec(begin), ivec(end), self._stream()), "examg_sys_relax")

    def pointwise_mul(self, lx, x, ly, y, ld, dst, s: float, begin, end):
        """dst = (s * x) * y, s = +-1.0 (examg_pointwise_mul)."""
        check(self.L.examg_pointwise_mul(C.byref(lx), self.ptr(x), C.byref(ly), self.ptr(y), C.byref(ld), self.ptr(dst), float(s), ivec(begin),
                                         ivec(end), self._stream()), "examg_pointwise_mul")

    # -- vector-valued cell fields: a vector argument is (layout, array of n * size doubles), the component slowest ---------------
    def vec_op(self, mode: int, n: int, lu, u, lf, f, ld, dst, M: MatrixStencil, begin, end):
        """dst = M * u (lib.SYS_APPLY) or f - M * u (lib.SYS_RESIDUAL), every row of the matrix stencil M in one launch (examg_vec_op)."""
        mc = M.c_struct(self.ptr, lu)
        check(self.L.examg_vec_op(int(mode), int(n), C.byref(lu), self.ptr(u), C.byref(lf) if lf is not None else None,
                                  self.ptr(f) if f is not None else None, C.byref(ld), self.ptr(dst), C.byref(mc), ivec(begin), ivec(end),
                                  self._stream()), "examg_vec_op")

    def vec_smooth(self, n: int, lu, u, lf, f, M: MatrixStencil, relax: float, colour: int, begin, end):
        """One colour of u = u + relax * (inverse(diag(M)) * (f - M * u)), in place (examg_vec_smooth)."""
        mc = M.c_struct(self.ptr, lu)
        check(self.L.examg_vec_smooth(int(n), C.byref(lu), self.ptr(u), C.byref(lf), self.ptr(f), C.byref(mc), float(relax), int(colour),
                                      ivec(begin), ivec(end), self._stream()), "examg_vec_smooth")

    def vec_dot(self, n: int, lx, x, ly, y, begin, end, out=None):
        """sum over the box of dot(x, y) of the cell, on the device (examg_vec_dot)."""
        out = self.new_scalar() if out is None else out
        check(self.L.examg_vec_dot(int(n), C.byref(lx), self.ptr(x), C.byref(ly), self.ptr(y), ivec(begin), ivec(end), self.ptr(out),
                                   self.ptr(self._work), self._stream()), "examg_vec_dot")
        return out

    def vec_set(self, n: int, l, x, v: float, begin, end):
        check(self.L.examg_vec_set(int(n), C.byref(l), self.ptr(x), float(v), ivec(begin), ivec(end), self._stream()), "examg_vec_set")

    def vec_axpby(self, n: int, lx, x, ly, y, a: float, b: float, begin, end):
        check(self.L.examg_vec_axpby(int(n), C.byref(lx), self.ptr(x), C.byref(ly), self.ptr(y), float(a), float(b), ivec(begin), ivec(end),
                                     self._stream()), "examg_vec_axpby")

    def vec_restrict_cell(self, n: int, lfine, rf, lc, fc, scale: float, begin, end):
        check(self.L.examg_vec_restrict_cell(int(n), C.byref(lfine), self.ptr(rf), C.byref(lc), self.ptr(fc), float(scale), ivec(begin),
                                             ivec(end), self._stream()), "examg_vec_restrict_cell")

    def vec_prolong_add_cell(self, n: int, lc, uc, lfine, uf, begin, end):
        check(self.L.examg_vec_prolong_add_cell(int(n), C.byref(lc), self.ptr(uc), C.byref(lfine), self.ptr(uf), ivec(begin), ivec(end),
                                                self._stream()), "examg_vec_prolong_add_cell")

    def vec_apply_bc_cell(self, n: int, l, x, geom, kind: int, face_mask: int):
        """ghost = interior on every face of the mask and every component, one launch (examg_vec_apply_bc_cell; lib.BC_NEUMANN only)."""
        check(self.L.examg_vec_apply_bc_cell(int(n), C.byref(l), self.ptr(x), C.byref(geom), int(kind), int(face_mask), self._stream()),
              "examg_vec_apply_bc_cell")

    # -- coupled systems of node fields whose blocks are stencils --------------------------------------
    def _bsys(self, lu, u, lf, f, A, ld=None, dst=None):
        """examg_bsys_t of the unknowns u (layout lu), right-hand sides f (lf; None where not read), the n x n table A of constant
        stencils (rows of n, None: no block; a block need not have a centre entry) and the destinations dst (ld).  The stencil
        structs live as long as the returned struct (`keep`)."""
        n = len(u)
        y = _lib.BsysC()
        y.n = n
        for name, l in (("lu", lu), ("lf", lf if lf is not None else lu), ("ld", ld if ld is not None else lu)):
            C.memmove(C.byref(getattr(y, name)), C.byref(l), C.sizeof(_lib.LayoutC))
        m = min(n, _lib.BSYS_MAX)       # an n the library refuses still reaches it
        y.keep = []
        for c in range(m):
            y.u[c] = self.ptr(u[c])
            y.f[c] = self.ptr(f[c]) if f is not None and f[c] is not None else None
            y.dst[c] = self.ptr(dst[c]) if dst is not None and dst[c] is not None else None
            for d in range(m):
                st = A[c][d]
                if st is None:
                    continue
                sc = _lib.StencilC()
                sc.nent = len(st.offsets)
                sc.diag = st.offsets.index((0, 0, 0)) if (0, 0, 0) in st.offsets else 0      # (not looked at)
                for k, o in enumerate(st.offsets[:_lib.MAXE]):
                    for t in range(3):
                        sc.off[k][t] = o[t]
                    sc.coef[k] = st.coefs[k] if st.coefs else 0.0
                if st.cfield is not None:
                    sc.cfield = self.ptr(st.cfield)
                    sc.clayout = st.clayout.c_struct()
                y.keep.append(sc)
                y.A[c * m + d] = C.pointer(sc)
        return y

    def bsys_op(self, mode: int, lu, u, lf, f, ld, dst, A, row_mask: int, begin, end):
        """dst_c = sum_d A[c][d] * u_d (lib.SYS_APPLY) or f_c minus it (lib.SYS_RESIDUAL) for the rows of row_mask (examg_bsys_op)."""
        y = self._bsys(lu, u, lf, f, A, ld, dst)
        check(self.L.examg_bsys_op(int(mode), C.byref(y), int(row_mask), ivec(begin), ivec(end), self._stream()), "examg_bsys_op")

    def bsys_relax(self, lu, u, lf, f, A, relax: float, col: Colouring, begin, end):
        """The local solves of one colour of the collective point smoother of the block system A, in place on u (examg_bsys_relax)."""
        y, cc = self._bsys(lu, u, lf, f, A), col.c_struct()
        check(self.L.examg_bsys_relax(C.byref(y), float(relax), C.byref(cc), ivec(begin), ivec(end), self._stream()), "examg_bsys_relax")

    def bsys_route(self, mode: int, lu, u, lf, f, ld, dst, A, row_mask: int, begin, end) -> int:
        """What bsys_op does with these arguments: -1 refused (the reason in examg_last_error), 0 empty box, lib.BSYS_GATHER."""
        y = self._bsys(lu, u, lf, f, A, ld, dst)
        return int(self.L.examg_bsys_route(int(mode), C.byref(y), int(row_mask), ivec(begin), ivec(end)))

    # -- staggered grids: face fields, the three-field operator and the box smoother ---------------------------
    def _mac(self, sys: MacSystem, who: str):
        """examg_mac_t of a MacSystem; the stencil structs live as long as the returned struct (`keep`)."""
        sys.check_elements(who)
        y = _lib.MacC()
        y.nd = sys.nd
        m = min(max(sys.nd, 0), 3)      # an nd the library refuses still reaches it
        y.keep = []

        def put(dst, l):
            if l is not None:
                cs = l.c_struct()
                C.memmove(C.byref(dst), C.byref(cs), C.sizeof(_lib.LayoutC))

        put(y.lp, sys.lp)
        put(y.lfp, sys.lfp)
        put(y.ldp, sys.ldp)
        y.p = self.ptr(sys.p) if sys.p is not None else None
        y.fp = self.ptr(sys.fp) if sys.fp is not None else None
        y.dstp = self.ptr(sys.dstp) if sys.dstp is not None else None
        for d in range(min(m, len(sys.u))):
            put(y.lu[d], sys.lu[d])
            y.u[d] = self.ptr(sys.u[d]) if sys.u[d] is not None else None
            if sys.f is not None and sys.f[d] is not None:
                put(y.lf[d], sys.lf[d])
                y.f[d] = self.ptr(sys.f[d])
            if sys.dst is not None and sys.dst[d] is not None:
                put(y.ld[d], sys.ld[d])
                y.dst[d] = self.ptr(sys.dst[d])
            y.bc[d], y.bm[d], y.cc[d], y.cp[d] = float(sys.bc[d]), float(sys.bm[d]), float(sys.cc[d]), float(sys.cp[d])
            st = sys.A[d]
            if st is None:
                continue
            sc = _lib.StencilC()
            sc.nent = len(st.offsets)
            sc.diag = st.offsets.index((0, 0, 0)) if (0, 0, 0) in st.offsets else 0
            for k, o in enumerate(st.offsets[:_lib.MAXE]):
                for t in range(3):
                    sc.off[k][t] = o[t]
                sc.coef[k] = st.coefs[k] if st.coefs else 0.0
            if st.cfield is not None:
                sc.cfield = self.ptr(st.cfield)
                sc.clayout = st.clayout.c_struct()
            y.keep.append(sc)
            y.A[d] = C.pointer(sc)
        return y

    @staticmethod
    def _row_boxes(nd: int, begin, end):
        """One box per row, flattened: begin[r] / end[r] are the (x, y, z) of row r; None for a row outside the mask."""
        n = max(nd, 0) + 1
        b, e = (C.c_int32 * (3 * 4))(), (C.c_int32 * (3 * 4))()
        for r in range(min(n, 4)):
            if r < len(begin) and begin[r] is not None:
                for t in range(3):
                    b[3 * r + t], e[3 * r + t] = int(begin[r][t]), int(end[r][t])
        return b, e

    def mac_op(self, mode: int, sys: MacSystem, row_mask: int, begin, end):
        """dst_r = row r of the staggered operator (lib.SYS_APPLY) or f_r minus it (lib.SYS_RESIDUAL) for the rows of row_mask, each on its
        own box begin[r] .. end[r], in one launch (examg_mac_op)."""
        y = self._mac(sys, "examg_mac_op")
        b, e = self._row_boxes(sys.nd, begin, end)
        check(self.L.examg_mac_op(int(mode), C.byref(y), int(row_mask), b, e, self._stream()), "examg_mac_op")

    def mac_relax(self, sys: MacSystem, relax: float, col: Colouring, begin, end):
        """The box solves of the cells of one colour, in place on u and p (examg_mac_relax)."""
        y, cc = self._mac(sys, "examg_mac_relax"), col.c_struct()
        check(self.L.examg_mac_relax(C.byref(y), float(relax), C.byref(cc), ivec(begin), ivec(end), self._stream()), "examg_mac_relax")

    def mac_sweep(self, sys: MacSystem, relax: float, col: Colouring, begin, end):
        """All colours of the box smoother in the reference's order (examg_mac_sweep)."""
        y, cc = self._mac(sys, "examg_mac_sweep"), col.c_struct()
        check(self.L.examg_mac_sweep(C.byref(y), float(relax), C.byref(cc), ivec(begin), ivec(end), self._stream()), "examg_mac_sweep")

    def restrict_face(self, axis: int, lfine, rf, lc, fc, scale: float, begin, end):
        check(self.L.examg_restrict_face(int(axis), C.byref(lfine), self.ptr(rf), C.byref(lc), self.ptr(fc), float(scale), ivec(begin), ivec(end),
                                         self._stream()), "examg_restrict_face")

    def prolong_add_face(self, axis: int, lc, uc, lfine, uf, begin, end):
        check(self.L.examg_prolong_add_face(int(axis), C.byref(lc), self.ptr(uc), C.byref(lfine), self.ptr(uf), ivec(begin), ivec(end), self._stream()),
              "examg_prolong_add_face")

    def apply_bc_face(self, axis: int, l, x, geom, kind: int, expr, face_mask: int):
        """`apply bc` of a face field: the node rule on the walls normal to `axis`, the cell rule on the others (examg_apply_bc_face)."""
        check(self.L.examg_apply_bc_face(int(axis), C.byref(l), self.ptr(x), C.byref(geom), int(kind), C.byref(expr) if expr is not None else None,
                                         int(face_mask), self._stream()), "examg_apply_bc_face")

    def fill_expr_face(self, axis: int, l, x, geom, expr, begin, end):
        check(self.L.examg_fill_expr_face(int(axis), C.byref(l), self.ptr(x), C.byref(geom), C.byref(expr), ivec(begin), ivec(end), self._stream()),
              "examg_fill_expr_face")

    def max_err_expr_face(self, axis: int, l, x, geom, expr, begin, end, out=None):
        out = self.new_scalar() if out is None else out
        check(self.L.examg_max_err_expr_face(int(axis), C.byref(l), self.ptr(x), C.byref(geom), C.byref(expr), ivec(begin), ivec(end), self.ptr(out),
                                             self.ptr(self._work), self._stream()), "examg_max_err_expr_face")
        return out

    # -- semilinear operators A * u + c(q) . u -------------------------------------------------------
    def nl_op(self, mode: int, lu, u, lq, q, lf, rhs, ld, dst, st: Stencil, c, begin, end):
        """dst = N (lib.NL_APPLY), rhs - N (lib.NL_RESIDUAL) or dst + N (lib.NL_ADD), N = st * u + c(q) . u; c: lib.NlExprC (examg_nl_op)."""
        sc = st.c_struct(self.ptr)
        check(self.L.examg_nl_op(int(mode), C.byref(lu), self.ptr(u), C.byref(lq), self.ptr(q), C.byref(lf) if lf is not None else None,
                                 self.ptr(rhs) if rhs is not None else None, C.byref(ld), self.ptr(dst), C.byref(sc), C.byref(c), ivec(begin),
                                 ivec(end), self._stream()), "examg_nl_op")

    def nl_smooth(self, lu, u_in, ld, u_out, lf, rhs, st: Stencil, c, d, w: float, colour: int, begin, end):
        """u_out = u + w * ((rhs - (st * u + c(u) . u)) / (diag(st) + d(u))): colour -1 out of place, 0 / 1 in place (examg_nl_smooth)."""
        sc = st.c_struct(self.ptr)
        check(self.L.examg_nl_smooth(C.byref(lu), self.ptr(u_in), C.byref(ld), self.ptr(u_out), C.byref(lf), self.ptr(rhs), C.byref(sc),
                                     C.byref(c), C.byref(d), float(w), int(colour), ivec(begin), ivec(end), self._stream()), "examg_nl_smooth")

    # -- explicit flux-form steps on cell fields -------------------------------------------------------
    def flux_step(self, lin, ins, lout, outs, spec, begin, end):
        """One explicit update of the components of `spec` (flux.FluxSpec): outs[c] = C_c * ins[field_c] + sum_t scale_t * (P_t(i + plus_t) -
        P_t(i + minus_t)), one launch for all components (examg_flux_step)."""
        fx = spec.c_struct(self.ptr, lin, ins, lout, outs)
        check(self.L.examg_flux_step(C.byref(fx), ivec(begin), ivec(end), self._stream()), "examg_flux_step")

    def flux_route(self, lin, ins, lout, outs, spec, begin, end) -> int:
        """What flux_step does with these arguments: -1 refused (the reason in examg_last_error), 0 empty box, lib.FLUX_GATHER, lib.FLUX_MARCH."""
        fx = spec.c_struct(self.ptr, lin, ins, lout, outs)
        return int(self.L.examg_flux_route(C.byref(fx), ivec(begin), ivec(end)))

    def reduce_expr_cell(self, op: int, l, xs, prog, begin, end, out=None):
        """max (lib.REDUCE_MAX) or min (lib.REDUCE_MIN) over the box of the program over the cell fields xs at the cell; prog: lib.NlExprC
        over lib.FLUX_OPS (flux.field_program).  The result stays on the device (examg_reduce_expr_cell)."""
        out = self.new_scalar() if out is None else out
        ptrs = (C.c_void_p * len(xs))(*[self.ptr(x) for x in xs])
        check(self.L.examg_reduce_expr_cell(int(op), len(xs), C.byref(l), ptrs, C.byref(prog), ivec(begin), ivec(end), self.ptr(out),
                                            self.ptr(self._work), self._stream()), "examg_reduce_expr_cell")
        return out

    # -- complex-valued node fields: arrays of 2 * size(layout) doubles, (re, im) per point -------------------------------------------
    def new_complex_array(self, npoints: int):
        """A zeroed complex field of npoints points: 2 * npoints doubles, 16-byte aligned (torch allocations are)."""
        return self.new_array(2 * int(npoints))

    def new_complex_scalar(self):
        return self.torch.zeros(2, dtype=self.torch.float64, device=self.device)

    def _cstencil(self, st: Stencil):
        """examg_stencil_t with the real parts of the entries, and the array of their imaginary parts."""
        real = Stencil(st.offsets, [complex(c).real for c in st.coefs], st.cfield, st.clayout, st.ctransform, st.wform)
        im = (C.c_double * _lib.MAXE)(*[complex(c).imag for c in st.coefs])
        return real.c_struct(self.ptr), im

    def _cstencil_args(self, mode, lu, u, lf, rhs, ld, dst, st, w, colour, begin, end):
        sc, im = self._cstencil(st)
        return (int(mode), C.byref(lu), self.ptr(u), C.byref(lf) if lf is not None else None, self.ptr(rhs) if rhs is not None else None,
                C.byref(ld) if ld is not None else None, self.ptr(dst) if dst is not None else None, C.byref(sc), im, _lib.dvec2(w), int(colour),
                ivec(begin), ivec(end))

    def cstencil_op(self, mode: int, lu, u, lf, rhs, ld, dst, st: Stencil, w, colour: int, begin, end):
        """A loop over a constant stencil with complex entries on complex fields: mode 0 / 1 / 2 as stencil_op with a complex w, lib.CRELAX the
        local solve of one colour in place on u (examg_cstencil_op)."""
        check(self.L.examg_cstencil_op(*self._cstencil_args(mode, lu, u, lf, rhs, ld, dst, st, w, colour, begin, end), self._stream()),
              "examg_cstencil_op")

    def cstencil_route(self, mode: int, lu, u, lf, rhs, ld, dst, st: Stencil, w, colour: int, begin, end) -> int:
        """What cstencil_op does with these arguments: -1 refused (the reason in examg_last_error), 0 empty box, lib.CSTENCIL_GATHER,
        lib.CSTENCIL_MARCH."""
        return int(self.L.examg_cstencil_route(*self._cstencil_args(mode, lu, u, lf, rhs, ld, dst, st, w, colour, begin, end)))

    def clincomb(self, form: int, lx, x, ly, y, lz, z, ld, dst, a, b, begin, end):
        """dst = x + a y (lib.C_XPAY), x - a y (lib.C_XMAY) or x + a (y - b z) (lib.C_XPAYMBZ), a and b complex (examg_clincomb)."""
        check(self.L.examg_clincomb(int(form), C.byref(lx), self.ptr(x), C.byref(ly), self.ptr(y), C.byref(lz) if lz is not None else None,
                                    self.ptr(z) if z is not None else None, C.byref(ld), self.ptr(dst), _lib.dvec2(a),
                                    _lib.dvec2(b) if b is not None else None, ivec(begin), ivec(end), self._stream()), "examg_clincomb")

    def cdot(self, lx, x, ly, y, begin, end, out=None):
        """The unconjugated sum of x * y over the box; the two parts stay on the device (examg_cdot)."""
        out = self.new_complex_scalar() if out is None else out
        check(self.L.examg_cdot(C.byref(lx), self.ptr(x), C.byref(ly), self.ptr(y), ivec(begin), ivec(end), self.ptr(out), self.ptr(self._work),
                                self._stream()), "examg_cdot")
        return out

    def complex_value(self, t) -> complex:
        """Host value of a device complex scalar."""
        v = t.tolist()
        return complex(v[0], v[1])

    def crestrict(self, lfine, rf, lc, fc, scale: float, begin, end):
        check(self.L.examg_crestrict(C.byref(lfine), self.ptr(rf), C.byref(lc), self.ptr(fc), float(scale), ivec(begin), ivec(end), self._stream()),
              "examg_crestrict")

    def cprolong_add(self, lc, uc, lfine, uf, begin, end):
        check(self.L.examg_cprolong_add(C.byref(lc), self.ptr(uc), C.byref(lfine), self.ptr(uf), ivec(begin), ivec(end), self._stream()),
              "examg_cprolong_add")

    def cshift_div(self, l, x, off, c, begin, end):
        """x(i) = x(i + off) / c on the box: the absorbing-boundary assignment (examg_cshift_div)."""
        check(self.L.examg_cshift_div(C.byref(l), self.ptr(x), ivec(off), _lib.dvec2(c), ivec(begin), ivec(end), self._stream()), "examg_cshift_div")

    def cfrom_parts(self, l, dst, lre, re, lim, im, begin, end):
        """dst = (re, im) from real fields; a part that is None is 0.0 (examg_cfrom_parts)."""
        check(self.L.examg_cfrom_parts(C.byref(l), self.ptr(dst), C.byref(lre) if lre is not None else None, self.ptr(re) if re is not None else None,
                                       C.byref(lim) if lim is not None else None, self.ptr(im) if im is not None else None, ivec(begin), ivec(end),
                                       self._stream()), "examg_cfrom_parts")

    def scalar_value(self, t) -> float:
        """Host value of a device scalar (the reference's 8-byte D2H copy after a reduction)."""
        return float(t.item())

    # -- boundary / init ----------------------------------------------------------------------------
    def fill_fn(self, l, x, geom, fn: int, params: Sequence[float], begin, end):
        self.fill_expr(l, x, geom, fn_expr(fn, params), begin, end)

    def fill_dup_faces(self, l, x, geom, fn: int, params: Sequence[float], face_mask: int):
        """`loop over F only dup [dir] on boundary { F = fn }` for every physical face of the mask, one launch."""
        check(self.L.examg_fill_dup_faces_expr(C.byref(l), self.ptr(x), C.byref(geom), C.byref(fn_expr(fn, params)), int(face_mask), self._stream()),
              "examg_fill_dup_faces_expr")

    def apply_dirichlet(self, l, x, geom, fn: int, params: Sequence[float], face_mask: int):
        self.apply_dirichlet_expr(l, x, geom, fn_expr(fn, params), face_mask)

    def init_varcoeff7(self, lc, cf, geom, coef_fn: int, params: Sequence[float], begin, end):
        check(self.L.examg_init_varcoeff7(C.byref(lc), self.ptr(cf), C.byref(geom), C.byref(fn_expr(coef_fn, params)),
                                          ivec(begin), ivec(end), self._stream()), "examg_init_varcoeff7")

    def init_helmholtz27(self, lc, cf, geom, coef_fn: int, params: Sequence[float], begin, end):
        prm = list(params) + [0.0, 0.0]
        check(self.L.examg_init_helmholtz27(C.byref(lc), self.ptr(cf), C.byref(geom), C.byref(fn_expr(coef_fn, params)), float(prm[1]),
                                            ivec(begin), ivec(end), self._stream()), "examg_init_helmholtz27")

    def transform_stencilfield(self, lc, nent: int, src, dst, to_entry_fastest: bool):
        """`transform <coefficient field> with [x, y, z, i] => [i, x, y, z]` (or its inverse) applied to the data."""
        check(self.L.examg_transform_stencilfield(C.byref(lc), int(nent), self.ptr(src), self.ptr(dst), 1 if to_entry_fastest else 0,
                                                  self._stream()), "examg_transform_stencilfield")

    def transform_field(self, lsrc, src, ldst, dst):
        """The same field under another layout transformation (`transform <field> with [x, y, z] => [x / 2, y, z, x % 2]` or back)."""
        check(self.L.examg_transform_field(C.byref(lsrc), self.ptr(src), C.byref(ldst), self.ptr(dst), self._stream()), "examg_transform_field")

    # -- halo ------------------------------------------------------------------------------------------
    def pack(self, l, x, buf, begin, end):
        check(self.L.examg_pack(C.byref(l), self.ptr(x), self.ptr(buf), ivec(begin), ivec(end), self._stream()), "examg_pack")

    def unpack(self, l, x, buf, begin, end):
        check(self.L.examg_unpack(C.byref(l), self.ptr(x), self.ptr(buf), ivec(begin), ivec(end), self._stream()),
              "examg_unpack")

    # -- coarse solve ---------------------------------------------------------------------------------
    def cg_coarse(self, lu, sol, lf, rhs, lr, res, lp, p, lq, ap, st: Stencil, geom, face_mask: int, max_it: int,
                  rel_tol: float, begin, end, info, flags: int = 0):
        """flags: CG_ALPHA_FROM_NORM | CG_NO_BC (include/examg.h: the layer-3 generator's form of the solver)."""
        sc = st.c_struct(self.ptr)
        check(self.L.examg_cg_coarse_variant(C.byref(lu), self.ptr(sol), C.byref(lf), self.ptr(rhs), C.byref(lr), self.ptr(res),
                                             C.byref(lp), self.ptr(p), C.byref(lq), self.ptr(ap), C.byref(sc), C.byref(geom),
                                             int(face_mask), int(max_it), float(rel_tol), ivec(begin), ivec(end), int(flags),
                                             self.ptr(info), self._stream()), "examg_cg_coarse_variant")

    def fill_random(self, x, seed: int):
        check(self.L.examg_fill_random(self.ptr(x), int(x.numel()), int(seed), self._stream()), "examg_fill_random")

    # -- external fields -------------------------------------------------------------------------------
    def copy_to_external(self, l_int, x_int, l_ext, dest):
        check(self.L.examg_copy_to_external(C.byref(l_int), self.ptr(x_int), C.byref(l_ext), self.ptr(dest), self._stream()),
              "examg_copy_to_external")

    def copy_from_external(self, l_ext, src, l_int, x_int):
        check(self.L.examg_copy_from_external(C.byref(l_ext), self.ptr(src), C.byref(l_int), self.ptr(x_int), self._stream()),
              "examg_copy_from_external")
