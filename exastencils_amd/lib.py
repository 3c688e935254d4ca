"""ctypes binding of libexamg.so (the C ABI declared in include/examg.h).

The library is built in-tree by `__graft_entry__.build()` (hipcc --offload-arch=gfx950).
No fallback: a missing library raises ImportError-like RuntimeError at load().
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EXAMG_LIB", os.path.join(_HERE, "libexamg.so"))   # EXAMG_LIB: experimental builds (tools/)
MAXE = 27


class LayoutC(C.Structure):
    _fields_ = [("nd", C.c_int32)] + [
        (n, C.c_int32 * 3) for n in ("pad_l", "ghost_l", "dup_l", "inner", "dup_r", "ghost_r", "pad_r")
    ] + [("transform", C.c_int32)]


class StencilC(C.Structure):
    _fields_ = [
        ("nent", C.c_int32),
        ("diag", C.c_int32),
        ("off", (C.c_int32 * 3) * MAXE),
        ("coef", C.c_double * MAXE),
        ("cfield", C.c_void_p),
        ("clayout", LayoutC),
        ("ctransform", C.c_int32),
        ("wform", C.c_int32),
    ]


class GeomC(C.Structure):
    _fields_ = [("pos_begin", C.c_double * 3), ("h", C.c_double * 3)]


class GridC(C.Structure):
    """examg_grid_t: the node tables of an axis-aligned grid on the device; element j of a table is node j - ghost."""
    _fields_ = [("nodes", C.c_void_p * 3), ("n", C.c_int32 * 3), ("ghost", C.c_int32)]


class ColouringC(C.Structure):
    """examg_colouring_t: 1 to 3 colour expressions (shift + sum of the axes' indices) % mod and the remainders of one colour."""
    _fields_ = [("nexpr", C.c_int32)] + [(n, C.c_int32 * 3) for n in ("axes", "shift", "mod", "rem")]


AXIS_MAX_TERMS = 32
AXIS_AUTO, AXIS_GENERIC, AXIS_STAR = 0, 1, 2      # examg_axis_stencil_t.route, and what examg_axis_route answers


class AxisTermC(C.Structure):
    """examg_axis_term_t: X[tab[0]][i0] * ((s * Z[tab[2]][i2]) * Y[tab[1]][i1]); tab[d] = -1: no table of that axis."""
    _fields_ = [("entry", C.c_int32), ("tab", C.c_int32 * 3), ("s", C.c_double)]


class AxisStencilC(C.Structure):
    """examg_axis_stencil_t: a stencil whose coefficients are sums of products of per-axis tables (include/examg.h)."""
    _fields_ = [("nent", C.c_int32), ("diag", C.c_int32), ("off", (C.c_int32 * 3) * MAXE), ("wform", C.c_int32), ("nterm", C.c_int32),
                ("term", AxisTermC * AXIS_MAX_TERMS), ("tables", C.c_void_p * 3), ("ntab", C.c_int32 * 3), ("tab_begin", C.c_int32 * 3),
                ("tab_len", C.c_int32 * 3), ("route", C.c_int32)]


SYS_MAX = 3
SYS_APPLY, SYS_RESIDUAL = 0, 1


class SysC(C.Structure):
    """examg_sys_t: the arrays of a coupled system of n = 2 or 3 cell fields (include/examg.h)."""
    _fields_ = [("n", C.c_int32), ("lu", LayoutC), ("lf", LayoutC), ("lg", LayoutC), ("ld", LayoutC), ("u", C.c_void_p * SYS_MAX),
                ("f", C.c_void_p * SYS_MAX), ("g", C.c_void_p * (SYS_MAX * SYS_MAX)), ("dst", C.c_void_p * SYS_MAX)]


VEC_MAX = 3


class VecEntryC(C.Structure):
    """examg_vec_entry_t: one entry of a matrix stencil -- element (c, d) at index c * n + d: a constant (kmask bit), a cell coefficient
    field (g), both or neither."""
    _fields_ = [("off", C.c_int32 * 3), ("kmask", C.c_uint32), ("k", C.c_double * (VEC_MAX * VEC_MAX)), ("g", C.c_void_p * (VEC_MAX * VEC_MAX))]


class VecStencilC(C.Structure):
    """examg_vec_stencil_t: a matrix stencil on a vector-valued cell field (include/examg.h)."""
    _fields_ = [("nent", C.c_int32), ("lg", LayoutC), ("ent", VecEntryC * 7)]


BSYS_MAX = 3
BSYS_GATHER = 1                           # what examg_bsys_route answers (-1 refused, 0 empty box)


class BsysC(C.Structure):
    """examg_bsys_t: the arrays and the n x n table of constant stencils of a coupled system of n = 2 or 3 node fields (include/examg.h)."""
    _fields_ = [("n", C.c_int32), ("lu", LayoutC), ("lf", LayoutC), ("ld", LayoutC), ("u", C.c_void_p * BSYS_MAX), ("f", C.c_void_p * BSYS_MAX),
                ("dst", C.c_void_p * BSYS_MAX), ("A", C.POINTER(StencilC) * (BSYS_MAX * BSYS_MAX))]


class MacC(C.Structure):
    """examg_mac_t: the arrays and the operator of a staggered saddle-point system: nd face fields and the cell pressure (include/examg.h)."""
    _fields_ = [("nd", C.c_int32), ("lu", LayoutC * 3), ("lp", LayoutC), ("lf", LayoutC * 3), ("lfp", LayoutC), ("ld", LayoutC * 3), ("ldp", LayoutC),
                ("u", C.c_void_p * 3), ("p", C.c_void_p), ("f", C.c_void_p * 3), ("fp", C.c_void_p), ("dst", C.c_void_p * 3), ("dstp", C.c_void_p),
                ("A", C.POINTER(StencilC) * 3), ("bc", C.c_double * 3), ("bm", C.c_double * 3), ("cc", C.c_double * 3), ("cp", C.c_double * 3)]


MAX_EXPR = 256
OPS = {"const": 0, "x": 1, "y": 2, "z": 3, "+": 4, "-": 5, "*": 6, "/": 7, "neg": 8, "sin": 9, "cos": 10, "exp": 11, "sinh": 12,
       "cosh": 13, "sqrt": 14, "pow": 15, "tan": 16, "log": 17, "fabs": 18, "max": 19, "min": 20, "tanh": 21}
# ... and the widths of the point's cell, which the _grid entry points know beside them (every other entry point refuses them)
# ... and the node of the cell's own index, an operand of the EXAMG_BC_VALUE_MINUS kind of examg_apply_bc_cell alone
GRID_OPS = dict(OPS, wx=23, wy=24, wz=25, nx=26, ny=27, nz=28)


class ExprC(C.Structure):
    """examg_expr_t: a postfix program over the node position (include/examg.h)."""
    _fields_ = [("n", C.c_int32), ("op", C.c_int32 * MAX_EXPR), ("c", C.c_double * MAX_EXPR)]

    @staticmethod
    def from_program(prog):
        """prog: list of (opcode name, constant or None)."""
        if not 1 <= len(prog) <= MAX_EXPR:
            raise ValueError("expression program with %d instructions (limit %d)" % (len(prog), MAX_EXPR))
        e = ExprC()
        e.n = len(prog)
        for i, (name, c) in enumerate(prog):
            e.op[i] = GRID_OPS[name]
            e.c[i] = float(c) if c is not None else 0.0
        e.program = list(prog)
        return e


class BcFaceC(C.Structure):
    """examg_bc_face_t: the kind and the program of one face of examg_apply_bc_cell_faces."""
    _fields_ = [("kind", C.c_int32), ("expr", C.POINTER(ExprC))]


MAX_NL_EXPR = 32
NL_STACK = 8
NL_APPLY, NL_RESIDUAL, NL_ADD = 0, 1, 2
NL_OPS = dict(OPS, u=22)
for _pos in ("x", "y", "z"):      # a program over a field value has no node position
    del NL_OPS[_pos]


class NlExprC(C.Structure):
    """examg_nlexpr_t: a postfix program over the value of a field at the point (include/examg.h); `u` pushes that value."""
    _fields_ = [("n", C.c_int32), ("op", C.c_int32 * MAX_NL_EXPR), ("c", C.c_double * MAX_NL_EXPR)]

    @staticmethod
    def from_program(prog):
        """prog: list of (opcode name, constant or None)."""
        if not 1 <= len(prog) <= MAX_NL_EXPR:
            raise ValueError("point program with %d instructions (limit %d)" % (len(prog), MAX_NL_EXPR))
        e = NlExprC()
        e.n = len(prog)
        for i, (name, c) in enumerate(prog):
            if name not in NL_OPS:
                raise ValueError("point program with the instruction %r" % name)
            e.op[i] = NL_OPS[name]
            e.c[i] = float(c) if c is not None else 0.0
        e.program = list(prog)
        return e


# ---- explicit flux-form steps on cell fields (include/examg.h: examg_flux_t) ----------------------------------------------------------
FLUX_MAX_FIELDS, FLUX_MAX_PROGS, FLUX_MAX_COMP, FLUX_MAX_TERMS, FLUX_MAX_ENTRIES = 6, 8, 4, 4, 5
FLUX_GATHER, FLUX_MARCH = 1, 2            # what examg_flux_route answers (-1 refused, 0 empty box)
FLUX_DEFAULT = FLUX_MARCH                 # the kernel examg_flux_step takes (the measured table decides it)
REDUCE_MAX, REDUCE_MIN = 0, 1
OP_FIELD0 = 32
# ---- complex-valued node fields (include/examg.h: examg_cstencil_op and what follows it) --------------------------------------------------
CRELAX = 3                                # the fourth loop kind of examg_cstencil_op, beside EXAMG_APPLY / RESIDUAL / SMOOTH
CSTENCIL_GATHER, CSTENCIL_MARCH = 1, 2    # what examg_cstencil_route answers (-1 refused, 0 empty box)
C_XPAY, C_XMAY, C_XPAYMBZ = 0, 1, 2       # the forms of examg_clincomb
# `f<k>` pushes the value of input field k at the cell the program is evaluated at; no `u`, no position
FLUX_OPS = dict((k, v) for k, v in NL_OPS.items() if k != "u")
FLUX_OPS.update(("f%d" % k, OP_FIELD0 + k) for k in range(FLUX_MAX_FIELDS))


class FluxTermC(C.Structure):
    """examg_flux_term_t: scale * (P(i + plus) - P(i + minus)), P = prog[prog]."""
    _fields_ = [("prog", C.c_int32), ("plus", C.c_int32 * 3), ("minus", C.c_int32 * 3), ("scale", C.c_double)]


class FluxCompC(C.Structure):
    """examg_flux_comp_t: one component: a constant axis stencil on in[field] and up to FLUX_MAX_TERMS terms."""
    _fields_ = [("field", C.c_int32), ("nent", C.c_int32), ("off", (C.c_int32 * 3) * FLUX_MAX_ENTRIES), ("coef", C.c_double * FLUX_MAX_ENTRIES),
                ("nterms", C.c_int32), ("term", FluxTermC * FLUX_MAX_TERMS)]


class FluxC(C.Structure):
    """examg_flux_t"""
    _fields_ = [("nfields", C.c_int32), ("nprogs", C.c_int32), ("ncomp", C.c_int32), ("lin", LayoutC), ("lout", LayoutC),
                ("in_", C.c_void_p * FLUX_MAX_FIELDS), ("out", C.c_void_p * FLUX_MAX_COMP), ("prog", NlExprC * FLUX_MAX_PROGS),
                ("comp", FluxCompC * FLUX_MAX_COMP)]


class ExamgError(RuntimeError):
    pass


_lib = None
_libs = {}
DBG_LIB_PATH = os.path.join(_HERE, "libexamg_dbg.so")   # -DEXAMG_DEBUG_HOOKS build: variant selection for the parity tests

# every symbol include/examg.h declares
SYMBOLS = [
    "examg_version", "examg_last_error", "examg_device_count", "examg_stencil_op", "examg_jacobi",
    "examg_rbgs_colour", "examg_residual", "examg_rbgs_sweep_fused", "examg_rbgs_sweep_fused_boxes", "examg_jacobi2", "examg_jacobi3", "examg_rbgs_colours3", "examg_three_stage_eligible", "examg_pow2_fma_eligible", "examg_jacobi2_boxes", "examg_jacobi_residual", "examg_rbgs_sweep_fused_prolong", "examg_jacobi2_prolong", "examg_rbgs_sweep_fused_zero", "examg_two_stage_eligible", "examg_restrict", "examg_residual_restrict", "examg_prolong_add",
    "examg_set", "examg_axpby", "examg_axpby_dev", "examg_reduce_work_bytes", "examg_dot", "examg_residual_norm2",
    "examg_fill_expr", "examg_apply_dirichlet_expr", "examg_fill_dup_faces_expr", "examg_max_err_expr", "examg_init_varcoeff7", "examg_init_helmholtz27", "examg_pack", "examg_unpack",
    "examg_cg_coarse", "examg_cg_coarse_variant", "examg_fill_random", "examg_copy_to_external", "examg_copy_from_external",
    "examg_comm_unique_id", "examg_comm_create", "examg_comm_destroy", "examg_comm_rank", "examg_comm_size",
    "examg_exchange_workspace_bytes", "examg_exchange", "examg_allreduce", "examg_allgather",
    "examg_jacobi2_blocks", "examg_rbgs_sweep_blocks", "examg_crand_seed", "examg_crand_draw_host",
    "examg_transform_stencilfield", "examg_transform_field", "examg_layout_size", "examg_comm_peer_release", "examg_residual_restrict_one_pass", "examg_residual_restrict_blocks", "examg_prolong_add_blocks",
    "examg_comm_create_peer", "examg_comm_peer_alloc", "examg_comm_peer_connect", "examg_comm_peer_slab_bytes",
    "examg_comm_peer_gather_bytes", "examg_comm_status",
    "examg_sum", "examg_add_scalar", "examg_fill_expr_cell", "examg_max_err_expr_cell", "examg_apply_bc_cell", "examg_apply_bc_cell_faces", "examg_restrict_cell",
    "examg_prolong_add_cell",
    "examg_stencil_op_coloured", "examg_mcgs_sweep", "examg_mcgs_one_pass_eligible",
    "examg_sys_op", "examg_sys_relax", "examg_pointwise_mul",
    "examg_vec_op", "examg_vec_smooth", "examg_vec_dot", "examg_vec_set", "examg_vec_axpby", "examg_vec_restrict_cell",
    "examg_vec_prolong_add_cell", "examg_vec_apply_bc_cell",
    "examg_bsys_op", "examg_bsys_relax", "examg_bsys_route",
    "examg_nl_op", "examg_nl_smooth",
    "examg_gs_sweep", "examg_gs_route",
    "examg_axis_op", "examg_axis_route", "examg_fill_expr_grid", "examg_apply_dirichlet_expr_grid", "examg_max_err_expr_grid",
    "examg_flux_step", "examg_flux_route", "examg_reduce_expr_cell",
    "examg_cstencil_op", "examg_cstencil_route", "examg_clincomb", "examg_cdot", "examg_crestrict", "examg_cprolong_add", "examg_cshift_div",
    "examg_cfrom_parts",
    "examg_mac_op", "examg_mac_relax", "examg_mac_sweep", "examg_restrict_face", "examg_prolong_add_face", "examg_apply_bc_face",
    "examg_fill_expr_face", "examg_max_err_expr_face",
]

COMM_ID_BYTES = 128
PEER_HANDLE_BYTES = 128
EXCH_DUP, EXCH_GHOST, EXCH_ALL, EXCH_CONCURRENT_AXES = 1, 2, 3, 4
PASS_TMP_PLANES_VALID = 8
BC_DIRICHLET, BC_NEUMANN, BC_NEGATE, BC_VALUE_MINUS = 0, 1, 2, 4
CG_ALPHA_FROM_NORM, CG_NO_BC, CG_ZERO_START = 1, 2, 4
GS_REFUSED, GS_EMPTY, GS_ONE_WORKGROUP, GS_TILED, GS_PER_HYPERPLANE = -1, 0, 1, 2, 3      # examg_gs_route


class CrandStateC(C.Structure):
    """examg_crand_state_t"""
    _fields_ = [("r", C.c_uint32 * 31), ("k", C.c_int32)]


class NeighborsC(C.Structure):
    """examg_neighbors_t"""
    _fields_ = [("rank", (C.c_int32 * 2) * 3)]


def load(path=None):
    """Load libexamg.so (or the library at `path`) and declare the prototypes.  Raises if the HIP library is not built."""
    global _lib
    path = path or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise ExamgError(
            "%s not found -- build it with `python -c 'import __graft_entry__ as g; g.build()'`; "
            "there is no CPU fallback" % path)
    # torch first: libexamg.so needs libamdhip64.so.7 and must bind to the one HIP runtime of the process,
    # the copy PyTorch ships and loads (two runtimes in one process do not both see the device)
    import torch  # noqa: F401

    L = C.CDLL(path)
    vp, ip = C.c_void_p, C.POINTER(C.c_int32)
    lp, sp, gp, dp = C.POINTER(LayoutC), C.POINTER(StencilC), C.POINTER(GeomC), C.POINTER(C.c_double)
    L.examg_version.restype = C.c_int
    L.examg_last_error.restype = C.c_char_p
    L.examg_device_count.restype = C.c_int
    L.examg_stencil_op.argtypes = [C.c_int, lp, vp, lp, vp, lp, vp, sp, C.c_double, C.c_int, ip, ip, vp]
    L.examg_jacobi.argtypes = [lp, vp, vp, lp, vp, sp, C.c_double, ip, ip, vp]
    L.examg_rbgs_colour.argtypes = [lp, vp, lp, vp, sp, C.c_double, C.c_int, ip, ip, vp]
    L.examg_residual.argtypes = [lp, vp, lp, vp, lp, vp, sp, ip, ip, vp]
    L.examg_rbgs_sweep_fused.argtypes = [lp, vp, vp, lp, vp, sp, C.c_double, C.c_int, ip, ip, vp]
    L.examg_jacobi2.argtypes = [lp, vp, vp, vp, lp, vp, sp, C.c_double, ip, ip, vp]
    L.examg_jacobi3.argtypes = [lp, vp, vp, vp, lp, vp, sp, C.c_double, ip, ip, vp]
    L.examg_rbgs_colours3.argtypes = [lp, vp, vp, lp, vp, sp, C.c_double, C.c_int, ip, ip, vp]
    L.examg_three_stage_eligible.argtypes = [lp, lp, sp, ip, ip]
    L.examg_pow2_fma_eligible.argtypes = [sp]
    L.examg_jacobi_residual.argtypes = [lp, vp, vp, lp, vp, lp, vp, sp, C.c_double, ip, ip, vp]
    L.examg_jacobi2_boxes.argtypes = [lp, vp, vp, vp, lp, vp, sp, C.c_double, ip, ip, ip, ip, vp]
    L.examg_rbgs_sweep_fused_boxes.argtypes = [lp, vp, vp, vp, lp, vp, sp, C.c_double, C.c_int, ip, ip, ip, ip, vp]
    L.examg_rbgs_sweep_fused_prolong.argtypes = [lp, vp, vp, lp, vp, sp, C.c_double, C.c_int, ip, ip, lp, vp, vp]
    L.examg_rbgs_sweep_fused_zero.argtypes = [lp, vp, lp, vp, sp, C.c_double, C.c_int, ip, ip, vp]
    L.examg_jacobi2_prolong.argtypes = [lp, vp, vp, vp, lp, vp, sp, C.c_double, ip, ip, lp, vp, vp]
    L.examg_two_stage_eligible.argtypes = [lp, lp, sp, ip, ip, ip, ip]
    L.examg_restrict.argtypes = [lp, vp, lp, vp, C.c_double, ip, ip, vp]
    L.examg_residual_restrict.argtypes = [lp, vp, lp, vp, lp, vp, sp, lp, vp, C.c_double, ip, ip, ip, ip, vp]
    L.examg_prolong_add.argtypes = [lp, vp, lp, vp, ip, ip, vp]
    L.examg_set.argtypes = [lp, vp, C.c_double, ip, ip, vp]
    L.examg_axpby.argtypes = [lp, vp, lp, vp, C.c_double, C.c_double, ip, ip, vp]
    L.examg_axpby_dev.argtypes = [lp, vp, lp, vp, C.c_double, C.c_double, C.c_int, C.c_double, vp, vp, ip, ip, vp]
    L.examg_reduce_work_bytes.restype = C.c_size_t
    L.examg_dot.argtypes = [lp, vp, lp, vp, ip, ip, vp, vp, vp]
    L.examg_residual_norm2.argtypes = [lp, vp, lp, vp, sp, ip, ip, lp, vp, vp, vp, vp]
    ep = C.POINTER(ExprC)
    L.examg_fill_expr.argtypes = [lp, vp, gp, ep, ip, ip, vp]
    L.examg_apply_dirichlet_expr.argtypes = [lp, vp, gp, ep, C.c_uint32, vp]
    L.examg_fill_dup_faces_expr.argtypes = [lp, vp, gp, ep, C.c_uint32, vp]
    L.examg_max_err_expr.argtypes = [lp, vp, gp, ep, ip, ip, vp, vp, vp]
    L.examg_init_varcoeff7.argtypes = [lp, vp, gp, ep, ip, ip, vp]
    L.examg_init_helmholtz27.argtypes = [lp, vp, gp, ep, C.c_double, ip, ip, vp]
    L.examg_transform_stencilfield.argtypes = [lp, C.c_int, vp, vp, C.c_int, vp]
    L.examg_transform_field.argtypes = [lp, vp, lp, vp, vp]
    L.examg_layout_size.argtypes = [lp]
    L.examg_layout_size.restype = C.c_int64
    L.examg_pack.argtypes = [lp, vp, vp, ip, ip, vp]
    L.examg_unpack.argtypes = [lp, vp, vp, ip, ip, vp]
    L.examg_cg_coarse.argtypes = [lp, vp, lp, vp, lp, vp, lp, vp, lp, vp, sp, gp, C.c_uint32, C.c_int, C.c_double, ip, ip, vp, vp]
    L.examg_cg_coarse_variant.argtypes = [lp, vp, lp, vp, lp, vp, lp, vp, lp, vp, sp, gp, C.c_uint32, C.c_int, C.c_double, ip, ip,
                                          C.c_uint32, vp, vp]
    L.examg_copy_to_external.argtypes = [lp, vp, lp, vp, vp]
    L.examg_copy_from_external.argtypes = [lp, vp, lp, vp, vp]
    L.examg_fill_random.argtypes = [vp, C.c_int64, C.c_uint64, vp]
    L.examg_comm_unique_id.argtypes = [vp]
    L.examg_comm_create.argtypes = [C.POINTER(vp), vp, C.c_int, C.c_int]
    L.examg_comm_destroy.argtypes = [vp]
    L.examg_comm_rank.argtypes = [vp]
    L.examg_comm_size.argtypes = [vp]
    L.examg_exchange_workspace_bytes.argtypes = [lp]
    L.examg_exchange_workspace_bytes.restype = C.c_size_t
    L.examg_exchange.argtypes = [vp, lp, vp, C.POINTER(NeighborsC), C.c_int, vp, C.c_size_t, vp]
    L.examg_allreduce.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    nbp = C.POINTER(NeighborsC)
    L.examg_crand_seed.argtypes = [C.POINTER(CrandStateC), C.c_uint32]
    L.examg_crand_draw_host.argtypes = [C.POINTER(CrandStateC), vp, C.c_int64]
    L.examg_jacobi2_blocks.argtypes = [vp, nbp, lp, vp, vp, vp, lp, vp, sp, C.c_double, ip, ip, C.c_int, vp, C.c_size_t, C.c_int, vp]
    L.examg_rbgs_sweep_blocks.argtypes = [vp, nbp, lp, vp, vp, vp, lp, vp, sp, C.c_double, C.c_int, ip, ip, C.c_int, vp, C.c_size_t, C.c_int, vp]
    L.examg_allgather.argtypes = [vp, vp, vp, C.c_int64, vp]
    L.examg_residual_restrict_one_pass.argtypes = [lp, lp, sp, lp, ip, ip, ip, ip]
    L.examg_residual_restrict_blocks.argtypes = [vp, nbp, lp, vp, lp, vp, lp, vp, sp, lp, vp, C.c_double, ip, ip, ip, ip, C.c_int, vp, C.c_size_t,
                                                 C.c_int, vp]
    L.examg_prolong_add_blocks.argtypes = [vp, nbp, lp, vp, lp, vp, ip, ip, C.c_int, vp, C.c_size_t, C.c_int, vp]
    L.examg_comm_create_peer.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
    L.examg_comm_peer_alloc.argtypes = [vp, C.c_size_t, C.c_size_t, vp]
    L.examg_comm_peer_connect.argtypes = [vp, vp]
    L.examg_comm_peer_slab_bytes.argtypes = [vp]
    L.examg_comm_peer_slab_bytes.restype = C.c_size_t
    L.examg_comm_peer_gather_bytes.argtypes = [vp]
    L.examg_comm_peer_gather_bytes.restype = C.c_size_t
    L.examg_comm_status.argtypes = [vp, vp]
    L.examg_sum.argtypes = [lp, vp, ip, ip, vp, vp, vp]
    L.examg_add_scalar.argtypes = [lp, vp, C.c_double, ip, ip, vp]
    L.examg_fill_expr_cell.argtypes = [lp, vp, gp, ep, ip, ip, vp]
    L.examg_max_err_expr_cell.argtypes = [lp, vp, gp, ep, ip, ip, vp, vp, vp]
    L.examg_apply_bc_cell.argtypes = [lp, vp, gp, C.c_int, ep, C.c_uint32, vp]
    L.examg_apply_bc_cell_faces.argtypes = [lp, vp, gp, C.POINTER(BcFaceC), C.c_uint32, vp]
    L.examg_restrict_cell.argtypes = [lp, vp, lp, vp, C.c_double, ip, ip, vp]
    L.examg_prolong_add_cell.argtypes = [lp, vp, lp, vp, ip, ip, vp]
    cp = C.POINTER(ColouringC)
    L.examg_stencil_op_coloured.argtypes = [C.c_int, lp, vp, lp, vp, lp, vp, sp, C.c_double, cp, ip, ip, vp]
    L.examg_mcgs_sweep.argtypes = [lp, vp, lp, vp, sp, C.c_double, cp, ip, ip, vp]
    L.examg_mcgs_one_pass_eligible.argtypes = [lp, lp, sp, cp, ip, ip]
    yp = C.POINTER(SysC)
    L.examg_sys_op.argtypes = [C.c_int, yp, sp, C.c_uint32, ip, ip, vp]
    L.examg_sys_relax.argtypes = [yp, sp, C.c_double, C.c_int, ip, ip, vp]
    L.examg_pointwise_mul.argtypes = [lp, vp, lp, vp, lp, vp, C.c_double, ip, ip, vp]
    mp = C.POINTER(VecStencilC)
    L.examg_vec_op.argtypes = [C.c_int, C.c_int, lp, vp, lp, vp, lp, vp, mp, ip, ip, vp]
    L.examg_vec_smooth.argtypes = [C.c_int, lp, vp, lp, vp, mp, C.c_double, C.c_int, ip, ip, vp]
    L.examg_vec_dot.argtypes = [C.c_int, lp, vp, lp, vp, ip, ip, vp, vp, vp]
    L.examg_vec_set.argtypes = [C.c_int, lp, vp, C.c_double, ip, ip, vp]
    L.examg_vec_axpby.argtypes = [C.c_int, lp, vp, lp, vp, C.c_double, C.c_double, ip, ip, vp]
    L.examg_vec_restrict_cell.argtypes = [C.c_int, lp, vp, lp, vp, C.c_double, ip, ip, vp]
    L.examg_vec_prolong_add_cell.argtypes = [C.c_int, lp, vp, lp, vp, ip, ip, vp]
    L.examg_vec_apply_bc_cell.argtypes = [C.c_int, lp, vp, gp, C.c_int, C.c_uint32, vp]
    bp = C.POINTER(BsysC)
    L.examg_bsys_op.argtypes = [C.c_int, bp, C.c_uint32, ip, ip, vp]
    L.examg_bsys_relax.argtypes = [bp, C.c_double, cp, ip, ip, vp]
    L.examg_bsys_route.argtypes = [C.c_int, bp, C.c_uint32, ip, ip]
    np_ = C.POINTER(NlExprC)
    L.examg_nl_op.argtypes = [C.c_int, lp, vp, lp, vp, lp, vp, lp, vp, sp, np_, ip, ip, vp]
    L.examg_nl_smooth.argtypes = [lp, vp, lp, vp, lp, vp, sp, np_, np_, C.c_double, C.c_int, ip, ip, vp]
    L.examg_gs_sweep.argtypes = [lp, vp, lp, vp, sp, C.c_double, ip, ip, vp]
    L.examg_gs_route.argtypes = [lp, lp, sp, ip, ip]
    ap = C.POINTER(AxisStencilC)
    L.examg_axis_op.argtypes = [C.c_int, lp, vp, lp, vp, lp, vp, ap, C.c_double, C.c_int, ip, ip, vp]
    L.examg_axis_route.argtypes = [C.c_int, lp, lp, lp, ap, C.c_int, ip, ip]
    rp = C.POINTER(GridC)
    L.examg_fill_expr_grid.argtypes = [lp, vp, rp, ep, ip, ip, vp]
    L.examg_apply_dirichlet_expr_grid.argtypes = [lp, vp, rp, ep, C.c_uint32, vp]
    L.examg_max_err_expr_grid.argtypes = [lp, vp, rp, ep, ip, ip, vp, vp, vp]
    xp = C.POINTER(FluxC)
    L.examg_flux_step.argtypes = [xp, ip, ip, vp]
    L.examg_flux_route.argtypes = [xp, ip, ip]
    L.examg_reduce_expr_cell.argtypes = [C.c_int, C.c_int, lp, C.POINTER(vp), np_, ip, ip, vp, vp, vp]
    L.examg_cstencil_op.argtypes = [C.c_int, lp, vp, lp, vp, lp, vp, sp, dp, dp, C.c_int, ip, ip, vp]
    L.examg_cstencil_route.argtypes = [C.c_int, lp, vp, lp, vp, lp, vp, sp, dp, dp, C.c_int, ip, ip]
    L.examg_clincomb.argtypes = [C.c_int, lp, vp, lp, vp, lp, vp, lp, vp, dp, dp, ip, ip, vp]
    L.examg_cdot.argtypes = [lp, vp, lp, vp, ip, ip, vp, vp, vp]
    L.examg_crestrict.argtypes = [lp, vp, lp, vp, C.c_double, ip, ip, vp]
    L.examg_cprolong_add.argtypes = [lp, vp, lp, vp, ip, ip, vp]
    L.examg_cshift_div.argtypes = [lp, vp, ip, dp, ip, ip, vp]
    L.examg_cfrom_parts.argtypes = [lp, vp, lp, vp, lp, vp, ip, ip, vp]
    kp = C.POINTER(MacC)
    L.examg_mac_op.argtypes = [C.c_int, kp, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp]
    L.examg_mac_relax.argtypes = [kp, C.c_double, cp, ip, ip, vp]
    L.examg_mac_sweep.argtypes = [kp, C.c_double, cp, ip, ip, vp]
    L.examg_restrict_face.argtypes = [C.c_int, lp, vp, lp, vp, C.c_double, ip, ip, vp]
    L.examg_prolong_add_face.argtypes = [C.c_int, lp, vp, lp, vp, ip, ip, vp]
    L.examg_apply_bc_face.argtypes = [C.c_int, lp, vp, gp, C.c_int, ep, C.c_uint32, vp]
    L.examg_fill_expr_face.argtypes = [C.c_int, lp, vp, gp, ep, ip, ip, vp]
    L.examg_max_err_expr_face.argtypes = [C.c_int, lp, vp, gp, ep, ip, ip, vp, vp, vp]
    for name in SYMBOLS:
        fn = getattr(L, name)  # AttributeError if a declared symbol is not exported
        if name not in ("examg_version", "examg_last_error", "examg_device_count", "examg_reduce_work_bytes", "examg_exchange_workspace_bytes",
                        "examg_comm_peer_slab_bytes", "examg_comm_peer_gather_bytes"):
            fn.restype = C.c_int
    if hasattr(L, "examg_debug_force_generic"):      # debug build only
        L.examg_debug_force_generic.argtypes = [C.c_int]
        L.examg_debug_force_generic.restype = C.c_int
    if hasattr(L, "examg_debug_star2d"):             # debug build only: the y-marching 2-D star off / by the rule / wherever possible, rows per chunk
        L.examg_debug_star2d.argtypes = [C.c_int, C.c_int]
        L.examg_debug_star2d.restype = C.c_int
    if hasattr(L, "examg_debug_cell_narrow"):        # debug build only: the 8-byte form of the cell transfer kernels
        L.examg_debug_cell_narrow.argtypes = [C.c_int]
        L.examg_debug_cell_narrow.restype = C.c_int
    if hasattr(L, "examg_debug_mcgs_per_colour"):    # debug build only: examg_mcgs_sweep as its colour loops
        L.examg_debug_mcgs_per_colour.argtypes = [C.c_int]
        L.examg_debug_mcgs_per_colour.restype = C.c_int
    if hasattr(L, "examg_debug_nl_gather_only"):     # debug build only: star stencils of the semilinear kernels on the gather kernel
        L.examg_debug_nl_gather_only.argtypes = [C.c_int]
        L.examg_debug_nl_gather_only.restype = C.c_int
    if hasattr(L, "examg_debug_flux_route"):         # debug build only: examg_flux_step on the kernel named (0: the default)
        L.examg_debug_flux_route.argtypes = [C.c_int]
        L.examg_debug_flux_route.restype = C.c_int
    if hasattr(L, "examg_debug_cstencil_route"):     # debug build only: examg_cstencil_op on the kernel named (0: the default), rows per wave
        L.examg_debug_cstencil_route.argtypes = [C.c_int, C.c_int]
        L.examg_debug_cstencil_route.restype = C.c_int
    if hasattr(L, "examg_debug_sys_narrow"):         # debug build only: the 8-byte form of the system kernels
        L.examg_debug_sys_narrow.argtypes = [C.c_int]
        L.examg_debug_sys_narrow.restype = C.c_int
    if hasattr(L, "examg_debug_vec_narrow"):         # debug build only: the 8-byte form of the vector-field kernels
        L.examg_debug_vec_narrow.argtypes = [C.c_int]
        L.examg_debug_vec_narrow.restype = C.c_int
    if hasattr(L, "examg_debug_cg_route"):           # debug build only: the form of the one-kernel coarse solver, and which one a call takes
        L.examg_debug_cg.argtypes = [C.c_int]
        L.examg_debug_cg.restype = C.c_int
        L.examg_debug_cg_route.argtypes = [lp, lp, lp, lp, lp, sp, C.c_uint32, ip, ip, C.c_uint32]
        L.examg_debug_cg_route.restype = C.c_int
    if hasattr(L, "examg_debug_gs_route"):           # debug build only: the route of examg_gs_sweep forced, its schedule point by point
        L.examg_debug_gs_route.argtypes = [C.c_int]
        L.examg_debug_gs_route.restype = C.c_int
        L.examg_debug_gs_launches.argtypes = [lp, lp, sp, ip, ip]
        L.examg_debug_gs_launches.restype = C.c_int
        L.examg_debug_gs_schedule.argtypes = [lp, lp, sp, ip, ip, vp, vp]
        L.examg_debug_gs_schedule.restype = C.c_int
    _libs[path] = L
    if path == LIB_PATH:
        _lib = L
    return L


def check(rc: int, what: str = ""):
    if rc != 0:
        raise ExamgError("%s failed (%d): %s" % (what or "libexamg call", rc, load().examg_last_error().decode()))


def ivec(v):
    return (C.c_int32 * 3)(*[int(x) for x in v])


def dvec2(z):
    """(re, im) of a Python number as the two doubles the complex entry points take."""
    z = complex(z)
    return (C.c_double * 2)(z.real, z.imag)


def dvec4(v):
    v = list(v) + [0.0] * (4 - len(v))
    return (C.c_double * 4)(*v[:4])
