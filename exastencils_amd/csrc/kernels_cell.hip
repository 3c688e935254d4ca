// Cell-centred fields on gfx950: ghost-layer boundary conditions and the linear cell transfer operators.
//
// Reference: `Layout X< Real, Cell >` fields (Testing/CellBased/{2D,3D}_{Basic,Neumann}.exa4); boundary updates
// Compiler/src/exastencils/boundary/ir/IR_DirichletBC.scala / IR_NeumannBC.scala (generateFieldUpdatesCell, order 1) over the
// boundary row of boundary/ir/IR_ApplyBCFunction.scala:53-83, face-centre coordinates boundary/ir/IR_HandleBoundaries.scala:55-70;
// transfer stencils operator/l4/L4_DefaultRestriction.scala:37-43,63-90 and L4_DefaultProlongation.scala:30-45.
//
// The transfer kernels are pure streams (8 B in, 1 B out per fine cell for the restriction; 8 B in, 8 B out, 1 B in for the
// prolongation): a wave owns a contiguous x-run of 64 coarse cells of one coarse row; lane l takes coarse cell I = first + l,
// whose two fine x-children (2I, 2I+1) are adjacent -- one 16-byte load (or store) per fine row where the fine rows start
// 16-byte aligned (FieldLayout.cell(..., align=2)), two 8-byte accesses otherwise; both forms compute the same bits.  A wave
// covers all 2^(d-1) fine rows of its coarse row, so every fine value is read once and every coarse value once per wave.
#include "examg_common.h"

namespace examg {

// ---- apply bc ---------------------------------------------------------------------------------------------------------------
struct CellFaces {
  Box box[6];          // the boundary row of cells of each face (iterator coordinates)
  int dim[6], up[6];   // normal dimension, 1 for the upper side
  long long start[7];  // prefix sums of the counts
  int n;
};

// One launch for every face of the mask.  Thread t -> (face, boundary cell); the ghost is the cell one step outwards.
// cs: doubles between the components of a vector-valued field, blockIdx.y the component (a scalar field: one) -- in all three kernels.
template <int KIND>
__global__ void __launch_bounds__(256) k_apply_bc_cell(LayoutDev l, double *x, Geom g, ExprEval fn, CellFaces fc, int3 inner, long long cs) {
  x += blockIdx.y * cs;
  const long long total = fc.start[fc.n];
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    int f = 0;
    while (f + 1 < fc.n && t >= fc.start[f + 1]) ++f;
    const Box &bx = fc.box[f];
    const long long r = t - fc.start[f];
    const int n0 = bx.n0(), n1 = bx.n1();
    int i[3];
    i[0] = bx.b0 + (int)(r % n0);
    i[1] = bx.b1 + (int)((r / n0) % n1);
    i[2] = bx.b2 + (int)(r / ((long long)n0 * n1));
    const int d = fc.dim[f], up = fc.up[f];
    int o[3] = {i[0], i[1], i[2]};
    o[d] += up ? 1 : -1;
    const double interior = x[lidx(l, i[0], i[1], i[2])];
    double v;
    if (KIND == EXAMG_BC_NEUMANN) {
      v = interior;
    } else if (KIND == EXAMG_BC_NEGATE) {
      v = -interior;
    } else {
      // face centre: cell centres tangentially, the node position of the face (index 0 / inner) in the normal dimension
      double p[3];
      point_position<true>(g, i[0], i[1], i[2], p[0], p[1], p[2]);
      const double hh[3] = {g.h0, g.h1, g.h2}, pb[3] = {g.pb0, g.pb1, g.pb2};
      const int nidx = up ? (d == 0 ? inner.x : (d == 1 ? inner.y : inner.z)) : 0;
      p[d] = nidx * hh[d] + pb[d];
      v = (2.0 * fn(p[0], p[1], p[2])) - interior;
    }
    x[lidx(l, o[0], o[1], o[2])] = v;
  }
}

// Every face of the mask with a kind and a program of its own (examg_apply_bc_cell_faces; EXAMG_BC_VALUE_MINUS of examg_apply_bc_cell).
// The programs travel packed, one copy per distinct program: six examg_expr_t would not fit the kernel arguments.
constexpr int FACE_PROG_MAX = EXAMG_MAX_EXPR;      // instructions of the distinct programs of one call together
struct FaceTable {
  int kind[6];             // per entry of CellFaces
  int ps[6], pn[6];        // the program of the face: first instruction, length
  unsigned char op[FACE_PROG_MAX];
  double c[FACE_PROG_MAX];
};

// expr_eval over a packed program; (x, y, z) the cell centre, (nx, ny, nz) the node of the cell's own index (EXAMG_OP_NODE_*): the same
// operations in the same order
__device__ __forceinline__ double face_expr_eval(const FaceTable &e, int b, int n, double x, double y, double z, double nx, double ny, double nz) {
  double st[24];
  int sp = 0;
  for (int i = b; i < b + n; ++i) {
    switch (e.op[i]) {
      case EXAMG_OP_CONST: st[sp++] = e.c[i]; break;
      case EXAMG_OP_X: st[sp++] = x; break;
      case EXAMG_OP_Y: st[sp++] = y; break;
      case EXAMG_OP_Z: st[sp++] = z; break;
      case EXAMG_OP_NODE_X: st[sp++] = nx; break;
      case EXAMG_OP_NODE_Y: st[sp++] = ny; break;
      case EXAMG_OP_NODE_Z: st[sp++] = nz; break;
      case EXAMG_OP_ADD: --sp; st[sp - 1] = st[sp - 1] + st[sp]; break;
      case EXAMG_OP_SUB: --sp; st[sp - 1] = st[sp - 1] - st[sp]; break;
      case EXAMG_OP_MUL: --sp; st[sp - 1] = st[sp - 1] * st[sp]; break;
      case EXAMG_OP_DIV: --sp; st[sp - 1] = st[sp - 1] / st[sp]; break;
      case EXAMG_OP_NEG: st[sp - 1] = -st[sp - 1]; break;
      case EXAMG_OP_SIN: st[sp - 1] = sin(st[sp - 1]); break;
      case EXAMG_OP_COS: st[sp - 1] = cos(st[sp - 1]); break;
      case EXAMG_OP_EXP: st[sp - 1] = exp(st[sp - 1]); break;
      case EXAMG_OP_SINH: st[sp - 1] = sinh(st[sp - 1]); break;
      case EXAMG_OP_COSH: st[sp - 1] = cosh(st[sp - 1]); break;
      case EXAMG_OP_SQRT: st[sp - 1] = sqrt(st[sp - 1]); break;
      case EXAMG_OP_POW: --sp; st[sp - 1] = pow(st[sp - 1], st[sp]); break;
      case EXAMG_OP_TAN: st[sp - 1] = tan(st[sp - 1]); break;
      case EXAMG_OP_LOG: st[sp - 1] = log(st[sp - 1]); break;
      case EXAMG_OP_FABS: st[sp - 1] = fabs(st[sp - 1]); break;
      case EXAMG_OP_MAX: --sp; st[sp - 1] = fmax(st[sp - 1], st[sp]); break;
      case EXAMG_OP_MIN: --sp; st[sp - 1] = fmin(st[sp - 1], st[sp]); break;
      case EXAMG_OP_TANH: st[sp - 1] = tanh(st[sp - 1]); break;
      default: st[sp++] = __builtin_nan(""); break;
    }
  }
  return st[0];
}

// Thread t -> (face, boundary cell) as in k_apply_bc_cell; the kind is the face's.  The faces of a cell field never read one another's
// ghosts (edge and corner ghosts are not written), so the launch equals the single-face launches in any order.
__global__ void __launch_bounds__(256) k_apply_bc_cell_faces(LayoutDev l, double *x, Geom g, CellFaces fc, FaceTable ft, int3 inner) {
  const long long total = fc.start[fc.n];
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    int f = 0;
    while (f + 1 < fc.n && t >= fc.start[f + 1]) ++f;
    const Box &bx = fc.box[f];
    const long long r = t - fc.start[f];
    const int n0 = bx.n0(), n1 = bx.n1();
    int i[3];
    i[0] = bx.b0 + (int)(r % n0);
    i[1] = bx.b1 + (int)((r / n0) % n1);
    i[2] = bx.b2 + (int)(r / ((long long)n0 * n1));
    const int d = fc.dim[f], up = fc.up[f], kind = ft.kind[f];
    int o[3] = {i[0], i[1], i[2]};
    o[d] += up ? 1 : -1;
    const double interior = x[lidx(l, i[0], i[1], i[2])];
    double v;
    if (kind == EXAMG_BC_NEUMANN) {
      v = interior;
    } else if (kind == EXAMG_BC_NEGATE) {
      v = -interior;
    } else if (kind == EXAMG_BC_VALUE_MINUS) {
      // g at the ghost cell itself: its centre, and the node of its own index
      double p[3], q[3];
      point_position<1>(g, o[0], o[1], o[2], p[0], p[1], p[2]);
      point_position<0>(g, o[0], o[1], o[2], q[0], q[1], q[2]);
      v = face_expr_eval(ft, ft.ps[f], ft.pn[f], p[0], p[1], p[2], q[0], q[1], q[2]) - interior;
    } else {
      // face centre: cell centres tangentially, the node position of the face (index 0 / inner) in the normal dimension
      double p[3];
      point_position<1>(g, i[0], i[1], i[2], p[0], p[1], p[2]);
      const double hh[3] = {g.h0, g.h1, g.h2}, pb[3] = {g.pb0, g.pb1, g.pb2};
      const int nidx = up ? (d == 0 ? inner.x : (d == 1 ? inner.y : inner.z)) : 0;
      p[d] = nidx * hh[d] + pb[d];
      v = (2.0 * face_expr_eval(ft, ft.ps[f], ft.pn[f], p[0], p[1], p[2], 0.0, 0.0, 0.0)) - interior;
    }
    x[lidx(l, o[0], o[1], o[2])] = v;
  }
}

// ---- restriction ----------------------------------------------------------------------------------------------------------
// fc(I) = sum_{a, b, c in {0,1}} (scale * 0.5^d) * rf(2I + (a, b, c)), terms added in the entry order of the composed stencil
// kron(kron(Rx, Ry), Rz) (L4_StencilOps.kron: left entries outer, right entries inner): x offset outermost, then y, then z.
// VEC: the pair (2I, 2I+1) of every fine row with one aligned 16-byte load.
template <int ND, bool VEC>
__global__ void __launch_bounds__(256)
k_restrict_cell(LayoutDev lf, const double *__restrict__ rf, LayoutDev lc, double *__restrict__ fc, double wgt, Box box, int ntx, int nwaves,
                long long csf, long long csc) {
  rf += blockIdx.y * csf;
  fc += blockIdx.y * csc;
  const int lane = threadIdx.x;
  const long long wg = xcd_band(blockIdx.x, ntx * ((box.n1() + 3) >> 2));
  const int wpl = ntx * ((box.n1() + 3) >> 2);
  const long long lz = wg / wpl;
  const int r = (int)(wg - lz * wpl);
  const int tx = r % ntx;
  const int jw = (r / ntx) * 4 + (int)__builtin_amdgcn_readfirstlane(threadIdx.y);
  if (jw >= box.n1()) return;
  const long long w = lz * box.n1() + jw;
  if (w >= nwaves) return;
  const int I0 = box.b0 + tx * 64 + lane;
  if (I0 >= box.e0) return;
  const int I1 = box.b1 + jw;
  const int I2 = box.b2 + (int)lz;
  constexpr int NR = ND == 3 ? 4 : 2;     // fine rows of the coarse cell: (b, c) with b outer
  double v[NR][2];
#pragma unroll
  for (int q = 0; q < NR; ++q) {
    const int b = ND == 3 ? (q >> 1) : q, c = ND == 3 ? (q & 1) : 0;
    const double *p = rf + lidx_plain(lf, 2 * I0, 2 * I1 + b, ND == 3 ? 2 * I2 + c : 0);
    if (VEC) {
      const d2 t = *reinterpret_cast<const d2 *>(p);
      v[q][0] = t.x;
      v[q][1] = t.y;
    } else {
      v[q][0] = p[0];
      v[q][1] = p[1];
    }
  }
  double acc = wgt * v[0][0];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      if (a == 0 && q == 0) continue;
      acc = acc + wgt * v[q][a];
    }
  fc[lidx_plain(lc, I0, I1, I2)] = acc;
}

// ---- prolongation + correction --------------------------------------------------------------------------------------------
// uf(i) = uf(i) + uc(floor(i / 2)) over the fine box.  Lane l takes the fine pair (2I, 2I+1) of coarse cell I = I0first + l in
// every fine row of coarse row (J, K) that lies in the box: one coarse load serves 2^d fine cells.
template <int ND, bool VEC>
__global__ void __launch_bounds__(256)
k_prolong_add_cell(LayoutDev lc, const double *__restrict__ uc, LayoutDev lf, double *__restrict__ uf, Box box, int cb0, int cb1, int cb2,
                   int nc0, int nc1, int ntx, int nwaves, long long csc, long long csf) {
  uc += blockIdx.y * csc;
  uf += blockIdx.y * csf;
  const int lane = threadIdx.x;
  const int wpl = ntx * ((nc1 + 3) >> 2);
  const long long wg = xcd_band(blockIdx.x, wpl);
  const long long lz = wg / wpl;
  const int r = (int)(wg - lz * wpl);
  const int tx = r % ntx;
  const int jw = (r / ntx) * 4 + (int)__builtin_amdgcn_readfirstlane(threadIdx.y);
  if (jw >= nc1) return;
  const long long w = lz * nc1 + jw;
  if (w >= nwaves) return;
  const int ci = tx * 64 + lane;
  if (ci >= nc0) return;
  const int I0 = cb0 + ci, I1 = cb1 + jw, I2 = cb2 + (int)lz;
  const double c = uc[lidx_plain(lc, I0, I1, I2)];
  const int f0 = 2 * I0;
  const bool ok0 = f0 >= box.b0, ok1 = f0 + 1 < box.e0;
#pragma unroll
  for (int q = 0; q < (ND == 3 ? 4 : 2); ++q) {
    const int j = 2 * I1 + (ND == 3 ? (q >> 1) : q), k = ND == 3 ? 2 * I2 + (q & 1) : box.b2;
    if (j < box.b1 || j >= box.e1 || k < box.b2 || k >= box.e2) continue;
    double *p = uf + lidx_plain(lf, f0, j, k);
    if (VEC && ok0 && ok1) {
      d2 t = *reinterpret_cast<d2 *>(p);
      t.x = t.x + c;
      t.y = t.y + c;
      *reinterpret_cast<d2 *>(p) = t;
    } else {
      if (ok0) p[0] = p[0] + c;
      if (ok1) p[1] = p[1] + c;
    }
  }
}

static bool cell_layout_ok(const char *who, const examg_layout_t *l) {
  for (int d = 0; d < l->nd; ++d)
    if (l->dup_l[d] != 0 || l->dup_r[d] != 0) {
      set_error("%s: a cell layout has no duplicate layers (dim %d has %d / %d)", who, d, l->dup_l[d], l->dup_r[d]);
      return false;
    }
  if (lay_split(l)) { set_error("%s: cell layouts under a layout transformation are not supported", who); return false; }
  return true;
}

// 16-byte access to the fine pair (2I, 2I+1) of every fine row: the pointer and the linear index of every even fine x index
// are even (reference offset and row strides even)
static bool pairs_aligned(const examg_layout_t *l, const double *p) {
  const LayoutDev d = make_layout(l);
  return ((uintptr_t)p & 15) == 0 && (d.origin & 1) == 0 && (d.s1 & 1) == 0 && (l->nd < 3 || (d.s2 & 1) == 0);
}

static int g_force_narrow = 0;   // debug build: force the 8-byte form

}  // namespace examg

using namespace examg;

#ifdef EXAMG_DEBUG_HOOKS
extern "C" int examg_debug_cell_narrow(int on) {
  g_force_narrow = on;
  return 0;
}
#endif

// the boundary row of cells of every face of the mask, in the order dimension, side; false: error text set
static bool cell_faces(const char *who, const examg_layout_t *l, uint32_t face_mask, CellFaces &fc, int (&face_of)[6]) {
  fc.n = 0;
  fc.start[0] = 0;
  for (int d = 0; d < l->nd; ++d)
    for (int side = 0; side < 2; ++side) {
      if (!(face_mask & (1u << (2 * d + side)))) continue;
      if ((side ? l->ghost_r[d] : l->ghost_l[d]) < 1) {
        set_error("%s: face %d of dim %d has no ghost layer", who, side, d);
        return false;
      }
      int b[3] = {0, 0, 0}, e[3] = {1, 1, 1};
      for (int t = 0; t < l->nd; ++t) {
        b[t] = 0;
        e[t] = l->inner[t];
      }
      if (side == 0) e[d] = 1;
      else b[d] = l->inner[d] - 1;
      const Box bx{b[0], b[1], b[2], e[0], e[1], e[2]};
      if (bx.count() == 0) continue;
      fc.box[fc.n] = bx;
      fc.dim[fc.n] = d;
      fc.up[fc.n] = side;
      face_of[fc.n] = 2 * d + side;
      fc.start[fc.n + 1] = fc.start[fc.n] + bx.count();
      ++fc.n;
    }
  return true;
}

// ncomp > 1: every component of a vector-valued field (examg_vec_*), the component the y dimension of the grid
static int apply_bc_cell_impl(const char *who, const examg_layout_t *l, double *x, const examg_geom_t *g, int kind, const examg_expr_t *expr,
                              uint32_t face_mask, examg_stream_t stream, int ncomp) {
  if (!l || !x || !g) { set_error("%s: null argument", who); return 1; }
  if (kind != EXAMG_BC_DIRICHLET && kind != EXAMG_BC_NEUMANN && kind != EXAMG_BC_NEGATE) { set_error("%s: unknown kind %d", who, kind); return 1; }
  if (kind == EXAMG_BC_DIRICHLET && !expr_ok(expr)) return 1;
  if (!cell_layout_ok(who, l)) return 1;
  CellFaces fc;
  int face_of[6];
  if (!cell_faces(who, l, face_mask, fc, face_of)) return 1;
  if (fc.n == 0) return 0;
  examg_expr_t none;
  if (kind != EXAMG_BC_DIRICHLET) {
    none.n = 1;
    none.op[0] = EXAMG_OP_CONST;
    none.c[0] = 0.0;
  }
  const ExprEval fn{kind != EXAMG_BC_DIRICHLET ? none : *expr};
  const int3 inner = make_int3(l->inner[0], l->inner[1], l->inner[2]);
  const long long total = fc.start[fc.n];
  long long nb = (total + 255) / 256;
  if (nb > 2048) nb = 2048;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)nb, ncomp);
  const LayoutDev ld = make_layout(l);
  const long long cs = ncomp > 1 ? ld.size : 0;
  if (kind == EXAMG_BC_NEUMANN)
    hipLaunchKernelGGL((k_apply_bc_cell<EXAMG_BC_NEUMANN>), grid, dim3(256), 0, s, ld, x, make_geom(g), fn, fc, inner, cs);
  else if (kind == EXAMG_BC_NEGATE)
    hipLaunchKernelGGL((k_apply_bc_cell<EXAMG_BC_NEGATE>), grid, dim3(256), 0, s, ld, x, make_geom(g), fn, fc, inner, cs);
  else
    hipLaunchKernelGGL((k_apply_bc_cell<EXAMG_BC_DIRICHLET>), grid, dim3(256), 0, s, ld, x, make_geom(g), fn, fc, inner, cs);
  EXAMG_CHECK_LAUNCH("k_apply_bc_cell");
  return 0;
}

// the program of a face: the stack discipline of expr_ok; the node-position opcodes are operands of EXAMG_BC_VALUE_MINUS only
static bool face_expr_ok(int kind, const examg_expr_t *e) {
  if (kind != EXAMG_BC_VALUE_MINUS) return expr_ok(e);
  if (!e || e->n < 1 || e->n > EXAMG_MAX_EXPR) { set_error("examg expression: null or too long"); return false; }
  examg_expr_t q = *e;
  for (int i = 0; i < q.n; ++i)
    if (q.op[i] >= EXAMG_OP_NODE_X && q.op[i] <= EXAMG_OP_NODE_Z) q.op[i] = EXAMG_OP_X;      // an operand like the position
  return expr_ok(&q);
}

// faces[2 * d + side]: the kind and the program of every face of the mask
static int apply_bc_cell_faces_impl(const char *who, const examg_layout_t *l, double *x, const examg_geom_t *g, const examg_bc_face_t *faces,
                                    uint32_t face_mask, examg_stream_t stream) {
  if (!l || !x || !g || !faces) { set_error("%s: null argument", who); return 1; }
  if (l->nd < 1 || l->nd > 3) { set_error("%s: bad layout dimensionality %d", who, l->nd); return 1; }
  for (int f = 0; f < 2 * l->nd; ++f) {
    if (!(face_mask & (1u << f))) continue;
    const int kind = faces[f].kind;
    if (kind != EXAMG_BC_DIRICHLET && kind != EXAMG_BC_NEUMANN && kind != EXAMG_BC_NEGATE && kind != EXAMG_BC_VALUE_MINUS) {
      set_error("%s: unknown kind %d", who, kind);
      return 1;
    }
    if ((kind == EXAMG_BC_DIRICHLET || kind == EXAMG_BC_VALUE_MINUS) && !face_expr_ok(kind, faces[f].expr)) return 1;
  }
  if (!cell_layout_ok(who, l)) return 1;
  CellFaces fc;
  int face_of[6];
  if (!cell_faces(who, l, face_mask, fc, face_of)) return 1;
  if (fc.n == 0) return 0;
  FaceTable ft;
  int used = 0;
  for (int k = 0; k < 6; ++k) ft.kind[k] = EXAMG_BC_NEUMANN, ft.ps[k] = 0, ft.pn[k] = 0;
  for (int k = 0; k < fc.n; ++k) {
    const examg_bc_face_t &fa = faces[face_of[k]];
    ft.kind[k] = fa.kind;
    if (fa.kind != EXAMG_BC_DIRICHLET && fa.kind != EXAMG_BC_VALUE_MINUS) continue;
    int same = -1;      // faces that name one program share its copy
    for (int j = 0; j < k && same < 0; ++j)
      if (ft.pn[j] > 0 && faces[face_of[j]].expr == fa.expr) same = j;
    if (same >= 0) { ft.ps[k] = ft.ps[same]; ft.pn[k] = ft.pn[same]; continue; }
    if (used + fa.expr->n > FACE_PROG_MAX) {
      set_error("%s: the programs of the faces have more than %d instructions together", who, FACE_PROG_MAX);
      return 1;
    }
    ft.ps[k] = used;
    ft.pn[k] = fa.expr->n;
    for (int i = 0; i < fa.expr->n; ++i) {
      ft.op[used + i] = (unsigned char)fa.expr->op[i];
      ft.c[used + i] = fa.expr->c[i];
    }
    used += fa.expr->n;
  }
  for (int i = used; i < FACE_PROG_MAX; ++i) ft.op[i] = 0, ft.c[i] = 0.0;
  const int3 inner = make_int3(l->inner[0], l->inner[1], l->inner[2]);
  long long nb = (fc.start[fc.n] + 255) / 256;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(k_apply_bc_cell_faces, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, make_layout(l), x, make_geom(g), fc, ft, inner);
  EXAMG_CHECK_LAUNCH("k_apply_bc_cell_faces");
  return 0;
}

extern "C" int examg_apply_bc_cell(const examg_layout_t *l, double *x, const examg_geom_t *g, int kind, const examg_expr_t *expr,
                                   uint32_t face_mask, examg_stream_t stream) {
  if (kind == EXAMG_BC_VALUE_MINUS) {      // the kind that evaluates at the ghost cell: the kernel of the faces call, one program for every face
    examg_bc_face_t faces[6];
    for (int f = 0; f < 6; ++f) faces[f].kind = kind, faces[f].expr = expr;
    return apply_bc_cell_faces_impl("examg_apply_bc_cell", l, x, g, faces, face_mask, stream);
  }
  return apply_bc_cell_impl("examg_apply_bc_cell", l, x, g, kind, expr, face_mask, stream, 1);
}

extern "C" int examg_apply_bc_cell_faces(const examg_layout_t *l, double *x, const examg_geom_t *g, const examg_bc_face_t *faces,
                                         uint32_t face_mask, examg_stream_t stream) {
  return apply_bc_cell_faces_impl("examg_apply_bc_cell_faces", l, x, g, faces, face_mask, stream);
}

extern "C" int examg_vec_apply_bc_cell(int n, const examg_layout_t *l, double *x, const examg_geom_t *g, int kind, uint32_t face_mask,
                                       examg_stream_t stream) {
  if (!l) { set_error("examg_vec_apply_bc_cell: null argument"); return 1; }
  if (!vec_fields_ok("examg_vec_apply_bc_cell", n, l, nullptr)) return 1;
  if (kind == EXAMG_BC_VALUE_MINUS) { set_error("examg_vec_apply_bc_cell: EXAMG_BC_VALUE_MINUS; vector-valued fields take EXAMG_BC_NEUMANN only"); return 1; }
  if (kind != EXAMG_BC_NEUMANN) { set_error("examg_vec_apply_bc_cell: kind %d; vector-valued fields take EXAMG_BC_NEUMANN only", kind); return 1; }
  return apply_bc_cell_impl("examg_vec_apply_bc_cell", l, x, g, kind, nullptr, face_mask, stream, n);
}

static int restrict_cell_impl(const char *who, const examg_layout_t *lf_, const double *rf, const examg_layout_t *lc_, double *fc, double scale, const int32_t *begin,
                              const int32_t *end, examg_stream_t stream, int ncomp) {
  if (!lf_ || !rf || !lc_ || !fc || !begin || !end) { set_error("%s: null argument", who); return 1; }
  // the dimensionality first: cell_layout_ok walks the nd dimensions of the per-dimension arrays, and nd = 4 would run as 2-D
  if (lf_->nd != lc_->nd || (lf_->nd != 2 && lf_->nd != 3)) { set_error("%s: 2-D or 3-D layouts of one dimensionality", who); return 1; }
  if (!cell_layout_ok(who, lf_) || !cell_layout_ok(who, lc_)) return 1;
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 0;
  const int nd = lf_->nd;
  const Box fine{2 * box.b0, 2 * box.b1, nd == 3 ? 2 * box.b2 : 0, 2 * box.e0, 2 * box.e1, nd == 3 ? 2 * box.e2 : 1};
  if (!box_inside(lc_, box, 0) || !box_inside(lf_, fine, 0)) { set_error("%s: box leaves an allocation", who); return 1; }
  if (nd == 2 && (box.b2 != 0 || box.e2 != 1)) { set_error("%s: 2-D box must have [0,1) in dim 2", who); return 1; }
  const double wgt = scale * (nd == 3 ? 0.125 : 0.25);
  const int ntx = (box.n0() + 63) / 64;
  const long long nwaves = (long long)box.n1() * box.n2();
  const long long nwg = (long long)ntx * ((box.n1() + 3) / 4) * box.n2();
  if (nwg > 0x7fffffffLL) { set_error("%s: grid too large", who); return 1; }
  const LayoutDev lf = make_layout(lf_), lc = make_layout(lc_);
  // every component's pairs: an odd size(lfine) puts every other component on the 8-byte form, and then all of them
  const bool vec = !g_force_narrow && pairs_aligned(lf_, rf) && (ncomp == 1 || (lf.size & 1) == 0);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)nwg, ncomp), blk(64, 4);
  const long long csf = ncomp > 1 ? lf.size : 0, csc = ncomp > 1 ? lc.size : 0;
  if (nd == 3) {
    if (vec) hipLaunchKernelGGL((k_restrict_cell<3, true>), grid, blk, 0, s, lf, rf, lc, fc, wgt, box, ntx, (int)nwaves, csf, csc);
    else hipLaunchKernelGGL((k_restrict_cell<3, false>), grid, blk, 0, s, lf, rf, lc, fc, wgt, box, ntx, (int)nwaves, csf, csc);
  } else {
    if (vec) hipLaunchKernelGGL((k_restrict_cell<2, true>), grid, blk, 0, s, lf, rf, lc, fc, wgt, box, ntx, (int)nwaves, csf, csc);
    else hipLaunchKernelGGL((k_restrict_cell<2, false>), grid, blk, 0, s, lf, rf, lc, fc, wgt, box, ntx, (int)nwaves, csf, csc);
  }
  EXAMG_CHECK_LAUNCH("k_restrict_cell");
  return 0;
}

extern "C" int examg_restrict_cell(const examg_layout_t *lf_, const double *rf, const examg_layout_t *lc_, double *fc, double scale,
                                   const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  return restrict_cell_impl("examg_restrict_cell", lf_, rf, lc_, fc, scale, begin, end, stream, 1);
}

extern "C" int examg_vec_restrict_cell(int n, const examg_layout_t *lf_, const double *rf, const examg_layout_t *lc_, double *fc, double scale,
                                       const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  if (!lf_ || !lc_) { set_error("examg_vec_restrict_cell: null argument"); return 1; }
  if (!vec_fields_ok("examg_vec_restrict_cell", n, lf_, lc_)) return 1;
  return restrict_cell_impl("examg_vec_restrict_cell", lf_, rf, lc_, fc, scale, begin, end, stream, n);
}

static int prolong_add_cell_impl(const char *who, const examg_layout_t *lc_, const double *uc, const examg_layout_t *lf_, double *uf, const int32_t *begin,
                                 const int32_t *end, examg_stream_t stream, int ncomp) {
  if (!lc_ || !uc || !lf_ || !uf || !begin || !end) { set_error("%s: null argument", who); return 1; }
  // the dimensionality first: cell_layout_ok walks the nd dimensions of the per-dimension arrays, and nd = 4 would run as 2-D
  if (lf_->nd != lc_->nd || (lf_->nd != 2 && lf_->nd != 3)) { set_error("%s: 2-D or 3-D layouts of one dimensionality", who); return 1; }
  if (!cell_layout_ok(who, lf_) || !cell_layout_ok(who, lc_)) return 1;
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 0;
  const int nd = lf_->nd;
  if (nd == 2 && (box.b2 != 0 || box.e2 != 1)) { set_error("%s: 2-D box must have [0,1) in dim 2", who); return 1; }
  // parent box: floor(i / 2) over the fine box (arithmetic shifts floor negative indices too)
  const int cb0 = box.b0 >> 1, cb1 = box.b1 >> 1, cb2 = nd == 3 ? box.b2 >> 1 : 0;
  const int ce0 = ((box.e0 - 1) >> 1) + 1, ce1 = ((box.e1 - 1) >> 1) + 1, ce2 = nd == 3 ? ((box.e2 - 1) >> 1) + 1 : 1;
  const Box cbox{cb0, cb1, cb2, ce0, ce1, ce2};
  if (!box_inside(lf_, box, 0) || !box_inside(lc_, cbox, 0)) { set_error("%s: box leaves an allocation", who); return 1; }
  const int nc0 = ce0 - cb0, nc1 = ce1 - cb1, nc2 = ce2 - cb2;
  const int ntx = (nc0 + 63) / 64;
  const long long nwaves = (long long)nc1 * nc2;
  const long long nwg = (long long)ntx * ((nc1 + 3) / 4) * nc2;
  if (nwg > 0x7fffffffLL) { set_error("%s: grid too large", who); return 1; }
  const LayoutDev lc = make_layout(lc_), lf = make_layout(lf_);
  const bool vec = !g_force_narrow && pairs_aligned(lf_, uf) && (ncomp == 1 || (lf.size & 1) == 0);   // every component's pairs
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)nwg, ncomp), blk(64, 4);
  const long long csc = ncomp > 1 ? lc.size : 0, csf = ncomp > 1 ? lf.size : 0;
  if (nd == 3) {
    if (vec) hipLaunchKernelGGL((k_prolong_add_cell<3, true>), grid, blk, 0, s, lc, uc, lf, uf, box, cb0, cb1, cb2, nc0, nc1, ntx, (int)nwaves, csc, csf);
    else hipLaunchKernelGGL((k_prolong_add_cell<3, false>), grid, blk, 0, s, lc, uc, lf, uf, box, cb0, cb1, cb2, nc0, nc1, ntx, (int)nwaves, csc, csf);
  } else {
    if (vec) hipLaunchKernelGGL((k_prolong_add_cell<2, true>), grid, blk, 0, s, lc, uc, lf, uf, box, cb0, cb1, cb2, nc0, nc1, ntx, (int)nwaves, csc, csf);
    else hipLaunchKernelGGL((k_prolong_add_cell<2, false>), grid, blk, 0, s, lc, uc, lf, uf, box, cb0, cb1, cb2, nc0, nc1, ntx, (int)nwaves, csc, csf);
  }
  EXAMG_CHECK_LAUNCH("k_prolong_add_cell");
  return 0;
}

extern "C" int examg_prolong_add_cell(const examg_layout_t *lc_, const double *uc, const examg_layout_t *lf_, double *uf,
                                      const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  return prolong_add_cell_impl("examg_prolong_add_cell", lc_, uc, lf_, uf, begin, end, stream, 1);
}

extern "C" int examg_vec_prolong_add_cell(int n, const examg_layout_t *lc_, const double *uc, const examg_layout_t *lf_, double *uf,
                                          const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  if (!lc_ || !lf_) { set_error("examg_vec_prolong_add_cell: null argument"); return 1; }
  if (!vec_fields_ok("examg_vec_prolong_add_cell", n, lc_, lf_)) return 1;
  return prolong_add_cell_impl("examg_vec_prolong_add_cell", lc_, uc, lf_, uf, begin, end, stream, n);
}
