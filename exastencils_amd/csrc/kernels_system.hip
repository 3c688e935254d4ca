// Coupled systems of n = 2 or 3 cell-centred unknowns on gfx950: the operator A = L * I + G(x) (one constant axis stencil L on every
// component, a point-wise n x n matrix of coefficient fields G) and the local solves of its red-black smoother.
//
// Reference: Benchmark/OptFlow2D/2D_FD_OptFlow.exa4 (Horn-Schunck optical flow: `uuSten * u + uvSten * v + alpha * alpha * Laplace * u`),
// `solve locally relax w { u => .. == rhs_u  v => .. == rhs_v }` (solver/l4/L4_LocalSolve.scala, solver/ir/IR_LocalSolve.scala: the
// unknowns of the loop's cell go into AVals, everything else into fVals) inside `repeat with { colour conditions, .. }`
// (baseExt/l4/L4_RepeatLoops.scala).  The arithmetic order is fixed in include/examg.h; this file is compiled with contraction off.
//
// Access pattern (both kernels): a wave owns 128 consecutive x cells of one row, lane l the pair (x, x + 1), x = xo + 128 * tile + 2 * l;
// four rows per workgroup, workgroups of a z layer in XCD bands.  xo is the box's first cell or the cell before it, whichever makes the
// pairs of every argument 16-byte aligned (FieldLayout.cell(..., align=2), or any layout with even strides and origin parity); then the
// own row of every unknown is read with one 16-byte load per lane, otherwise with two 8-byte loads: the same values either way.  The x
// neighbour of a cell is the other value of the lane's pair or the adjacent lane's (DPP wave shift), from memory only at the ends of
// the wave's run.  Coefficient pointers that alias are loaded once.  No LDS, no scratch.
//   k_sys_op    every cell of the pair: y / z neighbours as pairs of the rows beside; coefficients, right-hand sides and results as
//               pairs where both cells lie in the box, single values at its ends.
//   k_sys_relax one cell of the pair carries the colour, the same one in every lane of the wave ((xo + row + plane) parity): y / z
//               neighbours, coefficients, right-hand sides and the n stores are 8-byte accesses at that cell (stride 2 across lanes);
//               only cells of the other colour and the cell's own values are read: race-free in place.
#include "sys_common.h"   // pair loads, wave coordinates, local solves, layout checks: shared with kernels_vector.hip

namespace examg {

// the stencil L as the kernels take it: entry k multiplies the value `code` names: 0 centre, 1 + 2d the lower, 2 + 2d the upper neighbour in d
struct SysStencil {
  int nent;
  int code[7];
  double coef[7];
  double centre;
};

template <int N>
struct SysArgs {
  double *u[N];
  const double *f[N];
  double *dst[N];
  const double *g[N * N];
  int same[N * N];   // index of an earlier entry of g with the same pointer (its value is reused), else -1
  LayoutDev lu, lf, lg, ld;
  SysStencil L;
};

// entries of L folded left to right in declared order (examg_common.h: conv7); OFFC: the entries off the centre only.  any: was there one?
template <bool OFFC>
__device__ __forceinline__ double sys_fold(const SysStencil &L, double c, double xm, double xp, double ym, double yp, double zm, double zp, bool &any) {
  double acc = 0.0;
  bool first = true;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    if (k < L.nent && !(OFFC && L.code[k] == 0)) {
      const double t = L.coef[k] * sys_pick(L.code[k], c, xm, xp, ym, yp, zm, zp);
      acc = first ? t : acc + t;
      first = false;
    }
  }
  any = !first;
  return acc;
}

// ---- dst_c = A u (EXAMG_SYS_APPLY) or f_c - A u (EXAMG_SYS_RESIDUAL) for the rows c of the mask ------------------------------------
template <int ND, int N, bool VEC>
__global__ void __launch_bounds__(256) k_sys_op(SysArgs<N> a, int mode, unsigned mask, Box box, int xo, int ntx) {
  int x, row, plane;
  if (!sys_wave_coords(box, xo, ntx, x, row, plane)) return;
  const int lane = threadIdx.x;
  const bool va = x >= box.b0 && x < box.e0, vb = x + 1 >= box.b0 && x + 1 < box.e0;
  const bool act = va || vb;    // then x - 1 .. x + 2 lie in the box grown by one cell: inside the allocation of the unknowns
  const bool lload = va && (lane == 0 || x - 2 < box.b0 - 1);   // the lane below holds no pair
  const bool rload = vb && (lane == 63 || x + 2 >= box.e0);     // the lane above holds no pair
  const long long iu = lidx_plain(a.lu, act ? x : box.b0, row, plane);
  const long long ig = lidx_plain(a.lg, x, row, plane), jf = lidx_plain(a.lf, x, row, plane), id = lidx_plain(a.ld, x, row, plane);

  // which unknowns the rows of the mask read at the cell
  bool needu[N];
#pragma unroll
  for (int d = 0; d < N; ++d) {
    needu[d] = (mask >> d) & 1u;
#pragma unroll
    for (int c = 0; c < N; ++c) needu[d] = needu[d] || (((mask >> c) & 1u) && a.g[c * N + d] != nullptr);
  }
  d2 P[N];
#pragma unroll
  for (int d = 0; d < N; ++d) {
    P[d] = d2{0.0, 0.0};
    if (needu[d] && act) P[d] = sys_load_pair<VEC>(a.u[d] + iu);
  }
  // coefficients of the rows of the mask, an aliased pointer once
  d2 G[N * N];
#pragma unroll
  for (int e = 0; e < N * N; ++e) {
    G[e] = d2{0.0, 0.0};
    if (((mask >> (e / N)) & 1u) && a.g[e] != nullptr) {
      if (a.same[e] < 0) {
        G[e] = sys_load_pair_g<VEC>(a.g[e] + ig, va, vb);
      } else {
#pragma unroll
        for (int q = 0; q < e; ++q)
          if (a.same[e] == q) G[e] = G[q];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < N; ++c) {
    // the lane exchange stands outside every divergent branch: all 64 lanes take part
    double xl = lane_below(P[c].y), xr = lane_above(P[c].x);
    if (!((mask >> c) & 1u)) continue;    // uniform
    const double *uc = a.u[c] + iu;
    if (lload) xl = uc[-1];
    if (rload) xr = uc[2];
    d2 ym = {0.0, 0.0}, yp = ym, zm = ym, zp = ym;
    if (act) {
      ym = sys_load_pair<VEC>(uc - a.lu.s1);
      yp = sys_load_pair<VEC>(uc + a.lu.s1);
      if (ND == 3) {
        zm = sys_load_pair<VEC>(uc - a.lu.s2);
        zp = sys_load_pair<VEC>(uc + a.lu.s2);
      }
    }
    bool any;
    const double cva = sys_fold<false>(a.L, P[c].x, xl, P[c].y, ym.x, yp.x, zm.x, zp.x, any);
    const double cvb = sys_fold<false>(a.L, P[c].y, P[c].x, xr, ym.y, yp.y, zm.y, zp.y, any);
    d2 s = {0.0, 0.0};
    bool first = true;
#pragma unroll
    for (int d = 0; d < N; ++d) {
      if (a.g[c * N + d] != nullptr) {
        const d2 t = {G[c * N + d].x * P[d].x, G[c * N + d].y * P[d].y};
        s = first ? t : d2{s.x + t.x, s.y + t.y};
        first = false;
      }
    }
    d2 o = first ? d2{cva, cvb} : d2{s.x + cva, s.y + cvb};
    if (mode == EXAMG_SYS_RESIDUAL) {
      const d2 fv = sys_load_pair_g<VEC>(a.f[c] + jf, va, vb);
      o = d2{fv.x - o.x, fv.y - o.y};
    }
    double *q = a.dst[c] + id;
    if (va && vb) {
      if (VEC) *reinterpret_cast<d2 *>(q) = o;
      else { q[0] = o.x; q[1] = o.y; }
    } else if (va) {
      q[0] = o.x;
    } else if (vb) {
      q[1] = o.y;
    }
  }
}

// ---- the local solve of one colour, in place (sys_solve: sys_common.h) -----------------------------------------------------------------
template <int ND, int N, bool VEC>
__global__ void __launch_bounds__(256) k_sys_relax(SysArgs<N> a, double relax, int colour, Box box, int xo, int ntx) {
  int x, row, plane;
  if (!sys_wave_coords(box, xo, ntx, x, row, plane)) return;
  const int lane = threadIdx.x;
  const bool va = x >= box.b0 && x < box.e0, vb = x + 1 >= box.b0 && x + 1 < box.e0;
  const bool act = va || vb;
  // x = xo + 128 * tile + 2 * lane: the cell of the pair that carries the colour is the same in every lane (scalar)
  const int sel = (((xo + row + plane) & 1) == colour) ? 0 : 1;
  const bool cv = sel == 0 ? va : vb;                            // this lane's cell of the colour lies in the box
  const bool lload = sel == 0 && va && (lane == 0 || x - 2 < box.b0 - 1);
  const bool rload = sel == 1 && vb && (lane == 63 || x + 2 >= box.e0);
  const long long iu = lidx_plain(a.lu, act ? x : box.b0, row, plane);
  const long long ig = lidx_plain(a.lg, x + sel, row, plane), jf = lidx_plain(a.lf, x + sel, row, plane);

  double m[N * N], b[N], own[N];
  double xl[N], xr[N];
#pragma unroll
  for (int c = 0; c < N; ++c) {
    d2 p = {0.0, 0.0};
    if (act) p = sys_load_pair<VEC>(a.u[c] + iu);
    // all 64 lanes take part in the exchange; the ends of the run read memory
    const double below = lane_below(p.y), above = lane_above(p.x);
    own[c] = sel == 0 ? p.x : p.y;
    xl[c] = sel == 0 ? below : p.x;
    xr[c] = sel == 0 ? p.y : above;
    if (lload) xl[c] = a.u[c][iu - 1];
    if (rload) xr[c] = a.u[c][iu + 2];
  }
  if (!cv) return;
#pragma unroll
  for (int e = 0; e < N * N; ++e) {
    m[e] = 0.0;
    if (a.g[e] != nullptr) {
      if (a.same[e] < 0) {
        m[e] = a.g[e][ig];
      } else {
#pragma unroll
        for (int q = 0; q < e; ++q)
          if (a.same[e] == q) m[e] = m[q];
      }
    }
  }
  // the diagonal after every alias has taken the plain coefficient
#pragma unroll
  for (int c = 0; c < N; ++c) m[c * N + c] = a.g[c * N + c] != nullptr ? m[c * N + c] + a.L.centre : a.L.centre;
#pragma unroll
  for (int c = 0; c < N; ++c) {
    const double *uc = a.u[c] + iu + sel;
    double ym = 0.0, yp = 0.0, zm = 0.0, zp = 0.0;
    ym = uc[-a.lu.s1];
    yp = uc[a.lu.s1];
    if (ND == 3) {
      zm = uc[-a.lu.s2];
      zp = uc[a.lu.s2];
    }
    bool any;
    const double off = sys_fold<true>(a.L, own[c], xl[c], xr[c], ym, yp, zm, zp, any);
    const double fv = a.f[c][jf];
    b[c] = any ? fv - off : fv;
  }
  double xs[N];
  sys_solve<N>(m, b, xs);
#pragma unroll
  for (int c = 0; c < N; ++c) a.u[c][iu + sel] = relax == 1.0 ? xs[c] : own[c] + relax * (xs[c] - own[c]);
}

// ---- dst = (s * x) * y -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pointwise_mul(LayoutDev lx, const double *x, LayoutDev ly, const double *y, LayoutDev ld, double *dst, double s,
                                                       Box box) {
  const long long total = box.count();
  const int n0 = box.n0(), n1 = box.n1();
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int i0 = box.b0 + (int)(t % n0), i1 = box.b1 + (int)((t / n0) % n1), i2 = box.b2 + (int)(t / ((long long)n0 * n1));
    dst[lidx_plain(ld, i0, i1, i2)] = (s * x[lidx_plain(lx, i0, i1, i2)]) * y[lidx_plain(ly, i0, i1, i2)];
  }
}

static int g_sys_narrow = 0;   // debug build: force the 8-byte form

// The checks both entry points share, and the kernels' arguments.  relax: the unknowns are the destination.
template <int N>
static int sys_prepare(const char *who, const examg_sys_t *sys, const examg_stencil_t *L, bool relax, bool need_f, unsigned mask, const Box &box,
                       SysArgs<N> &a, int &xo, bool &vec) {
  const int nd = sys->lu.nd;
  a.lu = make_layout(&sys->lu);
  a.lf = make_layout(&sys->lf);
  a.lg = make_layout(&sys->lg);
  a.ld = relax ? a.lu : make_layout(&sys->ld);   // examg_sys_relax has no destination: sys->ld is not looked at
  bool anyg = false;
  for (int e = 0; e < N * N; ++e) {
    a.g[e] = sys->g[e];
    a.same[e] = -1;
    // ... among the rows of the mask: the others are not loaded
    for (int q = 0; q < e && a.same[e] < 0; ++q)
      if (sys->g[e] && sys->g[q] == sys->g[e] && ((mask >> (q / N)) & 1u)) a.same[e] = a.same[q] >= 0 ? a.same[q] : q;
    anyg = anyg || sys->g[e];
  }
  for (int c = 0; c < N; ++c) {
    if (!sys->u[c]) { set_error("%s: unknown %d is a null pointer", who, c); return 1; }
    if (need_f && ((mask >> c) & 1u) && !sys->f[c]) { set_error("%s: right-hand side %d is a null pointer", who, c); return 1; }
    if (!relax && ((mask >> c) & 1u) && !sys->dst[c]) { set_error("%s: destination %d is a null pointer", who, c); return 1; }
    if (!relax && ((mask >> c) & 1u))
      for (int d = 0; d < N; ++d)
        if (sys->dst[c] == sys->u[d]) { set_error("%s: destination %d is unknown %d; the operator does not run in place", who, c, d); return 1; }
    a.u[c] = sys->u[c];
    a.f[c] = sys->f[c];
    a.dst[c] = relax ? nullptr : sys->dst[c];
  }
  if (!box_inside(&sys->lu, box, 1)) { set_error("%s: box + one cell leaves the allocation of the unknowns", who); return 1; }
  if (need_f && !box_inside(&sys->lf, box, 0)) { set_error("%s: box leaves the rhs allocation", who); return 1; }
  if (anyg && !box_inside(&sys->lg, box, 0)) { set_error("%s: box leaves the coefficient allocation", who); return 1; }
  if (!relax && !box_inside(&sys->ld, box, 0)) { set_error("%s: box leaves the dst allocation", who); return 1; }
  if (nd == 2 && (box.b2 != 0 || box.e2 != 1)) { set_error("%s: 2-D box must have [0,1) in dim 2", who); return 1; }
  // the stencil: axis entries of reach 1, each offset once, the centre among them
  a.L.nent = L->nent;
  a.L.centre = 0.0;
  bool centre = false;
  unsigned seen = 0;
  for (int k = 0; k < 7; ++k) {
    a.L.code[k] = 0;
    a.L.coef[k] = 0.0;
  }
  for (int k = 0; k < L->nent; ++k) {
    int nz = 0, code = 0;
    for (int d = 0; d < 3; ++d) {
      const int o = L->off[k][d];
      if (o == 0) continue;
      ++nz;
      if (d >= nd || o < -1 || o > 1) nz = 9;
      code = 1 + 2 * d + (o > 0 ? 1 : 0);
    }
    if (nz > 1) { set_error("%s: stencil entry %d (%d, %d, %d) is not an axis entry of reach 1 of a %d-D cell field", who, k, L->off[k][0], L->off[k][1], L->off[k][2], nd); return 1; }
    if (seen & (1u << code)) { set_error("%s: stencil entry %d repeats an offset", who, k); return 1; }
    seen |= 1u << code;
    a.L.code[k] = code;
    a.L.coef[k] = L->coef[k];
    if (code == 0) {
      centre = true;
      a.L.centre = L->coef[k];
    }
  }
  if (!centre) { set_error("%s: the stencil has no centre entry", who); return 1; }
  // pairs: xo = the first cell or the one before it, whichever is even in the unknowns' array; 16-byte accesses when every argument agrees
  xo = box.b0;
  vec = false;
  if (!g_sys_narrow) {
    const int cand = ((a.lu.origin + box.b0) & 1) ? box.b0 - 1 : box.b0;
    bool ok = true;
    for (int c = 0; c < N; ++c) {
      ok = ok && pairs_even(a.lu, nd, sys->u[c], cand);
      if (!relax) {
        if (need_f && sys->f[c]) ok = ok && pairs_even(a.lf, nd, sys->f[c], cand);
        if (sys->dst[c]) ok = ok && pairs_even(a.ld, nd, sys->dst[c], cand);
      }
    }
    if (!relax)
      for (int e = 0; e < N * N; ++e)
        if (sys->g[e]) ok = ok && pairs_even(a.lg, nd, sys->g[e], cand);
    if (ok) {
      xo = cand;
      vec = true;
    }
  }
  return 0;
}

static int sys_check_head(const char *who, const examg_sys_t *sys, const examg_stencil_t *L, const int32_t *begin, const int32_t *end, bool relax) {
  if (!sys || !L || !begin || !end) { set_error("%s: null argument", who); return 1; }
  if (sys->n < 2 || sys->n > SYS_MAXN) { set_error("%s: n = %d components; systems have 2 or 3", who, sys->n); return 1; }
  const int nd = sys->lu.nd;
  if (nd != 2 && nd != 3) { set_error("%s: 2-D or 3-D layouts", who); return 1; }
  if (!sys_layout_ok(who, "unknowns'", &sys->lu, nd) || !sys_layout_ok(who, "rhs", &sys->lf, nd) || !sys_layout_ok(who, "coefficient", &sys->lg, nd)) return 1;
  if (!relax && !sys_layout_ok(who, "dst", &sys->ld, nd)) return 1;
  for (int d = 0; d < nd; ++d) {
    if (sys->lf.inner[d] != sys->lu.inner[d]) { set_error("%s: the rhs layout has %d cells in dim %d, the unknowns %d", who, sys->lf.inner[d], d, sys->lu.inner[d]); return 1; }
    if (sys->lg.inner[d] != sys->lu.inner[d]) { set_error("%s: the coefficient layout has %d cells in dim %d, the unknowns %d", who, sys->lg.inner[d], d, sys->lu.inner[d]); return 1; }
    if (!relax && sys->ld.inner[d] != sys->lu.inner[d]) { set_error("%s: the dst layout has %d cells in dim %d, the unknowns %d", who, sys->ld.inner[d], d, sys->lu.inner[d]); return 1; }
    if (sys->lu.ghost_l[d] < 1 || sys->lu.ghost_r[d] < 1) { set_error("%s: the unknowns need a ghost layer in dim %d", who, d); return 1; }
  }
  if (L->cfield) { set_error("%s: a stencil field cannot be the constant stencil of a system", who); return 1; }
  if (L->nent < 1 || L->nent > 7) { set_error("%s: nent %d; an axis stencil of reach 1 has 1 to 7 entries", who, L->nent); return 1; }
  return 0;
}

template <int ND, int N>
static int sys_launch(const examg_sys_t *sys, const examg_stencil_t *L, bool relax, int mode, unsigned mask, double w, int colour, const Box &box, hipStream_t s) {
  const char *who = relax ? "examg_sys_relax" : "examg_sys_op";
  SysArgs<N> a;
  int xo;
  bool vec;
  if (sys_prepare<N>(who, sys, L, relax, relax || mode == EXAMG_SYS_RESIDUAL, mask, box, a, xo, vec)) return 1;
  const int ntx = (box.e0 - xo + 127) / 128;
  const long long nwg = (long long)ntx * ((box.n1() + 3) / 4) * box.n2();
  if (nwg > 0x7fffffffLL) { set_error("%s: grid too large", who); return 1; }
  const dim3 grid((unsigned)nwg), blk(64, 4);
  if (relax) {
    if (vec) hipLaunchKernelGGL((k_sys_relax<ND, N, true>), grid, blk, 0, s, a, w, colour, box, xo, ntx);
    else hipLaunchKernelGGL((k_sys_relax<ND, N, false>), grid, blk, 0, s, a, w, colour, box, xo, ntx);
    EXAMG_CHECK_LAUNCH("k_sys_relax");
  } else {
    if (vec) hipLaunchKernelGGL((k_sys_op<ND, N, true>), grid, blk, 0, s, a, mode, mask, box, xo, ntx);
    else hipLaunchKernelGGL((k_sys_op<ND, N, false>), grid, blk, 0, s, a, mode, mask, box, xo, ntx);
    EXAMG_CHECK_LAUNCH("k_sys_op");
  }
  return 0;
}

static int sys_dispatch(const examg_sys_t *sys, const examg_stencil_t *L, bool relax, int mode, unsigned mask, double w, int colour, const Box &box, hipStream_t s) {
  if (sys->lu.nd == 3) return sys->n == 2 ? sys_launch<3, 2>(sys, L, relax, mode, mask, w, colour, box, s) : sys_launch<3, 3>(sys, L, relax, mode, mask, w, colour, box, s);
  return sys->n == 2 ? sys_launch<2, 2>(sys, L, relax, mode, mask, w, colour, box, s) : sys_launch<2, 3>(sys, L, relax, mode, mask, w, colour, box, s);
}

}  // namespace examg

using namespace examg;

#ifdef EXAMG_DEBUG_HOOKS
extern "C" int examg_debug_sys_narrow(int on) {
  g_sys_narrow = on;
  return 0;
}
#endif

extern "C" int examg_sys_op(int mode, const examg_sys_t *sys, const examg_stencil_t *L, uint32_t row_mask, const int32_t *begin, const int32_t *end,
                            examg_stream_t stream) {
  if (mode != EXAMG_SYS_APPLY && mode != EXAMG_SYS_RESIDUAL) { set_error("examg_sys_op: bad mode %d", mode); return 1; }
  if (sys_check_head("examg_sys_op", sys, L, begin, end, false)) return 1;
  if (row_mask == 0 || (row_mask >> sys->n) != 0) { set_error("examg_sys_op: row mask 0x%x for %d rows", row_mask, sys->n); return 1; }
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 0;
  return sys_dispatch(sys, L, false, mode, row_mask, 0.0, 0, box, (hipStream_t)stream);
}

extern "C" int examg_sys_relax(const examg_sys_t *sys, const examg_stencil_t *L, double relax, int colour, const int32_t *begin, const int32_t *end,
                               examg_stream_t stream) {
  if (sys_check_head("examg_sys_relax", sys, L, begin, end, true)) return 1;
  if (colour != 0 && colour != 1) { set_error("examg_sys_relax: colour must be 0 or 1"); return 1; }
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 0;
  return sys_dispatch(sys, L, true, 0, (1u << sys->n) - 1u, relax, colour, box, (hipStream_t)stream);
}

extern "C" int examg_pointwise_mul(const examg_layout_t *lx, const double *x, const examg_layout_t *ly, const double *y, const examg_layout_t *ld,
                                   double *dst, double s, const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  if (!lx || !x || !ly || !y || !ld || !dst || !begin || !end) { set_error("examg_pointwise_mul: null argument"); return 1; }
  if (lay_split(lx) || lay_split(ly) || lay_split(ld)) { set_error("examg_pointwise_mul: layouts under a layout transformation are not supported"); return 1; }
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 0;
  if (!box_inside(lx, box, 0) || !box_inside(ly, box, 0) || !box_inside(ld, box, 0)) { set_error("examg_pointwise_mul: box leaves an allocation"); return 1; }
  long long nb = (box.count() + 255) / 256;
  if (nb > 8192) nb = 8192;
  hipLaunchKernelGGL(k_pointwise_mul, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, make_layout(lx), x, make_layout(ly), y, make_layout(ld), dst, s, box);
  EXAMG_CHECK_LAUNCH("k_pointwise_mul");
  return 0;
}
