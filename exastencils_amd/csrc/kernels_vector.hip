// Vector-valued cell fields of n = 2 or 3 components on gfx950: the matrix-stencil operator and the block smoother
// `u = u + w * ( inverse ( diag ( S ) ) * ( f - S * u ) )` of one colour, all components in one launch.
//
// Reference: Testing/Application/OpticalFlow2D.exa4 / OpticalFlow3D.exa4 (`Layout .. < Vec2, Cell >`, a stencil whose entries are
// matrices); a vector field stores the component slowest (field/l4/L4_FieldLayout.scala:63-73): component c at base + c * size(layout).
// The arithmetic order is fixed in include/examg.h; this file is compiled with contraction off.
//
// Access pattern: that of kernels_system.hip, whose helpers it shares (sys_common.h).  A wave owns 128 consecutive x cells of one row,
// lane l the pair (x, x + 1); four rows per workgroup, workgroups of a z layer in XCD bands; 16-byte accesses where the pairs of every
// argument and component are aligned, 8-byte accesses otherwise, the same bits either way; the x neighbour of a cell is the other value
// of the lane's pair or the adjacent lane's (DPP wave shift), from memory only at the ends of the wave's run.  Coefficient pointers that
// alias are loaded once.  No LDS, no scratch.
//   k_vec_op     every cell of the pair, every row of the matrix.
//   k_vec_smooth one cell of the pair carries the colour, the same one in every lane of the wave; it reads cells of the other colour and
//                the cell's own values only: race-free in place.
#include "sys_common.h"

namespace examg {

// the matrix stencil as the kernels take it
template <int N>
struct VecStencil {
  int nent;
  int code[7];            // sys_pick's code of entry k
  unsigned omask[7];      // off-centre entry k: bit c, the diagonal element of component c is present
  double coef[7][N];      // ... and its value
  unsigned kmask, gmask;  // the centre entry: bit c * N + d, the element has a constant / a coefficient field
  double kc[N * N];
  const double *g[N * N];
  int same[N * N];        // index of an earlier element of g with the same pointer (its value is reused), else -1
};

template <int N>
struct VecArgs {
  double *u;
  const double *f;
  double *dst;
  long long cu, cf, cd;   // doubles between the components of u, f, dst
  LayoutDev lu, lf, lg, ld;
  VecStencil<N> S;
};

// the centre element e at a cell whose coefficient value is gv: k + g, g or k
template <int N>
__device__ __forceinline__ double vec_centre(const VecStencil<N> &S, int e, double gv) {
  const bool hk = (S.kmask >> e) & 1u, hg = (S.gmask >> e) & 1u;
  return hk && hg ? S.kc[e] + gv : (hg ? gv : S.kc[e]);
}

// Mu_c at one cell: own[d] the unknowns at the cell, m the centre matrix there, the rest the neighbours of u_c (include/examg.h)
template <int N>
__device__ __forceinline__ double vec_row(const VecStencil<N> &S, int c, const double (&m)[N * N], const double (&own)[N], double xm, double xp, double ym,
                                          double yp, double zm, double zp) {
  double acc = 0.0;
  bool first = true;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    if (k >= S.nent) continue;
    double t = 0.0;
    bool has = false;
    if (S.code[k] == 0) {
#pragma unroll
      for (int d = 0; d < N; ++d) {
        if (((S.kmask | S.gmask) >> (c * N + d)) & 1u) {
          const double p = m[c * N + d] * own[d];
          t = has ? t + p : p;
          has = true;
        }
      }
    } else if ((S.omask[k] >> c) & 1u) {
      t = S.coef[k][c] * sys_pick(S.code[k], 0.0, xm, xp, ym, yp, zm, zp);
      has = true;
    }
    if (has) {
      acc = first ? t : acc + t;
      first = false;
    }
  }
  return acc;
}

// ---- dst = M u (EXAMG_SYS_APPLY) or f - M u (EXAMG_SYS_RESIDUAL), all rows -------------------------------------------------------------
template <int ND, int N, bool VEC>
__global__ void __launch_bounds__(256) k_vec_op(VecArgs<N> a, int mode, Box box, int xo, int ntx) {
  int x, row, plane;
  if (!sys_wave_coords(box, xo, ntx, x, row, plane)) return;
  const int lane = threadIdx.x;
  const bool va = x >= box.b0 && x < box.e0, vb = x + 1 >= box.b0 && x + 1 < box.e0;
  const bool act = va || vb;    // then x - 1 .. x + 2 lie in the box grown by one cell: inside the allocation of the unknowns
  const bool lload = va && (lane == 0 || x - 2 < box.b0 - 1);   // the lane below holds no pair
  const bool rload = vb && (lane == 63 || x + 2 >= box.e0);     // the lane above holds no pair
  const long long iu = lidx_plain(a.lu, act ? x : box.b0, row, plane);
  const long long ig = lidx_plain(a.lg, x, row, plane), jf = lidx_plain(a.lf, x, row, plane), id = lidx_plain(a.ld, x, row, plane);

  d2 P[N];
#pragma unroll
  for (int d = 0; d < N; ++d) {
    P[d] = d2{0.0, 0.0};
    if (act) P[d] = sys_load_pair<VEC>(a.u + d * a.cu + iu);
  }
  // the centre matrix at both cells, an aliased coefficient pointer once
  d2 G[N * N];
  double ma[N * N], mb[N * N];
#pragma unroll
  for (int e = 0; e < N * N; ++e) {
    G[e] = d2{0.0, 0.0};
    if ((a.S.gmask >> e) & 1u) {
      if (a.S.same[e] < 0) {
        G[e] = sys_load_pair_g<VEC>(a.S.g[e] + ig, va, vb);
      } else {
#pragma unroll
        for (int q = 0; q < e; ++q)
          if (a.S.same[e] == q) G[e] = G[q];
      }
    }
    ma[e] = vec_centre<N>(a.S, e, G[e].x);
    mb[e] = vec_centre<N>(a.S, e, G[e].y);
  }
  double owna[N], ownb[N];
#pragma unroll
  for (int d = 0; d < N; ++d) {
    owna[d] = P[d].x;
    ownb[d] = P[d].y;
  }
#pragma unroll
  for (int c = 0; c < N; ++c) {
    // the lane exchange stands outside every divergent branch: all 64 lanes take part
    double xl = lane_below(P[c].y), xr = lane_above(P[c].x);
    const double *uc = a.u + c * a.cu + iu;
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
    d2 o;
    o.x = vec_row<N>(a.S, c, ma, owna, xl, P[c].y, ym.x, yp.x, zm.x, zp.x);
    o.y = vec_row<N>(a.S, c, mb, ownb, P[c].x, xr, ym.y, yp.y, zm.y, zp.y);
    if (mode == EXAMG_SYS_RESIDUAL) {
      const d2 fv = sys_load_pair_g<VEC>(a.f + c * a.cf + jf, va, vb);
      o = d2{fv.x - o.x, fv.y - o.y};
    }
    double *q = a.dst + c * a.cd + id;
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

// ---- one colour of u = u + relax * (inverse(D) * (f - M u)), in place -----------------------------------------------------------------
template <int ND, int N, bool VEC>
__global__ void __launch_bounds__(256) k_vec_smooth(VecArgs<N> a, double relax, int colour, Box box, int xo, int ntx) {
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

  double own[N], xl[N], xr[N];
#pragma unroll
  for (int c = 0; c < N; ++c) {
    d2 p = {0.0, 0.0};
    if (act) p = sys_load_pair<VEC>(a.u + c * a.cu + iu);
    // all 64 lanes take part in the exchange; the ends of the run read memory
    const double below = lane_below(p.y), above = lane_above(p.x);
    own[c] = sel == 0 ? p.x : p.y;
    xl[c] = sel == 0 ? below : p.x;
    xr[c] = sel == 0 ? p.y : above;
    if (lload) xl[c] = a.u[c * a.cu + iu - 1];
    if (rload) xr[c] = a.u[c * a.cu + iu + 2];
  }
  if (!cv) return;
  double gv[N * N], m[N * N], dm[N * N];
#pragma unroll
  for (int e = 0; e < N * N; ++e) {
    gv[e] = 0.0;
    if ((a.S.gmask >> e) & 1u) {
      if (a.S.same[e] < 0) {
        gv[e] = a.S.g[e][ig];
      } else {
#pragma unroll
        for (int q = 0; q < e; ++q)
          if (a.S.same[e] == q) gv[e] = gv[q];
      }
    }
    m[e] = vec_centre<N>(a.S, e, gv[e]);
    dm[e] = (((a.S.kmask | a.S.gmask) >> e) & 1u) ? m[e] : 0.0;     // D: absent elements read as 0.0
  }
  double r[N];
#pragma unroll
  for (int c = 0; c < N; ++c) {
    const double *uc = a.u + c * a.cu + iu + sel;
    double zm = 0.0, zp = 0.0;
    const double ym = uc[-a.lu.s1], yp = uc[a.lu.s1];
    if (ND == 3) {
      zm = uc[-a.lu.s2];
      zp = uc[a.lu.s2];
    }
    r[c] = a.f[c * a.cf + jf] - vec_row<N>(a.S, c, m, own, xl[c], xr[c], ym, yp, zm, zp);
  }
  double xs[N];
  sys_solve<N>(dm, r, xs);
#pragma unroll
  for (int c = 0; c < N; ++c) a.u[c * a.cu + iu + sel] = relax == 1.0 ? own[c] + xs[c] : own[c] + relax * xs[c];
}

static int g_vec_narrow = 0;   // debug build: force the 8-byte form

static bool ranges_overlap(const double *p, long long np, const double *q, long long nq) {
  return p < q + nq && q < p + np;
}

// Every check of the two entry points, and the kernels' arguments.  smooth: the unknowns are the destination.  0: launch; 1: refused; -1: empty box
template <int N>
static int vec_prepare(const char *who, int mode, bool smooth, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *f,
                       const examg_layout_t *ld, const double *dst, const examg_vec_stencil_t *M, const Box &box, VecArgs<N> &a, int &xo, bool &vec) {
  const int nd = lu->nd;
  const bool need_f = smooth || mode == EXAMG_SYS_RESIDUAL;
  a.lu = make_layout(lu);
  a.lf = need_f ? make_layout(lf) : a.lu;
  a.ld = smooth ? a.lu : make_layout(ld);
  a.cu = a.lu.size;
  a.cf = a.lf.size;
  a.cd = a.ld.size;
  VecStencil<N> &S = a.S;
  S.nent = M->nent;
  S.kmask = S.gmask = 0;
  for (int e = 0; e < N * N; ++e) {
    S.kc[e] = 0.0;
    S.g[e] = nullptr;
    S.same[e] = -1;
  }
  bool centre = false;
  unsigned seen = 0;
  for (int k = 0; k < 7; ++k) {
    S.code[k] = 0;
    S.omask[k] = 0;
    for (int c = 0; c < N; ++c) S.coef[k][c] = 0.0;
  }
  for (int k = 0; k < M->nent; ++k) {
    const examg_vec_entry_t &en = M->ent[k];
    const int code = sys_entry_code(en.off, nd);
    if (code < 0) { set_error("%s: stencil entry %d (%d, %d, %d) is not an axis entry of reach 1 of a %d-D cell field", who, k, en.off[0], en.off[1], en.off[2], nd); return 1; }
    if (seen & (1u << code)) { set_error("%s: stencil entry %d repeats an offset", who, k); return 1; }
    seen |= 1u << code;
    S.code[k] = code;
    for (int c = 0; c < N; ++c)
      for (int d = 0; d < N; ++d) {
        // the caller's table has rows of n = N elements
        const int e = c * N + d;
        const bool hk = (en.kmask >> e) & 1u, hg = en.g[e] != nullptr;
        if (code == 0) {
          if (hk) { S.kmask |= 1u << e; S.kc[e] = en.k[e]; }
          if (hg) { S.gmask |= 1u << e; S.g[e] = en.g[e]; }
        } else {
          if (hg) { set_error("%s: stencil entry %d has a coefficient field at element (%d, %d); fields stand in the centre entry only", who, k, c, d); return 1; }
          if (hk && c != d) { set_error("%s: stencil entry %d has the element (%d, %d) off the diagonal; an off-centre entry is a diagonal matrix", who, k, c, d); return 1; }
          if (hk) { S.omask[k] |= 1u << c; S.coef[k][c] = en.k[e]; }
        }
      }
    if (code == 0) centre = true;
  }
  if (!centre) { set_error("%s: the stencil has no centre entry", who); return 1; }
  a.lg = S.gmask ? make_layout(&M->lg) : a.lu;      // not read without a coefficient field
  for (int e = 0; e < N * N; ++e)
    for (int q = 0; q < e && S.same[e] < 0; ++q)
      if (S.g[e] && S.g[q] == S.g[e]) S.same[e] = S.same[q] >= 0 ? S.same[q] : q;
  if (box.count() == 0) return -1;
  if (!box_inside(lu, box, 1)) { set_error("%s: box + one cell leaves the allocation of the unknowns", who); return 1; }
  if (need_f && !box_inside(lf, box, 0)) { set_error("%s: box leaves the rhs allocation", who); return 1; }
  if (S.gmask && !box_inside(&M->lg, box, 0)) { set_error("%s: box leaves the coefficient allocation", who); return 1; }
  if (!smooth && !box_inside(ld, box, 0)) { set_error("%s: box leaves the dst allocation", who); return 1; }
  if (nd == 2 && (box.b2 != 0 || box.e2 != 1)) { set_error("%s: 2-D box must have [0,1) in dim 2", who); return 1; }
  if (!smooth) {
    if (ranges_overlap(dst, N * a.cd, u, N * a.cu)) { set_error("%s: dst overlaps the unknowns; the operator does not run in place", who); return 1; }
    if (need_f && ranges_overlap(dst, N * a.cd, f, N * a.cf)) { set_error("%s: dst overlaps the right-hand side (the rows are stored one after the other)", who); return 1; }
  }
  a.u = const_cast<double *>(u);
  a.f = need_f ? f : nullptr;
  a.dst = smooth ? nullptr : const_cast<double *>(dst);
  // pairs: xo = the first cell or the one before it, whichever is even in the unknowns' array; 16-byte accesses when every argument and component agrees
  xo = box.b0;
  vec = false;
  const int cand = ((a.lu.origin + box.b0) & 1) ? box.b0 - 1 : box.b0;
  bool ok = !g_vec_narrow;
  for (int c = 0; c < N; ++c) {
    ok = ok && pairs_even(a.lu, nd, u + c * a.cu, cand);
    if (!smooth) {
      if (need_f) ok = ok && pairs_even(a.lf, nd, f + c * a.cf, cand);
      ok = ok && pairs_even(a.ld, nd, dst + c * a.cd, cand);
    }
  }
  if (!smooth)
    for (int e = 0; e < N * N; ++e)
      if (S.g[e]) ok = ok && pairs_even(a.lg, nd, S.g[e], cand);
  if (ok) {
    xo = cand;
    vec = true;
  }
  return 0;
}

static int vec_check_head(const char *who, int n, bool smooth, bool need_f, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *f,
                          const examg_layout_t *ld, const double *dst, const examg_vec_stencil_t *M, const int32_t *begin, const int32_t *end) {
  if (!lu || !u || !M || !begin || !end || (need_f && (!lf || !f)) || (!smooth && (!ld || !dst))) { set_error("%s: null argument", who); return 1; }
  if (!vec_fields_ok(who, n, nullptr, nullptr)) return 1;
  const int nd = lu->nd;
  if (nd != 2 && nd != 3) { set_error("%s: 2-D or 3-D layouts", who); return 1; }
  // lg is looked at only when some element has a coefficient field: a stencil of constants needs none
  bool hasg = false;
  for (int k = 0; k < M->nent && k < 7; ++k)
    for (int e = 0; e < n * n; ++e) hasg = hasg || M->ent[k].g[e] != nullptr;
  if (!sys_layout_ok(who, "unknowns'", lu, nd) || (need_f && !sys_layout_ok(who, "rhs", lf, nd)) || (hasg && !sys_layout_ok(who, "coefficient", &M->lg, nd))) return 1;
  if (!smooth && !sys_layout_ok(who, "dst", ld, nd)) return 1;
  for (int d = 0; d < nd; ++d) {
    if (need_f && lf->inner[d] != lu->inner[d]) { set_error("%s: the rhs layout has %d cells in dim %d, the unknowns %d", who, lf->inner[d], d, lu->inner[d]); return 1; }
    if (hasg && M->lg.inner[d] != lu->inner[d]) { set_error("%s: the coefficient layout has %d cells in dim %d, the unknowns %d", who, M->lg.inner[d], d, lu->inner[d]); return 1; }
    if (!smooth && ld->inner[d] != lu->inner[d]) { set_error("%s: the dst layout has %d cells in dim %d, the unknowns %d", who, ld->inner[d], d, lu->inner[d]); return 1; }
    if (lu->ghost_l[d] < 1 || lu->ghost_r[d] < 1) { set_error("%s: the unknowns need a ghost layer in dim %d", who, d); return 1; }
  }
  if (M->nent < 1 || M->nent > 7) { set_error("%s: nent %d; an axis stencil of reach 1 has 1 to 7 entries", who, M->nent); return 1; }
  return 0;
}

template <int ND, int N>
static int vec_launch(int mode, bool smooth, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *f, const examg_layout_t *ld,
                      const double *dst, const examg_vec_stencil_t *M, double w, int colour, const Box &box, hipStream_t s) {
  const char *who = smooth ? "examg_vec_smooth" : "examg_vec_op";
  VecArgs<N> a;
  int xo;
  bool vec;
  const int rc = vec_prepare<N>(who, mode, smooth, lu, u, lf, f, ld, dst, M, box, a, xo, vec);
  if (rc) return rc < 0 ? 0 : rc;
  const int ntx = (box.e0 - xo + 127) / 128;
  const long long nwg = (long long)ntx * ((box.n1() + 3) / 4) * box.n2();
  if (nwg > 0x7fffffffLL) { set_error("%s: grid too large", who); return 1; }
  const dim3 grid((unsigned)nwg), blk(64, 4);
  if (smooth) {
    if (vec) hipLaunchKernelGGL((k_vec_smooth<ND, N, true>), grid, blk, 0, s, a, w, colour, box, xo, ntx);
    else hipLaunchKernelGGL((k_vec_smooth<ND, N, false>), grid, blk, 0, s, a, w, colour, box, xo, ntx);
    EXAMG_CHECK_LAUNCH("k_vec_smooth");
  } else {
    if (vec) hipLaunchKernelGGL((k_vec_op<ND, N, true>), grid, blk, 0, s, a, mode, box, xo, ntx);
    else hipLaunchKernelGGL((k_vec_op<ND, N, false>), grid, blk, 0, s, a, mode, box, xo, ntx);
    EXAMG_CHECK_LAUNCH("k_vec_op");
  }
  return 0;
}

static int vec_dispatch(int n, int mode, bool smooth, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *f,
                        const examg_layout_t *ld, const double *dst, const examg_vec_stencil_t *M, double w, int colour, const Box &box, hipStream_t s) {
  if (lu->nd == 3)
    return n == 2 ? vec_launch<3, 2>(mode, smooth, lu, u, lf, f, ld, dst, M, w, colour, box, s) : vec_launch<3, 3>(mode, smooth, lu, u, lf, f, ld, dst, M, w, colour, box, s);
  return n == 2 ? vec_launch<2, 2>(mode, smooth, lu, u, lf, f, ld, dst, M, w, colour, box, s) : vec_launch<2, 3>(mode, smooth, lu, u, lf, f, ld, dst, M, w, colour, box, s);
}

}  // namespace examg

using namespace examg;

#ifdef EXAMG_DEBUG_HOOKS
extern "C" int examg_debug_vec_narrow(int on) {
  g_vec_narrow = on;
  return 0;
}
#endif

extern "C" int examg_vec_op(int mode, int n, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *f, const examg_layout_t *ld,
                            double *dst, const examg_vec_stencil_t *M, const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  if (mode != EXAMG_SYS_APPLY && mode != EXAMG_SYS_RESIDUAL) { set_error("examg_vec_op: bad mode %d", mode); return 1; }
  if (vec_check_head("examg_vec_op", n, false, mode == EXAMG_SYS_RESIDUAL, lu, u, lf, f, ld, dst, M, begin, end)) return 1;
  return vec_dispatch(n, mode, false, lu, u, lf, f, ld, dst, M, 0.0, 0, make_box(begin, end), (hipStream_t)stream);
}

extern "C" int examg_vec_smooth(int n, const examg_layout_t *lu, double *u, const examg_layout_t *lf, const double *f, const examg_vec_stencil_t *M,
                                double relax, int colour, const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  if (vec_check_head("examg_vec_smooth", n, true, true, lu, u, lf, f, nullptr, nullptr, M, begin, end)) return 1;
  if (colour != 0 && colour != 1) { set_error("examg_vec_smooth: colour must be 0 or 1"); return 1; }
  return vec_dispatch(n, 0, true, lu, u, lf, f, nullptr, nullptr, M, relax, colour, make_box(begin, end), (hipStream_t)stream);
}
