// Shared helpers of libexamg (gfx950).  Device and host: layouts, boxes, lane exchanges, 16-byte accesses, conv7, point functions.  Host only:
// what the stencil launchers share -- with_mode / with_order, the fills of the kernels' stencil arguments, the argument checks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <cmath>
#include <type_traits>

#include "../../include/examg.h"

namespace examg {

// Flattened layout facts a kernel needs: strides and the offset of iterator (0,0,0).
struct LayoutDev {
  int tot0, tot1, tot2;
  int ref0, ref1, ref2;
  long long s1, s2;    // strides of dim 1, dim 2 (dim 0 stride = 1); under the colour split: strides within a half array
  long long size;      // doubles per (scalar) field
  long long origin;    // linear index of iterator (0,0,0) (plain layouts)
  long long half;      // colour split (EXAMG_LAYOUT_SPLIT_X): doubles per half array, 0 for a plain layout
};

static inline int lay_tot(const examg_layout_t *l, int d) {
  return l->pad_l[d] + l->ghost_l[d] + l->dup_l[d] + l->inner[d] + l->dup_r[d] + l->ghost_r[d] + l->pad_r[d];
}

static inline bool lay_split(const examg_layout_t *l) { return l->transform == EXAMG_LAYOUT_SPLIT_X; }

static inline LayoutDev make_layout(const examg_layout_t *l) {
  LayoutDev d;
  d.tot0 = lay_tot(l, 0);
  d.tot1 = lay_tot(l, 1);
  d.tot2 = lay_tot(l, 2);
  d.ref0 = l->pad_l[0] + l->ghost_l[0];
  d.ref1 = l->pad_l[1] + l->ghost_l[1];
  d.ref2 = l->pad_l[2] + l->ghost_l[2];
  if (lay_split(l)) {
    // [x, y, z] => [x / 2, y, z, x % 2] on array indices (layoutTransformation/ir/IR_LayoutTransformStatement.scala): extents
    // ceil(TOTx / 2), TOTy, TOTz, 2 -- first index fastest
    d.s1 = (d.tot0 + 1) / 2;
    d.s2 = d.s1 * d.tot1;
    d.half = d.s2 * d.tot2;
    d.size = 2 * d.half;
    d.origin = 0;
    return d;
  }
  d.s1 = d.tot0;
  d.s2 = (long long)d.tot0 * d.tot1;
  d.size = d.s2 * d.tot2;
  d.origin = d.ref0 + d.s1 * d.ref1 + d.s2 * d.ref2;
  d.half = 0;
  return d;
}

// the index map of an UNTRANSFORMED layout: what the kernels use whose dispatch takes plain layouts only (the transformation test of lidx
// costs registers in kernels that have none to spare: k_stencilfield27_rec went from two waves per SIMD to one with it)
__host__ __device__ static inline long long lidx_plain(const LayoutDev &l, int i0, int i1, int i2) {
  return l.origin + i0 + l.s1 * i1 + l.s2 * i2;
}

__host__ __device__ static inline long long lidx(const LayoutDev &l, int i0, int i1, int i2) {
  if (l.half) {
    const int ax = i0 + l.ref0;
    return (ax >> 1) + l.s1 * (i1 + l.ref1) + l.s2 * (i2 + l.ref2) + (long long)(ax & 1) * l.half;
  }
  return l.origin + i0 + l.s1 * i1 + l.s2 * i2;
}

// iterator-coordinate box
struct Box {
  int b0, b1, b2, e0, e1, e2;
  __host__ __device__ int n0() const { return e0 - b0; }
  __host__ __device__ int n1() const { return e1 - b1; }
  __host__ __device__ int n2() const { return e2 - b2; }
  __host__ __device__ long long count() const {
    return (n0() <= 0 || n1() <= 0 || n2() <= 0) ? 0 : (long long)n0() * n1() * n2();
  }
  bool operator==(const Box &o) const { return b0 == o.b0 && b1 == o.b1 && b2 == o.b2 && e0 == o.e0 && e1 == o.e1 && e2 == o.e2; }
  bool contains(const Box &o) const { return o.b0 >= b0 && o.b1 >= b1 && o.b2 >= b2 && o.e0 <= e0 && o.e1 <= e1 && o.e2 <= e2; }
};

static inline Box make_box(const int32_t *begin, const int32_t *end) {
  Box b{begin[0], begin[1], begin[2], end[0], end[1], end[2]};
  return b;
}

// [begin,end) grown by `reach` points in the first nd dimensions: a box with its shell of that depth
static inline void grow_box(const int32_t *begin, const int32_t *end, int reach, int nd, int32_t *gbegin, int32_t *gend) {
  for (int d = 0; d < 3; ++d) {
    gbegin[d] = begin[d] - (d < nd ? reach : 0);
    gend[d] = end[d] + (d < nd ? reach : 0);
  }
}

// Does the box (grown by `halo` points, in iterator coords) stay inside the allocation?
static inline bool box_inside(const examg_layout_t *l, const Box &b, int halo) {
  const int bb[3] = {b.b0, b.b1, b.b2}, ee[3] = {b.e0, b.e1, b.e2};
  for (int d = 0; d < 3; ++d) {
    const int ref = l->pad_l[d] + l->ghost_l[d];
    const int h = (d < l->nd) ? halo : 0;
    if (ee[d] <= bb[d]) continue;
    if (bb[d] - h + ref < 0) return false;
    if (ee[d] + h + ref > lay_tot(l, d)) return false;
  }
  return true;
}

void set_error(const char *fmt, ...);
int check_hip(hipError_t e, const char *what);

// What every examg_vec_* entry point asks of its component count and of each layout of a vector-valued cell field (lb may be null):
// n = 2 or 3, no duplicate layers, no layout transformation.  false: error text set.
static inline bool vec_fields_ok(const char *who, int n, const examg_layout_t *la, const examg_layout_t *lb) {
  if (n < 2 || n > EXAMG_VEC_MAX) { set_error("%s: n = %d components; vector-valued fields have 2 or 3", who, n); return false; }
  const examg_layout_t *ls[2] = {la, lb};
  for (int k = 0; k < 2; ++k) {
    const examg_layout_t *l = ls[k];
    if (!l) continue;
    for (int d = 0; d < l->nd && d < 3; ++d)
      if (l->dup_l[d] != 0 || l->dup_r[d] != 0) { set_error("%s: a cell layout has no duplicate layers (dim %d has %d / %d)", who, d, l->dup_l[d], l->dup_r[d]); return false; }
    if (lay_split(l)) { set_error("%s: vector-valued fields under a layout transformation are not supported", who); return false; }
  }
  return true;
}

// Staggered grids (include/examg.h): what every entry point asks of the layout `what` of a staggered field -- a plain layout whose
// duplicate layers are those of its localization: loc = -1 a cell layout (none), else a face layout of axis loc (one per side on the own
// axis, none on the others).  The dimensions of l->nd are looked at (the caller has checked nd).  false: error text set.
static inline bool staggered_layout_ok(const char *who, const char *what, const examg_layout_t *l, int loc) {
  if (lay_split(l)) { set_error("%s: the %s layout is under a layout transformation; staggered fields take plain layouts only", who, what); return false; }
  for (int d = 0; d < l->nd && d < 3; ++d) {
    const int dup = d == loc ? 1 : 0;
    if (l->dup_l[d] == dup && l->dup_r[d] == dup) continue;
    if (loc < 0) set_error("%s: the %s layout is not a cell layout (dim %d has %d / %d duplicate layers)", who, what, d, l->dup_l[d], l->dup_r[d]);
    else set_error("%s: the %s layout is not a face layout of axis %d (dim %d has %d / %d duplicate layers, a face layout has %d)", who, what, loc, d, l->dup_l[d], l->dup_r[d], dup);
    return false;
  }
  return true;
}
// ... of the one layout of an entry point that takes the axis of a face field (kernels_mac.hip, kernels_blas.hip)
static inline bool face_layout_ok(const char *who, const char *what, int axis, const examg_layout_t *l) {
  if (l->nd != 2 && l->nd != 3) { set_error("%s: 2-D or 3-D layouts", who); return false; }
  if (axis < 0 || axis >= l->nd) { set_error("%s: axis %d of a %d-D face field", who, axis, l->nd); return false; }
  return staggered_layout_ok(who, what, l, axis);
}

// one-pass kernels of the launch-bound levels (kernels_small.hip), tried by the entry points when the large-level kernels decline
bool small_two_stage_ok(const examg_layout_t *lu, const examg_layout_t *lf, const examg_stencil_t *st, const Box &box);
int launch_small_two_stage(bool col, int var, const examg_layout_t *lu, const double *u_in, double *u_out, const examg_layout_t *lf, const double *rhs,
                      const examg_stencil_t *st, double w, int first, const Box &box, const examg_layout_t *lc, const double *uc, hipStream_t s);
bool small_residual_restrict_ok(const examg_layout_t *lu, const examg_layout_t *lf, const examg_stencil_t *st, const examg_layout_t *lc, const Box &fb,
                                const Box &cb);
int launch_small_residual_restrict(const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs, const examg_layout_t *lc,
                                   double *fc, const examg_stencil_t *st, double scale, const Box &cb, hipStream_t s);

// examg_stencil_op (kernels_stencil.hip) with one more argument, passthru: a coloured loop out of place carries the other colour over (examg_comm.hip)
int stencil_loop(int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs, const examg_layout_t *ld, double *dst,
                 const examg_stencil_t *st, double w, int colour, const int32_t *begin, const int32_t *end, bool passthru, hipStream_t s);

#define EXAMG_CHECK_LAUNCH(name)                                   \
  do {                                                             \
    hipError_t _e = hipGetLastError();                             \
    if (_e != hipSuccess) return examg::check_hip(_e, name);       \
  } while (0)

// Wavefront-level halo exchange: value of the neighbouring lane through DPP wave shifts (one v_mov_b32_dpp per
// dword, no LDS crossbar round trip as with ds_bpermute / __shfl).  Lane 0 (resp. 63) keeps its own value.
__device__ __forceinline__ double lane_below(double v) {   // lane l receives lane l-1
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xF, 0xF, false);   // wave_shr:1
  hi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_above(double v) {   // lane l receives lane l+1
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, 0x130, 0xF, 0xF, false);   // wave_shl:1
  hi = __builtin_amdgcn_update_dpp(hi, hi, 0x130, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

// The same shifts where the end lane's result is never used: it receives 0 (bound_ctrl) instead of its own value, which
// saves the copy that ties the old value to the destination (one v_mov_b32 per dword).
__device__ __forceinline__ double lane_below0(double v) {   // lane l receives lane l-1, lane 0 receives 0.0
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, 0x138, 0xF, 0xF, true);
  hi = __builtin_amdgcn_mov_dpp(hi, 0x138, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_above0(double v) {   // lane l receives lane l+1, lane 63 receives 0.0
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, 0x130, 0xF, 0xF, true);
  hi = __builtin_amdgcn_mov_dpp(hi, 0x130, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// XCD bands: workgroups are dealt round-robin to the 8 XCDs; within a z layer every XCD takes a band of consecutive workgroups
// (x tiles fastest, then coarse rows), so the cache lines that x-adjacent tiles share meet in one L2 (kernels_transfer.hip:
// k_restrict3_wide).  Shared by the cell transfer kernels (kernels_cell.hip) and the system kernels (kernels_system.hip).
__device__ __forceinline__ long long xcd_band(long long wg, int wpl) {
  if ((wpl & 7) == 0) {
    const int per = wpl >> 3;
    const long long lz = wg / wpl;
    const int r = (int)(wg - lz * wpl);
    return lz * wpl + (r & 7) * per + (r >> 3);
  }
  return wg;
}

// ---- shared by the 7-point kernels (kernels_stencil.hip, kernels_twostage.hip, kernels_stencilfield.hip) ----------
typedef double d2 __attribute__((ext_vector_type(2)));
struct __attribute__((packed, aligned(8))) d2u { double a, b; };  // 16-byte access at 8-byte alignment

__device__ __forceinline__ d2 load2(const double *p) {
  const d2u v = *reinterpret_cast<const d2u *>(p);
  d2 r;
  r.x = v.a;
  r.y = v.b;
  return r;
}
__device__ __forceinline__ void store2(double *p, d2 v) {
  d2u s;
  s.a = v.x;
  s.b = v.y;
  *reinterpret_cast<d2u *>(p) = s;
}
// non-temporal 16-byte store at 8-byte alignment (global_store_dwordx4 ... nt)
typedef d2 d2_a8 __attribute__((aligned(8)));
__device__ __forceinline__ void store2_nt(double *p, d2 v) { __builtin_nontemporal_store(v, (d2_a8 *)p); }
// 16-byte load where both points may be read, scalar loads at the edges of an allocation / box, 0 outside
__device__ __forceinline__ d2 load2g(const double *p, bool oka, bool okb) {
  d2 r = {0.0, 0.0};
  if (oka && okb) return load2(p);
  if (oka) r.x = p[0];
  else if (okb) r.y = p[1];
  return r;
}

struct Coef7 {
  double c[7];
};

// sum_k c_k * u[i + o_k] folded left to right in entry order
// (Compiler/src/exastencils/stencil/ir/IR_StencilConvolution.scala:65-68).
// ORDER 0: entries c,-x,+x,-y,+y,-z,+z (Benchmark/Poisson3D/3D_FD_Poisson_fromL4.exa4:39-47)
// ORDER 1: entries c,+x,-x,+y,-y,+z,-z (Testing/Smoothers/Jac.exa4:55-63)
// FMA: entries 1..6 as fused multiply-adds, for launches whose six off-centre coefficients are +-2^e, e >= 0 (pow2_offdiag7): such a
// product is exact for every double that it does not overflow, so acc + c*x and fma(c, x, acc) round the same real number once -- the
// same bits (the build keeps -ffp-contract=off: the fusion is this explicit one only).
template <int ORDER, bool FMA = false>
__device__ __forceinline__ double conv7(const Coef7 &k, double c, double xm, double xp, double ym, double yp, double zm,
                                        double zp) {
  double acc = k.c[0] * c;
  if (FMA) {
    acc = __builtin_fma(k.c[1], ORDER == 0 ? xm : xp, acc);
    acc = __builtin_fma(k.c[2], ORDER == 0 ? xp : xm, acc);
    acc = __builtin_fma(k.c[3], ORDER == 0 ? ym : yp, acc);
    acc = __builtin_fma(k.c[4], ORDER == 0 ? yp : ym, acc);
    acc = __builtin_fma(k.c[5], ORDER == 0 ? zm : zp, acc);
    acc = __builtin_fma(k.c[6], ORDER == 0 ? zp : zm, acc);
  } else if (ORDER == 0) {
    acc = acc + k.c[1] * xm;
    acc = acc + k.c[2] * xp;
    acc = acc + k.c[3] * ym;
    acc = acc + k.c[4] * yp;
    acc = acc + k.c[5] * zm;
    acc = acc + k.c[6] * zp;
  } else {
    acc = acc + k.c[1] * xp;
    acc = acc + k.c[2] * xm;
    acc = acc + k.c[3] * yp;
    acc = acc + k.c[4] * ym;
    acc = acc + k.c[5] * zp;
    acc = acc + k.c[6] * zm;
  }
  return acc;
}

// Which canonical 7-point entry order do the entries of a stencil (constant or field) have?  -1: none of the two.
static inline int star7_order(const examg_stencil_t *st) {
  static const int o0[7][3] = {{0, 0, 0}, {-1, 0, 0}, {1, 0, 0}, {0, -1, 0}, {0, 1, 0}, {0, 0, -1}, {0, 0, 1}};
  static const int o1[7][3] = {{0, 0, 0}, {1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
  if (st->nent != 7) return -1;
  bool m0 = true, m1 = true;
  for (int k = 0; k < 7; ++k)
    for (int d = 0; d < 3; ++d) {
      m0 = m0 && st->off[k][d] == o0[k][d];
      m1 = m1 && st->off[k][d] == o1[k][d];
    }
  return m0 ? 0 : (m1 ? 1 : -1);
}
static inline int canonical_order7(const examg_stencil_t *st) { return st->cfield ? -1 : star7_order(st); }   // ... and a constant stencil

// ... whose six off-centre coefficients are all +-2^e with e >= 0 (finite, not zero: frexp mantissa +-0.5, exponent >= 1)?  Then conv7<.., FMA>
// gives conv7's bits.  All six or none: one kernel template flag.  (1/h^2 of every power-of-two grid, laplace_unit's -1.0)
static inline bool pow2_offdiag7(const examg_stencil_t *st) {
  if (canonical_order7(st) < 0) return false;
  for (int k = 1; k < 7; ++k) {
    const double c = st->coef[k];
    int e = 0;
    if (!std::isfinite(c) || c == 0.0 || std::fabs(std::frexp(c, &e)) != 0.5 || e < 1) return false;
  }
  return true;
}

// 27-entry stencil field, the centre entry first and the diagonal (the unrolled kernels read both from entry 0); callers add their own conditions
static inline bool stencil_field27(const examg_stencil_t *st) {
  return st->cfield && st->nent == 27 && st->diag == 0 && st->off[0][0] == 0 && st->off[0][1] == 0 && st->off[0][2] == 0;
}

static inline int stencil_reach(const examg_stencil_t *st) {
  int reach = 0;
  for (int k = 0; k < st->nent; ++k)
    for (int d = 0; d < 3; ++d) {
      const int a = st->off[k][d] < 0 ? -st->off[k][d] : st->off[k][d];
      reach = reach > a ? reach : a;
    }
  return reach;
}

// ---- host side of the stencil launchers: f(std::integral_constant<int, V>{}), V the loop kind / canonical entry order of a call (kernel template arguments)
template <class F>
static inline void with_mode(int mode, F &&f) {
  if (mode == EXAMG_APPLY) f(std::integral_constant<int, EXAMG_APPLY>{});
  else if (mode == EXAMG_RESIDUAL) f(std::integral_constant<int, EXAMG_RESIDUAL>{});
  else f(std::integral_constant<int, EXAMG_SMOOTH>{});
}
template <class F>
static inline void with_order(int ord, F &&f) {
  if (ord == 0) f(std::integral_constant<int, 0>{});
  else f(std::integral_constant<int, 1>{});
}
static inline Coef7 make_coef7(const examg_stencil_t *st) {
  return Coef7{{st->coef[0], st->coef[1], st->coef[2], st->coef[3], st->coef[4], st->coef[5], st->coef[6]}};
}
// linear offsets of the entries in a plain u layout (0 behind the last entry)
template <int N>
static inline void fill_u_offsets(long long (&uo)[N], const examg_stencil_t *st, const LayoutDev &lu) {
  for (int k = 0; k < N; ++k) uo[k] = k < st->nent ? st->off[k][0] + lu.s1 * st->off[k][1] + lu.s2 * st->off[k][2] : 0;
}

// What StencilDev (kernels_stencil.hip), MCStencil (kernels_multicolour.hip) and StencilCG (kernels_coarse.hip) share: entries, offsets in u,
// coefficients, the strides of a coefficient field (cplane between entries, cpt between points; 1 and nent under the entry-fastest
// transformation).  Returns the coefficient layout (lu for a constant stencil, where no kernel uses it).
template <class SD>
static inline LayoutDev fill_stencil_dev(SD &sd, const examg_stencil_t *st, const LayoutDev &lu) {
  sd.nent = st->nent;
  sd.diag = st->diag;
  fill_u_offsets(sd.uo, st, lu);
  for (int k = 0; k < EXAMG_MAX_ENTRIES; ++k) sd.coef[k] = k < st->nent ? st->coef[k] : 0.0;
  sd.cfield = st->cfield;
  const LayoutDev lc = st->cfield ? make_layout(&st->clayout) : lu;
  const bool records = st->cfield && st->ctransform == EXAMG_CLAYOUT_ENTRY_FASTEST;
  sd.cplane = !st->cfield ? 0 : (records ? 1 : lc.size);
  sd.cpt = records ? st->nent : 1;
  return lc;
}

// The argument checks of examg_stencil_op, examg_stencil_op_coloured and examg_mcgs_sweep, in two parts: each entry point has checks of
// its own between them; false: error text set
static inline bool check_stencil_args(const char *who, int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs,
                                      const examg_layout_t *ld, const double *dst, const examg_stencil_t *st, const int32_t *begin, const int32_t *end) {
  if (!lu || !u || !ld || !dst || !st || !begin || !end) { set_error("%s: null argument", who); return false; }
  if (mode < 0 || mode > 2) { set_error("%s: bad mode %d", who, mode); return false; }
  if (mode != EXAMG_APPLY && (!rhs || !lf)) { set_error("%s: rhs required for mode %d", who, mode); return false; }
  if (st->nent < 1 || st->nent > EXAMG_MAX_ENTRIES) { set_error("%s: nent %d out of range", who, st->nent); return false; }
  return true;
}
// ... the box (not empty) against the u, dst, rhs and coefficient allocations
static inline bool check_stencil_box(const char *who, int mode, const examg_layout_t *lu, const examg_layout_t *lf, const examg_layout_t *ld,
                                     const examg_stencil_t *st, const Box &box) {
  if (!box_inside(lu, box, stencil_reach(st))) { set_error("%s: box + stencil reach leaves the u allocation", who); return false; }
  if (!box_inside(ld, box, 0)) { set_error("%s: box leaves the dst allocation", who); return false; }
  if (mode != EXAMG_APPLY && !box_inside(lf, box, 0)) { set_error("%s: box leaves the rhs allocation", who); return false; }
  if (st->cfield && !box_inside(&st->clayout, box, 0)) { set_error("%s: box leaves the coefficient allocation", who); return false; }
  return true;
}

// ---- colourings (include/examg.h: examg_colouring_t), shared by the multi-colour stencil loops (kernels_multicolour.hip) and the
// collective smoother of the block systems (kernels_blocksys.hip) ----------------------------------------------------------------------
struct MCColour {
  int nexpr;
  int axes[3], shift[3], mod[3], rem[3];
  int first[3], step[3], count[3];  // lattice per axis: i_d = first[d] + step[d] * j, j < count[d] (step 1: every point of the box)
  int rowk;                         // expression that sets the start and the stride of a row (its axes include x), or -1
  int row_w;                        // threads per row
};

__device__ __forceinline__ bool mc_member(const MCColour &c, int i0, int i1, int i2) {
  bool ok = true;
  for (int k = 0; k < c.nexpr; ++k) {
    const int s = c.shift[k] + ((c.axes[k] & 1) ? i0 : 0) + ((c.axes[k] & 2) ? i1 : 0) + ((c.axes[k] & 4) ? i2 : 0);
    ok = ok && (s % c.mod[k] == c.rem[k]);      // s >= 0 on the whole box (host check)
  }
  return ok;
}

// Thread t of mc_threads(col) -> its point of the colour in the box; false: the thread has none.  Expressions on a single axis are
// iterated as a lattice, one expression over several axes that include x becomes a start and a stride per row, whatever is left is a
// predicate: every expression is evaluated again on the point the lattice arrives at.  In two steps -- lattice row `row` of
// mc_rows(col) -> (i1, i2), then place c0 < col.row_w of that row -> i0 -- for kernels that give a lane several rows.
__device__ __forceinline__ void mc_row(const MCColour &col, long long row, int &i1, int &i2) {
  i1 = col.first[1] + col.step[1] * (int)(row % col.count[1]);
  i2 = col.first[2] + col.step[2] * (int)(row / col.count[1]);
}
__device__ __forceinline__ bool mc_place(const MCColour &col, const Box &box, int c0, int i1, int i2, int &i0) {
  if (col.rowk >= 0) {
    // (shift + i0 + the other summands) % n == rem: the first such i0 >= box.b0, then every n-th
    const int k = col.rowk, n = col.mod[k];
    const int s = col.shift[k] + box.b0 + ((col.axes[k] & 2) ? i1 : 0) + ((col.axes[k] & 4) ? i2 : 0);
    i0 = box.b0 + (col.rem[k] - s % n + n) % n + n * c0;
  } else {
    i0 = col.first[0] + col.step[0] * c0;
  }
  return i0 < box.e0 && mc_member(col, i0, i1, i2);
}
__device__ __forceinline__ bool mc_point(const MCColour &col, const Box &box, long long t, int &i0, int &i1, int &i2) {
  const long long row = t / col.row_w;
  mc_row(col, row, i1, i2);
  return mc_place(col, box, (int)(t - row * col.row_w), i1, i2, i0);
}
__host__ __device__ static inline long long mc_rows(const MCColour &c) { return (long long)c.count[1] * c.count[2]; }
__host__ __device__ static inline long long mc_threads(const MCColour &c) { return (long long)c.row_w * c.count[1] * c.count[2]; }

static inline const char *check_colouring(const examg_colouring_t *col, int nd, bool with_rem) {
  if (col->nexpr < 1 || col->nexpr > 3) return "nexpr must be 1, 2 or 3";
  for (int k = 0; k < col->nexpr; ++k) {
    if (col->mod[k] <= 0) return "mod must be positive";
    if (col->axes[k] <= 0 || col->axes[k] >= (1 << nd)) return "axes must name a non-empty set of the layout's axes";
    if (with_rem && (col->rem[k] < 0 || col->rem[k] >= col->mod[k])) return "rem must lie in [0, mod)";
  }
  return nullptr;
}

static inline bool starts_nonnegative(const examg_colouring_t *col, const int32_t *begin) {
  for (int k = 0; k < col->nexpr; ++k) {
    long long s = col->shift[k];
    for (int d = 0; d < 3; ++d)
      if (col->axes[k] & (1 << d)) s += begin[d];
    if (s < 0) return false;
  }
  return true;
}

// does some expression of the colouring change over the offset o?  (A colouring decouples a stencil when this holds for every entry off the centre.)
static inline bool colouring_separates(const examg_colouring_t *col, const int32_t *o) {
  for (int k = 0; k < col->nexpr; ++k) {
    int s = 0;
    for (int d = 0; d < 3; ++d)
      if (col->axes[k] & (1 << d)) s += o[d];
    if (s % col->mod[k] != 0) return true;
  }
  return false;
}

// the colour `col` on the box as the kernels iterate it (the colouring has passed check_colouring and starts_nonnegative)
static inline MCColour make_colour(const examg_colouring_t *col, const Box &box) {
  MCColour c;
  c.nexpr = col->nexpr;
  for (int k = 0; k < 3; ++k) {
    const bool on = k < col->nexpr;
    c.axes[k] = on ? col->axes[k] : 0;
    c.shift[k] = on ? col->shift[k] : 0;
    c.mod[k] = on ? col->mod[k] : 1;
    c.rem[k] = on ? col->rem[k] : 0;
  }
  const int bb[3] = {box.b0, box.b1, box.b2}, ee[3] = {box.e0, box.e1, box.e2};
  for (int d = 0; d < 3; ++d) {
    c.first[d] = bb[d];
    c.step[d] = 1;
    for (int k = 0; k < col->nexpr; ++k)
      if (col->axes[k] == (1 << d) && c.step[d] == 1 && col->mod[k] > 1) {      // the first single-axis expression of the axis
        const int n = col->mod[k];
        c.step[d] = n;
        c.first[d] = bb[d] + (col->rem[k] - (col->shift[k] + bb[d]) % n + n) % n;
      }
    c.count[d] = c.first[d] < ee[d] ? (ee[d] - c.first[d] + c.step[d] - 1) / c.step[d] : 0;
  }
  c.rowk = -1;
  c.row_w = c.count[0];
  if (c.step[0] == 1)
    for (int k = 0; k < col->nexpr && c.rowk < 0; ++k)
      if ((col->axes[k] & 1) && col->axes[k] != 1 && col->mod[k] > 1) {
        c.rowk = k;
        c.row_w = (box.n0() + col->mod[k] - 1) / col->mod[k];
      }
  return c;
}

struct Params4 {
  double v[4];
};
struct Geom {
  double pb0, pb1, pb2, h0, h1, h2;
};
static inline Geom make_geom(const examg_geom_t *g) {
  return Geom{g->pos_begin[0], g->pos_begin[1], g->pos_begin[2], g->h[0], g->h[1], g->h[2]};
}
// Evaluation point of iterator index (i0, i1, i2): the node position index * h + pos_begin, or the cell centre
// (index * h + pos_begin) + 0.5 * h (grid/ir/IR_VF_CellCenter.scala:97-100).  LOC: 0 the node, 1 the cell centre, 2 + a the centre of the
// face normal to axis a -- the node position on axis a, the cell centre on the other axes.
template <int LOC>
__host__ __device__ __forceinline__ void point_position(const Geom &g, int i0, int i1, int i2, double &x, double &y, double &z) {
  x = i0 * g.h0 + g.pb0;
  y = i1 * g.h1 + g.pb1;
  z = i2 * g.h2 + g.pb2;
  if (LOC != 0 && LOC != 2) x = x + 0.5 * g.h0;
  if (LOC != 0 && LOC != 3) y = y + 0.5 * g.h1;
  if (LOC != 0 && LOC != 4) z = z + 0.5 * g.h2;
}

// A point function: a postfix program (include/examg.h), evaluated in the order of the expression tree.  W: the program may read the
// widths of the point's cell (EXAMG_OP_WX/WY/WZ: the _grid entry points); without W they are unknown opcodes like any other.
template <bool W>
__device__ __forceinline__ double expr_eval(const examg_expr_t &e, double x, double y, double z, double wx, double wy, double wz) {
  double st[24];
  int sp = 0;
  for (int i = 0; i < e.n; ++i) {
    switch (e.op[i]) {
      case EXAMG_OP_CONST: st[sp++] = e.c[i]; break;
      case EXAMG_OP_X: st[sp++] = x; break;
      case EXAMG_OP_Y: st[sp++] = y; break;
      case EXAMG_OP_Z: st[sp++] = z; break;
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
      default:
        if (W && e.op[i] >= EXAMG_OP_WX && e.op[i] <= EXAMG_OP_WZ) st[sp++] = e.op[i] == EXAMG_OP_WX ? wx : (e.op[i] == EXAMG_OP_WY ? wy : wz);
        else st[sp++] = __builtin_nan("");
        break;
    }
  }
  return st[0];
}
struct ExprEval {
  examg_expr_t e;
  __device__ double operator()(double x, double y, double z) const { return expr_eval<false>(e, x, y, z, 0.0, 0.0, 0.0); }
};
// ... over the node tables of an axis-aligned grid (examg_grid_t): positions and the widths of the point's cell
struct ExprEvalGrid {
  examg_expr_t e;
  __device__ double operator()(double x, double y, double z, double wx, double wy, double wz) const { return expr_eval<true>(e, x, y, z, wx, wy, wz); }
};
struct GridGeom {
  const double *n0, *n1, *n2;   // node tables; element j is node j - ghost; null for an axis the layout does not have
  int ghost;
};
static inline GridGeom make_geom(const examg_grid_t *g) { return GridGeom{g->nodes[0], g->nodes[1], g->nodes[2], g->ghost}; }

// The value of a point function at iterator index (i0, i1, i2): the ONE place where the point-expression kernels (kernels_blas.hip)
// turn an index into a position -- the uniform formula, or the tables (position x[i], width x[i + 1] - x[i]; 0.0 on an axis without table)
template <int CELL, class F>
__device__ __forceinline__ double eval_point(const Geom &g, const F &fn, int i0, int i1, int i2) {
  double px, py, pz;
  point_position<CELL>(g, i0, i1, i2, px, py, pz);
  return fn(px, py, pz);
}
template <int CELL, class F>
__device__ __forceinline__ double eval_point(const GridGeom &g, const F &fn, int i0, int i1, int i2) {
  double p[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
  if (g.n0) { p[0] = g.n0[i0 + g.ghost]; w[0] = g.n0[i0 + g.ghost + 1] - p[0]; }
  if (g.n1) { p[1] = g.n1[i1 + g.ghost]; w[1] = g.n1[i1 + g.ghost + 1] - p[1]; }
  if (g.n2) { p[2] = g.n2[i2 + g.ghost]; w[2] = g.n2[i2 + g.ghost + 1] - p[2]; }
  return fn(p[0], p[1], p[2], w[0], w[1], w[2]);
}

// host check of an expression program's stack discipline (kernels_blas.hip); sets the error text when it fails
bool expr_ok(const examg_expr_t *e);

static inline Params4 make_params(const double *p) {
  Params4 q{{0, 0, 0, 0}};
  if (p) for (int i = 0; i < 4; ++i) q.v[i] = p[i];
  return q;
}

}  // namespace examg
