// Complex-valued node fields (gfx950): constant-stencil loops, the BiCGStab vector updates, the unconjugated dot product, the node transfer
// operators, the absorbing-boundary assignment and the assembly of a complex field from real parts.
//
// Reference: std::complex<double> per point (base/ir/IR_Datatype.scala:191-201), Examples/Helmholtz/2D_FD_Helmholtz_fromL3.  A point is
// (re, im) in two consecutive doubles, 16-byte aligned: one global_load_dwordx4 / global_store_dwordx4 per lane and point, the widest
// coalesced access of the chip.  The arithmetic on the parts is written out in include/examg.h; every kernel here evaluates exactly that, so
// the two stencil kernels give the same bits: they share cfold (the entries in declared order) and cfinish (the loop kind).
#include "examg_common.h"

namespace examg {

typedef d2 cplx;   // .x = re, .y = im

__device__ __forceinline__ cplx cload(const double *p, long long pt) { return *reinterpret_cast<const d2 *>(p + 2 * pt); }
__device__ __forceinline__ void cstore(double *p, long long pt, cplx v) { *reinterpret_cast<d2 *>(p + 2 * pt) = v; }
__device__ __forceinline__ cplx cmake(double re, double im) {
  cplx r;
  r.x = re;
  r.y = im;
  return r;
}
// c . v; the coefficient is wave-uniform: a scalar branch
__device__ __forceinline__ cplx cmul(double a, double b, cplx v) {
  if (b == 0.0) return cmake(a * v.x, a * v.y);
  return cmake(a * v.x - b * v.y, a * v.y + b * v.x);
}
__device__ __forceinline__ cplx cdiv(cplx z, double cr, double ci) {
  if (ci == 0.0) return cmake(z.x / cr, z.y / cr);
  const double den = cr * cr + ci * ci;
  return cmake((z.x * cr + z.y * ci) / den, (z.y * cr - z.x * ci) / den);
}
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return cmake(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return cmake(a.x - b.x, a.y - b.y); }

// which register of the marching kernel holds the point of an entry
enum { SEL_C = 0, SEL_XM = 1, SEL_XP = 2, SEL_YM = 3, SEL_YP = 4, SEL_ZM = 5, SEL_ZP = 6 };

struct CStencilDev {
  int nent, diag;
  long long uo[EXAMG_MAX_ENTRIES];   // offsets in u, in points
  double cr[EXAMG_MAX_ENTRIES], ci[EXAMG_MAX_ENTRIES];
  int sel[EXAMG_MAX_ENTRIES];        // SEL_* of the entry (star stencils)
};

// The entries folded left to right in declared order; OFF: the centre entry skipped (EXAMG_CRELAX; (0, 0) where nothing is left).  N: the
// entry count where it is a compile-time constant (unrolled: get(k) selects among registers), 0: st.nent.
template <int N, bool OFF, class GET>
__device__ __forceinline__ cplx cfold(const CStencilDev &st, GET get) {
  const int n = N ? N : st.nent;
  cplx acc = cmake(0.0, 0.0);
  bool first = true;
#pragma unroll
  for (int k = 0; k < n; ++k) {
    if (OFF && k == st.diag) continue;
    const cplx t = cmul(st.cr[k], st.ci[k], get(k));
    acc = first ? t : cadd(acc, t);
    first = false;
  }
  return acc;
}

template <int MODE>
__device__ __forceinline__ cplx cfinish(const CStencilDev &st, cplx acc, cplx uc, cplx f, double wr, double wi) {
  if (MODE == EXAMG_APPLY) return acc;
  if (MODE == EXAMG_RESIDUAL) return csub(f, acc);
  if (MODE == EXAMG_SMOOTH) return cadd(uc, cmul(wr, wi, csub(f, acc)));
  const cplx x = cdiv(csub(f, acc), st.cr[st.diag], st.ci[st.diag]);
  if (wr == 1.0) return x;
  const double om = 1.0 - wr;
  return cmake(uc.x * om + wr * x.x, uc.y * om + wr * x.y);
}

// ---- gather: one lane per point (of the colour), every entry from memory ------------------------------------------------------------------
template <int MODE>
__global__ void __launch_bounds__(256)
k_cstencil_gather(LayoutDev lu, const double *u, LayoutDev lf, const double *rhs, LayoutDev ld, double *dst, CStencilDev st, double wr, double wi,
                  int colour, Box box, int row_w) {
  const long long total = (long long)box.n1() * box.n2() * row_w;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long row = t / row_w;
    const int c0 = (int)(t - row * row_w);
    const int i1 = box.b1 + (int)(row % box.n1());
    const int i2 = box.b2 + (int)(row / box.n1());
    const int i0 = colour >= 0 ? box.b0 + (((box.b0 + i1 + i2) & 1) != colour ? 1 : 0) + 2 * c0 : box.b0 + c0;
    if (i0 >= box.e0) continue;
    const long long iu = lidx_plain(lu, i0, i1, i2);
    auto get = [&](int k) { return cload(u, iu + st.uo[k]); };
    const cplx acc = cfold<0, MODE == EXAMG_CRELAX>(st, get);
    const cplx uc = (MODE == EXAMG_SMOOTH || MODE == EXAMG_CRELAX) ? cload(u, iu) : cmake(0.0, 0.0);
    const cplx f = MODE != EXAMG_APPLY ? cload(rhs, lidx_plain(lf, i0, i1, i2)) : cmake(0.0, 0.0);
    cstore(dst, lidx_plain(ld, i0, i1, i2), cfinish<MODE>(st, acc, uc, f, wr, wi));
  }
}

// ---- march: star stencils of reach 1 ---------------------------------------------------------------------------------------------------------
// A wave owns 64 consecutive points of a row (a window) and a run of rows (ND == 2, marching in y) or of planes of one row (ND == 3, marching
// in z).  Lane l holds its point of the rows m - 1, m, m + 1 in registers (cm, c, cn) and loads one new point per step; x neighbours are the
// adjacent lanes' c through wave shifts, the first lane and the last lane with a point read theirs from memory.  ND == 3: the y neighbours
// are read from memory (their rows are marched by other waves; L2 serves them).
// In place on one colour (dst == u): a point's neighbours have the other colour and are never written by this launch, its own value is
// in c before the lane stores it -- whatever other waves have or have not stored yet, no value that is used differs from the old field.
struct CMarchGeom {
  int ntx;        // windows per row
  int chunk;      // rows (planes) per wave
  long long nwaves;
};
constexpr int CM_WY = 4;   // waves per workgroup

template <int MODE, int ND>
__global__ void __launch_bounds__(64 * CM_WY)
k_cstencil_march(LayoutDev lu, const double *u, LayoutDev lf, const double *rhs, LayoutDev ld, double *dst, CStencilDev st, double wr, double wi,
                 int colour, Box box, CMarchGeom g) {
  const long long wid = (long long)blockIdx.x * CM_WY + threadIdx.y;
  if (wid >= g.nwaves) return;      // wave-uniform
  const int lane = threadIdx.x;
  const int tx = (int)(wid % g.ntx);
  const long long r = wid / g.ntx;
  int i1 = 0, mb;
  if (ND == 2) {
    mb = box.b1 + (int)r * g.chunk;
  } else {
    i1 = box.b1 + (int)(r % box.n1());
    mb = box.b2 + (int)(r / box.n1()) * g.chunk;
  }
  const int mend = ND == 2 ? box.e1 : box.e2;
  const int me = mb + g.chunk < mend ? mb + g.chunk : mend;
  const int i0 = box.b0 + tx * 64 + lane;
  const bool act = i0 < box.e0;
  const bool last = act && (lane == 63 || i0 + 1 >= box.e0);
  const long long sm = ND == 2 ? lu.s1 : lu.s2, fm = ND == 2 ? lf.s1 : lf.s2, dm = ND == 2 ? ld.s1 : ld.s2;
  long long pu = ND == 2 ? lidx_plain(lu, i0, mb, box.b2) : lidx_plain(lu, i0, i1, mb);
  long long pf = ND == 2 ? lidx_plain(lf, i0, mb, box.b2) : lidx_plain(lf, i0, i1, mb);
  long long pd = ND == 2 ? lidx_plain(ld, i0, mb, box.b2) : lidx_plain(ld, i0, i1, mb);
  const cplx zero = cmake(0.0, 0.0);
  cplx cm = act ? cload(u, pu - sm) : zero;
  cplx c = act ? cload(u, pu) : zero;
  const int par0 = ND == 2 ? i0 + box.b2 : i0 + i1;
  for (int m = mb; m < me; ++m, pu += sm, pf += fm, pd += dm) {
    const cplx cn = act ? cload(u, pu + sm) : zero;
    cplx xm = cmake(lane_below0(c.x), lane_below0(c.y));
    cplx xp = cmake(lane_above0(c.x), lane_above0(c.y));
    if (act && lane == 0) xm = cload(u, pu - 1);
    if (last) xp = cload(u, pu + 1);
    if (act && (colour < 0 || ((par0 + m) & 1) == colour)) {
      cplx ym = cm, yp = cn;
      if (ND == 3) {
        ym = cload(u, pu - lu.s1);
        yp = cload(u, pu + lu.s1);
      }
      auto get = [&](int k) {
        switch (st.sel[k]) {
          case SEL_XM: return xm;
          case SEL_XP: return xp;
          case SEL_YM: return ym;
          case SEL_YP: return yp;
          case SEL_ZM: return cm;
          case SEL_ZP: return cn;
          default: return c;
        }
      };
      const cplx acc = cfold<2 * ND + 1, MODE == EXAMG_CRELAX>(st, get);
      const cplx f = MODE != EXAMG_APPLY ? cload(rhs, pf) : zero;
      cstore(dst, pd, cfinish<MODE>(st, acc, c, f, wr, wi));
    }
    cm = c;
    c = cn;
  }
}

// ---- vector updates ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void unflatten_box(const Box &box, long long t, int &i0, int &i1, int &i2) {
  const int n0 = box.n0(), n1 = box.n1();
  i0 = box.b0 + (int)(t % n0);
  const long long row = t / n0;
  i1 = box.b1 + (int)(row % n1);
  i2 = box.b2 + (int)(row / n1);
}

template <int FORM>
__global__ void __launch_bounds__(256)
k_clincomb(LayoutDev lx, const double *x, LayoutDev ly, const double *y, LayoutDev lz, const double *z, LayoutDev ld, double *dst, double ar, double ai,
           double br, double bi, Box box) {
  const long long total = box.count();
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    int i0, i1, i2;
    unflatten_box(box, t, i0, i1, i2);
    const cplx xv = cload(x, lidx_plain(lx, i0, i1, i2)), yv = cload(y, lidx_plain(ly, i0, i1, i2));
    cplx r;
    if (FORM == EXAMG_C_XPAY) r = cadd(xv, cmul(ar, ai, yv));
    else if (FORM == EXAMG_C_XMAY) r = csub(xv, cmul(ar, ai, yv));
    else r = cadd(xv, cmul(ar, ai, csub(yv, cmul(br, bi, cload(z, lidx_plain(lz, i0, i1, i2))))));
    cstore(dst, lidx_plain(ld, i0, i1, i2), r);
  }
}

// ---- unconjugated dot product: two sums on one fixed tree (lane -> wave -> workgroup -> one workgroup) ------------------------------------------
constexpr int CRED_BLOCK = 256;
constexpr int CRED_MAX_BLOCKS = 2048;

__device__ __forceinline__ double cwave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o);
  return v;
}
// the sums of the workgroup, valid in thread 0
__device__ __forceinline__ cplx cblock_sum(cplx v) {
  __shared__ double sm[2][CRED_BLOCK / 64];
  v.x = cwave_sum(v.x);
  v.y = cwave_sum(v.y);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    sm[0][wv] = v.x;
    sm[1][wv] = v.y;
  }
  __syncthreads();
  cplx r = cmake(0.0, 0.0);
  if (threadIdx.x == 0) {
    r = cmake(sm[0][0], sm[1][0]);
    for (int i = 1; i < CRED_BLOCK / 64; ++i) r = cmake(r.x + sm[0][i], r.y + sm[1][i]);
  }
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(CRED_BLOCK)
k_cdot_partial(LayoutDev lx, const double *__restrict__ x, LayoutDev ly, const double *__restrict__ y, Box box, double *part) {
  const long long total = box.count();
  double sr = 0.0, si = 0.0;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    int i0, i1, i2;
    unflatten_box(box, t, i0, i1, i2);
    const cplx a = cload(x, lidx_plain(lx, i0, i1, i2)), b = cload(y, lidx_plain(ly, i0, i1, i2));
    sr = sr + a.x * b.x;
    sr = sr - a.y * b.y;
    si = si + a.x * b.y;
    si = si + a.y * b.x;
  }
  const cplx r = cblock_sum(cmake(sr, si));
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = r.x;
    part[2 * blockIdx.x + 1] = r.y;
  }
}

__global__ void __launch_bounds__(CRED_BLOCK) k_cdot_final(const double *part, int n, double *result) {
  double sr = 0.0, si = 0.0;
  for (int i = threadIdx.x; i < n; i += CRED_BLOCK) {
    sr = sr + part[2 * i];
    si = si + part[2 * i + 1];
  }
  const cplx r = cblock_sum(cmake(sr, si));
  if (threadIdx.x == 0) {
    result[0] = r.x;
    result[1] = r.y;
  }
}

// ---- node transfer operators on each part: the terms and their order are those of k_restrict / k_prolong_add (kernels_transfer.hip) -----------
template <int ND>
__global__ void __launch_bounds__(256)
k_crestrict(LayoutDev lfine, const double *__restrict__ rf, LayoutDev lc, double *__restrict__ fc, double scale, Box box) {
  const long long total = box.count();
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    int I0, I1, I2;
    unflatten_box(box, t, I0, I1, I2);
    const double w1[3] = {0.25, 0.5, 0.25};
    const long long base = lidx_plain(lfine, 2 * I0, 2 * I1, ND == 3 ? 2 * I2 : 0);
    cplx acc = cmake(0.0, 0.0);
    bool first = true;
#pragma unroll
    for (int a = -1; a <= 1; ++a)
#pragma unroll
      for (int b = -1; b <= 1; ++b) {
        if (ND == 2) {
          const double wgt = scale * (w1[a + 1] * w1[b + 1]);
          const cplx v = cload(rf, base + a + lfine.s1 * b);
          const cplx tv = cmake(wgt * v.x, wgt * v.y);
          acc = first ? tv : cadd(acc, tv);
          first = false;
        } else {
#pragma unroll
          for (int c = -1; c <= 1; ++c) {
            const double wgt = scale * ((w1[a + 1] * w1[b + 1]) * w1[c + 1]);
            const cplx v = cload(rf, base + a + lfine.s1 * b + lfine.s2 * c);
            const cplx tv = cmake(wgt * v.x, wgt * v.y);
            acc = first ? tv : cadd(acc, tv);
            first = false;
          }
        }
      }
    cstore(fc, lidx_plain(lc, I0, I1, I2), acc);
  }
}

template <int ND>
__global__ void __launch_bounds__(256)
k_cprolong_add(LayoutDev lc, const double *__restrict__ uc, LayoutDev lfine, double *__restrict__ uf, Box box) {
  const long long total = box.count();
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    int i0, i1, i2;
    unflatten_box(box, t, i0, i1, i2);
    const int ii[3] = {i0, i1, i2};
    int n[3], ci[3][2];
    double cw[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (d >= ND) { n[d] = 1; ci[d][0] = 0; ci[d][1] = 0; cw[d][0] = 1.0; cw[d][1] = 0.0; continue; }
      if ((ii[d] & 1) == 0) { n[d] = 1; ci[d][0] = ii[d] / 2; ci[d][1] = ii[d] / 2; cw[d][0] = 1.0; cw[d][1] = 0.0; }
      else { n[d] = 2; ci[d][0] = (ii[d] + 1) / 2; ci[d][1] = (ii[d] - 1) / 2; cw[d][0] = 0.5; cw[d][1] = 0.5; }
    }
    cplx acc = cmake(0.0, 0.0);
    bool first = true;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          if (a < n[0] && b < n[1] && c < n[2]) {
            const double wgt = (cw[0][a] * cw[1][b]) * cw[2][c];
            const cplx v = cload(uc, lidx_plain(lc, ci[0][a], ci[1][b], ci[2][c]));
            const cplx tv = cmake(wgt * v.x, wgt * v.y);
            acc = first ? tv : cadd(acc, tv);
            first = false;
          }
        }
    const long long kf = lidx_plain(lfine, i0, i1, i2);
    cstore(uf, kf, cadd(cload(uf, kf), acc));
  }
}

// ---- boundary assignment, assembly from parts ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cshift_div(LayoutDev l, double *x, long long shift, double cr, double ci, Box box) {
  const long long total = box.count();
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    int i0, i1, i2;
    unflatten_box(box, t, i0, i1, i2);
    const long long k = lidx_plain(l, i0, i1, i2);
    cstore(x, k, cdiv(cload(x, k + shift), cr, ci));
  }
}

__global__ void __launch_bounds__(256)
k_cfrom_parts(LayoutDev l, double *dst, LayoutDev lre, const double *__restrict__ re, LayoutDev lim, const double *__restrict__ im, Box box) {
  const long long total = box.count();
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    int i0, i1, i2;
    unflatten_box(box, t, i0, i1, i2);
    cstore(dst, lidx_plain(l, i0, i1, i2), cmake(re ? re[lidx(lre, i0, i1, i2)] : 0.0, im ? im[lidx(lim, i0, i1, i2)] : 0.0));
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------------
static thread_local int g_cst_route = 0;   // examg_debug_cstencil_route (debug build): 0 the default, else EXAMG_CSTENCIL_*
static thread_local int g_cst_chunk = 0;   // ... rows (planes) per wave of the marching kernel, 0: by size

// The default route follows the measured tables (tools/complex_bench.py; profiles/complex_bench.json and complex_bench_sizes.json; DESIGN.md
// 4.15).  Loops over all points: the marching kernel is ahead or level at every measured size from 1.05 * 10^6 points up (1024^2 0.0133
// against 0.0136 ms, 128^3 0.0237 against 0.0273, 4096^2 0.165 against 0.174, 256^3 0.197 against 0.251) and behind or level at every one
// below (96^3 = 0.86 * 10^6: 0.0184 against 0.0151; 512^2 and smaller: both launch-bound); 10^6 is the round number in that gap.  On one
// colour half of the marching lanes idle: gather wins in 3-D and at 4096^2, loses at 1024^2 and 2048^2 -- coloured loops gather.
constexpr int CST_MARCH_MIN_ROW = 64;
constexpr long long CST_MARCH_MIN_POINTS = 1000000;

static inline dim3 cgrid_for(long long total, int cap = 8192) {
  long long nb = (total + 255) / 256;
  if (nb > cap) nb = cap;
  if (nb < 1) nb = 1;
  return dim3((unsigned)nb);
}

static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// a complex argument: 2-D or 3-D, untransformed
static bool clayout_ok(const char *who, const char *what, const examg_layout_t *l) {
  if (l->nd != 2 && l->nd != 3) { set_error("%s: the %s layout is not 2-D or 3-D", who, what); return false; }
  if (l->transform != EXAMG_LAYOUT_PLAIN) { set_error("%s: the %s layout is under a layout transformation", who, what); return false; }
  return true;
}

struct CStencilArgs {
  CStencilDev sd;
  Box box;
  bool star;
};

// checks of examg_cstencil_op / examg_cstencil_route: -1 refused (text set), 0 empty box, else the route
static int cstencil_prepare(const char *who, int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs,
                            const examg_layout_t *ld, const double *dst, const examg_stencil_t *st, const double *coef_im, const double *w, int colour,
                            const int32_t *begin, const int32_t *end, CStencilArgs &a) {
  if (!lu || !u || !st || !begin || !end) { set_error("%s: null argument", who); return -1; }
  if (mode < 0 || mode > EXAMG_CRELAX) { set_error("%s: bad mode %d", who, mode); return -1; }
  if (mode != EXAMG_APPLY && (!rhs || !lf)) { set_error("%s: rhs required for mode %d", who, mode); return -1; }
  if ((mode == EXAMG_SMOOTH || mode == EXAMG_CRELAX) && !w) { set_error("%s: w required for mode %d", who, mode); return -1; }
  if (mode == EXAMG_CRELAX) {
    if (dst && dst != u) { set_error("%s: EXAMG_CRELAX is in place: dst must be u", who); return -1; }
    dst = u;
    ld = lu;
  }
  if (!ld || !dst) { set_error("%s: null argument", who); return -1; }
  if (st->nent < 1 || st->nent > EXAMG_MAX_ENTRIES) { set_error("%s: nent %d out of range", who, st->nent); return -1; }
  if (st->cfield) { set_error("%s: complex stencil fields are not supported", who); return -1; }
  if (!clayout_ok(who, "u", lu) || !clayout_ok(who, "dst", ld) || (mode != EXAMG_APPLY && !clayout_ok(who, "rhs", lf))) return -1;
  const int nd = lu->nd;
  if (ld->nd != nd || (mode != EXAMG_APPLY && lf->nd != nd)) { set_error("%s: layouts of different dimensionality", who); return -1; }
  for (int k = 0; k < st->nent; ++k)
    for (int d = 0; d < 3; ++d) {
      const int o = st->off[k][d];
      if (o < -1 || o > 1) { set_error("%s: entry %d has an offset outside {-1, 0, 1}", who, k); return -1; }
      if (d >= nd && o != 0) { set_error("%s: entry %d has an offset in a dimension the layouts do not have", who, k); return -1; }
    }
  if (!aligned16(u) || !aligned16(dst) || (mode != EXAMG_APPLY && !aligned16(rhs))) { set_error("%s: an array is not 16-byte aligned", who); return -1; }
  if (colour < -1 || colour > 1) { set_error("%s: bad colour %d", who, colour); return -1; }
  if (dst == u) {
    // in place: every point read must keep its old value -- one colour, and no off-centre entry that reaches a point of that colour
    bool decoupled = colour >= 0;
    for (int k = 0; k < st->nent; ++k) {
      const int sum = st->off[k][0] + st->off[k][1] + st->off[k][2];
      if ((st->off[k][0] || st->off[k][1] || st->off[k][2]) && (sum & 1) == 0) decoupled = false;
    }
    if (!decoupled && mode != EXAMG_CRELAX) { set_error("%s: u and dst alias, which needs a colour and a stencil whose off-centre entries all reach the other colour", who); return -1; }
    if (!decoupled && colour >= 0) { set_error("%s: EXAMG_CRELAX needs a stencil whose off-centre entries all reach the other colour", who); return -1; }
  }
  if (mode == EXAMG_CRELAX) {
    if (colour < 0) { set_error("%s: EXAMG_CRELAX needs a colour (0 or 1)", who); return -1; }
    if (w[1] != 0.0) { set_error("%s: EXAMG_CRELAX needs a real relaxation weight (w[1] == 0.0)", who); return -1; }
    if (st->diag < 0 || st->diag >= st->nent || st->off[st->diag][0] || st->off[st->diag][1] || st->off[st->diag][2]) {
      set_error("%s: st->diag is not the (0, 0, 0) entry", who);
      return -1;
    }
  }
  a.box = make_box(begin, end);
  if (a.box.count() == 0) return 0;
  if (!box_inside(lu, a.box, stencil_reach(st))) { set_error("%s: box + stencil reach leaves the u allocation", who); return -1; }
  if (!box_inside(ld, a.box, 0)) { set_error("%s: box leaves the dst allocation", who); return -1; }
  if (mode != EXAMG_APPLY && !box_inside(lf, a.box, 0)) { set_error("%s: box leaves the rhs allocation", who); return -1; }

  const LayoutDev lud = make_layout(lu);
  CStencilDev &sd = a.sd;
  sd.nent = st->nent;
  sd.diag = st->diag;
  fill_u_offsets(sd.uo, st, lud);
  // star: all 2 nd + 1 axis offsets of reach 1, each once
  unsigned seen = 0;
  bool star = st->nent == 2 * nd + 1;
  for (int k = 0; k < EXAMG_MAX_ENTRIES; ++k) {
    sd.cr[k] = k < st->nent ? st->coef[k] : 0.0;
    sd.ci[k] = k < st->nent && coef_im ? coef_im[k] : 0.0;
    sd.sel[k] = SEL_C;
    if (k >= st->nent) continue;
    int nz = 0, code = SEL_C;
    for (int d = 0; d < 3; ++d)
      if (st->off[k][d]) {
        ++nz;
        code = 1 + 2 * d + (st->off[k][d] > 0 ? 1 : 0);
      }
    if (nd == 2 && code >= SEL_YM) code += 2;      // 2-D marches in y: the y neighbours are the rows held in registers
    if (nz > 1 || (seen & (1u << code))) star = false;
    seen |= 1u << code;
    sd.sel[k] = code;
  }
  a.star = star;
  if (g_cst_route == EXAMG_CSTENCIL_GATHER) return EXAMG_CSTENCIL_GATHER;
  if (g_cst_route == EXAMG_CSTENCIL_MARCH) return star ? EXAMG_CSTENCIL_MARCH : EXAMG_CSTENCIL_GATHER;
  return star && colour < 0 && a.box.n0() >= CST_MARCH_MIN_ROW && a.box.count() >= CST_MARCH_MIN_POINTS ? EXAMG_CSTENCIL_MARCH : EXAMG_CSTENCIL_GATHER;
}

template <class F>
static inline void with_cmode(int mode, F &&f) {
  if (mode == EXAMG_APPLY) f(std::integral_constant<int, EXAMG_APPLY>{});
  else if (mode == EXAMG_RESIDUAL) f(std::integral_constant<int, EXAMG_RESIDUAL>{});
  else if (mode == EXAMG_SMOOTH) f(std::integral_constant<int, EXAMG_SMOOTH>{});
  else f(std::integral_constant<int, EXAMG_CRELAX>{});
}

// checks shared by the point-wise entry points: a complex argument and the box
static bool carg_ok(const char *who, const char *what, const examg_layout_t *l, const void *p, const Box &box) {
  if (!clayout_ok(who, what, l)) return false;
  if (!aligned16(p)) { set_error("%s: %s is not 16-byte aligned", who, what); return false; }
  if (!box_inside(l, box, 0)) { set_error("%s: box leaves the %s allocation", who, what); return false; }
  return true;
}

}  // namespace examg

using namespace examg;

#ifdef EXAMG_DEBUG_HOOKS
// debug build libexamg_dbg.so only (per host thread): the kernel of examg_cstencil_op (0: the default; the marching kernel takes star stencils
// only, others stay on the gather kernel) and the rows (planes) per wave of the marching kernel (0: by size)
extern "C" int examg_debug_cstencil_route(int route, int chunk) {
  if (route != 0 && route != EXAMG_CSTENCIL_GATHER && route != EXAMG_CSTENCIL_MARCH) return 1;
  g_cst_route = route;
  g_cst_chunk = chunk > 0 ? chunk : 0;
  return 0;
}
#endif

extern "C" int examg_cstencil_route(int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs,
                                    const examg_layout_t *ld, const double *dst, const examg_stencil_t *st, const double *coef_im, const double *w,
                                    int colour, const int32_t *begin, const int32_t *end) {
  CStencilArgs a;
  return cstencil_prepare("examg_cstencil_route", mode, lu, u, lf, rhs, ld, dst, st, coef_im, w, colour, begin, end, a);
}

extern "C" int examg_cstencil_op(int mode, const examg_layout_t *lu_, const double *u, const examg_layout_t *lf_, const double *rhs,
                                 const examg_layout_t *ld_, double *dst, const examg_stencil_t *st, const double *coef_im, const double *w, int colour,
                                 const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  CStencilArgs a;
  const int route = cstencil_prepare("examg_cstencil_op", mode, lu_, u, lf_, rhs, ld_, dst, st, coef_im, w, colour, begin, end, a);
  if (route < 0) return 1;
  if (route == 0) return 0;
  if (mode == EXAMG_CRELAX) {
    dst = const_cast<double *>(u);
    ld_ = lu_;
  }
  const LayoutDev lu = make_layout(lu_), ld = make_layout(ld_), lf = mode != EXAMG_APPLY ? make_layout(lf_) : lu;
  const double wr = w ? w[0] : 0.0, wi = w ? w[1] : 0.0;
  const Box box = a.box;
  hipStream_t s = (hipStream_t)stream;
  if (route == EXAMG_CSTENCIL_GATHER) {
    const int row_w = colour >= 0 ? (box.n0() + 1) / 2 : box.n0();
    const long long total = (long long)box.n1() * box.n2() * row_w;
    with_cmode(mode, [&](auto M) {
      hipLaunchKernelGGL((k_cstencil_gather<decltype(M)::value>), cgrid_for(total, 1 << 20), dim3(256), 0, s, lu, u, lf, rhs, ld, dst, a.sd, wr, wi, colour,
                         box, row_w);
    });
    EXAMG_CHECK_LAUNCH("k_cstencil_gather");
    return 0;
  }
  const int nd = lu_->nd;
  CMarchGeom g;
  g.ntx = (box.n0() + 63) / 64;
  const int nm = nd == 2 ? box.n1() : box.n2();
  const long long cols = (long long)g.ntx * (nd == 2 ? 1 : box.n1());
  // about 16384 waves, runs of at least 4 rows (8 planes): a run reads two rows more than it writes, mostly from L2 -- measured
  // (profiles/complex_bench_chunks.json, residual): 4096^2 0.158 / 0.162 / 0.291 ms with 4 / 16 / 128 rows per wave, 256^3 0.207 / 0.196 /
  // 0.293 ms and 128^3 0.0273 / 0.0315 / 0.1783 ms with 4 / 16 / 128 planes (8 planes: 0.202 and 0.0248)
  const int min_run = nd == 2 ? 4 : 8;
  long long nchunk = (16384 + cols - 1) / cols;
  if (nchunk > nm / min_run) nchunk = nm / min_run;
  if (nchunk < 1) nchunk = 1;
  g.chunk = (int)((nm + nchunk - 1) / nchunk);
  if (g_cst_chunk > 0) g.chunk = g_cst_chunk;
  g.nwaves = cols * ((nm + g.chunk - 1) / g.chunk);
  dim3 block(64, CM_WY, 1), grid((unsigned)((g.nwaves + CM_WY - 1) / CM_WY), 1, 1);
  with_cmode(mode, [&](auto M) {
    if (nd == 2) hipLaunchKernelGGL((k_cstencil_march<decltype(M)::value, 2>), grid, block, 0, s, lu, u, lf, rhs, ld, dst, a.sd, wr, wi, colour, box, g);
    else hipLaunchKernelGGL((k_cstencil_march<decltype(M)::value, 3>), grid, block, 0, s, lu, u, lf, rhs, ld, dst, a.sd, wr, wi, colour, box, g);
  });
  EXAMG_CHECK_LAUNCH("k_cstencil_march");
  return 0;
}

extern "C" int examg_clincomb(int form, const examg_layout_t *lx, const double *x, const examg_layout_t *ly, const double *y, const examg_layout_t *lz,
                              const double *z, const examg_layout_t *ld, double *dst, const double *a, const double *b, const int32_t *begin,
                              const int32_t *end, examg_stream_t stream) {
  const char *who = "examg_clincomb";
  if (!lx || !x || !ly || !y || !ld || !dst || !a || !begin || !end) { set_error("%s: null argument", who); return 1; }
  if (form < EXAMG_C_XPAY || form > EXAMG_C_XPAYMBZ) { set_error("%s: unknown form %d", who, form); return 1; }
  if (form == EXAMG_C_XPAYMBZ && (!lz || !z || !b)) { set_error("%s: EXAMG_C_XPAYMBZ needs z and b", who); return 1; }
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 0;
  if (!carg_ok(who, "x", lx, x, box) || !carg_ok(who, "y", ly, y, box) || !carg_ok(who, "dst", ld, dst, box)) return 1;
  if (form == EXAMG_C_XPAYMBZ && !carg_ok(who, "z", lz, z, box)) return 1;
  const LayoutDev dx = make_layout(lx), dy = make_layout(ly), dd = make_layout(ld), dz = form == EXAMG_C_XPAYMBZ ? make_layout(lz) : dx;
  const double br = form == EXAMG_C_XPAYMBZ ? b[0] : 0.0, bi = form == EXAMG_C_XPAYMBZ ? b[1] : 0.0;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid = cgrid_for(box.count(), 1 << 16);
  if (form == EXAMG_C_XPAY) hipLaunchKernelGGL((k_clincomb<EXAMG_C_XPAY>), grid, dim3(256), 0, s, dx, x, dy, y, dz, z, dd, dst, a[0], a[1], br, bi, box);
  else if (form == EXAMG_C_XMAY) hipLaunchKernelGGL((k_clincomb<EXAMG_C_XMAY>), grid, dim3(256), 0, s, dx, x, dy, y, dz, z, dd, dst, a[0], a[1], br, bi, box);
  else hipLaunchKernelGGL((k_clincomb<EXAMG_C_XPAYMBZ>), grid, dim3(256), 0, s, dx, x, dy, y, dz, z, dd, dst, a[0], a[1], br, bi, box);
  EXAMG_CHECK_LAUNCH("k_clincomb");
  return 0;
}

extern "C" int examg_cdot(const examg_layout_t *lx, const double *x, const examg_layout_t *ly, const double *y, const int32_t *begin, const int32_t *end,
                          double *result, void *work, examg_stream_t stream) {
  const char *who = "examg_cdot";
  if (!lx || !x || !ly || !y || !begin || !end || !result || !work) { set_error("%s: null argument", who); return 1; }
  const Box box = make_box(begin, end);
  hipStream_t s = (hipStream_t)stream;
  if (box.count() == 0) return check_hip(hipMemsetAsync(result, 0, 2 * sizeof(double), s), "examg_cdot memset");
  if (!carg_ok(who, "x", lx, x, box) || !carg_ok(who, "y", ly, y, box)) return 1;
  long long nb = (box.count() + CRED_BLOCK * 4 - 1) / (CRED_BLOCK * 4);
  if (nb > CRED_MAX_BLOCKS) nb = CRED_MAX_BLOCKS;
  hipLaunchKernelGGL(k_cdot_partial, dim3((unsigned)nb), dim3(CRED_BLOCK), 0, s, make_layout(lx), x, make_layout(ly), y, box, (double *)work);
  hipLaunchKernelGGL(k_cdot_final, dim3(1), dim3(CRED_BLOCK), 0, s, (const double *)work, (int)nb, result);
  EXAMG_CHECK_LAUNCH("k_cdot");
  return 0;
}

extern "C" int examg_crestrict(const examg_layout_t *lfine, const double *rf, const examg_layout_t *lc, double *fc, double scale, const int32_t *begin,
                               const int32_t *end, examg_stream_t stream) {
  const char *who = "examg_crestrict";
  if (!lfine || !rf || !lc || !fc || !begin || !end) { set_error("%s: null argument", who); return 1; }
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 0;
  if (!clayout_ok(who, "fine", lfine)) return 1;
  if (lc->nd != lfine->nd) { set_error("%s: layouts of different dimensionality", who); return 1; }
  if (!carg_ok(who, "coarse", lc, fc, box)) return 1;
  if (!aligned16(rf)) { set_error("%s: fine is not 16-byte aligned", who); return 1; }
  Box fb = box;      // fine footprint [2 * b - 1, 2 * (e - 1) + 1]
  fb.b0 = 2 * box.b0; fb.e0 = 2 * (box.e0 - 1) + 1;
  fb.b1 = 2 * box.b1; fb.e1 = 2 * (box.e1 - 1) + 1;
  if (lfine->nd == 3) { fb.b2 = 2 * box.b2; fb.e2 = 2 * (box.e2 - 1) + 1; }
  if (!box_inside(lfine, fb, 1)) { set_error("%s: fine footprint leaves the fine allocation", who); return 1; }
  hipStream_t s = (hipStream_t)stream;
  if (lfine->nd == 3) hipLaunchKernelGGL((k_crestrict<3>), cgrid_for(box.count(), 1 << 16), dim3(256), 0, s, make_layout(lfine), rf, make_layout(lc), fc, scale, box);
  else hipLaunchKernelGGL((k_crestrict<2>), cgrid_for(box.count(), 1 << 16), dim3(256), 0, s, make_layout(lfine), rf, make_layout(lc), fc, scale, box);
  EXAMG_CHECK_LAUNCH("k_crestrict");
  return 0;
}

extern "C" int examg_cprolong_add(const examg_layout_t *lc, const double *uc, const examg_layout_t *lfine, double *uf, const int32_t *begin,
                                  const int32_t *end, examg_stream_t stream) {
  const char *who = "examg_cprolong_add";
  if (!lfine || !uf || !lc || !uc || !begin || !end) { set_error("%s: null argument", who); return 1; }
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 0;
  if (!clayout_ok(who, "coarse", lc)) return 1;
  if (lc->nd != lfine->nd) { set_error("%s: layouts of different dimensionality", who); return 1; }
  if (!carg_ok(who, "fine", lfine, uf, box)) return 1;
  if (!aligned16(uc)) { set_error("%s: coarse is not 16-byte aligned", who); return 1; }
  if (box.b0 < 0 || box.b1 < 0 || box.b2 < 0) { set_error("%s: negative fine index", who); return 1; }
  Box cb = box;      // coarse footprint [b / 2, e / 2]
  cb.b0 = box.b0 / 2; cb.e0 = box.e0 / 2 + 1;
  cb.b1 = box.b1 / 2; cb.e1 = box.e1 / 2 + 1;
  if (lfine->nd == 3) { cb.b2 = box.b2 / 2; cb.e2 = box.e2 / 2 + 1; }
  if (!box_inside(lc, cb, 0)) { set_error("%s: coarse footprint leaves the coarse allocation", who); return 1; }
  hipStream_t s = (hipStream_t)stream;
  if (lfine->nd == 3) hipLaunchKernelGGL((k_cprolong_add<3>), cgrid_for(box.count(), 1 << 16), dim3(256), 0, s, make_layout(lc), uc, make_layout(lfine), uf, box);
  else hipLaunchKernelGGL((k_cprolong_add<2>), cgrid_for(box.count(), 1 << 16), dim3(256), 0, s, make_layout(lc), uc, make_layout(lfine), uf, box);
  EXAMG_CHECK_LAUNCH("k_cprolong_add");
  return 0;
}

extern "C" int examg_cshift_div(const examg_layout_t *l, double *x, const int32_t *off, const double *c, const int32_t *begin, const int32_t *end,
                                examg_stream_t stream) {
  const char *who = "examg_cshift_div";
  if (!l || !x || !off || !c || !begin || !end) { set_error("%s: null argument", who); return 1; }
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 0;
  if (!carg_ok(who, "x", l, x, box)) return 1;
  for (int d = l->nd; d < 3; ++d)
    if (off[d]) { set_error("%s: offset in a dimension the layout does not have", who); return 1; }
  const int n[3] = {box.n0(), box.n1(), box.n2()};
  bool overlap = true;
  for (int d = 0; d < 3; ++d) {
    const int o = off[d] < 0 ? -off[d] : off[d];
    if (o >= n[d]) overlap = false;
  }
  if (overlap) { set_error("%s: the box overlaps its own shifted image", who); return 1; }
  const Box img{box.b0 + off[0], box.b1 + off[1], box.b2 + off[2], box.e0 + off[0], box.e1 + off[1], box.e2 + off[2]};
  if (!box_inside(l, img, 0)) { set_error("%s: the shifted box leaves the x allocation", who); return 1; }
  const LayoutDev ld = make_layout(l);
  const long long shift = off[0] + ld.s1 * off[1] + ld.s2 * off[2];
  hipLaunchKernelGGL(k_cshift_div, cgrid_for(box.count(), 1 << 16), dim3(256), 0, (hipStream_t)stream, ld, x, shift, c[0], c[1], box);
  EXAMG_CHECK_LAUNCH("k_cshift_div");
  return 0;
}

extern "C" int examg_cfrom_parts(const examg_layout_t *l, double *dst, const examg_layout_t *lre, const double *re, const examg_layout_t *lim,
                                 const double *im, const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  const char *who = "examg_cfrom_parts";
  if (!l || !dst || !begin || !end || (re && !lre) || (im && !lim)) { set_error("%s: null argument", who); return 1; }
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 0;
  if (!carg_ok(who, "dst", l, dst, box)) return 1;
  if ((re && lre->nd != l->nd) || (im && lim->nd != l->nd)) { set_error("%s: layouts of different dimensionality", who); return 1; }
  if (re && !box_inside(lre, box, 0)) { set_error("%s: box leaves the re allocation", who); return 1; }
  if (im && !box_inside(lim, box, 0)) { set_error("%s: box leaves the im allocation", who); return 1; }
  const LayoutDev ld = make_layout(l);
  hipLaunchKernelGGL(k_cfrom_parts, cgrid_for(box.count(), 1 << 16), dim3(256), 0, (hipStream_t)stream, ld, dst, re ? make_layout(lre) : ld, re,
                     im ? make_layout(lim) : ld, im, box);
  EXAMG_CHECK_LAUNCH("k_cfrom_parts");
  return 0;
}
