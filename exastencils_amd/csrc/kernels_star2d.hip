// 2-D 5-point constant-coefficient star on gfx950: the y-marching route of examg_stencil_op (SR_YMARCH, kernels_stencil.hip).
//
// The 2-D counterpart of k_stencil7_zmarch.  A wave owns a window of 128 consecutive x points (two per lane, one 16-byte access at
// 8-byte alignment) and marches in y with a register pipeline: rows y-1, y, y+1 of u stay in registers, so every u value is fetched
// once per chunk; x neighbours come from the adjacent lane (DPP wave shifts), the two values beside the window from one 8-byte load
// each, fetched with the stage.  The loads of step y+1 -- row y+2 of u, the right-hand side of row y+1, the two edge values of row
// y+1 -- are in flight while step y is computed.  y is cut into chunks (launch_star2d); a chunk re-reads its two halo rows.
//
// Accesses: a lane touches u only where its first point lies in the box -- columns x .. x+1 of rows b1-1 .. e1 and the columns
// b0-1 / e0, all inside the box grown by the stencil's reach, which the entry point has checked against the allocation.  The
// right-hand side and the destination are touched point by point where only one point of a pair lies in the box (load2g, 8-byte
// store): a ghost-0 right-hand side whose box holds the first or the last allocated double is never read outside.
//
// Arithmetic: the entries folded left to right in entry order (conv5), finish as the generic kernel -- bit-identical to
// k_stencil_generic; the file is compiled with -ffp-contract=off.
#include "examg_common.h"

namespace examg {

struct Coef5 {
  double c[5];
};

// ORDER 0: entries c,-x,+x,-y,+y    ORDER 1: entries c,+x,-x,+y,-y (the reference's 5-point Jacobi benchmark; field.laplace_fd)
template <int ORDER>
__device__ __forceinline__ double conv5(const Coef5 &k, double c, double xm, double xp, double ym, double yp) {
  double acc = k.c[0] * c;
  if (ORDER == 0) {
    acc = acc + k.c[1] * xm;
    acc = acc + k.c[2] * xp;
    acc = acc + k.c[3] * ym;
    acc = acc + k.c[4] * yp;
  } else {
    acc = acc + k.c[1] * xp;
    acc = acc + k.c[2] * xm;
    acc = acc + k.c[3] * yp;
    acc = acc + k.c[4] * ym;
  }
  return acc;
}

template <int MODE>
__device__ __forceinline__ double finish5(double u, double acc, double f, double w) {
  if (MODE == EXAMG_APPLY) return acc;
  if (MODE == EXAMG_RESIDUAL) return f - acc;
  return u + w * (f - acc);
}

// Which canonical 5-point entry order does a constant 2-D stencil have?  -1: none (permuted orders keep the generic kernel)
int star5_order(const examg_stencil_t *st) {
  static const int o0[5][2] = {{0, 0}, {-1, 0}, {1, 0}, {0, -1}, {0, 1}};
  static const int o1[5][2] = {{0, 0}, {1, 0}, {-1, 0}, {0, 1}, {0, -1}};
  if (st->cfield || st->nent != 5) return -1;
  bool m0 = true, m1 = true;
  for (int k = 0; k < 5; ++k) {
    if (st->off[k][2] != 0) return -1;
    for (int d = 0; d < 2; ++d) {
      m0 = m0 && st->off[k][d] == o0[k][d];
      m1 = m1 && st->off[k][d] == o1[k][d];
    }
  }
  return m0 ? 0 : (m1 ? 1 : -1);
}

constexpr int YM_WAVES = 4;          // waves per workgroup: four x-adjacent windows (the cache lines they share meet in one CU)
constexpr int YM_TARGET = 4096;      // waves the chunk rule aims at: four per SIMD of the 256 CUs
constexpr int YM_MINCHUNK = 16;      // rows per chunk at least: two halo rows re-read per chunk
// boxes from this many points take the route by default (tools/star2d_bench.py: the size sweep of DESIGN.md 4.19)
constexpr long long YM_MIN_POINTS = 1LL << 20;
static thread_local int g_s2_on = -1, g_s2_chunk = 0;   // examg_debug_star2d (debug build)

struct YMarchGeom {
  int colour;    // COL kernels: the colour to update
  int ntx, nch;  // windows per row, chunks in y
  int yc;        // rows per chunk
  int nt;        // 1: non-temporal stores
};

template <bool ALIAS> struct Ptr5 { typedef double *__restrict__ out; typedef const double *__restrict__ in; };
template <> struct Ptr5<true> { typedef double *out; typedef const double *in; };

// COL: red-black half sweep in place (dst == u): of the two points a lane holds exactly one has (i0 + i1 + i2) % 2 == g.colour; it is
// updated, the other is written back unchanged.  Race-free: only values of the other colour (never changed in this sweep) and the
// lane's own centre are used; the rows kept in registers were loaded before the wave updated them, and what is read of them is of
// the other colour.
template <int MODE, int ORDER, bool COL>
__global__ void __launch_bounds__(64 * YM_WAVES)
k_star5_ymarch(LayoutDev lu, typename Ptr5<COL>::in u, LayoutDev lf, const double *__restrict__ rhs, LayoutDev ld,
               typename Ptr5<COL>::out dst, Coef5 k, double w, Box box, YMarchGeom g) {
  const int lane = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const long long t = (long long)blockIdx.x * YM_WAVES + wv;
  const int tc = (int)(t / g.ntx);
  if (tc >= g.nch) return;      // wave-uniform
  const int tx = (int)(t - (long long)tc * g.ntx);
  const int x = box.b0 + tx * 128 + lane * 2;
  const int mb = box.b1 + tc * g.yc;
  const int me = min(mb + g.yc, box.e1);
  const bool va = x < box.e0, vb = x + 1 < box.e0;
  // the right neighbour of b comes from lane + 1 unless that lane is past the box; the left neighbour of a from lane - 1
  const bool rload = vb && (lane == 63 || x + 2 >= box.e0);
  const bool lload = va && lane == 0;

  const double *up = u + (lu.origin + lu.s2 * box.b2 + x);
  const double *fp = rhs + (lf.origin + lf.s2 * box.b2 + x);
  double *dp = dst + (ld.origin + ld.s2 * box.b2 + x);
  auto urow = [&](int m) {
    d2 r = {0.0, 0.0};
    if (va) r = load2(up + lu.s1 * m);       // x + 1 <= e0: inside the box grown by the reach
    return r;
  };
  d2 um = urow(mb - 1), uc = urow(mb);
  // one pipeline stage = everything step m needs from memory
  struct Stage {
    d2 un, f;
    double el, er;
  };
  auto load_stage = [&](Stage &st, int m) {
    st.un = urow(m + 1);
    st.f = d2{0.0, 0.0};
    if (MODE != EXAMG_APPLY) st.f = load2g(fp + lf.s1 * m, va, vb);
    st.el = 0.0;
    st.er = 0.0;
    if (lload) st.el = up[lu.s1 * m - 1];
    if (rload) st.er = up[lu.s1 * m + 2];
  };
  auto compute = [&](const Stage &st, int m) {
    double xl = lane_below(uc.y);
    double xr = lane_above(uc.x);
    if (lload) xl = st.el;
    if (rload) xr = st.er;
    d2 o;
    if (COL) {
      // x = b0 + 128 * tx + 2 * lane: the parity of (x + m + b2) is the same in every lane -- a scalar branch, one convolution
      o = uc;
      if (((box.b0 + m + box.b2) & 1) == g.colour) {
        const double acc = conv5<ORDER>(k, uc.x, xl, uc.y, um.x, st.un.x);
        o.x = finish5<MODE>(uc.x, acc, st.f.x, w);
      } else {
        const double acc = conv5<ORDER>(k, uc.y, uc.x, xr, um.y, st.un.y);
        o.y = finish5<MODE>(uc.y, acc, st.f.y, w);
      }
    } else {
      const double acc_a = conv5<ORDER>(k, uc.x, xl, uc.y, um.x, st.un.x);
      const double acc_b = conv5<ORDER>(k, uc.y, uc.x, xr, um.y, st.un.y);
      o.x = finish5<MODE>(uc.x, acc_a, st.f.x, w);
      o.y = finish5<MODE>(uc.y, acc_b, st.f.y, w);
    }
    double *q = dp + ld.s1 * m;
    if (vb) {
      if (g.nt) store2_nt(q, o);
      else store2(q, o);
    } else if (va) {
      q[0] = o.x;
    }
    um = uc;
    uc = st.un;
  };
  // software pipeline of depth 1: the loads of step m + 1 are in flight while step m is computed
  Stage st[2];
  load_stage(st[0], mb);
  int m = mb;
  while (m < me) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (m < me) {
        if (m + 1 < me) load_stage(st[j ^ 1], m + 1);
        compute(st[j], m);
        ++m;
      }
    }
  }
}

// Does the y-marching kernel take this 2-D loop?  Called by stencil_route (kernels_stencil.hip) for plain layouts, with colour_ok: no
// colour, or the in-place half sweep of the smoother.
bool star2d_wanted(const examg_layout_t *lu, const examg_stencil_t *st, const Box &box) {
  if (g_s2_on == 0 || lu->nd != 2 || box.n2() != 1 || star5_order(st) < 0) return false;
  return g_s2_on == 1 || box.count() >= YM_MIN_POINTS;
}

int launch_star2d(int mode, const LayoutDev &lu, const double *u, const LayoutDev &lf, const double *rhs, const LayoutDev &ld, double *dst,
                  const examg_stencil_t *st, double w, int colour, const Box &box, hipStream_t s) {
  const Coef5 k{{st->coef[0], st->coef[1], st->coef[2], st->coef[3], st->coef[4]}};
  YMarchGeom g;
  g.colour = colour;
  g.ntx = (box.n0() + 127) / 128;
  // chunk length: enough waves for the chip (YM_TARGET), chunks of at least YM_MINCHUNK rows (two halo rows re-read per chunk)
  int yc = g_s2_chunk;
  if (yc <= 0) {
    const int nch = YM_TARGET / g.ntx > 0 ? YM_TARGET / g.ntx : 1;
    yc = (box.n1() + nch - 1) / nch;
    if (yc < YM_MINCHUNK) yc = YM_MINCHUNK;
  }
  if (yc > box.n1()) yc = box.n1();
  g.yc = yc;
  g.nch = (box.n1() + yc - 1) / yc;
  // stores: non-temporal where the loop streams, plain where input, output and right-hand side fit the Infinity Cache together (the
  // rule of launch_zmarch)
  g.nt = box.count() * 24LL > 200000000LL ? 1 : 0;
  const long long tiles = (long long)g.ntx * g.nch;
  dim3 block(64, YM_WAVES, 1), grid((unsigned)((tiles + YM_WAVES - 1) / YM_WAVES), 1, 1);
  const int ord = star5_order(st);
  with_order(ord, [&](auto O) {
    constexpr int ORD = decltype(O)::value;
    if (colour >= 0) {
      hipLaunchKernelGGL((k_star5_ymarch<EXAMG_SMOOTH, ORD, true>), grid, block, 0, s, lu, u, lf, rhs, ld, dst, k, w, box, g);
    } else {
      with_mode(mode, [&](auto M) {
        hipLaunchKernelGGL((k_star5_ymarch<decltype(M)::value, ORD, false>), grid, block, 0, s, lu, u, lf, rhs, ld, dst, k, w, box, g);
      });
    }
  });
  EXAMG_CHECK_LAUNCH("k_star5_ymarch");
  return 0;
}

}  // namespace examg

#ifdef EXAMG_DEBUG_HOOKS
// on: -1 the rule, 0 never, 1 wherever structurally possible at any size; chunk_rows: 0 the rule (debug build only; per host thread)
extern "C" int examg_debug_star2d(int on, int chunk_rows) {
  examg::g_s2_on = on;
  examg::g_s2_chunk = chunk_rows;
  return 0;
}
#endif
