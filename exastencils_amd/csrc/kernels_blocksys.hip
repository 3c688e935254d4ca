// Coupled systems of n = 2 or 3 node-centred unknowns whose blocks are constant stencils, on gfx950: the operator rows
// Au_c = sum_d A_cd * u_d and the local solves of the collective point smoother.
//
// Reference: Examples/LinearElasticity/2D_FD_LinearElasticity_fromL2.exa2 (`( lambda + mu ) * ( dxx * u + dxy * v ) + lambda * Laplace * u`),
// `solve locally relax w { u => rowU == rhs_u  v => rowV == rhs_v }` (solver/l4/L4_LocalSolve.scala, solver/ir/IR_LocalSolve.scala)
// inside `color with { i0 % 2, i1 % 2, .. }` (baseExt/l4/L4_ColorLoops.scala).  The arithmetic order is fixed in include/examg.h; this
// file is compiled with contraction off.
//
// Access pattern (both kernels): one lane owns BSYS_PTS points, the same x in BSYS_PTS consecutive rows (lattice rows of the colour), x
// fastest across lanes, so the 64 lanes of a wave read 64 consecutive doubles of a row for every entry (every second double under a
// colouring with an x parity).  The ENTRY loop is the outer one: the blocks travel by value as kernel arguments -- per entry a
// coefficient and the linear offset of its neighbour in the unknowns' layout -- and are read through scalar loads (the entry index is
// wave-uniform); one such pair serves BSYS_PTS independent loads and products, which is what hides the latency of a scalar load
// behind work.  All rows of the call are evaluated by the lane that owns the points: the neighbourhood of u_d is
// fetched from memory for the first row that reads it and comes from the vector L1 for the others and for the neighbouring rows of
// the same lane (the elasticity blocks of one unknown have disjoint offsets: nothing is read twice for another row there).  No LDS,
// no scratch, no allocation.
//   k_bsys_op     the rows of the mask at every point of the box; dst_c = Au_c or f_c - Au_c.
//   k_bsys_relax  the points of one colour (the lattice of examg_common.h: make_colour / mc_row / mc_place; no lane idles on another
//                 colour's point where the expressions are single-axis parities): b_c = f_c - off-centre part, x = a^-1 b by the cofactor
//                 formulas, u_c = u_c + relax * (x_c - u_c).  The host has checked that the colouring decouples every off-centre offset:
//                 a lane reads points of other colours and its own points only, so the loop is race-free in place.
// A lane whose last rows lie outside the box (the lattice) computes the last valid row again and stores nothing for them.
// There is one route: a marching kernel for all-rows loops (the three current planes of every unknown in an LDS ring) gave the same
// bits and lost to k_bsys_op at every size measured, 1.08 at 4096^2 to 4.9 at 64^3 (profiles/bsys_bench_routes.json), and was deleted.
#include <limits.h>

#include "examg_common.h"

namespace examg {

constexpr int BSYS_MAXN = EXAMG_BSYS_MAX;
constexpr int BSYS_PTS = 4;

// one block: entry k multiplies the value at linear offset off[k] in the unknowns' layout
struct BsysBlock {
  int nent;                                // 0: no block (or, for the smoother, no entry off the centre)
  int off[EXAMG_MAX_ENTRIES];
  double coef[EXAMG_MAX_ENTRIES];
};

template <int N>
struct BsysArgs {
  double *u[N];
  const double *f[N];
  double *dst[N];
  LayoutDev lu, lf, ld;
  double centre[N * N];    // k_bsys_relax: a_cd
  BsysBlock A[N * N];      // k_bsys_relax: the entries off the centre only
};

// the blocks of row c left to right in d, the entries of each folded left to right in declared order, at the lane's points; any: was there one?
template <int N>
__device__ __forceinline__ void bsys_row(const BsysArgs<N> &a, int c, const long long (&iu)[BSYS_PTS], double (&row)[BSYS_PTS], bool &any) {
  any = false;
#pragma unroll
  for (int p = 0; p < BSYS_PTS; ++p) row[p] = 0.0;
#pragma unroll
  for (int d = 0; d < N; ++d) {
    const BsysBlock &B = a.A[c * N + d];
    if (B.nent == 0) continue;      // uniform
    const double *ud = a.u[d];
    double s[BSYS_PTS];
    {
      const double co = B.coef[0];
      const long long o = B.off[0];
#pragma unroll
      for (int p = 0; p < BSYS_PTS; ++p) s[p] = co * ud[iu[p] + o];
    }
#pragma unroll 2
    for (int k = 1; k < B.nent; ++k) {
      const double co = B.coef[k];
      const long long o = B.off[k];
#pragma unroll
      for (int p = 0; p < BSYS_PTS; ++p) s[p] = s[p] + co * ud[iu[p] + o];
    }
#pragma unroll
    for (int p = 0; p < BSYS_PTS; ++p) row[p] = any ? row[p] + s[p] : s[p];
    any = true;
  }
}

// ---- dst_c = A u (EXAMG_SYS_APPLY) or f_c - A u (EXAMG_SYS_RESIDUAL) for the rows c of the mask -------------------------------------------
template <int N>
__global__ void __launch_bounds__(256) k_bsys_op(BsysArgs<N> a, int mode, unsigned mask, Box box) {
  const int n0 = box.n0(), n1 = box.n1();
  const int ng = (n1 + BSYS_PTS - 1) / BSYS_PTS;
  const long long total = (long long)n0 * ng * box.n2();
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long r = t / n0;
    const int i0 = box.b0 + (int)(t - r * n0), j0 = (int)(r % ng) * BSYS_PTS, i2 = box.b2 + (int)(r / ng);
    long long iu[BSYS_PTS], jf[BSYS_PTS], id[BSYS_PTS];
    bool ok[BSYS_PTS];
#pragma unroll
    for (int p = 0; p < BSYS_PTS; ++p) {
      ok[p] = j0 + p < n1;
      const int i1 = box.b1 + (ok[p] ? j0 + p : n1 - 1);
      iu[p] = lidx_plain(a.lu, i0, i1, i2);
      jf[p] = lidx_plain(a.lf, i0, i1, i2);
      id[p] = lidx_plain(a.ld, i0, i1, i2);
    }
#pragma unroll
    for (int c = 0; c < N; ++c) {
      if (!((mask >> c) & 1u)) continue;      // uniform
      double row[BSYS_PTS];
      bool any;
      bsys_row<N>(a, c, iu, row, any);        // (a row of the mask has a block: host check)
      // no dst is an unknown (host check): the stores of this row are not read by the next one
#pragma unroll
      for (int p = 0; p < BSYS_PTS; ++p) {
        const double o = mode == EXAMG_SYS_RESIDUAL ? a.f[c][jf[p]] - row[p] : row[p];
        if (ok[p]) a.dst[c][id[p]] = o;
      }
    }
  }
}

// ---- the local solve of one colour, in place -----------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void bsys_solve(const double (&m)[N * N], const double (&b)[N], double (&xs)[N]);

// include/examg.h: examg_sys_relax, n = 2
template <>
__device__ __forceinline__ void bsys_solve<2>(const double (&m)[4], const double (&b)[2], double (&xs)[2]) {
  const double det = m[0] * m[3] - m[1] * m[2];
  xs[0] = (b[0] * m[3] - m[1] * b[1]) / det;
  xs[1] = (m[0] * b[1] - m[2] * b[0]) / det;
}
// n = 3: cofactors k_ij of a_ij, the determinant along the first row, x_i = ((k_0i * b_0 + k_1i * b_1) + k_2i * b_2) / det
template <>
__device__ __forceinline__ void bsys_solve<3>(const double (&m)[9], const double (&b)[3], double (&xs)[3]) {
  const double k00 = m[4] * m[8] - m[5] * m[7];
  const double k01 = m[5] * m[6] - m[3] * m[8];
  const double k02 = m[3] * m[7] - m[4] * m[6];
  const double k10 = m[2] * m[7] - m[1] * m[8];
  const double k11 = m[0] * m[8] - m[2] * m[6];
  const double k12 = m[1] * m[6] - m[0] * m[7];
  const double k20 = m[1] * m[5] - m[2] * m[4];
  const double k21 = m[2] * m[3] - m[0] * m[5];
  const double k22 = m[0] * m[4] - m[1] * m[3];
  const double det = (m[0] * k00 + m[1] * k01) + m[2] * k02;
  xs[0] = ((k00 * b[0] + k10 * b[1]) + k20 * b[2]) / det;
  xs[1] = ((k01 * b[0] + k11 * b[1]) + k21 * b[2]) / det;
  xs[2] = ((k02 * b[0] + k12 * b[1]) + k22 * b[2]) / det;
}

template <int N>
__global__ void __launch_bounds__(256) k_bsys_relax(BsysArgs<N> a, double relax, MCColour col, Box box) {
  const long long nrows = mc_rows(col);
  const long long total = (long long)col.row_w * ((nrows + BSYS_PTS - 1) / BSYS_PTS);
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long g = t / col.row_w;
    const int c0 = (int)(t - g * col.row_w);
    long long iu[BSYS_PTS], jf[BSYS_PTS];
    bool ok[BSYS_PTS];
#pragma unroll
    for (int p = 0; p < BSYS_PTS; ++p) {
      const long long rr = g * BSYS_PTS + p;
      int i0, i1, i2;
      mc_row(col, rr < nrows ? rr : nrows - 1, i1, i2);
      ok[p] = mc_place(col, box, c0, i1, i2, i0) && rr < nrows;
      if (i0 >= box.e0) i0 = box.b0;      // no point of the colour at this place of the row: a point of the box, computed and not stored
      iu[p] = lidx_plain(a.lu, i0, i1, i2);
      jf[p] = lidx_plain(a.lf, i0, i1, i2);
    }
    double b[N][BSYS_PTS];
#pragma unroll
    for (int c = 0; c < N; ++c) {
      double off[BSYS_PTS];
      bool any;
      bsys_row<N>(a, c, iu, off, any);
#pragma unroll
      for (int p = 0; p < BSYS_PTS; ++p) {
        const double fv = a.f[c][jf[p]];
        b[c][p] = any ? fv - off[p] : fv;
      }
    }
#pragma unroll
    for (int p = 0; p < BSYS_PTS; ++p) {
      double bp[N], xs[N];
#pragma unroll
      for (int c = 0; c < N; ++c) bp[c] = b[c][p];
      bsys_solve<N>(a.centre, bp, xs);
      if (!ok[p]) continue;
#pragma unroll
      for (int c = 0; c < N; ++c) {
        double *q = a.u[c] + iu[p];
        if (relax == 1.0) {
          *q = xs[c];
        } else {
          const double own = *q;
          *q = own + relax * (xs[c] - own);
        }
      }
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
static bool bsys_layout_ok(const char *who, const char *what, const examg_layout_t *l, const examg_layout_t *lu) {
  const int nd = lu->nd;
  if (l->nd != nd) { set_error("%s: the %s layout has %d dimensions, the unknowns %d", who, what, l->nd, nd); return false; }
  if (lay_split(l)) { set_error("%s: the %s layout is colour-split; block systems take plain layouts only", who, what); return false; }
  for (int d = 0; d < nd; ++d) {
    if (l->dup_l[d] == 0 && l->dup_r[d] == 0) { set_error("%s: the %s layout is a cell layout (no duplicate layers in dim %d); block systems are built for node fields", who, what, d); return false; }
    if (l->inner[d] != lu->inner[d] || l->dup_l[d] != lu->dup_l[d] || l->dup_r[d] != lu->dup_r[d]) {
      set_error("%s: the %s layout has %d + %d + %d points in dim %d, the unknowns %d + %d + %d", who, what, l->dup_l[d], l->inner[d], l->dup_r[d], d,
                lu->dup_l[d], lu->inner[d], lu->dup_r[d]);
      return false;
    }
  }
  return true;
}

// The checks both entry points share, and the kernels' arguments; relax: the unknowns are the destination, the blocks lose their centres.
// 0: go on, 1: error (message set), 2: nothing to do
template <int N>
static int bsys_prepare(const char *who, const examg_bsys_t *sys, bool relax, bool need_f, unsigned mask, const Box &box, BsysArgs<N> &a) {
  const int nd = sys->lu.nd;
  const LayoutDev lu = make_layout(&sys->lu);
  if (lu.s1 + lu.s2 + 1 > INT_MAX) { set_error("%s: the unknowns' layout is too large for 32-bit neighbour offsets", who); return 1; }
  for (int c = 0; c < N; ++c) {
    const bool row = (mask >> c) & 1u;
    if (!sys->u[c]) { set_error("%s: unknown %d is a null pointer", who, c); return 1; }
    if (need_f && row && !sys->f[c]) { set_error("%s: right-hand side %d is a null pointer", who, c); return 1; }
    if (!relax && row && !sys->dst[c]) { set_error("%s: destination %d is a null pointer", who, c); return 1; }
    if (!relax && row)
      for (int d = 0; d < N; ++d)
      {
        if (sys->dst[c] == sys->u[d]) { set_error("%s: destination %d is unknown %d; the operator does not run in place", who, c, d); return 1; }
        if (need_f && sys->dst[c] == sys->f[d]) { set_error("%s: destination %d is right-hand side %d; the rows are stored one after the other", who, c, d); return 1; }
      }
    a.u[c] = sys->u[c];
    a.f[c] = sys->f[c];
    a.dst[c] = relax ? nullptr : sys->dst[c];
  }
  for (int c = 0; c < N; ++c) {
    bool any = false;
    for (int d = 0; d < N; ++d) {
      const examg_stencil_t *st = sys->A[c * N + d];
      BsysBlock &B = a.A[c * N + d];
      B.nent = 0;
      a.centre[c * N + d] = 0.0;
      for (int k = 0; k < EXAMG_MAX_ENTRIES; ++k) {
        B.off[k] = 0;
        B.coef[k] = 0.0;
      }
      if (!st) continue;
      any = true;
      if (st->cfield) { set_error("%s: block (%d, %d) is a stencil field; the blocks of a block system are constant stencils", who, c, d); return 1; }
      if (st->nent < 1 || st->nent > EXAMG_MAX_ENTRIES) { set_error("%s: block (%d, %d): nent %d out of range", who, c, d, st->nent); return 1; }
      unsigned seen = 0;
      for (int k = 0; k < st->nent; ++k) {
        const int32_t *o = st->off[k];
        for (int t = 0; t < 3; ++t)
          if (o[t] < -1 || o[t] > 1 || (t >= nd && o[t] != 0)) {
            set_error("%s: block (%d, %d), entry %d (%d, %d, %d) reaches further than one point of a %d-D node field", who, c, d, k, o[0], o[1], o[2], nd);
            return 1;
          }
        const int pos = (o[0] + 1) + 3 * (o[1] + 1) + 9 * (o[2] + 1);
        if (seen & (1u << pos)) { set_error("%s: block (%d, %d), entry %d repeats the offset (%d, %d, %d)", who, c, d, k, o[0], o[1], o[2]); return 1; }
        seen |= 1u << pos;
        if (relax && pos == 13) {
          a.centre[c * N + d] = st->coef[k];
          continue;
        }
        B.off[B.nent] = (int)(o[0] + lu.s1 * o[1] + lu.s2 * o[2]);
        B.coef[B.nent] = st->coef[k];
        ++B.nent;
      }
    }
    if (!any && ((mask >> c) & 1u)) { set_error("%s: row %d has no block", who, c); return 1; }
    if (relax && a.centre[c * N + c] == 0.0) { set_error("%s: a_%d%d, the centre coefficient of block (%d, %d), is zero", who, c, c, c, c); return 1; }
  }
  if (box.count() == 0) return 2;
  if (nd == 2 && (box.b2 != 0 || box.e2 != 1)) { set_error("%s: 2-D box must have [0,1) in dim 2", who); return 1; }
  if (!box_inside(&sys->lu, box, 1)) { set_error("%s: box + one point leaves the allocation of the unknowns", who); return 1; }
  if (need_f && !box_inside(&sys->lf, box, 0)) { set_error("%s: box leaves the rhs allocation", who); return 1; }
  if (!relax && !box_inside(&sys->ld, box, 0)) { set_error("%s: box leaves the dst allocation", who); return 1; }
  a.lu = lu;
  a.lf = make_layout(&sys->lf);
  a.ld = relax ? a.lu : make_layout(&sys->ld);      // examg_bsys_relax has no destination: sys->ld is not looked at
  return 0;
}

static int bsys_check_head(const char *who, const examg_bsys_t *sys, const int32_t *begin, const int32_t *end, bool relax) {
  if (!sys || !begin || !end) { set_error("%s: null argument", who); return 1; }
  if (sys->n < 2 || sys->n > BSYS_MAXN) { set_error("%s: n = %d unknowns; block systems have 2 or 3", who, sys->n); return 1; }
  if (sys->lu.nd != 2 && sys->lu.nd != 3) { set_error("%s: 2-D or 3-D layouts", who); return 1; }
  if (!bsys_layout_ok(who, "unknowns'", &sys->lu, &sys->lu) || !bsys_layout_ok(who, "rhs", &sys->lf, &sys->lu)) return 1;
  if (!relax && !bsys_layout_ok(who, "dst", &sys->ld, &sys->lu)) return 1;
  return 0;
}

static unsigned bsys_grid(long long threads) {
  long long nb = (threads + 255) / 256;
  return (unsigned)(nb > 8192 ? 8192 : nb);
}

// examg_bsys_op and examg_bsys_route: launch == false answers with the route and launches nothing
template <int N>
static int bsys_op(const examg_bsys_t *sys, int mode, unsigned mask, const Box &box, bool launch, hipStream_t s) {
  BsysArgs<N> a;
  const int rc = bsys_prepare<N>(launch ? "examg_bsys_op" : "examg_bsys_route", sys, false, mode == EXAMG_SYS_RESIDUAL, mask, box, a);
  if (!launch) return rc == 1 ? -1 : (rc == 2 ? 0 : EXAMG_BSYS_GATHER);
  if (rc) return rc == 2 ? 0 : 1;
  const long long lanes = (long long)box.n0() * ((box.n1() + BSYS_PTS - 1) / BSYS_PTS) * box.n2();
  hipLaunchKernelGGL((k_bsys_op<N>), dim3(bsys_grid(lanes)), dim3(256), 0, s, a, mode, mask, box);
  EXAMG_CHECK_LAUNCH("k_bsys_op");
  return 0;
}

template <int N>
static int bsys_relax(const examg_bsys_t *sys, double relax, const examg_colouring_t *col, const int32_t *begin, const Box &box, hipStream_t s) {
  const char *who = "examg_bsys_relax";
  BsysArgs<N> a;
  const int rc = bsys_prepare<N>(who, sys, true, true, (1u << N) - 1u, box, a);
  if (rc == 1) return 1;
  // no neighbour that a point reads may belong to its own colour
  for (int e = 0; e < N * N; ++e)
    for (int k = 0; sys->A[e] && k < sys->A[e]->nent; ++k) {
      const int32_t *o = sys->A[e]->off[k];
      if ((o[0] || o[1] || o[2]) && !colouring_separates(col, o)) {
        set_error("%s: the colouring does not decouple block (%d, %d): its offset (%d, %d, %d) leads to a point of the same colour, an in-place "
                  "loop over one colour would depend on the loop order", who, e / N, e % N, o[0], o[1], o[2]);
        return 1;
      }
    }
  if (rc == 2) return 0;
  if (!starts_nonnegative(col, begin)) { set_error("%s: a colour expression can be negative in this box (shift + begin < 0)", who); return 1; }
  const MCColour c = make_colour(col, box);
  if (mc_threads(c) == 0) return 0;      // no lattice point in the box
  const long long lanes = (long long)c.row_w * ((mc_rows(c) + BSYS_PTS - 1) / BSYS_PTS);
  hipLaunchKernelGGL((k_bsys_relax<N>), dim3(bsys_grid(lanes)), dim3(256), 0, s, a, relax, c, box);
  EXAMG_CHECK_LAUNCH("k_bsys_relax");
  return 0;
}

// launch: 0 or 1 (error text set); otherwise the route, -1 for a call that examg_bsys_op refuses
static int bsys_op_entry(int mode, const examg_bsys_t *sys, uint32_t row_mask, const int32_t *begin, const int32_t *end, bool launch, hipStream_t s) {
  const char *who = launch ? "examg_bsys_op" : "examg_bsys_route";
  const int refused = launch ? 1 : -1;
  if (mode != EXAMG_SYS_APPLY && mode != EXAMG_SYS_RESIDUAL) { set_error("%s: bad mode %d", who, mode); return refused; }
  if (bsys_check_head(who, sys, begin, end, false)) return refused;
  if (row_mask == 0 || (row_mask >> sys->n) != 0) { set_error("%s: row mask 0x%x for %d rows", who, row_mask, sys->n); return refused; }
  const Box box = make_box(begin, end);
  return sys->n == 2 ? bsys_op<2>(sys, mode, row_mask, box, launch, s) : bsys_op<3>(sys, mode, row_mask, box, launch, s);
}

}  // namespace examg

using namespace examg;

extern "C" int examg_bsys_op(int mode, const examg_bsys_t *sys, uint32_t row_mask, const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  return bsys_op_entry(mode, sys, row_mask, begin, end, true, (hipStream_t)stream);
}

extern "C" int examg_bsys_route(int mode, const examg_bsys_t *sys, uint32_t row_mask, const int32_t *begin, const int32_t *end) {
  return bsys_op_entry(mode, sys, row_mask, begin, end, false, nullptr);
}

extern "C" int examg_bsys_relax(const examg_bsys_t *sys, double relax, const examg_colouring_t *col, const int32_t *begin, const int32_t *end,
                                examg_stream_t stream) {
  const char *who = "examg_bsys_relax";
  if (!col) { set_error("%s: null argument", who); return 1; }
  if (bsys_check_head(who, sys, begin, end, true)) return 1;
  if (const char *msg = check_colouring(col, sys->lu.nd, true)) { set_error("%s: colouring: %s", who, msg); return 1; }
  const Box box = make_box(begin, end);
  return sys->n == 2 ? bsys_relax<2>(sys, relax, col, begin, box, (hipStream_t)stream) : bsys_relax<3>(sys, relax, col, begin, box, (hipStream_t)stream);
}
