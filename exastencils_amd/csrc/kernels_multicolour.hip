// Multi-colour loops for gfx950: `color with { e_0, e_1, .. }` with several colour expressions, or with one that is not the parity of
// all indices (Compiler/src/exastencils/baseExt/l4/L4_ColorLoops.scala:32-66) -- the 8-colour Gauss-Seidel sweep of 27-point
// stencils, the 4- and 9-colour sweeps of 2-D 9-point ones.  include/examg.h defines colourings, colours, their order and decoupling.
//
// Two kernels:
//   * k_stencil_coloured: the arithmetic of k_stencil_generic (kernels_stencil.hip) on the points of one colour.  Expressions on a
//     single axis are iterated as a lattice (first + n * j per axis: no idle lanes); one expression over several axes that include x
//     becomes a start and a stride per row; whatever is left is a predicate.  Every expression is evaluated again on the point the
//     lattice arrives at: the lattice decides how many threads idle, never which points are written.
//   * k_mcgs_rowpair27: the colours (0, c1, c2) and (1, c1, c2) of the axis-parity colouring `i0 % 2, i1 % 2, i2 % 2` in one launch,
//     for 27-entry stencil fields of reach 1 in the record layout (EXAMG_CLAYOUT_ENTRY_FASTEST).  The dependency argument: the two
//     colours are consecutive in the reference's order; a point of the second has exactly two neighbours in the first, (x +- 1, y, z)
//     in its own row, because any dy or dz != 0 changes the y or z parity; and no other point written by either loop is a neighbour
//     of a point written by either.  The unit of ownership is therefore a ROW whose (y, z) parities are (c1, c2): ONE WAVE owns the
//     whole row, updates its first x colour tile by tile, waits for its own stores (a workgroup-scope fence: the waves of a
//     workgroup share one vector L1, and a wave reads back nothing but what it wrote itself), and then updates the second x colour.
//     No row is split between waves: a neighbour that recomputed a halo point of the first colour would read second-colour points
//     that the row's owner may already have overwritten.  Nothing is exchanged between workgroups.
//     Coefficients: every 216-byte record is read once per sweep -- the records of the first x colour in the first stage, the others
//     in the second.  A tile is 64 points of one colour (128 columns); its 64 records are fetched with consecutive lanes on
//     consecutive doubles of a record (flat index j -> record j / 27, entry j % 27, every second record of the row), pass through a
//     wave-private LDS strip and come back as the lane's own 27 values, as in k_stencilfield27_rec.  u: the 27 neighbours through
//     L1 / L2 as in that kernel.  Same products in the same order as the generic kernel: bit-identical to the eight loops.
// Compiled with -ffp-contract=off.
#include "examg_common.h"

namespace examg {

struct MCStencil {
  int nent, diag;
  long long uo[EXAMG_MAX_ENTRIES];  // linear offsets in the u layout
  double coef[EXAMG_MAX_ENTRIES];
  const double *cfield;
  long long cplane, cpt;            // strides between the entries of a point / between points (StencilDev of kernels_stencil.hip)
  int wdiv;
};

template <int MODE>
__global__ void __launch_bounds__(256)
k_stencil_coloured(LayoutDev lu, const double *u, LayoutDev lf, const double *__restrict__ rhs, LayoutDev ld, double *dst, LayoutDev lc,
                   MCStencil st, double w, MCColour col, Box box) {
  const long long total = mc_threads(col);
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    int i0, i1, i2;
    if (!mc_point(col, box, t, i0, i1, i2)) continue;
    const long long iu = lidx_plain(lu, i0, i1, i2);
    double acc;
    if (st.cfield) {
      const long long ic = lidx_plain(lc, i0, i1, i2) * st.cpt;
      acc = st.cfield[ic] * u[iu + st.uo[0]];
      for (int k = 1; k < st.nent; ++k) acc = acc + st.cfield[ic + k * st.cplane] * u[iu + st.uo[k]];
      if (MODE == EXAMG_SMOOTH) {
        const double dg = st.cfield[ic + st.diag * st.cplane];
        const double ww = st.wdiv ? w / dg : (1.0 / dg) * w;
        acc = u[iu] + ww * (rhs[lidx_plain(lf, i0, i1, i2)] - acc);
      }
    } else {
      acc = st.coef[0] * u[iu + st.uo[0]];
      for (int k = 1; k < st.nent; ++k) acc = acc + st.coef[k] * u[iu + st.uo[k]];
      if (MODE == EXAMG_SMOOTH) acc = u[iu] + w * (rhs[lidx_plain(lf, i0, i1, i2)] - acc);
    }
    if (MODE == EXAMG_RESIDUAL) acc = rhs[lidx_plain(lf, i0, i1, i2)] - acc;
    dst[lidx_plain(ld, i0, i1, i2)] = acc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// row-pair kernel
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int MC_WAVES = 4;

struct MCOffsets {
  long long o[27];
};

struct MCRows {
  int xs[2];        // first column of the first / second x colour in the box (>= box.b0; may be >= box.e0: no such point)
  int y0, ny;       // rows of this launch: i1 = y0 + 2 * j, j < ny
  int z0, nz;       // i2 = z0 + 2 * j, j < nz
};

template <bool WDIV>
__global__ void __launch_bounds__(64 * MC_WAVES)
k_mcgs_rowpair27(LayoutDev lu, double *u, LayoutDev lf, const double *__restrict__ rhs, LayoutDev lc, const double *__restrict__ cf, MCOffsets uo,
                 double w, Box box, MCRows rw) {
  __shared__ __attribute__((aligned(16))) double strip[MC_WAVES][64 * 27];
  const int lane = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const long long row = (long long)blockIdx.x * MC_WAVES + wv;
  if (row >= (long long)rw.ny * rw.nz) return;
  const int i1 = rw.y0 + 2 * (int)(row % rw.ny);
  const int i2 = rw.z0 + 2 * (int)(row / rw.ny);
  double *sb = strip[wv];
  for (int stage = 0; stage < 2; ++stage) {
    const int xs = rw.xs[stage];
    const int npts = xs < box.e0 ? (box.e0 - xs + 1) / 2 : 0;       // points of this x colour in the row
    for (int p0 = 0; p0 < npts; p0 += 64) {
      const int nv = min(64, npts - p0);
      const long long rec0 = lidx_plain(lc, xs + 2 * p0, i1, i2) * 27;
      // 64 records, every second one of the row: lane l takes doubles 64 i + l of the tile's 27 * 64
      double raw[27];
#pragma unroll
      for (int i = 0; i < 27; ++i) {
        const int j = 64 * i + lane, r = j / 27;
        raw[i] = cf[r < nv ? rec0 + 54LL * r + (j - 27 * r) : rec0];      // past the tile's records: a value nobody reads
      }
      const int x = xs + 2 * (p0 + (lane < nv ? lane : 0));
      const long long iu = lidx_plain(lu, x, i1, i2);
      double v[27];
#pragma unroll
      for (int k = 0; k < 27; ++k) v[k] = u[iu + uo.o[k]];
      const double f = rhs[lidx_plain(lf, x, i1, i2)];
#pragma unroll
      for (int i = 0; i < 27; ++i) sb[64 * i + lane] = raw[i];
      // the LDS operations of one wave execute in order: no barrier between the strip's writes and reads
      double c[27];
#pragma unroll
      for (int k = 0; k < 27; ++k) c[k] = sb[27 * lane + k];
      double acc = c[0] * v[0];
#pragma unroll
      for (int k = 1; k < 27; ++k) acc = acc + c[k] * v[k];
      const double ww = WDIV ? w / c[0] : (1.0 / c[0]) * w;      // the centre entry comes first (dispatch condition)
      acc = v[0] + ww * (f - acc);
      if (lane < nv) u[iu] = acc;
    }
    // the second x colour reads what this wave has just stored, (x +- 1, y, z): stores complete, then loads.  These loads take values
    // that OTHER LANES of the wave stored -- an exchange through plain memory, which only the fence pair orders: it lowers to
    // s_waitcnt vmcnt(0) (plus an invalidate of the vector L1 in threadgroup-split mode, where a wave's CU-local L1 is not enough).
    // Do not drop it because the kernel has no barrier.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
}

static thread_local int g_mc_per_colour = 0;      // examg_debug_mcgs_per_colour (debug build): the sweep as its colour loops

static bool decouples(const examg_colouring_t *col, const examg_stencil_t *st) {
  for (int e = 0; e < st->nent; ++e) {
    const int32_t *o = st->off[e];
    if (o[0] == 0 && o[1] == 0 && o[2] == 0) continue;
    if (!colouring_separates(col, o)) return false;
  }
  return true;
}

static bool is_parity_of_all(const examg_colouring_t *col, int nd) {
  return col->nexpr == 1 && col->mod[0] == 2 && col->axes[0] == (1 << nd) - 1;
}

// the checks of both entry points; 0: go on, 1: error (message set), 2: nothing to do
static int check_coloured(const char *who, int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs,
                          const examg_layout_t *ld, const double *dst, const examg_stencil_t *st, const examg_colouring_t *col, bool with_rem,
                          const int32_t *begin, const int32_t *end) {
  if (!col) { set_error("%s: null argument", who); return 1; }
  if (!check_stencil_args(who, mode, lu, u, lf, rhs, ld, dst, st, begin, end)) return 1;
  if (lu->nd < 1 || lu->nd > 3) { set_error("%s: nd %d out of range", who, lu->nd); return 1; }
  if (const char *msg = check_colouring(col, lu->nd, with_rem)) { set_error("%s: colouring: %s", who, msg); return 1; }
  if (lay_split(lu) || lay_split(ld) || (lf && lay_split(lf)) || (st->cfield && lay_split(&st->clayout))) {
    set_error("%s: a colour-split layout (EXAMG_LAYOUT_SPLIT_X) has no form under a multi-colouring", who);
    return 1;
  }
  if (u == dst && !decouples(col, st)) {
    set_error("%s: the colouring does not decouple the stencil: an in-place loop over one colour would depend on the loop order", who);
    return 1;
  }
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 2;
  if (!starts_nonnegative(col, begin)) { set_error("%s: a colour expression can be negative in this box (shift + begin < 0)", who); return 1; }
  return check_stencil_box(who, mode, lu, lf, ld, st, box) ? 0 : 1;
}

// one colour loop on the generic coloured kernel; the arguments have passed check_coloured
static int launch_coloured(int mode, const examg_layout_t *lu_, const double *u, const examg_layout_t *lf_, const double *rhs,
                           const examg_layout_t *ld_, double *dst, const examg_stencil_t *st, double w, const examg_colouring_t *col,
                           const Box &box, hipStream_t s) {
  const LayoutDev lu = make_layout(lu_), ld = make_layout(ld_);
  const LayoutDev lf = lf_ ? make_layout(lf_) : lu;
  MCStencil sd;
  const LayoutDev lc = fill_stencil_dev(sd, st, lu);
  sd.wdiv = st->wform == EXAMG_WEIGHT_DIVIDE ? 1 : 0;

  const MCColour c = make_colour(col, box);
  const long long total = mc_threads(c);
  if (total == 0) return 0;      // no lattice point in the box
  long long nb = (total + 255) / 256;
  if (nb > 8192) nb = 8192;
  dim3 grid((unsigned)nb), block(256);
  with_mode(mode, [&](auto M) {
    hipLaunchKernelGGL((k_stencil_coloured<decltype(M)::value>), grid, block, 0, s, lu, u, lf, rhs, ld, dst, lc, sd, w, c, box);
  });
  EXAMG_CHECK_LAUNCH("k_stencil_coloured");
  return 0;
}

// The route of examg_mcgs_sweep: what examg_mcgs_one_pass_eligible answers and the entry point switches on.
static bool rowpair_route(const examg_layout_t *lu, const examg_layout_t *lf, const examg_stencil_t *st, const examg_colouring_t *col,
                          const Box &box) {
  if (g_mc_per_colour) return false;
  if (lu->nd != 3 || col->nexpr != 3) return false;
  for (int k = 0; k < 3; ++k)
    if (col->axes[k] != (1 << k) || col->mod[k] != 2) return false;
  if (!stencil_field27(st) || st->ctransform != EXAMG_CLAYOUT_ENTRY_FASTEST || stencil_reach(st) != 1) return false;
  if (lay_split(lu) || lay_split(lf) || lay_split(&st->clayout)) return false;
  if (box.count() == 0) return false;
  return box_inside(lu, box, 1) && box_inside(lf, box, 0) && box_inside(&st->clayout, box, 0);
}

static int launch_rowpair(const examg_layout_t *lu_, double *u, const examg_layout_t *lf_, const double *rhs, const examg_stencil_t *st, double w,
                          const examg_colouring_t *col, const Box &box, hipStream_t s) {
  const LayoutDev lu = make_layout(lu_), lf = make_layout(lf_), lc = make_layout(&st->clayout);
  MCOffsets uo;
  fill_u_offsets(uo.o, st, lu);
  const int bb[3] = {box.b0, box.b1, box.b2}, ee[3] = {box.e0, box.e1, box.e2};
  // first point >= begin with (shift + i) % 2 == r, per axis and remainder (shift + begin >= 0: checked)
  auto first_of = [&](int d, int r) { return bb[d] + (r - (col->shift[d] + bb[d]) % 2 + 2) % 2; };
  for (int c2 = 0; c2 < 2; ++c2)
    for (int c1 = 0; c1 < 2; ++c1) {
      MCRows rw;
      rw.xs[0] = first_of(0, 0);
      rw.xs[1] = first_of(0, 1);
      rw.y0 = first_of(1, c1);
      rw.z0 = first_of(2, c2);
      rw.ny = rw.y0 < ee[1] ? (ee[1] - rw.y0 + 1) / 2 : 0;
      rw.nz = rw.z0 < ee[2] ? (ee[2] - rw.z0 + 1) / 2 : 0;
      const long long rows = (long long)rw.ny * rw.nz;
      if (rows == 0) continue;
      dim3 grid((unsigned)((rows + MC_WAVES - 1) / MC_WAVES)), block(64, MC_WAVES);
      if (st->wform == EXAMG_WEIGHT_DIVIDE)
        hipLaunchKernelGGL((k_mcgs_rowpair27<true>), grid, block, 0, s, lu, u, lf, rhs, lc, st->cfield, uo, w, box, rw);
      else
        hipLaunchKernelGGL((k_mcgs_rowpair27<false>), grid, block, 0, s, lu, u, lf, rhs, lc, st->cfield, uo, w, box, rw);
      EXAMG_CHECK_LAUNCH("k_mcgs_rowpair27");
    }
  return 0;
}

}  // namespace examg

using namespace examg;

#ifdef EXAMG_DEBUG_HOOKS
// debug build libexamg_dbg.so only (per host thread): examg_mcgs_sweep issues its colour loops one by one; returns the old value
extern "C" int examg_debug_mcgs_per_colour(int on) {
  const int old = g_mc_per_colour;
  g_mc_per_colour = on;
  return old;
}
#endif

extern "C" int examg_stencil_op_coloured(int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs,
                                         const examg_layout_t *ld, double *dst, const examg_stencil_t *st, double w,
                                         const examg_colouring_t *col, const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  const int rc = check_coloured("examg_stencil_op_coloured", mode, lu, u, lf, rhs, ld, dst, st, col, true, begin, end);
  if (rc) return rc == 2 ? 0 : 1;
  if (is_parity_of_all(col, lu->nd)) {
    // the colouring examg_stencil_op knows: (i0 + i1 + i2) % 2 == (rem - shift) mod 2, with every kernel it has for it
    const int colour = ((col->rem[0] - col->shift[0]) % 2 + 2) % 2;
    return examg_stencil_op(mode, lu, u, lf, rhs, ld, dst, st, w, colour, begin, end, stream);
  }
  return launch_coloured(mode, lu, u, lf, rhs, ld, dst, st, w, col, make_box(begin, end), (hipStream_t)stream);
}

extern "C" int examg_mcgs_one_pass_eligible(const examg_layout_t *lu, const examg_layout_t *lf, const examg_stencil_t *st,
                                            const examg_colouring_t *col, const int32_t *begin, const int32_t *end) {
  if (!lu || !lf || !st || !col || !begin || !end) return 0;
  if (lu->nd < 1 || lu->nd > 3) return 0;
  if (check_colouring(col, lu->nd, false) || !starts_nonnegative(col, begin)) return 0;
  return rowpair_route(lu, lf, st, col, make_box(begin, end)) ? 1 : 0;
}

extern "C" int examg_mcgs_sweep(const examg_layout_t *lu, double *u, const examg_layout_t *lf, const double *rhs, const examg_stencil_t *st,
                                double w, const examg_colouring_t *col, const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  // u == dst: check_coloured refuses a colouring that does not decouple the stencil
  const int rc = check_coloured("examg_mcgs_sweep", EXAMG_SMOOTH, lu, u, lf, rhs, lu, u, st, col, false, begin, end);
  if (rc) return rc == 2 ? 0 : 1;
  const Box box = make_box(begin, end);
  hipStream_t s = (hipStream_t)stream;
  if (rowpair_route(lu, lf, st, col, box)) return launch_rowpair(lu, u, lf, rhs, st, w, col, box, s);
  // the colour loops one by one, the first expression varying fastest (L4_ColorLoops.toRepeatLoops)
  examg_colouring_t c = *col;
  long long ncol = 1;
  for (int k = 0; k < c.nexpr; ++k) ncol *= c.mod[k];
  for (long long i = 0; i < ncol; ++i) {
    long long q = i;
    for (int k = 0; k < c.nexpr; ++k) {
      c.rem[k] = (int)(q % c.mod[k]);
      q /= c.mod[k];
    }
    int r;
    if (is_parity_of_all(&c, lu->nd))
      r = examg_stencil_op(EXAMG_SMOOTH, lu, u, lf, rhs, lu, u, st, w, ((c.rem[0] - c.shift[0]) % 2 + 2) % 2, begin, end, stream);
    else
      r = launch_coloured(EXAMG_SMOOTH, lu, u, lf, rhs, lu, u, st, w, &c, box, s);
    if (r) return r;
  }
  return 0;
}
