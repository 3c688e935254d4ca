// Lexicographic Gauss-Seidel for gfx950: the in-place loop `loop over u { u = u + ww * (rhs - A * u) }` WITHOUT a colouring, whose result
// depends on the order of its points.  The reference prints it as a sequential nest, x fastest (one per fragment); examg_gs_sweep
// computes exactly that nest's values -- every point with the same operations in the same order, so a correct parallel schedule gives
// the nest's bits -- on a parallel schedule derived from the stencil's offsets.  include/examg.h states the semantics.
//
// Skew.  Call an offset o LATER when the point i + o comes after i in the nest (o2 > 0, or o2 == 0 and o1 > 0, or o2 == o1 == 0 and
// o0 > 0).  A point reads the new value of its earlier neighbours and the old value of its later ones, so the later offsets of the
// stencil -- and the negated earlier ones: what a neighbour reads of the point -- are the dependencies.  gs_skew picks, once, the
// smallest a, b >= 1 with  o0 + a * o1 + b * o2 > 0  for every dependency: (1, 1) for star stencils, (2, 4) for every stencil of reach
// 1.  With the time t = i0 + a * i1 + b * i2 every point can then be updated once all points of smaller t are done, and points of
// equal t are independent of each other.
//
// Tiles.  Boxes of (i0, i1, i2) cannot be the units of a coarser schedule: with the offsets (1, -1, 0) and (-1, 0, 0) in one stencil
// two x-adjacent boxes each need the other's new values.  The units are boxes of (t, y', i2) with y' = i1 + c * i2, c = 1 when some
// dependency has o1 = -1 (then o2 = +1) and 0 otherwise: in these coordinates every dependency has three non-negative components
// (t strictly positive), so a tile (T, I1, I2) depends on tiles with smaller-or-equal indices only and the tile time T + I1 + I2
// orders them.  ONE LAUNCH updates all tiles of one tile time; the order between launches is the stream's.  No workgroup ever waits
// for another one: no flag, no cooperative launch, no persistent grid.
//
// Inside a tile one workgroup (one wave: 8 x 8 lanes over (y', i2) in 3-D, 64 x 1 in 2-D) loads the tile and the shell its stencil
// reaches into LDS, rows along t (consecutive t of a row are consecutive x: coalesced), then marches GS_TT steps along t: at step s
// lane (j, k) updates the point x = t - a * y - b * z of its row from LDS, a barrier between steps.  All lanes of a step read the same
// column of their rows; the row length is odd, so the 8-byte reads of a lane group fall on distinct bank pairs where rows are
// consecutive.  The tile's points are stored back row by row.  The right-hand sides of the tile's points are staged in LDS before the
// march (nothing a step waits for comes from memory); the coefficients of a stencil field are fetched one step ahead into registers.
//
// Routes (gs_route decides once, examg_gs_route answers from it):
//   one workgroup  k_gs_planes with one block: the point hyperplanes of the whole box, a barrier between them, values exchanged through
//                  memory (the waves of a workgroup share one vector L1; the fences order stores before loads) -- launch-bound levels
//   tiled          k_gs_tile, one launch per tile time
//   per hyperplane k_gs_planes, one launch per t: the simplest correct schedule -- large stencil fields of more than 9 entries, where the
//                  measurement puts it ahead of the tiles; elsewhere through the debug build's hook
// Compiled with -ffp-contract=off.
#include "examg_common.h"

namespace examg {

enum GsRoute { GS_REFUSED = -1, GS_EMPTY = 0, GS_ONE_WG = 1, GS_TILED = 2, GS_PLANES = 3 };

constexpr int GS_TT = 32;                  // steps of a tile along t
constexpr int GS_LANES = 64;               // lanes of a tile: one wave
constexpr int GS_TY3 = 8, GS_TZ3 = 8;      // 3-D tiles: 8 skewed rows by 8 planes; 2-D: 64 rows
constexpr int GS_WG_THREADS = 1024;        // the one-workgroup route
// largest box of the one-workgroup route, in points (profiles/gs_bench.json, 7- and 27-point constant stencils: one workgroup takes about 0.6
// and 0.8 of the tiled route's time at 31^3 points, 1.2 and 1.6 at 47^3)
constexpr long long GS_ONE_WG_MAX = 32 * 32 * 32;
// stencil fields of more than 9 entries above this many points take one launch per point hyperplane instead of tiles (27-entry field,
// profiles/gs_bench.json: tiles take 0.80 of that schedule's time at 63^3 points, 0.97 at 127^3, 1.45 at 255^3 -- a tile's wave reads
// its 27 coefficient planes one step ahead, a hyperplane launch has all its points in flight)
constexpr long long GS_FIELD_TILED_MAX = 128 * 128 * 128;

struct GsPlan {
  int a, b, c;        // t = i0 + a * i1 + b * i2,  y' = i1 + c * i2
  int ty, tz;         // lanes of a tile over (y', i2)
  int tmin, ymin;     // smallest t / y' of the box
  int nt;             // number of times of the box
  int NT, NY, NZ;     // tiles per direction
  int R, RY, RZ;      // reach of the stencil in (t, y', i2)
  int LT, LY, LZ;     // extents of a tile with its shell in LDS; LT odd
  Box box;

  __host__ __device__ int time(int i0, int i1, int i2) const { return i0 + a * i1 + b * i2; }
  __host__ __device__ int yskew(int i1, int i2) const { return i1 + c * i2; }
  __host__ __device__ int x_at(int t, int i1, int i2) const { return t - a * i1 - b * i2; }
  __host__ __device__ int y_at(int yp, int i2) const { return yp - c * i2; }
  // tile coordinates of a point, first time / row / plane of a tile
  __host__ __device__ int tile_t(int t) const { return (t - tmin) / GS_TT; }
  __host__ __device__ int tile_y(int yp) const { return (yp - ymin) / ty; }
  __host__ __device__ int tile_z(int i2) const { return (i2 - box.b2) / tz; }
  __host__ __device__ int tile_t0(int T) const { return tmin + T * GS_TT; }
  __host__ __device__ int tile_y0(int I1) const { return ymin + I1 * ty; }
  __host__ __device__ int tile_z0(int I2) const { return box.b2 + I2 * tz; }
  __host__ __device__ int tile_time(int T, int I1, int I2) const { return T + I1 + I2; }
  // the inverse maps, what k_gs_tile and the schedule hook enumerate with: the T of tile (I1, I2) in a launch, the row (y, z) of lane
  // (j, kk) of a tile, the x of that row at step s
  __host__ __device__ int tile_of_launch(int launch, int I1, int I2) const { return launch - I1 - I2; }
  __host__ __device__ int row_z(int I2, int kk) const { return tile_z0(I2) + kk; }
  __host__ __device__ int row_y(int I1, int j, int z) const { return y_at(tile_y0(I1) + j, z); }
  __host__ __device__ int row_x(int T, int s, int y, int z) const { return x_at(tile_t0(T) + s, y, z); }
  __host__ __device__ bool row_in_box(int y, int z) const { return z >= box.b2 && z < box.e2 && y >= box.b1 && y < box.e1; }
  __host__ __device__ bool x_in_box(int x) const { return x >= box.b0 && x < box.e0; }
  __host__ __device__ int tile_times() const { return NT + NY + NZ - 2; }
  __host__ __device__ int step_in_tile(int t) const { return (t - tmin) % GS_TT; }
  __host__ __device__ int lds_doubles() const { return LT * LY * LZ; }
};

static inline bool gs_later(const int32_t *o) { return o[2] > 0 || (o[2] == 0 && (o[1] > 0 || (o[1] == 0 && o[0] > 0))); }

// the skew of a stencil of reach 1, chosen here and nowhere else
static void gs_skew(const examg_stencil_t *st, int &a, int &b, int &c) {
  a = 1, b = 1, c = 0;
  int32_t dep[EXAMG_MAX_ENTRIES][3];
  int n = 0;
  for (int k = 0; k < st->nent; ++k) {
    const int32_t *o = st->off[k];
    if (o[0] == 0 && o[1] == 0 && o[2] == 0) continue;
    const int s = gs_later(o) ? 1 : -1;
    for (int d = 0; d < 3; ++d) dep[n][d] = s * o[d];
    ++n;
  }
  for (int k = 0; k < n; ++k)
    if (dep[k][2] == 0 && dep[k][1] > 0 && 1 - dep[k][0] > a) a = 1 - dep[k][0];
  for (int k = 0; k < n; ++k)
    if (dep[k][2] > 0) {
      const int need = 1 - (dep[k][0] + a * dep[k][1]);
      if (need > b) b = need;
      if (-dep[k][1] > c) c = -dep[k][1];
    }
}

static GsPlan gs_plan(const examg_layout_t *lu, const examg_stencil_t *st, const Box &box) {
  GsPlan p;
  gs_skew(st, p.a, p.b, p.c);
  p.box = box;
  p.ty = lu->nd == 3 ? GS_TY3 : GS_LANES;
  p.tz = lu->nd == 3 ? GS_TZ3 : 1;
  p.tmin = p.time(box.b0, box.b1, box.b2);
  p.nt = p.time(box.e0 - 1, box.e1 - 1, box.e2 - 1) - p.tmin + 1;
  p.ymin = p.yskew(box.b1, box.b2);
  const int nyp = p.yskew(box.e1 - 1, box.e2 - 1) - p.ymin + 1;
  p.NT = (p.nt + GS_TT - 1) / GS_TT;
  p.NY = (nyp + p.ty - 1) / p.ty;
  p.NZ = (box.n2() + p.tz - 1) / p.tz;
  p.R = p.RY = p.RZ = 0;
  for (int k = 0; k < st->nent; ++k) {
    const int32_t *o = st->off[k];
    const int dt = abs(p.time(o[0], o[1], o[2])), dy = abs(p.yskew(o[1], o[2])), dz = abs(o[2]);
    p.R = dt > p.R ? dt : p.R;
    p.RY = dy > p.RY ? dy : p.RY;
    p.RZ = dz > p.RZ ? dz : p.RZ;
  }
  p.LT = (GS_TT + 2 * p.R) | 1;
  p.LY = p.ty + 2 * p.RY;
  p.LZ = p.tz + 2 * p.RZ;
  return p;
}

struct GsStencil {
  int nent, diag;
  long long uo[EXAMG_MAX_ENTRIES];   // linear offsets in the u layout (k_gs_planes)
  int ldo[EXAMG_MAX_ENTRIES];        // offsets in a tile's LDS image (k_gs_tile)
  double coef[EXAMG_MAX_ENTRIES];
  const double *cfield;
  long long cplane, cpt;
  int wdiv;
};

// u[i] + ww * (rhs[i] - fold_k(c_k * u[i + o_k])), entries folded left to right in entry order; nb(k): the value of neighbour k.
// NENT > 0: the number of entries at compile time -- the loops unroll and the coefficients and offsets of a constant stencil stay in
// registers (read from the kernel arguments with a run-time index they cost a scalar load and a wait per entry and point, which is
// what a step of the tile march then consists of); 0: st.nent.
template <int NENT, class NB>
__device__ __forceinline__ double gs_point(const GsStencil &st, double w, long long ic, double f, double uc, NB &&nb) {
  const int n = NENT ? NENT : st.nent;
  if (st.cfield) {
    double acc = st.cfield[ic] * nb(0);
    double dg = st.cfield[ic + st.diag * st.cplane];
#pragma unroll
    for (int k = 1; k < n; ++k) acc = acc + st.cfield[ic + k * st.cplane] * nb(k);
    const double ww = st.wdiv ? w / dg : (1.0 / dg) * w;
    return uc + ww * (f - acc);
  }
  double acc = st.coef[0] * nb(0);
#pragma unroll
  for (int k = 1; k < n; ++k) acc = acc + st.coef[k] * nb(k);
  return uc + w * (f - acc);
}

// The points of the hyperplanes t_first .. t_first + t_count - 1, one hyperplane after the other.  t_count > 1 is for ONE block only:
// the barrier between two hyperplanes orders this block's waves and no others.
template <int NENT>
__global__ void __launch_bounds__(GS_WG_THREADS)
k_gs_planes(LayoutDev lu, double *u, LayoutDev lf, const double *__restrict__ rhs, LayoutDev lc, GsStencil st, double w, GsPlan p, int t_first,
            int t_count) {
  const int n1 = p.box.n1();
  const long long rows = (long long)n1 * p.box.n2();
  for (int tc = 0; tc < t_count; ++tc) {
    const int t = t_first + tc;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (long long)gridDim.x * blockDim.x) {
      const int i1 = p.box.b1 + (int)(r % n1), i2 = p.box.b2 + (int)(r / n1);
      const int i0 = p.x_at(t, i1, i2);
      if (!p.x_in_box(i0)) continue;
      const long long iu = lidx_plain(lu, i0, i1, i2);
      const long long ic = st.cfield ? lidx_plain(lc, i0, i1, i2) : 0;
      u[iu] = gs_point<NENT>(st, w, ic, rhs[lidx_plain(lf, i0, i1, i2)], u[iu], [&](int k) { return u[iu + st.uo[k]]; });
    }
    if (t_count > 1) {
      // the next hyperplane reads what OTHER waves of the block have just stored: stores complete, barrier, then loads (an exchange
      // through plain memory within one workgroup, as in k_mcgs_rowpair27)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __syncthreads();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
  }
}

// One tile per block; blockIdx = (I1, I2), T from the launch's tile time.  TY: rows y' of a tile (GS_LANES / TY planes).  CF: a stencil
// field; with NENT > 0 the coefficients of the next step are fetched while the current one computes.
// Dynamic LDS: the image of u (p.lds_doubles()), then the right-hand sides of the tile's points, GS_TT + 1 doubles per lane.
template <int TY, int NENT, bool CF>
__global__ void __launch_bounds__(GS_LANES)
k_gs_tile(LayoutDev lu, double *u, LayoutDev lf, const double *__restrict__ rhs, LayoutDev lc, GsStencil st, double w, GsPlan p, int tile_time,
          int nd) {
  extern __shared__ __attribute__((aligned(16))) double img[];
  const int I1 = blockIdx.x, I2 = blockIdx.y;
  const int T = p.tile_of_launch(tile_time, I1, I2);
  if (T < 0 || T >= p.NT) return;
  const Box &bx = p.box;
  const int t0 = p.tile_t0(T), yp0 = p.tile_y0(I1), z0 = p.tile_z0(I2);
  const int lane = threadIdx.x;
  // this lane's row: plane z, row y, x = x0 + s at step s
  const int j = lane % TY, kk = lane / TY;
  const int z = p.row_z(I2, kk), y = p.row_y(I1, j, z);
  const int x0 = p.row_x(T, 0, y, z);
  const bool row_ok = p.row_in_box(y, z) && x0 < bx.e0 && x0 + GS_TT > bx.b0;
  if (!__syncthreads_or(row_ok)) return;      // no point of the box in this tile (the same answer in every lane)
  double *fimg = img + p.lds_doubles();

  // the right-hand sides of the tile's points, 32 consecutive x per row (a point outside the box: the nearest one inside).  One wave
  // per tile and two or three tiles per CU: nothing hides a load's latency but the loads issued beside it, so both load loops are
  // unrolled far enough to keep 32 loads in flight per lane
#pragma unroll
  for (int q = 0; q < GS_TT; ++q) {
    const int i = lane + GS_LANES * q;
    const int s = i % GS_TT, l = i / GS_TT;
    const int cz = min(z0 + l / TY, bx.e2 - 1), cy = min(max(p.y_at(yp0 + l % TY, z0 + l / TY), bx.b1), bx.e1 - 1);
    const int cx = min(max(p.x_at(t0 + s, p.y_at(yp0 + l % TY, z0 + l / TY), z0 + l / TY), bx.b0), bx.e0 - 1);
    fimg[l * (GS_TT + 1) + s] = rhs[lidx_plain(lf, cx, cy, cz)];
  }
  // the tile and its shell, one row along t per load (LT <= 64 lanes), 32 rows in flight.  Only points of the box grown by one point are read -- the
  // host has checked that they are allocated; cells outside take the value of the nearest such point and are never used.
  const int g2 = nd == 3 ? 1 : 0;
  const int rows = p.LY * p.LZ;
  const int tt = min(lane, p.LT - 1);
  constexpr int GS_BATCH = 32;
  for (int r0 = 0; r0 < rows; r0 += GS_BATCH) {
    double v[GS_BATCH];
#pragma unroll
    for (int q = 0; q < GS_BATCH; ++q) {
      const int r = min(r0 + q, rows - 1);
      const int yy = r % p.LY, zz = r / p.LY;
      const int cz = z0 - p.RZ + zz, cy = p.y_at(yp0 - p.RY + yy, cz);
      const int cx = p.x_at(t0 - p.R + tt, cy, cz);
      v[q] = u[lidx_plain(lu, min(max(cx, bx.b0 - 1), bx.e0), min(max(cy, bx.b1 - 1), bx.e1), min(max(cz, bx.b2 - g2), bx.e2 - 1 + g2))];
    }
#pragma unroll
    for (int q = 0; q < GS_BATCH; ++q)
      if (lane < p.LT && r0 + q < rows) img[(r0 + q) * p.LT + lane] = v[q];
  }
  __syncthreads();

  const int cell0 = ((kk + p.RZ) * p.LY + (j + p.RY)) * p.LT + p.R;
  const double *fl = fimg + lane * (GS_TT + 1);
  if (CF && NENT > 0) {
    // the lane's coefficients one step ahead: a row of a coefficient plane per entry, a point outside the box clamped into it
    constexpr int NE = NENT > 0 ? NENT : 1;
    const int cy = min(max(y, bx.b1), bx.e1 - 1), cz = min(z, bx.e2 - 1);
    double c[NE], cn[NE];
    {
      const long long ic = lidx_plain(lc, min(max(x0, bx.b0), bx.e0 - 1), cy, cz);
#pragma unroll
      for (int k = 0; k < NE; ++k) cn[k] = st.cfield[ic + k * st.cplane];
    }
#pragma unroll 2
    for (int s = 0; s < GS_TT; ++s) {
#pragma unroll
      for (int k = 0; k < NE; ++k) c[k] = cn[k];
      {
        const long long ic = lidx_plain(lc, min(max(x0 + s + 1, bx.b0), bx.e0 - 1), cy, cz);
#pragma unroll
        for (int k = 0; k < NE; ++k) cn[k] = st.cfield[ic + k * st.cplane];
      }
      const int x = x0 + s;
      if (row_ok && p.x_in_box(x)) {
        const int cell = cell0 + s;
        double acc = c[0] * img[cell + st.ldo[0]];
        double dg = c[0];
#pragma unroll
        for (int k = 1; k < NE; ++k) {
          acc = acc + c[k] * img[cell + st.ldo[k]];
          dg = k == st.diag ? c[k] : dg;
        }
        const double ww = st.wdiv ? w / dg : (1.0 / dg) * w;
        img[cell] = img[cell] + ww * (fl[s] - acc);
      }
      __syncthreads();
    }
  } else {
#pragma unroll 2
    for (int s = 0; s < GS_TT; ++s) {
      const int x = x0 + s;
      if (row_ok && p.x_in_box(x)) {
        const int cell = cell0 + s;
        const long long ic = CF ? lidx_plain(lc, x, y, z) : 0;
        img[cell] = gs_point<NENT>(st, w, ic, fl[s], img[cell], [&](int k) { return img[cell + st.ldo[k]]; });
      }
      __syncthreads();      // the points of one step are independent; the next step reads them
    }
  }

#pragma unroll 8
  for (int q = 0; q < GS_TT; ++q) {
    const int i = lane + GS_LANES * q;
    const int s = i % GS_TT, l = i / GS_TT;
    const int lj = l % TY, lk = l / TY;
    const int cz = z0 + lk, cy = p.y_at(yp0 + lj, cz);
    const int cx = p.x_at(t0 + s, cy, cz);
    if (cx >= bx.b0 && cx < bx.e0 && cy >= bx.b1 && cy < bx.e1 && cz < bx.e2)
      u[lidx_plain(lu, cx, cy, cz)] = img[((lk + p.RZ) * p.LY + (lj + p.RY)) * p.LT + p.R + s];
  }
}

// f(std::integral_constant<int, N>{}): N the entry count where a kernel is compiled for it, else 0 -- the tile kernels of 3-D and of 2-D
// fields, and k_gs_planes (which keeps a constant stencil in scalar registers: 27 coefficients and 27 offsets do not fit)
template <class F>
static inline void with_nent3(int nent, F &&f) {
  if (nent == 7) f(std::integral_constant<int, 7>{});
  else if (nent == 27) f(std::integral_constant<int, 27>{});
  else f(std::integral_constant<int, 0>{});
}
template <class F>
static inline void with_nent2(int nent, F &&f) {
  if (nent == 5) f(std::integral_constant<int, 5>{});
  else if (nent == 9) f(std::integral_constant<int, 9>{});
  else f(std::integral_constant<int, 0>{});
}
template <class F>
static inline void with_nent_planes(int nent, F &&f) {
  if (nent == 5) f(std::integral_constant<int, 5>{});
  else if (nent == 7) f(std::integral_constant<int, 7>{});
  else if (nent == 9) f(std::integral_constant<int, 9>{});
  else f(std::integral_constant<int, 0>{});
}

static thread_local int g_gs_route = 0;      // examg_debug_gs_route (debug build): 0 as routed, else the GsRoute to force

// What a call does, decided once from its arguments alone: the refusals (error text set), the empty box, and the kernel route with its
// plan (`plan` is filled for the kernel routes only).
static GsRoute gs_route(const examg_layout_t *lu, const examg_layout_t *lf, const examg_stencil_t *st, const int32_t *begin, const int32_t *end,
                        GsPlan *plan) {
  const char *who = "examg_gs_sweep";
  if (!lu || !lf || !st || !begin || !end) { set_error("%s: null argument", who); return GS_REFUSED; }
  if (lu->nd < 2 || lu->nd > 3 || lf->nd != lu->nd) { set_error("%s: 2-D and 3-D fields only (nd %d, rhs nd %d)", who, lu->nd, lf->nd); return GS_REFUSED; }
  if (st->nent < 1 || st->nent > EXAMG_MAX_ENTRIES) { set_error("%s: nent %d out of range", who, st->nent); return GS_REFUSED; }
  if (st->diag < 0 || st->diag >= st->nent) { set_error("%s: diag %d out of range", who, st->diag); return GS_REFUSED; }
  if (lay_split(lu) || lay_split(lf) || (st->cfield && lay_split(&st->clayout))) {
    set_error("%s: a colour-split layout (EXAMG_LAYOUT_SPLIT_X) has no lexicographic sweep (examg_transform_field)", who);
    return GS_REFUSED;
  }
  for (int d = 0; d < lu->nd; ++d)
    if (lu->dup_l[d] < 1 || lu->dup_r[d] < 1 || lf->dup_l[d] < 1 || lf->dup_r[d] < 1) {
      set_error("%s: cell layout (no duplicate layers): the sweep is defined for node fields", who);
      return GS_REFUSED;
    }
  if (st->cfield && st->ctransform != EXAMG_CLAYOUT_PLANES) {
    set_error("%s: entry-fastest coefficient records (EXAMG_CLAYOUT_ENTRY_FASTEST) are not supported: planes only", who);
    return GS_REFUSED;
  }
  if (stencil_reach(st) > 1) { set_error("%s: offsets of reach 2 or more are not supported (reach %d)", who, stencil_reach(st)); return GS_REFUSED; }
  for (int k = 0; k < st->nent; ++k)
    if (lu->nd == 2 && st->off[k][2] != 0) { set_error("%s: a z offset in a 2-D stencil", who); return GS_REFUSED; }
  const Box box = make_box(begin, end);
  if (box.count() == 0) return GS_EMPTY;
  // k_gs_tile loads the one-point shell of the box whatever the stencil reaches (a centre-only stencil has reach 0): the shell must be
  // allocated for every stencil, which is what include/examg.h promises to refuse otherwise
  if (!box_inside(lu, box, 1)) { set_error("%s: the one-point shell of the box leaves the u allocation", who); return GS_REFUSED; }
  if (!check_stencil_box(who, EXAMG_SMOOTH, lu, lf, lu, st, box)) return GS_REFUSED;
  *plan = gs_plan(lu, st, box);
  if (plan->NZ > 65535) { set_error("%s: box too large", who); return GS_REFUSED; }
  if (g_gs_route) return (GsRoute)g_gs_route;
  if (box.count() <= GS_ONE_WG_MAX) return GS_ONE_WG;
  return st->cfield && st->nent > 9 && box.count() > GS_FIELD_TILED_MAX ? GS_PLANES : GS_TILED;
}

static GsStencil gs_stencil(const examg_stencil_t *st, const LayoutDev &lu, const GsPlan &p, LayoutDev &lc) {
  GsStencil sd;
  lc = fill_stencil_dev(sd, st, lu);
  sd.wdiv = st->wform == EXAMG_WEIGHT_DIVIDE ? 1 : 0;
  for (int k = 0; k < EXAMG_MAX_ENTRIES; ++k) {
    const int32_t *o = st->off[k];
    sd.ldo[k] = k < st->nent ? p.time(o[0], o[1], o[2]) + p.LT * (p.yskew(o[1], o[2]) + p.LY * o[2]) : 0;
  }
  return sd;
}

static int gs_launches(GsRoute route, const GsPlan &p) {
  return route == GS_ONE_WG ? 1 : route == GS_TILED ? p.tile_times() : route == GS_PLANES ? p.nt : 0;
}

}  // namespace examg

using namespace examg;

#ifdef EXAMG_DEBUG_HOOKS
// debug build libexamg_dbg.so only (per host thread): 0 = as routed, 1 = one workgroup, 2 = tiled, 3 = one launch per point hyperplane,
// whatever the size of the box; returns the old value
extern "C" int examg_debug_gs_route(int route) {
  const int old = g_gs_route;
  g_gs_route = (route >= 1 && route <= 3) ? route : 0;
  return old;
}

// launches of one sweep on the route these arguments take (under the hook); -1: refused.  For the measurements, whose boxes are too
// large for the per-point arrays of examg_debug_gs_schedule.
extern "C" int examg_debug_gs_launches(const examg_layout_t *lu, const examg_layout_t *lf, const examg_stencil_t *st, const int32_t *begin,
                                       const int32_t *end) {
  GsPlan p;
  const GsRoute route = gs_route(lu, lf, st, begin, end, &p);
  if (route == GS_REFUSED) return -1;
  if (route == GS_EMPTY) return 0;
  return gs_launches(route, p);
}

// The sweep enumerated on the host the way the kernels enumerate it -- launches, blocks, lanes and steps, through the same GsPlan
// functions (tile_of_launch, row_z / row_y / row_x, row_in_box / x_in_box; x_at for k_gs_planes) -- and every point it visits marked:
// for every point of the box (x fastest, n0 * n1 * n2 entries) the launch that updates it and the barrier step within that launch; -1
// for a point no lane visits, -2 in `launch` for a point visited more than once.  Returns the route, -1 refused.
extern "C" int examg_debug_gs_schedule(const examg_layout_t *lu, const examg_layout_t *lf, const examg_stencil_t *st, const int32_t *begin,
                                       const int32_t *end, int32_t *launch, int32_t *step) {
  GsPlan p;
  const GsRoute route = gs_route(lu, lf, st, begin, end, &p);
  if (route == GS_REFUSED || route == GS_EMPTY) return route;
  if (!launch || !step) { set_error("examg_debug_gs_schedule: null argument"); return GS_REFUSED; }
  const Box &box = p.box;
  const long long total = box.count();
  for (long long i = 0; i < total; ++i) launch[i] = step[i] = -1;
  auto mark = [&](int x, int y, int z, int l, int s) {
    const long long i = (x - box.b0) + (long long)box.n0() * ((y - box.b1) + (long long)box.n1() * (z - box.b2));
    launch[i] = launch[i] == -1 ? l : -2;
    step[i] = s;
  };
  if (route == GS_TILED) {
    for (int l = 0; l < p.tile_times(); ++l)
      for (int I2 = 0; I2 < p.NZ; ++I2)
        for (int I1 = 0; I1 < p.NY; ++I1) {
          const int T = p.tile_of_launch(l, I1, I2);
          if (T < 0 || T >= p.NT) continue;
          for (int lane = 0; lane < GS_LANES; ++lane) {
            const int z = p.row_z(I2, lane / p.ty), y = p.row_y(I1, lane % p.ty, z);
            if (!p.row_in_box(y, z)) continue;
            for (int s = 0; s < GS_TT; ++s)
              if (p.x_in_box(p.row_x(T, s, y, z))) mark(p.row_x(T, s, y, z), y, z, l, s);
          }
        }
    return route;
  }
  // k_gs_planes: every row of the box at every time
  for (int tc = 0; tc < p.nt; ++tc)
    for (int i2 = box.b2; i2 < box.e2; ++i2)
      for (int i1 = box.b1; i1 < box.e1; ++i1) {
        const int i0 = p.x_at(p.tmin + tc, i1, i2);
        if (p.x_in_box(i0)) mark(i0, i1, i2, route == GS_ONE_WG ? 0 : tc, route == GS_ONE_WG ? tc : 0);
      }
  return route;
}
#endif

extern "C" int examg_gs_route(const examg_layout_t *lu, const examg_layout_t *lf, const examg_stencil_t *st, const int32_t *begin,
                              const int32_t *end) {
  GsPlan p;
  return gs_route(lu, lf, st, begin, end, &p);
}

extern "C" int examg_gs_sweep(const examg_layout_t *lu_, double *u, const examg_layout_t *lf_, const double *rhs, const examg_stencil_t *st,
                              double w, const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  if (!u || !rhs) { set_error("examg_gs_sweep: null argument"); return 1; }
  GsPlan p;
  const GsRoute route = gs_route(lu_, lf_, st, begin, end, &p);
  if (route == GS_REFUSED) return 1;
  if (route == GS_EMPTY) return 0;
  hipStream_t s = (hipStream_t)stream;
  const LayoutDev lu = make_layout(lu_), lf = make_layout(lf_);
  LayoutDev lc;
  const GsStencil sd = gs_stencil(st, lu, p, lc);
  if (route == GS_ONE_WG || route == GS_PLANES) {
    // one block for all hyperplanes, or one launch of many blocks per hyperplane
    const long long rows = (long long)p.box.n1() * p.box.n2();
    const long long nb = route == GS_ONE_WG ? 1 : (rows + 255) / 256 < 65536 ? (rows + 255) / 256 : 65536;
    const dim3 grid((unsigned)nb), block(route == GS_ONE_WG ? GS_WG_THREADS : 256);
    const int count = route == GS_ONE_WG ? p.nt : 1;
    for (int t = 0; t < p.nt; t += count) {
      with_nent_planes(st->nent, [&](auto N) {
        hipLaunchKernelGGL((k_gs_planes<decltype(N)::value>), grid, block, 0, s, lu, u, lf, rhs, lc, sd, w, p, p.tmin + t, count);
      });
      EXAMG_CHECK_LAUNCH("k_gs_planes");
    }
    return 0;
  }
  const size_t lds = ((size_t)p.lds_doubles() + GS_LANES * (GS_TT + 1)) * sizeof(double);
  const dim3 grid((unsigned)p.NY, (unsigned)p.NZ), block(GS_LANES);
  for (int tt = 0; tt < p.tile_times(); ++tt) {
    auto tile = [&](auto TY, auto N) {
      if (st->cfield) hipLaunchKernelGGL((k_gs_tile<decltype(TY)::value, decltype(N)::value, true>), grid, block, lds, s, lu, u, lf, rhs, lc, sd, w, p, tt, lu_->nd);
      else hipLaunchKernelGGL((k_gs_tile<decltype(TY)::value, decltype(N)::value, false>), grid, block, lds, s, lu, u, lf, rhs, lc, sd, w, p, tt, lu_->nd);
    };
    if (lu_->nd == 3) with_nent3(st->nent, [&](auto N) { tile(std::integral_constant<int, GS_TY3>{}, N); });
    else with_nent2(st->nent, [&](auto N) { tile(std::integral_constant<int, GS_LANES>{}, N); });
    EXAMG_CHECK_LAUNCH("k_gs_tile");
  }
  return 0;
}
