// What the kernels of the coupled cell systems (kernels_system.hip) and of the vector-valued cell fields (kernels_vector.hip) share:
// the pair loads, the wave's coordinates, the pick of a stencil entry's value, the local solves, the layout checks.
#pragma once
#include "examg_common.h"

namespace examg {

constexpr int SYS_MAXN = EXAMG_SYS_MAX;

template <bool VEC>
__device__ __forceinline__ d2 sys_load_pair(const double *p) {
  d2 r;
  if (VEC) {
    r = *reinterpret_cast<const d2 *>(p);
  } else {
    r.x = p[0];
    r.y = p[1];
  }
  return r;
}
// the pair where both cells may be read, one value at an end of the box, 0 outside
template <bool VEC>
__device__ __forceinline__ d2 sys_load_pair_g(const double *p, bool oka, bool okb) {
  d2 r = {0.0, 0.0};
  if (oka && okb) return sys_load_pair<VEC>(p);
  if (oka) r.x = p[0];
  else if (okb) r.y = p[1];
  return r;
}

// the value an entry multiplies: 0 centre, 1 + 2d the lower, 2 + 2d the upper neighbour in d
__device__ __forceinline__ double sys_pick(int code, double c, double xm, double xp, double ym, double yp, double zm, double zp) {
  switch (code) {
    case 0: return c;
    case 1: return xm;
    case 2: return xp;
    case 3: return ym;
    case 4: return yp;
    case 5: return zm;
    default: return zp;
  }
}

// wave -> (x tile, row, plane) of the box; false: nothing to do for this wave (uniform)
__device__ __forceinline__ bool sys_wave_coords(const Box &box, int xo, int ntx, int &x, int &row, int &plane) {
  const int nry = (box.n1() + 3) >> 2;
  const int wpl = ntx * nry;
  const long long wg = xcd_band(blockIdx.x, wpl);
  const long long lz = wg / wpl;
  const int r = (int)(wg - lz * wpl);
  const int tx = r % ntx;
  const int jw = (r / ntx) * 4 + (int)__builtin_amdgcn_readfirstlane(threadIdx.y);
  x = xo + tx * 128 + 2 * (int)threadIdx.x;
  row = box.b1 + jw;
  plane = box.b2 + (int)lz;
  return jw < box.n1();
}

// ---- the local solve of one cell ------------------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void sys_solve(const double (&m)[N * N], const double (&b)[N], double (&xs)[N]);

// include/examg.h: examg_sys_relax, n = 2
template <>
__device__ __forceinline__ void sys_solve<2>(const double (&m)[4], const double (&b)[2], double (&xs)[2]) {
  const double det = m[0] * m[3] - m[1] * m[2];
  xs[0] = (b[0] * m[3] - m[1] * b[1]) / det;
  xs[1] = (m[0] * b[1] - m[2] * b[0]) / det;
}
// n = 3: cofactors k_ij of a_ij, the determinant along the first row, x_i = ((k_0i * b_0 + k_1i * b_1) + k_2i * b_2) / det
template <>
__device__ __forceinline__ void sys_solve<3>(const double (&m)[9], const double (&b)[3], double (&xs)[3]) {
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

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
static bool sys_layout_ok(const char *who, const char *what, const examg_layout_t *l, int nd) {
  if (l->nd != nd) { set_error("%s: the %s layout has %d dimensions, the unknowns %d", who, what, l->nd, nd); return false; }
  for (int d = 0; d < l->nd; ++d)
    if (l->dup_l[d] != 0 || l->dup_r[d] != 0) { set_error("%s: the %s layout is not a cell layout (duplicate layers in dim %d)", who, what, d); return false; }
  if (lay_split(l)) { set_error("%s: the %s layout is colour-split; systems take plain layouts only", who, what); return false; }
  return true;
}

// pairs (xo + 2j, xo + 2j + 1) of every row of the array at p are 16-byte aligned
static bool pairs_even(const LayoutDev &d, int nd, const void *p, int xo) {
  return ((uintptr_t)p & 15) == 0 && ((d.origin + xo) & 1) == 0 && (d.s1 & 1) == 0 && (nd < 3 || (d.s2 & 1) == 0);
}

// an axis entry of reach 1 of an nd-dimensional cell field -> its code for sys_pick; -1: not such an entry
static inline int sys_entry_code(const int32_t *off, int nd) {
  int nz = 0, code = 0;
  for (int d = 0; d < 3; ++d) {
    const int o = off[d];
    if (o == 0) continue;
    ++nz;
    if (d >= nd || o < -1 || o > 1) nz = 9;
    code = 1 + 2 * d + (o > 0 ? 1 : 0);
  }
  return nz > 1 ? -1 : code;
}

}  // namespace examg
