// Table-coefficient stencil loops on gfx950: operators on axis-aligned non-uniform grids (examg_axis_op).
//
// On an axis-aligned grid (grid_isUniform = false, grid_isAxisAligned = true; grid/ir/IR_SetupNodePositions.scala) a discretised
// operator depends on the position through one-dimensional tables only: every coefficient is a short sum of terms
// X_t[i0] * ((s_t * Z_t[i2]) * Y_t[i1]).  The kernels form the coefficients of a point from the tables (a few KB, cache resident) instead
// of reading one 8-byte stream per entry: u, rhs and dst are the only streams (24 B per point against 80 B for a 7-entry stencil field).
// The arithmetic order is fixed in include/examg.h; this file is compiled with contraction off.
//
// Two kernels that compute the same bits.  k_axis_generic: any stencil of reach 1 in 2-D and 3-D, a lane owns one point (of the
// colour); a workgroup is 64 x points by 4 rows, and stages in LDS what its points share: the window of every term's X table and the
// row products (s * Z) * Y of its four rows.  k_axis_star: 3-D star stencils of at most AXIS_STAR_TERMS terms, in the shape of
// k_stencil7_zmarch (kernels_stencil.hip) -- a wave owns 128 x points (two per lane) of one row and marches in z with the register
// pipeline u[z-1], u[z], u[z+1]; the X tables of the window are loaded into registers once before the march, the row products are
// wave-uniform (the row index is read through readfirstlane, the tables through scalar loads).
// Measured at 512^3 (tools/axis_bench.py, profiles/axis_bench.json): Jacobi step 2.01 ms (star), 2.03 ms (generic), 2.87 ms for the same
// operator as a 7-entry stencil field, 0.58 ms for the constant-coefficient kernel -- not bound by bytes.
#include "examg_common.h"

namespace examg {

constexpr int AXIS_STAR_TERMS = 12;      // the 7-point operators of the finite-difference and finite-volume programs: 6 + 6 terms

struct AxisArgs {
  LayoutDev lu, lf, ld;
  const double *u, *rhs;
  double *dst;
  int nent, diag, nterm, wdiv;
  long long uo[EXAMG_MAX_ENTRIES];       // linear offsets of the entries in the u layout
  int tend[EXAMG_MAX_ENTRIES];           // one past the last term of entry k (terms are sorted by entry)
  int code[8];                           // star kernel: what entry k multiplies (0 centre, 1 + 2d lower, 2 + 2d upper neighbour in d)
  int tab[EXAMG_AXIS_MAX_TERMS][3];
  double s[EXAMG_AXIS_MAX_TERMS];
  const double *tables[3];               // per axis: table t at tables[d] + t * tlen[d]; element 0 is iterator index tbeg[d]
  int tbeg[3], tlen[3];
  double w;
  int colour;
  Box box;
};

template <int MODE>
__device__ __forceinline__ double axis_finish(const AxisArgs &a, double uc, double acc, double f, double dg) {
  if (MODE == EXAMG_APPLY) return acc;
  if (MODE == EXAMG_RESIDUAL) return f - acc;
  const double ww = a.wdiv ? a.w / dg : (1.0 / dg) * a.w;
  return uc + ww * (f - acc);
}

// ---- generic: one lane per point, 64 x points by 4 rows per workgroup ---------------------------------------------------------------
constexpr int AXIS_ROWS = 4;

template <int MODE>
__global__ void __launch_bounds__(64 * AXIS_ROWS) k_axis_generic(AxisArgs a, int ntx, int nty) {
  extern __shared__ double lds[];
  const Box box = a.box;
  const int span = a.colour >= 0 ? 128 : 64;         // x indices a workgroup's window covers
  double *sx = lds;                                  // [nterm][span]: X_t over the window, 1.0 for an absent table and past the box
  double *sr = lds + a.nterm * span;                 // [AXIS_ROWS][nterm]: (s_t * Z_t[i2]) * Y_t[i1]
  int t = blockIdx.x;
  const int tx = t % ntx;
  t /= ntx;
  const int ty = t % nty, pz = t / nty;
  const int lane = threadIdx.x, r = threadIdx.y, tid = r * 64 + lane;
  const int i2 = box.b2 + pz, row0 = box.b1 + ty * AXIS_ROWS;
  const int x0 = box.b0 + tx * span;
  for (int j = tid; j < a.nterm * span; j += 64 * AXIS_ROWS) {
    const int tt = j / span, x = x0 + (j - tt * span);
    double v = 1.0;
    if (a.tab[tt][0] >= 0 && x < box.e0) v = a.tables[0][(long long)a.tab[tt][0] * a.tlen[0] + (x - a.tbeg[0])];
    sx[j] = v;
  }
  for (int j = tid; j < a.nterm * AXIS_ROWS; j += 64 * AXIS_ROWS) {
    const int rr = j / a.nterm, tt = j - rr * a.nterm, i1 = row0 + rr;
    double v = 1.0;
    if (i1 < box.e1) {
      v = a.s[tt];
      if (a.tab[tt][2] >= 0) v = v * a.tables[2][(long long)a.tab[tt][2] * a.tlen[2] + (i2 - a.tbeg[2])];
      if (a.tab[tt][1] >= 0) v = v * a.tables[1][(long long)a.tab[tt][1] * a.tlen[1] + (i1 - a.tbeg[1])];
    }
    sr[j] = v;
  }
  __syncthreads();
  const int i1 = row0 + r;
  int i0 = x0 + lane;
  if (a.colour >= 0) i0 = x0 + (((box.b0 + i1 + i2) & 1) != a.colour ? 1 : 0) + 2 * lane;      // x0 - box.b0 is even
  if (i1 >= box.e1 || i0 >= box.e0) return;
  const double *xs = sx + (i0 - x0);
  const double *rs = sr + r * a.nterm;
  const long long iu = lidx_plain(a.lu, i0, i1, i2);
  const double *up = a.u + iu;
  double acc = 0.0, dg = 0.0;
  int tt = 0;
  for (int k = 0; k < a.nent; ++k) {
    double c = xs[tt * span] * rs[tt];
    for (++tt; tt < a.tend[k]; ++tt) c = c + xs[tt * span] * rs[tt];
    if (k == a.diag) dg = c;
    const double p = c * up[a.uo[k]];
    acc = k == 0 ? p : acc + p;
  }
  const double f = MODE == EXAMG_APPLY ? 0.0 : a.rhs[lidx_plain(a.lf, i0, i1, i2)];
  a.dst[lidx_plain(a.ld, i0, i1, i2)] = axis_finish<MODE>(a, up[0], acc, f, dg);
}

// ---- 3-D star stencils: 128 x points of one row per wave, z march ------------------------------------------------------------------
__device__ __forceinline__ double axis_pick(int code, double c, double xm, double xp, double ym, double yp, double zm, double zp) {
  return code == 0 ? c : (code == 1 ? xm : (code == 2 ? xp : (code == 3 ? ym : (code == 4 ? yp : (code == 5 ? zm : zp)))));
}

template <int MODE>
__global__ void __launch_bounds__(64 * AXIS_ROWS) k_axis_star(AxisArgs a, int ntx, int nty, int zc) {
  const Box box = a.box;
  const int lane = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
  int t = blockIdx.x;
  const int tx = t % ntx;
  t /= ntx;
  const int ty = t % nty, tz = t / nty;
  const int row = box.b1 + ty * AXIS_ROWS + wv;      // wave-uniform, in scalar registers
  if (row >= box.e1) return;
  const int x = box.b0 + tx * 128 + 2 * lane;
  const int mb = box.b2 + tz * zc, me = min(mb + zc, box.e2);
  const bool va = x < box.e0, vb = x + 1 < box.e0;
  const bool lload = va && lane == 0, rload = vb && (lane == 63 || x + 2 >= box.e0);
  const int xs = va ? x : box.b0;                    // idle lanes work on the row's first pair and store nothing

  // the X tables of the window, in registers for the whole march; per term, wave-uniform: s, the Y factor of this row, the Z table and
  // what the fold does with the term (first / last of its entry, the entry's code, the diagonal) -- read from the kernel arguments once,
  // so that the march reads no argument through a run-time index
  double xa[AXIS_STAR_TERMS], xb[AXIS_STAR_TERMS], yv[AXIS_STAR_TERMS], sv[AXIS_STAR_TERMS];
  const double *zt[AXIS_STAR_TERMS];
  int meta[AXIS_STAR_TERMS];      // bit 0: first term of its entry, bit 1: last, bit 2: the diagonal entry, bits 4..6: the entry's code
  int k = 0;
#pragma unroll
  for (int tt = 0; tt < AXIS_STAR_TERMS; ++tt) {
    xa[tt] = 1.0;
    xb[tt] = 1.0;
    yv[tt] = 1.0;
    sv[tt] = 1.0;
    zt[tt] = nullptr;
    meta[tt] = 0;
    if (tt < a.nterm) {
      if (a.tab[tt][0] >= 0) {
        const double *p = a.tables[0] + (long long)a.tab[tt][0] * a.tlen[0] - a.tbeg[0];
        if (va) xa[tt] = p[x];
        if (vb) xb[tt] = p[x + 1];
      }
      if (a.tab[tt][1] >= 0) yv[tt] = a.tables[1][(long long)a.tab[tt][1] * a.tlen[1] + (row - a.tbeg[1])];
      if (a.tab[tt][2] >= 0) zt[tt] = a.tables[2] + (long long)a.tab[tt][2] * a.tlen[2] - a.tbeg[2];
      sv[tt] = a.s[tt];
      const bool first = tt == 0 || tt == a.tend[k == 0 ? 0 : k - 1], last = tt + 1 == a.tend[k];
      meta[tt] = (first ? 1 : 0) | (last ? 2 : 0) | (k == a.diag ? 4 : 0) | (a.code[k] << 4);
      if (last) ++k;
    }
  }
  const double *ur = a.u + a.lu.origin + xs + a.lu.s1 * row;
  const double *fr = a.rhs + a.lf.origin + xs + a.lf.s1 * row;
  double *dr = a.dst + a.ld.origin + xs + a.ld.s1 * row;
  // one pipeline stage = everything step m needs from memory: the loads of step m + 1 are in flight while step m is computed
  struct Stage {
    d2 up, ym, yp, f;
    double el, er;
    double rv[AXIS_STAR_TERMS];      // (s * Z[m]) * Y[row]
  };
  auto load_stage = [&](Stage &g, int m) {
    const double *um_ = ur + a.lu.s2 * m;
    g.up = load2(um_ + a.lu.s2);
    g.ym = load2(um_ - a.lu.s1);
    g.yp = load2(um_ + a.lu.s1);
    g.f.x = 0.0;
    g.f.y = 0.0;
    if (MODE != EXAMG_APPLY) g.f = load2g(fr + a.lf.s2 * m, va, vb);
    g.el = 0.0;
    g.er = 0.0;
    if (lload) g.el = um_[-1];
    if (rload) g.er = um_[2];
#pragma unroll
    for (int tt = 0; tt < AXIS_STAR_TERMS; ++tt) {
      double rv = sv[tt];
      if (zt[tt]) rv = rv * zt[tt][m];
      g.rv[tt] = rv * yv[tt];
    }
  };
  d2 um = load2(ur + a.lu.s2 * (mb - 1)), uc = load2(ur + a.lu.s2 * mb);
  auto compute = [&](const Stage &g, int m) {
    double xl = lane_below(uc.y), xr = lane_above(uc.x);       // all 64 lanes take part
    if (lload) xl = g.el;
    if (rload) xr = g.er;
    double acc_a = 0.0, acc_b = 0.0, ca = 0.0, cb = 0.0, dga = 0.0, dgb = 0.0;
#pragma unroll
    for (int tt = 0; tt < AXIS_STAR_TERMS; ++tt) {
      if (tt < a.nterm) {                                      // uniform: the term list is a kernel argument
        const double ta = xa[tt] * g.rv[tt], tb = xb[tt] * g.rv[tt];
        const int mt = meta[tt];
        ca = (mt & 1) ? ta : ca + ta;
        cb = (mt & 1) ? tb : cb + tb;
        if (mt & 2) {                                          // the entry's coefficient is complete
          const int cd = mt >> 4;
          const double pa = ca * axis_pick(cd, uc.x, xl, uc.y, g.ym.x, g.yp.x, um.x, g.up.x);
          const double pb = cb * axis_pick(cd, uc.y, uc.x, xr, g.ym.y, g.yp.y, um.y, g.up.y);
          const bool e0 = tt + 1 == a.tend[0];                 // the first entry starts the fold
          acc_a = e0 ? pa : acc_a + pa;
          acc_b = e0 ? pb : acc_b + pb;
          if (mt & 4) {
            dga = ca;
            dgb = cb;
          }
        }
      }
    }
    const double oa = axis_finish<MODE>(a, uc.x, acc_a, g.f.x, dga), ob = axis_finish<MODE>(a, uc.y, acc_b, g.f.y, dgb);
    double *q = dr + a.ld.s2 * m;
    if (a.colour < 0) {
      if (va && vb) {
        d2 o;
        o.x = oa;
        o.y = ob;
        store2(q, o);
      } else if (va) {
        q[0] = oa;
      }
    } else if (((x + row + m) & 1) == a.colour) {      // the same parity in every lane: x - box.b0 is even
      if (va) q[0] = oa;
    } else if (vb) {
      q[1] = ob;
    }
    um = uc;
    uc = g.up;
  };
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

// The codes of a 3-D star stencil of reach 1 with the centre and every axis neighbour exactly once; false: not one
static bool axis_star_codes(const examg_axis_stencil_t *st, int (&code)[8]) {
  if (st->nent != 7) return false;
  unsigned seen = 0;
  for (int k = 0; k < 7; ++k) {
    int nz = 0, cd = 0;
    for (int d = 0; d < 3; ++d) {
      const int o = st->off[k][d];
      if (o == 0) continue;
      ++nz;
      cd = 1 + 2 * d + (o > 0 ? 1 : 0);
    }
    if (nz > 1 || (seen & (1u << cd))) return false;
    seen |= 1u << cd;
    code[k] = cd;
  }
  return true;
}

static bool axis_plain_node(const char *who, const char *what, const examg_layout_t *l, int nd) {
  if (l->nd != nd) { set_error("%s: the %s layout has %d dimensions, u has %d", who, what, l->nd, nd); return false; }
  if (l->transform != EXAMG_LAYOUT_PLAIN) { set_error("%s: the %s layout is under a layout transformation; the table kernels take plain layouts only", who, what); return false; }
  return true;
}

// Every check of examg_axis_op; the route in *route (EXAMG_AXIS_GENERIC / EXAMG_AXIS_STAR), 0 for an empty box.  false: refused.
static bool axis_check(const char *who, int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs,
                       const examg_layout_t *ld, const double *dst, const examg_axis_stencil_t *st, int colour, const int32_t *begin,
                       const int32_t *end, bool pointers, int *route) {
  *route = 0;
  if (!lu || !ld || !st || !begin || !end || (pointers && (!u || !dst))) { set_error("%s: null argument", who); return false; }
  if (mode < 0 || mode > 2) { set_error("%s: bad mode %d", who, mode); return false; }
  if (mode != EXAMG_APPLY && (!lf || (pointers && !rhs))) { set_error("%s: rhs required for mode %d", who, mode); return false; }
  const int nd = lu->nd;
  if (nd != 2 && nd != 3) { set_error("%s: 2-D or 3-D layouts (nd = %d)", who, nd); return false; }
  if (!axis_plain_node(who, "u", lu, nd) || !axis_plain_node(who, "dst", ld, nd)) return false;
  if (mode != EXAMG_APPLY && !axis_plain_node(who, "rhs", lf, nd)) return false;
  if (st->nent < 1 || st->nent > EXAMG_MAX_ENTRIES) { set_error("%s: nent %d out of range", who, st->nent); return false; }
  if (st->nterm < st->nent || st->nterm > EXAMG_AXIS_MAX_TERMS) {
    set_error("%s: %d terms for %d entries (every entry has one, at most %d in all)", who, st->nterm, st->nent, EXAMG_AXIS_MAX_TERMS);
    return false;
  }
  if (st->wform != EXAMG_WEIGHT_INV_TIMES && st->wform != EXAMG_WEIGHT_DIVIDE) { set_error("%s: bad weight form %d", who, st->wform); return false; }
  if (st->route < EXAMG_AXIS_AUTO || st->route > EXAMG_AXIS_STAR) { set_error("%s: bad route %d", who, st->route); return false; }
  if (st->diag < 0 || st->diag >= st->nent || st->off[st->diag][0] != 0 || st->off[st->diag][1] != 0 || st->off[st->diag][2] != 0) {
    set_error("%s: the stencil has no centre entry (diag = %d)", who, st->diag);
    return false;
  }
  for (int k = 0; k < st->nent; ++k)
    for (int d = 0; d < 3; ++d) {
      const int o = st->off[k][d];
      if (o < -1 || o > 1) { set_error("%s: stencil entry %d reaches further than one point", who, k); return false; }
      if (d >= nd && o != 0) { set_error("%s: stencil entry %d leaves the %d dimensions of the layouts", who, k, nd); return false; }
    }
  bool used[3] = {false, false, false};
  for (int t = 0, prev = 0; t < st->nterm; ++t) {
    const int e = st->term[t].entry;
    if (e < 0 || e >= st->nent || e < prev || e > prev + 1 || (t == 0 && e != 0)) {
      set_error("%s: term %d names entry %d: the terms are sorted by entry and every entry has one", who, t, e);
      return false;
    }
    prev = e;
    if (t == st->nterm - 1 && e != st->nent - 1) { set_error("%s: entry %d has no term", who, st->nent - 1); return false; }
    for (int d = 0; d < 3; ++d) {
      const int tb = st->term[t].tab[d];
      if (tb < -1 || tb >= st->ntab[d] || (tb >= 0 && d >= nd)) { set_error("%s: term %d names table %d of axis %d (%d tables)", who, t, tb, d, st->ntab[d]); return false; }
      if (tb >= 0) used[d] = true;
    }
  }
  for (int d = 0; d < 3; ++d)
    if (used[d] && (!st->tables[d] || st->tab_len[d] < 1)) { set_error("%s: axis %d has no tables", who, d); return false; }
  if (colour < -1 || colour > 1) { set_error("%s: colour must be -1, 0 or 1", who); return false; }
  if (pointers && dst == u && colour < 0) { set_error("%s: dst is u; only a coloured loop runs in place", who); return false; }
  const Box box = make_box(begin, end);
  if (box.count() == 0) return true;
  if (nd == 2 && (box.b2 != 0 || box.e2 != 1)) { set_error("%s: 2-D box must have [0,1) in dim 2", who); return false; }
  if (!box_inside(lu, box, 1)) { set_error("%s: the one-point shell of the box leaves the u allocation", who); return false; }
  if (!box_inside(ld, box, 0)) { set_error("%s: box leaves the dst allocation", who); return false; }
  if (mode != EXAMG_APPLY && !box_inside(lf, box, 0)) { set_error("%s: box leaves the rhs allocation", who); return false; }
  const int bb[3] = {box.b0, box.b1, box.b2}, ee[3] = {box.e0, box.e1, box.e2};
  for (int d = 0; d < nd; ++d)
    if (used[d] && (bb[d] < st->tab_begin[d] || (long long)ee[d] > (long long)st->tab_begin[d] + st->tab_len[d])) {
      set_error("%s: the tables of axis %d cover [%d, %lld), the box needs [%d, %d)", who, d, st->tab_begin[d],
                (long long)st->tab_begin[d] + st->tab_len[d], bb[d], ee[d]);
      return false;
    }
  int code[8];
  const bool star = nd == 3 && st->nterm <= AXIS_STAR_TERMS && axis_star_codes(st, code);
  if (st->route == EXAMG_AXIS_STAR && !star) {
    set_error("%s: the star route takes 3-D stencils of the centre and the six axis neighbours with at most %d terms", who, AXIS_STAR_TERMS);
    return false;
  }
  *route = (star && st->route != EXAMG_AXIS_GENERIC) ? EXAMG_AXIS_STAR : EXAMG_AXIS_GENERIC;
  return true;
}

}  // namespace examg

using namespace examg;

extern "C" int examg_axis_route(int mode, const examg_layout_t *lu, const examg_layout_t *lf, const examg_layout_t *ld, const examg_axis_stencil_t *st,
                                int colour, const int32_t *begin, const int32_t *end) {
  int route = 0;
  if (!axis_check("examg_axis_route", mode, lu, nullptr, lf, nullptr, ld, nullptr, st, colour, begin, end, false, &route)) return -1;
  return route;
}

extern "C" int examg_axis_op(int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs,
                             const examg_layout_t *ld, double *dst, const examg_axis_stencil_t *st, double w, int colour, const int32_t *begin,
                             const int32_t *end, examg_stream_t stream) {
  const char *who = "examg_axis_op";
  int route = 0;
  if (!axis_check(who, mode, lu, u, lf, rhs, ld, dst, st, colour, begin, end, true, &route)) return 1;
  if (route == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  AxisArgs a;
  memset(&a, 0, sizeof(a));
  a.lu = make_layout(lu);
  a.ld = make_layout(ld);
  a.lf = mode != EXAMG_APPLY ? make_layout(lf) : a.ld;
  a.u = u;
  a.rhs = mode != EXAMG_APPLY ? rhs : u;
  a.dst = dst;
  a.nent = st->nent;
  a.diag = st->diag;
  a.nterm = st->nterm;
  a.wdiv = st->wform == EXAMG_WEIGHT_DIVIDE ? 1 : 0;
  for (int k = 0; k < EXAMG_MAX_ENTRIES; ++k)
    a.uo[k] = k < st->nent ? st->off[k][0] + a.lu.s1 * st->off[k][1] + a.lu.s2 * st->off[k][2] : 0;
  for (int t = 0; t < st->nterm; ++t) {
    a.tend[st->term[t].entry] = t + 1;
    a.s[t] = st->term[t].s;
    for (int d = 0; d < 3; ++d) a.tab[t][d] = st->term[t].tab[d];
  }
  for (int d = 0; d < 3; ++d) {
    a.tables[d] = st->tables[d];
    a.tbeg[d] = st->tab_begin[d];
    a.tlen[d] = st->tab_len[d];
  }
  a.w = w;
  a.colour = colour;
  a.box = make_box(begin, end);
  const Box &box = a.box;
  const dim3 blk(64, AXIS_ROWS);
  const int nty = (box.n1() + AXIS_ROWS - 1) / AXIS_ROWS;
  if (route == EXAMG_AXIS_STAR) {
    int code[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    axis_star_codes(st, code);
    for (int k = 0; k < 8; ++k) a.code[k] = code[k];
    const int ntx = (box.n0() + 127) / 128;
    // z chunks: enough workgroups to fill the chip (256 CUs, two workgroups each), chunks of at least 8 planes
    int zc = box.n2();
    const long long per_layer = (long long)ntx * nty;
    if (per_layer < 512) {
      const long long want = (512 + per_layer - 1) / per_layer;
      zc = (int)((box.n2() + want - 1) / want);
      if (zc < 8) zc = 8;
      if (zc > box.n2()) zc = box.n2();
    }
    const int ntz = (box.n2() + zc - 1) / zc;
    const long long nb = per_layer * ntz;
    if (nb > 0x7fffffffLL) { set_error("%s: grid too large", who); return 1; }
    with_mode(mode, [&](auto M) { hipLaunchKernelGGL((k_axis_star<decltype(M)::value>), dim3((unsigned)nb), blk, 0, s, a, ntx, nty, zc); });
    EXAMG_CHECK_LAUNCH("k_axis_star");
    return 0;
  }
  const int span = colour >= 0 ? 128 : 64;
  const int ntx = (box.n0() + span - 1) / span;
  const long long nb = (long long)ntx * nty * box.n2();
  if (nb > 0x7fffffffLL) { set_error("%s: grid too large", who); return 1; }
  const size_t shmem = sizeof(double) * (size_t)st->nterm * (span + AXIS_ROWS);
  with_mode(mode, [&](auto M) { hipLaunchKernelGGL((k_axis_generic<decltype(M)::value>), dim3((unsigned)nb), blk, shmem, s, a, ntx, nty); });
  EXAMG_CHECK_LAUNCH("k_axis_generic");
  return 0;
}
