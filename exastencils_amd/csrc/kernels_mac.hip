// Staggered grids on gfx950: velocities on the faces of the cells, the pressure in the cells (`Layout X< Real, Face_x >`), the three-field
// operator of a Stokes problem and the box ("Vanka") smoother that solves for a cell's pressure and its 2 * nd face velocities at once.
//
// Reference: Examples/Stokes/2D_FV_Stokes_fromL4.exa4:588-601 (`color with { i0 % 3, i1 % 3, loop over p { solve locally relax w { .. } } }`),
// solver/ir/IR_LocalSolve.scala, IR_LocalDirectInvert.scala:78-139; face layouts fieldlike/l4/L4_FieldLikeLayoutDecl.scala:53-57; transfer
// stencils operator/l4/L4_DefaultRestriction.scala:63-82; boundary rules boundary/ir/IR_BoundaryCondition.scala:38-45.  The arithmetic
// order is fixed in include/examg.h; this file is compiled with contraction off.
//
// Access pattern: every kernel gives a lane one point and runs x fastest across the lanes.
//   k_mac_op     blockIdx.y is the row (wave-uniform: the stencil entries and the arrays of the row come through scalar loads); the 64
//                lanes of a wave read 64 consecutive doubles of a row of u_d for every entry and of p for the gradient.
//   k_mac_relax  the cells of ONE colour, enumerated densely (the lattice of examg_common.h: make_colour): consecutive lanes are
//                consecutive cells of the colour in x, three cells apart.  A lane reads the star of both faces of its cell on every
//                axis (the x pair lies in the lane's own 24 bytes of the row; the lines are shared with the lanes beside it), eliminates
//                in registers and stores 2 * nd + 1 values.  The host has checked that no cell within reach is of the lane's colour: the
//                loop is race-free in place.  No LDS, no scratch, no allocation.
//   transfers    one coarse (restriction) or fine (prolongation) point per lane.
#include <limits.h>

#include "examg_common.h"

namespace examg {

constexpr int MAC_MAXE = 7;      // the centre and two neighbours per axis

struct MacStar {
  int nent;
  int off[MAC_MAXE];             // linear offsets in the layout of the unknown
  double coef[MAC_MAXE];
};

struct MacArgs {
  double *u[3], *p;
  const double *f[3], *fp;
  double *dst[3], *dstp;
  LayoutDev lu[3], lp, lf[3], lfp, ld[3], ldp;
  MacStar A[3];                  // k_mac_op: all entries of A_d
  MacStar RL[3], RU[3];          // k_mac_relax: the entries of A_d that go to the right-hand side of the lower / the upper face's row
  double a[3], q[3], m[3];       // k_mac_relax: centre, the +e_d entry (0.0: none), the -e_d entry
  double bc[3], bm[3], cc[3], cp[3];
  long long ustep[3], fstep[3], pstep[3];      // one step along axis d in lu[d], lf[d], lp
  int n[3];                      // cells per axis
};

struct MacBoxes {
  Box box[4];
};

__device__ __forceinline__ void mac_unflatten(const Box &b, long long t, int &i0, int &i1, int &i2) {
  const int n0 = b.n0(), n1 = b.n1();
  const long long r = t / n0;
  i0 = b.b0 + (int)(t - r * n0);
  i1 = b.b1 + (int)(r % n1);
  i2 = b.b2 + (int)(r / n1);
}

// the entries of S folded left to right about the point `at` (S.nent >= 1)
__device__ __forceinline__ double mac_fold(const MacStar &S, const double *__restrict__ u, long long at) {
  double acc = S.coef[0] * u[at + S.off[0]];
  for (int k = 1; k < S.nent; ++k) acc = acc + S.coef[k] * u[at + S.off[k]];
  return acc;
}
// ... with `tail` joined as the last term; a star without entries is the tail alone
__device__ __forceinline__ double mac_fold_tail(const MacStar &S, const double *u, long long at, double tail) {
  if (S.nent == 0) return tail;      // uniform
  return mac_fold(S, u, at) + tail;
}

// ---- dst_r = [f_r -] row r of the operator, all rows of the mask in one launch ------------------------------------------------------------
template <int ND>
__global__ void __launch_bounds__(256) k_mac_op(MacArgs a, int mode, unsigned mask, MacBoxes bx) {
  const int r = blockIdx.y;
  if (!((mask >> r) & 1u)) return;
  const Box box = bx.box[r];
  const long long total = box.count();
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    int i0, i1, i2;
    mac_unflatten(box, t, i0, i1, i2);
    const long long ip = lidx_plain(a.lp, i0, i1, i2);
    if (r == ND) {
      double acc = 0.0;
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const long long iu = lidx_plain(a.lu[d], i0, i1, i2);
        const double lo = a.cc[d] * a.u[d][iu];
        const double hi = a.cp[d] * a.u[d][iu + a.ustep[d]];
        acc = d == 0 ? lo : acc + lo;
        acc = acc + hi;
      }
      const long long id = lidx_plain(a.ldp, i0, i1, i2);
      a.dstp[id] = mode == EXAMG_SYS_RESIDUAL ? a.fp[lidx_plain(a.lfp, i0, i1, i2)] - acc : acc;
    } else {
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        if (r != d) continue;      // uniform
        const long long iu = lidx_plain(a.lu[d], i0, i1, i2);
        const double conv = mac_fold(a.A[d], a.u[d], iu);
        const double grad = (a.bc[d] * a.p[ip]) + (a.bm[d] * a.p[ip - a.pstep[d]]);
        const double v = conv + grad;
        const long long id = lidx_plain(a.ld[d], i0, i1, i2);
        a.dst[d][id] = mode == EXAMG_SYS_RESIDUAL ? a.f[d][lidx_plain(a.lf[d], i0, i1, i2)] - v : v;
      }
    }
  }
}

// ---- the local solves of one colour, in place -----------------------------------------------------------------------------------------------
template <int ND>
__global__ void __launch_bounds__(256) k_mac_relax(MacArgs a, double relax, MCColour col) {
  const long long total = mc_threads(col);
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long row = t / col.row_w;
    int i1, i2;
    mc_row(col, row, i1, i2);
    const int i0 = col.first[0] + col.step[0] * (int)(t - row * col.row_w);
    const int idx[3] = {i0, i1, i2};
    const long long ip = lidx_plain(a.lp, i0, i1, i2);
    double y0[ND], y1[ND], z0[ND], z1[ND], old0[ND], old1[ND];
    long long at[ND];
    bool h0[ND], h1[ND];
    double sy = 0.0, sz = 0.0;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      const double *ud = a.u[d];
      const long long iu = lidx_plain(a.lu[d], i0, i1, i2), iv = iu + a.ustep[d];
      const long long jf = lidx_plain(a.lf[d], i0, i1, i2);
      const double tl = mac_fold_tail(a.RL[d], ud, iu, a.bm[d] * a.p[ip - a.pstep[d]]);
      const double tu = mac_fold_tail(a.RU[d], ud, iv, a.bc[d] * a.p[ip + a.pstep[d]]);
      const double rl = a.f[d][jf] - tl, ru = a.f[d][jf + a.fstep[d]] - tu;
      at[d] = iu;
      old0[d] = ud[iu];
      old1[d] = ud[iv];
      h0[d] = idx[d] == 0;                 // the lower face lies on the boundary: held
      h1[d] = idx[d] + 1 == a.n[d];        // the upper one
      const double a00 = h0[d] ? 1.0 : a.a[d], a01 = h0[d] ? 0.0 : a.q[d], c0 = h0[d] ? 0.0 : a.bc[d], r0 = h0[d] ? old0[d] : rl;
      const double a11 = h1[d] ? 1.0 : a.a[d], a10 = h1[d] ? 0.0 : a.m[d], c1 = h1[d] ? 0.0 : a.bm[d], r1 = h1[d] ? old1[d] : ru;
      const double det = a00 * a11 - a01 * a10;
      y0[d] = (r0 * a11 - a01 * r1) / det;
      y1[d] = (a00 * r1 - a10 * r0) / det;
      z0[d] = (c0 * a11 - a01 * c1) / det;
      z1[d] = (a00 * c1 - a10 * c0) / det;
      const double ty = a.cc[d] * y0[d], tz = a.cc[d] * z0[d];
      sy = d == 0 ? ty : sy + ty;
      sz = d == 0 ? tz : sz + tz;
      sy = sy + a.cp[d] * y1[d];
      sz = sz + a.cp[d] * z1[d];
    }
    const double pn = (sy - a.fp[lidx_plain(a.lfp, i0, i1, i2)]) / sz;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      const double x0 = y0[d] - z0[d] * pn, x1 = y1[d] - z1[d] * pn;
      double *ud = a.u[d];
      if (!h0[d]) ud[at[d]] = relax == 1.0 ? x0 : old0[d] + relax * (x0 - old0[d]);
      if (!h1[d]) ud[at[d] + a.ustep[d]] = relax == 1.0 ? x1 : old1[d] + relax * (x1 - old1[d]);
    }
    if (relax == 1.0) {
      a.p[ip] = pn;
    } else {
      const double po = a.p[ip];
      a.p[ip] = po + relax * (pn - po);
    }
  }
}

// ---- transfers of a face field of axis AX ----------------------------------------------------------------------------------------------------
// fc(I) = sum of wgt(o) * rf(fine point), the own axis -1, 0, +1 about 2I (weights 1/4, 1/2, 1/4), the other axes the children 2I, 2I + 1
// (1/2 each); x outermost, then y, then z.  w[k]: the weight of own-axis offset k - 1 with `scale` and the other axes' halves folded in.
template <int ND>
__global__ void __launch_bounds__(256)
k_restrict_face(int ax, LayoutDev lf, const double *__restrict__ rf, LayoutDev lc, double *__restrict__ fc, double w0, double w1, double w2, Box box) {
  const long long total = box.count();
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    int I[3];
    mac_unflatten(box, t, I[0], I[1], I[2]);
    int lo[3], cnt[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      lo[d] = d >= ND ? 0 : (d == ax ? 2 * I[d] - 1 : 2 * I[d]);
      cnt[d] = d >= ND ? 1 : (d == ax ? 3 : 2);
    }
    double acc = 0.0;
    bool first = true;
    for (int x = 0; x < cnt[0]; ++x)
      for (int y = 0; y < cnt[1]; ++y)
        for (int z = 0; z < cnt[2]; ++z) {
          const int own = ax == 0 ? x : (ax == 1 ? y : z);
          const double wt = own == 0 ? w0 : (own == 1 ? w1 : w2);
          const double term = wt * rf[lidx_plain(lf, lo[0] + x, lo[1] + y, lo[2] + z)];
          acc = first ? term : acc + term;
          first = false;
        }
    fc[lidx_plain(lc, I[0], I[1], I[2])] = acc;
  }
}

// uf(i) = uf(i) + uc(parent) for an even own-axis index, uf(i) + ((0.5 * uc(upper)) + (0.5 * uc(lower))) for an odd one; the parent on the
// other axes is floor(i / 2)
template <int ND>
__global__ void __launch_bounds__(256)
k_prolong_add_face(int ax, LayoutDev lc, const double *__restrict__ uc, LayoutDev lf, double *__restrict__ uf, Box box) {
  const long long total = box.count();
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    int i[3];
    mac_unflatten(box, t, i[0], i[1], i[2]);
    const int c0 = i[0] >> 1, c1 = i[1] >> 1, c2 = ND == 3 ? i[2] >> 1 : 0;
    const int own = ax == 0 ? i[0] : (ax == 1 ? i[1] : i[2]);
    // the coarse point with v on the own axis
    auto coarse = [&](int v) { return uc[lidx_plain(lc, ax == 0 ? v : c0, ax == 1 ? v : c1, ax == 2 ? v : c2)]; };
    double add;
    if (own & 1) {
      const double up = 0.5 * coarse((own + 1) >> 1);
      add = up + 0.5 * coarse((own - 1) >> 1);
    } else {
      add = coarse(own >> 1);
    }
    double *q = uf + lidx_plain(lf, i[0], i[1], i[2]);
    *q = *q + add;
  }
}

// ---- apply bc of a face field ------------------------------------------------------------------------------------------------------------------
struct MacWalls {
  Box box[6];          // per wall: the faces it reads (cell rule: the boundary row) or writes (node rule: the boundary plane)
  int dim[6], up[6];
  long long start[7];
  int n;
};

// EXAMG_BC_DIRICHLET, one launch for every wall of the mask.  Walls normal to the field's axis: x = g (the node rule).  The others: the
// ghost one step outwards = 2.0 * g - interior (the cell rule).  dmask: the normal walls of the mask -- a boundary face of such a wall is
// read by the cell rule as the value the node rule gives it, whichever thread comes first.
__global__ void __launch_bounds__(256) k_dirichlet_bc_face(int ax, LayoutDev l, double *x, Geom g, ExprEval fn, MacWalls wl, int3 ncell, unsigned dmask) {
  const long long total = wl.start[wl.n];
  const double hh[3] = {g.h0, g.h1, g.h2}, pb[3] = {g.pb0, g.pb1, g.pb2};
  const int nc[3] = {ncell.x, ncell.y, ncell.z};
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    int f = 0;
    while (f + 1 < wl.n && t >= wl.start[f + 1]) ++f;
    int i[3];
    mac_unflatten(wl.box[f], t - wl.start[f], i[0], i[1], i[2]);
    const int d = wl.dim[f], up = wl.up[f];
    // the face's own position: the node position on the own axis, the cell centre on the others
    double p[3];
    for (int k = 0; k < 3; ++k) {
      p[k] = i[k] * hh[k] + pb[k];
      if (k != ax) p[k] = p[k] + 0.5 * hh[k];
    }
    if (d == ax) {
      x[lidx_plain(l, i[0], i[1], i[2])] = fn(p[0], p[1], p[2]);
      continue;
    }
    int o[3] = {i[0], i[1], i[2]};
    o[d] += up ? 1 : -1;
    double interior = x[lidx_plain(l, i[0], i[1], i[2])];
    if ((i[ax] == 0 && (dmask & 1u)) || (i[ax] == nc[ax] && (dmask & 2u))) interior = fn(p[0], p[1], p[2]);
    p[d] = (up ? nc[d] : 0) * hh[d] + pb[d];
    x[lidx_plain(l, o[0], o[1], o[2])] = (2.0 * fn(p[0], p[1], p[2])) - interior;
  }
}

// EXAMG_BC_NEUMANN: the cell rule alone (no wall of the mask is normal to the axis: host check), ghost = interior; no program, no geometry
__global__ void __launch_bounds__(256) k_neumann_bc_face(LayoutDev l, double *x, MacWalls wl) {
  const long long total = wl.start[wl.n];
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    int f = 0;
    while (f + 1 < wl.n && t >= wl.start[f + 1]) ++f;
    int i0, i1, i2;
    mac_unflatten(wl.box[f], t - wl.start[f], i0, i1, i2);
    const int d = wl.dim[f], s = wl.up[f] ? 1 : -1;
    x[lidx_plain(l, i0 + (d == 0 ? s : 0), i1 + (d == 1 ? s : 0), i2 + (d == 2 ? s : 0))] = x[lidx_plain(l, i0, i1, i2)];
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
// loc: -1 a cell layout, else the axis of a face layout.  n: the cells per axis (n[0] == 0: taken from this layout).
static bool mac_layout_ok(const char *who, const char *what, const examg_layout_t *l, int nd, int loc, int *n) {
  if (l->nd != nd) { set_error("%s: the %s layout has %d dimensions, the system %d", who, what, l->nd, nd); return false; }
  if (!staggered_layout_ok(who, what, l, loc)) return false;
  for (int d = 0; d < nd; ++d) {
    const int dup = d == loc ? 1 : 0;
    const int cells = l->inner[d] + dup;
    if (cells < 1) { set_error("%s: the %s layout has no cell in dim %d", who, what, d); return false; }
    if (n[d] == 0) n[d] = cells;
    if (cells != n[d]) { set_error("%s: the %s layout has %d cells in dim %d, the pressure %d", who, what, cells, d, n[d]); return false; }
  }
  return true;
}

static bool mac_ghost_ok(const char *who, const char *what, const examg_layout_t *l) {
  for (int d = 0; d < l->nd; ++d)
    if (l->ghost_l[d] < 1 || l->ghost_r[d] < 1) { set_error("%s: %s has no ghost layer in dim %d", who, what, d); return false; }
  return true;
}

static const char *const MAC_U[3] = {"u_0", "u_1", "u_2"};

// The checks the entry points share and the kernels' arguments.  rows: which rows' f (need_f) and dst (!relax) are looked at.
// 0: go on, 1: error (message set)
static int mac_prepare(const char *who, const examg_mac_t *sys, bool relax, bool need_f, unsigned rows, MacArgs &a) {
  if (!sys) { set_error("%s: null argument", who); return 1; }
  const int nd = sys->nd;
  if (nd != 2 && nd != 3) { set_error("%s: nd = %d; staggered systems are 2-D or 3-D", who, nd); return 1; }
  int n[3] = {0, 0, 0};
  char what[32];
  if (!mac_layout_ok(who, "pressure", &sys->lp, nd, -1, n) || !mac_ghost_ok(who, "the pressure", &sys->lp)) return 1;
  if (!sys->p) { set_error("%s: the pressure is a null pointer", who); return 1; }
  for (int d = 0; d < nd; ++d) {
    snprintf(what, sizeof what, "%s", MAC_U[d]);
    if (!mac_layout_ok(who, what, &sys->lu[d], nd, d, n) || !mac_ghost_ok(who, what, &sys->lu[d])) return 1;
    if (!sys->u[d]) { set_error("%s: %s is a null pointer", who, what); return 1; }
  }
  for (int r = 0; r <= nd; ++r) {
    if (!((rows >> r) & 1u)) continue;
    const int loc = r < nd ? r : -1;
    if (need_f) {
      snprintf(what, sizeof what, "rhs %d", r);
      if (!mac_layout_ok(who, what, r < nd ? &sys->lf[r] : &sys->lfp, nd, loc, n)) return 1;
      if (!(r < nd ? sys->f[r] : sys->fp)) { set_error("%s: right-hand side %d is a null pointer", who, r); return 1; }
    }
    if (!relax) {
      snprintf(what, sizeof what, "dst %d", r);
      if (!mac_layout_ok(who, what, r < nd ? &sys->ld[r] : &sys->ldp, nd, loc, n)) return 1;
      const double *dp = r < nd ? sys->dst[r] : sys->dstp;
      if (!dp) { set_error("%s: destination %d is a null pointer", who, r); return 1; }
      for (int c = 0; c <= nd; ++c) {
        if (dp == (c < nd ? sys->u[c] : sys->p)) { set_error("%s: destination %d is unknown %d; the operator does not run in place", who, r, c); return 1; }
        if (need_f && ((rows >> c) & 1u) && dp == (c < nd ? sys->f[c] : sys->fp)) {
          set_error("%s: destination %d is right-hand side %d; the rows are evaluated side by side", who, r, c);
          return 1;
        }
        if (c != r && ((rows >> c) & 1u) && dp == (c < nd ? sys->dst[c] : sys->dstp)) { set_error("%s: destinations %d and %d are one array", who, r, c); return 1; }
      }
    }
  }
  a.p = sys->p;
  a.fp = sys->fp;
  a.dstp = sys->dstp;
  a.lp = make_layout(&sys->lp);
  a.lfp = make_layout(&sys->lfp);
  a.ldp = make_layout(&sys->ldp);
  for (int d = 0; d < 3; ++d) {
    a.n[d] = d < nd ? n[d] : 1;
    a.u[d] = d < nd ? sys->u[d] : nullptr;
    a.f[d] = d < nd ? sys->f[d] : nullptr;
    a.dst[d] = d < nd ? sys->dst[d] : nullptr;
    a.lu[d] = make_layout(&sys->lu[d < nd ? d : 0]);
    a.lf[d] = make_layout(&sys->lf[d < nd ? d : 0]);
    a.ld[d] = make_layout(&sys->ld[d < nd ? d : 0]);
    a.bc[d] = sys->bc[d];
    a.bm[d] = sys->bm[d];
    a.cc[d] = sys->cc[d];
    a.cp[d] = sys->cp[d];
    a.a[d] = a.q[d] = a.m[d] = 0.0;
    const long long su[3] = {1, a.lu[d].s1, a.lu[d].s2}, sf[3] = {1, a.lf[d].s1, a.lf[d].s2}, sp[3] = {1, a.lp.s1, a.lp.s2};
    a.ustep[d] = su[d];
    a.fstep[d] = sf[d];
    a.pstep[d] = sp[d];
    MacStar *stars[3] = {&a.A[d], &a.RL[d], &a.RU[d]};
    for (MacStar *S : stars) {
      S->nent = 0;
      for (int k = 0; k < MAC_MAXE; ++k) {
        S->off[k] = 0;
        S->coef[k] = 0.0;
      }
    }
    if (d >= nd) continue;
    if (a.lu[d].s1 + a.lu[d].s2 + 1 > INT_MAX) { set_error("%s: the layout of %s is too large for 32-bit neighbour offsets", who, MAC_U[d]); return 1; }
    const examg_stencil_t *st = sys->A[d];
    if (!st) { set_error("%s: A_%d is a null pointer", who, d); return 1; }
    if (st->cfield) { set_error("%s: A_%d is a stencil field; the velocity blocks are constant stencils", who, d); return 1; }
    if (st->nent < 1 || st->nent > MAC_MAXE) { set_error("%s: A_%d: nent %d outside 1 .. %d", who, d, st->nent, MAC_MAXE); return 1; }
    unsigned seen = 0;
    bool centre = false;
    for (int k = 0; k < st->nent; ++k) {
      const int32_t *o = st->off[k];
      int nz = 0, axis = -1;
      for (int t = 0; t < 3; ++t)
        if (o[t]) {
          ++nz;
          axis = t;
        }
      if (nz > 1 || (nz == 1 && (axis >= nd || o[axis] < -1 || o[axis] > 1))) {
        set_error("%s: A_%d, entry %d (%d, %d, %d) is not the centre or an axis neighbour at distance 1 of a %d-D field", who, d, k, o[0], o[1], o[2], nd);
        return 1;
      }
      const int pos = nz == 0 ? 0 : 1 + 2 * axis + (o[axis] > 0);
      if (seen & (1u << pos)) { set_error("%s: A_%d, entry %d repeats the offset (%d, %d, %d)", who, d, k, o[0], o[1], o[2]); return 1; }
      seen |= 1u << pos;
      const int lin = (int)(o[0] + a.lu[d].s1 * o[1] + a.lu[d].s2 * o[2]);
      MacStar &A = a.A[d];
      A.off[A.nent] = lin;
      A.coef[A.nent++] = st->coef[k];
      if (nz == 0) {
        centre = true;
        a.a[d] = st->coef[k];
        continue;
      }
      const bool plus = axis == d && o[axis] > 0, minus = axis == d && o[axis] < 0;
      if (plus) a.q[d] = st->coef[k];
      else {
        MacStar &R = a.RL[d];
        R.off[R.nent] = lin;
        R.coef[R.nent++] = st->coef[k];
      }
      if (minus) a.m[d] = st->coef[k];
      else {
        MacStar &R = a.RU[d];
        R.off[R.nent] = lin;
        R.coef[R.nent++] = st->coef[k];
      }
    }
    if (!centre) { set_error("%s: A_%d has no centre entry", who, d); return 1; }
  }
  return 0;
}

// per axis the lower and upper reach of A_d
static void mac_reach(const examg_stencil_t *st, int (&lo)[3], int (&hi)[3]) {
  for (int t = 0; t < 3; ++t) lo[t] = hi[t] = 0;
  for (int k = 0; k < st->nent; ++k)
    for (int t = 0; t < 3; ++t) {
      if (st->off[k][t] < 0) lo[t] = 1;
      if (st->off[k][t] > 0) hi[t] = 1;
    }
}

static bool mac_inside(const examg_layout_t *l, const Box &b, const int (&lo)[3], const int (&hi)[3]) {
  const Box g{b.b0 - lo[0], b.b1 - lo[1], b.b2 - lo[2], b.e0 + hi[0], b.e1 + hi[1], b.e2 + hi[2]};
  return box_inside(l, g, 0);
}

static unsigned mac_grid(long long threads) {
  long long nb = (threads + 255) / 256;
  return (unsigned)(nb > 8192 ? 8192 : (nb < 1 ? 1 : nb));
}

static int mac_op(int mode, const examg_mac_t *sys, uint32_t row_mask, const int32_t *begin, const int32_t *end, hipStream_t s) {
  const char *who = "examg_mac_op";
  if (mode != EXAMG_SYS_APPLY && mode != EXAMG_SYS_RESIDUAL) { set_error("%s: bad mode %d", who, mode); return 1; }
  if (!sys || !begin || !end) { set_error("%s: null argument", who); return 1; }
  if (sys->nd != 2 && sys->nd != 3) { set_error("%s: nd = %d; staggered systems are 2-D or 3-D", who, sys->nd); return 1; }
  const int nd = sys->nd;
  if (row_mask == 0 || (row_mask >> (nd + 1)) != 0) { set_error("%s: row mask 0x%x for %d rows", who, row_mask, nd + 1); return 1; }
  MacArgs a;
  if (mac_prepare(who, sys, false, mode == EXAMG_SYS_RESIDUAL, row_mask, a)) return 1;
  MacBoxes bx;
  long long most = 0;
  unsigned live = 0;
  const int zero[3] = {0, 0, 0};
  for (int r = 0; r <= nd; ++r) {
    bx.box[r] = Box{0, 0, 0, 0, 0, 0};
    if (!((row_mask >> r) & 1u)) continue;
    const Box box = make_box(begin + 3 * r, end + 3 * r);
    if (box.count() == 0) continue;
    if (nd == 2 && (box.b2 != 0 || box.e2 != 1)) { set_error("%s: row %d: a 2-D box must have [0,1) in dim 2", who, r); return 1; }
    if (r < nd) {
      int lo[3], hi[3];
      mac_reach(sys->A[r], lo, hi);
      if (!mac_inside(&sys->lu[r], box, lo, hi)) { set_error("%s: row %d: box + the reach of A_%d leaves the allocation of %s", who, r, r, MAC_U[r]); return 1; }
      int plo[3] = {0, 0, 0};
      plo[r] = 1;
      if (!mac_inside(&sys->lp, box, plo, zero)) { set_error("%s: row %d: the gradient leaves the allocation of the pressure", who, r); return 1; }
    } else {
      for (int d = 0; d < nd; ++d) {
        int hi[3] = {0, 0, 0};
        hi[d] = 1;
        if (!mac_inside(&sys->lu[d], box, zero, hi)) { set_error("%s: row %d: the divergence leaves the allocation of %s", who, r, MAC_U[d]); return 1; }
      }
    }
    if (mode == EXAMG_SYS_RESIDUAL && !box_inside(r < nd ? &sys->lf[r] : &sys->lfp, box, 0)) { set_error("%s: row %d: box leaves the rhs allocation", who, r); return 1; }
    if (!box_inside(r < nd ? &sys->ld[r] : &sys->ldp, box, 0)) { set_error("%s: row %d: box leaves the dst allocation", who, r); return 1; }
    bx.box[r] = box;
    live |= 1u << r;
    most = most > box.count() ? most : box.count();
  }
  if (!live) return 0;
  const dim3 grid(mac_grid(most), nd + 1);
  if (nd == 2) hipLaunchKernelGGL((k_mac_op<2>), grid, dim3(256), 0, s, a, mode, live, bx);
  else hipLaunchKernelGGL((k_mac_op<3>), grid, dim3(256), 0, s, a, mode, live, bx);
  EXAMG_CHECK_LAUNCH("k_mac_op");
  return 0;
}

// The colourings under which the box smoother is independent of the loop order: two cells conflict when one writes what the other reads
// or writes, which for full stars is every offset o != 0 with |o_d| <= 2 on every axis and at most two axes -- among them all of 1-norm
// 1 and 2.  One expression per axis with a modulus of 3 or more separates them all; that form is also what the kernel enumerates.
static bool mac_colouring_ok(const char *who, const examg_colouring_t *col, int nd, bool with_rem) {
  if (const char *msg = check_colouring(col, nd, with_rem)) { set_error("%s: colouring: %s", who, msg); return false; }
  for (int reach = 1; reach <= 2; ++reach)      // the neighbours first: the conflict named is the nearest one
    for (int o0 = -reach; o0 <= reach; ++o0)
      for (int o1 = -reach; o1 <= reach; ++o1)
        for (int o2 = (nd == 3 ? -reach : 0); o2 <= (nd == 3 ? reach : 0); ++o2) {
          const int32_t o[3] = {o0, o1, o2};
          const int norm = abs(o0) + abs(o1) + abs(o2);
          if (norm < 1 || norm > 2) continue;
          if (!colouring_separates(col, o)) {
            set_error("%s: the colouring does not decouple the boxes: cells i and i + (%d, %d, %d) have the same colour, and the box of one reads or "
                      "writes a face or a pressure of the other's -- an in-place loop over one colour would depend on the loop order",
                      who, o0, o1, o2);
            return false;
          }
        }
  unsigned axes = 0;
  for (int k = 0; k < col->nexpr; ++k) {
    const int ax = col->axes[k];
    if ((ax & (ax - 1)) != 0 || (axes & ax) || col->mod[k] < 3) {
      set_error("%s: colouring: the box smoother takes one expression (s_d + i_d) %% m_d per axis, every m_d >= 3", who);
      return false;
    }
    axes |= ax;
  }
  if (col->nexpr != nd) { set_error("%s: colouring: the box smoother takes one expression (s_d + i_d) %% m_d per axis, every m_d >= 3", who); return false; }
  return true;
}

// the eliminations of examg_mac_relax on the host, for every pattern of held faces the block has: a zero determinant or Schur complement?
static bool mac_regular(const char *who, const MacArgs &a, int nd) {
  // per axis: 0 no face held, 1 the lower, 2 the upper, 3 both
  int states[3][4], ns[3];
  for (int d = 0; d < 3; ++d) {
    ns[d] = 0;
    if (d >= nd) { states[d][ns[d]++] = 0; continue; }
    if (a.n[d] == 1) states[d][ns[d]++] = 3;
    else {
      states[d][ns[d]++] = 1;
      states[d][ns[d]++] = 2;
      if (a.n[d] > 2) states[d][ns[d]++] = 0;
    }
  }
  for (int s0 = 0; s0 < ns[0]; ++s0)
    for (int s1 = 0; s1 < ns[1]; ++s1)
      for (int s2 = 0; s2 < ns[2]; ++s2) {
        const int st[3] = {states[0][s0], states[1][s1], states[2][s2]};
        double sz = 0.0;
        for (int d = 0; d < nd; ++d) {
          const bool h0 = st[d] & 1, h1 = st[d] & 2;
          const double a00 = h0 ? 1.0 : a.a[d], a01 = h0 ? 0.0 : a.q[d], c0 = h0 ? 0.0 : a.bc[d];
          const double a11 = h1 ? 1.0 : a.a[d], a10 = h1 ? 0.0 : a.m[d], c1 = h1 ? 0.0 : a.bm[d];
          const double det = a00 * a11 - a01 * a10;
          if (det == 0.0) { set_error("%s: the 2 x 2 block of the faces of axis %d has the determinant zero", who, d); return false; }
          const double z0 = (c0 * a11 - a01 * c1) / det, z1 = (a00 * c1 - a10 * c0) / det;
          const double tz = a.cc[d] * z0;
          sz = d == 0 ? tz : sz + tz;
          sz = sz + a.cp[d] * z1;
        }
        if (sz == 0.0) {
          set_error("%s: the Schur complement of a cell's pressure is zero (held faces per axis: %d, %d, %d; 3 = both: fewer than 2 cells on every axis?)", who, st[0], st[1],
                    st[2]);
          return false;
        }
      }
  return true;
}

// sweep: all colours in the reference's order (the first expression fastest), col->rem not looked at
static int mac_relax(const char *who, const examg_mac_t *sys, double relax, const examg_colouring_t *col, const int32_t *begin, const int32_t *end, bool sweep,
                     hipStream_t s) {
  if (!sys || !col || !begin || !end) { set_error("%s: null argument", who); return 1; }
  MacArgs a;
  if (sys->nd != 2 && sys->nd != 3) { set_error("%s: nd = %d; staggered systems are 2-D or 3-D", who, sys->nd); return 1; }
  const int nd = sys->nd;
  if (mac_prepare(who, sys, true, true, (1u << (nd + 1)) - 1u, a)) return 1;
  if (!mac_colouring_ok(who, col, nd, !sweep)) return 1;
  if (!mac_regular(who, a, nd)) return 1;
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 0;
  if (nd == 2 && (box.b2 != 0 || box.e2 != 1)) { set_error("%s: a 2-D box must have [0,1) in dim 2", who); return 1; }
  const int bb[3] = {box.b0, box.b1, box.b2}, ee[3] = {box.e0, box.e1, box.e2};
  for (int d = 0; d < nd; ++d)
    if (bb[d] < 0 || ee[d] > a.n[d]) { set_error("%s: the box [%d, %d) of dim %d leaves the cells [0, %d) of the block", who, bb[d], ee[d], d, a.n[d]); return 1; }
  // cells of the block, ghost layers all round: the shells are inside the unknowns' allocations.  The right-hand sides:
  for (int d = 0; d < nd; ++d) {
    int hi[3] = {0, 0, 0};
    const int zero[3] = {0, 0, 0};
    hi[d] = 1;
    if (!mac_inside(&sys->lf[d], box, zero, hi)) { set_error("%s: box leaves the allocation of rhs %d", who, d); return 1; }
  }
  if (!box_inside(&sys->lfp, box, 0)) { set_error("%s: box leaves the allocation of rhs %d", who, nd); return 1; }
  if (!starts_nonnegative(col, begin)) { set_error("%s: a colour expression can be negative in this box (shift + begin < 0)", who); return 1; }
  examg_colouring_t one = *col;
  long long ncol = 1;
  for (int k = 0; k < col->nexpr; ++k) ncol *= col->mod[k];
  for (long long c = 0; c < (sweep ? ncol : 1); ++c) {
    if (sweep) {
      long long r = c;
      for (int k = 0; k < col->nexpr; ++k) {
        one.rem[k] = (int32_t)(r % col->mod[k]);
        r /= col->mod[k];
      }
    }
    const MCColour mc = make_colour(&one, box);
    if (mc_threads(mc) == 0) continue;      // no cell of the colour in the box
    if (nd == 2) hipLaunchKernelGGL((k_mac_relax<2>), dim3(mac_grid(mc_threads(mc))), dim3(256), 0, s, a, relax, mc);
    else hipLaunchKernelGGL((k_mac_relax<3>), dim3(mac_grid(mc_threads(mc))), dim3(256), 0, s, a, relax, mc);
    EXAMG_CHECK_LAUNCH("k_mac_relax");
  }
  return 0;
}

// the checks the single-field entry points of a face field share; n: cells per axis of l
static bool face_field_ok(const char *who, const char *what, int axis, const examg_layout_t *l, int *n) {
  n[0] = n[1] = n[2] = 0;
  return face_layout_ok(who, what, axis, l) && mac_layout_ok(who, what, l, l->nd, axis, n);
}

}  // namespace examg

using namespace examg;

extern "C" int examg_mac_op(int mode, const examg_mac_t *sys, uint32_t row_mask, const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  return mac_op(mode, sys, row_mask, begin, end, (hipStream_t)stream);
}

extern "C" int examg_mac_relax(const examg_mac_t *sys, double relax, const examg_colouring_t *col, const int32_t *begin, const int32_t *end,
                               examg_stream_t stream) {
  return mac_relax("examg_mac_relax", sys, relax, col, begin, end, false, (hipStream_t)stream);
}

extern "C" int examg_mac_sweep(const examg_mac_t *sys, double relax, const examg_colouring_t *col, const int32_t *begin, const int32_t *end,
                               examg_stream_t stream) {
  return mac_relax("examg_mac_sweep", sys, relax, col, begin, end, true, (hipStream_t)stream);
}

extern "C" int examg_restrict_face(int axis, const examg_layout_t *lf_, const double *rf, const examg_layout_t *lc_, double *fc, double scale,
                                   const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  const char *who = "examg_restrict_face";
  if (!lf_ || !rf || !lc_ || !fc || !begin || !end) { set_error("%s: null argument", who); return 1; }
  if (lf_->nd != lc_->nd) { set_error("%s: layouts of one dimensionality", who); return 1; }
  int nf[3], nc[3];
  if (!face_field_ok(who, "fine", axis, lf_, nf) || !face_field_ok(who, "coarse", axis, lc_, nc)) return 1;
  if (rf == fc) { set_error("%s: the two arrays are one", who); return 1; }
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 0;
  const int nd = lf_->nd;
  if (nd == 2 && (box.b2 != 0 || box.e2 != 1)) { set_error("%s: 2-D box must have [0,1) in dim 2", who); return 1; }
  int fb[3] = {0, 0, 0}, fe[3] = {1, 1, 1};
  for (int d = 0; d < nd; ++d) {
    fb[d] = d == axis ? 2 * begin[d] - 1 : 2 * begin[d];
    fe[d] = d == axis ? 2 * (end[d] - 1) + 2 : 2 * end[d];
  }
  if (!box_inside(lc_, box, 0) || !box_inside(lf_, make_box(fb, fe), 0)) { set_error("%s: box leaves an allocation", who); return 1; }
  const double half = nd == 3 ? 0.25 : 0.5;      // the other axes' weights, exact
  const double w0 = scale * (0.25 * half), w1 = scale * (0.5 * half);
  hipStream_t s = (hipStream_t)stream;
  if (nd == 2) hipLaunchKernelGGL((k_restrict_face<2>), dim3(mac_grid(box.count())), dim3(256), 0, s, axis, make_layout(lf_), rf, make_layout(lc_), fc, w0, w1, w0, box);
  else hipLaunchKernelGGL((k_restrict_face<3>), dim3(mac_grid(box.count())), dim3(256), 0, s, axis, make_layout(lf_), rf, make_layout(lc_), fc, w0, w1, w0, box);
  EXAMG_CHECK_LAUNCH("k_restrict_face");
  return 0;
}

extern "C" int examg_prolong_add_face(int axis, const examg_layout_t *lc_, const double *uc, const examg_layout_t *lf_, double *uf, const int32_t *begin,
                                      const int32_t *end, examg_stream_t stream) {
  const char *who = "examg_prolong_add_face";
  if (!lf_ || !uf || !lc_ || !uc || !begin || !end) { set_error("%s: null argument", who); return 1; }
  if (lf_->nd != lc_->nd) { set_error("%s: layouts of one dimensionality", who); return 1; }
  int nf[3], nc[3];
  if (!face_field_ok(who, "fine", axis, lf_, nf) || !face_field_ok(who, "coarse", axis, lc_, nc)) return 1;
  if (uc == uf) { set_error("%s: the two arrays are one", who); return 1; }
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 0;
  const int nd = lf_->nd;
  if (nd == 2 && (box.b2 != 0 || box.e2 != 1)) { set_error("%s: 2-D box must have [0,1) in dim 2", who); return 1; }
  if (begin[axis] < 0) { set_error("%s: negative index on the field's own axis (the parity cases are those of a loop that starts at the boundary face 0)", who); return 1; }
  int cb[3] = {0, 0, 0}, ce[3] = {1, 1, 1};
  for (int d = 0; d < nd; ++d) {
    cb[d] = begin[d] >> 1;
    ce[d] = (d == axis ? (end[d] >> 1) : ((end[d] - 1) >> 1)) + 1;      // own axis: the upper parent of the last odd index
  }
  if (!box_inside(lf_, box, 0) || !box_inside(lc_, make_box(cb, ce), 0)) { set_error("%s: box leaves an allocation", who); return 1; }
  hipStream_t s = (hipStream_t)stream;
  if (nd == 2) hipLaunchKernelGGL((k_prolong_add_face<2>), dim3(mac_grid(box.count())), dim3(256), 0, s, axis, make_layout(lc_), uc, make_layout(lf_), uf, box);
  else hipLaunchKernelGGL((k_prolong_add_face<3>), dim3(mac_grid(box.count())), dim3(256), 0, s, axis, make_layout(lc_), uc, make_layout(lf_), uf, box);
  EXAMG_CHECK_LAUNCH("k_prolong_add_face");
  return 0;
}

extern "C" int examg_apply_bc_face(int axis, const examg_layout_t *l, double *x, const examg_geom_t *g, int kind, const examg_expr_t *expr, uint32_t face_mask,
                                   examg_stream_t stream) {
  const char *who = "examg_apply_bc_face";
  if (!l || !x || !g) { set_error("%s: null argument", who); return 1; }
  if (kind == EXAMG_BC_VALUE_MINUS) { set_error("%s: EXAMG_BC_VALUE_MINUS; face fields take EXAMG_BC_DIRICHLET or EXAMG_BC_NEUMANN", who); return 1; }
  if (kind != EXAMG_BC_DIRICHLET && kind != EXAMG_BC_NEUMANN) { set_error("%s: kind %d; face fields take EXAMG_BC_DIRICHLET or EXAMG_BC_NEUMANN", who, kind); return 1; }
  if (kind == EXAMG_BC_DIRICHLET && !expr_ok(expr)) return 1;
  int n[3];
  if (!face_field_ok(who, "field's", axis, l, n)) return 1;
  const int nd = l->nd;
  if (kind == EXAMG_BC_NEUMANN && (face_mask & (3u << (2 * axis)))) {
    set_error("%s: a Neumann wall normal to the field's own axis %d (the node rule for it is not built)", who, axis);
    return 1;
  }
  MacWalls wl;
  wl.n = 0;
  wl.start[0] = 0;
  for (int d = 0; d < nd; ++d)
    for (int side = 0; side < 2; ++side) {
      if (!(face_mask & (1u << (2 * d + side)))) continue;
      if (d != axis && (side ? l->ghost_r[d] : l->ghost_l[d]) < 1) { set_error("%s: wall %d of dim %d has no ghost layer", who, side, d); return 1; }
      int b[3] = {0, 0, 0}, e[3] = {1, 1, 1};
      for (int t = 0; t < nd; ++t) e[t] = t == axis ? n[t] + 1 : n[t];
      if (side == 0) e[d] = 1;
      else b[d] = e[d] - 1;
      wl.box[wl.n] = Box{b[0], b[1], b[2], e[0], e[1], e[2]};
      wl.dim[wl.n] = d;
      wl.up[wl.n] = side;
      wl.start[wl.n + 1] = wl.start[wl.n] + wl.box[wl.n].count();
      ++wl.n;
    }
  if (wl.n == 0) return 0;
  long long nb = (wl.start[wl.n] + 255) / 256;
  if (nb > 2048) nb = 2048;
  hipStream_t s = (hipStream_t)stream;
  if (kind == EXAMG_BC_NEUMANN) {
    hipLaunchKernelGGL(k_neumann_bc_face, dim3((unsigned)nb), dim3(256), 0, s, make_layout(l), x, wl);
  } else {
    const int3 ncell = make_int3(n[0], n[1], nd == 3 ? n[2] : 1);
    hipLaunchKernelGGL(k_dirichlet_bc_face, dim3((unsigned)nb), dim3(256), 0, s, axis, make_layout(l), x, make_geom(g), ExprEval{*expr}, wl, ncell,
                       (face_mask >> (2 * axis)) & 3u);
  }
  EXAMG_CHECK_LAUNCH("examg_apply_bc_face");
  return 0;
}
