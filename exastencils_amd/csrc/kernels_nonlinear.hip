// Semilinear operators N(q; u) = A * u + c(q) . u on gfx950: apply / residual / add (examg_nl_op) and the damped Newton-Jacobi and
// red-black smoother u + w * ((f - N(u; u)) / (diag(A) + d(u))) (examg_nl_smooth).  A is a constant stencil, c and d are postfix
// programs over the value of a field at the point.
//
// Reference: Testing/NonLinear/FAS_2D_Basic.exa4 (`Stencil gamSten { [0, 0] => gam * exp ( Solution<active>@current ) }`, the FAS
// V-cycle's smoother :78-86, residual :88-93, `RHS@coarser += ..` :127-129).  The arithmetic order is fixed in include/examg.h; this
// file is compiled with contraction off.
//
// Two kernels.  k_nl_star (below): star stencils of reach 1 on all points, row marching.  k_nl_gather, everything else (other
// stencils, the coloured loops): a lane owns one point (of the colour: the colour's points of a row are compacted, no idle lanes), x
// fastest across the lanes; the stencil's neighbours are gathered per entry through linear offsets (rows beside and the lane
// neighbours come from L1/L2: every u value leaves HBM once).  The programs are interpreted wave-uniformly: the instruction stream
// is a kernel argument, read through scalar loads (once, into scalar registers: the opcodes are packed), the dispatch is scalar
// branches, every lane executes the same instruction on its own operands.  The operand stack is eight named registers (the top of
// the stack and seven below it) selected by the uniform stack pointer through scalar branches -- never an indexed array, so nothing
// goes to scratch (private segment 0 in the code-object metadata of every instantiation; 156-169 VGPRs, no spills).
#include "examg_common.h"
#include "nl_program.h"      // NlProg, pack_program, nl_eval<R>: the interpreter the flux kernels share

namespace examg {

struct NlArgs {
  LayoutDev lu, lq, lf, ld;
  const double *u, *q, *rhs;
  double *dst;
  int nent, diag;
  long long uo[EXAMG_MAX_ENTRIES];   // linear offsets of the entries in the u layout
  double coef[EXAMG_MAX_ENTRIES];
  int code[8];                       // star path: what entry k multiplies (nl_pick)
  NlProg prog[2];                    // c, d (d: the smoother only)
  double w;
  int colour;
  Box box;
  int row_w;                         // points per row (of the colour)
};

enum { NL_SMOOTH = 3 };              // beside EXAMG_NL_APPLY / RESIDUAL / ADD

// NENT: the entry count of the stencil when the fold is unrolled (5, 7: coefficients and offsets arrive in two scalar loads and all
// neighbour loads are in flight together), 0: a loop over a.nent entries.  Same products, same order.
template <int MODE, int NENT>
__global__ void __launch_bounds__(256) k_nl_gather(NlArgs a) {
  const Box box = a.box;
  const long long total = (long long)box.n1() * box.n2() * a.row_w;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  int c0 = 0, i1 = box.b1, i2 = box.b2;
  if (total < (1LL << 31)) {         // 32-bit index arithmetic (uniform choice; same indices)
    const unsigned tt = (unsigned)t, row = tt / (unsigned)a.row_w, p = row / (unsigned)box.n1();
    c0 = (int)(tt - row * (unsigned)a.row_w);
    i1 = box.b1 + (int)(row - p * (unsigned)box.n1());
    i2 = box.b2 + (int)p;
  } else {
    const long long row = t / a.row_w;
    c0 = (int)(t - row * a.row_w);
    i1 = box.b1 + (int)(row % box.n1());
    i2 = box.b2 + (int)(row / box.n1());
  }
  int i0 = box.b0 + c0;
  if (a.colour >= 0) i0 = box.b0 + (((box.b0 + i1 + i2) & 1) != a.colour ? 1 : 0) + 2 * c0;
  const bool on = t < total && i0 < box.e0;
  if (!on) {                         // idle lanes compute on the box's first point and store nothing: the interpreter below stays uniform
    i0 = box.b0;
    i1 = box.b1;
    i2 = box.b2;
  }
  const long long iu = lidx_plain(a.lu, i0, i1, i2);
  const double *up = a.u + iu;
  double conv = a.coef[0] * up[a.uo[0]];
  if (NENT > 0) {
#pragma unroll
    for (int k = 1; k < NENT; ++k) conv = conv + a.coef[k] * up[a.uo[k]];
  } else {
    for (int k = 1; k < a.nent; ++k) conv = conv + a.coef[k] * up[a.uo[k]];
  }
  const double uc = up[0];
  const double qv = MODE == NL_SMOOTH ? uc : a.q[lidx_plain(a.lq, i0, i1, i2)];
  double cv = 0.0, dv = 0.0;
  for (int p = 0; p < (MODE == NL_SMOOTH ? 2 : 1); ++p) {      // one copy of the interpreter for both programs
    const double in[1] = {qv};
    double r[1];
    nl_eval<1>(a.prog[p], in, r);
    if (p == 0) cv = r[0];
    else dv = r[0];
  }
  const double n = conv + cv * uc;
  const long long id = lidx_plain(a.ld, i0, i1, i2);
  double out;
  if (MODE == EXAMG_NL_APPLY) out = n;
  else if (MODE == EXAMG_NL_RESIDUAL) out = a.rhs[lidx_plain(a.lf, i0, i1, i2)] - n;
  else if (MODE == EXAMG_NL_ADD) out = a.dst[id] + n;
  else out = uc + a.w * ((a.rhs[lidx_plain(a.lf, i0, i1, i2)] - n) / (a.coef[a.diag] + dv));
  if (on) a.dst[id] = out;
}

// ---- star stencils of reach 1 (2-D 5-point, 3-D 7-point), all points: row marching --------------------------------------------------
// A wave owns a run of 64 x points and R consecutive rows of one plane.  A lane loads its column of the rows y0 - 1 .. y0 + R once (R + 2
// loads for R points) and keeps it in registers: the y neighbours of a row are the rows beside it in that column; the x neighbours
// are the adjacent lanes' values (DPP wave shift), from memory only at the two ends of the run; the z neighbours are loaded.  The
// programs are interpreted once per instruction for all R rows of the lane.  The fold is the gather kernel's: the entries in declared
// order, entry k times the value its code names (0 centre, 1 + 2d lower, 2 + 2d upper neighbour in d) -- the same products in the
// same order, the same bits.  Lanes and rows past the end of the box work on the box's last column / row and store nothing.
__device__ __forceinline__ double nl_pick(int code, double c, double xm, double xp, double ym, double yp, double zm, double zp) {
  return code == 0 ? c : (code == 1 ? xm : (code == 2 ? xp : (code == 3 ? ym : (code == 4 ? yp : (code == 5 ? zm : zp)))));
}

template <int MODE, int ND, int R>
__global__ void __launch_bounds__(256) k_nl_star(NlArgs a, int ntx, int ngy) {
  constexpr int NENT = 2 * ND + 1;
  const Box box = a.box;
  const long long wv = (long long)blockIdx.x * 4 + (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long per_plane = (long long)ntx * ngy;
  if (wv >= per_plane * box.n2()) return;      // uniform
  const int lane = threadIdx.x & 63;
  const int pz = (int)(wv / per_plane);
  const int rem = (int)(wv - pz * per_plane);
  const int gy = rem / ntx, tx = rem - gy * ntx;
  const int x = box.b0 + tx * 64 + lane, z = box.b2 + pz, y0 = box.b1 + gy * R;
  const bool vx = x < box.e0;
  const int xc = vx ? x : box.e0 - 1;
  double col[R + 2];
#pragma unroll
  for (int j = 0; j < R + 2; ++j) {
    const int yy = min(y0 - 1 + j, box.e1);
    col[j] = a.u[lidx_plain(a.lu, xc, yy, z)];
  }
  double conv[R], uc[R], qv[R];
  long long io[R];      // own point in the u layout
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int yc = min(y0 + r, box.e1 - 1);
    io[r] = lidx_plain(a.lu, xc, yc, z);
    const double c = col[r + 1];
    // the lane exchange stands outside every divergent branch: all 64 lanes take part
    double xm = lane_below(c), xp = lane_above(c);
    const long long ir = lidx_plain(a.lu, xc, min(y0 + r, box.e1), z);
    if (lane == 0) xm = a.u[ir - 1];
    if (lane == 63 || x + 1 >= box.e0) xp = a.u[ir + 1];
    double zm = 0.0, zp = 0.0;
    if (ND == 3) {
      zm = a.u[ir - a.lu.s2];
      zp = a.u[ir + a.lu.s2];
    }
    double acc = a.coef[0] * nl_pick(a.code[0], c, xm, xp, col[r], col[r + 2], zm, zp);
#pragma unroll
    for (int k = 1; k < NENT; ++k) acc = acc + a.coef[k] * nl_pick(a.code[k], c, xm, xp, col[r], col[r + 2], zm, zp);
    conv[r] = acc;
    uc[r] = c;
    qv[r] = MODE == NL_SMOOTH ? c : a.q[lidx_plain(a.lq, xc, yc, z)];
  }
  double cv[R], dv[R];
#pragma unroll
  for (int r = 0; r < R; ++r) dv[r] = 0.0;
  nl_eval<R>(a.prog[0], qv, cv);
  if (MODE == NL_SMOOTH) nl_eval<R>(a.prog[1], qv, dv);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int yc = min(y0 + r, box.e1 - 1);
    const double n = conv[r] + cv[r] * uc[r];
    const long long id = lidx_plain(a.ld, xc, yc, z);
    double out;
    if (MODE == EXAMG_NL_APPLY) out = n;
    else if (MODE == EXAMG_NL_RESIDUAL) out = a.rhs[lidx_plain(a.lf, xc, yc, z)] - n;
    else if (MODE == EXAMG_NL_ADD) out = a.dst[id] + n;
    else out = uc[r] + a.w * ((a.rhs[lidx_plain(a.lf, xc, yc, z)] - n) / (a.coef[a.diag] + dv[r]));
    if (vx && y0 + r < box.e1) a.dst[id] = out;
  }
}

constexpr int NL_STAR_ROWS = 2;
static thread_local int g_nl_gather_only = 0;      // examg_debug_nl_gather_only (debug build): star stencils on the gather kernel too

// The codes of a star stencil of reach 1 with every axis entry exactly once (2 nd + 1 entries); false: not one
static bool nl_star_codes(const examg_stencil_t *st, int nd, int (&code)[7]) {
  if (st->nent != 2 * nd + 1) return false;
  unsigned seen = 0;
  for (int k = 0; k < st->nent; ++k) {
    int nz = 0, cd = 0;
    for (int d = 0; d < 3; ++d) {
      const int o = st->off[k][d];
      if (o == 0) continue;
      ++nz;
      if (d >= nd || o < -1 || o > 1) return false;
      cd = 1 + 2 * d + (o > 0 ? 1 : 0);
    }
    if (nz > 1 || (seen & (1u << cd))) return false;
    seen |= 1u << cd;
    code[k] = cd;
  }
  return true;
}

// include/examg.h: what a program of the semilinear entry points may hold
static bool nl_expr_ok(const char *who, const char *what, const examg_nlexpr_t *e) {
  if (!e) { set_error("%s: the program %s is a null pointer", who, what); return false; }
  if (e->n < 1) { set_error("%s: the program %s is empty", who, what); return false; }
  if (e->n > EXAMG_MAX_NL_EXPR) { set_error("%s: the program %s has %d instructions (limit %d)", who, what, e->n, EXAMG_MAX_NL_EXPR); return false; }
  int sp = 0;
  for (int i = 0; i < e->n; ++i) {
    switch (e->op[i]) {
      case EXAMG_OP_CONST: case EXAMG_OP_U: ++sp; break;
      case EXAMG_OP_X: case EXAMG_OP_Y: case EXAMG_OP_Z:
        set_error("%s: the program %s reads the node position (instruction %d); it is a function of the field value alone", who, what, i);
        return false;
      case EXAMG_OP_ADD: case EXAMG_OP_SUB: case EXAMG_OP_MUL: case EXAMG_OP_DIV: case EXAMG_OP_POW: case EXAMG_OP_MAX: case EXAMG_OP_MIN:
        if (sp < 2) { set_error("%s: the program %s underflows its stack at instruction %d", who, what, i); return false; }
        --sp;
        break;
      case EXAMG_OP_NEG: case EXAMG_OP_SIN: case EXAMG_OP_COS: case EXAMG_OP_EXP: case EXAMG_OP_SINH: case EXAMG_OP_COSH: case EXAMG_OP_SQRT:
      case EXAMG_OP_TAN: case EXAMG_OP_LOG: case EXAMG_OP_FABS: case EXAMG_OP_TANH:
        if (sp < 1) { set_error("%s: the program %s underflows its stack at instruction %d", who, what, i); return false; }
        break;
      default: set_error("%s: the program %s holds the unknown opcode %d", who, what, e->op[i]); return false;
    }
    if (sp > EXAMG_NL_STACK) { set_error("%s: the program %s needs a stack deeper than %d", who, what, EXAMG_NL_STACK); return false; }
  }
  if (sp != 1) { set_error("%s: the program %s must leave exactly one value (%d)", who, what, sp); return false; }
  return true;
}

static bool nl_layout_ok(const char *who, const char *what, const examg_layout_t *l, int nd) {
  if (l->nd != nd) { set_error("%s: the %s layout has %d dimensions, u has %d", who, what, l->nd, nd); return false; }
  if (lay_split(l)) { set_error("%s: the %s layout is colour-split; the semilinear kernels take plain layouts only", who, what); return false; }
  bool cell = true;
  for (int d = 0; d < nd; ++d) cell = cell && l->dup_l[d] == 0 && l->dup_r[d] == 0;
  if (cell) { set_error("%s: the %s layout is a cell layout (no duplicate layers); the semilinear kernels take node fields", who, what); return false; }
  return true;
}

// Checks and launch of both entry points.  mode: EXAMG_NL_* or NL_SMOOTH.
static int nl_run(const char *who, int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lq, const double *q,
                  const examg_layout_t *lf, const double *rhs, const examg_layout_t *ld, double *dst, const examg_stencil_t *st,
                  const examg_nlexpr_t *c, const examg_nlexpr_t *d, double w, int colour, const int32_t *begin, const int32_t *end, hipStream_t s) {
  const bool need_f = mode == EXAMG_NL_RESIDUAL || mode == NL_SMOOTH;
  if (!lu || !u || !lq || !q || !ld || !dst || !st || !begin || !end) { set_error("%s: null argument", who); return 1; }
  if (need_f && (!lf || !rhs)) { set_error("%s: a right-hand side is required", who); return 1; }
  const int nd = lu->nd;
  if (nd != 2 && nd != 3) { set_error("%s: 2-D or 3-D layouts (nd = %d)", who, nd); return 1; }
  if (!nl_layout_ok(who, "u", lu, nd) || !nl_layout_ok(who, "q", lq, nd) || !nl_layout_ok(who, "dst", ld, nd)) return 1;
  if (need_f && !nl_layout_ok(who, "rhs", lf, nd)) return 1;
  if (st->cfield) { set_error("%s: a stencil field cannot be the constant stencil of a semilinear operator", who); return 1; }
  if (st->nent < 1 || st->nent > EXAMG_MAX_ENTRIES) { set_error("%s: nent %d out of range", who, st->nent); return 1; }
  if (st->diag < 0 || st->diag >= st->nent || st->off[st->diag][0] != 0 || st->off[st->diag][1] != 0 || st->off[st->diag][2] != 0) {
    set_error("%s: the stencil has no centre entry (diag = %d)", who, st->diag);
    return 1;
  }
  for (int k = 0; k < st->nent; ++k)
    for (int dd = nd; dd < 3; ++dd)
      if (st->off[k][dd] != 0) { set_error("%s: stencil entry %d leaves the %d dimensions of the layouts", who, k, nd); return 1; }
  if (!nl_expr_ok(who, "c", c)) return 1;
  if (mode == NL_SMOOTH && !nl_expr_ok(who, "d", d)) return 1;
  if (mode == NL_SMOOTH) {
    if (colour < -1 || colour > 1) { set_error("%s: colour must be -1, 0 or 1", who); return 1; }
    if (colour < 0 && dst == u) { set_error("%s: colour -1 (Jacobi) runs out of place; u_out is u_in", who); return 1; }
    if (colour >= 0 && dst != u) { set_error("%s: a colour runs in place; u_out is not u_in", who); return 1; }
    if (colour >= 0 && memcmp(lu, ld, sizeof(*lu)) != 0) { set_error("%s: a colour runs in place; the layout of u_out is not that of u_in", who); return 1; }
    if (colour >= 0)
      for (int k = 0; k < st->nent; ++k)
        if (k != st->diag && ((st->off[k][0] + st->off[k][1] + st->off[k][2]) & 1) == 0) {
          set_error("%s: the parity colouring does not decouple the stencil (entry %d joins two points of one colour)", who, k);
          return 1;
        }
  } else if (dst == u) {
    set_error("%s: dst is u; the operator does not run in place", who);
    return 1;
  }
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 0;
  if (nd == 2 && (box.b2 != 0 || box.e2 != 1)) { set_error("%s: 2-D box must have [0,1) in dim 2", who); return 1; }
  if (!box_inside(lu, box, stencil_reach(st))) { set_error("%s: box + stencil reach leaves the u allocation", who); return 1; }
  if (!box_inside(lq, box, 0)) { set_error("%s: box leaves the q allocation", who); return 1; }
  if (!box_inside(ld, box, 0)) { set_error("%s: box leaves the dst allocation", who); return 1; }
  if (need_f && !box_inside(lf, box, 0)) { set_error("%s: box leaves the rhs allocation", who); return 1; }

  NlArgs a;
  memset(&a, 0, sizeof(a));
  a.lu = make_layout(lu);
  a.lq = make_layout(lq);
  a.ld = make_layout(ld);
  a.lf = need_f ? make_layout(lf) : a.ld;
  a.u = u;
  a.q = q;
  a.rhs = rhs;
  a.dst = dst;
  a.nent = st->nent;
  a.diag = st->diag;
  fill_u_offsets(a.uo, st, a.lu);
  for (int k = 0; k < st->nent; ++k) a.coef[k] = st->coef[k];
  a.prog[0] = pack_program(c);
  if (mode == NL_SMOOTH) a.prog[1] = pack_program(d);
  a.w = w;
  a.colour = mode == NL_SMOOTH ? colour : -1;
  a.box = box;
  a.row_w = a.colour >= 0 ? (box.n0() + 1) / 2 : box.n0();
  int code[7] = {0, 0, 0, 0, 0, 0, 0};
  if (a.colour < 0 && !g_nl_gather_only && nl_star_codes(st, nd, code)) {
    for (int k = 0; k < 7; ++k) a.code[k] = code[k];
    const int ntx = (box.n0() + 63) / 64, ngy = (box.n1() + NL_STAR_ROWS - 1) / NL_STAR_ROWS;
    const long long waves = (long long)ntx * ngy * box.n2();
    if ((waves + 3) / 4 > 0x7fffffffLL) { set_error("%s: grid too large", who); return 1; }
    const dim3 sgrid((unsigned)((waves + 3) / 4)), sblk(256);
#define NL_STAR(M)                                                                                               \
  do {                                                                                                           \
    if (nd == 2) hipLaunchKernelGGL((k_nl_star<M, 2, NL_STAR_ROWS>), sgrid, sblk, 0, s, a, ntx, ngy);            \
    else hipLaunchKernelGGL((k_nl_star<M, 3, NL_STAR_ROWS>), sgrid, sblk, 0, s, a, ntx, ngy);                    \
  } while (0)
    switch (mode) {
      case EXAMG_NL_APPLY: NL_STAR(EXAMG_NL_APPLY); break;
      case EXAMG_NL_RESIDUAL: NL_STAR(EXAMG_NL_RESIDUAL); break;
      case EXAMG_NL_ADD: NL_STAR(EXAMG_NL_ADD); break;
      default: NL_STAR(NL_SMOOTH); break;
    }
#undef NL_STAR
    EXAMG_CHECK_LAUNCH("k_nl_star");
    return 0;
  }
  const long long total = (long long)box.n1() * box.n2() * a.row_w;
  const long long nb = (total + 255) / 256;
  if (nb > 0x7fffffffLL) { set_error("%s: grid too large", who); return 1; }
  const dim3 grid((unsigned)nb), blk(256);
#define NL_LAUNCH(M)                                                                                \
  do {                                                                                              \
    if (st->nent == 5) hipLaunchKernelGGL((k_nl_gather<M, 5>), grid, blk, 0, s, a);                 \
    else if (st->nent == 7) hipLaunchKernelGGL((k_nl_gather<M, 7>), grid, blk, 0, s, a);            \
    else hipLaunchKernelGGL((k_nl_gather<M, 0>), grid, blk, 0, s, a);                               \
  } while (0)
  switch (mode) {
    case EXAMG_NL_APPLY: NL_LAUNCH(EXAMG_NL_APPLY); break;
    case EXAMG_NL_RESIDUAL: NL_LAUNCH(EXAMG_NL_RESIDUAL); break;
    case EXAMG_NL_ADD: NL_LAUNCH(EXAMG_NL_ADD); break;
    default: NL_LAUNCH(NL_SMOOTH); break;
  }
#undef NL_LAUNCH
  EXAMG_CHECK_LAUNCH("k_nl_gather");
  return 0;
}

}  // namespace examg

using namespace examg;

#ifdef EXAMG_DEBUG_HOOKS
extern "C" int examg_debug_nl_gather_only(int on) {
  g_nl_gather_only = on;
  return 0;
}
#endif

extern "C" int examg_nl_op(int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lq, const double *q, const examg_layout_t *lf,
                           const double *rhs, const examg_layout_t *ld, double *dst, const examg_stencil_t *st, const examg_nlexpr_t *c,
                           const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  if (mode != EXAMG_NL_APPLY && mode != EXAMG_NL_RESIDUAL && mode != EXAMG_NL_ADD) { set_error("examg_nl_op: bad mode %d", mode); return 1; }
  return nl_run("examg_nl_op", mode, lu, u, lq, q, lf, rhs, ld, dst, st, c, nullptr, 0.0, -1, begin, end, (hipStream_t)stream);
}

extern "C" int examg_nl_smooth(const examg_layout_t *lu, const double *u_in, const examg_layout_t *ld, double *u_out, const examg_layout_t *lf,
                               const double *rhs, const examg_stencil_t *st, const examg_nlexpr_t *c, const examg_nlexpr_t *d, double w, int colour,
                               const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  return nl_run("examg_nl_smooth", NL_SMOOTH, lu, u_in, lu, u_in, lf, rhs, ld, u_out, st, c, d, w, colour, begin, end, (hipStream_t)stream);
}
