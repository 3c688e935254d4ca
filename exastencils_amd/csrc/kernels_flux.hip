// Explicit flux-form time steps on cell fields on gfx950 (examg_flux_step), reductions of point programs over cell fields
// (examg_reduce_expr_cell).
//
// Reference: Examples/SWE/2D_FV_SWE.exa4 and Testing/MatrixClassTests/2D_FV_SWE/ (the Lax-Friedrichs step of the shallow-water
// equations: `Expr` declarations read at @east / @west / @north / @south, baseExt/l4/L4_ExpressionDeclaration.scala,
// util/l4/L4_OffsetAlias.scala; the CFL step from a `max` reduction over a point expression).  The arithmetic order is fixed in
// include/examg.h; this file is compiled with contraction off.
//
// Two kernels, the same bits.  k_flux_gather: a lane owns one cell, x fastest; every term evaluates its program at both of its
// cells (one copy of the interpreter, a loop over components, terms and sides).  k_flux_march: a wave owns a window of 64 columns
// of a chunk of rows and marches in y, R = 2 rows per step; every program is evaluated ONCE per cell, for both new rows of a lane in
// one dispatch of each instruction.  The field values and program values of the rows y - 1 .. y + 2 of the lane's column live in
// registers (a ring of two rows and the two new ones); y neighbours are other registers of the lane, x neighbours the adjacent lanes'
// values (DPP wave shifts).  Lanes 0 and 63 are the halo columns of the window: they load and evaluate, and store nothing -- the
// neighbouring window recomputes them.  A chunk starts with one step that only fills the ring (rows ys - 1, ys).  Every register
// array is indexed by constants after unrolling; what a term or a component names at run time (its program, its field, its
// neighbours) is selected through uniform branches.  Nothing goes to scratch: private segment 0 in the code-object metadata of both
// kernels.
#include "examg_common.h"
#include "nl_program.h"

namespace examg {

// what a stencil entry or a term's cell is, relative to the lane's cell: 0 centre, 1 x - 1, 2 x + 1, 3 y - 1, 4 y + 1
struct FluxTermDev {
  int prog, pc, mc;
  double scale;
};
struct FluxCompDev {
  int field, nent, nterms;
  int code[EXAMG_FLUX_MAX_ENTRIES];
  double coef[EXAMG_FLUX_MAX_ENTRIES];
  FluxTermDev term[EXAMG_FLUX_MAX_TERMS];
};
struct FluxArgs {
  LayoutDev lin, lout;
  const double *in[EXAMG_FLUX_MAX_FIELDS];
  double *out[EXAMG_FLUX_MAX_COMP];
  int nfields, nprogs, ncomp;
  Box box;
  FluxCompDev comp[EXAMG_FLUX_MAX_COMP];
  NlProg prog[EXAMG_FLUX_MAX_PROGS];
};
static_assert(sizeof(FluxArgs) + 16 <= 4096, "the arguments of the flux kernels travel by value: 4 KiB of kernel arguments");

__device__ __forceinline__ long long flux_off(int code, long long s1) {
  return code == 0 ? 0 : (code == 1 ? -1 : (code == 2 ? 1 : (code == 3 ? -s1 : s1)));
}
__device__ __forceinline__ double flux_pick(int code, double c, double xm, double xp, double ym, double yp) {
  switch (code) {      // uniform: scalar branches, no select chain
    case 0: return c;
    case 1: return xm;
    case 2: return xp;
    case 3: return ym;
    default: return yp;
  }
}

// ---- one lane per cell ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_flux_gather(FluxArgs a) {
  const Box box = a.box;
  const long long total = (long long)box.n0() * box.n1();
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool on = t < total;      // idle lanes compute on the box's first cell and store nothing: the interpreter stays uniform
  const long long tt = on ? t : 0;
  const int row = (int)(tt / box.n0());
  const int i0 = box.b0 + (int)(tt - (long long)row * box.n0()), i1 = box.b1 + row;
  const long long ii = lidx_plain(a.lin, i0, i1, 0), io = lidx_plain(a.lout, i0, i1, 0);
  const long long s1 = a.lin.s1;
  for (int c = 0; c < a.ncomp; ++c) {
    const FluxCompDev &cc = a.comp[c];
    const double *q = a.in[cc.field] + ii;
    double acc = cc.coef[0] * q[flux_off(cc.code[0], s1)];
    for (int k = 1; k < cc.nent; ++k) acc = acc + cc.coef[k] * q[flux_off(cc.code[k], s1)];
    for (int m = 0; m < cc.nterms; ++m) {
      const FluxTermDev &tm = cc.term[m];
      double pp = 0.0, pm = 0.0;
#pragma unroll 1
      for (int side = 0; side < 2; ++side) {      // one copy of the interpreter for both cells
        const long long at = ii + flux_off(side ? tm.mc : tm.pc, s1);
        double f[EXAMG_FLUX_MAX_FIELDS][1], r[1];
#pragma unroll
        for (int k = 0; k < EXAMG_FLUX_MAX_FIELDS; ++k) f[k][0] = k < a.nfields ? a.in[k][at] : 0.0;
        nl_eval_fields<1, EXAMG_FLUX_MAX_FIELDS>(a.prog[tm.prog], f, r);
        if (side) pm = r[0];
        else pp = r[0];
      }
      acc = acc + tm.scale * (pp - pm);
    }
    if (on) a.out[c][io] = acc;
  }
}

// ---- row marching: every program once per cell ----------------------------------------------------------------------------------------
constexpr int FLUX_R = 2;          // rows per step; the ring holds the two rows before them
constexpr int FLUX_WIN = 62;       // columns a window writes (64 lanes less the two halo columns)

// rows j = 0 .. 3 (y0 - 1 .. y0 + 2) of the array k names, out of the ring and the new rows -- k is uniform: scalar branches
#define FLUX_ROWS(dst, k, ring, fresh, N)                                                                                  \
  _Pragma("unroll") for (int kk = 0; kk < N; ++kk) if (kk == (k)) {                                                        \
    dst[0] = ring[kk][0]; dst[1] = ring[kk][1]; dst[2] = fresh[kk][0]; dst[3] = fresh[kk][1];                               \
  }

__global__ void __launch_bounds__(256) k_flux_march(FluxArgs a, int ntx, int nch, int chunk) {
  constexpr int NF = EXAMG_FLUX_MAX_FIELDS, NP = EXAMG_FLUX_MAX_PROGS;
  const Box box = a.box;
  const long long wv = (long long)blockIdx.x * 4 + (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wv >= (long long)ntx * nch) return;      // uniform
  const int lane = threadIdx.x & 63;
  const int ch = (int)(wv / ntx), tx = (int)(wv - (long long)ch * ntx);
  const int x = box.b0 - 1 + tx * FLUX_WIN + lane;
  const int xc = min(x, box.e0);               // columns b0 - 1 .. e0: the box and its shell
  const bool vx = lane >= 1 && lane <= FLUX_WIN && x < box.e0;
  const int ys = box.b1 + ch * chunk, ye = min(ys + chunk, box.e1);
  const double *col[NF];                       // the lane's column of every field (per-lane pointers: the bases need no scalar registers in the loop)
#pragma unroll
  for (int k = 0; k < NF; ++k) col[k] = a.in[k < a.nfields ? k : 0] + (a.lin.origin + xc);
  const long long s1 = a.lin.s1;
  double fr[NF][2], pr[NP][2];                 // the ring: rows y0 - 1, y0
#pragma unroll
  for (int k = 0; k < NF; ++k) fr[k][0] = fr[k][1] = 0.0;
#pragma unroll
  for (int p = 0; p < NP; ++p) pr[p][0] = pr[p][1] = 0.0;
  for (int y0 = ys - 2; y0 < ye; y0 += FLUX_R) {
    // the new rows y0 + 1, y0 + 2 (rows past the shell repeat its last row; they reach no stored value)
    double fn[NF][FLUX_R], pn[NP][FLUX_R];
#pragma unroll
    for (int k = 0; k < NF; ++k)
#pragma unroll
      for (int j = 0; j < FLUX_R; ++j) fn[k][j] = k < a.nfields ? col[k][s1 * min(y0 + 1 + j, box.e1)] : 0.0;
#pragma unroll
    for (int p = 0; p < NP; ++p) pn[p][0] = pn[p][1] = 0.0;
#pragma unroll 1
    for (int p = 0; p < a.nprogs; ++p) {       // one copy of the interpreter; the result into the registers p names
      double r[FLUX_R];
      nl_eval_fields<FLUX_R, NF>(a.prog[p], fn, r);
      switch (p) {
        case 0: pn[0][0] = r[0]; pn[0][1] = r[1]; break;
        case 1: pn[1][0] = r[0]; pn[1][1] = r[1]; break;
        case 2: pn[2][0] = r[0]; pn[2][1] = r[1]; break;
        case 3: pn[3][0] = r[0]; pn[3][1] = r[1]; break;
        case 4: pn[4][0] = r[0]; pn[4][1] = r[1]; break;
        case 5: pn[5][0] = r[0]; pn[5][1] = r[1]; break;
        case 6: pn[6][0] = r[0]; pn[6][1] = r[1]; break;
        default: pn[7][0] = r[0]; pn[7][1] = r[1]; break;
      }
    }
    if (y0 >= ys) {                            // uniform: the first step of a chunk only fills the ring
#pragma unroll 1
      for (int c = 0; c < a.ncomp; ++c) {      // components and terms are run-time loops: only the register arrays need constant indices
        const FluxCompDev &cc = a.comp[c];
        double acc[FLUX_R];
        {
          double q[4] = {0.0, 0.0, 0.0, 0.0};
          FLUX_ROWS(q, cc.field, fr, fn, NF)
#pragma unroll
          for (int r = 0; r < FLUX_R; ++r) {
            // the lane exchange stands outside every divergent branch: all 64 lanes take part
            const double ctr = q[r + 1], xm = lane_below(ctr), xp = lane_above(ctr);
            acc[r] = cc.coef[0] * flux_pick(cc.code[0], ctr, xm, xp, q[r], q[r + 2]);
#pragma unroll
            for (int k = 1; k < EXAMG_FLUX_MAX_ENTRIES; ++k)
              if (k < cc.nent) acc[r] = acc[r] + cc.coef[k] * flux_pick(cc.code[k], ctr, xm, xp, q[r], q[r + 2]);
          }
        }
#pragma unroll 1
        for (int m = 0; m < cc.nterms; ++m) {
          const FluxTermDev &tm = cc.term[m];
          double v[4] = {0.0, 0.0, 0.0, 0.0};
          FLUX_ROWS(v, tm.prog, pr, pn, NP)
#pragma unroll
          for (int r = 0; r < FLUX_R; ++r) {
            const double ctr = v[r + 1], xm = lane_below(ctr), xp = lane_above(ctr);
            const double plus = flux_pick(tm.pc, ctr, xm, xp, v[r], v[r + 2]), minus = flux_pick(tm.mc, ctr, xm, xp, v[r], v[r + 2]);
            acc[r] = acc[r] + tm.scale * (plus - minus);
          }
        }
#pragma unroll
        for (int r = 0; r < FLUX_R; ++r)
          if (vx && y0 + r < ye) a.out[c][lidx_plain(a.lout, x, y0 + r, 0)] = acc[r];
      }
    }
#pragma unroll
    for (int k = 0; k < NF; ++k) { fr[k][0] = fn[k][0]; fr[k][1] = fn[k][1]; }
#pragma unroll
    for (int p = 0; p < NP; ++p) { pr[p][0] = pn[p][0]; pr[p][1] = pn[p][1]; }
  }
}

// ---- reductions of a point program over cell fields -------------------------------------------------------------------------------------
constexpr int FLUX_RED_BLOCK = 256, FLUX_RED_MAX_BLOCKS = 2048;

struct RedExprArgs {
  LayoutDev l;
  const double *x[EXAMG_FLUX_MAX_FIELDS];
  int nfields;
  Box box;
  NlProg prog;
};

template <bool IS_MAX>
__device__ __forceinline__ double flux_block_reduce(double v) {
  __shared__ double sm[FLUX_RED_BLOCK / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double w = __shfl_down(v, o);
    v = IS_MAX ? fmax(v, w) : fmin(v, w);
  }
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = sm[0];
  for (int i = 1; i < FLUX_RED_BLOCK / 64; ++i) r = IS_MAX ? fmax(r, sm[i]) : fmin(r, sm[i]);
  __syncthreads();
  return r;
}

// every lane of a block makes the same number of trips: lanes past the end evaluate the box's first cell and drop the value
template <bool IS_MAX>
__global__ void __launch_bounds__(FLUX_RED_BLOCK) k_reduce_expr_partial(RedExprArgs a, double *part) {
  const Box box = a.box;
  const long long total = box.count(), stride = (long long)gridDim.x * blockDim.x;
  double m = IS_MAX ? -__builtin_inf() : __builtin_inf();
  for (long long base = (long long)blockIdx.x * blockDim.x; base < total; base += stride) {
    const long long t = base + threadIdx.x;
    const bool on = t < total;
    const long long tt = on ? t : 0;
    const long long row = tt / box.n0();
    const int i0 = box.b0 + (int)(tt - row * box.n0()), i1 = box.b1 + (int)(row % box.n1()), i2 = box.b2 + (int)(row / box.n1());
    const long long at = lidx_plain(a.l, i0, i1, i2);
    double f[EXAMG_FLUX_MAX_FIELDS][1], r[1];
#pragma unroll
    for (int k = 0; k < EXAMG_FLUX_MAX_FIELDS; ++k) f[k][0] = k < a.nfields ? a.x[k][at] : 0.0;
    nl_eval_fields<1, EXAMG_FLUX_MAX_FIELDS>(a.prog, f, r);
    if (on) m = IS_MAX ? fmax(m, r[0]) : fmin(m, r[0]);
  }
  const double r = flux_block_reduce<IS_MAX>(m);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

template <bool IS_MAX>
__global__ void __launch_bounds__(FLUX_RED_BLOCK) k_reduce_expr_final(const double *part, int n, double *result) {
  double m = IS_MAX ? -__builtin_inf() : __builtin_inf();
  for (int i = threadIdx.x; i < n; i += blockDim.x) m = IS_MAX ? fmax(m, part[i]) : fmin(m, part[i]);
  const double r = flux_block_reduce<IS_MAX>(m);
  if (threadIdx.x == 0) *result = r;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
static thread_local int g_flux_route = 0;      // examg_debug_flux_route (debug build): 0 the default, else EXAMG_FLUX_GATHER / EXAMG_FLUX_MARCH

// The default route (the measured table decides it).
constexpr int FLUX_DEFAULT_ROUTE = EXAMG_FLUX_MARCH;

// include/examg.h: what a program over cell fields may hold
static bool flux_expr_ok(const char *who, int p, const examg_nlexpr_t *e, int nfields) {
  if (e->n < 1) { set_error("%s: program %d is empty", who, p); return false; }
  if (e->n > EXAMG_MAX_NL_EXPR) { set_error("%s: program %d has %d instructions (limit %d)", who, p, e->n, EXAMG_MAX_NL_EXPR); return false; }
  int sp = 0;
  for (int i = 0; i < e->n; ++i) {
    const int op = e->op[i];
    if (op >= EXAMG_OP_FIELD0 && op < EXAMG_OP_FIELD0 + EXAMG_FLUX_MAX_FIELDS) {
      if (op - EXAMG_OP_FIELD0 >= nfields) {
        set_error("%s: program %d reads field %d at instruction %d; there are %d fields", who, p, op - EXAMG_OP_FIELD0, i, nfields);
        return false;
      }
      ++sp;
    } else {
      switch (op) {
        case EXAMG_OP_CONST: ++sp; break;
        case EXAMG_OP_U:
          set_error("%s: program %d holds EXAMG_OP_U (instruction %d); fields are read through EXAMG_OP_FIELD0 + k here", who, p, i);
          return false;
        case EXAMG_OP_X: case EXAMG_OP_Y: case EXAMG_OP_Z:
          set_error("%s: program %d reads the position (instruction %d); it is a function of the field values alone", who, p, i);
          return false;
        case EXAMG_OP_WX: case EXAMG_OP_WY: case EXAMG_OP_WZ:
          set_error("%s: program %d reads a cell width (instruction %d); it is a function of the field values alone", who, p, i);
          return false;
        case EXAMG_OP_ADD: case EXAMG_OP_SUB: case EXAMG_OP_MUL: case EXAMG_OP_DIV: case EXAMG_OP_POW: case EXAMG_OP_MAX: case EXAMG_OP_MIN:
          if (sp < 2) { set_error("%s: program %d underflows its stack at instruction %d", who, p, i); return false; }
          --sp;
          break;
        case EXAMG_OP_NEG: case EXAMG_OP_SIN: case EXAMG_OP_COS: case EXAMG_OP_EXP: case EXAMG_OP_SINH: case EXAMG_OP_COSH: case EXAMG_OP_SQRT:
        case EXAMG_OP_TAN: case EXAMG_OP_LOG: case EXAMG_OP_FABS: case EXAMG_OP_TANH:
          if (sp < 1) { set_error("%s: program %d underflows its stack at instruction %d", who, p, i); return false; }
          break;
        default: set_error("%s: program %d holds the unknown opcode %d", who, p, op); return false;
      }
    }
    if (sp > EXAMG_NL_STACK) { set_error("%s: program %d needs a stack deeper than %d", who, p, EXAMG_NL_STACK); return false; }
  }
  if (sp != 1) { set_error("%s: program %d must leave exactly one value (%d)", who, p, sp); return false; }
  return true;
}

static bool flux_layout_ok(const char *who, const char *what, const examg_layout_t *l) {
  for (int d = 0; d < 3; ++d)
    if (l->dup_l[d] != 0 || l->dup_r[d] != 0) {
      set_error("%s: the %s layout has duplicate layers (a node layout); these kernels take cell fields", who, what);
      return false;
    }
  if (lay_split(l)) { set_error("%s: the %s layout is colour-split; these kernels take plain layouts only", who, what); return false; }
  return true;
}

// 0 centre, 1 .. 4 the unit axis offsets in x and y; -1: none of them
static int flux_code(const int32_t *o) {
  if (o[2] != 0) return -1;
  if (o[0] == 0 && o[1] == 0) return 0;
  if (o[1] == 0 && (o[0] == -1 || o[0] == 1)) return o[0] < 0 ? 1 : 2;
  if (o[0] == 0 && (o[1] == -1 || o[1] == 1)) return o[1] < 0 ? 3 : 4;
  return -1;
}

static bool flux_overlap(const double *a, long long na, const double *b, long long nb) {
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * 8, b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * 8;
  return a0 < b1 && b0 < a1;
}

// The checks of examg_flux_step; the kernels' arguments.  -1: refused (error text set), 0: empty box, else the route.
static int flux_prepare(const char *who, const examg_flux_t *fx, const int32_t *begin, const int32_t *end, FluxArgs &a) {
  if (!fx || !begin || !end) { set_error("%s: null argument", who); return -1; }
  if (fx->lin.nd != 2 || fx->lout.nd != 2) {
    set_error("%s: layouts of %d and %d dimensions; the 3-D kernels are not built", who, fx->lin.nd, fx->lout.nd);
    return -1;
  }
  if (!flux_layout_ok(who, "input", &fx->lin) || !flux_layout_ok(who, "output", &fx->lout)) return -1;
  if (fx->nfields < 1 || fx->nfields > EXAMG_FLUX_MAX_FIELDS) { set_error("%s: %d input fields (1 .. %d)", who, fx->nfields, EXAMG_FLUX_MAX_FIELDS); return -1; }
  if (fx->nprogs < 0 || fx->nprogs > EXAMG_FLUX_MAX_PROGS) { set_error("%s: %d programs (0 .. %d)", who, fx->nprogs, EXAMG_FLUX_MAX_PROGS); return -1; }
  if (fx->ncomp < 1 || fx->ncomp > EXAMG_FLUX_MAX_COMP) { set_error("%s: %d components (1 .. %d)", who, fx->ncomp, EXAMG_FLUX_MAX_COMP); return -1; }
  memset(&a, 0, sizeof(a));
  a.lin = make_layout(&fx->lin);
  a.lout = make_layout(&fx->lout);
  a.nfields = fx->nfields;
  a.nprogs = fx->nprogs;
  a.ncomp = fx->ncomp;
  for (int k = 0; k < fx->nfields; ++k) {
    if (!fx->in[k]) { set_error("%s: input field %d is a null pointer", who, k); return -1; }
    a.in[k] = fx->in[k];
  }
  for (int c = 0; c < fx->ncomp; ++c) {
    const examg_flux_comp_t &cc = fx->comp[c];
    FluxCompDev &cd = a.comp[c];
    if (!fx->out[c]) { set_error("%s: the destination of component %d is a null pointer", who, c); return -1; }
    a.out[c] = fx->out[c];
    for (int k = 0; k < fx->nfields; ++k)
      if (flux_overlap(fx->out[c], a.lout.size, fx->in[k], a.lin.size)) {
        set_error("%s: the destination of component %d overlaps input field %d; the step does not run in place", who, c, k);
        return -1;
      }
    for (int c2 = 0; c2 < c; ++c2)
      if (flux_overlap(fx->out[c], a.lout.size, fx->out[c2], a.lout.size)) {
        set_error("%s: components %d and %d write one array", who, c2, c);
        return -1;
      }
    if (cc.field < 0 || cc.field >= fx->nfields) { set_error("%s: component %d names field %d; there are %d fields", who, c, cc.field, fx->nfields); return -1; }
    if (cc.nent == 0) { set_error("%s: the stencil of component %d is empty", who, c); return -1; }
    if (cc.nent < 0 || cc.nent > EXAMG_FLUX_MAX_ENTRIES) { set_error("%s: the stencil of component %d has %d entries (1 .. %d)", who, c, cc.nent, EXAMG_FLUX_MAX_ENTRIES); return -1; }
    if (cc.nterms < 0 || cc.nterms > EXAMG_FLUX_MAX_TERMS) { set_error("%s: component %d has %d terms (0 .. %d)", who, c, cc.nterms, EXAMG_FLUX_MAX_TERMS); return -1; }
    cd.field = cc.field;
    cd.nent = cc.nent;
    cd.nterms = cc.nterms;
    for (int k = 0; k < cc.nent; ++k) {
      cd.code[k] = flux_code(cc.off[k]);
      cd.coef[k] = cc.coef[k];
      if (cd.code[k] < 0) {
        set_error("%s: stencil entry %d of component %d, [%d, %d, %d], is not the centre or a unit axis offset in x or y", who, k, c, cc.off[k][0],
                  cc.off[k][1], cc.off[k][2]);
        return -1;
      }
    }
    for (int m = 0; m < cc.nterms; ++m) {
      const examg_flux_term_t &tm = cc.term[m];
      if (tm.prog < 0 || tm.prog >= fx->nprogs) { set_error("%s: term %d of component %d names program %d; there are %d programs", who, m, c, tm.prog, fx->nprogs); return -1; }
      const int pc = flux_code(tm.plus), mc = flux_code(tm.minus);
      if (pc < 0 || mc < 0) {
        set_error("%s: term %d of component %d reads [%d, %d, %d] and [%d, %d, %d]; each must be the cell or a unit axis offset in x or y", who, m, c,
                  tm.plus[0], tm.plus[1], tm.plus[2], tm.minus[0], tm.minus[1], tm.minus[2]);
        return -1;
      }
      cd.term[m] = FluxTermDev{tm.prog, pc, mc, tm.scale};
    }
  }
  for (int p = 0; p < fx->nprogs; ++p) {
    if (!flux_expr_ok(who, p, &fx->prog[p], fx->nfields)) return -1;
    a.prog[p] = pack_program(&fx->prog[p]);
  }
  const Box box = make_box(begin, end);
  if (box.count() == 0) return 0;
  if (box.b2 != 0 || box.e2 != 1) { set_error("%s: 2-D box must have [0,1) in dim 2", who); return -1; }
  if (!box_inside(&fx->lout, box, 0)) { set_error("%s: box leaves the output allocation", who); return -1; }
  if (!box_inside(&fx->lin, box, 1)) { set_error("%s: box grown by one cell leaves the input allocation", who); return -1; }
  a.box = box;
  return g_flux_route ? g_flux_route : FLUX_DEFAULT_ROUTE;
}

}  // namespace examg

using namespace examg;

#ifdef EXAMG_DEBUG_HOOKS
extern "C" int examg_debug_flux_route(int route) {
  if (route != 0 && route != EXAMG_FLUX_GATHER && route != EXAMG_FLUX_MARCH) return 1;
  g_flux_route = route;
  return 0;
}
#endif

extern "C" int examg_flux_route(const examg_flux_t *fx, const int32_t *begin, const int32_t *end) {
  FluxArgs a;
  return flux_prepare("examg_flux_route", fx, begin, end, a);
}

extern "C" int examg_flux_step(const examg_flux_t *fx, const int32_t *begin, const int32_t *end, examg_stream_t stream) {
  FluxArgs a;
  const int route = flux_prepare("examg_flux_step", fx, begin, end, a);
  if (route < 0) return 1;
  if (route == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const Box &box = a.box;
  if (route == EXAMG_FLUX_GATHER) {
    const long long nb = ((long long)box.n0() * box.n1() + 255) / 256;
    if (nb > 0x7fffffffLL) { set_error("examg_flux_step: grid too large"); return 1; }
    hipLaunchKernelGGL(k_flux_gather, dim3((unsigned)nb), dim3(256), 0, s, a);
    EXAMG_CHECK_LAUNCH("k_flux_gather");
    return 0;
  }
  // rows per wave: long chunks amortise the two rows that fill the ring, short ones keep the chip busy on small boxes
  const int ntx = (box.n0() + FLUX_WIN - 1) / FLUX_WIN;
  int chunk = 32;
  while (chunk > 8 && (long long)ntx * ((box.n1() + chunk - 1) / chunk) < 2048) chunk >>= 1;
  const int nch = (box.n1() + chunk - 1) / chunk;
  const long long waves = (long long)ntx * nch;
  if ((waves + 3) / 4 > 0x7fffffffLL) { set_error("examg_flux_step: grid too large"); return 1; }
  hipLaunchKernelGGL(k_flux_march, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a, ntx, nch, chunk);
  EXAMG_CHECK_LAUNCH("k_flux_march");
  return 0;
}

extern "C" int examg_reduce_expr_cell(int op, int nfields, const examg_layout_t *l, const double *const *x, const examg_nlexpr_t *prog,
                                      const int32_t *begin, const int32_t *end, double *result, void *work, examg_stream_t stream) {
  const char *who = "examg_reduce_expr_cell";
  if (!l || !x || !prog || !begin || !end || !result || !work) { set_error("%s: null argument", who); return 1; }
  if (op != EXAMG_REDUCE_MAX && op != EXAMG_REDUCE_MIN) { set_error("%s: unknown reduction %d", who, op); return 1; }
  if (l->nd != 2 && l->nd != 3) { set_error("%s: 2-D or 3-D layouts (nd = %d)", who, l->nd); return 1; }
  if (!flux_layout_ok(who, "field", l)) return 1;
  if (nfields < 1 || nfields > EXAMG_FLUX_MAX_FIELDS) { set_error("%s: %d fields (1 .. %d)", who, nfields, EXAMG_FLUX_MAX_FIELDS); return 1; }
  if (!flux_expr_ok(who, 0, prog, nfields)) return 1;
  RedExprArgs a;
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < nfields; ++k) {
    if (!x[k]) { set_error("%s: field %d is a null pointer", who, k); return 1; }
    a.x[k] = x[k];
  }
  const Box box = make_box(begin, end);
  hipStream_t s = (hipStream_t)stream;
  int nb = 0;      // an empty box: the final stage alone writes the identity
  if (box.count() > 0) {
    if (l->nd == 2 && (box.b2 != 0 || box.e2 != 1)) { set_error("%s: 2-D box must have [0,1) in dim 2", who); return 1; }
    if (!box_inside(l, box, 0)) { set_error("%s: box leaves the allocation", who); return 1; }
    a.l = make_layout(l);
    a.nfields = nfields;
    a.box = box;
    a.prog = pack_program(prog);
    const long long want = (box.count() + FLUX_RED_BLOCK * 4 - 1) / (FLUX_RED_BLOCK * 4);
    nb = (int)(want > FLUX_RED_MAX_BLOCKS ? FLUX_RED_MAX_BLOCKS : want);
    if (op == EXAMG_REDUCE_MAX) hipLaunchKernelGGL((k_reduce_expr_partial<true>), dim3(nb), dim3(FLUX_RED_BLOCK), 0, s, a, (double *)work);
    else hipLaunchKernelGGL((k_reduce_expr_partial<false>), dim3(nb), dim3(FLUX_RED_BLOCK), 0, s, a, (double *)work);
  }
  if (op == EXAMG_REDUCE_MAX) hipLaunchKernelGGL((k_reduce_expr_final<true>), dim3(1), dim3(FLUX_RED_BLOCK), 0, s, (const double *)work, nb, result);
  else hipLaunchKernelGGL((k_reduce_expr_final<false>), dim3(1), dim3(FLUX_RED_BLOCK), 0, s, (const double *)work, nb, result);
  EXAMG_CHECK_LAUNCH("k_reduce_expr");
  return 0;
}
