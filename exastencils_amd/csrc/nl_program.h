// Point programs (examg_nlexpr_t) as the kernels take them, and their interpreter.  Shared by the semilinear kernels
// (kernels_nonlinear.hip: one operand, EXAMG_OP_U) and the flux kernels (kernels_flux.hip: up to EXAMG_FLUX_MAX_FIELDS operands,
// EXAMG_OP_FIELD0 + k).
//
// The programs are interpreted wave-uniformly: the instruction stream is a kernel argument, read through scalar loads (once, into
// scalar registers: the opcodes are packed), the dispatch is scalar branches, every lane executes the same instruction on its own
// operands.  The operand stack is eight named registers (the top of the stack and seven below it) selected by the uniform stack
// pointer through scalar branches -- never an indexed array, so nothing goes to scratch.
#pragma once
#include "examg_common.h"

namespace examg {

// A program as the kernel takes it: the opcodes packed eight to a 64-bit word (four scalar register pairs hold a whole program: the
// dispatch loop reads no memory), the literals of its CONST instructions in order of appearance.
struct NlProg {
  int n, nconst;
  unsigned long long w[EXAMG_MAX_NL_EXPR / 8];
  double pool[EXAMG_MAX_NL_EXPR + 1];
};

static inline NlProg pack_program(const examg_nlexpr_t *e) {
  NlProg p;
  memset(&p, 0, sizeof(p));
  p.n = e->n;
  for (int i = 0; i < e->n; ++i) {
    p.w[i >> 3] |= (unsigned long long)(e->op[i] & 255) << (8 * (i & 7));
    if (e->op[i] == EXAMG_OP_CONST) p.pool[p.nconst++] = e->c[i];
  }
  return p;
}

// A program on R values per lane at once (R = 1: the gather kernels; the row-marching kernels interpret every instruction once for the
// R rows a lane holds).  NF = 1: the one operand f[0] is pushed by EXAMG_OP_U; NF > 1: operand k by EXAMG_OP_FIELD0 + k (the host has
// checked k against the number of fields; operands behind it are never pushed).  sp counts the values on the stack; the top one is
// t, the ones below s0 (bottom) .. s6.  The literal of the next CONST instruction is fetched one instruction ahead (cnext), so its
// scalar load is in flight while the instructions before it execute.
#define NL_R(stmt) _Pragma("unroll") for (int r = 0; r < R; ++r) { stmt; }
template <int R, int NF>
__device__ __forceinline__ void nl_eval_fields(const NlProg &e, const double (&f)[NF][R], double (&res)[R]) {
  double t[R], s0[R], s1[R], s2[R], s3[R], s4[R], s5[R], s6[R];
  NL_R(t[r] = 0.0; s0[r] = 0.0; s1[r] = 0.0; s2[r] = 0.0; s3[r] = 0.0; s4[r] = 0.0; s5[r] = 0.0; s6[r] = 0.0)
  int sp = 0, ci = 0;
  const unsigned long long w0 = e.w[0], w1 = e.w[1], w2 = e.w[2], w3 = e.w[3];
  double cnext = e.pool[0];
  for (int i = 0; i < e.n; ++i) {
    const int j = i >> 3;
    const unsigned long long w = j == 0 ? w0 : (j == 1 ? w1 : (j == 2 ? w2 : w3));
    const int op = (int)((w >> (8 * (i & 7))) & 255u);
    const bool operand = NF == 1 ? op == EXAMG_OP_U : (op >= EXAMG_OP_FIELD0 && op < EXAMG_OP_FIELD0 + NF);
    if (op == EXAMG_OP_CONST || operand) {
      switch (sp) {                  // push: the old top goes below
        case 1: NL_R(s0[r] = t[r]) break;
        case 2: NL_R(s1[r] = t[r]) break;
        case 3: NL_R(s2[r] = t[r]) break;
        case 4: NL_R(s3[r] = t[r]) break;
        case 5: NL_R(s4[r] = t[r]) break;
        case 6: NL_R(s5[r] = t[r]) break;
        case 7: NL_R(s6[r] = t[r]) break;
        default: break;
      }
      if (op == EXAMG_OP_CONST) {
        NL_R(t[r] = cnext)
        ++ci;
        cnext = e.pool[ci];
      } else if (NF == 1) {
        NL_R(t[r] = f[0][r])
      } else {
        switch (op - EXAMG_OP_FIELD0) {      // the operand's registers by name
          case 0: NL_R(t[r] = f[0][r]) break;
          case 1: NL_R(t[r] = f[NF > 1 ? 1 : 0][r]) break;
          case 2: NL_R(t[r] = f[NF > 2 ? 2 : 0][r]) break;
          case 3: NL_R(t[r] = f[NF > 3 ? 3 : 0][r]) break;
          case 4: NL_R(t[r] = f[NF > 4 ? 4 : 0][r]) break;
          default: NL_R(t[r] = f[NF > 5 ? 5 : 0][r]) break;
        }
      }
      ++sp;
      continue;
    }
    if (op == EXAMG_OP_ADD || op == EXAMG_OP_SUB || op == EXAMG_OP_MUL || op == EXAMG_OP_DIV || op == EXAMG_OP_POW || op == EXAMG_OP_MAX ||
        op == EXAMG_OP_MIN) {
      double a[R];                   // the value below the top
      switch (sp) {
        case 2: NL_R(a[r] = s0[r]) break;
        case 3: NL_R(a[r] = s1[r]) break;
        case 4: NL_R(a[r] = s2[r]) break;
        case 5: NL_R(a[r] = s3[r]) break;
        case 6: NL_R(a[r] = s4[r]) break;
        case 7: NL_R(a[r] = s5[r]) break;
        default: NL_R(a[r] = s6[r]) break;
      }
      --sp;
      switch (op) {
        case EXAMG_OP_ADD: NL_R(t[r] = a[r] + t[r]) break;
        case EXAMG_OP_SUB: NL_R(t[r] = a[r] - t[r]) break;
        case EXAMG_OP_MUL: NL_R(t[r] = a[r] * t[r]) break;
        case EXAMG_OP_DIV: NL_R(t[r] = a[r] / t[r]) break;
        case EXAMG_OP_POW: NL_R(t[r] = pow(a[r], t[r])) break;
        case EXAMG_OP_MAX: NL_R(t[r] = fmax(a[r], t[r])) break;
        default: NL_R(t[r] = fmin(a[r], t[r])) break;
      }
      continue;
    }
    switch (op) {
      case EXAMG_OP_NEG: NL_R(t[r] = -t[r]) break;
      case EXAMG_OP_SIN: NL_R(t[r] = sin(t[r])) break;
      case EXAMG_OP_COS: NL_R(t[r] = cos(t[r])) break;
      case EXAMG_OP_EXP: NL_R(t[r] = exp(t[r])) break;
      case EXAMG_OP_SINH: NL_R(t[r] = sinh(t[r])) break;
      case EXAMG_OP_COSH: NL_R(t[r] = cosh(t[r])) break;
      case EXAMG_OP_SQRT: NL_R(t[r] = sqrt(t[r])) break;
      case EXAMG_OP_TAN: NL_R(t[r] = tan(t[r])) break;
      case EXAMG_OP_LOG: NL_R(t[r] = log(t[r])) break;
      case EXAMG_OP_FABS: NL_R(t[r] = fabs(t[r])) break;
      default: NL_R(t[r] = tanh(t[r])) break;
    }
  }
  NL_R(res[r] = t[r])
}

// the semilinear kernels' form: one operand
template <int R>
__device__ __forceinline__ void nl_eval(const NlProg &e, const double (&v)[R], double (&res)[R]) {
  nl_eval_fields<R, 1>(e, reinterpret_cast<const double (&)[1][R]>(v), res);
}

}  // namespace examg
