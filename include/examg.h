/*
 * examg.h -- C ABI of libexamg: the MI355X (gfx950) multigrid hot path that drops in where
 * ExaStencils' generated CUDA kernel wrappers sit.
 *
 * What this replaces.  For every device-eligible `loop over` the reference generator prints
 *     extern "C" void <fn>_k<NNN>_wrapper(<pass-through args>[, double* reductionTmp])
 * into Kernel/Kernel_<fn>_k<NNN>.cu (Compiler/src/exastencils/parallelization/api/cuda/
 * CUDA_Kernel.scala:546-632, naming CUDA_KernelFunctions.scala:78-110, call site
 * CUDA_ExtractDeviceCode.scala:262-280), called from generated host functions mgCycle_<lvl>(),
 * Solve_<lvl>() on process-global device arrays fieldDeviceData_<F>[lvl][slot]
 * (cuda/CUDA_Memory.scala:121-141) laid out as IR_FieldLayout prescribes
 * (field/ir/IR_FieldLayout.scala:30-129).  The <NNN> numbering is an artefact of strategy order,
 * so this header defines one *semantic* entry point per kind of emitted loop; INTEGRATION.md shows
 * the one-line `_wrapper` shims a maintainer adds to bind them.
 *
 * Conventions (same as the generated code):
 *   - all pointers are DEVICE pointers owned by the caller (setupBuffers()/destroyGlobals(),
 *     globals/ir/IR_AddInternalVariables.scala:115-182); nothing here allocates or frees;
 *   - fields are raw double arrays in the reference layout, x fastest
 *     (baseExt/ir/IR_Linearization.scala:27-36); `examg_layout_t` carries the per-dimension
 *     pad|ghost|dup|inner|dup|ghost|pad counts, referenceOffset = pad_l + ghost_l;
 *   - loop bounds `begin`/`end` are in iterator coordinates (0 = lower duplicate node), half-open,
 *     exactly the `_cu_begin_d`/`_cu_end_d` kernel arguments (cuda/CUDA_Kernel.scala:364-393) that
 *     baseExt/ir/IR_LoopOverPointsInOneFragment.scala:84-101 computes; unused dims use [0,1);
 *   - `stream` is a hipStream_t (cuda/CUDA_Stream.scala:96-202); launches are asynchronous and
 *     capturable into a hipGraph; no call synchronises the device;
 *   - return value: 0 on success, non-zero on error with a message in examg_last_error().
 *     (The reference wrappers are void and print+exit on error, cuda/CUDA_Error.scala; the
 *     reference-named shims in INTEGRATION.md reproduce that on top of these.)
 *   - arithmetic: fp64, each statement evaluated in the order the generator prints it
 *     (stencil entries folded left to right, stencil/ir/IR_StencilConvolution.scala:65-68),
 *     no FMA contraction -- point-wise results are bit-identical to the CPU path.
 */
#ifndef EXAMG_H
#define EXAMG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXAMG_MAX_ENTRIES 27

/* field/ir/IR_FieldLayout.scala:103-129 (IR_FieldLayoutPerDim). Unused dims: inner = 1, rest 0.
 * transform: the field under a layout transformation of the program's `LayoutTransformations` block (layoutTransformation/ir/
 * IR_LayoutTransformStatement.scala; Testing/LayoutTrafo/rbgs.exa4:2).  EXAMG_LAYOUT_SPLIT_X is the colour split
 * `transform <field> with [x, y, z] => [x / 2, y, z, x % 2]`: with ax = array index in x (iterator + referenceOffset) the value of a
 * point lives at  ax / 2 + H * (ay + TOTy * (az + TOTz * (ax % 2))),  H = ceil(TOTx / 2): the even and the odd columns of every row
 * are two contiguous half rows in two half arrays, so the points of one red-black colour of a row -- and their x neighbours -- are
 * contiguous (32 B per update for a half sweep instead of 48).  A transformation changes where a value lives, never a value; regions,
 * iterator coordinates and boxes are those of the untransformed layout.  Entry points that have no form for a transformed layout
 * refuse it (examg_last_error); examg_transform_field converts. */
enum { EXAMG_LAYOUT_PLAIN = 0, EXAMG_LAYOUT_SPLIT_X = 1 };
typedef struct examg_layout {
  int32_t nd;
  int32_t pad_l[3], ghost_l[3], dup_l[3], inner[3], dup_r[3], ghost_r[3], pad_r[3];
  int32_t transform; /* EXAMG_LAYOUT_* */
} examg_layout_t;

/* operator/ir/IR_Stencil.scala:34-211 (constant coefficients, entry order significant) or a
 * stencil field whose entry index is the slowest array dimension
 * (stencil/ir/IR_StencilConvolution.scala:73-95): cfield[k * size(clayout) + linear(clayout, i)].
 * ctransform: the coefficient field under a layout transformation (layoutTransformation/, the `LayoutTransformations` block of an
 * ExaSlang-4 program, Testing/LayoutTrafo/{rbgs,opts}.exa4) -- EXAMG_CLAYOUT_ENTRY_FASTEST is `transform <field> with [x, y, z, i] => [i, x, y, z]`:
 * the entries of a point are contiguous, cfield[linear(clayout, i) * nent + k]: ONE stream of 8 * nent bytes per point instead of
 * nent streams (27-entry fields: 30 -> 4 streams per sweep).  A transformation changes where values live, never a value. */
enum { EXAMG_CLAYOUT_PLANES = 0, EXAMG_CLAYOUT_ENTRY_FASTEST = 1 };
typedef struct examg_stencil {
  int32_t nent;
  int32_t diag; /* index of the (0,0,0) entry, `diag(A)` */
  int32_t off[EXAMG_MAX_ENTRIES][3];
  double coef[EXAMG_MAX_ENTRIES];
  const double *cfield; /* device pointer or NULL */
  examg_layout_t clayout;
  int32_t ctransform;   /* EXAMG_CLAYOUT_* */
  /* smoother weight of a stencil FIELD (EXAMG_SMOOTH with cfield): how the statement writes it.  EXAMG_WEIGHT_INV_TIMES:
   * `((1.0 / diag(A)) * omega)` (Testing/SISC/3D_VarCoeff.exa4:145) -- per point (1.0 / c_diag) * w;  EXAMG_WEIGHT_DIVIDE:
   * `(omega / diag(A))` (Testing/PolyExpl/RBGS3Dvc.exa4:52) -- per point w / c_diag.  Both round differently; the kernels evaluate
   * what the program says.  Constant stencils take the folded literal in `w` and ignore this. */
  int32_t wform;
} examg_stencil_t;
enum { EXAMG_WEIGHT_INV_TIMES = 0, EXAMG_WEIGHT_DIVIDE = 1 };

/* Uniform node grid of one fragment at one level: position = index * h + pos_begin
 * (grid/ir/IR_VF_NodePosition.scala:109-111, domain/ir/IR_DomainFromAABB.scala:31-40). */
typedef struct examg_geom {
  double pos_begin[3];
  double h[3];
} examg_geom_t;

typedef void *examg_stream_t; /* hipStream_t */

/* stencil loop kinds */
enum { EXAMG_APPLY = 0, EXAMG_RESIDUAL = 1, EXAMG_SMOOTH = 2 };

int examg_version(void);
const char *examg_last_error(void);
/* Number of visible HIP devices (cuda/CUDA_AddGlobals.scala:30-48 does cudaGetDeviceCount). */
int examg_device_count(void);

/* ---- K1/K2/K3: stencil loops ---------------------------------------------
 * mode EXAMG_APPLY    : dst = A*u                       (cgTmp1 = Laplace * cgTmp0, ...exa4:166-168)
 *      EXAMG_RESIDUAL : dst = rhs - A*u                 (Residual = RHS - Laplace * Solution, :215-219)
 *      EXAMG_SMOOTH   : dst = u + ww * (rhs - A*u)      (Jacobi, Testing/Smoothers/Jac.exa4:125-131;
 *                       with colour >= 0 and dst == u: one red-black half sweep, ...exa4:204-213)
 *   ww = w for constant stencils (w is the folded constant omega/diag(A));
 *   ww = (1.0 / cfield[diag]) * w for stencil fields (w = omega, Testing/SISC/3D_VarCoeff.exa4:145).
 * colour: -1 = all points, else only points with (i0+i1+i2) % 2 == colour
 *   (baseExt/l4/L4_ColorLoops.scala:44-66; condition emitted by IR_LoopOverDimensions.scala:215-216).
 * u and dst may alias only when colour >= 0 (or for disjoint boxes).
 * Every argument is indexed through its own layout: u through lu, rhs through lf, dst through ld and the coefficients of a stencil
 * field through st->clayout; the four may differ in ghost and pad widths (`cgTmp1 = Laplace * cgTmp0`: no ghost layers / one).  The
 * diagonal of a stencil field is entry st->diag, wherever it stands in the entry list.  Only the points of the box (of the colour)
 * are written, in dst alone; u, rhs and the coefficient array are read only -- constant stencils and stencil fields alike. */
int examg_stencil_op(int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs,
                     const examg_layout_t *ld, double *dst, const examg_stencil_t *st, double w, int colour,
                     const int32_t *begin, const int32_t *end, examg_stream_t stream);

/* Names of SURVEY.md 8b; thin forms of examg_stencil_op. */
int examg_jacobi(const examg_layout_t *lu, const double *u, double *u_next, const examg_layout_t *lf, const double *rhs,
                 const examg_stencil_t *st, double w, const int32_t *begin, const int32_t *end, examg_stream_t stream);
int examg_rbgs_colour(const examg_layout_t *lu, double *u, const examg_layout_t *lf, const double *rhs,
                      const examg_stencil_t *st, double w, int colour, const int32_t *begin, const int32_t *end,
                      examg_stream_t stream);
int examg_residual(const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs,
                   const examg_layout_t *lr, double *res, const examg_stencil_t *st, const int32_t *begin,
                   const int32_t *end, examg_stream_t stream);

/* ---- multi-colour loops: `color with { e_0, e_1, ... }` with more than one colour expression, or with an expression other than the
 * parity of all indices (baseExt/l4/L4_ColorLoops.scala:32-66; Examples/Stokes/2D_FV_Stokes_fromL4.exa4:588-591 `i0 % 3, i1 % 3`).
 * A COLOURING is a list of nexpr = 1 .. 3 expressions
 *     e_k = (shift[k] + sum of i_d over the axes d with bit d of axes[k] set) % mod[k]
 * mod[k] a positive constant, axes[k] a non-empty set of axes of the layout (bits below nd), shift[k] an integer constant, i_d the
 * loop's iterator coordinates (fragment-local, 0 = lower duplicate node: the coordinates of `colour` above).  A COLOUR fixes a
 * remainder rem[k] in [0, mod[k]) for every expression; a point belongs to it when every e_k == rem[k].
 * Order of the colour loops (L4_ColorLoops.toRepeatLoops): the body runs once per element of the cross product of the remainders, the
 * FIRST expression varying fastest: for `i0 % 2, i1 % 2, i2 % 2` the colours (0,0,0), (1,0,0), (0,1,0), (1,1,0), (0,0,1), ...
 * A colouring DECOUPLES a stencil when every entry offset o != 0 has an expression k with (sum of o_d over the axes of e_k) mod mod[k]
 * != 0: no point of a colour is then a neighbour of another point of that colour, and only then is an in-place loop over one colour
 * independent of the loop order -- only then may u and dst alias.  `i0 % 2, i1 % 2, i2 % 2` decouples every stencil of reach 1 (the
 * 8-colour Gauss-Seidel sweep of 27-point stencils: what red-black is for 7-point ones); the parity of all indices decouples star
 * stencils only.
 * The coloured entry points refuse a box in which shift[k] + sum of begin_d can be negative (C's % and the mathematical remainder
 * differ there, and the reference's loops never go there), nexpr outside 1 .. 3, mod <= 0, rem outside [0, mod), an empty or
 * out-of-range axis set, and fields under a layout transformation (EXAMG_LAYOUT_SPLIT_X) -- all before anything is launched. */
typedef struct examg_colouring {
  int32_t nexpr;
  int32_t axes[3];  /* bit d: i_d is a summand */
  int32_t shift[3];
  int32_t mod[3];
  int32_t rem[3];
} examg_colouring_t;

/* examg_stencil_op restricted to the points of one colour of `col`: the three loop kinds, any dimensionality and entry list, constant
 * stencils and stencil fields in both coefficient layouts, every argument through its own layout, the same arithmetic (entries folded
 * left to right, no contraction, ww in the form st->wform names).  Only the colour's points of the box are written, in dst alone.
 * u == dst is an error unless the colouring decouples st.  With nexpr == 1, all axes and mod 2 the result is, bit for bit, that of
 * examg_stencil_op(..., colour = (rem - shift) mod 2). */
int examg_stencil_op_coloured(int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs,
                              const examg_layout_t *ld, double *dst, const examg_stencil_t *st, double w, const examg_colouring_t *col,
                              const int32_t *begin, const int32_t *end, examg_stream_t stream);

/* One whole multi-colour Gauss-Seidel sweep of a block without neighbours: all mod[0] * mod[1] * .. colour loops of EXAMG_SMOOTH in
 * place on u, in the reference's order (col->rem is ignored) -- `color with { e_0, .., loop over u { u += ww * (rhs - A * u) } }`.
 * Bit-identical to that many examg_stencil_op_coloured calls.  Refuses a colouring that does not decouple st.
 * 27-entry stencil fields in the record layout under the axis-parity colouring `i0 % 2, i1 % 2, i2 % 2` (any shifts) run the colours
 * (0, c1, c2) and (1, c1, c2) in ONE launch (examg_mcgs_one_pass_eligible): a point of the second has exactly two neighbours in the
 * first, (x +- 1, y, z) in its own row, and no other point written by either loop is a neighbour of a point written by either; one
 * wave owns a whole row, updates its first x colour, makes the values visible to itself and updates the second from them.  A sweep is
 * 4 launches instead of 8, and every 216-byte coefficient record is read once. */
int examg_mcgs_sweep(const examg_layout_t *lu, double *u, const examg_layout_t *lf, const double *rhs, const examg_stencil_t *st, double w,
                     const examg_colouring_t *col, const int32_t *begin, const int32_t *end, examg_stream_t stream);

/* 1 if examg_mcgs_sweep runs its row-pair kernel for these arguments, 0 if it issues the colour loops one by one: 3-D, the colouring
 * `(s0 + i0) % 2, (s1 + i1) % 2, (s2 + i2) % 2`, a 27-entry stencil field of reach 1 under EXAMG_CLAYOUT_ENTRY_FASTEST with the
 * centre entry first, untransformed layouts. */
int examg_mcgs_one_pass_eligible(const examg_layout_t *lu, const examg_layout_t *lf, const examg_stencil_t *st, const examg_colouring_t *col,
                                 const int32_t *begin, const int32_t *end);

/* ---- lexicographic Gauss-Seidel: the in-place `loop over u { u = u + ww * (rhs - A * u) }` with NO colouring, the one loop whose result
 * depends on the order of its points.  The reference prints it as a sequential nest, x fastest; examg_gs_sweep computes exactly
 *     for i2 in [b2, e2): for i1 in [b1, e1): for i0 in [b0, e0):
 *         u[i] = u[i] + ww * (rhs[i] - fold_k(c_k * u[i + o_k]))
 * in place.  Arithmetic order: acc = c_0 * u[i + o_0]; acc = acc + c_k * u[i + o_k] for k = 1 .. nent - 1 in entry order; then
 * rhs[i] - acc; then ww * (..); then u[i] + (..) -- no contraction.  ww as in examg_stencil_op(EXAMG_SMOOTH): the folded constant `w`
 * for constant stencils; per point (1.0 / c_diag) * w or w / c_diag for stencil fields, as st->wform names.  A point reads the NEW value
 * of every neighbour that precedes it in the nest and lies inside the box, and the OLD value of every other one: later points, and
 * everything outside the box (boundary planes, ghost layers).  Nothing outside the box is written.  Forward sweep only (the reference
 * generates no backward one).  The kernels update the points on a parallel schedule that respects every dependency of the nest; as
 * each point is computed with the same operations in the same order, the result is the nest's bit for bit.
 * Supported: 2-D and 3-D node fields, u and rhs each in its own layout; every stencil whose offsets lie in {-1, 0, 1}^d -- 5-, 9-, 7-,
 * 27-point, asymmetric ones, entries in any order -- constant or a stencil field in planes, both weight forms.  Refused (non-zero,
 * examg_last_error, nothing written): offsets of reach 2, entry-fastest coefficient records, colour-split layouts, cell layouts (no
 * duplicate layers), a box whose one-point shell leaves the u allocation.  An empty box is a no-op that returns 0.
 * A sweep is a sequence of launches of one kernel on `stream` (or a single launch for small boxes): no host synchronisation, no
 * allocation -- capturable into a hipGraph; no workgroup ever waits for another one. */
int examg_gs_sweep(const examg_layout_t *lu, double *u, const examg_layout_t *lf, const double *rhs, const examg_stencil_t *st, double w,
                   const int32_t *begin, const int32_t *end, examg_stream_t stream);
/* What examg_gs_sweep does with these arguments, decided from them alone (nothing is launched): -1 refused (error text set), 0 empty
 * box, 1 one workgroup walks the point hyperplanes of the whole box, 2 tiles, one launch per tile hyperplane, 3 one launch per point
 * hyperplane (stencil fields of more than 9 entries on boxes of more than 128^3 points, where it is the faster schedule). */
int examg_gs_route(const examg_layout_t *lu, const examg_layout_t *lf, const examg_stencil_t *st, const int32_t *begin, const int32_t *end);

/* One full red-black sweep (colour `first`, then the other) out of place, in ONE pass over HBM: the points of
 * [begin,end) of u_out receive exactly (bit for bit) what the two examg_rbgs_colour calls would leave there;
 * outside the box at most the one-stencil-reach shell is touched, and only by copying u_in's values there; the
 * caller keeps u_out's duplicate/ghost shell valid the way the program does anyway (`apply bc` / `communicate`
 * after the loop) and swaps the two pointers.  24 B per update instead of 48 B.  3-D 7-point constant stencils
 * take the two-stage kernel (writes the box only); anything else -- every stencil field among it -- falls back to copy + two half
 * sweeps.  What holds for "the fallback" of this and of the following one-pass entry points holds for stencil fields: they have no
 * one-pass form except the 27-entry record form of examg_jacobi2 / examg_jacobi2_boxes / examg_jacobi_residual, the eligibility
 * queries answer 0 for them, and outside the box they write what the fallback is said to write. */
int examg_rbgs_sweep_fused(const examg_layout_t *lu, const double *u_in, double *u_out, const examg_layout_t *lf,
                           const double *rhs, const examg_stencil_t *st, double w, int first, const int32_t *begin,
                           const int32_t *end, examg_stream_t stream);

/* As examg_rbgs_sweep_fused with separate boxes, for blocks with neighbours: colour `first` on [begin1,end1) (points
 * outside keep u_in's value), then the other colour of that field on [begin2,end2), inside box 1; u_out receives both
 * colours on box 2 and is not touched elsewhere, on every path.  Box 1 = the loop's box shrunk by one point at interior faces, box 2 by
 * two: everything inside is independent of the halo exchange between the two half sweeps
 * (communicate inside `color with`, Benchmark/Poisson3D/3D_FD_Poisson_fromL4.exa4:204-213).  `tmp` is used by the fallback
 * path only (general stencils, short rows) and may be NULL otherwise. */
int examg_rbgs_sweep_fused_boxes(const examg_layout_t *lu, const double *u_in, double *u_out, double *tmp,
                                 const examg_layout_t *lf, const double *rhs, const examg_stencil_t *st, double w, int first,
                                 const int32_t *begin1, const int32_t *end1, const int32_t *begin2, const int32_t *end2,
                                 examg_stream_t stream);

/* Two Jacobi steps (Smoother called twice, Testing/Smoothers/Jac.exa4:125-131) in ONE pass: temporal blocking in the
 * sense of baseExt/ir/IR_ContractingLoop.scala.  u_out[box] = J(J(u_in)); bit-identical to two examg_jacobi calls
 * u_in -> tmp -> u_out.  Only valid when no halo exchange is needed between the two steps (single block, or ghost
 * layers two deep); `tmp` is used by the fallback path only (general stencils, small boxes) and may be NULL otherwise.
 * Outside the box nothing of u_out is written, on every path (the fallback keeps the shell it needs in `tmp`).
 * One-pass forms exist for the 3-D 7-point constant stencil and for 27-entry stencil fields in the record layout
 * (EXAMG_CLAYOUT_ENTRY_FASTEST, entry order of examg_init_helmholtz27: the two steps of a point share its 216 B of coefficients). */
int examg_jacobi2(const examg_layout_t *lu, const double *u_in, double *u_out, double *tmp, const examg_layout_t *lf,
                  const double *rhs, const examg_stencil_t *st, double w, const int32_t *begin, const int32_t *end,
                  examg_stream_t stream);

/* Three Jacobi steps in ONE pass (temporal blocking of depth 3: `repeat 5 times with contraction [1,1,1]` of
 * Testing/PolyExpl/Jac3Dcc.exa4:27 runs as 3 + 2; baseExt/ir/IR_ContractingLoop.scala:45-196): u_out[box] = J(J(J(u_in))), bit-identical
 * to three examg_jacobi calls.  Same conditions as examg_jacobi2 (no halo exchange needed in between); the one-pass form exists for the
 * 3-D 7-point constant stencil on rows of at least 64 points; otherwise a step into `tmp` and a pair from there (`tmp` must then be a
 * distinct array; NULL is allowed where the one-pass form applies).  Outside the box: the one-pass form (examg_three_stage_eligible)
 * writes nothing; so does the fallback where the pair after its first step runs in one pass (examg_two_stage_eligible with both
 * boxes = [begin,end)); otherwise it copies u_in's values to the box's one-stencil-reach shell of u_out, and nothing further out. */
int examg_jacobi3(const examg_layout_t *lu, const double *u_in, double *u_out, double *tmp, const examg_layout_t *lf,
                  const double *rhs, const examg_stencil_t *st, double w, const int32_t *begin, const int32_t *end,
                  examg_stream_t stream);

/* Three colour loops of a red-black smoother in ONE pass, out of place: colour `first`, the other colour, `first` again -- three sweeps
 * (`repeat 3 times { color with { ... } }`, Benchmark/Poisson3D/3D_FD_Poisson_fromL4.exa4:204-213) are two such passes, the second with
 * first = 1 - first.  u_out[box] = the three loops applied to u_in; bit-identical to three examg_rbgs_colour calls in place.  One-pass
 * form: 3-D 7-point constant stencil, rows of at least 64 points (examg_three_stage_eligible); otherwise a copy and the three loops.
 * Outside the box: the one-pass form writes nothing; the fallback copies u_in's values to the box's one-stencil-reach shell of u_out
 * and writes nothing further out. */
int examg_rbgs_colours3(const examg_layout_t *lu, const double *u_in, double *u_out, const examg_layout_t *lf, const double *rhs,
                        const examg_stencil_t *st, double w, int first, const int32_t *begin, const int32_t *end, examg_stream_t stream);

/* 1 if examg_jacobi3 / examg_rbgs_colours3 run their one-pass kernel for this box, 0 if they run their loops one after the other. */
int examg_three_stage_eligible(const examg_layout_t *lu, const examg_layout_t *lf, const examg_stencil_t *st, const int32_t *begin,
                               const int32_t *end);

/* 1 if the one-pass kernels that have the form (the three-step Jacobi pass of examg_jacobi3; the Jacobi pair of examg_jacobi2 /
 * examg_jacobi2_boxes on boxes of 192 rows and 8.4 * 10^6 points and more) fuse the six off-centre products of this stencil into their sums: a constant 7-point star in one of the two canonical entry orders whose six off-centre coefficients are
 * all finite, non-zero and of magnitude exactly 2^e, e >= 0 (1/h^2 of every power-of-two grid; -1.0).  Such a product c * x is exact, so
 * acc + c * x and fma(c, x, acc) round the same number once: the pass stays bit-identical to the loops for all inputs whose products
 * c * x are finite.  Beyond 2^1024 a fused product can survive where a separate one became inf; NaN payloads are not compared.  The
 * centre product and c + w * (f - acc) are never fused.  0 for every other stencil: separate products and sums, as in the loops. */
int examg_pow2_fma_eligible(const examg_stencil_t *st);

/* One Jacobi step on [begin,end) and the residual of its result in ONE pass: u_out = J(u_in), res = rhs - A u_out on the box (the
 * last pre-smoothing `Smoother@current` + `Residual@current = RHS - Laplace * Solution`, Testing/SISC/3D_VarCoeff.exa4:141-153,
 * Benchmark/Poisson3D/3D_FD_Poisson_fromL4.exa4:215-219).  27-entry stencil fields in the record layout (EXAMG_CLAYOUT_ENTRY_FASTEST,
 * entry order of examg_init_helmholtz27) share the 216 B of coefficients per point between the two loops; everything else runs
 * examg_jacobi, then examg_residual.  The residual reads the one-point shell of the box from u_in: bit-identical to those two calls
 * when u_out holds u_in's values there (the slots of a field after `apply bc` / `communicate`).  u_in != u_out.  Outside the box
 * nothing of u_out or res is written. */
int examg_jacobi_residual(const examg_layout_t *lu, const double *u_in, double *u_out, const examg_layout_t *lf, const double *rhs,
                          const examg_layout_t *lr, double *res, const examg_stencil_t *st, double w, const int32_t *begin,
                          const int32_t *end, examg_stream_t stream);

/* As examg_jacobi2 with separate boxes: stage 1 = J on [begin1,end1) (points outside keep u_in's value), stage 2 = J of
 * that field on [begin2,end2), inside box 1, written to u_out.  With block neighbours: box 1 = the loop's box, box 2 =
 * box 1 without the duplicate planes at interior faces, whose second step needs the neighbour's first-step values
 * (halo exchange of the intermediate field, then a thin single-step launch on those planes).  u_out is written on box 2 only,
 * on every path. */
int examg_jacobi2_boxes(const examg_layout_t *lu, const double *u_in, double *u_out, double *tmp, const examg_layout_t *lf,
                        const double *rhs, const examg_stencil_t *st, double w, const int32_t *begin1, const int32_t *end1,
                        const int32_t *begin2, const int32_t *end2, examg_stream_t stream);

/* examg_rbgs_sweep_fused for a u_in that is 0.0 everywhere, boundary planes included -- a coarse level's first pre-smoothing
 * sweep after `Solution@coarser = 0` (mgCycle, Benchmark/Poisson3D/3D_FD_Poisson_fromL4.exa4:225-229 followed by :204-213): u_in is
 * not passed and not read (16 B per point instead of 24, and the zeroing loop need not run), the arithmetic is the same
 * expression evaluated on the constant 0.0: bit-identical.  Outside the box: the one-pass kernels (examg_two_stage_eligible with
 * both boxes = [begin,end)) write nothing; the fallback zeroes the box's one-stencil-reach shell of u_out. */
int examg_rbgs_sweep_fused_zero(const examg_layout_t *lu, double *u_out, const examg_layout_t *lf, const double *rhs,
                                const examg_stencil_t *st, double w, int first, const int32_t *begin, const int32_t *end,
                                examg_stream_t stream);

/* `Solution += Prolongation@coarser * Solution@coarser` on [begin,end) followed by the first post-smoothing pass on the same box
 * (mgCycle, Benchmark/Poisson3D/3D_FD_Poisson_fromL4.exa4:240-247: correction loop, `apply bc`, smoother) in ONE pass: the
 * one-pass kernels interpolate the coarse values (1/8 of the points, staged through LDS) while they load u_in, instead of a
 * separate read-modify-write loop over the fine field (16 B per point).  u_in is not modified; u_out receives on the box
 * exactly (bit for bit) what examg_prolong_add on u_in followed by examg_rbgs_sweep_fused / examg_jacobi2 would put there.
 * Single block only (the correction's `communicate` and the halo exchanges of the smoother must be empty).  Arguments that the
 * one-pass kernel does not take (examg_two_stage_eligible with both boxes = [begin,end)) run copy + the plain loops.  Outside the
 * box: the one-pass kernels write nothing; the fallback of examg_rbgs_sweep_fused_prolong and of examg_jacobi2_prolong copies
 * u_in's values to the box's one-stencil-reach shell of u_out and writes nothing further out. */
int examg_rbgs_sweep_fused_prolong(const examg_layout_t *lu, const double *u_in, double *u_out, const examg_layout_t *lf,
                                   const double *rhs, const examg_stencil_t *st, double w, int first, const int32_t *begin,
                                   const int32_t *end, const examg_layout_t *lc, const double *uc, examg_stream_t stream);
int examg_jacobi2_prolong(const examg_layout_t *lu, const double *u_in, double *u_out, double *tmp, const examg_layout_t *lf,
                          const double *rhs, const examg_stencil_t *st, double w, const int32_t *begin, const int32_t *end,
                          const examg_layout_t *lc, const double *uc, examg_stream_t stream);

/* 1 if examg_jacobi2_boxes / examg_rbgs_sweep_fused_boxes will run their one-pass kernel for these arguments, 0 if they will
 * take the fallback that writes `tmp` on the launch stream (other stencils or entry orders, short rows, boxes at the edge of
 * the allocation, planes of 2^32 elements or more).  A caller that overlaps the pass with work on `tmp` on another stream, or that
 * passes no `tmp`, must ask here first.  The entry points take their route from the function that answers here: where the answer
 * is 1 they neither read nor write `tmp`.  (Where it is 0, examg_jacobi2 / examg_jacobi2_boxes may still run 27-entry record
 * fields in one pass.) */
int examg_two_stage_eligible(const examg_layout_t *lu, const examg_layout_t *lf, const examg_stencil_t *st, const int32_t *begin1,
                             const int32_t *end1, const int32_t *begin2, const int32_t *end2);

/* `Residual = RHS - A * Solution` followed by `RHS@coarser = scale * R * Residual` (mgCycle,
 * Benchmark/Poisson3D/3D_FD_Poisson_fromL4.exa4:215-223) as ONE pass when nothing else reads the fine residual: it is never
 * written (48 + 8 B per fine point -> 16 B).  [fbegin,fend): the residual loop's box; [cbegin,cend): the restriction loop's
 * box, whose fine footprint must lie inside it (a block without neighbours; with neighbours the restriction reads residuals
 * on ghost points, which only an exchange of the stored field provides -- use the two calls).  3-D 7-point constant
 * stencils on long rows take the fused kernel and never touch `res`/`lr` (may be NULL); everything else runs
 * examg_residual + examg_restrict through `res`.  Bit-identical to the two calls either way.
 * The fallback is exactly those two calls with their contracts: `res` receives the residual on [fbegin, fend) and is read on the
 * fine footprint [2 * cbegin - 1, 2 * (cend - 1) + 1] of the restriction, which must lie in its allocation `lr` (points of the
 * footprint outside [fbegin, fend) are read as `res` holds them); `lr` and `res` are then required (an error without them).
 * Either way only the box [cbegin, cend) of fc is written, u and rhs are not modified, and no two arrays may overlap. */
int examg_residual_restrict(const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs,
                            const examg_layout_t *lr, double *res, const examg_stencil_t *st, const examg_layout_t *lc,
                            double *fc, double scale, const int32_t *fbegin, const int32_t *fend, const int32_t *cbegin,
                            const int32_t *cend, examg_stream_t stream);
/* 1 if examg_residual_restrict will run its one-pass kernel for these arguments (and leave `res` untouched), else 0 */
int examg_residual_restrict_one_pass(const examg_layout_t *lu, const examg_layout_t *lf, const examg_stencil_t *st, const examg_layout_t *lc,
                                     const int32_t *fbegin, const int32_t *fend, const int32_t *cbegin, const int32_t *cend);

/* ---- K4: RHS@coarser = scale * R * Residual, R = kron [1/4 1/2 1/4]
 * (operator/l4/L4_DefaultRestriction.scala:29-36,63-88; solver/ir/IR_ResolveIntergridIndices.scala);
 * begin/end: coarse iterator box.  For every coarse point I of the box
 *   rhs_coarse(I) = sum over o in {-1, 0, 1}^d of (scale * ((w(o0) * w(o1)) * w(o2))) * res_fine(2I + o),   w = 1/4, 1/2, 1/4
 * the terms added in entry order of the composed stencil: the x offset outermost, then y, then z, each -1, 0, +1 (2-D: no z
 * factor and no z offset; dim 2 of the box is [0, 1)).
 * Footprints: the box must lie in the coarse allocation and the fine points [2 * begin - 1, 2 * (end - 1) + 1] of every dimension
 * of the layouts in the fine allocation (ghost and pad points count) -- else an error, and nothing is launched.  A box that holds
 * the duplicate points of a block with neighbours (begin 0 or end = cells + 1) reads the fine ghost layer.
 * Writes the box of rhs_coarse and nothing else; res_fine is not modified.  The two arrays must not overlap.  Either layout
 * may be colour-split (EXAMG_LAYOUT_SPLIT_X); nd must be 2 or 3.  An empty box is a no-op that returns 0. */
int examg_restrict(const examg_layout_t *lfine, const double *res_fine, const examg_layout_t *lcoarse,
                   double *rhs_coarse, double scale, const int32_t *begin, const int32_t *end,
                   examg_stream_t stream);

/* ---- K5: Solution += P@coarser * Solution@coarser, P = 2^d R^T
 * (operator/l4/L4_DefaultProlongation.scala:30-45; parity cases
 * stencil/ir/IR_FindStencilConvolutions.scala:135-156); begin/end: fine iterator box.  Per dimension an even fine index i takes
 * the coarse point i / 2 with weight 1, an odd one (i + 1) / 2 and then (i - 1) / 2 with weight 1/2 each:
 *   u_fine(i) = u_fine(i) + (sum of ((w0 * w1) * w2) * u_coarse(c0, c1, c2))
 * the terms added with the x entry outermost, then y, then z, the upper coarse neighbour first.
 * Footprints: the box must lie in the fine allocation, its indices must not be negative (the parity cases are those of the
 * reference's loop, which starts at the lower duplicate point 0), and the coarse points [begin / 2, end / 2] of every dimension
 * of the layouts must lie in the coarse allocation -- else an error, and nothing is launched.
 * Writes the box of u_fine and nothing else; u_coarse is not modified.  The two arrays must not overlap.  Either layout may
 * be colour-split; nd must be 2 or 3.  An empty box is a no-op that returns 0. */
int examg_prolong_add(const examg_layout_t *lcoarse, const double *u_coarse, const examg_layout_t *lfine,
                      double *u_fine, const int32_t *begin, const int32_t *end, examg_stream_t stream);

/* ---- K6: BLAS-1 loops (Benchmark/Poisson3D/3D_FD_Poisson_fromL4.exa4:160-198, 226-229) */
int examg_set(const examg_layout_t *l, double *x, double v, const int32_t *begin, const int32_t *end,
              examg_stream_t stream);
/* y = a*x + b*y, evaluated as the reference statements are written:
 * b==0: a*x (copy for a==1);  b==1: y + a*x;  a==1: x + b*y. */
int examg_axpby(const examg_layout_t *lx, const double *x, const examg_layout_t *ly, double *y, double a, double b,
                const int32_t *begin, const int32_t *end, examg_stream_t stream);
/* As examg_axpby with a = sign * (*num / *den) or b = (*num / *den) read from device memory
 * (CG's alpha and beta without a host round trip); which: 0 => a, 1 => b. */
int examg_axpby_dev(const examg_layout_t *lx, const double *x, const examg_layout_t *ly, double *y, double a,
                    double b, int which, double sign, const double *num, const double *den, const int32_t *begin,
                    const int32_t *end, examg_stream_t stream);

/* ---- K7: reductions (`loop over ... with reduction`, ...exa4:113-119; replaces
 * cuda/CUDA_Reduction.scala:84-131 + DefaultReductionKernel, cuda/CUDA_KernelFunctions.scala:112-238).
 * Result (one double) is written to device memory `result`; `work` is caller-owned scratch of
 * examg_reduce_work_bytes() bytes.  Deterministic (fixed tree) for a fixed box. */
size_t examg_reduce_work_bytes(void);
int examg_dot(const examg_layout_t *lx, const double *x, const examg_layout_t *ly, const double *y,
              const int32_t *begin, const int32_t *end, double *result, void *work, examg_stream_t stream);

/* `Residual = RHS - A * Solution` followed by the norm's reduction loop (`ResNorm`, Benchmark/Poisson3D/3D_FD_Poisson_fromL4.exa4:113-119
 * after :215-219) as ONE pass when nothing else reads the residual: *result (device) = sum over [begin,end) of (rhs - A u)^2, the
 * residual is not stored (16 B per point instead of 24 + 8).  [begin,end) is the reduction loop's box (the residual is only needed
 * there).  3-D 7-point constant stencils on long rows take the one-pass kernel and never touch `res` / `lr` (may be NULL); everything
 * else runs examg_residual + examg_dot through `res`.  Same partial sums every run; their order differs from examg_dot's (1e-15
 * relative).  `work`: examg_reduce_work_bytes() bytes. */
int examg_residual_norm2(const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs,
                         const examg_stencil_t *st, const int32_t *begin, const int32_t *end, const examg_layout_t *lr, double *res,
                         double *result, void *work, examg_stream_t stream);

/* ---- start values from the C library's generator (host side).  Programs of the reference's test suite initialise their solution
 * with `loop over F sequentially { F = native ( "((double)std::rand()/RAND_MAX)" ) }` (Testing/Opts/base.exa4:166-170), every
 * MPI process after std::srand(mpiRank) (parallelization/api/mpi/MPI_IVs.scala:41-45); their results files come from glibc's rand()
 * (TYPE_3 additive feedback generator).  examg_crand_seed / examg_crand_draw_host restate that generator, so that a host program
 * gets the reference's start values whatever C library it runs with: the next n values of (double)rand()/RAND_MAX into a HOST
 * buffer, in the order the generated loop nest draws them (x fastest; several draws per point interleave).  The caller places and
 * uploads them. */
typedef struct {
  uint32_t r[31];
  int32_t k;
} examg_crand_state_t;
int examg_crand_seed(examg_crand_state_t *state, uint32_t seed);
int examg_crand_draw_host(examg_crand_state_t *state, double *host_out, int64_t n);

/* ---- analytic expressions as stack programs: the ONE mechanism for boundary values, right-hand sides, exact solutions and
 * coefficient profiles (round 1 also had 17 built-in function ids of the reference's test programs; they are gone -- the same
 * expression trees now travel as programs, exastencils_amd/field.py:FN_PROGRAMS) --------------------------------------- ------------------------------------------------------------------------
 * The generator inlines whatever expression a program gives for boundary values, right-hand sides and exact solutions
 * into the loop body (boundary/ir/IR_DirichletBC.scala:37-40; `loop over RHS { RHS = <expr> }`).  A library cannot be
 * recompiled per program, so an expression over the node position travels as a postfix program that a generic kernel
 * evaluates per point, in the order the expression tree prescribes (same operations in the same order as the printed
 * code).  op[i]: EXAMG_OP_*; c[i]: the literal of a CONST instruction. */
#define EXAMG_MAX_EXPR 256
enum {
  EXAMG_OP_CONST = 0, EXAMG_OP_X = 1, EXAMG_OP_Y = 2, EXAMG_OP_Z = 3, EXAMG_OP_ADD = 4, EXAMG_OP_SUB = 5, EXAMG_OP_MUL = 6,
  EXAMG_OP_DIV = 7, EXAMG_OP_NEG = 8, EXAMG_OP_SIN = 9, EXAMG_OP_COS = 10, EXAMG_OP_EXP = 11, EXAMG_OP_SINH = 12,
  EXAMG_OP_COSH = 13, EXAMG_OP_SQRT = 14, EXAMG_OP_POW = 15, EXAMG_OP_TAN = 16, EXAMG_OP_LOG = 17, EXAMG_OP_FABS = 18,
  EXAMG_OP_MAX = 19, EXAMG_OP_MIN = 20, EXAMG_OP_TANH = 21
};
typedef struct {
  int32_t n;
  int32_t op[EXAMG_MAX_EXPR];
  double c[EXAMG_MAX_EXPR];
} examg_expr_t;

/* x[box] = e(node position): InitRHS, SetFuncDir, `loop over F { F = <expr> }`. */
int examg_fill_expr(const examg_layout_t *l, double *x, const examg_geom_t *g, const examg_expr_t *e, const int32_t *begin,
                    const int32_t *end, examg_stream_t stream);
/* All faces of `apply bc` in one launch (boundary/ir/IR_DirichletBC.scala:37-40 over the ranges of
 * boundary/ir/IR_ApplyBCFunction.scala:53-83): face_mask bit (2*d + (side>0)) set => that face has no neighbour
 * (IR_IV_NeighborIsValid false) and gets its duplicate plane, tangentially GLB..GRE, set to e(node position). */
int examg_apply_dirichlet_expr(const examg_layout_t *l, double *x, const examg_geom_t *g, const examg_expr_t *e,
                               uint32_t face_mask, examg_stream_t stream);
/* `loop over F only dup [dir] on boundary { F = <expr> }` for every direction of the mask in one launch (the SetFuncDir loops of
 * Testing/FMG/3D_Trigonometric.exa4:189-201; baseExt/ir/IR_LoopOverPointsInOneFragment.scala:57-70): the duplicate plane of each
 * physical face, tangentially DLB..DRE.  Same values as one examg_fill_expr per face (edges are written by two faces: same value). */
int examg_fill_dup_faces_expr(const examg_layout_t *l, double *x, const examg_geom_t *g, const examg_expr_t *e,
                              uint32_t face_mask, examg_stream_t stream);
/* max |x - e(node position)| over the box (`loop over F with reduction(max : err)`); result in device memory */
int examg_max_err_expr(const examg_layout_t *l, const double *x, const examg_geom_t *g, const examg_expr_t *e,
                       const int32_t *begin, const int32_t *end, double *result, void *work, examg_stream_t stream);

/* ---- the same three over the node tables of an axis-aligned, non-uniform grid (grid_isUniform = false, grid_isAxisAligned = true;
 * grid/ir/IR_SetupNodePositions.scala).  examg_grid_t: per axis d of the layout a DEVICE array nodes[d] of n[d] node positions; element j
 * is the position of the node with iterator index j - ghost (ghost nodes of the table in front).  The position of point i is
 * nodes[d][i_d + ghost]; programs may also read the width of the point's cell, nodes[d][i_d + ghost + 1] - nodes[d][i_d + ghost], through
 * EXAMG_OP_WX / WY / WZ (`vf_cellWidth_*`; `vf_cellVolume` is their product, spelt out by the caller).  On an axis the layout does not have,
 * position and width are 0.0.  Otherwise the arithmetic, the boxes and the faces are those of examg_fill_expr, examg_apply_dirichlet_expr
 * and examg_max_err_expr -- one kernel each, instantiated for the two kinds of geometry.  The width opcodes are refused by every entry
 * point that takes an examg_geom_t.  Refused before anything is launched: a box (a face, its tangential ghost range included) with a point
 * whose node or whose cell's upper node the table does not hold; a layout under a layout transformation. */
#define EXAMG_OP_WX 23
#define EXAMG_OP_WY 24
#define EXAMG_OP_WZ 25
typedef struct examg_grid {
  const double *nodes[3];
  int32_t n[3];
  int32_t ghost;
} examg_grid_t;
int examg_fill_expr_grid(const examg_layout_t *l, double *x, const examg_grid_t *g, const examg_expr_t *e, const int32_t *begin,
                         const int32_t *end, examg_stream_t stream);
int examg_apply_dirichlet_expr_grid(const examg_layout_t *l, double *x, const examg_grid_t *g, const examg_expr_t *e, uint32_t face_mask,
                                    examg_stream_t stream);
int examg_max_err_expr_grid(const examg_layout_t *l, const double *x, const examg_grid_t *g, const examg_expr_t *e, const int32_t *begin,
                            const int32_t *end, double *result, void *work, examg_stream_t stream);

/* ---- stencil-field initialisation.  Testing/SISC/3D_VarCoeff.exa4:206-217 (2*nd+1 entries): -div(a grad u) with the
 * coefficient expression `a` evaluated half a mesh width to either side of the node.  With (x, y, z) the node position
 * (index * h + pos_begin) and, per dimension d, ap_d = a(position + (0.5 * h_d) in d), am_d = a(position - (0.5 * h_d) in d):
 *   entry 0 (0,0,0)   = ((ap_x + am_x) / (h_x * h_x)) + ((ap_y + am_y) / (h_y * h_y)) [+ ((ap_z + am_z) / (h_z * h_z))]
 *   entry 1 + 2d (+d) = (-1.0 * ap_d) / (h_d * h_d)
 *   entry 2 + 2d (-d) = (-1.0 * am_d) / (h_d * h_d)
 * in the planes layout (EXAMG_CLAYOUT_PLANES) of lc, on the points of [begin,end) only. */
int examg_init_varcoeff7(const examg_layout_t *lc, double *cfield, const examg_geom_t *g, const examg_expr_t *a,
                         const int32_t *begin, const int32_t *end, examg_stream_t stream);

/* 27-entry stencil field of -div(a grad u) - k^2 u (BASELINE.json config 4): trilinear elements with element-wise
 * constant a = a(element centre) (expression program), lumped mass, scaled by 1/h^3; ksq = k^2.
 * Entry order: (0,0,0), then the other 26 offsets (dx,dy,dz) with dz slowest and dx fastest: (-1,-1,-1), (0,-1,-1), (1,-1,-1),
 * (-1,0,-1), ... (1,1,1).  The elements are cubes: g->h[1] != g->h[0] or g->h[2] != g->h[0] is refused before anything is launched (the
 * error text names the three widths).  With h that one width and a_e = a(x +- 0.5 * h, y +- 0.5 * h, z +- 0.5 * h) for the eight
 * elements around the node (x, y, z the node position index * h + pos_begin; the half step is the product (+-0.5) * h), entry (dx,dy,dz) = (S * kf) / (h * h), S = the sum of a_e over the elements that hold both nodes (those on the side of every
 * non-zero offset component; added with the x side outermost and the z side innermost, the lower side first) and kf = 1.0 / 3.0
 * for the centre, 0.0 across an edge (one non-zero component), -1.0 / 12.0 across a face or body diagonal; the centre entry then has
 * ksq subtracted.  Planes layout of lc, the points of [begin,end) only.  The stencil-field mechanism is the reference's
 * (stencil/ir/IR_StencilConvolution.scala:73-95); the reference itself ships 2d+1-entry fields only. */
int examg_init_helmholtz27(const examg_layout_t *lc, double *cfield, const examg_geom_t *g, const examg_expr_t *a, double ksq,
                           const int32_t *begin, const int32_t *end, examg_stream_t stream);

/* Apply (to_entry_fastest = 1) or undo (0) the layout transformation `[x, y, z, i] => [i, x, y, z]` of a stencil field's
 * coefficient array: dst[linear * nent + k] <-> src[k * size(lc) + linear] over the whole allocation; src != dst. */
int examg_transform_stencilfield(const examg_layout_t *lc, int nent, const double *src, double *dst, int to_entry_fastest,
                                 examg_stream_t stream);

/* Copy a field between two layouts that differ in `transform` only (same regions): dst[index under ldst] = src[index under lsrc] over
 * the whole allocation; src != dst.  doubles of an array: examg_layout_size. */
int examg_transform_field(const examg_layout_t *lsrc, const double *src, const examg_layout_t *ldst, double *dst, examg_stream_t stream);
int64_t examg_layout_size(const examg_layout_t *l);

/* ---- K9: halo pack / unpack (communication/ir/IR_NoInterpPacking.scala:53-83): box <-> contiguous
 * buffer, x fastest; ranges from IR_PackInfoDuplicate.scala:15-39 / IR_PackInfoGhost.scala:13-60. */
int examg_pack(const examg_layout_t *l, const double *x, double *buf, const int32_t *begin, const int32_t *end,
               examg_stream_t stream);
int examg_unpack(const examg_layout_t *l, double *x, const double *buf, const int32_t *begin, const int32_t *end,
                 examg_stream_t stream);

/* ---- a-16: coarse-grid CG, mgCycle@coarsest (...exa4:152-201) as ONE persistent single-workgroup
 * kernel (no host round trips).  Fields in the reference layout.  info: >= 4 doubles in device memory, zeroed by the
 * caller once: info[0] = iterations, info[1] = initial residual, info[2] = final residual of this call; info[3] is
 * incremented when the loop ended at max_it without meeting the tolerance -- where the generated function prints
 * "Maximum number of cgs iterations (max_it) was exceeded" (the host reads the count when it next synchronises).  info may be
 * NULL.  An empty box is a solve of nothing: info[0..2] = 0, nothing else is written.
 * What is written: sol, res and p on [begin,end); ap on [begin,end) by the first iteration (max_it = 0: ap keeps what it held); the
 * boundary planes of sol, res and p that `apply bc` zeroes -- per face the duplicate planes of the field's own layout, tangentially
 * over the ghost range -- `apply bc to Solution` once after the loop, whatever max_it.  Nothing else, and never rhs or the
 * coefficients.
 * `apply bc` zeroes duplicate planes.  A layout without a duplicate plane on a face (a cell layout) has ghost cells next to the box
 * there, which no statement of the solver writes: the mat-vec reads what they hold, as the statements do.  The answer to a call
 * does not depend on which of the library's two kernels runs it (to the bit). */
int examg_cg_coarse(const examg_layout_t *lu, double *sol, const examg_layout_t *lf, const double *rhs,
                    const examg_layout_t *lr, double *res, const examg_layout_t *lp, double *p,
                    const examg_layout_t *lq, double *ap, const examg_stencil_t *st, const examg_geom_t *g,
                    uint32_t face_mask, int max_it, double rel_tol, const int32_t *begin, const int32_t *end,
                    double *info, examg_stream_t stream);
/* The same solver as the reference's layer-3 solver generator writes it (Function VCycle_0@coarsest, Testing/Smoothers/Jac.exa4:75-109,
 * Testing/FMG/3D_Trigonometric.exa4: the programs with slotted fields): the numerator of alpha is the SQUARE OF THE ROUNDED NORM carried
 * from the previous iteration (`alpha = res * res / alphaDenom`) instead of a fresh sum of squares, and the solver contains no
 * `apply bc` statements -- boundary planes are read as they are and never written (Solution@coarsest carries the Dirichlet values of
 * the FMG start there). */
#define EXAMG_CG_ALPHA_FROM_NORM 1u
#define EXAMG_CG_NO_BC 2u
/* `Solution@coarsest = 0` (mgCycle of the next finer level, ...exa4:225-229) rides along: the solver takes the zero field as its start --
 * `sol` is not read (inner points; its boundary planes hold 0 already) and the zeroing loop need not run.  Same expressions on the
 * constant 0.0: bit-identical to examg_set + the solver. */
#define EXAMG_CG_ZERO_START 4u
int examg_cg_coarse_variant(const examg_layout_t *lu, double *sol, const examg_layout_t *lf, const double *rhs,
                            const examg_layout_t *lr, double *res, const examg_layout_t *lp, double *p,
                            const examg_layout_t *lq, double *ap, const examg_stencil_t *st, const examg_geom_t *g,
                            uint32_t face_mask, int max_it, double rel_tol, const int32_t *begin, const int32_t *end,
                            uint32_t flags, double *info, examg_stream_t stream);

/* ---- external fields: get<Name>(dest, slot) / set<Name>(src, slot) of `external Field` declarations
 * (interfacing/ir/IR_CopyToExternalField.scala:31-90, IR_CopyFromExternalField.scala): device-to-device copy between a
 * caller-owned array in its own layout (same duplicate/inner extents, its own ghost/pad widths) and the internal field
 * over [DLB - min(ghosts), DRE + min(ghosts)) per dimension. */
int examg_copy_to_external(const examg_layout_t *l_int, const double *x_int, const examg_layout_t *l_ext, double *dest,
                           examg_stream_t stream);
int examg_copy_from_external(const examg_layout_t *l_ext, const double *src, const examg_layout_t *l_int, double *x_int,
                             examg_stream_t stream);

/* ---- a-13 / e: block-to-block transport over RCCL (one process per GPU) -----------------------------------------------
 * What the generated host calls `exch<Field>_<level>(slot)` (communication/ir/IR_CommunicateFunction.scala:194-219,412-480,
 * naming IR_SetupCommunication.scala:119-147) and the MPI_Allreduce after a reduction loop
 * (parallelization/api/mpi/MPI_Reduction.scala:100-126).  The communicator stands where MPI_COMM_WORLD does; it is created
 * from a 128-byte id that rank 0 obtains and the host distributes by its own means (MPI_Bcast in a generated program, a
 * file, torch.distributed).  All calls are asynchronous on `stream` (ncclSend / ncclRecv groups, pack / unpack kernels).  NOT for
 * stream capture: RCCL point-to-point groups hang inside a hipGraph capture on ROCm 7.2 -- the peer-write transport below is
 * the capturable one.  A communicator of one rank needs no RCCL (id may be NULL). */
typedef struct examg_comm examg_comm_t;
#define EXAMG_COMM_ID_BYTES 128
int examg_comm_unique_id(void *id /* EXAMG_COMM_ID_BYTES */);
int examg_comm_create(examg_comm_t **comm, const void *id, int nranks, int rank);   /* collective; binds the current HIP device */
int examg_comm_destroy(examg_comm_t *comm);
int examg_comm_rank(const examg_comm_t *comm);
int examg_comm_size(const examg_comm_t *comm);

/* Ranks of the axis neighbours of this block, rank[d][0] across the lower and rank[d][1] across the upper face of dimension d;
 * -1 = physical boundary (IR_IV_NeighborIsValid false, domain/ir/IR_ConnectFragments.scala:110-151); the own rank = periodic
 * dimension with one block. */
typedef struct examg_neighbors {
  int32_t rank[3][2];
} examg_neighbors_t;

/* what: EXAMG_EXCH_DUP  duplicate layers, upstream (own upper plane -> '+' neighbour's lower plane), axis by axis;
 *       EXAMG_EXCH_GHOST ghost layers both ways, axis by axis with tangential extent GLB..GRE (corner ghosts become valid);
 *       | EXAMG_EXCH_CONCURRENT_AXES: ghost layers of all axes as ONE send/recv group -- face ghosts only, for loops that read
 *       nothing else (5/7-point stencils).  Which parts a field communicates is the layout declaration's business
 *       (`ghostLayers = [..] with communication`): the caller passes `what` accordingly. */
enum { EXAMG_EXCH_DUP = 1, EXAMG_EXCH_GHOST = 2, EXAMG_EXCH_ALL = 3, EXAMG_EXCH_CONCURRENT_AXES = 4,
       /* examg_jacobi2_blocks / examg_rbgs_sweep_blocks only: tmp's duplicate planes on the physical faces already hold u_in's values
        * (position-only Dirichlet values, written once by the caller): the pass does not refresh them */
       EXAMG_PASS_TMP_PLANES_VALID = 8 };
/* caller-owned device scratch for the packed slabs (the generated program's buffer_Send / buffer_Recv arrays) */
size_t examg_exchange_workspace_bytes(const examg_layout_t *l);
int examg_exchange(examg_comm_t *comm, const examg_layout_t *l, double *x, const examg_neighbors_t *nb, int what,
                   void *workspace, size_t workspace_bytes, examg_stream_t stream);
/* Smoother passes on a block WITH neighbours, halo traffic overlapped with the interior kernel -- the reference's core / boundary
 * split (baseExt/ir/IR_LoopOverPointsInOneFragment.scala:143-222) applied to a pair of dependent sweeps, as one call:
 *   examg_jacobi2_blocks     two Jacobi steps  (`communicate ghost of u; loop; advance` twice, Testing/Smoothers/Jac.exa4:125-131)
 *   examg_rbgs_sweep_blocks  one red-black sweep (`color with { .., communicate u; loop; .. }`, ...exa4:204-213), colour `first` first
 * The loop's box [begin, end) shrunk by one point (first stage) and two (second stage) at interior faces runs as ONE two-stage kernel
 * on `stream`; meanwhile a side stream owned by the communicator exchanges the ghost layers of u_in, evaluates the first stage on
 * the three planes next to every interior face into `tmp`, exchanges tmp's ghost layers and evaluates the second stage on the two
 * planes next to every interior face into u_out; events join the streams.  Two exchanges per pass, as the plain loops have;
 * results bit-identical to them.  u_in, u_out, tmp: three arrays of layout lu (tmp: scratch; its duplicate planes on physical
 * faces are refreshed from u_in).  exchange_flags: EXAMG_EXCH_CONCURRENT_AXES or 0.  overlap = 0, or a stencil / box for which
 * the one-pass kernel is not eligible: the same steps in sequence on `stream`.  The caller swaps u_in / u_out afterwards. */
int examg_jacobi2_blocks(examg_comm_t *comm, const examg_neighbors_t *nb, const examg_layout_t *lu, const double *u_in, double *u_out,
                         double *tmp, const examg_layout_t *lf, const double *rhs, const examg_stencil_t *st, double w,
                         const int32_t *begin, const int32_t *end, int exchange_flags, void *workspace, size_t workspace_bytes,
                         int overlap, examg_stream_t stream);
int examg_rbgs_sweep_blocks(examg_comm_t *comm, const examg_neighbors_t *nb, const examg_layout_t *lu, const double *u_in, double *u_out,
                            double *tmp, const examg_layout_t *lf, const double *rhs, const examg_stencil_t *st, double w, int first,
                            const int32_t *begin, const int32_t *end, int exchange_flags, void *workspace, size_t workspace_bytes,
                            int overlap, examg_stream_t stream);
/* The transfer operators of mgCycle on a block WITH neighbours, one call each (same split, around the `communicate` statements of
 * Benchmark/Poisson3D/3D_FD_Poisson_fromL4.exa4:215-237):
 *   examg_residual_restrict_blocks  `communicate Solution; Residual = RHS - A * Solution; communicate Residual; RHS@coarser = R * Residual`:
 *       the one-pass residual + restriction kernel on the coarse box shrunk by one point at interior faces (reads no ghost value,
 *       stores no residual) on `stream`; on the side stream the ghost exchange of u, the residual on the two fine planes next to
 *       every interior face into `res`, the exchange of `res` and the restriction of the coarse planes on the interior faces.
 *       `res` holds the residual on that two-plane shell only afterwards.  Bit-identical to the four statements.
 *   examg_prolong_add_blocks        `communicate Solution@coarser; Solution += P * Solution@coarser`: the interpolation reads duplicate
 *       and inner coarse points only, so the ghost part of the exchange runs beside the kernel.
 * exchange_flags: EXAMG_EXCH_DUP -- also exchange the duplicate layers (first, in sequence; leave it out when both owners of a
 * shared plane are known to hold the same bits); EXAMG_EXCH_CONCURRENT_AXES -- ghost layers of u in one batch (7-point stencil). */
int examg_residual_restrict_blocks(examg_comm_t *comm, const examg_neighbors_t *nb, const examg_layout_t *lu, double *u,
                                   const examg_layout_t *lf, const double *rhs, const examg_layout_t *lr, double *res,
                                   const examg_stencil_t *st, const examg_layout_t *lc, double *fc, double scale, const int32_t *fbegin,
                                   const int32_t *fend, const int32_t *cbegin, const int32_t *cend, int exchange_flags, void *workspace,
                                   size_t workspace_bytes, int overlap, examg_stream_t stream);
int examg_prolong_add_blocks(examg_comm_t *comm, const examg_neighbors_t *nb, const examg_layout_t *lc, double *uc,
                             const examg_layout_t *lfine, double *uf, const int32_t *begin, const int32_t *end, int exchange_flags,
                             void *workspace, size_t workspace_bytes, int overlap, examg_stream_t stream);
/* MPI_Allreduce(MPI_IN_PLACE, x, n, MPI_DOUBLE, op): x is device memory; op 0 = sum, 1 = max, 2 = min */
int examg_allreduce(examg_comm_t *comm, double *x, int n, int op, examg_stream_t stream);
/* every rank's n doubles, in rank order (coarse-level agglomeration: fewer, larger collectives over xGMI) */
int examg_allgather(examg_comm_t *comm, const double *send, double *recv, int64_t n, examg_stream_t stream);

/* ---- a-13 / e, second transport: peer writes through HIP IPC (SURVEY.md section 5.8 "direct peer writes"; replaces the
 * MPI_Isend / MPI_Irecv branch of communication/ir/IR_CommunicateFunction.scala:412-471, IR_RemoteSend.scala:48-58,
 * IR_RemoteRecv.scala:50-65) -- no communication library: every rank owns a region of uncached device memory that its
 * neighbours map (hipIpcOpenMemHandle: xGMI peer mapping across the GPUs of a node, a plain mapping when ranks share a device);
 * the send kernel packs a field box straight into the neighbour's receive slab and publishes a sequence number, the receive
 * kernel waits for it and unpacks.  Ordering is done by device-side flags whose counters live in device memory, so
 * examg_exchange / examg_allreduce / examg_allgather / examg_*_blocks on such a communicator are stream-ordered, free of host
 * round trips and CAPTURABLE INTO A hipGraph (replayed by all ranks alike).  Set-up, all collective:
 *   examg_comm_create_peer(&c, nranks, rank);
 *   examg_comm_peer_alloc(c, slab_bytes, gather_bytes, handle);    slab_bytes >= the largest halo message (one face slab,
 *                                                                  examg_exchange_workspace_bytes(l) / 4 is always enough),
 *                                                                  gather_bytes >= the largest examg_allgather piece (0: none)
 *   <all-gather the EXAMG_PEER_HANDLE_BYTES of every rank by the host's own means: MPI_Allgather, torch.distributed, files>
 *   examg_comm_peer_connect(c, all_handles);
 * To grow the slabs later: synchronise the device on every rank, host barrier, examg_comm_peer_release on every rank (no region is
 * freed while a neighbour still maps it), host barrier, then alloc / gather / connect again (sequence numbers restart).  The workspace arguments of examg_exchange / examg_*_blocks are ignored (may be NULL).  A wait that sees no
 * progress for EXAMG_PEER_TIMEOUT_MS (default 120000) gives up, makes every later wait return at once and is reported by
 * examg_comm_status() -- a lost neighbour never leaves a kernel spinning. */
#define EXAMG_PEER_HANDLE_BYTES 128
int examg_comm_create_peer(examg_comm_t **comm, int nranks, int rank);
int examg_comm_peer_alloc(examg_comm_t *comm, size_t slab_bytes, size_t gather_bytes, void *handle_out /* EXAMG_PEER_HANDLE_BYTES */);
int examg_comm_peer_connect(examg_comm_t *comm, const void *all_handles /* nranks x EXAMG_PEER_HANDLE_BYTES, rank order */);
/* growing: examg_comm_peer_release on every rank (unmaps the other ranks' regions), host barrier, then alloc / gather / connect */
int examg_comm_peer_release(examg_comm_t *comm);
size_t examg_comm_peer_slab_bytes(const examg_comm_t *comm);
size_t examg_comm_peer_gather_bytes(const examg_comm_t *comm);
/* synchronises `stream`, then 0 if no wait of the peer-write transport has given up (always 0 for RCCL communicators) */
int examg_comm_status(examg_comm_t *comm, examg_stream_t stream);

/* Deterministic synthetic field (SplitMix64 of the linear index, U(-1,1)); same bits as the oracle's. */
int examg_fill_random(double *x, int64_t n, uint64_t seed, examg_stream_t stream);

/* ---- Sum over a box and a scalar added over a box (any localization) ---------------------------------------------------
 * examg_sum: *result = sum of x over [begin,end) -- `s += F` with `reduction (+ : s)`; the fixed reduction tree and the work
 * buffer of examg_dot.  examg_add_scalar: x = x + c over the box -- `F += s`; `F -= s` is c = -s (x + (-s) is bitwise x - s). */
int examg_sum(const examg_layout_t *l, const double *x, const int32_t *begin, const int32_t *end, double *result, void *work,
              examg_stream_t stream);
int examg_add_scalar(const examg_layout_t *l, double *x, double c, const int32_t *begin, const int32_t *end, examg_stream_t stream);

/* ---- Cell-centred fields (`Layout X< Real, Cell >`) ---------------------------------------------------------------------
 * A cell layout has no duplicate layers (dup_l = dup_r = 0): inner = cells of the fragment, iterator index 0 is the first
 * cell, `loop over` covers [0, inner) (baseExt/ir/IR_LoopOverPointsInOneFragment.scala, the IR_AtCellCenter case).  The
 * layout struct is the node one; the localization is the choice of entry point.
 * Positions: cell centre = (i * h + pos_begin) + 0.5 * h (grid/ir/IR_VF_CellCenter.scala:97-100).
 *
 * examg_fill_expr_cell / examg_max_err_expr_cell: examg_fill_expr / examg_max_err_expr with the program evaluated at the
 * cell centres. */
int examg_fill_expr_cell(const examg_layout_t *l, double *x, const examg_geom_t *g, const examg_expr_t *e, const int32_t *begin,
                         const int32_t *end, examg_stream_t stream);
int examg_max_err_expr_cell(const examg_layout_t *l, const double *x, const examg_geom_t *g, const examg_expr_t *e,
                            const int32_t *begin, const int32_t *end, double *result, void *work, examg_stream_t stream);

/* `apply bc` of a cell field (boundary/ir/IR_ApplyBCFunction.scala:53-83): the ghost cell beside every boundary cell of each
 * face in face_mask (bit 2*d + (side > 0)), all faces in ONE launch, order 1:
 *   EXAMG_BC_DIRICHLET: ghost = 2.0 * g(face centre) - interior   (boundary/ir/IR_DirichletBC.scala, generateFieldUpdatesCell)
 *   EXAMG_BC_NEUMANN  : ghost = interior                           (boundary/ir/IR_NeumannBC.scala, generateFieldUpdatesCell)
 *   EXAMG_BC_NEGATE   : ghost = -interior                          (a reflecting wall written as a boundary function:
 *                                                                   `loop over hu only ghost [-1, 0] on boundary { hu = -hu@[1, 0] }`)
 * g is the program `expr` (a constant is a one-instruction program; ignored for Neumann) evaluated at the face centre
 * (boundary/ir/IR_HandleBoundaries.scala:55-70): the cell centre in the tangential dimensions, the node position of the face
 * (index 0 below, index inner above) in the normal one.
 * Edge and corner ghosts are NOT written: tangentially each face covers the inner cells only.  The reference handles the
 * faces one after the other over a range that includes them; a cell stencil with entries off the axes would see the
 * difference, which is why the interpreter refuses those (only axis entries read ghosts, and every axis ghost is written
 * here exactly as the reference writes it).  Needs ghost >= 1 in every dimension of the mask.
 *
 *   EXAMG_BC_VALUE_MINUS: ghost = g(ghost cell) - interior         (a ghost loop with a value:
 *                                                                   `loop over F only ghost [0, 1] on boundary { F = E - F@[0, -1] }`)
 * ONE subtraction: it is neither the Dirichlet kind (no factor 2.0, another evaluation point) nor, with g = 0, EXAMG_BC_NEGATE --
 * 0.0 - (+0.0) is +0.0 where -(+0.0) is -0.0.  g is `expr` evaluated AT THE GHOST CELL ITSELF, the loop index of the reference's ghost
 * loop (index -1 below the first cell, index inner above the last), not at the face centre: EXAMG_OP_X/Y/Z are the centre of the
 * ghost cell, (i * h + pos_begin) + 0.5 * h (`vf_cellCenter_*`), and EXAMG_OP_NODE_X/Y/Z the node of the ghost cell's own index,
 * i * h + pos_begin (`vf_nodePosition_*`: the inner term of the cell-centre formula, the value examg_fill_expr uses for a node).  The
 * node-position opcodes are operands of this kind only: every other kind and every other entry point refuses them ("unknown opcode").
 * Tangential range, unwritten edge and corner ghosts and the ghost >= 1 check as for the other kinds.
 * examg_vec_apply_bc_cell and examg_apply_bc_face refuse this kind.
 *
 * examg_apply_bc_cell_faces: every face of the mask in ONE launch, each with a kind and a program of its own -- faces[2*d + (side > 0)]
 * for every bit of the mask (the other entries are not read; expr is not read for Neumann and NEGATE).  The faces of a cell field never
 * read one another's ghosts, so the result has the bits of one examg_apply_bc_cell call per face, in any order.  The refusals of
 * examg_apply_bc_cell apply per face; the distinct programs of one call may have EXAMG_MAX_EXPR instructions together (faces that
 * name the same examg_expr_t share it). */
/* (3 is no kind: it stays refused as "unknown kind", as every number that is none of these) */
enum { EXAMG_BC_DIRICHLET = 0, EXAMG_BC_NEUMANN = 1, EXAMG_BC_NEGATE = 2, EXAMG_BC_VALUE_MINUS = 4 };
#define EXAMG_OP_NODE_X 26
#define EXAMG_OP_NODE_Y 27
#define EXAMG_OP_NODE_Z 28
typedef struct {
  int32_t kind;              /* EXAMG_BC_* */
  const examg_expr_t *expr;  /* the face's program (Dirichlet, VALUE_MINUS) */
} examg_bc_face_t;
int examg_apply_bc_cell(const examg_layout_t *l, double *x, const examg_geom_t *g, int kind, const examg_expr_t *expr,
                        uint32_t face_mask, examg_stream_t stream);
int examg_apply_bc_cell_faces(const examg_layout_t *l, double *x, const examg_geom_t *g, const examg_bc_face_t *faces, uint32_t face_mask,
                              examg_stream_t stream);

/* RHS@coarser = scale * R * Residual with R the linear cell restriction (operator/l4/L4_DefaultRestriction.scala:37-43,63-90):
 * kron over the dimensions of [2i -> 0.5, 2i+1 -> 0.5], the mean of the 2^d child cells, weight 0.5^d exactly.
 *   fc(I) = sum over the children o in {0, 1}^d, in entry order of the composed stencil (x offset outermost, then y, then z, each
 *           0 before 1), of (scale * 0.5^d) * rf(2I + o)
 * begin/end: coarse iterator box (2-D: [0, 1) in dim 2).  Footprints: the box must lie in the coarse allocation and the fine
 * cells [2 * begin, 2 * end) in the fine allocation -- else an error, and nothing is launched.  It reads exactly the children of
 * the box's cells: no ghost cell unless the box holds coarse ghost cells.  Writes the box of fc and nothing else; rf is not
 * modified; the arrays must not overlap.  Both layouts are cell layouts of one dimensionality (2 or 3): no duplicate layers,
 * and no layout transformation (a colour-split cell layout is an error).  An empty box is a no-op that returns 0.
 * Fine rows whose pairs (2I, 2I+1) are 16-byte aligned (FieldLayout.cell(..., align=2)) are read 16 bytes at a time, others 8:
 * the same bits either way. */
int examg_restrict_cell(const examg_layout_t *lfine, const double *rf, const examg_layout_t *lcoarse, double *fc, double scale,
                        const int32_t *begin, const int32_t *end, examg_stream_t stream);

/* Solution += P@coarser * Solution@coarser with P = 2^d R^T (operator/l4/L4_DefaultProlongation.scala:30-45): every fine cell
 * receives 1.0 * its parent, uf(i) = uf(i) + uc(floor(i / 2)) -- piecewise-constant injection; floor also for the negative
 * indices of ghost cells (cell -1 has the parent -1).  begin/end: fine iterator box (2-D: [0, 1) in dim 2).  Footprints: the
 * box must lie in the fine allocation and the parents [floor(begin / 2), floor((end - 1) / 2)] in the coarse allocation -- else
 * an error, and nothing is launched.  Writes the box of uf and nothing else; uc is not modified; the arrays must not overlap.
 * Layouts as for examg_restrict_cell.  An empty box is a no-op that returns 0. */
int examg_prolong_add_cell(const examg_layout_t *lcoarse, const double *uc, const examg_layout_t *lfine, double *uf,
                           const int32_t *begin, const int32_t *end, examg_stream_t stream);

/* ---- Coupled systems of cell-centred unknowns ---------------------------------------------------------------------------
 * n = 2 or 3 scalar cell fields u_0 .. u_{n-1} coupled at every cell by the operator  A = L * I + G(x):  one constant stencil L
 * on every component and a point-wise n x n matrix G of coefficient fields (Benchmark/OptFlow2D/2D_FD_OptFlow.exa4: Horn-Schunck
 * optical flow, `uuSten * u + uvSten * v + alpha * alpha * Laplace * u` with `Stencil uuSten { [0, 0] => IxIx }`; n need not be
 * the dimensionality).  examg_sys_t names the arrays:
 *   u[c]        the unknowns, all in layout lu (a cell layout with ghost >= 1 in every dimension)
 *   f[c]        the right-hand sides, all in layout lf
 *   g[c * n + d] the coefficient field that multiplies u_d in row c, all in layout lg, read at the cell only; NULL: no such
 *               term; entries may name one array several times (uvSten and vuSten both hold IxIy): it is loaded once
 *   dst[c]      the destinations of examg_sys_op, all in layout ld; no dst may be one of the unknowns
 * Entries of the arrays behind n are ignored.  All four layouts are plain cell layouts (no duplicate layers, no layout
 * transformation) of one dimensionality (2 or 3) with the same inner sizes; ghost and pad widths may differ.
 * L: a constant stencil (cfield NULL) whose entries are the centre (required) and axis neighbours at distance 1, each at most
 * once, in any order; the order is significant.  SCALAR FACTORS ON L are the host's business: `(alpha * alpha) * Laplace` is
 * stencil arithmetic, the generator folds the factor into the coefficients before it prints the convolution, and so does the
 * caller here.  (`(alpha ** 2) * (Laplace * u)` multiplies the finished convolution instead; folded into the coefficients it
 * differs from the generated code in the last bit unless the factor is a power of two.  It is 1 in every reference program.)
 *
 * Arithmetic, fp64, no contraction.  conv(L, u_c) = the entries of L folded left to right in declared order: c_0 * u_c(i + o_0),
 * then + c_k * u_c(i + o_k) (stencil/ir/IR_StencilConvolution.scala:65-68).
 *   row value    Au_c = (((g[c][0] * u_0) + (g[c][1] * u_1)) [+ (g[c][2] * u_2)]) + conv(L, u_c); NULL terms are skipped, not
 *                multiplied by zero (a row without coefficient fields is conv(L, u_c) alone)
 *
 * examg_sys_op: for every row c of row_mask (bit c) and every cell of [begin,end)
 *   EXAMG_SYS_APPLY:    dst_c = Au_c                          (`cgTmp1_u = uuSten * cgTmp0_u + uvSten * cgTmp0_v + .. Laplace * cgTmp0_u`)
 *   EXAMG_SYS_RESIDUAL: dst_c = f_c - Au_c                    (`residual_u = rhs_u - ( uuSten * u + uvSten * v + .. )`)
 * Rows outside the mask are neither evaluated nor written (the scalar-component programs evaluate one row per loop).  Reads
 * the unknowns on the box and its one-cell axis shell (ghost cells at the block's faces), coefficients and right-hand sides on
 * the box; writes the box of dst_c and nothing else.
 *
 * examg_sys_relax: one colour of the red-black smoother with the local solve of every cell, in place -- the cells of [begin,end)
 * with (i0 + i1 + i2) % 2 == colour (the parity of the iterator coordinates, as examg_stencil_op's colour):
 *     `repeat with { (0 == ((i0 + i1) % 2)), (1 == ((i0 + i1) % 2)), .. loop over u { solve locally relax w { u => .. == rhs_u   v => .. == rhs_v } } .. }`
 * (baseExt/l4/L4_RepeatLoops.scala; solver/l4/L4_LocalSolve.scala, solver/ir/IR_LocalSolve.scala: the unknowns at the loop's cell
 * form AVals, every other term goes to fVals).  Per cell
 *   b_c  = f_c - (the entries of L off the centre folded left to right in declared order over u_c)      [f_c when there are none]
 *   a_cd = g[c][d], 0.0 for NULL;  a_cc = g[c][c] + L_centre, L_centre alone for NULL
 *   x solves a x = b:
 *     n = 2:  det = a00 * a11 - a01 * a10;   x0 = (b0 * a11 - a01 * b1) / det;   x1 = (a00 * b1 - a10 * b0) / det
 *     n = 3:  the cofactors, each a difference of two products,
 *               k00 = a11 * a22 - a12 * a21;  k01 = a12 * a20 - a10 * a22;  k02 = a10 * a21 - a11 * a20
 *               k10 = a02 * a21 - a01 * a22;  k11 = a00 * a22 - a02 * a20;  k12 = a01 * a20 - a00 * a21
 *               k20 = a01 * a12 - a02 * a11;  k21 = a02 * a10 - a00 * a12;  k22 = a00 * a11 - a01 * a10
 *             det = (a00 * k00 + a01 * k01) + a02 * k02
 *             x_i = ((k0i * b0 + k1i * b1) + k2i * b2) / det
 *   u_c = u_c + relax * (x_c - u_c);  relax == 1.0: u_c = x_c, no arithmetic
 * The generator emits an inverse times a vector; these are not its bits (its results files carry four digits).  Reads the
 * neighbours of the other colour and the cell's own values only; writes the colour's cells of the box in u_c and nothing else.
 *
 * Both refuse, before anything is launched: n outside 2 .. 3, a layout with duplicate layers (not a cell layout) or under a layout
 * transformation, layouts of different inner sizes or dimensionality, unknowns without a ghost layer, a stencil field as L, an
 * entry of L off the axes, further than one cell or repeated, L without a centre entry, a box that leaves an allocation.  An empty
 * box is a no-op that returns 0.  Rows whose pairs of cells (even array index first) are 16-byte aligned in every argument
 * (FieldLayout.cell(..., align=2)) are read and written 16 bytes at a time, others 8: the same bits either way. */
#define EXAMG_SYS_MAX 3
enum { EXAMG_SYS_APPLY = 0, EXAMG_SYS_RESIDUAL = 1 };
typedef struct examg_sys {
  int32_t n;
  examg_layout_t lu, lf, lg, ld;
  double *u[EXAMG_SYS_MAX];
  const double *f[EXAMG_SYS_MAX];
  const double *g[EXAMG_SYS_MAX * EXAMG_SYS_MAX];
  double *dst[EXAMG_SYS_MAX];
} examg_sys_t;
int examg_sys_op(int mode, const examg_sys_t *sys, const examg_stencil_t *L, uint32_t row_mask, const int32_t *begin, const int32_t *end,
                 examg_stream_t stream);
int examg_sys_relax(const examg_sys_t *sys, const examg_stencil_t *L, double relax, int colour, const int32_t *begin, const int32_t *end,
                    examg_stream_t stream);

/* dst = (s * x) * y over the box, s = +-1.0 exact: the set-up loops `IxIy = Ix * Iy` (s = 1.0) and `rhs_u = -Ix * It` (s = -1.0: the
 * negation, then the product).  Any localization; every argument through its own layout; plain layouts only; dst may be x or y.
 * (`It = img1 - img0` needs no entry of its own: examg_axpby with a = 1, b = -1 on a copy of img0 gives x + (-1.0 * y), bitwise x - y.) */
int examg_pointwise_mul(const examg_layout_t *lx, const double *x, const examg_layout_t *ly, const double *y, const examg_layout_t *ld,
                        double *dst, double s, const int32_t *begin, const int32_t *end, examg_stream_t stream);

/* ---- Vector-valued cell fields and matrix stencils ---------------------------------------------------------------------------
 * `Layout X< Vec2, Cell >`, `Field flow< global, X, Neumann >`, `Stencil S { [0, 0] => { { IxIx, IxIy }, { IxIy, IyIy } }, .. }`
 * (Testing/Application/OpticalFlow2D.exa4).  A vector field of n = 2 or 3 components in layout l is n scalar arrays one behind the other,
 * the component slowest (field/l4/L4_FieldLayout.scala:63-73): component c lives at  base + c * size(l),  size(l) the doubles of
 * one array of the layout (examg_layout_size).  A vector argument is (layout, base pointer); n is a call argument.  The layout
 * struct is the scalar one.
 *
 * examg_vec_stencil_t, a MATRIX STENCIL M: 1 .. 7 entries, the centre (required) and axis neighbours at distance 1, each at most once, in
 * any order; the order is significant.  Entry k is an n x n matrix, element (c, d) at index c * n + d:
 *   kmask bit c*n+d   the element has the constant k[c*n+d]
 *   g[c*n+d]          the element has a cell coefficient field (a scalar array in layout lg, read at the cell); NULL: none
 *                     (lg is looked at only when some element has a field: a stencil of constants may leave it zeroed)
 *   both: the element is  k_cd + g_cd(i),  evaluated at every cell; neither: the element is ABSENT
 * An off-centre entry is a diagonal matrix of constants (its diagonal elements may differ per component, and may be absent); a
 * coefficient field or an element off the diagonal there is an error.  Coefficient pointers that alias are loaded once.
 *
 * Arithmetic, fp64, no contraction.  With m_cd the element of entry k and o_k its offset:
 *   t_k,c = the present elements of row c of entry k folded left to right in d over  m_cd * u_d(i + o_k)
 *   Mu_c  = the t_k,c folded left to right in entry order
 * Absent elements, and entries without a present element in row c, are skipped, not multiplied by zero; a row without any element
 * gives Mu_c = 0.0.
 *
 * examg_vec_op, every row c and every cell of [begin,end) in one launch:
 *   EXAMG_SYS_APPLY:    dst_c = Mu_c                  (`dst = S * u`)
 *   EXAMG_SYS_RESIDUAL: dst_c = f_c - Mu_c            (`dst = f - S * u`)
 * u, f and dst are vector fields in lu, lf and ld.  Reads u on the box and its one-cell axis shell, f and the coefficients on the box;
 * writes the box of dst and nothing else.  dst may overlap neither u nor, in EXAMG_SYS_RESIDUAL, f.
 *
 * examg_vec_smooth: one colour (i0 + i1 + i2) % 2 == colour of
 *     `u = u + relax * ( inverse ( diag ( S ) ) * ( f - S * u ) )`
 * in place, inside `repeat with { colour conditions .. }` / `color with`:
 *   r    = f - Mu exactly as EXAMG_SYS_RESIDUAL computes it (the centre entry included)
 *   D    = the centre matrix, absent elements read as 0.0
 *   x    solves D x = r with the n = 2 and n = 3 formulas of examg_sys_relax above
 *   u_c  = u_c + x_c when relax == 1.0, else u_c + relax * x_c
 * Reads only cells of the other colour and the cell's own values; writes the colour's cells of the box and nothing else.  As for
 * examg_sys_relax, these are not the generator's bits (it emits an inverse times a vector; its results files carry four digits).
 *
 * examg_vec_dot: *result = sum over the box of the per-cell term ((x_0 * y_0) + (x_1 * y_1)) [+ (x_2 * y_2)] -- `v += dot ( x, y )`
 * with `reduction ( + : v )` -- through the kernels, the fixed tree and the work buffer of examg_dot (the same launch plan as
 * examg_dot on that box).
 *
 * examg_vec_set, examg_vec_axpby, examg_vec_restrict_cell, examg_vec_prolong_add_cell, examg_vec_apply_bc_cell: the scalar entry
 * point's kernel over all n components in ONE launch; on every component the bits the scalar entry point writes when called on that
 * component (same arguments otherwise, same checks).  examg_vec_apply_bc_cell knows EXAMG_BC_NEUMANN only.
 *
 * Refused before anything is launched: n outside 2 .. 3; a layout with duplicate layers or under a layout transformation; layouts of
 * different inner sizes or dimensionality; unknowns without a ghost layer; an entry off the axes, of reach 2 or repeated; a stencil
 * without a centre entry; an off-centre entry with an element off the diagonal or with a coefficient field; a box that leaves an
 * allocation; a dst that overlaps an input; a BC kind other than Neumann.  An empty box is a no-op that returns 0 (examg_vec_dot:
 * *result = 0).  Rows whose pairs of cells are 16-byte aligned in every argument and component are accessed 16 bytes at a time,
 * others 8: the same bits either way. */
#define EXAMG_VEC_MAX 3
typedef struct examg_vec_entry {
  int32_t off[3];
  uint32_t kmask;
  double k[EXAMG_VEC_MAX * EXAMG_VEC_MAX];
  const double *g[EXAMG_VEC_MAX * EXAMG_VEC_MAX];
} examg_vec_entry_t;
typedef struct examg_vec_stencil {
  int32_t nent;
  examg_layout_t lg;
  examg_vec_entry_t ent[7];
} examg_vec_stencil_t;
int examg_vec_op(int mode, int n, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *f, const examg_layout_t *ld,
                 double *dst, const examg_vec_stencil_t *M, const int32_t *begin, const int32_t *end, examg_stream_t stream);
int examg_vec_smooth(int n, const examg_layout_t *lu, double *u, const examg_layout_t *lf, const double *f, const examg_vec_stencil_t *M, double relax,
                     int colour, const int32_t *begin, const int32_t *end, examg_stream_t stream);
int examg_vec_dot(int n, const examg_layout_t *lx, const double *x, const examg_layout_t *ly, const double *y, const int32_t *begin,
                  const int32_t *end, double *result, void *work, examg_stream_t stream);
int examg_vec_set(int n, const examg_layout_t *l, double *x, double v, const int32_t *begin, const int32_t *end, examg_stream_t stream);
int examg_vec_axpby(int n, const examg_layout_t *lx, const double *x, const examg_layout_t *ly, double *y, double a, double b,
                    const int32_t *begin, const int32_t *end, examg_stream_t stream);
int examg_vec_restrict_cell(int n, const examg_layout_t *lfine, const double *rf, const examg_layout_t *lcoarse, double *fc, double scale,
                            const int32_t *begin, const int32_t *end, examg_stream_t stream);
int examg_vec_prolong_add_cell(int n, const examg_layout_t *lcoarse, const double *uc, const examg_layout_t *lfine, double *uf,
                               const int32_t *begin, const int32_t *end, examg_stream_t stream);
int examg_vec_apply_bc_cell(int n, const examg_layout_t *l, double *x, const examg_geom_t *g, int kind, uint32_t face_mask,
                            examg_stream_t stream);

/* ---- Coupled systems of node-centred unknowns whose blocks are stencils ------------------------------------------------------
 * n = 2 or 3 scalar node fields u_0 .. u_{n-1} and an n x n table of constant stencils: row c of the operator is
 *     Au_c = sum over d of A_cd * u_d
 * (Examples/LinearElasticity/2D_FD_LinearElasticity_fromL2.exa2: `( lambda + mu ) * ( dxx * u + dxy * v ) + lambda * Laplace * u`,
 * the displacement form of linear elasticity: the off-diagonal block dxy has four diagonal neighbours and no centre).
 * examg_bsys_t names the arrays:
 *   u[c]          the unknowns, all in layout lu
 *   f[c]          the right-hand sides, all in layout lf
 *   dst[c]        the destinations of examg_bsys_op, all in layout ld; no dst may be one of the unknowns, nor -- in EXAMG_SYS_RESIDUAL -- one
 *                 of the right-hand sides (the rows are stored one after the other)
 *   A[c * n + d]  the stencil that acts on u_d in row c; NULL: no such block.  A constant stencil (cfield NULL) with 1 .. 27 entries,
 *                 offsets in {-1, 0, 1}^nd, in any order, each offset at most once; a block need not have a centre entry.  The order
 *                 of the entries is significant; `diag` is not looked at.
 * Entries of the arrays behind n are ignored.  The three layouts are plain layouts (no layout transformation) of node fields (not
 * cell layouts: inner + duplicate points per axis count) of one dimensionality (2 or 3) with the same inner sizes and duplicate
 * layers; ghost and pad widths may differ.
 * STENCIL ARITHMETIC is the host's business, as for examg_sys_op: a scalar factor in front of a stencil, evaluated left to right as
 * written, multiplies every coefficient; two stencils on one unknown (`( lambda + mu ) * dxx` and `lambda * Laplace` on u) are added
 * into one block in order of appearance -- an offset already present gets c_old + c_new, a new offset is appended.
 *
 * Arithmetic, fp64, no contraction.  conv(S, x) = the entries of S folded left to right in declared order: c_0 * x(i + o_0), then
 * + c_k * x(i + o_k) (stencil/ir/IR_StencilConvolution.scala:65-68).
 *   row value    Au_c = (conv(A_c0, u_0) + conv(A_c1, u_1)) [+ conv(A_c2, u_2)]: the blocks left to right in d; NULL blocks are
 *                skipped, not multiplied by zero.  A row of the call without any block is an error.
 *
 * examg_bsys_op: for every row c of row_mask (bit c) and every point of [begin,end)
 *   EXAMG_SYS_APPLY:    dst_c = Au_c
 *   EXAMG_SYS_RESIDUAL: dst_c = f_c - Au_c
 * Rows outside the mask are neither evaluated nor written.  Reads the unknowns on the box and its one-point shell, diagonal
 * neighbours included, right-hand sides on the box; writes the box of dst_c and nothing else.
 *
 * examg_bsys_relax: one colour of the collective point smoother, in place --
 *     `color with { .., loop over u { solve locally relax w { u => rowU == rhs_u   v => rowV == rhs_v } } }`
 * (solver/l4/L4_LocalSolve.scala, solver/ir/IR_LocalSolve.scala: the unknowns at the loop's point form AVals, every other term goes
 * to fVals).  For every point of [begin,end) that belongs to the colour `col` (examg_colouring_t above: every e_k == rem[k])
 *   a_cd = the centre coefficient of A_cd, 0.0 for a NULL block or a block without a centre entry
 *   b_c  = f_c - (off-centre part of row c);  the off-centre part: the entries of A_cd off the centre folded left to right in declared
 *          order over u_d, for each d in order, the per-block sums added left to right; blocks without an off-centre entry are skipped;
 *          b_c = f_c when no block of the row has one
 *   x solves a x = b with the n = 2 and n = 3 formulas of examg_sys_relax above (det; the cofactors each a difference of two products)
 *   u_c = u_c + relax * (x_c - u_c);  relax == 1.0: u_c = x_c, no arithmetic
 * Reads the neighbours and the point's own values; writes the colour's points of the box in the u_c and nothing else.  The loop is
 * independent of its order only when no neighbour that a point reads belongs to its own colour: the colouring must DECOUPLE (see
 * examg_colouring_t) the union of the off-centre offsets of all blocks.  The parity of all indices does not decouple dxy, whose four
 * diagonal neighbours have the point's own colour; `i0 % 2, i1 % 2 [, i2 % 2]` decouples every block of reach 1.
 *
 * Both refuse, before anything is launched: n outside 2 .. 3; a cell layout, a layout under a layout transformation or one that is
 * not 2-D or 3-D; layouts of different inner sizes or dimensionality; a stencil field as a block; an entry that reaches further than
 * one point (or off the layout's axes); a repeated offset; a row (of the mask) without blocks; a dst that is one of the unknowns or of the right-hand sides read; a
 * box whose one-point shell leaves the allocation of the unknowns, or that leaves the allocation of f or dst.  examg_bsys_relax also
 * refuses a zero a_cc in the input (det is not checked), a colouring that does not decouple the blocks, and what the coloured entry
 * points refuse of a colouring (nexpr, mod, rem, axes, a colour expression that can be negative in the box).  An empty box is a no-op
 * that returns 0.
 *
 * One kernel per entry point, a lane owns four points (of the colour) in consecutive rows: every row of the call is evaluated in one
 * pass, the neighbourhood of an unknown that several rows read comes from memory once and from the vector L1 afterwards (24 * n
 * compulsory bytes per point for a full residual).  The stencils travel as kernel arguments: no allocation, no scratch, no host
 * synchronisation; capturable.  A plane of the unknowns' layout has fewer than 2^31 points (32-bit neighbour offsets; refused otherwise).
 * examg_bsys_route: what examg_bsys_op does with these arguments: -1 refused (the reason in examg_last_error), 0 empty box,
 * EXAMG_BSYS_GATHER -- the one route: a marching kernel was measured against it and lost at every size. */
#define EXAMG_BSYS_MAX 3
enum { EXAMG_BSYS_GATHER = 1 };
typedef struct examg_bsys {
  int32_t n;
  examg_layout_t lu, lf, ld;
  double *u[EXAMG_BSYS_MAX];
  const double *f[EXAMG_BSYS_MAX];
  double *dst[EXAMG_BSYS_MAX];
  const examg_stencil_t *A[EXAMG_BSYS_MAX * EXAMG_BSYS_MAX];
} examg_bsys_t;
int examg_bsys_op(int mode, const examg_bsys_t *sys, uint32_t row_mask, const int32_t *begin, const int32_t *end, examg_stream_t stream);
int examg_bsys_relax(const examg_bsys_t *sys, double relax, const examg_colouring_t *col, const int32_t *begin, const int32_t *end,
                     examg_stream_t stream);
int examg_bsys_route(int mode, const examg_bsys_t *sys, uint32_t row_mask, const int32_t *begin, const int32_t *end);

/* ---- Staggered grids: velocities on the faces, the pressure in the cells (Examples/Stokes/2D_FV_Stokes_fromL4.exa4) ---------------
 * `Layout X< Real, Face_x >` (fieldlike/l4/L4_FieldLikeLayoutDecl.scala:53-57): a FACE LAYOUT of axis a is the layout struct with dup = 1
 * and inner = cells - 1 on axis a (like a node field) and dup = 0, inner = cells on every other axis (like a cell field).  Iterator
 * coordinate 0 on the own axis is the lower boundary face, `loop over` covers [0, cells + 1) there and [0, cells) on the other axes; face i
 * is the lower face of cell i.  Position of a face: the node position i * h + pos_begin on the own axis, the cell centre
 * (i * h + pos_begin) + 0.5 * h on the others.  As for cell layouts the localization is the choice of entry point; the face entry points
 * take the axis and refuse a layout whose dup pattern is not that of the axis, and every layout under a layout transformation.
 *
 * examg_mac_t names the arrays and the operator of the saddle-point system of nd = 2 or 3 velocity components u_d and the pressure p:
 *   u[d], lu[d]     the unknown on the faces of axis d, a face layout of axis d with ghost >= 1 on every axis
 *   p, lp           the pressure, a cell layout with ghost >= 1 on every axis
 *   f[d], lf[d], fp, lfp        the right-hand sides;   dst[d], ld[d], dstp, ldp    the destinations of examg_mac_op
 *   A[d]            a constant stencil on u_d: the centre (required) and axis neighbours at distance 1, each at most once, in any order;
 *                   the order is significant
 *   bc[d], bm[d]    the gradient at face i of axis d:  (bc_d * p(i)) + (bm_d * p(i - e_d))         (`B1` of the reference programs)
 *   cc[d], cp[d]    the divergence at cell i adds      (cc_d * u_d(i)), then (cp_d * u_d(i + e_d))   (`C1`)
 * Every array in its own layout; all layouts of one dimensionality and of the same number of cells per axis.  Scalar factors (1/h^2, the
 * widths of a uniform finite-volume grid) are the caller's to fold into the coefficients, as for examg_sys_t.  Entries behind nd are ignored.
 *
 * Arithmetic, fp64, no contraction.  conv(A_d, u_d)(i) = the entries folded left to right in declared order: c_0 * u_d(i + o_0), then
 * + c_k * u_d(i + o_k).
 *
 * examg_mac_op: for every row r of row_mask (bit r; rows 0 .. nd - 1 the momentum rows, row nd the continuity row) and every point of the
 * row's box -- begin / end hold one box per row, begin[3 * r .. 3 * r + 2], in the iterator coordinates of the row's field -- in ONE launch:
 *   row d < nd:   Au_d = conv(A_d, u_d)(i) + ((bc_d * p(i)) + (bm_d * p(i - e_d)))
 *   row nd:       Au_p = the terms (cc_0 * u_0(i)), (cp_0 * u_0(i + e_0)), (cc_1 * u_1(i)), (cp_1 * u_1(i + e_1)), .. added one after the other
 *   EXAMG_SYS_APPLY: dst_r = Au_r;   EXAMG_SYS_RESIDUAL: dst_r = f_r - Au_r
 * Rows outside the mask are neither evaluated nor written, and their f, dst and boxes are not looked at.  Writes the boxes of the dst
 * of the mask and nothing else.  No dst may be an unknown, a right-hand side of the mask or another dst of the mask.
 *
 * examg_mac_relax: one colour of the box smoother, in place:
 *     `color with { i0 % 3, i1 % 3, loop over p { solve locally relax w { u@[0,0] => .. u@[1,0] => .. v@[0,0] => .. v@[0,1] => .. p => .. } } }`
 * (2D_FV_Stokes_fromL4.exa4:588-601; solver/ir/IR_LocalSolve.scala, IR_LocalDirectInvert.scala:78-139: the accesses to the box's own
 * unknowns form the matrix, everything else goes to the right-hand side).  [begin,end) is a box of CELLS inside the block, [0, cells).
 * The unknowns of cell i are, per axis d, l_d = u_d(i) and h_d = u_d(i + e_d), and p(i).  A face on the domain boundary -- index 0 or
 * cells on its own axis -- is no valid computation point (boundary/ir/IR_IsOnBoundary.scala:54-97): it is HELD, its row is the identity
 * with its old value, its column stays, and it is not written back.  With a the centre of A_d, q its +e_d entry, m its -e_d entry
 * (0.0 where A_d has none), per axis d:
 *   tl = (the entries of A_d other than the centre and +e_d, folded in declared order over u_d about face i) + (bm_d * p(i - e_d))
 *   th = (the entries of A_d other than the centre and -e_d, folded in declared order over u_d about face i + e_d) + (bc_d * p(i + e_d))
 *        (no such entry: the pressure term alone)
 *   r0 = f_d(i) - tl,        a00 = a, a01 = q, c0 = bc_d;      l_d held: r0 = l_d, a00 = 1.0, a01 = 0.0, c0 = 0.0
 *   r1 = f_d(i + e_d) - th,  a11 = a, a10 = m, c1 = bm_d;      h_d held: r1 = h_d, a11 = 1.0, a10 = 0.0, c1 = 0.0
 *   det = a00 * a11 - a01 * a10                                 (Cramer on the 2 x 2 block, as examg_sys_relax n = 2)
 *   y0 = (r0 * a11 - a01 * r1) / det;   y1 = (a00 * r1 - a10 * r0) / det           (the block's inverse on its right-hand side)
 *   z0 = (c0 * a11 - a01 * c1) / det;   z1 = (a00 * c1 - a10 * c0) / det           (.. on its border column)
 * then, the terms added one after the other over d = 0 .. nd - 1,
 *   sy = (cc_0 * y0_0) + (cp_0 * y1_0) + (cc_1 * y0_1) + ..;    sz = (cc_0 * z0_0) + (cp_0 * z1_0) + (cc_1 * z0_1) + ..
 *   p_new = (sy - f_p(i)) / sz                                  (the Schur complement of the pressure is -sz)
 *   l_new = y0_d - z0_d * p_new;   h_new = y1_d - z1_d * p_new  (back-substitution)
 *   x = x_old + relax * (x_new - x_old) for the 2 * nd + 1 unknowns, held faces left out;  relax == 1.0: x = x_new, no arithmetic
 * As with examg_sys_relax these are not the generator's bits (it emits an inverse times a vector).
 * Colourings: two cells conflict when the box of one reads or writes an unknown of the other's; for full stars that is every offset of
 * 1-norm 1 or 2 (and (2, +-1), (+-2, +-2) on two axes, which the accepted form separates too).  Accepted: one expression per axis,
 * (s_d + i_d) % m_d with every m_d >= 3, the expressions in any order -- `i0 % 3, i1 % 3 [, i2 % 3]`.  Everything else is refused before
 * anything is launched, with the conflict named: the parity of all indices, (i0 + i1 [+ i2]) % 2, which the finite-difference programs
 * of the reference use (2D_FD_Stokes_fromL4.exa4), gives cells i and i + (-1, 1) one colour, the first reads u_0(i + e_1) and the second
 * writes it (so do i and i + (-1, -1), the nearest conflict and the one the message names) -- that generated loop depends on its execution order.  The kernel enumerates the colour's cells densely, consecutive lanes
 * consecutive cells of the colour in x.
 *
 * examg_mac_sweep: all m_0 * m_1 * .. colours in the reference's order (L4_ColorLoops.toRepeatLoops: the first expression fastest),
 * col->rem ignored; it issues the examg_mac_relax launches one after the other and is bit-identical to those calls.
 *
 * All three refuse, before anything is launched: nd outside 2 .. 3; a layout whose dup pattern is not that of its localization, of
 * another dimensionality, under a layout transformation or of other cell counts than the pressure's; unknowns without a ghost layer on
 * some axis; A_d a stencil field, with an entry off the axes, of reach 2, repeated, or without the centre; a box (with the reach of the
 * row's reads) that leaves an allocation; a destination that is an input.  The smoother also refuses a zero determinant of a 2 x 2 block
 * and a zero sz for any pattern of held faces the block has (all faces of a cell held: fewer than 2 cells on every axis), and a box that
 * leaves the cells of the block.  An empty box is a no-op that returns 0.  No allocation, no host synchronisation; capturable. */
typedef struct examg_mac {
  int32_t nd;
  examg_layout_t lu[3], lp, lf[3], lfp, ld[3], ldp;
  double *u[3], *p;
  const double *f[3], *fp;
  double *dst[3], *dstp;
  const examg_stencil_t *A[3];
  double bc[3], bm[3], cc[3], cp[3];
} examg_mac_t;
int examg_mac_op(int mode, const examg_mac_t *sys, uint32_t row_mask, const int32_t *begin, const int32_t *end, examg_stream_t stream);
int examg_mac_relax(const examg_mac_t *sys, double relax, const examg_colouring_t *col, const int32_t *begin, const int32_t *end,
                    examg_stream_t stream);
int examg_mac_sweep(const examg_mac_t *sys, double relax, const examg_colouring_t *col, const int32_t *begin, const int32_t *end,
                    examg_stream_t stream);

/* Transfers of a face field of `axis` (operator/l4/L4_DefaultRestriction.scala:63-82): the Kronecker product of the node-linear operator
 * on the own axis and the cell-linear one on the others.
 * examg_restrict_face: for every coarse face I of [begin,end)
 *   fc(I) = sum of (scale * W) * rf(fine), W = the product of the per-axis weights (powers of two: exact in any order),
 *           own axis: the fine faces 2I - 1, 2I, 2I + 1 with 1/4, 1/2, 1/4;   other axes: the children 2I, 2I + 1 with 1/2 each;
 *           the terms added in the entry order of the composed stencil: the x offset outermost, then y, then z, each ascending.
 * Footprint: the fine faces [2 * begin - 1, 2 * (end - 1) + 1] on the own axis and [2 * begin, 2 * end) on the others must lie in the
 * fine allocation (restricting over interior faces only, [1, cells), reads no ghost).
 * examg_prolong_add_face: 2^d R^T -- linear on the own axis, the parent's value on the others.  For every fine face i of [begin,end)
 *   own index even:  uf(i) = uf(i) + uc(c),  c = i / 2 on the own axis
 *   own index odd:   uf(i) = uf(i) + ((0.5 * uc(c with (i + 1) / 2)) + (0.5 * uc(c with (i - 1) / 2)))
 *   on the other axes c = floor(i / 2), also for the negative indices of ghost cells.
 * Footprint: the coarse points named must lie in the coarse allocation; the own-axis indices of the box must not be negative.
 * Both: 2-D or 3-D face layouts of `axis`, both of one dimensionality; a box that leaves an allocation and two arguments that are one
 * array are errors, and nothing is launched.  Only the box of the destination is written.  An empty box is a no-op that returns 0. */
int examg_restrict_face(int axis, const examg_layout_t *lfine, const double *rf, const examg_layout_t *lcoarse, double *fc, double scale,
                        const int32_t *begin, const int32_t *end, examg_stream_t stream);
int examg_prolong_add_face(int axis, const examg_layout_t *lcoarse, const double *uc, const examg_layout_t *lfine, double *uf,
                           const int32_t *begin, const int32_t *end, examg_stream_t stream);

/* `apply bc` of a face field of `axis` (boundary/ir/IR_BoundaryCondition.scala:38-45, IR_ApplyBCFunction.scala:53-83), every wall of
 * face_mask (bit 2*d + (side > 0)) in ONE launch:
 *   walls normal to `axis`, the NODE rule: the boundary face (own index 0 / cells) = g(position of the face); EXAMG_BC_DIRICHLET only
 *   the other walls, the CELL rule of examg_apply_bc_cell: the ghost beside every face of the boundary row,
 *     EXAMG_BC_DIRICHLET: ghost = (2.0 * g(wall point)) - interior;    EXAMG_BC_NEUMANN: ghost = interior
 * g is the program `expr` evaluated as boundary/ir/IR_HandleBoundaries.scala:53-70 says: on the own axis the node position, on the
 * wall's normal the wall's coordinate (index 0 below, cells above), elsewhere the cell centre.
 * Ranges: tangentially the cells [0, cells) and, on the own axis, the faces [0, cells + 1); edge and corner ghosts are not written (as
 * for examg_apply_bc_cell).  The node rule comes first, as in the reference's order of the walls for the x faces: where the cell rule
 * reads a boundary face of a normal wall of the mask, `interior` is the value the node rule gives it, g(position of the face).
 * Refused: EXAMG_BC_NEUMANN with a wall normal to `axis` in the mask, EXAMG_BC_NEGATE, a cell-rule wall without a ghost layer, a layout
 * that is no face layout of `axis`. */
int examg_apply_bc_face(int axis, const examg_layout_t *l, double *x, const examg_geom_t *g, int kind, const examg_expr_t *expr,
                        uint32_t face_mask, examg_stream_t stream);

/* examg_fill_expr / examg_max_err_expr with the program evaluated at the positions of the faces of `axis`: the same kernels,
 * instantiated for the third localization. */
int examg_fill_expr_face(int axis, const examg_layout_t *l, double *x, const examg_geom_t *g, const examg_expr_t *e, const int32_t *begin,
                         const int32_t *end, examg_stream_t stream);
int examg_max_err_expr_face(int axis, const examg_layout_t *l, const double *x, const examg_geom_t *g, const examg_expr_t *e,
                            const int32_t *begin, const int32_t *end, double *result, void *work, examg_stream_t stream);

/* ---- Semilinear operators: N(q; u) = A * u + c(q) . u ---------------------------------------------------------------------
 * A a constant stencil (cfield NULL; any entry list, 2-D or 3-D), c a point expression over the value of a node field q AT THE POINT:
 * `Stencil gamSten { [0, 0] => gam * exp ( Solution<active>@current ) }`, `Laplace * Solution + gamSten * Solution`
 * (Testing/NonLinear/FAS_2D_Basic.exa4:26-28, 82, 91, 128: -Laplace u + gam u e^u = f with a full-approximation-scheme V-cycle).  q and u
 * are separate arguments: `gamSten@coarser * Approximation@coarser` reads Solution inside the stencil and multiplies Approximation.
 * The expression travels as a postfix program like every analytic expression of the library, in a compact type: the kernels take
 * the stencil and up to two programs by value as kernel arguments, and examg_expr_t (3 KB) would not fit beside them.
 * EXAMG_OP_U pushes the value of q at the point; the position ops EXAMG_OP_X/Y/Z are refused in these programs, and EXAMG_OP_U is
 * refused by every entry point that takes an examg_expr_t.  The operand stack of a program may be at most EXAMG_NL_STACK deep (it
 * lives in registers).
 *
 * Arithmetic, fp64, no contraction, per point of the box:
 *   conv = the entries of A folded left to right in declared order over u (c_0 * u(i + o_0), then + c_k * u(i + o_k))
 *   N    = conv + (c(q(i)) * u(i)),      c evaluated in the order of the program
 * examg_nl_op:
 *   EXAMG_NL_APPLY    dst = N                      (`D = A * U + S * U`)
 *   EXAMG_NL_RESIDUAL dst = rhs - N                (`Residual = RHS - ( Laplace * Solution + gamSten * Solution )`)
 *   EXAMG_NL_ADD      dst = dst + N                (`RHS@coarser += Laplace@coarser * Approximation@coarser + gamSten@coarser * Approximation@coarser`)
 * examg_nl_smooth: one damped Newton step per point on the diagonal of the Jacobian, q = u:
 *   u_out = u + w * ((rhs - N) / (diag(A) + d(u(i))))         diag(A) = st->coef[st->diag], d a second program over u(i)
 *   (`Solution<next> = Solution<active> + 0.8 * ( ( RHS - ( Laplace * Solution<active> + gamSten * Solution<active> ) )
 *                      / ( diag ( Laplace ) + gam * ( 1.0 + Solution<active> ) * exp ( Solution<active> ) ) )`, ...exa4:81-83)
 *   colour = -1: all points, out of place (u_out != u_in: Jacobi); colour 0 / 1: the points with (i0 + i1 [+ i2]) % 2 == colour, in place
 *   (u_out == u_in: a nonlinear red-black Gauss-Seidel half sweep), and only for stencils the parity decouples (every entry off the
 *   centre has an odd offset sum: star stencils) -- on any other stencil the in-place loop depends on its order.
 * Every argument is indexed through its own layout (u: lu, q: lq, rhs: lf, dst / u_out: ld); only the points of the box (of the
 * colour) are written, in dst / u_out alone.  examg_nl_op: dst must not be u; q may be any of the arrays.  rhs / lf may be NULL
 * for EXAMG_NL_APPLY and EXAMG_NL_ADD.
 * Both refuse, before anything is launched: a stencil field, a stencil without a centre entry (st->diag must name the (0,0,0)
 * entry), layouts under a layout transformation (colour split), cell layouts (no duplicate layers), layouts that are not 2-D or
 * 3-D, a box that leaves an allocation (u: grown by the stencil's reach), a program that is empty, longer than EXAMG_MAX_NL_EXPR,
 * deeper than EXAMG_NL_STACK, breaks the stack discipline or holds an unknown or a position opcode.  An empty box is a no-op that
 * returns 0.  Nothing is allocated; the launches are capturable. */
#define EXAMG_OP_U 22
#define EXAMG_MAX_NL_EXPR 32
#define EXAMG_NL_STACK 8
typedef struct {
  int32_t n;
  int32_t op[EXAMG_MAX_NL_EXPR];
  double c[EXAMG_MAX_NL_EXPR];
} examg_nlexpr_t;
enum { EXAMG_NL_APPLY = 0, EXAMG_NL_RESIDUAL = 1, EXAMG_NL_ADD = 2 };
int examg_nl_op(int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lq, const double *q, const examg_layout_t *lf,
                const double *rhs, const examg_layout_t *ld, double *dst, const examg_stencil_t *st, const examg_nlexpr_t *c,
                const int32_t *begin, const int32_t *end, examg_stream_t stream);
int examg_nl_smooth(const examg_layout_t *lu, const double *u_in, const examg_layout_t *ld, double *u_out, const examg_layout_t *lf,
                    const double *rhs, const examg_stencil_t *st, const examg_nlexpr_t *c, const examg_nlexpr_t *d, double w, int colour,
                    const int32_t *begin, const int32_t *end, examg_stream_t stream);

/* ---- Table-coefficient stencils: operators on axis-aligned non-uniform grids ------------------------------------------------
 * `grid_isUniform = false, grid_isAxisAligned = true` (grid/ir/IR_SetupNodePositions.scala): the node positions are one table per axis,
 * and a stencil written over the virtual fields of the grid (`vf_cellWidth_x@[-1, 0, 0]`, Examples/Poisson/3D_FV_Poisson_fromL4.exa4:39-58)
 * depends on the position through one-dimensional tables only.  The host separates every entry into TERMS
 *     c_t(i) = X_t[i0] * ((s_t * Z_t[i2]) * Y_t[i1])
 * s_t a scalar, X_t / Y_t / Z_t tables over the iterator index of one axis; an absent table (tab[d] = -1) is the factor 1.0, and Z is
 * absent in 2-D.  The kernels form the coefficients of a point from the tables: u, rhs and dst are the only streams (24 B per point
 * where a 7-entry stencil field streams 80 B).
 *
 * examg_axis_stencil_t:
 *   nent, diag, off   the entries as in examg_stencil_t; every offset in {-1, 0, 1}, diag names the (0,0,0) entry
 *   wform             EXAMG_WEIGHT_INV_TIMES / EXAMG_WEIGHT_DIVIDE: how the smoother statement writes its weight (as for a stencil field)
 *   nterm, term[]     1 .. EXAMG_AXIS_MAX_TERMS terms, SORTED BY ENTRY, every entry with at least one; term[t].tab[d] is the index of a
 *                     table of axis d or -1
 *   tables[d]         device array of ntab[d] tables of tab_len[d] doubles each (table k at tables[d] + k * tab_len[d]); element j of
 *                     a table belongs to the iterator index tab_begin[d] + j
 *   route             EXAMG_AXIS_AUTO, or one of the two kernels by name (below)
 *
 * examg_axis_op: the three loop kinds of examg_stencil_op (EXAMG_APPLY, EXAMG_RESIDUAL, EXAMG_SMOOTH) on [begin, end).  Arithmetic, fp64,
 * no contraction, per point:
 *   term         c_t = X_t[i0] * ((s_t * Z_t[i2]) * Y_t[i1])
 *   coefficient  c_k = the terms of entry k folded left to right in declared order (c_t0, then + c_t1, ..)
 *   convolution  acc = c_0 * u(i + o_0), then acc + c_k * u(i + o_k) in entry order
 *   APPLY dst = acc;  RESIDUAL dst = rhs - acc;  SMOOTH dst = u + ww * (rhs - acc), ww = (1.0 / c_diag) * w or w / c_diag as wform names
 * -- from the coefficients on exactly what examg_stencil_op computes for a stencil field in planes that holds the c_k.  colour -1: all
 * points; 0 / 1: the points with (i0 + i1 + i2) % 2 == colour.  dst may be u only when colour >= 0.  Every argument through its own
 * layout; only the points of the box (of the colour) are written, in dst alone.
 * Refused, before anything is launched (non-zero, examg_last_error): a box with an index that a table of a used axis does not cover; a
 * box whose one-point shell leaves the u allocation, or that leaves the dst / rhs allocation; a layout under a layout transformation;
 * layouts that are not 2-D or 3-D or differ in dimensionality; offsets outside {-1, 0, 1}; terms not sorted by entry, an entry without
 * a term, a table index outside the axis's tables; dst == u without a colour.  An empty box is a no-op that returns 0.  Nothing is
 * allocated; the launches are capturable.
 *
 * Two kernels, the same bits.  EXAMG_AXIS_GENERIC: any stencil, one lane per point, the X table windows and the row products
 * (s * Z) * Y of a workgroup's rows staged in LDS.  EXAMG_AXIS_STAR: 3-D stencils of the centre and the six axis neighbours (each once,
 * in any order) with at most 12 terms; two x points per lane, z march with u[z-1], u[z], u[z+1] in registers, the X tables of the
 * wave's 128-point window in registers, the row products wave-uniform.  Eligibility depends on the stencil's shape alone, never on the
 * size of the box.  st->route = EXAMG_AXIS_AUTO takes the star kernel where it is eligible; EXAMG_AXIS_STAR on any other stencil is an
 * error.  examg_axis_route answers what examg_axis_op would do with these arguments, nothing launched: -1 refused (error text set),
 * 0 empty box, EXAMG_AXIS_GENERIC or EXAMG_AXIS_STAR. */
#define EXAMG_AXIS_MAX_TERMS 32
enum { EXAMG_AXIS_AUTO = 0, EXAMG_AXIS_GENERIC = 1, EXAMG_AXIS_STAR = 2 };
typedef struct examg_axis_term {
  int32_t entry;
  int32_t tab[3];
  double s;
} examg_axis_term_t;
typedef struct examg_axis_stencil {
  int32_t nent;
  int32_t diag;
  int32_t off[EXAMG_MAX_ENTRIES][3];
  int32_t wform;
  int32_t nterm;
  examg_axis_term_t term[EXAMG_AXIS_MAX_TERMS];
  const double *tables[3];
  int32_t ntab[3];
  int32_t tab_begin[3];
  int32_t tab_len[3];
  int32_t route;
} examg_axis_stencil_t;
int examg_axis_op(int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs, const examg_layout_t *ld,
                  double *dst, const examg_axis_stencil_t *st, double w, int colour, const int32_t *begin, const int32_t *end,
                  examg_stream_t stream);
int examg_axis_route(int mode, const examg_layout_t *lu, const examg_layout_t *lf, const examg_layout_t *ld, const examg_axis_stencil_t *st,
                     int colour, const int32_t *begin, const int32_t *end);

/* ---- Explicit flux-form time steps on cell fields ---------------------------------------------------------------------------
 * An explicit finite-volume update of coupled cell fields in 2-D: every component is a constant axis stencil on one field plus scaled
 * differences of point expressions evaluated at two neighbouring cells -- the Lax-Friedrichs step of the shallow-water equations
 * (Examples/SWE/2D_FV_SWE.exa4: `hNext = Centering * h - (dt / dx) * 0.5 * ( F0@east - F0@west ) - ..`).
 *
 * examg_flux_t:
 *   nfields, in[k]    1 .. EXAMG_FLUX_MAX_FIELDS input cell fields, all in the layout lin (ghost >= 1 in x and y where the box touches them)
 *   nprogs, prog[p]   0 .. EXAMG_FLUX_MAX_PROGS point programs in the compact type of the semilinear kernels.  EXAMG_OP_FIELD0 + k pushes the
 *                     value of in[k] AT THE CELL THE PROGRAM IS EVALUATED AT (k < nfields).  EXAMG_OP_U and the position and cell-width
 *                     opcodes are refused here; EXAMG_OP_FIELD* is refused by every other entry point.  Limits as for examg_nlexpr_t:
 *                     EXAMG_MAX_NL_EXPR (32) instructions, an operand stack of EXAMG_NL_STACK (8).
 *   ncomp, comp[c]    1 .. EXAMG_FLUX_MAX_COMP components:
 *       field         the index in `in` of the field q the stencil multiplies
 *       nent, off, coef   the constant stencil C_c: 1 .. EXAMG_FLUX_MAX_ENTRIES entries, each the centre or a unit axis offset in x or y
 *       nterms, term[t]   0 .. EXAMG_FLUX_MAX_TERMS terms {prog, plus, minus, scale}; plus and minus are each the zero offset or a unit
 *                         axis offset in x or y
 *   out[c]            the destination of component c, in the layout lout; overlaps no input and no other destination
 *
 * Arithmetic per cell i of [begin, end), fp64, no contraction:
 *   acc = C_c[0] * q(i + o_0);  acc = acc + C_c[k] * q(i + o_k)                      entries in declared order
 *   acc = acc + scale_t * ( P_t(i + plus_t) - P_t(i + minus_t) )                     terms in declared order
 *   out_c(i) = acc
 * P_t(j) is the program prog[term.prog] evaluated in the order of the program over the values in[k](j) at that ONE cell j.
 * Only the box of each out[c] is written.  Reads the inputs on the box and its one-cell axis shell.
 *
 * Refused before anything is launched, each with its own text in examg_last_error: layouts that are not 2-D (the 3-D kernels are not
 * built); a layout with duplicate layers (a node layout) or under a layout transformation; nfields, nprogs, ncomp, nent (an empty C_c
 * too) or nterms outside the limits; a field or program index out of range; an offset of a term or a stencil entry off the axes, of
 * reach 2 or in z; an out[c] that overlaps an input or another out; a box that leaves lout, or that grown by one cell leaves lin; a
 * program that is empty, too long, too deep, breaks the stack discipline or holds a refused opcode.  An empty box is a no-op that
 * returns 0.  Nothing is allocated; the launch is capturable.
 *
 * Two kernels, the same bits.  EXAMG_FLUX_GATHER: one lane per cell, x fastest; every term evaluates its program at both of its
 * cells; it takes any admissible call.  EXAMG_FLUX_MARCH: every program is evaluated once per cell -- a wave owns a window of 64
 * columns (62 of them written, the two halo columns are recomputed by the neighbouring windows) and marches in y two rows at a time with
 * the program values and field values of the rows y - 1 .. y + 2 in registers; x neighbours come from the adjacent lanes.  It takes
 * any admissible call too.  examg_flux_route answers which kernel examg_flux_step runs with these arguments, nothing launched: -1
 * refused (error text set), 0 empty box, EXAMG_FLUX_GATHER or EXAMG_FLUX_MARCH. */
#define EXAMG_OP_FIELD0 32
#define EXAMG_FLUX_MAX_FIELDS 6
#define EXAMG_FLUX_MAX_PROGS 8
#define EXAMG_FLUX_MAX_COMP 4
#define EXAMG_FLUX_MAX_TERMS 4
#define EXAMG_FLUX_MAX_ENTRIES 5
enum { EXAMG_FLUX_GATHER = 1, EXAMG_FLUX_MARCH = 2 };
typedef struct examg_flux_term {
  int32_t prog;
  int32_t plus[3];
  int32_t minus[3];
  double scale;
} examg_flux_term_t;
typedef struct examg_flux_comp {
  int32_t field;
  int32_t nent;
  int32_t off[EXAMG_FLUX_MAX_ENTRIES][3];
  double coef[EXAMG_FLUX_MAX_ENTRIES];
  int32_t nterms;
  examg_flux_term_t term[EXAMG_FLUX_MAX_TERMS];
} examg_flux_comp_t;
typedef struct examg_flux {
  int32_t nfields, nprogs, ncomp;
  examg_layout_t lin, lout;
  const double *in[EXAMG_FLUX_MAX_FIELDS];
  double *out[EXAMG_FLUX_MAX_COMP];
  examg_nlexpr_t prog[EXAMG_FLUX_MAX_PROGS];
  examg_flux_comp_t comp[EXAMG_FLUX_MAX_COMP];
} examg_flux_t;
int examg_flux_step(const examg_flux_t *fx, const int32_t *begin, const int32_t *end, examg_stream_t stream);
int examg_flux_route(const examg_flux_t *fx, const int32_t *begin, const int32_t *end);

/* max (EXAMG_REDUCE_MAX) or min (EXAMG_REDUCE_MIN) over the cells of [begin, end) of one such program over the values x[k] (k < nfields <=
 * EXAMG_FLUX_MAX_FIELDS, all in the layout l) at the cell: `loop over h with reduction ( max : v ) { v = max ( v, fabs ( hu / h ) + sqrt ( g * h ) ) }`.
 * The result stays on the device (*result; work: examg_reduce_work_bytes() bytes), in two stages like every reduction here; fmax and
 * fmin are exact, so the result has the same bits in any order of evaluation.  An empty box gives the identity: -inf for max, +inf for
 * min.  Refusals as for examg_flux_step: layouts (2-D or 3-D here), the program, a box that leaves the allocation, an unknown op. */
enum { EXAMG_REDUCE_MAX = 0, EXAMG_REDUCE_MIN = 1 };
int examg_reduce_expr_cell(int op, int nfields, const examg_layout_t *l, const double *const *x, const examg_nlexpr_t *prog, const int32_t *begin,
                           const int32_t *end, double *result, void *work, examg_stream_t stream);

/* ---- complex-valued node fields: `Layout X< Complex<Real>, Node >` (base/ir/IR_Datatype.scala:191-201: std::complex<double> per point;
 * Examples/Helmholtz/2D_FD_Helmholtz_fromL3: BiCGStab preconditioned by a cycle on the complex shifted Laplacian).
 * Data model.  A point of a complex field is two consecutive doubles (re, im); the array holds 2 * size(layout) doubles and starts 16-byte
 * aligned, so every point is one 16-byte access.  examg_layout_t is unchanged: every count is in POINTS.  A complex field seen as a real
 * field with every x count doubled (pad, ghost, dup, inner and the x bounds of a box) is a valid real layout: `set` to a real constant,
 * copies and pack / unpack of complex fields are the real entry points on that view (same bits) -- there are no complex twins of those.
 *
 * Arithmetic of every entry point below: fp64, no contraction, on the parts.  For a coefficient c = (a, b) and a value v = (x, y)
 *     c . v = (a * x, a * y)                       when b is exactly 0.0 (how `double * std::complex<double>` multiplies)
 *     c . v = (a * x - b * y, a * y + b * x)       otherwise
 * and for a divisor c = (cr, ci)
 *     z / c = (zr / cr, zi / cr)                   when ci is exactly 0.0
 *     z / c = ((zr * cr + zi * ci) / den, (zi * cr - zr * ci) / den),  den = cr * cr + ci * ci      otherwise.
 * These are NOT the bits of libstdc++'s scaled operator/ (which divides by max(|cr|, |ci|) first); the reference's results file carries six
 * digits.  Sums and differences are componentwise.
 *
 * examg_cstencil_op: a loop over a CONSTANT stencil (st->cfield NULL) whose offsets lie in {-1, 0, 1}^nd, nd = 2 or 3, any entry order.
 * Entry k has the coefficient (st->coef[k], coef_im[k]); coef_im NULL: all imaginary parts 0.0.  w = (w[0], w[1]).
 *     conv = c_0 . u(i + o_0);  conv = conv + c_k . u(i + o_k), k = 1 .. nent - 1 in declared order
 *     EXAMG_APPLY     dst = conv
 *     EXAMG_RESIDUAL  dst = rhs - conv
 *     EXAMG_SMOOTH    dst = u + w . (rhs - conv)
 *     EXAMG_CRELAX    `solve locally relax w { u => (A * u) == rhs }` with one unknown, in the form of solver/ir/IR_LocalDirectInvert.scala:
 *                     126-136, in place on the points of one colour: off = the off-centre entries folded in declared order like conv (the
 *                     centre entry st->diag skipped), b = rhs - off (b = rhs where there is no off-centre entry), x = b / c_centre,
 *                     u = (u * (1.0 - w[0])) + (w[0] * x) on each part; w[0] == 1.0 gives u = x.  colour must be 0 or 1, w[1] must be 0.0,
 *                     dst must be u (or NULL) and ld is not read.
 * colour, the box, the per-argument layouts (u through lu, rhs through lf, dst through ld) and aliasing as for examg_stencil_op: -1 all
 * points, else the points with (i0 + i1 + i2) % 2 == colour.  u and dst may be the same array only when colour >= 0 and every off-centre
 * entry reaches a point of the other colour (the sum of its offsets is odd: star stencils, with or without all their entries); EXAMG_CRELAX
 * needs such a stencil.  Only the points of the box (of the colour) are written, in dst alone.
 * Refused before anything is launched, each with its own text: a null argument; a mode outside the four; nent outside 1 .. 27; a stencil
 * field (st->cfield); a layout that is not 2-D or 3-D or is under a layout transformation; an offset outside {-1, 0, 1} or in a dimension
 * the layouts do not have; an array that is not 16-byte aligned; a box that leaves the dst or rhs allocation, or that grown by the stencil's
 * reach leaves the u allocation; dst == u without a colour or with an off-centre entry whose offsets sum to an even number; for EXAMG_CRELAX
 * a colour other than 0 / 1, w[1] != 0.0, a dst other than u, such an entry, a st->diag that is not the (0, 0, 0) entry.  An empty box is a no-op that returns 0.
 * Two kernels, the same bits.  EXAMG_CSTENCIL_GATHER: one lane per point, every entry read from memory; any admissible call.
 * EXAMG_CSTENCIL_MARCH: star stencils of reach 1 with all 2 * nd + 1 entries (5-point in 2-D, 7-point in 3-D), any entry order, all four
 * modes and colours: a wave owns 64 consecutive points of a row and marches in y (2-D) or z (3-D), one lane per point with 16-byte loads
 * and stores, the three rows (planes) of u in registers, x neighbours from the adjacent lanes (the end lanes read theirs).
 * examg_cstencil_route answers which one a call takes, nothing launched: -1 refused (text set), 0 empty box, else EXAMG_CSTENCIL_*. */
#define EXAMG_CRELAX 3
enum { EXAMG_CSTENCIL_GATHER = 1, EXAMG_CSTENCIL_MARCH = 2 };
int examg_cstencil_op(int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs, const examg_layout_t *ld,
                      double *dst, const examg_stencil_t *st, const double *coef_im, const double *w, int colour, const int32_t *begin,
                      const int32_t *end, examg_stream_t stream);
int examg_cstencil_route(int mode, const examg_layout_t *lu, const double *u, const examg_layout_t *lf, const double *rhs, const examg_layout_t *ld,
                         const double *dst, const examg_stencil_t *st, const double *coef_im, const double *w, int colour, const int32_t *begin,
                         const int32_t *end);

/* The vector updates of BiCGStab on complex fields, evaluated in this association (a = (a[0], a[1]), b likewise; b is read by the last
 * form only and may be NULL otherwise, as may lz / z):
 *     EXAMG_C_XPAY     dst = x + a . y
 *     EXAMG_C_XMAY     dst = x - a . y
 *     EXAMG_C_XPAYMBZ  dst = x + a . (y - b . z)
 * Each argument through its own layout; dst may be any of the operands (every point reads its own operands first).  Refused: null
 * arguments, an unknown form, transformed layouts, misaligned arrays, a box that leaves an allocation. */
enum { EXAMG_C_XPAY = 0, EXAMG_C_XMAY = 1, EXAMG_C_XPAYMBZ = 2 };
int examg_clincomb(int form, const examg_layout_t *lx, const double *x, const examg_layout_t *ly, const double *y, const examg_layout_t *lz,
                   const double *z, const examg_layout_t *ld, double *dst, const double *a, const double *b, const int32_t *begin,
                   const int32_t *end, examg_stream_t stream);

/* The UNCONJUGATED sum over the box of x . y (the reference's loops read `resHat * Residual`): result[0] = sum of (xr * yr) - (xi * yi),
 * result[1] = sum of (xr * yi) + (xi * yr), every product rounded on its own and added on its own (2 K terms per part for K points).
 * result: 2 doubles in device memory; work: examg_reduce_work_bytes() bytes.  A fixed tree: the same bits on every call with the same
 * box.  An empty box gives (0.0, 0.0).  Refused: a null argument, layouts that are not 2-D or 3-D or are under a layout transformation, a
 * misaligned array, a box that leaves the x or the y allocation. */
int examg_cdot(const examg_layout_t *lx, const double *x, const examg_layout_t *ly, const double *y, const int32_t *begin, const int32_t *end,
               double *result, void *work, examg_stream_t stream);

/* The node transfer operators of examg_restrict and examg_prolong_add (real weights, 2-D and 3-D, `scale`; the same boxes, footprints and
 * order of the terms) applied to each part: bit-equal to the real entry points run on the de-interleaved parts.  An empty box is a no-op that
 * returns 0.  Refused, both: a null argument, layouts that are not 2-D or 3-D, of different dimensionality or under a layout transformation, a
 * misaligned array.  examg_crestrict: a box that leaves the coarse allocation, a fine footprint [2 * begin - 1, 2 * (end - 1) + 1] that leaves
 * the fine allocation.  examg_cprolong_add: a box that leaves the fine allocation, a negative fine index, a coarse footprint [begin / 2, end / 2]
 * that leaves the coarse allocation. */
int examg_crestrict(const examg_layout_t *lfine, const double *res_fine, const examg_layout_t *lcoarse, double *rhs_coarse, double scale,
                    const int32_t *begin, const int32_t *end, examg_stream_t stream);
int examg_cprolong_add(const examg_layout_t *lcoarse, const double *u_coarse, const examg_layout_t *lfine, double *u_fine, const int32_t *begin,
                       const int32_t *end, examg_stream_t stream);

/* x(i) = x(i + off) / c on the box, c = (c[0], c[1]): the absorbing-boundary assignment `u@[0,0] = u@[1,0] / (1 - (0+1j) * k * h)` of a
 * boundary function.  Refused: a box that overlaps its own image shifted by off (off = 0 among them), a box or an image that leaves the
 * allocation, an offset in a dimension the layout does not have, transformed layouts, a misaligned array. */
int examg_cshift_div(const examg_layout_t *l, double *x, const int32_t *off, const double *c, const int32_t *begin, const int32_t *end,
                     examg_stream_t stream);

/* dst(i) = (re(i), im(i)) on the box from two REAL fields, each through its own layout; a NULL part is 0.0.  How `RHS = <real point
 * expression>` reaches a complex field: examg_fill_expr into a real scratch field, then this call.  Refused: a box that leaves an allocation, a
 * misaligned or transformed dst, a part whose layout has another dimensionality than dst. */
int examg_cfrom_parts(const examg_layout_t *l, double *dst, const examg_layout_t *lre, const double *re, const examg_layout_t *lim, const double *im,
                      const int32_t *begin, const int32_t *end, examg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EXAMG_H */
