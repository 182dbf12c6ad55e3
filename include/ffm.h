/*
 * ffm.h -- C ABI of libffm.so, the MI355X (gfx950) implementation of fireFoam's
 * per-time-step hot path: lduMatrix kernels, preconditioned Krylov solves and
 * finite-volume assembly, as hand-written HIP kernels.
 *
 * This is the drop-in boundary.  Each entry point names the
 * reference call site it serves and the OpenFOAM-dev (pinned @940e28f,
 * reference CHANGELOG:1-3; not vendored in the reference) interface it
 * replaces.  INTEGRATION.md shows the OpenFOAM-side binding
 * (a lduMatrix::solver registered through the run-time selection table and
 * loaded with controlDict `libs (...)`, the mechanism the reference itself
 * uses in cases/pyrolysis1D/system/controlDict:59-62).
 *
 * Conventions: plain C; opaque handles; every function returns 0 on success or
 * a negative ffm_status; no exceptions cross the boundary; pointers are HOST
 * pointers unless the parameter name ends in `_d` (device pointer in the
 * context's HIP device); the library never frees caller memory; one context =
 * one GPU = one host thread (OpenFOAM runs one rank per process).
 * All floating point is fp64, all labels int32 (OpenFOAM WM_PRECISION_OPTION=DP,
 * WM_LABEL_SIZE=32).
 */
#ifndef FFM_H
#define FFM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ffm_ctx ffm_ctx;
typedef struct ffm_ldu ffm_ldu;

typedef enum ffm_status {
    FFM_OK = 0,
    FFM_ERR_ARG = -1,        /* bad argument / inconsistent sizes             */
    FFM_ERR_ADDR = -2,       /* LDU addressing not upper-triangular ordered   */
    FFM_ERR_HIP = -3,        /* HIP runtime error (see ffm_last_error)        */
    FFM_ERR_NODEVICE = -4,   /* no usable GPU                                 */
    FFM_ERR_UNSUPPORTED = -5,/* solver/preconditioner combination not offered */
    FFM_ERR_COMM = -6        /* RCCL error                                    */
} ffm_status;

/* lduMatrix::solver run-time table keys (fvSolution `solver`), reference
 * cases/steckler/system/fvSolution:21-81, cases/wallFireSpread2D/system/fvSolution:115-152 */
typedef enum ffm_solver {
    FFM_PCG = 0, FFM_PBICGSTAB = 1, FFM_PBICG = 2, FFM_DIAGONAL = 3, FFM_SMOOTH = 4,
    FFM_GAMG = 5      /* through ffm_gamg_* only (an agglomeration object per mesh); ffm_solve_d refuses it */
} ffm_solver;
/* fvSolution `preconditioner` / `smoother` */
typedef enum ffm_precond {
    FFM_NONE = 0, FFM_DIC = 1, FFM_DILU = 2, FFM_GS = 3, FFM_SYMGS = 4, FFM_DIAGONALP = 5
} ffm_precond;

/* SolverPerformance<scalar> (what `DICPCG:  Solving for p_rgh, Initial residual
 * = ..., Final residual = ..., No Iterations n` prints; golden log
 * cases/steckler/original/linux64/log.fireFoam:220)                          */
typedef struct ffm_perf {
    double initialResidual, finalResidual;
    int nIterations, converged, singular;
} ffm_perf;

/* ------------------------------------------------------------------ context */
/* stream: a hipStream_t to launch on, or NULL to create a private stream.    */
int ffm_ctx_create(int device, void *stream, ffm_ctx **out);
int ffm_ctx_destroy(ffm_ctx *ctx);
int ffm_ctx_sync(ffm_ctx *ctx);
void *ffm_ctx_stream(ffm_ctx *ctx);
const char *ffm_last_error(void);
const char *ffm_version(void);

/* device memory helpers so a host without HIP headers (the C++ Foam layer, an
 * OpenFOAM shim) can hold fields on the GPU                                  */
int ffm_malloc(ffm_ctx *ctx, size_t bytes, void **ptr_d);
int ffm_free(ffm_ctx *ctx, void *ptr_d);
/* the same allocator without the zero-fill: for a block whose every byte the caller overwrites next (the result of a field
 * operation, a copy) -- on small meshes the fill kernel costs as much as the operation */
int ffm_malloc_uninit(ffm_ctx *ctx, size_t bytes, void **ptr_d);
/* ffm_malloc / ffm_free go through a stream-ordered caching allocator (freed blocks are reused by later allocations of the same
 * size class on the context stream, without synchronising; every block is handed out zero-filled); ffm_ctx_trim returns the cached
 * blocks to the runtime */
int ffm_ctx_trim(ffm_ctx *ctx);
int ffm_memcpy_h2d(ffm_ctx *ctx, void *dst_d, const void *src, size_t bytes);
int ffm_memcpy_d2h(ffm_ctx *ctx, void *dst, const void *src_d, size_t bytes);
int ffm_memcpy_d2d(ffm_ctx *ctx, void *dst_d, const void *src_d, size_t bytes);
int ffm_memset(ffm_ctx *ctx, void *dst_d, int value, size_t bytes);

/* element-wise field algebra (Field<scalar> operators of the Foam layer): one pass per operator, like
 * OpenFOAM's own tmp-field evaluation, so an expression rounds the way the reference's does                        */
enum { FFM_OP_ADD = 0, FFM_OP_SUB = 1, FFM_OP_MUL = 2, FFM_OP_DIV = 3, FFM_OP_MAX = 4, FFM_OP_MIN = 5,
       FFM_OP_NEGSEL = 6 /* a < 0 ? b : a  (a marker value selects the other operand) */ };
enum { FFM_UN_NEG = 0, FFM_UN_SQR = 1, FFM_UN_MAG = 2, FFM_UN_SQRT = 3, FFM_UN_POS0 = 4 /* pos0(x) = x >= 0 ? 1 : 0 */ };
int ffm_field_binary(ffm_ctx *ctx, int op, long n, const double *a_d, const double *b_d, double *out_d);
/* out = a op s, or s op a when scalarFirst != 0 */
int ffm_field_scalar(ffm_ctx *ctx, int op, long n, const double *a_d, double s, int scalarFirst, double *out_d);
int ffm_field_unary(ffm_ctx *ctx, int op, long n, const double *a_d, double *out_d);
int ffm_field_fill(ffm_ctx *ctx, long n, double s, double *out_d);
/* One element-wise expression over fields in ONE pass (the Foam layer's lazily evaluated field algebra, include/ffmFoam.H: dField):
 * a postfix program over an operand stack of depth <= 4.  code[k] = kind << 12 | arg:
 *   FFM_EVAL_LOAD   arg = index into arrays[]          push arrays[arg][i]
 *   FFM_EVAL_IMM    arg = index into imm[]             push imm[arg]
 *   FFM_EVAL_BINARY arg = FFM_OP_*                     b = pop, a = pop, push (a op b)
 *   FFM_EVAL_UNARY  arg = FFM_UN_*                     top = op(top)
 * The value left on the stack is out[i]; at least one array (a constant is ffm_field_fill).  Every operation rounds as the separate ffm_field_binary / _scalar / _unary call does, so the
 * result is bit for bit that of the chain of calls (OpenFOAM's tmp<Field> operator chains, e.g. solver/pEqn.H:5-12); `out` must not
 * overlap an input.                                                                                                              */
enum { FFM_EVAL_LOAD = 1, FFM_EVAL_IMM = 2, FFM_EVAL_BINARY = 3, FFM_EVAL_UNARY = 4 };
#define FFM_EVAL_MAX_ARRAYS 8
#define FFM_EVAL_MAX_IMM 8
#define FFM_EVAL_MAX_INSTR 32
int ffm_field_eval(ffm_ctx *ctx, long n, int nArrays, const double *const *arrays_d, int nImm, const double *imm, int nInstr,
                   const unsigned short *code, double *out_d);

/* ----------------------------------------------------------- lduAddressing */
/* Replaces lduAddressing + lduMatrix construction
 * [upstream src/OpenFOAM/matrices/lduMatrix/lduAddressing/lduAddressing.H].
 * lowerAddr/upperAddr: owner/neighbour cell of every internal face in
 * OpenFOAM's upper-triangular order (l<u, faces sorted by owner).  Builds on
 * the device: ownerStart, losort, losortStart, the dependency levels of the
 * DIC/DILU/Gauss-Seidel sweeps and a level-major cell renumbering (skipped
 * when the caller's numbering is already level-major).                       */
int ffm_ldu_create(ffm_ctx *ctx, int nCells, int nFaces, const int *lowerAddr,
                   const int *upperAddr, ffm_ldu **out);
/* Decomposed (one rank per GPU) form: cells [0,nOwned) are this rank's, cells
 * [nOwned, nOwned+nGhost) are copies of neighbour-rank cells (one layer across the
 * cut faces, which are ordinary faces owned by the owned cell).  Rows exist for owned
 * cells only; DIC/DILU ignore faces towards ghosts (block-Jacobi, as OpenFOAM's
 * processor interfaces); Amul refreshes the ghost entries of its argument first
 * (ffm_ldu_set_ghost_exchange).  Cell fields have nOwned+nGhost entries.          */
int ffm_ldu_create_ext(ffm_ctx *ctx, int nOwned, int nGhost, int nFaces, const int *lowerAddr,
                       const int *upperAddr, ffm_ldu **out);
int ffm_renumber_levels_ext(int nOwned, int nGhost, int nFaces, const int *lowerAddr,
                            const int *upperAddr, int *newToOldCell, int *newToOldFace);
/* Would ffm_ldu_create_ext accept this addressing?  Host code only, no device and no
 * context: FFM_OK, or the code ffm_ldu_create_ext would return, with its message in
 * ffm_last_error.  The limits of the row layout: at most 32 upper and 32 lower faces
 * per cell; fewer than 2^27 cells, and fewer than 2^26 where some cell owns more than
 * 16 faces towards owned cells (wide coarse GAMG levels).                            */
int ffm_ldu_check_layout(int nOwned, int nGhost, int nFaces, const int *lowerAddr,
                         const int *upperAddr);
/* Same with a grouping hint for the sweeps: groupHint[c] = any label shared by owned cells that should be swept by one
 * workgroup (e.g. a 2-D tile of cell columns, from the cell centres).  Used when the label classes form an acyclic
 * dependency graph, ignored otherwise (NULL: the library chunks the caller's cell order).                         */
int ffm_ldu_create_hint(ffm_ctx *ctx, int nOwned, int nGhost, int nFaces, const int *lowerAddr,
                        const int *upperAddr, const int *groupHint, ffm_ldu **out);
int ffm_renumber_hint(int nOwned, int nGhost, int nFaces, const int *lowerAddr, const int *upperAddr,
                      const int *groupHint, int *newToOldCell, int *newToOldFace);
/* a group hint from the cell centres C[3][nCells] (mesh.C()): 2-D tiles, about tileCells (0: default 16) cells wide, of
 * columns along the axis consecutive cell labels follow; pure host code                                              */
int ffm_tile_hint_from_centres(int nCells, const double *C, int tileCells, int *hint);
/* neighbour q (rank nbrRank[q]) receives this rank's cells sendCells[...] (sendCount[q] of
 * them, concatenated) and fills recvCount[q] consecutive ghost cells, in neighbour order    */
int ffm_ldu_set_ghost_exchange(ffm_ldu *ldu, int nNbr, const int *nbrRank, const int *sendCount,
                               const int *sendCells, const int *recvCount);
int ffm_halo_refresh_d(ffm_ldu *ldu, double *field_d);
int ffm_ldu_nowned(const ffm_ldu *ldu);
int ffm_ldu_destroy(ffm_ldu *ldu);
int ffm_ldu_ncells(const ffm_ldu *ldu);
int ffm_ldu_nfaces(const ffm_ldu *ldu);
int ffm_ldu_nlevels(const ffm_ldu *ldu);
/* which sweep kernels DIC / DILU / Gauss-Seidel use on this matrix: 0 dataflow sweeps in level-major numbering, 2 tiled
 * wavefront (ffm_tile.hip: group hint or detected blockMesh box)                                                    */
int ffm_ldu_sweep_mode(const ffm_ldu *ldu);
/* 1 when the caller's cell numbering is used as is (no permutation passes)   */
int ffm_ldu_is_native_order(const ffm_ldu *ldu);
/* new->old cell permutation chosen by the library (host, int[nCells])        */
int ffm_ldu_get_cell_order(const ffm_ldu *ldu, int *newToOld);

/* Level-major renumbering of an LDU graph, for hosts that want to renumber the
 * mesh once (like renumberMesh) so that no permutation pass is ever needed:
 * newToOldCell[nCells], newToOldFace[nFaces]; the renumbered faces are again in
 * upper-triangular order and keep owner<neighbour.  Pure host code.          */
int ffm_renumber_levels(int nCells, int nFaces, const int *lowerAddr,
                        const int *upperAddr, int *newToOldCell,
                        int *newToOldFace);

/* lduMatrix::diag()/upper()/lower(): lower == NULL => symmetric matrix.      */
int ffm_ldu_set_coeffs(ffm_ldu *ldu, const double *diag, const double *upper,
                       const double *lower);
int ffm_ldu_set_coeffs_d(ffm_ldu *ldu, const double *diag_d,
                         const double *upper_d, const double *lower_d);

/* Native face layout (for hosts that assemble on the device in the library's own
 * layout and skip the LDU-order gather): the library stores faces as a sliced
 * owner-ELL; nNative >= nFaces entries incl. padding.  callerToNative[f] = native
 * index of caller face f.  Only valid when ffm_ldu_is_native_order() == 1.     */
int ffm_ldu_n_native_faces(const ffm_ldu *ldu);
int ffm_ldu_get_face_map(const ffm_ldu *ldu, int *callerToNative);
int ffm_ldu_set_coeffs_native_d(ffm_ldu *ldu, const double *diag_d,
                                const double *upper_d, const double *lower_d);
/* zero-copy form of the same: the matrix reads the caller's device arrays until the next set/bind call (the caller keeps them
 * alive and unchanged); offDiagUnchanged != 0 tells the library that upper/lower hold the same values as at the previous call
 * (the components of a vector equation differ in the boundary diagonal only: fvMatrix::solveSegregated)               */
int ffm_ldu_bind_coeffs_native_d(ffm_ldu *ldu, const double *diag_d, const double *upper_d,
                                 const double *lower_d, int offDiagUnchanged);
/* ends a bind: the matrix refers to its own buffers again (contents unspecified until the next set / bind), the caller may free its arrays */
int ffm_ldu_unbind_coeffs(ffm_ldu *ldu);
/* the generation of the off-diagonal coefficients: every set call and every bind with offDiagUnchanged == 0 advances it, unbind and
 * a bind with offDiagUnchanged != 0 do not.  A caller that remembers which arrays it bound last may pass offDiagUnchanged != 0 only
 * while this value is the one it saw after that bind: nobody else has given the matrix other off-diagonals meanwhile          */
unsigned long ffm_ldu_offdiag_epoch(const ffm_ldu *ldu);
/* test support of the tiled sweeps' coefficient arrays (three doubles per cell and array: the present entries of a row in row order,
 * then 0.0): one of them, made current first as a sweep would, copied to the host -- which: 0 forward upper, 1 forward lower,
 * 2 backward upper, 3 backward lower; out_h [3 * owned cells]; FFM_ERR_UNSUPPORTED without a tile plan -- and the number of gather passes
 * the matrix has launched to fill them (the *_direct assembly entry points below fill them without one)                        */
int ffm_ldu_tile_coef_read(ffm_ldu *ldu, int which, double *out_h);
long ffm_ldu_tile_gathers(const ffm_ldu *ldu);
/* The neighbour codes of the tile plan (16-bit LDS slots and cell distances, per cell and entry) are kept once per distinct entry
 * block: entries whose blocks are equal byte for byte share one.  which: 0 forward sweep, 1 backward sweep, 2 tiled Amul;
 * *uniqueBytes: the blocks the plan keeps, *totalBytes: the blocks its entries refer to (what one array per cell would hold).
 * FFM_TILE_CODE_SHARE=0 in the environment when the matrix is created gives every entry a block of its own (unique == total);
 * 1 shares the sweeps' blocks only, 2 the tiled Amul's only (A/B runs of one reader), unset or 3 both.
 * FFM_ERR_UNSUPPORTED without a tile plan.                                                                                      */
int ffm_ldu_tile_code_bytes(const ffm_ldu *ldu, int which, long *uniqueBytes, long *totalBytes);
/* test support: the sharing itself on host arrays (no device).  Block i = codes[start[i], start[i] + len[i]) in shorts.  share != 0:
 * pool_out receives every distinct block once, in the order of first appearance; share == 0: pool_out is a copy of codes.  Then
 * padShorts shorts of 0xFFFF.  offset_out[i]: byte offset of block i in pool_out (0 for an empty block); *uniqueShorts: shorts of
 * the pool's blocks; *poolShorts: shorts written, padding included; FFM_ERR_ARG if poolCapacity (shorts) is too small.         */
int ffm_tile_share_codes(int nBlocks, const long *start, const int *len, const unsigned short *codes, long nCodes, int share, long padShorts,
                         unsigned int *offset_out, unsigned short *pool_out, long poolCapacity, long *uniqueShorts, long *poolShorts);

/* processor patches (lduInterface / interfaceBouCoeffs / interfaceIntCoeffs):
 * face i of patch p couples cell faceCells[p][i] (caller numbering) with face i
 * of the matching patch on rank neighbRank[p]; as in OpenFOAM there is one
 * patch per neighbour rank (or both sides list their common patches in the
 * same order).  Amul: y[faceCells] -= bouCoeffs*psi_neighbour.  DIC/DILU ignore
 * the interfaces (block-Jacobi).  Needs ffm_comm_init / ffm_comm_init_host.
 * A call replaces the interfaces of an earlier one; nPatches == 0 removes them.  A refused call (FFM_ERR_ARG: a negative
 * size, a neighbour rank outside the context's ranks, a faceCell outside the matrix, a null array) leaves the matrix with
 * no interfaces at all.
 * Entry points that take such a matrix: ffm_spmv, ffm_tmul (interfaceIntCoeffs), ffm_residual, ffm_sumA, ffm_gs_smooth,
 * ffm_precond_* (block-Jacobi), ffm_solve / ffm_solve_d with every solver they offer (FFM_GAMG is not one, see above), and
 * ffm_solve_multi_d, which solves several such systems one after the other (one system is the matrix's own lane as ever).
 * Entry points that refuse it with FFM_ERR_UNSUPPORTED: ffm_gamg_create -- and ffm_gamg_set_matrix_d / _native_d and
 * ffm_gamg_solve_d where the interfaces were set after the hierarchy was made -- (the coarse levels couple the ranks
 * through ghost cells: give the rank as ffm_ldu_create_ext + ffm_ldu_set_ghost_exchange), ffm_flow_order_create,
 * ffm_flow_order_create_staged, ffm_solve_ordered_d, ffm_solve_ordered_staged_d and ffm_solve_triangular_rows_d.  The FV
 * operators, the fused assembly and the plume driver work on the ghost-cell form only.                                      */
int ffm_ldu_set_interfaces(ffm_ldu *ldu, int nPatches, const int *patchSizes,
                           const int *const *faceCells,
                           const double *const *bouCoeffs,
                           const double *const *intCoeffs,
                           const int *neighbRank);
int ffm_ldu_set_global_cells(ffm_ldu *ldu, long globalCells);
/* the count set above; the owned cells of this rank until it is set (gAverage divides by it) */
long ffm_ldu_global_cells(const ffm_ldu *ldu);
/* Pair tags of the point-to-point messages of one exchange (kind 0: the processor patches of ffm_ldu_set_interfaces, kind 1:
 * the neighbour entries of ffm_ldu_set_ghost_exchange): tags[i] is a label both ranks give to the two entries that exchange
 * with each other.  Messages are posted in ascending tag order, so two ranks that share several patches (cyclic / periodic
 * two-rank decompositions, split processor patches) match them correctly whatever their local patch order.  Without tags
 * the entry order is used, i.e. both sides must list their common patches in the same order (as OpenFOAM does).          */
int ffm_ldu_set_exchange_tags(ffm_ldu *ldu, int kind, int n, const int *tags);

/* ------------------------------------------------------- lduMatrix kernels */
/* lduMatrix::Amul -- the metric kernel (solver/pEqn.H:39 via PCG; UEqn.H() in
 * solver/pEqn.H:5).  x_d, y_d in the caller's cell numbering.                */
int ffm_spmv(ffm_ldu *ldu, const double *x_d, double *y_d);
int ffm_tmul(ffm_ldu *ldu, const double *x_d, double *y_d);      /* ::Tmul     */
int ffm_sumA(ffm_ldu *ldu, double *s_d);                         /* ::sumA     */
int ffm_residual(ffm_ldu *ldu, const double *x_d, const double *b_d, double *r_d);
/* preconditioner pieces, exposed for parity tests             */
int ffm_precond_setup(ffm_ldu *ldu, int precond, double *rD_out_d /*nullable*/);
int ffm_precond_apply(ffm_ldu *ldu, int precond, int transpose,
                      const double *r_d, double *w_d);
/* calcReciprocalD (DIC / DILU) of nSys = 2..5 systems that share the bound off-diagonal coefficients and differ in the diagonal,
 * in the ONE sweep ffm_solve_multi_d uses for them (tiled matrix in the library's cell order; anything else is refused).           */
int ffm_precond_setup_multi(ffm_ldu *ldu, int precond, int nSys, const double *const *diag_d, double *const *rD_out_d);
/* The tile plan's largest cell distance between a cell and a neighbour served from the sweeps' LDS ring, the limit of the plan's own
 * ring (up to four lock-step systems) and the limit of the short ring that five systems need: with reach > limit5,
 * ffm_solve_multi_d solves five systems one after the other and ffm_precond_setup_multi refuses five.  Tiled matrices only.   */
int ffm_ldu_tile_reach(const ffm_ldu *ldu, int *reach, int *limit, int *limit5);
int ffm_gs_smooth(ffm_ldu *ldu, int symmetric_sweep, int nSweeps, double *psi_d,
                  const double *b_d);

/* lduMatrix::solver::New(...)->solve(psi, source):
 * psi in/out, source in; controls = fvSolution entries tolerance, relTol,
 * minIter, maxIter, nSweeps (defaults 1e-6, 0, 0, 1000, 1).                  */
int ffm_solve_d(ffm_ldu *ldu, int solver, int precond, double tolerance,
                double relTol, int minIter, int maxIter, int nSweeps,
                double *psi_d, const double *source_d, ffm_perf *out);
int ffm_solve(ffm_ldu *ldu, int solver, int precond, double tolerance,
              double relTol, int minIter, int maxIter, int nSweeps,
              double *psi, const double *source, ffm_perf *out);
/* nSys systems that share the off-diagonal coefficients and differ in the diagonal and the right-hand side: the components of a
 * vector equation (fvMatrix<Type>::solveSegregated, OpenFOAM-dev fvMatrixSolve.C; solver/UEqn.H:19-30) and the species equations
 * under a multivariateSelection scheme with one diffusivity (solver/YEEqn.H:43-60).  Every system gets the solve a call of
 * ffm_ldu_bind_coeffs_native_d(diag_d[i], upper_d, lower_d) + ffm_solve_d would give it -- the same operations in the same order,
 * its own iteration count and residuals in out[i] -- but for PBiCGStab with DILU / DIC on a tiled matrix in the library's cell order
 * the systems (at most 5 at a time; 5 only where ffm_ldu_tile_reach reports reach <= limit5) advance in lock step and the preconditioner
 * sweeps and calcReciprocalD of those still iterating are one sweep each (coefficients and addressing read once).  Any other selection:
 * one solve after the other.  nSys = 1 is that one solve (the same routine: a single lane).
 * diag_d[i] [cells], upper_d / lower_d [native faces; lower_d NULL or == upper_d: symmetric], psi_d[i] in/out, source_d[i].
 * The matrix is left bound to the caller's arrays as by ffm_ldu_bind_coeffs_native_d.                                         */
int ffm_solve_multi_d(ffm_ldu *ldu, int nSys, int solver, int precond, double tolerance, double relTol, int minIter, int maxIter,
                      const double *const *diag_d, const double *upper_d, const double *lower_d, double *const *psi_d,
                      const double *const *source_d, ffm_perf *out /* [nSys] */);

/* timing helper for bench.py: runs `reps` back-to-back launches of the SpMV
 * kernel used inside the solvers on the context stream, bracketed by HIP
 * events on that stream; returns the average kernel time in milliseconds.    */
int ffm_bench_spmv(ffm_ldu *ldu, const double *x_d, double *y_d, int reps,
                   double *avg_ms);
/* the same for one preconditioner application (DIC: forward + backward sweep) on the bound matrix */
int ffm_bench_precond(ffm_ldu *ldu, int precond, const double *r_d, double *w_d, int reps, double *avg_ms);

/* ------------------------------------------------------- finite-volume mesh */
/* fvMesh geometry on the device (mesh.V(), Sf(), magSf(), weights(), deltaCoeffs(),
 * boundary(); reference use: solver/UEqn.H:28, solver/pEqn.H:7).  The LDU must
 * be in the library's cell order (ffm_renumber_levels).  Host arrays: V[N],
 * C[3][N]; Sf[3][F], magSf[F], weights[F], deltaCoeffs[F] in LDU face order;
 * per patch faceCells[n], Sf[3][n], deltaCoeffs[n].  Face fields handed to the
 * fv entry points are in the NATIVE face layout (ffm_mesh_nnative entries,
 * conversion helpers below); boundary fields have ffm_mesh_nboundary entries,
 * patches concatenated in the order given here.                              */
typedef struct ffm_mesh ffm_mesh;
int ffm_mesh_create(ffm_ldu *ldu, const double *V, const double *C,
                    const double *Sf, const double *magSf, const double *weights,
                    const double *deltaCoeffs, int nPatches, const int *patchSizes,
                    const int *const *faceCells, const double *const *patchSf,
                    const double *const *patchDeltaCoeffs, ffm_mesh **out);
/* mesh.Cf() of the internal faces, host array Cf[3][F] in LDU face order (needed by the LUST correction only) */
int ffm_mesh_set_face_centres(ffm_mesh *mesh, const double *Cf);
/* mesh.nonOrthCorrectionVectors() of the internal faces, host array [3][F] in LDU face order; needed by the `corrected`
 * snGrad / laplacian schemes on non-orthogonal meshes only (cases/wallFireSpread2D/system/fvSchemes: `Gauss linear corrected`) */
int ffm_mesh_set_nonorth_correction(ffm_mesh *mesh, const double *corrVec);
int ffm_mesh_destroy(ffm_mesh *mesh);
int ffm_mesh_nboundary(const ffm_mesh *mesh);
/* device geometry fields for the Foam layer: 0 V[N], 1 magSf[nNative], 2 deltaCoeffs[nNative], 3 weights[nNative],
 * 4 boundary magSf[B], 5 boundary deltaCoeffs[B], 6-8 boundary Sf x,y,z [B], 9-11 Sf x,y,z of the internal faces [nNative],
 * 12-14 cell centres x,y,z [N]                                                                                 */
const double *ffm_mesh_geometry_d(const ffm_mesh *mesh, int which);
int ffm_mesh_nnative(const ffm_mesh *mesh);
int ffm_faces_to_native(const ffm_mesh *mesh, const double *lduOrder, double *native_d);
int ffm_faces_from_native(const ffm_mesh *mesh, const double *native_d, double *lduOrder);

/* ------------------------------------------------------- fvc:: (explicit)    */
/* solver/UEqn.H:23-29, solver/pEqn.H:4-17,43-44, solver/YEEqn.H:87-95.  All
 * pointers are device pointers; *_f = face field (native), *_b = boundary field. */
int ffm_fvc_interpolate(ffm_mesh *m, const double *w_f, const double *vf, double *out_f);
int ffm_fvc_snGrad(ffm_mesh *m, const double *vf, double *out_f);
int ffm_fvc_snGrad_b(ffm_mesh *m, const double *vf, const double *vb, double *out_b);
int ffm_fvc_flux(ffm_mesh *m, const double *vx, const double *vy, const double *vz, double *out_f);
int ffm_fvc_surface_integrate(ffm_mesh *m, const double *ssf_f, const double *ssf_b, double *out);
int ffm_fvc_surface_sum(ffm_mesh *m, const double *ssf_f, const double *ssf_b, double *out);
int ffm_fvc_grad(ffm_mesh *m, const double *vf, const double *vb, double *gx, double *gy, double *gz);
int ffm_fvc_reconstruct(ffm_mesh *m, const double *ssf_f, const double *ssf_b, double *ox, double *oy, double *oz);
/* correctedSnGrad::correction(vf) = nonOrthCorrectionVectors & interpolate(grad(vf)), internal faces (one scalar component).
 * `corrected` snGrad = ffm_fvc_snGrad + this; `Gauss linear corrected` laplacian = the uncorrected matrix with
 * source -= V*ffm_fvc_surface_integrate(gamma_f*magSf*this, 0) */
int ffm_fvc_snGrad_correction(ffm_mesh *m, const double *gx, const double *gy, const double *gz, double *out_f);
/* limitedSurfaceInterpolationScheme weights: scheme 0 upwind, 1 linear,
 * 2 limitedLinear k, 3 limitedLinear01 k with bounds [lo,hi], 4 LUST (0.75 linear +
 * 0.25 upwind; vf and gradients unused), 5 linearUpwind (upwind weights; its explicit correction is
 * ffm_fv_linear_upwind_correction)  (cases/steckler/system/fvSchemes:28-54) */
int ffm_fv_limited_weights(ffm_mesh *m, int scheme, double k, double lo, double hi,
                           const double *phi_f, const double *vf, const double *gx,
                           const double *gy, const double *gz, double *out_w_f);
/* multivariateSelectionScheme (solver/YEEqn.H:1-10 `fv::convectionScheme<scalar>::New(mesh, fields, phi, mesh.divScheme("div(phi,Yi_h)"))`,
 * cases/steckler/system/fvSchemes:36-47): ONE limiter for all fields of the table, the face-wise minimum of the member schemes' limiters,
 * and the weights made of it.  ffm_fv_limited_limiter: the limiter of limitedLinear k (scheme 2) / limitedLinear01 k (scheme 3) of one
 * field into lim_f, or the running minimum when accumulateMin != 0; ffm_fv_weights_from_limiter: limiter*linear + (1 - limiter)*upwind. */
int ffm_fv_limited_limiter(ffm_mesh *m, int scheme, double k, double lo, double hi, const double *phi_f, const double *vf,
                           const double *gx, const double *gy, const double *gz, double *lim_f, int accumulateMin);
int ffm_fv_weights_from_limiter(ffm_mesh *m, const double *phi_f, const double *lim_f, double *out_w);
/* the same in one pass: the common weights over nf fields (schemes[i]: 2 limitedLinear, 3 limitedLinear01), bitwise equal to the
 * running-minimum chain above */
int ffm_fv_multivariate_weights(ffm_mesh *m, int nf, const int *schemes, double k, double lo, double hi, const double *phi_f,
                                const double *const *vf, const double *const *gx, const double *const *gy, const double *const *gz,
                                double *out_w);
/* ffm_fvc_grad_multi over the nf <= 6 fields + ffm_fv_multivariate_weights in ONE pass with the cell values staged through LDS on the tile
 * numbering (a workgroup walks a run of dependency levels of one tile; the values of the levels e-1, e, e+1 sit in an LDS window, a cell
 * forms its own gradients in registers, a face is written by its upwind cell): bit for bit the two-pass form without the 3 nf gradient
 * arrays.  vb: the fields' boundary values.  FFM_ERR_UNSUPPORTED where the matrix has no tile plan, the mesh is one block of a decomposed
 * case, cells have more than 3 lower / upper neighbours or nf > 6: the caller then runs the two-pass form.                            */
int ffm_fv_multivariate_weights_tiled(ffm_mesh *m, int nf, const int *schemes, double k, double lo, double hi, const double *phi_f,
                                      const double *const *vf, const double *const *vb, double *out_w);
/* The same pass with one more staged field K (patch values K_b) that is NOT in the minimum: out_w as above, and out_phiK[e] = phi_f*Kf on
 * every internal face, Kf interpolated with K's own limitedLinear (schemeK 2) / limitedLinear01 (3) weight of coefficient kK, bounds loK, hiK,
 * from the gradient the face's upwind cell forms in registers -- per face what ffm_fvc_grad + ffm_fvc_div_phiK_terms form, bit for bit, so
 * fvc::grad(K) is neither written nor read.  ffm_fvc_div_phiK_sum finishes the three cell fields.  Same refusals, nothing written.   */
int ffm_fv_multivariate_weights_phiK_tiled(ffm_mesh *m, int nf, const int *schemes, double k, double lo, double hi, const double *phi_f,
                                           const double *const *vf, const double *const *vb, double *out_w, int schemeK, double kK,
                                           double loK, double hiK, const double *K, const double *K_b, double *out_phiK);
/* divK, ddtK, -dpdt of ffm_fvc_div_phiK_terms from the face products phiK_f of the call above (lower faces, upper faces, patch faces, in
 * that order): one row pass on any mesh                                                                                              */
int ffm_fvc_div_phiK_sum(ffm_mesh *m, double rDeltaT, const double *phiK_f, const double *phi_b, const double *K, const double *K_b,
                         const double *rho, const double *rho0, const double *K0, const double *dpdt, double *divK, double *ddtK,
                         double *negDpdt);
/* `div(phi,U) Gauss LUST grad(U)`, explicit part, by the same tile walk: out_q[i][e] = phi_f*LUST::correction(U_i) on every internal face,
 * from grad(U_i) of the face's upwind cell formed in registers (U[3], U_b[3], out_q[3]: host arrays of device pointers).  With
 * ffm_fvm_lust_source3_sum bit for bit ffm_fvc_grad_multi + ffm_fvm_lust_source3 without the nine gradient arrays.  FFM_ERR_UNSUPPORTED,
 * nothing written, where ffm_fv_multivariate_weights_tiled refuses.                                                                  */
int ffm_fv_lust_phi_correction3_tiled(ffm_mesh *m, const double *phi_f, const double *const *U, const double *const *U_b,
                                      double *const *out_q);
/* source_c = rDeltaT*rho0*U0_c*V - V*surfaceIntegrate(q_f[c]) from the face products of the call above: one row pass on any mesh */
int ffm_fvm_lust_source3_sum(ffm_mesh *m, double rDeltaT, const double *rho0, const double *const *U0, const double *const *q_f,
                             double *const *source);

/* filteredLinear2V k l: the face weights of a VECTOR field, one limiter per face for its three components
 * (`div(phi,U) Gauss filteredLinear2V 0.2 0.05`, cases/wallFireSpread2D/system/fvSchemes:41, cases/pyrolysis1D/system/fvSchemes:39;
 * solver/UEqn.H:5).  U[3], gx[3], gy[3], gz[3]: host arrays of device pointers, g?[c] = the gradient of component c.        */
int ffm_fv_filtered_linear2V_weights(ffm_mesh *m, double k, double l, const double *phi_f, const double *const *U,
                                     const double *const *gx, const double *const *gy, const double *const *gz, double *out_w_f);

/* LUST<Type>::correction(vf) for one scalar component, internal faces: 0.25*(Cf - C_c) & grad(vf)_c with c the upwind cell
 * (`div(phi,U) Gauss LUST grad(U)`, cases/steckler/system/fvSchemes:32; solver/UEqn.H:5).  gaussConvectionScheme::fvmDiv
 * then adds fvc::surfaceIntegrate(phi*correction) to the matrix: source -= V * ffm_fvc_surface_integrate(phi_f*corr_f, 0). */
int ffm_fv_lust_correction(ffm_mesh *m, const double *phi_f, const double *gx, const double *gy,
                           const double *gz, double *out_f);
/* linearUpwind<Type>::correction(vf): (Cf - C_c) & grad(vf)_c with c the upwind cell, no factor
 * (`div(Ji,Ii_h) Gauss linearUpwind grad(Ii_h)`, cases/wallFireSpread2D/system/fvSchemes:58); used like the LUST one. */
int ffm_fv_linear_upwind_correction(ffm_mesh *m, const double *phi_f, const double *gx, const double *gy,
                                    const double *gz, double *out_f);

/* ------------------------------------------------------- fvm:: (implicit)    */
/* [fvm::ddt(rho,.)] + [fvm::div(phi,.)] (+/-) [fvm::laplacian(gamma,.)] in one
 * pass; absent terms: NULL.  Writes lduMatrix diag/upper/lower (native layout).
 * upper = lower = NULL with a ddt term only (it has no face coefficients); lower = NULL without convection (symmetric: lower = upper). */
int ffm_fvm_transport(ffm_mesh *m, double rDeltaT, const double *rho,
                      const double *phi_f, const double *w_f, const double *gamma_f,
                      int laplacianSign, double *diag, double *upper, double *lower);
/* the same with the convection weights of a scheme that needs only phi and the mesh's linear weights formed where they are used, no
 * weight field: scheme 0 upwind, 1 linear, 4 LUST (any other: FFM_ERR_ARG).  Bitwise equal to ffm_fv_limited_weights(scheme) +
 * ffm_fvm_transport. */
int ffm_fvm_transport_scheme(ffm_mesh *m, double rDeltaT, const double *rho, const double *phi_f, int scheme,
                             const double *gamma_f, int laplacianSign, double *diag, double *upper, double *lower);
/* The *_direct form of an assembly entry point writes what the plain form writes, and from the same launch the layout in which the
 * tiled sweeps of the mesh's matrix read upper / lower.  The solve that binds EXACTLY these upper / lower arrays next
 * (ffm_ldu_bind_coeffs_native_d, ffm_solve_multi_d), unchanged, then needs no gather pass; any other set / bind in between, and any
 * plain assembly entry point of the mesh called in between (it may refill the same arrays), makes that solve gather as ever.  FFM_ERR_UNSUPPORTED, nothing written, where the matrix has ghost cells, no tile plan or rows of more than three lower or
 * upper entries: call the plain form.  upper != lower. */
int ffm_fvm_transport_scheme_direct(ffm_mesh *m, double rDeltaT, const double *rho, const double *phi_f, int scheme,
                                    const double *gamma_f, int laplacianSign, double *diag, double *upper, double *lower);
/* internalCoeffs / boundaryCoeffs of the same terms for a patch field in
 * `mixed` form (valueFraction f, refValue, refGradient); fixedValue,
 * zeroGradient, fixedGradient, inletOutlet are special cases               */
int ffm_fvm_boundary_coeffs(ffm_mesh *m, const double *phi_b, const double *gamma_b,
                            int laplacianSign, const double *f, const double *ref,
                            const double *refGrad, double *internalCoeffs, double *boundaryCoeffs);
int ffm_bc_values(ffm_mesh *m, const double *f, const double *ref, const double *refGrad,
                  const double *vf, double *out_b);
/* fvMatrix::addBoundaryDiag + addBoundarySource (+ V*su)                     */
int ffm_fvm_add_boundary(ffm_mesh *m, const double *internalCoeffs, const double *boundaryCoeffs,
                         const double *diag, const double *source, const double *su,
                         double *diagOut, double *sourceOut);
/* fvMatrix<Type>::relax(alpha) (solver/UEqn.H:13, solver/YEEqn.H:56,107; equation factors e.g.
 * cases/wallFireSpread2D/system/fvSolution:194-200): diagonal dominance + under-relaxation in place,
 * source_c += (D - D0)*psiPrev_c for nCmpt = 1 or 3 components sharing the coefficients.            */
int ffm_fvm_relax(ffm_mesh *m, double alpha, int nCmpt, const double *upper, const double *lower,
                  const double *ic0, const double *ic1, const double *ic2, double *diag,
                  const double *psiPrev0, const double *psiPrev1, const double *psiPrev2,
                  double *source0, double *source1, double *source2);
/* fvMatrix::A(), H() (one component), flux()  (solver/pEqn.H:3,5,43)          */
int ffm_fvm_A(ffm_mesh *m, int nCmpt, const double *diag, const double *ic0, const double *ic1,
              const double *ic2, double *out);
int ffm_fvm_H(ffm_mesh *m, int nCmpt, int cmpt, const double *upper, const double *lower,
              const double *source, const double *ic0, const double *ic1, const double *ic2,
              const double *bcCmpt, const double *psi, double *out);
/* the three components of fvMatrix<vector>::H() in one pass, times rAU when given: HbyA = rAU*UEqn.H() (solver/pEqn.H:9);
 * source / internalCoeffs / boundaryCoeffs / psi / out: arrays of three device pointers; bitwise equal to three ffm_fvm_H
 * calls followed by the product */
int ffm_fvm_HbyA3(ffm_mesh *m, const double *upper, const double *lower, const double *const *source,
                  const double *const *internalCoeffs, const double *const *boundaryCoeffs, const double *const *psi,
                  const double *rAU, double *const *out);
/* p_rghEqn of solver/pEqn.H:28-36 in one pass: fvm::ddt(psi, p_rgh) + fvc::ddt(psi, rho)*gh + fvc::ddt(psi)*pRef +
 * fvc::div(phiHbyA) - fvm::laplacian(gamma, p_rgh) with its boundary coefficients (internalCoeffs / boundaryCoeffs from
 * ffm_fvm_boundary_coeffs) already added: upper / lower [native faces], diagOut / sourceOut [cells] are what the solver takes.
 * Bitwise equal to ffm_fvm_transport + ffm_fvc_surface_integrate + the three source updates + ffm_fvm_add_boundary.
 * lower may be NULL: the matrix is symmetric (lower = upper), and a caller that reads `upper` in both roles needs no second array. */
int ffm_fvm_pressure_eqn(ffm_mesh *m, double rDeltaT, const double *psi, const double *psi0, const double *p0,
                         const double *rho, const double *rho0, const double *gh, double pRef, const double *gamma_f,
                         const double *phiHbyA_f, const double *phiHbyA_b, const double *internalCoeffs,
                         const double *boundaryCoeffs, double *upper, double *lower, double *diagOut, double *sourceOut);
/* its *_direct form (see ffm_fvm_transport_scheme_direct) */
int ffm_fvm_pressure_eqn_direct(ffm_mesh *m, double rDeltaT, const double *psi, const double *psi0, const double *p0,
                                const double *rho, const double *rho0, const double *gh, double pRef, const double *gamma_f,
                                const double *phiHbyA_f, const double *phiHbyA_b, const double *internalCoeffs,
                                const double *boundaryCoeffs, double *upper, double *lower, double *diagOut, double *sourceOut);
/* three face passes of the pressure corrector (solver/pEqn.H:9-19,43-44), each two per-operator passes in one with their arithmetic:
 * phig = -rhorAUf*ghf*fvc::snGrad(rho)*magSf;  phiHbyA = (fvc::flux(rho*HbyA) + rhorAUf*ddtCorr) + phig;
 * fl = p_rghEqn.flux(), phi = phiHbyA + fl, t = (fl + phig)/rhorAUf (internal faces, native layout; symmetric matrix: lower = upper) */
int ffm_pc_phig(ffm_mesh *m, const double *rhorAUf, const double *ghf, const double *rho, double *phig);
int ffm_pc_phiHbyA(ffm_mesh *m, const double *rho, const double *vx, const double *vy, const double *vz, const double *rhorAUf,
                   const double *ddtCorr, const double *phig, double *phiHbyA);
int ffm_pc_flux(ffm_mesh *m, const double *upper, const double *lower, const double *psi, const double *phiHbyA, const double *phig,
                const double *rhorAUf, double *flux_f, double *phi_f, double *t_f);
/* solver/UEqn.H:23-29: the face flux of fvc::reconstruct, t = (-ghf*fvc::snGrad(rho) - fvc::snGrad(p_rgh))*magSf, in one pass */
int ffm_ue_buoyancy_flux(ffm_mesh *m, const double *ghf, const double *rho, const double *p_rgh, double *t_f);
/* Passes that form a face field where it is used instead of storing it for one reader; each bitwise equal to the chain it replaces.
 * ffm_pc_face_fluxes: rhorAUf = ffm_fvc_interpolate(NULL, rhorAU), then ffm_pc_phig and ffm_pc_phiHbyA from it, in one owner-row pass;
 *   all three are stored, padding entries of the native layout get 0.
 * ffm_pc_finish (single block): everything after the p_rgh solve in one pass over the cells -- ffm_pc_flux (upper/lower/p_rgh ->
 *   phi_f, stored by the owner, padding 0; the flux and t = (flux + phig)/rhorAUf are not stored), ffm_fvc_reconstruct of t with the
 *   patch part t_b, U = HbyA + rAU*rec, K = 0.5 magSqr(U), p = p_rgh + rho*gh + pRef (the rho that comes in), dpdt = rDeltaT*(p - p0),
 *   then ffm_fvc_rho_eqn from phi_f / phi_b and rho0 into rho.  HbyA, U: three device pointers.  upper and lower may be one array.
 * ffm_ue_buoyancy_source3: ffm_ue_buoyancy_flux + ffm_fvc_reconstruct (patch part t_b) + ffm_fvm_add_boundary per component with the
 *   reconstructed vector as the explicit source: diagOut_c = diag + sum ic_c, sourceOut_c = source_c + sum bc_c + V*rec_c.
 * The two cell passes return FFM_ERR_UNSUPPORTED, nothing launched, on meshes with more than 8 lower or upper neighbours per cell. */
int ffm_pc_face_fluxes(ffm_mesh *m, const double *rhorAU, const double *ghf, const double *rho, const double *vx, const double *vy,
                       const double *vz, const double *ddtCorr, double *rhorAUf, double *phig, double *phiHbyA);
int ffm_pc_finish(ffm_mesh *m, double rDeltaT, double pRef, const double *upper, const double *lower, const double *p_rgh,
                  const double *phiHbyA, const double *phig, const double *rhorAUf, const double *phi_b, const double *t_b,
                  const double *rAU, const double *const *HbyA, const double *gh, const double *p0, const double *rho0,
                  double *phi_f, double *const *U, double *K, double *p, double *dpdt, double *rho);
int ffm_ue_buoyancy_source3(ffm_mesh *m, const double *ghf, const double *rho, const double *p_rgh, const double *t_b,
                            const double *const *internalCoeffs, const double *const *boundaryCoeffs, const double *diag,
                            const double *const *source, double *const *diagOut, double *const *sourceOut);
/* fvc::flux(rho*v) on the internal faces (solver/pEqn.H:15 fvc::flux(rho*HbyA); the old-time flux of fvc::ddtCorr) without
 * storing the product fields; bitwise equal to ffm_fvc_flux of the products */
int ffm_fvc_flux_rho(ffm_mesh *m, const double *rho, const double *vx, const double *vy, const double *vz, double *out_f);
/* fvc::ddtCorr(rho, U, phi) of solver/pEqn.H:13 on the internal faces in one pass: coeff*rDeltaT*(phi0 - fvc::flux(rho0*U0)) with
 * ddtCouplingCoeff's coeff = 1 - min(|phi0 - flux|/(|phi0| + SMALL), 1); bitwise equal to ffm_fvc_flux_rho + that face algebra */
int ffm_fvc_ddt_corr(ffm_mesh *m, double rDeltaT, const double *rho0, const double *vx0, const double *vy0, const double *vz0,
                     const double *phi0_f, double *out_f);
/* solver/pEqn.H:1-3 on a single block: rho = psi*p, rAU = 1/UEqn.A(), rhorAU = rho*rAU in the pass of ffm_fvm_A */
int ffm_fvm_rAU(ffm_mesh *m, int nCmpt, const double *diag, const double *ic0, const double *ic1, const double *ic2,
                const double *psi, const double *p, double *rho, double *rAU, double *rhorAU);
/* solver/rhoEqn.H: fvm::ddt(rho) + fvc::div(phi) == 0 solved on the owned cells, rho = (rDeltaT*rho0*V - V*div(phi))/(rDeltaT*V);
 * bitwise equal to ffm_fvc_surface_integrate + that cell algebra.  rho and rho0 are different arrays. */
int ffm_fvc_rho_eqn(ffm_mesh *m, double rDeltaT, const double *phi_f, const double *phi_b, const double *rho0, double *rho);
/* the explicit terms of EEqn (solver/YEEqn.H:89-101) on the owned cells in one pass: divK = fvc::div(phi, K) [scheme 2 limitedLinear k |
 * 3 limitedLinear01 k in [lo,hi]; gx, gy, gz = fvc::grad(K)], ddtK = rDeltaT*(rho*K - rho0*K0), negDpdt = -dpdt.  Bitwise equal to
 * ffm_fv_limited_weights + ffm_fvc_interpolate + the product with phi + ffm_fvc_surface_integrate + the cell algebra.
 * FFM_ERR_UNSUPPORTED, nothing launched, on meshes with more than 8 lower or upper neighbours per cell (ffm_fvc_rho_eqn: 16). */
int ffm_fvc_div_phiK_terms(ffm_mesh *m, int scheme, double k, double lo, double hi, double rDeltaT, const double *phi_f,
                           const double *phi_b, const double *K, const double *K_b, const double *gx, const double *gy,
                           const double *gz, const double *rho, const double *rho0, const double *K0, const double *dpdt,
                           double *divK, double *ddtK, double *negDpdt);
int ffm_fvm_flux(ffm_mesh *m, const double *upper, const double *lower, const double *internalCoeffs,
                 const double *boundaryCoeffs, const double *psi, double *out_f, double *out_b);

/* ------------------------------------------------------- fused assembly passes */
/* The entry points above evaluate one operator per pass, like OpenFOAM's tmp-field algebra (and like the Foam layer of
 * include/ffmFoam.H calls them).  These produce the same numbers, bit for bit, in one pass per equation and for up to 4
 * fields that share the flux / density / diffusivity per launch (the species loop of solver/YEEqn.H:37-67); the compiled
 * time step (ffm_plume_step) is built on them.  Arrays of nf device pointers are HOST arrays.                          */
/* fvc::grad (Gauss linear) of nf <= 4 fields */
int ffm_fvc_grad_multi(ffm_mesh *m, int nf, const double *const *vf, const double *const *vb, double *const *gx,
                       double *const *gy, double *const *gz);
/* per field i: fvm::ddt(rho,vf_i) + fvm::div(phi,vf_i) [scheme 2 limitedLinear k | 3 limitedLinear01 k in [lo,hi], limiter from
 * vf_i and its gradient] - fvm::laplacian(gamma,vf_i) == su_i + su2_i - fvm::Sp(sp_i, vf_i) (each nullable: a NULL array or a NULL
 * entry), minus the explicit volume terms expl3[3*i+0..2] (all three or none; NULL array: none), with the boundary coefficients
 * of the mixed condition (f_i, ref_i, refGrad_i) added:
 * diag_i, upper_i, lower_i, source_i are what fvMatrix::solveSegregated hands to the linear solver                       */
int ffm_fvm_scalar_transport_multi(ffm_mesh *m, int nf, int scheme, double k, double lo, double hi, double rDeltaT,
                                   const double *rho, const double *rho0, const double *phi_f, const double *phi_b,
                                   const double *gamma_f, const double *gamma_b,
                                   const double *const *vf, const double *const *gx, const double *const *gy,
                                   const double *const *gz, const double *const *vf0, const double *const *f,
                                   const double *const *ref, const double *const *refGrad, const double *const *su,
                                   const double *const *su2, const double *const *sp,
                                   const double *const *expl3, double *const *diag, double *const *upper,
                                   double *const *lower, double *const *source);
/* the same pass with the face weights given (a multivariateSelection scheme's common weights: ffm_fv_multivariate_weights) instead of
 * one limiter per field -- what mvConvection->fvmDiv(phi, Yi) of solver/YEEqn.H:44 assembles.  With common weights and one gamma every
 * field has the SAME off-diagonal coefficients: upper[i] = lower[i] = NULL for the fields i >= n0 (n0 = 0 .. nf) leaves them unwritten,
 * the caller solves those systems with the arrays of an earlier field (ffm_ldu_bind_coeffs_native_d with offDiagUnchanged).
 * nf <= 4; ffm_fvm_scalar_transport_multi_ws with suFactor given also takes nf = 5 (the four species and h). */
int ffm_fvm_scalar_transport_multi_w(ffm_mesh *m, int nf, const double *w_f, double rDeltaT, const double *rho, const double *rho0,
                                     const double *phi_f, const double *phi_b, const double *gamma_f, const double *gamma_b,
                                     const double *const *vf0, const double *const *f, const double *const *ref,
                                     const double *const *refGrad, const double *const *su, const double *const *su2,
                                     const double *const *sp, const double *const *expl3, double *const *diag,
                                     double *const *upper, double *const *lower, double *const *source);
/* ffm_fvm_scalar_transport_multi_w with the explicit source of field i given as suFactor[i]*su[i] (suFactor: HOST array of nf factors,
 * NULL: 1): the species of solver/YEEqn.H:37-67 share one reaction rate; bitwise equal to handing in the products */
int ffm_fvm_scalar_transport_multi_ws(ffm_mesh *m, int nf, const double *w_f, double rDeltaT, const double *rho, const double *rho0,
                                      const double *phi_f, const double *phi_b, const double *gamma_f, const double *gamma_b,
                                      const double *const *vf0, const double *const *f, const double *const *ref,
                                      const double *const *refGrad, const double *const *su, const double *suFactor,
                                      const double *const *su2, const double *const *sp, const double *const *expl3,
                                      double *const *diag, double *const *upper, double *const *lower, double *const *source);
/* its *_direct form (see ffm_fvm_transport_scheme_direct) for the forms the time step uses: nf = 4 or 5 fields with suFactor given that
 * share one set of off-diagonals, upper[0] / lower[0] non-NULL and different, all others NULL (anything else: FFM_ERR_UNSUPPORTED) */
int ffm_fvm_scalar_transport_multi_ws_direct(ffm_mesh *m, int nf, const double *w_f, double rDeltaT, const double *rho, const double *rho0,
                                             const double *phi_f, const double *phi_b, const double *gamma_f, const double *gamma_b,
                                             const double *const *vf0, const double *const *f, const double *const *ref,
                                             const double *const *refGrad, const double *const *su, const double *suFactor,
                                             const double *const *su2, const double *const *sp, const double *const *expl3,
                                             double *const *diag, double *const *upper, double *const *lower, double *const *source);
/* momentum source of solver/UEqn.H:5 with `div(phi,U) Gauss LUST grad(U)`: source_c = rDeltaT*rho0*U0_c*V
 * - V*fvc::surfaceIntegrate(phi*LUST::correction(U_c)) for the three components from their gradients                  */
int ffm_fvm_lust_source3(ffm_mesh *m, double rDeltaT, const double *phi_f, const double *rho0, const double *const *U0,
                         const double *const *gx, const double *const *gy, const double *const *gz, double *const *source);

/* ------------------------------------------------------- fvDOM wall condition (N1) */
/* greyDiffusiveRadiationMixedFvPatchScalarField::updateCoeffs (reference packages/thermophysicalModels/radiation/derivedFvPatchFields/
 * greyDiffusiveRadiation/greyDiffusiveRadiationMixedFvPatchScalarField.C:150-230) of ray `ray` on every boundary face: with n the face
 * normal, nAve = n & dAve and Iw the ray's stored patch values,
 *   qr[ray] = Iw nAve;  Ir = sum over the rays of their qin (this ray's own, reset by radiativeIntensityRay::correct, counts 0);
 *   faces the ray leaves the wall through ((-n & d) > 0): valueFraction 1, refValue (Ir (1 - e) + e sigma T_b^4)/pi, qem[ray] = refValue nAve, qin[ray] = 0
 *   the others: valueFraction 0 (zeroGradient), qem[ray] = 0, qin[ray] = Iw nAve.
 * qin_all / qem_all / qr_all: device arrays [nRay][nBoundary] the rays share; emissivity_b NULL = 1 everywhere.  The iteration of
 * fvDOM::calculate (fvDOM/fvDOM.C:547-584) is host code above this (include/fireFoamHandles.H: fvDOM::correct).               */
int ffm_fvdom_wall_coeffs_d(ffm_mesh *mesh, int nRay, int ray, const double *d3, const double *dAve3, double sigma, const double *Iw_b,
                            const double *emissivity_b, const double *T_b, double *qin_all, double *qem_all, double *qr_all,
                            double *valueFraction_b, double *refValue_b);
/* fvDOM::updateG, boundary fluxes (fvDOM.C:740-750): out_b[k] = sum over the rays, in ray order, of all[ray][k] */
int ffm_fvdom_sum_rays_d(ffm_mesh *mesh, int nRay, const double *all, double *out_b);
/* The system of ONE ray with `div(Ji,Ii_h) Gauss upwind` in one pass (radiativeIntensityRay.C:267-322):
 *   fvm::div(Ji, Ii) + fvm::Sp(absorption omega, Ii) == omega/pi (absorption sigma T^4 [+ E/4]),  Ji = dAve & Sf,
 * inflow boundary faces at ref_b, outflow faces zero-gradient, boundary coefficients added: upper / lower [native faces], diag /
 * source [cells] are what the solver takes.  Bit for bit what the chain Ji and upwind weights -> ffm_fvm_transport ->
 * ffm_fvm_boundary_coeffs -> absorption and source -> ffm_fvm_add_boundary gives.  E (the emission), J_f, w_f (Ji and the
 * weights, should the caller want them) may be NULL.                                                                        */
int ffm_fvdom_ray_assemble_d(ffm_mesh *mesh, const double *dAve3, double omega, double absorption, double sigma, const double *T,
                             const double *E, const double *ref_b, double *J_f, double *w_f, double *upper, double *lower,
                             double *diag, double *source);
/* radiation->Sh(thermo, he) of solver/YEEqn.H:101 as one streaming pass over n cells (radiationModel.C:229-244; fvDOM/fvDOM.C:588 Rp, :612 Ru;
 * E = radFraction*Qdot of constRadFractionEmission::ECont): with Rp = 4 absorption sigma, Ru = absorption G - radFraction*Qdot,
 * T3 = T*T*T and Cp = Cp_d[c] where Cp_d is given, CpConst where it is NULL,
 *   sp = 4.0*Rp*T3/Cp          (the coefficient of fvm::Sp(., he))
 *   su = Ru - Rp*T3*(T - 4.0*he/Cp)
 * in exactly this operation order (oracle/plume.py:464-468), no FMA contraction.  Reads and writes the first n entries of every
 * array and nothing else; n == 0 is a no-op.  FFM_ERR_ARG: a NULL context or array (Cp_d excepted), n < 0. */
int ffm_radiation_sh_d(ffm_ctx *ctx, long n, double absorption, double sigma, double radFraction, const double *G_d, const double *T_d,
                       const double *he_d, const double *Qdot_d, const double *Cp_d /* nullable */, double CpConst, double *su_d,
                       double *sp_d);
/* The field forms of the two passes above, for an absorptionEmissionModel whose a, e and E are cell fields (greyMeanAbsorptionEmission
 * below; the P1 entry points already take such fields).
 * ffm_fvdom_ray_assemble_v_d: ffm_fvdom_ray_assemble_d -- the same kernel, a template switch -- with a_d[c]*omega and a_d[c]*sigma per
 *   cell in place of the host-formed absorption*omega and absorption*sigma.  With a_d[c] == x everywhere it writes bit for bit what the
 *   scalar form writes for absorption = x, and for any a_d the bits of the operator chain with V[c]*(a[c]*omega) and (a[c]*sigma)*T^4.
 * ffm_radiation_sh_v_d: Rp = 4.0*e*sigma, Ru = a*G - E per cell, then sp and su exactly as ffm_radiation_sh_d; a_d and e_d may be the
 *   same array.  Uniform a = e = x and E = radFraction*Qdot give the scalar form's bits.  FFM_ERR_ARG (nothing written): a NULL
 *   context or array (Cp_d excepted), n < 0; n == 0 is a no-op. */
int ffm_fvdom_ray_assemble_v_d(ffm_mesh *mesh, const double *dAve3, double omega, const double *a_d, double sigma, const double *T,
                               const double *E, const double *ref_b, double *J_f, double *w_f, double *upper, double *lower,
                               double *diag, double *source);
int ffm_radiation_sh_v_d(ffm_ctx *ctx, long n, const double *a_d, const double *e_d, double sigma, const double *E_d, const double *G_d,
                         const double *T_d, const double *he_d, const double *Cp_d /* nullable */, double CpConst, double *su_d,
                         double *sp_d);
/* fvDOM::updateG, cell part (fvDOM/fvDOM.C:697-718): G[c] = ((0 + I_0[c] omega_0) + I_1[c] omega_1) + ... in ray-index order,
 * accumulated in a register: every ray is read once and G written once -- bitwise what nRay passes G = G + I_i*omega_i over a zeroed
 * G leave.  I_dd: DEVICE array of nRay device pointers, omega_d: device [nRay].  Any nRay >= 1; n == 0 is a no-op.  FFM_ERR_ARG: a
 * NULL argument, n < 0, nRay < 1. */
int ffm_fvdom_G_d(ffm_ctx *ctx, long n, int nRay, const double *const *I_dd, const double *omega_d, double *G_d);
/* One block of a decomposed mesh, a ray whose upstream neighbour blocks are done: for the owned cells cells[nCells] that have a
 * face towards a ghost cell g, source -= upper[face] I[g] in the row's face order, then both coefficients of the face are set to
 * 0 -- the inflow from the neighbour ranks becomes a known term and the rows couple owned cells only.                         */
int ffm_fvdom_fold_ghost_inflow_d(ffm_mesh *mesh, int nCells, const int *cells_d, const double *I, double *upper, double *lower,
                                  double *source);
/* ------------------------------------------------------- P1 radiation model */
/* P1::calculate() (reference packages/thermophysicalModels/radiation/radiationModels/P1/P1.C:213-258; selected by
 * cases/pyrolysis1D/constant/radiationProperties:21, solved with the `G` entry of cases/steckler/system/fvSolution:75-81):
 *   gamma = 1.0/(3.0*a + 3.0*sigmaEff + a0);  solve(fvm::laplacian(gamma, G) - fvm::Sp(a, G) == -4.0*(e*sigma*pow4(T)) - E)
 * with sigmaEff = sigma_s*(3 - C) of constantScatter.C:87 and a0 = ROOTVSMALL = 1e-150 (upstream OpenFOAM's, restated from knowledge),
 * every patch MarshakRadiation (cases/pyrolysis1D/0/G; MarshakRadiationFvPatchScalarField.C:156-190), and qr_b = -gamma_b*snGrad(G)_b.
 * Operation order everywhere: pow4(x) = (x*x)*(x*x); the denominator (3.0*a + 3.0*sigmaEff) + a0; no FMA contraction.
 * All pointers are device pointers; `_b` arrays hold ffm_mesh_nboundary entries, face arrays are in the native layout.
 *
 * gamma_d[i] = 1.0/((3.0*a + 3.0*sigmaEff) + a0), a = a_d[i] or aConst where a_d is NULL: cells (P1.C:219-226) and patch values alike.
 * FFM_ERR_ARG: NULL ctx or gamma_d, n < 0; n == 0 is a no-op. */
int ffm_p1_gamma_d(ffm_ctx *ctx, long n, const double *a_d /* nullable */, double aConst, double sigmaEff, double *gamma_d);
/* MarshakRadiationFvPatchScalarField::updateCoeffs on every boundary face: refValue = (4.0*sigma)*pow4(T_b), refGrad = 0 (not written),
 * Ep = emissivity/(2.0*(2.0 - emissivity)), valueFraction = 1.0/(1.0 + (gamma_b*deltaCoeffs)/Ep).  emissivity 0 gives Ep = 0, the quotient
 * +inf and the fraction exactly 0 (a reflecting, zero-gradient wall): IEEE arithmetic, not guarded.  emissivity_b NULL = 1 everywhere.
 * A mesh without boundary faces: no-op.  FFM_ERR_ARG (nothing written): NULL mesh or any other array. */
int ffm_p1_marshak_coeffs_d(ffm_mesh *mesh, double sigma, const double *gamma_b, const double *T_b, const double *emissivity_b /* nullable */,
                            double *valueFraction_b, double *refValue_b);
/* The whole system of P1::calculate() as the solver takes it (symmetric: upper [native faces], diag / source [cells], boundary
 * coefficients added) in one walk over the rows, with the Marshak coefficients and gamma_b it formed on the way.  Bit for bit the chain
 *   ffm_p1_gamma_d (cells; patches -> gamma_b) | ffm_fvc_interpolate (NULL weights) | ffm_fvm_transport (gamma_f alone, laplacianSign +1) |
 *   ffm_p1_marshak_coeffs_d | ffm_fvm_boundary_coeffs(NULL, gamma_b, +1, f, ref, 0) | diag -= V*a |
 *   source = 0 + V*((-(4.0*((e*sigma)*pow4(T)))) - E) (fvMatrix == volField: source += V*su) | ffm_fvm_add_boundary.
 * a_d / e_d NULL: the constants; a_b NULL: aConst on the patches; E_d NULL: no emission term.
 * FFM_ERR_ARG (nothing written): NULL mesh, T_d, upper, diag or source, or -- on a mesh with boundary faces -- T_b or an output _b array. */
int ffm_p1_assemble_d(ffm_mesh *mesh, double sigmaEff, double sigma, const double *a_d /* nullable */, double aConst,
                      const double *a_b /* nullable */, const double *e_d /* nullable */, double eConst, const double *E_d /* nullable */,
                      const double *T_d, const double *T_b, const double *emissivity_b /* nullable */, double *upper, double *diag, double *source,
                      double *gamma_b, double *valueFraction_b, double *refValue_b);
/* After the solve: the mixed evaluate of G on the patches and the wall flux of P1.C:251-257,
 *   G_b = f*ref + (1 - f)*(G[faceCell] + 0/delta);  qr_b = -gamma_b*(delta*(G_b - G[faceCell])),
 * bit for bit ffm_bc_values (refGrad 0) + ffm_fvc_snGrad_b + one multiply.  A mesh without boundary faces: no-op.
 * FFM_ERR_ARG (nothing written): any NULL argument. */
int ffm_p1_wall_flux_d(ffm_mesh *mesh, const double *gamma_b, const double *valueFraction_b, const double *refValue_b, const double *G_d,
                       double *G_b, double *qr_b);
/* The tick schedule of the direction-ordered ray solves on a px x py x pz box of blocks, for the block (bx,by,bz); pure host
 * code, no GPU.  Rays are grouped by octant (ffm_ray_octant); a block's stage in an octant is its Manhattan distance from the
 * octant's upstream corner block; at tick t of an octant the block at stage s solves the octant's ray number t - s (rays of an
 * octant in ray-index order); an octant with r > 0 rays on a grid with S = px + py + pz - 2 stages takes r + S - 1 ticks, one
 * without rays none; octants follow one another in index order.  tickRay[t], t < min(cap, ticks) = the ray this block solves in
 * tick t or -1.  Returns the total tick count -- the same for every block -- or a negative ffm_status (tickRay may be NULL
 * with cap 0 to ask for the count).  Every upstream face neighbour of a block solves a ray exactly one tick before the block. */
int ffm_ray_schedule(int px, int py, int pz, int bx, int by, int bz, int nRay, const double *dAve, int *tickRay, int cap);
/* octant index 0..7 of a direction: bit a set where component a is negative; +0.0 and -0.0 count as positive, the sign rule of
 * the upwind weights (w = 1 where d & Sf >= 0)                                                                               */
int ffm_ray_octant(const double *d3);
/* psi = A^-1 source for a bound matrix that is triangular in the library's cell order, as one calcReciprocalD + one DILU
 * application (the forward / backward substitution in face order) on THIS rank's rows: no ghost refresh, no sum over ranks.
 * Faces towards ghost cells must carry zero coefficients.  out: nIterations 1, the normalised residuals of the start value and
 * of the result over this rank's rows; converged = 1 only where sum |source - A psi| <= 1e-10 sum |source|, i.e. where the
 * substitution was the solve (0: the matrix is not triangular in this order).  Vectors in the library's cell order.           */
int ffm_solve_triangular_rows_d(ffm_ldu *ldu, double *psi_d, const double *source_d, ffm_perf *out);

/* ------------------------------------------------------- flow-ordered exact solve (N1) */
/* The dependency order of a matrix with at most one non-zero off-diagonal coefficient per face -- an upwind ray equation
 * fvm::div(Ji, Ii) + fvm::Sp(k omega, Ii) (radiativeIntensityRay.C:267-322; `upwind`, or `linearUpwind`, whose implicit part is
 * upwind) on any mesh.  Row upperAddr[f] needs cell lowerAddr[f] where lower[f] != 0, row lowerAddr[f] needs cell upperAddr[f]
 * where upper[f] != 0; a face with two zeros is no edge.  order[nCells]: the cells level-major (level = longest dependency
 * path, level 0 first, ascending cell index inside a level); under it the matrix is triangular.  Pure host code, O(cells +
 * faces).  FFM_ERR_UNSUPPORTED (and a message) where the non-zero entries form a cycle; a face with two non-zero coefficients
 * is one.                                                                                                                   */
int ffm_flow_levels(int nCells, int nFaces, const int *lowerAddr, const int *upperAddr, const double *upper, const double *lower,
                    int *order /* [nCells] */, int *nLevels);
/* The same order of the coefficients the matrix holds now (set or bound), kept on the device: int[nCells], 4 nCells bytes per
 * order.  Creating one downloads the off-diagonal coefficients once (set-up cost, like an agglomeration).  Single rank: a
 * matrix with ghost cells, processor interfaces or a ghost exchange is refused (FFM_ERR_UNSUPPORTED), as is a cyclic one.
 * This is the staged order below in the case of no ghost cells and one stage [0, nCells): one algorithm, and the single-rank
 * entry points (this one, ffm_solve_ordered_d) are the ones that never communicate, also on a rank of several.  An order
 * belongs to the entry point that made it: handed to the other kind's solve it is refused like another matrix's order.      */
typedef struct ffm_flow_order ffm_flow_order;
int ffm_flow_order_create(ffm_ldu *ldu, ffm_flow_order **out);
int ffm_flow_order_nlevels(const ffm_flow_order *o);
int ffm_flow_order_destroy(ffm_flow_order *o);
/* psi = A^-1 source as ONE forward substitution in that order: per row, source minus the lower faces' then the upper faces'
 * terms in face order (zero coefficients skipped), one division -- bit for bit the serial loop, whatever the matrix's sweep
 * mode.  Before anything else a pass over the rows checks the order against the coefficients the matrix holds NOW: if the
 * column of some non-zero entry does not stand earlier than its row (a stale order, another matrix's order, a cycle) the call
 * returns FFM_ERR_UNSUPPORTED and psi_d is untouched.  out: nIterations 1, OpenFOAM's normalised residuals of the start value
 * and of the result; converged = 1 only where sum |source - A psi| <= 1e-10 sum |source| (the rule of
 * ffm_solve_triangular_rows_d).  Vectors in the caller's cell numbering: where the library renumbered the cells
 * (ffm_ldu_is_native_order() == 0) they go through the permutation the other solvers use.  Single rank only: the one-stage
 * case of ffm_solve_ordered_staged_d, without its all-reduces and exchanges, the norms taken over this rank's rows.  An order of
 * another matrix (another context or size, or one made by ffm_flow_order_create_staged) is refused with FFM_ERR_UNSUPPORTED
 * before anything is launched; *out is zeroed before an order is refused, as in the staged call.                            */
int ffm_solve_ordered_d(ffm_ldu *ldu, const ffm_flow_order *o, double *psi_d, const double *source_d, ffm_perf *out);

/* ------------------------------------------------------- flow-ordered exact solve on a decomposed mesh, any partition */
/* The ranks' dependency graph of a ray is cyclic on general partitions (rank A feeds B across one cut face, B feeds A across
 * another); the cells' is not.  So every cell gets a STAGE: the largest number of rank crossings on any upstream path to it.
 * The rows of stage s need owned cells of stage <= s and ghost cells of stage < s, so a rank solves its stage-s rows exactly in
 * one sweep, all ranks exchange ghost values once, and stage s + 1 follows.
 * ffm_flow_stages is one rank's share of that analysis: pure host code, no GPU, no communication.  The rank's sub-domain in the
 * form of ffm_ldu_create_ext: cells [0, nOwned) have rows, cells [nOwned, nOwned + nGhost) are ghost cells, sources whose stage
 * on their own rank is ghostStage[].  Edges as in ffm_flow_levels, rows for owned cells only.  stage[c] = max over the cells u
 * row c needs of stage[u] (u owned) or ghostStage[u - nOwned] + 1 (u a ghost cell); 0 without any.  order[nOwned]: the owned
 * cells stage-major, inside a stage level-major by the levels of ffm_flow_levels on the owned sub-graph (ascending cell index
 * inside a level): every non-zero owned column stands before its row.  nLevels: the level count of the owned sub-graph.
 * FFM_ERR_UNSUPPORTED where the non-zero entries form a cycle among the owned cells (a cycle through several ranks is not
 * visible to one of them: ffm_flow_order_create_staged).                                                                    */
int ffm_flow_stages(int nOwned, int nGhost, int nFaces, const int *lowerAddr, const int *upperAddr, const double *upper, const double *lower,
                    const int *ghostStage /* [nGhost] */, int *stage /* [nOwned] */, int *order /* [nOwned] */, int *nLevels);
/* COLLECTIVE: every rank of the communicator calls it, for a matrix with ghost cells and a ghost exchange (ffm_ldu_create_ext +
 * ffm_ldu_set_ghost_exchange; no processor interfaces).  The staged order of the coefficients the matrix holds now as the least
 * fixpoint over the ranks: all ghost stages 0, ffm_flow_stages, one ghost exchange of the stages, one all-reduce of "some ghost
 * stage changed", until none did -- at most (stage count + 1) rounds, every rank the same number.  A stage above the number of
 * ghost cells of all ranks is a cycle through several ranks; that, and a failure on any one rank (a cycle among its own cells,
 * out of memory), makes EVERY rank return an error (FFM_ERR_UNSUPPORTED for the cycles), none leaves while another waits.
 * The order keeps order[nOwned], stage[nOwned] and ghostStage[nGhost] on the device.  A matrix without a ghost exchange is
 * refused (ffm_flow_order_create is the single-rank entry point), except the rank of a larger communicator that has no
 * neighbour.  ffm_flow_order_nlevels: the levels of this rank's owned sub-graph; ffm_flow_order_destroy as for any order.    */
int ffm_flow_order_create_staged(ffm_ldu *ldu, ffm_flow_order **out);
/* the stage count over all ranks, the same on every rank (0 for an order of ffm_flow_order_create): a solve costs one sweep
 * launch per stage on every rank and (stage count - 1) ghost exchanges -- 2 to 5 on RCB-like partitions of the test meshes,
 * tens to hundreds on the jagged ones of graph growing (README.md)                                                          */
int ffm_flow_order_nstages(const ffm_flow_order *o);
/* COLLECTIVE.  psi = A^-1 source over all ranks, stage by stage: per stage one sweep of this rank's rows of that stage (no
 * launch where it has none) -- a row as in ffm_solve_ordered_d: source minus the lower faces' then the upper faces' terms in the
 * rank's own face order, zero coefficients skipped, ghost columns read from psi's ghost entries, one division -- and after every
 * stage but the last one ghost refresh of psi, entered by every rank.  First of all the order is checked against the
 * coefficients the matrix holds NOW (every non-zero owned column earlier in the order and of a stage <= the row's, every
 * non-zero ghost column of a stage < the row's) and the failure count is all-reduced with the stage counts: if any row on any
 * rank fails, or the ranks' orders differ in their stage count, ALL ranks return FFM_ERR_UNSUPPORTED with psi_d untouched,
 * before any sweep or exchange (so does an order made by ffm_flow_order_create).  out: nIterations 1; OpenFOAM's normalised residuals of the start value and of the result and
 * converged (the rule of ffm_solve_ordered_d) with the sums over all ranks, the same on every rank.  A sweep that timed out on
 * any rank makes all ranks return FFM_ERR_HIP.  Vectors in the caller's numbering, owned + ghost entries; on return psi's ghost
 * entries hold the neighbour ranks' results.                                                                              */
int ffm_solve_ordered_staged_d(ffm_ldu *ldu, const ffm_flow_order *o, double *psi_d, const double *source_d, ffm_perf *out);

/* ------------------------------------------------------- synthetic plume case */
/* Host-side driver (C++ over the entry points above) of one fireFoam time step on
 * the synthetic buoyant-plume box of SURVEY 8(d): rhoEqn, UEqn, YEEqn, 2 x pEqn in
 * the order of solver/fireFoam.C:97-119.  bench.py's workload.                */
typedef struct ffm_plume ffm_plume;
typedef struct ffm_thermo ffm_thermo;      /* the thermo package below (ffm_thermo_create): ffm_plume_set_thermo borrows one */
typedef struct ffm_greymean ffm_greymean;  /* greyMeanAbsorptionEmission below (ffm_greymean_create): ffm_plume_set_absorption_emission borrows one */
int ffm_plume_create(ffm_ctx *ctx, int nx, int ny, int nz, double h, double deltaT, ffm_plume **out);
/* one rank's block [lo,hi) of the global box; nbrRank[6] = rank across the -x,+x,-y,+y,-z,+z side or -1
 * (physical boundary).  Needs ffm_comm_init / ffm_comm_init_host when any neighbour exists.            */
int ffm_plume_create_block(ffm_ctx *ctx, int gx, int gy, int gz, const int *lo, const int *hi,
                           const int *nbrRank, double h, double deltaT, ffm_plume **out);
int ffm_plume_destroy(ffm_plume *p);
int ffm_plume_step(ffm_plume *p);
/* tests: run every linear solve to 1e-13 with relTol 0 instead of the fvSolution controls */
int ffm_plume_set_tight(ffm_plume *p, int on);
/* linear solvers of the transport equations (U, Yi, h): 0 = PBiCGStab + DILU (default, the kernels BASELINE names),
 * 1 = smoothSolver + symGaussSeidel with maxIter 10, the selection of cases/steckler/system/fvSolution:49-62 */
int ffm_plume_set_solvers(ffm_plume *plume, int stecklerSelection);
/* The sub-grid model of the step: 0 none (default: constant mu and mu/Pr, as before), 1 the LES kEqn model with delta cubeRootVol that
 * every BASELINE case selects (cases/steckler/constant/turbulenceProperties:18-30).  With model 1
 *   UEqn   (solver/UEqn.H:7, turbulence->divDevRhoReff(U)): - fvm::laplacian(rho nuEff, U) - fvc::div(rho nuEff dev2(T(grad U))),
 *          rho nuEff = rho (nut + mu/rho);
 *   YEEqn  (solver/YEEqn.H:12, turbulence->alphaEff()): alpha + alphat for the species and h;
 *   turbulence->correct() after the second pressure corrector (solver/fireFoam.C:113-116): kEqn::correct -- ddt(rho,k) + div(phi,k)
 *          [limitedLinear 1] - laplacian(rho nuEff, k) == rho G - SuSp(2/3 rho divU, k) - Sp(Ce rho sqrt(k)/delta, k), solved by the
 *          selection and tolerance of h (one more solve-log entry "k" after the second p_rgh), bound(k, SMALL), correctNut():
 *          nut = Ck sqrt(k) delta, alphat = rho nut/Prt.
 * Patches: k fixed kInlet on the inlet, inletOutlet(kInlet) on top / sides, zeroGradient on the floor; nut and alphat zeroGradient,
 * 0 on the floor.  k0: host, the start value of k per owned cell in the cell order ffm_plume_set_initial_state takes its fields in
 * (a block's own natural order on a decomposed box), or NULL for kInlet everywhere.  Callable between steps (and after
 * ffm_plume_set_initial_state, which it does not follow); model 1 evaluates correctNut() once with the current rho, model 0 releases
 * the model's fields: the step is then the code and the launches of a handle that never had it.  FFM_ERR_ARG with the handle
 * unchanged: an unknown model, Ck < 0, Ce < 0, Prt <= 0, kInlet <= 0, a k0 entry that is not finite and positive.  Fields "k", "nut",
 * "alphat" become readable with ffm_plume_get_field while the model is on.  Parity of the plume with kEqn is unpinned by reference
 * data, as the plume itself is: the check is oracle/steckler_case.py's kEqn restated on the plume box (tests/plume_keqn_ref.py).  */
int ffm_plume_set_turbulence(ffm_plume *plume, int model /* 0 none (default), 1 kEqn */, double Ck, double Ce, double Prt, double kInlet,
                             const double *k0);
/* The thermo model of the step: NULL (default) the stand-in -- perfect gas with one constant Cp, T = Tref + h/Cp, constant mu and mu/Pr
 * -- or a handle of ffm_thermo_create: hePsiThermo<reactingMixture<sutherland<janaf<perfectGas<specie>>>>, sensibleEnthalpy>
 * (cases/steckler/constant/thermophysicalProperties:18-27).  With a handle
 *   thermo.correct() (solver/YEEqn.H:114 after the enthalpy solve; solver/phrghEqn.H inside the five hydrostatic correctors; at set-up):
 *          cell mixture by progressive mass-fraction sum, T by thermo::T's Newton iteration from the old T, psi, sutherland mu,
 *          modified-Eucken alpha and Cp at the new T, ghost cells included -- one pass (ffm_thermo_step_d).  "maximum number of
 *          iterations exceeded" is accumulated on the device and read at the synchronisation that closes the step (or the set-up):
 *          ffm_plume_step then returns FFM_ERR_ARG; the step has no further host synchronisation;
 *   UEqn   (solver/UEqn.H:7): laminar - fvm::laplacian(interpolate(mu), U); with kEqn rho nuEff = rho (nut + mu/rho), mu the cell field;
 *   YEEqn  (solver/YEEqn.H:12): alphaEff = alpha (+ alphat), one diffusivity for the species and h;
 *   inlet  h = Hs(inlet mixture, T_IN) by ffm_thermo_he_d's arithmetic on the inlet faces' species values, in place of Cp (T_IN - Tref);
 *          the inletOutlet value hAmb stays the caller's.
 * Patches: rho, psi, mu, alpha keep the plume's stand-in convention, zero-gradient copies of the cell values; the patch types of
 * heThermo (fixed T, mixedEnergy) stay with the class layer (include/fireFoamHandles.H).
 * The handle is BORROWED (created on the plume's context): it outlives the plume or is unset (NULL) first.  It must hold exactly the plume's five species in the
 * plume's order (O2, H2O, C3H8, CO2, N2; checked by count and molecular weight): anything else is FFM_ERR_ARG.  Allowed only while no
 * step has been taken since creation or ffm_plume_set_initial_state -- the hydrostatic start depends on psi -- otherwise FFM_ERR_ARG.
 * The call redoes the start-up from the Y and h the handle holds: T = Tref (the Newton start: thermo::T's result depends on it, a
 * restart must not inherit an old run's T), thermo.correct(), rho = psi p, the hydrostatic initialisation with the selected thermo in
 * its correctors; with kEqn on, correctNut() again with the new rho.  ffm_plume_set_initial_state on a handle with the model on does
 * the same: the two call orders give the same bytes.  Excludes ffm_plume_set_radiation* unless ffm_plume_set_radiation_thermo is on:
 * FFM_ERR_UNSUPPORTED in whichever order they are called.  A refused call leaves the handle unchanged.  Fields "mu", "alpha",
 * "Cp" become readable with ffm_plume_get_field while the model is on, and with them "wFuel", "Qdot" (the last step's, whichever
 * combustion model formed them; with neither model on they are scratch of the step and refused).  Unpinned by reference data, as the plume itself is: the check
 * is oracle/thermo.py's package restated on the plume box (tests/plume_thermo_ref.py). */
int ffm_plume_set_thermo(ffm_plume *plume, ffm_thermo *thermo /* NULL: the stand-in (default) */);
/* The combustion model of the step: 0 (default) the stand-in rate rho min(Yf, YO2/s)/tau, 1 the reference's eddyDissipationModel
 * (lib/thermophysicalModels/combustionModels/eddyDissipationModel/eddyDissipationModel.C:93-149; cases/steckler/constant/
 * combustionProperties: C_EDC 4, C_Diff 0, C_Stiff 1) at combustion->correct() of solver/YEEqn.H: ffm_edc_correct_d's expressions with the
 * step's deltaT, kEqn's Ce and delta (epsilon = Ce k sqrt(k)/delta) and the thermo model's alpha (mu/Pr with the stand-in thermo);
 * wFuel and Qdot = qFuel wFuel, readable as fields "wFuel", "Qdot".  s, qFuel: singleStepReactingMixture's; the species'
 * stoichiometric factors stay the plume's.  No patch values: the rate is a cell field.  Callable between steps.  Model 1 needs the
 * kEqn model (ffm_plume_set_turbulence) to be on: FFM_ERR_UNSUPPORTED without it, and ffm_plume_set_turbulence(.., 0, ..) is
 * refused the same way while model 1 is on.  FFM_ERR_ARG with the handle unchanged: an unknown model, a non-finite value, s <= 0,
 * C_Stiff <= 0, C_EDC < 0, C_Diff < 0, qFuel <= 0.  EDC with radiation on is as untested as kEqn with radiation is.  Unpinned by
 * reference data, as the plume itself is (tests/plume_thermo_ref.py restates oracle/steckler_case.py's edc_correct). */
int ffm_plume_set_combustion(ffm_plume *plume, int model /* 0 stand-in (default), 1 the reference's EDC */,
                             double C_EDC, double C_Diff, double C_Stiff, double s, double qFuel);
/* SURVEY 8(f) N1 stand-in: the reference's radiation->correct() (solver/YEEqn.H:80; fvDOM with nPhi 2, nTheta 4, solverFreq 100,
 * cases/steckler/constant/radiationProperties:32-40) as 4*nPhi*nTheta upwind ray-transport solves every `solverFreq` steps
 * (0 = off, the default).  dAve[3*nRay], omega[nRay]: the rays' mean directions and solid angles as fvDOM.C:55-90 builds
 * them, or both NULL to have them built from nPhi, nTheta.  Fields "G" and "I<n>" become readable with ffm_plume_get_field. */
int ffm_plume_set_radiation(ffm_plume *plume, int solverFreq, int nPhi, int nTheta, const double *dAve, const double *omega);
/* The reference's absorption / emission model for those rays and their coupling into the enthalpy equation:
 * constant absorption coefficient `absorption` [1/m] (constRadFractionEmission has aCont = 0: cases/steckler/constant/
 * radiationProperties:42; constantAbsorptionEmission: a) and the emission E = RadFraction*Qdot of lib/thermophysicalModels/
 * radiation/submodels/absorptionEmissionModel/constRadFractionEmission/constRadFractionEmission.C:ECont with radScaling:
 * RadFraction = max(min(Ehrr1, Ehrr2), (mlr1*Ehrr1 + mlr2*Ehrr2)/max(SMALL, mlr1 + mlr2)), mlr = -gSum(phi) of the burner patch
 * (cases/steckler: Ehrr1 0.5, Ehrr2 0.22).  Ray source omega/pi*(a sigma T^4 + E/4) (radiativeIntensityRay.C:286-300);
 * EEqn gets radiation->Sh(thermo, he) = Ru - fvm::Sp(4 Rp T^3/Cpv, he) - Rp T^3 (T - 4 he/Cpv), Rp = 4 a sigma, Ru = a G - E
 * (radiationModel.C:229-244; solver/YEEqn.H:101).  Without this call the rays keep the round-1 stand-in (a = 0.1, no E, no Sh). */
int ffm_plume_set_radiation_model(ffm_plume *plume, double absorption, double Ehrr1, double Ehrr2);
/* Opt-in (default 0): the fvDOM rays and radiation->Sh together with the thermo package of ffm_plume_set_thermo.  On, ffm_plume_set_thermo
 * and ffm_plume_set_radiation / _model / _ordering accept each other in either call order (ffm_plume_set_thermo keeps its own rules), and
 *   radiation->Sh(thermo, he) (solver/YEEqn.H:101) divides by thermo.Cpv(): the Cp field thermo.correct() wrote (ffm_radiation_sh_d with
 *          Cp_d), in the separate EEqn and where h is the fifth lock-step system;
 *   the rays (radiativeIntensityRay.C:267-322) read the package's T; E = RadFraction*Qdot with Qdot of the selected combustion model;
 *   RadFraction, the ambient black-body inflow and the zero-gradient outflow of the stand-in are unchanged; both orderings of a
 *          decomposed box run.
 * Off, the setters refuse each other as before.  With the switch on and the thermo package off the step is that of a handle that never
 * saw the switch.  Turning it off while the thermo package and any of ffm_plume_set_radiation* are on: FFM_ERR_UNSUPPORTED, the handle
 * unchanged.  "ShSu" / "ShSp" (ffm_plume_get_field) are the last radiation->Sh pass, an error before the first.  Unpinned by reference
 * data, as the plume itself is: the check is tests/plume_radiation_ref.py.
 * Not here: greyDiffusiveRadiation walls (they stay with the fvDOM handle of include/fireFoamHandles.H), a device-resident RadFraction,
 * wide-band models, rays pipelined against each other. */
int ffm_plume_set_radiation_thermo(ffm_plume *plume, int on);
/* Opt-in (solverFreq 0 = off, the default): the P1 model as the plume's radiation->correct() (solver/YEEqn.H:80) in place of the rays.
 * Every solverFreq-th step assembles the system of P1::calculate() (ffm_p1_assemble_d; the chain it restates under FFM_PLUME_UNFUSED, the
 * same bytes), solves G with PCG + DIC at the `G` entry's controls (tolerance 1e-6, relTol 0) from the previous G -- logged as "G" -- and
 * forms qr (ffm_p1_wall_flux_d).  One constant `absorption` for a and e, no scattering, E = RadFraction*Qdot and radiation->Sh exactly as
 * ffm_plume_set_radiation_model has them (Ehrr1, Ehrr2), every patch MarshakRadiation with the one `wallEmissivity` and the zero-gradient
 * patch values of T.  "G", "qr" ([nBoundary], patch-face order), "ShSu", "ShSp" are readable with ffm_plume_get_field.  Towards
 * ffm_plume_set_thermo the rules of ffm_plume_set_radiation_thermo hold.  FFM_ERR_UNSUPPORTED, the handle unchanged: the rays are on
 * (ffm_plume_set_radiation refuses likewise while P1 is on), or the handle is a block of a decomposed box.  FFM_ERR_ARG: negative arguments
 * or wallEmissivity outside [0, 1].  Unpinned by reference data: the reference ships no output of a P1 run; the check is tests/plume_p1_ref.py.
 * Not here: decomposed boxes, per-patch emissivities, MarshakRadiationFixedTemperature, coefficient models other than the constant. */
int ffm_plume_set_radiation_p1(ffm_plume *plume, int solverFreq, double absorption, double Ehrr1, double Ehrr2, double wallEmissivity);
/* greyMeanAbsorptionEmission (ffm_greymean_create below) as the step's absorptionEmissionModel, in place of the constant absorption
 * coefficient and of E = RadFraction*Qdot; gm NULL (the default): the constant again -- the step then issues exactly the launches of a
 * handle that never had the model.  The handle is borrowed, as ffm_plume_set_thermo's is.  Needs ffm_plume_set_radiation with
 * ffm_plume_set_radiation_model, or ffm_plume_set_radiation_p1, first (FFM_ERR_UNSUPPORTED otherwise); the model's species must be the
 * plume's five with the molecular weights of the selected thermo package, or the stand-in's (FFM_ERR_ARG).  With it on:
 *   radiation->correct() evaluates a once (ffm_greymean_a_d) and E = EhrrCoeff*Qdot (ffm_greymean_E_d); the RadFraction reduction over
 *     the burner patch and its host read-back drop out.  Every ray is assembled with the field (fused: ffm_fvdom_ray_assemble_v_d; per
 *     operator: the chain with V*(a*omega) and (a*sigma)*T^4 per cell); P1 passes a_d = e_d = a and its zero-gradient patch copy a_b to
 *     ffm_p1_assemble_d, and to the chain;
 *   radiation->Sh of EVERY step comes from ffm_radiation_sh_greymean_d (fused) or from ffm_greymean_a_d, ffm_greymean_E_d,
 *     ffm_radiation_sh_v_d (per operator): a is current every step, as Rp() / Ru() are upstream.  h keeps its separate EEqn in every
 *     step while the model is on, also in the steps without a correct() where it is otherwise the fifth lock-step system: Sh reads a
 *     of the species the Yi equations have just solved (solver/YEEqn.H:43-60 before :101), and five systems assembled together would
 *     give it the old ones.  Fused and per-operator steps are byte for byte equal.
 * Fields aRad (a of the last evaluation), ShSu, ShSp.  The temperature-range flag is read with the step's closing synchronisation; the
 * reference only warns (absorptionCoeffs::checkT), so the step prints a warning, leaves the text in ffm_last_error and goes on.
 * FFM_ERR_UNSUPPORTED with a message: a block of a decomposed box.  Unpinned by reference data (tests/plume_greymean_ref.py). */
int ffm_plume_set_absorption_emission(ffm_plume *plume, ffm_greymean *gm /* NULL: the constant, default */);
/* How the rays are solved on a block of a decomposed box.  0 (default): every ray is a block-Jacobi PBiCGStab + DILU solve over
 * all ranks.  1: the staged, direction-ordered sweep -- the ranks walk the ticks of ffm_ray_schedule; in a tick a rank assembles
 * at most one ray (ffm_fvdom_ray_assemble_d), moves the inflow from its upstream neighbours' ghost values into the source
 * (ffm_fvdom_fold_ghost_inflow_d) and solves its own, now triangular rows exactly (ffm_solve_triangular_rows_d; the solve is
 * logged as I<i> with 1 iteration); every tick ends with one ghost exchange entered by all ranks.  No other waiting between
 * ranks.  Needs the blocks of a box numbered x fastest (rank = bx + px (by + py bz), as ffm_plume_create_block's callers number
 * them): anything else is FFM_ERR_UNSUPPORTED, never a silent fall-back.  The plume's rays are always `Gauss upwind`.  On a
 * single block both modes are the direction-ordered solve.  Also read from FFM_PLUME_RADIATION_ORDERING at creation.           */
int ffm_plume_set_radiation_ordering(ffm_plume *plume, int mode);
/* tests: the system of one ray in the case's present state, assembled by the operator chain (fused 0) or by
 * ffm_fvdom_ray_assemble_d (fused 1): diag, source [owned cells, natural order], upper, lower [faces, the case's face order].
 * Overwrites the driver's matrix work arrays (what the next equation of a step assembles into anyway): call it between
 * ffm_plume_step calls only, never from inside one.                                                                          */
int ffm_plume_ray_system(ffm_plume *plume, int ray, int fused, double *diag, double *upper, double *lower, double *source);
/* tests: a start state and boundary values other than the quiescent ambient / pure-fuel inflow -- Y[5] and h as cell fields in
 * natural blockMesh order, Yamb / Yin the inletOutlet and inlet values of the species, hAmb the inletOutlet value of h; redoes
 * the hydrostatic initialisation (solver/phrghEqn.H).  Single block; after steps, a restart from time 0.                                  */
int ffm_plume_set_initial_state(ffm_plume *plume, const double *const *Y, const double *h, const double *Yamb, const double *Yin, double hAmb);
/* tests: the next step convects the species and h with the face weights w[F] (natural face order) instead of evaluating the
 * multivariateSelection limiter of solver/YEEqn.H:1-10 -- separates the limiter's conditioning from everything else in a step */
int ffm_plume_override_mv_weights(ffm_plume *plume, const double *w);
int ffm_plume_ncells(const ffm_plume *p);
int ffm_plume_nfaces(const ffm_plume *p);
int ffm_plume_get_field(ffm_plume *p, const char *name, double *out);
int ffm_plume_nsolves(const ffm_plume *p);
/* steps so far in which h was assembled and solved as the fifth system of the species (FFM_PLUME_SEPARATE_H=1: never)            */
int ffm_plume_joint_steps(const ffm_plume *p);
int ffm_plume_get_solve(const ffm_plume *p, int i, char *name16, ffm_perf *perf);
/* the case's raw state for a driver that runs the same case through another path (bench.py: the reference's equation files over the Foam
 * layer): cell fields [N] in the library's cell order, face fields [F] in the renumbered LDU face order, boundary arrays [B] in (patch, face)
 * order; returns the number of values or a negative FFM_ERR_*.  Names: rho p p_rgh h K dpdt gh Ux Uy Uz <specie> | phi ghf | phib ph_rgh_b kind
 * fStaticU<c> refU<c> fStaticS fStaticH refH refY<i> ghfB */
long ffm_plume_get_raw(ffm_plume *p, const char *name, double *out, long cap);
ffm_ldu *ffm_plume_ldu(ffm_plume *p);
ffm_mesh *ffm_plume_mesh(ffm_plume *p);          /* the case's device mesh (tests: operators on the tile-numbered mesh) */

/* ------------------------------------------------------- pyrolysis region (N3) */
/* reactingOneDim::evolveRegion (packages/regionModels/pyrolysisModels/reactingOneDim/reactingOneDim.C:686-721) for a panel of
 * nCol independent columns of nLay <= 16 layers (the region mesh extruded from a wall patch: cases/wallFireSpread2D/system/
 * extrudeToRegionMeshDict:17-39; cases/pyrolysis1D: one column, 8 layers): Arrhenius solid reaction, continuity, species and
 * the tridiagonal enthalpy equation of every column in one kernel, then solidThermo.correct().  Defaults: the solids and the
 * reaction of cases/pyrolysis1D/constant/panelRegion.  qSurf_d[nCol] (device): heat flux into the exposed face of every column
 * [W/m2] -- what the coupled wall conditions of lib/fvPatchFieldsPyrolysis hand over; the back face is adiabatic or held at Tback.
 * Out (device, [nCol]): the exposed cell's temperature and the pyrolysate mass flux phiGas [kg/s] of every column.            */
typedef struct ffm_pyro ffm_pyro;
int ffm_pyro_create(ffm_ctx *ctx, int nCol, int nLay, double thickness, double faceArea, double T0, double Yvirgin0, ffm_pyro **out);
int ffm_pyro_set_solids(ffm_pyro *p, const double *virgin /* rho Cp kappa Hf */, const double *charred);
int ffm_pyro_set_reaction(ffm_pyro *p, double A, double Ta, double Tcrit, double n);
int ffm_pyro_step(ffm_pyro *p, double deltaT, const double *qSurf_d, int backFixed, double Tback);
/* name: rho, Yw, T, h, alpha -> host [nCol][nLay]; Tsurf, phiGas, qSurf, Twall -> host [nCol] */
int ffm_pyro_get(ffm_pyro *p, const char *name, double *out);
const double *ffm_pyro_surface_T_d(const ffm_pyro *p);
const double *ffm_pyro_phiGas_d(const ffm_pyro *p);
/* The mapped patch conditions between the gas region's wall patch and the panel (lib/fvPatchFieldsPyrolysis), column i <->
 * gas boundary face map_d[i] (null: i).  Replaces turbulentTemperatureRadiationQinCoupledMixedFvPatchScalarField::updateCoeffs
 * (:176-292; solid side: qSurf = -(kappaDelta_gas (T_s,cell - T_g,cell) - a qin + e sigma T_w^4), wall value from refGrad;
 * gas side: refValue = T_s,cell, valueFraction 1 -> refT_d) and flowRateInletVelocityPyrolysisCoupledFvPatchVectorField::
 * updateCoeffs (:127-248; U_b = n (-phiGas hocPyr/qFuel/magSf)/rho_b -> Ux_d, Uy_d, Uz_d).  Gas-side arrays are indexed by
 * boundary face; only the mapped entries of the outputs are written.  ffm_pyro_qSurf_d is what ffm_pyro_step then takes. */
int ffm_pyro_couple_d(ffm_pyro *p, const int *map_d, const double *TgasCell_d, const double *kappaDelta_d, const double *qin_d,
                      double emissivity, double absorptivity, const double *rho_b_d, const double *magSf_d,
                      const double *nfx_d, const double *nfy_d, const double *nfz_d, double hocSolid, double qFuel,
                      double *refT_d, double *Ux_d, double *Uy_d, double *Uz_d);
const double *ffm_pyro_qSurf_d(const ffm_pyro *p);
/* Selections of the region's dictionaries.
 * ffm_pyro_set_model: reactingOneDim21 != 0 selects lib/regionModels/pyrolysisModels/reactingOneDim21/reactingOneDim21.C (solveEnergy
 *   :319-368: fvm::ddt(rho,h) - fvm::laplacian(alpha,h) + fvc::laplacian(alpha,h) - fvc::laplacian(kappa,T) == chemistryQdot +
 *   RRs(0) T Cp0 + RRs(1) T Cp1; evolveRegion :777-815), the pyrolysisModel of cases/wallFireSpread2D/constant/pyrolysisZones:23,
 *   instead of reactingOneDim (== chemistryQdot - fvm::Sp(RRg, h)); harmonicAlpha / harmonicKappa: `Gauss harmonic` instead of
 *   `Gauss linear` for laplacian(thermo:alpha,h) / laplacian(kappa,T) (system/panelRegion/fvSchemes of the two cases).
 * ffm_pyro_set_back: the back face of T -- 0 zeroGradient, 1 fixedValue Tinf, 2 constHTemperature (lib/fvPatchFields/
 *   constHTemperatureFvPatchScalarField/constHTemperatureFvPatchScalarField.C:156-180; cases/wallFireSpread2D/0/panelRegion/T:25-31).
 * ffm_pyro_set_surface_radiation: greyMeanSolidAbsorptionEmission (cases/wallFireSpread2D/constant/panelRegion/radiationProperties:
 *   19-31): absorptivity / emissivity of the exposed face = the solids' values weighted with their volume fractions in the exposed
 *   layer; used by ffm_pyro_evolve_d instead of its constants and handed to the gas side by ffm_pyro_gas_side_d.                      */
int ffm_pyro_set_model(ffm_pyro *p, int reactingOneDim21, int harmonicAlpha, int harmonicKappa);
int ffm_pyro_set_back(ffm_pyro *p, int mode, double h, double Tinf);
int ffm_pyro_set_surface_radiation(ffm_pyro *p, double absorptivityVirgin, double emissivityVirgin, double absorptivityChar, double emissivityChar);
/* pyrolysisModel::evolve() of one region with its exposed face coupled to the gas region (solver/fireFoam.C:90-93): evolveRegion with
 * the solid branch of turbulentTemperatureRadiationQinCoupledMixedFvPatchScalarField::updateCoeffs (:176-296) evaluated INSIDE the
 * step, where OpenFOAM evaluates it (construction of hEqn: old cell temperature, stored wall value, surface properties and
 * kappa(*this) of the composition after solveSpeciesMass); the wall value and qSurf of the step are stored.  Gas-side arrays
 * (cell temperature next to the wall, kappaEff*deltaCoeffs, incident radiation qin or NULL) are indexed by boundary face,
 * column i <-> face map_d[i] (NULL: i).  emissivity / absorptivity: constants used unless ffm_pyro_set_surface_radiation was called. */
int ffm_pyro_evolve_d(ffm_pyro *p, double deltaT, const int *map_d, const double *TgasCell_d, const double *kappaDelta_d, const double *qin_d,
                      double emissivity, double absorptivity);
/* what the gas region's wall patch reads from the panel after its evolve: refT_d (fluid branch of the coupled condition, :297-303),
 * U_b (flowRateInletVelocityPyrolysisCoupledFvPatchVectorField::updateCoeffs :127-248) and, if emissivity_d is given and the surface
 * radiation model is set, the wall emissivity of greyDiffusiveRadiation with `emissivityMode solidRadiation`
 * (packages/thermophysicalModels/radiation/derivedFvPatchFields/radiationCoupledBase/radiationCoupledBase.C:150-182).  Only the
 * mapped entries are written.                                                                                                      */
int ffm_pyro_gas_side_d(ffm_pyro *p, const int *map_d, const double *rho_b_d, const double *magSf_d, const double *nfx_d, const double *nfy_d,
                        const double *nfz_d, double hocSolid, double qFuel, double *refT_d, double *Ux_d, double *Uy_d, double *Uz_d,
                        double *emissivity_d);
/* reactingOneDim21::solidRegionDiffNo (reactingOneDim21.C:697-714; solver/solidRegionDiffusionNo.H): max over the region's internal faces of
 * deltaCoeffs^2 interpolate(kappa())/interpolate(Cp() rho) * deltaT -- the diffusion number solver/setMultiRegionDeltaT.H limits with maxDi */
int ffm_pyro_diff_no(ffm_pyro *p, double deltaT, double *out);
/* The closed column: BASELINE config 1 (cases/pyrolysis1D) on its own dictionaries.
 * ffm_pyro_set_incident_radiation: `QrIncident` of the fixedIncidentRadiation patch (cases/pyrolysis1D/0/panelRegion/T:51-55), one value
 *   per column: Qr_d[nCol] (device, copied) or, with Qr_d NULL, uniformQr everywhere.
 * ffm_pyro_step_incident: evolveRegion with the exposed face closed by fixedIncidentRadiationFvPatchScalarField::updateCoeffs
 *   (lib/fvPatchFieldsPyrolysis/fixedIncidentRadiation/fixedIncidentRadiationFvPatchScalarField.C:155-213): gradient = e (QrIncident -
 *   sigma pow4(T_cell))/kappa(*this), evaluated where OpenFOAM evaluates the patch (construction of hEqn: old cell temperature, emissivity
 *   and kappa() of the composition after solveSpeciesMass); qSurf and the wall value of the step are stored.  The emissivity is the
 *   surface radiation model's (`kappaMethod solidThermo`, radiationProperties:19-38): FFM_ERR_ARG with a message if
 *   ffm_pyro_set_surface_radiation or ffm_pyro_set_incident_radiation was not called -- there is no constant to fall back to.
 * ffm_pyro_set_qr_source: `qrHSource` of reactingOneDimCoeffs (constant/pyrolysisZones; off by default, as both shipped cases have it):
 *   on != 0 adds the in-depth absorption of reactingOneDim::updateqr / solveEnergy (reactingOneDim.C:95-144, 335-339; reactingOneDim21.C:
 *   96-145, 350-354) to every kind of step: qr0_d[nCol] (device, copied; clipped at 0, :110) is the radiative flux entering through the
 *   exposed face, attenuated with the absorptivities of the surface radiation model (kappaRad(), :656-659) of the composition before
 *   the step; cell i gains A (qr_face,i-1/2 - qr_face,i+1/2).  Call it again when qr0 changes.
 * ffm_pyro_run_incident: solver/fireFoam.C:92-97 with `solvePrimaryRegion false` (cases/pyrolysis1D/constant/additionalControls:18) --
 *   the time loop only calls pyrolysis.evolve() -- as ONE kernel launch: nSteps steps of ffm_pyro_step_incident with every column's
 *   state kept in registers, bitwise equal to nSteps single steps.  hist_d (device, histCap doubles; NULL: no history): after every
 *   sampleEvery-th step, what the case's function objects write (system/controlDict:64-176), hist_d[sample][row][column] with the
 *   2 + 4 nLay rows Twall, phiGas, T[nLay], rho[nLay], Yw[nLay], chemistryQdot[nLay]; nSteps/sampleEvery samples.  FFM_ERR_ARG, before
 *   anything is launched, if nSteps < 1, sampleEvery < 1 or histCap is too small.                                                    */
int ffm_pyro_set_incident_radiation(ffm_pyro *p, double uniformQr, const double *Qr_d);
int ffm_pyro_set_qr_source(ffm_pyro *p, int on, const double *qr0_d);
int ffm_pyro_step_incident(ffm_pyro *p, double deltaT);
int ffm_pyro_run_incident(ffm_pyro *p, double deltaT, int nSteps, int sampleEvery, double *hist_d, long histCap);
int ffm_pyro_destroy(ffm_pyro *p);

/* ------------------------------------------------------- thermo, combustion, LES (N2) */
/* The per-cell physics the reference's time step calls between its equations, one streaming kernel each.
 * ffm_thermo_*: hePsiThermo<reactingMixture<sutherland<janaf<perfectGas<specie>>>>, sensibleEnthalpy> (cases/steckler/constant/
 *   thermophysicalProperties:18-27, thermo.compressibleGas): replaces thermo.correct() (solver/YEEqn.H:114) = hePsiThermo::
 *   calculate() -- cell (or patch-face) mixture by mass fractions, T from he by thermo::T's Newton iteration started at the old
 *   T, psi = 1/(R T), Sutherland mu, alpha = kappa(modified Eucken)/Cp -- and he = Hs(T) where a patch fixes T.  Species table as
 *   in the thermo file (molar coefficients; highCpCoeffs / lowCpCoeffs [nSpecies][7]); Y_d: nSpecies device pointers.
 * ffm_edc_correct_d: the reference's eddyDissipationModel::correct (lib/thermophysicalModels/combustionModels/
 *   eddyDissipationModel/eddyDissipationModel.C:93-149) with kEqn::epsilon = Ce k sqrt(k)/delta: wFuel and Qdot = qFuel wFuel.
 * ffm_les_keqn_nut_d: kEqn::correctNut (nut = Ck sqrt(k) delta) and alphat = rho nut/Prt (alphat_d null: nut only). */
int ffm_thermo_create(ffm_ctx *ctx, int nSpecies, const double *W, const double *Tlow, const double *Thigh, const double *Tcommon,
                      const double *highCpCoeffs, const double *lowCpCoeffs, const double *As, const double *Ts, double RR,
                      ffm_thermo **out);
int ffm_thermo_correct_d(ffm_thermo *th, long n, const double *const *Y_d, const double *he_d, const double *p_d, double *T_d,
                         double *psi_d, double *mu_d, double *alpha_d);
int ffm_thermo_he_d(ffm_thermo *th, long n, const double *const *Y_d, const double *T_d, double *he_d);
/* psi, mu, alpha (each nullable) of the mixture at a given temperature, no iteration (patch faces whose T is fixed) */
int ffm_thermo_properties_d(ffm_thermo *th, long n, const double *const *Y_d, const double *T_d, double *psi_d, double *mu_d,
                            double *alpha_d);
/* Cp of the mixture at T (heThermo::Cp(p, T, patchi): kappaEff of compressible::thermalBaffle1D -- cases/steckler/0/T:51-82 --
 * and the gradient term of mixedEnergy::updateCoeffs) */
int ffm_thermo_Cp_d(ffm_thermo *th, long n, const double *const *Y_d, const double *T_d, double *Cp_d);
/* thermo.correct() of the compiled time step: ffm_thermo_correct_d + ffm_thermo_Cp_d as ONE streaming pass that forms the cell
 * mixture once and writes T (in: the Newton start), psi, mu, alpha and Cp at the new T -- bitwise the pair's values.  No read-back
 * and no synchronisation: *fail_d (a device int the caller owns and clears) is set to 1 where thermo::T exceeds its iteration limit. */
int ffm_thermo_step_d(ffm_thermo *th, long n, const double *const *Y_d, const double *he_d, double *T_d, double *psi_d, double *mu_d,
                      double *alpha_d, double *Cp_d, int *fail_d);
/* the table's species count and, W non-NULL, its molecular weights W[nSpecies] */
int ffm_thermo_species(const ffm_thermo *th, int *nSpecies, double *W);
int ffm_thermo_destroy(ffm_thermo *th);
int ffm_edc_correct_d(ffm_ctx *ctx, long n, const double *rho_d, const double *k_d, const double *delta_d, const double *alpha_d,
                      const double *Yfuel_d, const double *YO2_d, double s, double deltaT, double Ce, double C_EDC, double C_Diff,
                      double C_Stiff, double qFuel, double *wFuel_d, double *Qdot_d);
int ffm_les_keqn_nut_d(ffm_ctx *ctx, long n, double Ck, double Prt, const double *k_d, const double *delta_d, const double *rho_d,
                       double *nut_d, double *alphat_d);

/* ------------------------------------------------------- greyMeanAbsorptionEmission (gas phase) */
/* The reference's second gas absorption/emission model (packages/thermophysicalModels/radiation/submodels/absorptionEmissionModel/
 * greyMeanAbsorptionEmission/greyMeanAbsorptionEmission.C:177-314; coefficient set: cases/pyrolysis1D/constant/radiationProperties:58-146):
 * a polynomial in T or 1/T per participating species, weighted by the species' partial pressure in atm; e = a; E = EhrrCoeff*Qdot.
 * Per cell, in exactly this operation order and without FMA contraction:
 *   invWt = ((0 + Y_0/W_0) + Y_1/W_1) + ...          over ALL nSpecies, in index order (formed once; the reference recomputes it per
 *                                                     participating species with the same operations, hence the same bits)
 *   a = 0; for the participating species j = 0 .. nPart-1, s = specie[j]:
 *     Xk = Y_s/(W_s*invWt);  Xipi = Xk*(p/101325.0);  b = T < Tcommon_j ? lo_j : hi_j  (T == Tcommon takes hi);  Ti = invTemp_j ? 1.0/T : T
 *     a += Xipi*(((((b5*Ti + b4)*Ti + b3)*Ti + b2)*Ti + b1)*Ti + b0)
 * p/101325.0 is upstream OpenFOAM's paToAtm, restated from knowledge: the function is not in the reference tree.
 * SUMMATION ORDER: the caller's list order.  The reference walks a HashTable<label>, whose order follows upstream's string hash; that
 * hash is not in the reference tree and cannot be reproduced here.  The difference is the rounding of a sum of at most 8 terms; this
 * order is UNPINNED BY REFERENCE DATA (the reference ships no output of a run with this model).
 * Not built: the lookUpTableFileName branch (species from a mixture-fraction table), which needs an `ft` field no case here solves.
 *
 * ffm_greymean_create: W[nSpecies] of all species of the mixture in the order of Y_d; specie[nPart] (indices into that list, distinct),
 *   invTemp[nPart], Tcommon / Tlow / Thigh[nPart], lo / hi [nPart][6] = loTcoeffs / hiTcoeffs (b0 .. b5).  nSpecies <= 8 (the thermo
 *   table's limit), 1 <= nPart <= 8.  Anything else: FFM_ERR_ARG, nothing created.  The table travels by value in the kernel arguments.
 * ffm_greymean_a_d: a_d[0..n) as above; Y_d: a HOST array of nSpecies device pointers, as for ffm_thermo_*_d.  flag_d (nullable; a
 *   device int the caller owns and clears) is set to 1 by a plain store when a T lies outside [Tlow, Thigh] of a participating species --
 *   the reference only warns (absorptionCoeffs::checkT).  It is only ever raised; the caller reads it at its next synchronisation.
 *   n == 0 is a no-op; NULL arguments (flag_d excepted) or n < 0: FFM_ERR_ARG, nothing written.
 * ffm_greymean_E_d: E = EhrrCoeff*Qdot, Qdot per volume (the reference's dimEnergy/dimTime/dimVolume branch).
 * ffm_radiation_sh_greymean_d: radiation->Sh of one step with this model in ONE pass: a of the cell in registers, E = EhrrCoeff*Qdot,
 *   su and sp as ffm_radiation_sh_v_d with e = a; a written to a_out_d where that is given.  Bit for bit ffm_greymean_a_d, then
 *   ffm_greymean_E_d, then ffm_radiation_sh_v_d(a, a, sigma, E, ...), without the write and re-read of a and E. */
int ffm_greymean_create(ffm_ctx *ctx, int nSpecies, const double *W, int nPart, const int *specie, const int *invTemp, const double *Tcommon,
                        const double *Tlow, const double *Thigh, const double *lo, const double *hi, double EhrrCoeff, ffm_greymean **out);
int ffm_greymean_destroy(ffm_greymean *gm);
int ffm_greymean_a_d(ffm_greymean *gm, long n, const double *const *Y_d, const double *p_d, const double *T_d, double *a_d,
                     int *flag_d /* nullable */);
int ffm_greymean_E_d(ffm_greymean *gm, long n, const double *Qdot_d, double *E_d);
int ffm_radiation_sh_greymean_d(ffm_greymean *gm, long n, const double *const *Y_d, const double *p_d, const double *T_d, double sigma,
                                const double *G_d, const double *he_d, const double *Qdot_d, const double *Cp_d /* nullable */, double CpConst,
                                double *a_out_d /* nullable */, double *su_d, double *sp_d, int *flag_d /* nullable */);

/* turbulence->divDevRhoReff(U) (solver/UEqn.H:12), explicit part: out[j] = component j of fvc::div(gamma*dev2(T(fvc::grad(U)))),
 * Gauss linear, from the nine cell gradients g[3*i + j] = d_i U_j (ffm_fvc_grad_multi of the three components), gamma = rho*nuEff
 * on cells / patch faces, U and its patch values (the boundary gradient is gaussGrad's corrected one).  The implicit part is
 * ffm_fvm_transport with gamma_f.  ffm_les_keqn_G: G = nut*(gradU && dev(twoSymm(gradU))) of kEqn::correct. */
int ffm_fvc_div_dev2T_gradU(ffm_mesh *m, const double *const *g, const double *gamma, const double *gamma_b,
                            const double *const *U, const double *const *U_b, double *const *out);
int ffm_les_keqn_G(ffm_mesh *m, const double *const *g, const double *nut, double *G);
/* kEqn in the compiled time step (ffm_plume_set_turbulence), row kernels of ffm_fused.hip:
 * ffm_les_keqn_terms: the explicit terms of kEqn::correct in one owner-row pass -- divU = fvc::surfaceIntegrate(phi/interpolate(rho))
 *   (rho_b: patch values of rho), G as ffm_les_keqn_G, and the arrays a scalar transport assembly (ffm_fvm_scalar_transport_multi) takes
 *   as su / su2 / sp:  su = rho G,  su2 = -(min(s,0) k),  sp = max(s,0) + Ce rho sqrt(k)/delta  with  s = (2/3) rho divU,  i.e.
 *   rho G - fvm::SuSp(s, k) - fvm::Sp(Ce rho sqrt(k)/delta, k).  Bitwise equal to ffm_fvc_interpolate, the quotient, ffm_fvc_surface_integrate,
 *   ffm_les_keqn_G and the cell algebra in that order.
 * ffm_les_face_diffusivity: out_f = linear interpolation, out_b = patch values of a cell expression formed on the fly, no cell field:
 *   mode 0  rho*(x + c0/rho)  (rho nuEff: x = nut, c0 = mu; patch rho_b*(x_b + c0/rho_b));  mode 1  c0 + x  (alphaEff: x = alphat, c0 =
 *   alpha; rho, rho_b not read).  Bitwise equal to the cell expression + ffm_fvc_interpolate(NULL, .).
 * ffm_les_keqn_update: bound(k, kMin) and kEqn::correctNut on the first n cells: k = max(k, kMin), nut = Ck sqrt(k) delta,
 *   alphat = rho nut/Prt (ffm_les_keqn_nut_d's expressions). */
int ffm_les_keqn_terms(ffm_mesh *m, const double *const *g, const double *nut, const double *rho, const double *rho_b, const double *k,
                       const double *delta, const double *phi_f, const double *phi_b, double Ce, double *su, double *su2, double *sp);
int ffm_les_face_diffusivity(ffm_mesh *m, int mode, double c0, const double *rho, const double *rho_b, const double *x, const double *x_b,
                             double *out_f, double *out_b);
/* ffm_les_face_diffusivity with the laminar part taken from a cell field c (sutherland mu, modified-Eucken alpha of
 *   ffm_plume_set_thermo) in place of the constant c0; the patch value of c is its zero-gradient copy c[owner cell]:
 *   mode 0  rho*(x + c/rho)   mode 1  c + x   x == NULL (x_b, rho, rho_b then unread; either mode): c itself, i.e. plain linear
 *   interpolation of c and its zero-gradient patch values (the laminar case).  Every row-width bucket.  Bitwise equal to the cell
 *   expression + ffm_fvc_interpolate(NULL, .). */
int ffm_les_face_diffusivity_v(ffm_mesh *m, int mode, const double *c, const double *rho, const double *rho_b, const double *x,
                               const double *x_b, double *out_f, double *out_b);
int ffm_les_keqn_update(ffm_mesh *m, long n, double kMin, double Ck, double Prt, double *k, const double *delta, const double *rho,
                        double *nut, double *alphat);

/* ------------------------------------------------------------------------ GAMG */
/* pairGAMGAgglomeration::forward_ is a static upstream: the cell-visiting direction of the next pair agglomeration, toggled by every
 * agglomeration of the run (a second GAMG mesh or region continues where the first ended).  Here it lives in the context (= the run):
 * ffm_gamg_create reads and updates it; these two set / read it (a fresh context starts forward, as a fresh run does).               */
int ffm_ctx_set_gamg_forward(ffm_ctx *ctx, int forward);
int ffm_ctx_gamg_forward(const ffm_ctx *ctx);
/* lduMatrix::solver::New(... solver GAMG ...) as the reference's dictionaries select it: agglomerator faceAreaPair,
 * mergeLevels 1, nCellsInCoarsestLevel 10, cacheAgglomeration true, smoother GaussSeidel for p_rgh / ph_rgh
 * (cases/wallFireSpread2D/system/fvSolution:36-60, cases/pyrolysis1D/system/fvSolution) and DILU for Ii
 * (cases/steckler/system/fvSolution:63-73).  Replaces OpenFOAM-dev's GAMGSolver::solve + pairGAMGAgglomeration (the
 * algorithm is restated with its sources in oracle/gamg.py).  Decomposed meshes: `finest` is a ghost-cell matrix
 * (ffm_ldu_create_ext + ffm_ldu_set_ghost_exchange; nCells = owned + ghost, the cut faces in lowerAddr / upperAddr); every rank
 * agglomerates its own cells, the processor interfaces are agglomerated with them (coarse ghost cells, coarse cut faces, a ghost
 * exchange per level), continueAgglomerating / normFactor / residuals / scale factors are global -- OpenFOAM's behaviour without a
 * processorAgglomerator (oracle/gamg_multi.py; tests/test_partition_gpu.py::test_gamg_on_a_decomposed_mesh).  A mesh below
 * nCellsInCoarsestLevel gets no coarse level: the solve then is the coarsest-level solver on the fine matrix.
 * ffm_gamg_create: the agglomeration of the mesh behind `finest` (created from the same lowerAddr / upperAddr), built once
 *   (cacheAgglomeration); faceWeights [nFaces] host, e.g. from ffm_gamg_face_area_pair_weights(Sf [nFaces][3]).
 * ffm_gamg_set_matrix_d: GAMGSolver::agglomerateMatrix for every level, from device coefficient arrays in the caller's
 *   cell / face order (lower_d null: symmetric); also sets the coefficients of `finest`.  The arrays must stay alive until
 *   the next call.
 * ffm_gamg_solve_d: GAMGSolver::solve; smoother FFM_GS (GaussSeidel), FFM_SYMGS, FFM_DIC or FFM_DILU; nPreSweeps 0,
 *   nPostSweeps 2 (+1 per level, at most 4), nFinestSweeps 2 (ffm_gamg_set_sweeps), scaleCorrection on symmetric matrices,
 *   coarsest level by PCG+DIC / PBiCGStab+DILU to the same tolerance and relTol.  psi_d / source_d: device, caller order. */
typedef struct ffm_gamg ffm_gamg;
int ffm_gamg_face_area_pair_weights(int nFaces, const double *Sf, double *weights);
int ffm_gamg_create(ffm_ctx *ctx, ffm_ldu *finest, int nCells, int nFaces, const int *lowerAddr, const int *upperAddr,
                    const double *faceWeights, int nCellsInCoarsestLevel, int mergeLevels, ffm_gamg **out);
int ffm_gamg_set_sweeps(ffm_gamg *g, int nPreSweeps, int nPostSweeps, int nFinestSweeps);
int ffm_gamg_set_matrix_d(ffm_gamg *g, const double *diag_d, const double *upper_d, const double *lower_d);
/* the same from the library's native coefficient layout (ffm_ldu_set_coeffs_native_d; the fvMatrix of include/ffmFoam.H) */
int ffm_gamg_set_matrix_native_d(ffm_gamg *g, const double *diag_d, const double *upperNative_d, const double *lowerNative_d);
int ffm_gamg_solve_d(ffm_gamg *g, int smoother, double tolerance, double relTol, int minIter, int maxIter,
                     double *psi_d, const double *source_d, ffm_perf *out);
int ffm_gamg_nlevels(const ffm_gamg *g);                                     /* coarse levels                              */
int ffm_gamg_level_size(const ffm_gamg *g, int level, int *nCells, int *nFaces);          /* level 0: the caller's matrix */
int ffm_gamg_get_level_addressing(const ffm_gamg *g, int level, int *lowerAddr, int *upperAddr);
int ffm_gamg_get_level_coeffs(ffm_gamg *g, int level, double *diag, double *upper, double *lower);   /* host, level order */
int ffm_gamg_coarsest_solves(const ffm_gamg *g, int maxN, ffm_perf *out);    /* of the last solve; returns their number    */
int ffm_gamg_destroy(ffm_gamg *g);

int ffm_device_synchronize(void);     /* hipDeviceSynchronize (debugging aid of the Foam layer: FFM_SYNC_RANGE) */

/* ---------------------------------------------------------------- reductions */
/* gSum / gMin / gMax / gSumProd / gSumMag over a device field (solver/YEEqn.H:
 * 73-78,117-118; solver/phrghEqn.H:54-55).  All-reduced when a communicator is
 * attached.                                                                  */
int ffm_reduce_sum(ffm_ctx *ctx, const double *x_d, long n, double *out);
int ffm_reduce_min(ffm_ctx *ctx, const double *x_d, long n, double *out);
int ffm_reduce_max(ffm_ctx *ctx, const double *x_d, long n, double *out);
int ffm_reduce_dot(ffm_ctx *ctx, const double *x_d, const double *y_d, long n, double *out);
int ffm_reduce_summag(ffm_ctx *ctx, const double *x_d, long n, double *out);

/* ---------------------------------------------------------------------- comm */
/* Pstream replacement: one process per GPU, RCCL over xGMI.
 * uniqueId = the 128-byte ncclUniqueId made by rank 0 (ffm_comm_unique_id) and
 * distributed by the host launcher (torch.distributed / MPI / a file).        */
int ffm_comm_unique_id(void *uniqueId128);
int ffm_comm_init(ffm_ctx *ctx, int rank, int nRanks, const void *uniqueId128);
/* Alternative transport through the host launcher (MPI, gloo, ...): lets several
 * ranks share one GPU (single-GPU testing of the decomposed path).
 * allreduce: in-place over n doubles, op 0 = sum, 1 = min, 2 = max.
 * exchange: patch p sends sendBuf[offset[p] .. +size[p]) to rank nbrRank[p] and
 * receives the same count from it into recvBuf at the same offset.           */
typedef void (*ffm_host_allreduce_fn)(void *user, double *vals, int n, int op);
typedef void (*ffm_host_exchange_fn)(void *user, int nPatches, const int *size,
                                     const int *nbrRank, const int *offset,
                                     const double *sendBuf, double *recvBuf);
int ffm_comm_init_host(ffm_ctx *ctx, int rank, int nRanks, void *user,
                       ffm_host_allreduce_fn allreduce,
                       ffm_host_exchange_fn exchange);
/* variable-count form used by the ghost-cell halo: neighbour q sends
 * sendBuf[sendOff[q]..sendOff[q+1]) to nbrRank[q] and receives recvBuf[recvOff[q]..recvOff[q+1]) from it */
typedef void (*ffm_host_exchange2_fn)(void *user, int nNbr, const int *nbrRank, const int *sendOff,
                                      const int *recvOff, const double *sendBuf, double *recvBuf);
int ffm_comm_set_host_exchange2(ffm_ctx *ctx, ffm_host_exchange2_fn fn);
int ffm_comm_rank(const ffm_ctx *ctx);
int ffm_comm_size(const ffm_ctx *ctx);

/* tests: preset the group ticket counter of the tiled sweeps (every sweep launch zeroes it again on the stream, so a preset
 * close to 2^32 must not change any result)                                                                             */
int ffm_debug_set_sweep_ticket(ffm_ldu *A, unsigned int value);
/* tests: while on != 0, every block ffm_malloc_uninit hands out (fresh or recycled) is filled over its whole size class with one
 * quiet-NaN pattern on the context's stream, so that a consumer which lets a padding slot or a ghost row of such an array reach a
 * real value shows.  Returns the number of blocks filled since the switch was last turned on (< 0: error).  Off by default       */
int ffm_debug_pool_poison(ffm_ctx *ctx, int on);

/* ------------------------------------------------------- decomposition (host) */
/* decomposePar's job for this path (reference: scotch, cases/steckler/system/decomposeParDict:18-20; `simple`,
 * cases/wallFireSpread2D/system/decomposeParDict:18-27; BASELINE names METIS -- none of the three libraries is in this image).
 * part[nCells] = sub-domain of every cell:
 *   ffm_partition_rcb    recursive coordinate bisection of the cell centres C[3][nCells], any number of parts
 *   ffm_partition_graph  greedy graph growing on the LDU graph (no geometry needed)                                        */
int ffm_partition_rcb(int nCells, const double *C, int nParts, int *part);
int ffm_partition_graph(int nCells, int nFaces, const int *lowerAddr, const int *upperAddr, int nParts, int *part);
/* The sub-domain of `rank` in the ghost-cell form of ffm_ldu_create_ext: owned cells in their global relative order, then the
 * ghost cells grouped by neighbour rank (ascending global label inside a group); faces in upper-triangular order, a cut face
 * owned by its owned cell and flagged `flip` where the global owner is the ghost (its local upper coefficient is the global
 * lower one).  ffm_subdomain_exchange gives the arguments of ffm_ldu_set_ghost_exchange and the pair tags of
 * ffm_ldu_set_exchange_tags (kind 1); ffm_subdomain_cut_faces lists the cut faces per neighbour in ascending global face
 * label -- the processor-patch form (faceCells per patch, same order on both sides) for ffm_ldu_set_interfaces.           */
typedef struct ffm_subdomain ffm_subdomain;
int ffm_subdomain_create(int nCells, int nFaces, const int *lowerAddr, const int *upperAddr, const int *part, int nParts,
                         int rank, ffm_subdomain **out);
int ffm_subdomain_destroy(ffm_subdomain *s);
int ffm_subdomain_sizes(const ffm_subdomain *s, int *nOwned, int *nGhost, int *nFaces, int *nNbr, int *nSend, int *nCut);
int ffm_subdomain_cells(const ffm_subdomain *s, int *globalCell /* [nOwned+nGhost] */);
int ffm_subdomain_faces(const ffm_subdomain *s, int *lowerAddr, int *upperAddr, int *globalFace, int *flip);
int ffm_subdomain_exchange(const ffm_subdomain *s, int *nbrRank, int *sendCount, int *sendCells, int *recvCount, int *tags);
int ffm_subdomain_cut_faces(const ffm_subdomain *s, int *cutStart /* [nNbr+1] */, int *localCell, int *globalFace, int *flip);

/* ------------------------------------------------------- polyMesh (host)    */
/* SURVEY 8(f) N4, first part: OpenFOAM's on-disk mesh (ascii constant/polyMesh/{points,faces,owner,neighbour,boundary}, as
 * blockMesh / topoSet / createBaffles leave it: reference cases/steckler/mesh.sh:8-21) and the finite-volume geometry
 * derived from it with OpenFOAM's algorithms (face fans, cell pyramids, weights, nonOrthDeltaCoeffs, correction vectors):
 * the inputs of ffm_ldu_create / ffm_mesh_create / ffm_mesh_set_face_centres / ffm_mesh_set_nonorth_correction.  Host only. */
typedef struct ffm_polymesh ffm_polymesh;
int ffm_polymesh_read(const char *polyMeshDir, ffm_polymesh **out);
int ffm_polymesh_destroy(ffm_polymesh *pm);
int ffm_polymesh_sizes(const ffm_polymesh *pm, int *nPoints, int *nCells, int *nFaces, int *nInternalFaces, int *nPatches);
int ffm_polymesh_addressing(const ffm_polymesh *pm, int *lowerAddr, int *upperAddr);
/* cell arrays [N] / [3][N]; internal-face arrays [F] / [3][F]; NULL = not wanted */
int ffm_polymesh_geometry(const ffm_polymesh *pm, double *V, double *C, double *Sf, double *Cf, double *magSf, double *weights,
                          double *nonOrthDeltaCoeffs, double *nonOrthCorrectionVectors);
int ffm_polymesh_patch(const ffm_polymesh *pm, int i, char *name64, char *type32, int *startFace, int *nFaces);
/* processorN/constant/polyMesh of a case decomposed by decomposePar: 1 if patch i is `type processor` (then *myProcNo and
 * *neighbProcNo hold its entries), 0 if not.  Its faceCells (ffm_polymesh_patch_geometry) and the neighbour rank are the
 * faceCells / neighbRank of ffm_ldu_set_interfaces; both sides list the faces of a processor patch in the same order. */
int ffm_polymesh_patch_processor(const ffm_polymesh *pm, int i, int *myProcNo, int *neighbProcNo);
int ffm_polymesh_patch_geometry(const ffm_polymesh *pm, int i, int *faceCells, double *Sf, double *Cf, double *deltaCoeffs);

#ifdef __cplusplus
}
#endif
#endif
