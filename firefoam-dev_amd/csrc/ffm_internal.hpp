// ffm_internal.hpp -- private structures of libffm.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <tuple>
#include <unordered_map>

#include "ffm_host.hpp"          // ffm_set_error, FFM_TRY, ffm_parallel_for, the set-up timers, LduAnalysis / LduLayout

struct ncclComm;
struct ffm_tile_plan;

#define FFM_HIP(call)                                                            \
    do {                                                                         \
        hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) {                                                  \
            ffm_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call,           \
                          hipGetErrorString(e_));                                \
            return FFM_ERR_HIP;                                                  \
        }                                                                        \
    } while (0)

// Fixed reduction geometry: every dot product is a two-stage, atomics-free,
// order-fixed sum (RED_BLOCKS partials, then one block), so results are
// bitwise reproducible from run to run.
constexpr int RED_THREADS = 256;
constexpr int RED_BLOCKS = 2048;
constexpr int NSCAL = 64;  // device scalar slots per context

// device scalar slots
enum {
    S_TMP0 = 0, S_TMP1, S_TMP2, S_TMP3,
    S_XREF, S_NORMF, S_RES, S_RES0,
    S_WARA, S_WARA_OLD, S_WAPA, S_ALPHA, S_BETA, S_OMEGA,
    S_RA0RA, S_RA0RA_OLD, S_RA0AYA, S_TATA, S_TASA,
    S_SING,      // != 0 => singular flag
    S_NEG_ALPHA, S_ONE
};

// A solver's scalar operation (ffm_device.hpp: scalar_op_body) that rides on the one-workgroup launch which sums a reduction's
// partials: thread 0 runs it after storing the sum.  fused == false: the launch only sums (more than one rank: the all-reduce sits
// between the sum and the operation, ffm_solve.hip: finish_dot).
struct ffm_scal_op { int op = 0; double arg = 0.0; int iter = 0; int in = S_TMP0; bool fused = false; };

struct ffm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    double *scal_d = nullptr;      // [NSCAL]
    double *partials_d = nullptr;  // [4][RED_BLOCKS]
    double *scal_h = nullptr;      // pinned [NSCAL]
    double *multiScal_d = nullptr, *multiScal_h = nullptr;      // [FFM_TILE_MAXSYS][NSCAL]: the lanes of ffm_solve_multi_d (allocated on first use)
    // communicator (RCCL); nRanks == 1 => serial
    int rank = 0, nRanks = 1;
    ncclComm *comm = nullptr;
    // a communicator of its own for the ghost exchange that overlaps the interior rows on commStream: RCCL serialises the operations of
    // ONE communicator, so collectives of one communicator issued from two streams (halo group on commStream, dot-product all-reduces on
    // stream) may be launched in different orders on different ranks and deadlock; two communicators have independent queues
    ncclComm *haloComm = nullptr;
    void *hostUser = nullptr;
    ffm_host_allreduce_fn hostAllreduce = nullptr;
    ffm_host_exchange_fn hostExchange = nullptr;
    ffm_host_exchange2_fn hostExchange2 = nullptr;
    int cuCount = 256;
    // pairGAMGAgglomeration::forward_: a STATIC upstream -- the direction in which the next pair agglomeration visits the cells, toggled by
    // every agglomeration of the run, so a second GAMG mesh / region starts in the direction the first one ended with (ffm_ctx_set_gamg_forward)
    bool gamgForward = true;
    // second stream for the RCCL ghost exchange of an Amul whose interior rows do not need the ghost values (tiled Amul):
    // pack (main stream) -> evPack -> send / receive (commStream) -> evRecv -> ghost-face tail (main stream)
    hipStream_t commStream = nullptr;
    hipEvent_t evPack = nullptr, evRecv = nullptr;
    // stream-ordered caching allocator behind ffm_malloc / ffm_free (the Foam layer makes one temporary per operator):
    // a freed block goes to the free list of its size class without synchronising -- every consumer runs on `stream`, so a
    // later owner's kernels are ordered after the previous owner's -- and is handed out again by the next ffm_malloc of that
    // class; ffm_ctx_trim / ffm_ctx_destroy return the cached blocks to the runtime
    std::unordered_map<size_t, std::vector<void *>> poolFree;
    std::unordered_map<void *, size_t> poolSize;
    size_t poolCachedBytes = 0, poolCapBytes = (size_t)96 << 30;
    bool poolPoison = false;              // ffm_debug_pool_poison (tests): unzeroed blocks are handed out NaN-filled
    int poolPoisoned = 0;                 // ... and counted
};

// Host <-> device copies, correct by construction: the context's stream is created non-blocking, so a null-stream hipMemcpy neither
// waits for work queued on it (a pooled block's zero-fill, a kernel that writes the table being read back) nor is waited for by it.
// Every copy of the library therefore goes through these two -- queued on the context's stream and waited for -- and the bare
// runtime calls are poisoned for the rest of every translation unit that includes this header.
inline int ffm_h2d(ffm_ctx *c, void *dst_d, const void *src, size_t bytes)
{
    if (!bytes) return FFM_OK;
    FFM_HIP(hipMemcpyAsync(dst_d, src, bytes, hipMemcpyHostToDevice, c->stream)); FFM_HIP(hipStreamSynchronize(c->stream));
    return FFM_OK;
}
inline int ffm_d2h(ffm_ctx *c, void *dst, const void *src_d, size_t bytes)
{
    if (!bytes) return FFM_OK;
    FFM_HIP(hipMemcpyAsync(dst, src_d, bytes, hipMemcpyDeviceToHost, c->stream)); FFM_HIP(hipStreamSynchronize(c->stream));
    return FFM_OK;
}
inline int ffm_dzero(ffm_ctx *c, void *dst_d, size_t bytes)
{
    if (!bytes) return FFM_OK;
    FFM_HIP(hipMemsetAsync(dst_d, 0, bytes, c->stream));
    return FFM_OK;
}
template <class T, class Al> inline int ffm_upload_vec(ffm_ctx *c, T **d, const std::vector<T, Al> &v, size_t minCount = 1)
{
    FFM_HIP(hipMalloc((void **)d, sizeof(T) * std::max<size_t>(v.size(), minCount)));
    return ffm_h2d(c, *d, v.data(), sizeof(T) * v.size());
}
#pragma GCC poison hipMemcpy hipMemset

// Host set-up arrays of many GB (geometry of a 400^3 box) whose elements are not value-initialised on allocation: they are filled
// with ffm_parallel_for, so the first touch of their pages is spread over the host threads instead of falling on one
template <class T> struct ffm_noinit_alloc : std::allocator<T> {
    template <class U> struct rebind { using other = ffm_noinit_alloc<U>; };
    ffm_noinit_alloc() = default;
    template <class U> ffm_noinit_alloc(const ffm_noinit_alloc<U> &) {}
    template <class U> void construct(U *p) { ::new ((void *)p) U; }
    template <class U, class... A> void construct(U *p, A &&...a) { ::new ((void *)p) U(std::forward<A>(a)...); }
};
template <class T> using ffm_hvec = std::vector<T, ffm_noinit_alloc<T>>;
template <class T> inline ffm_hvec<T> ffm_hvec_fill(size_t n, T v)
{
    ffm_hvec<T> a(n);
    T *p = a.data();
    ffm_parallel_for((long)n, [=](long lo, long hi) { for (long i = lo; i < hi; i++) p[i] = v; });
    return a;
}

struct ffm_iface {
    int size = 0, nbrRank = -1;
    int offset = 0;                 // offset into the packed halo buffers
};

struct ffm_ldu {
    ffm_ctx *ctx = nullptr;
    int nCells = 0, nFaces = 0;        // nCells = owned + ghost cells (array length of every cell field)
    int nOwned = 0;                    // rows of this rank; ghost cells [nOwned, nCells) are copies of neighbour-rank cells
    long globalCells = 0;
    std::vector<int> h_ghSendCaller;        // the send cells of the ghost exchange in the caller's cell labels (GAMG: agglomerated per level)
    bool identity = true;           // caller numbering == internal numbering
    bool symmetric = true;

    // host copies of the analysis (internal numbering)
    std::vector<int> h_newToOldCell, h_newToOldFace;
    int nLevels = 0;                    // forward dependency levels

    // device addressing (internal cell numbering): sliced owner-ELL.
    // Cells are grouped in slices of 64 (one wavefront).  Slice sl stores its faces slot-major:
    //   upper part: entry e = upOff[sl] + s*64 + lane, s < upper width of the slice
    //       upNbr[e]  = neighbour cell of the s-th face OWNED by cell sl*64+lane (-1 = padding)
    //       upper[e] / lower[e] = the face's upper / lower coefficient (0 on padding)
    //     e is the library's NATIVE FACE INDEX; the owner of a native face is implicit.
    //   lower part: entry q = loOff[sl] + s*64 + lane
    //       loEnt[q] = (owner cell << loShift) | slot of that face in the owner's row  (-1 = padding)
    //     listing the faces whose NEIGHBOUR is the cell, in the caller's face order.  loShift is 4 unless some cell owns more than
    //     16 faces towards owned cells (wide coarse GAMG levels): then 5, and the matrix may have 2^26 cells instead of 2^27
    //     (ffm_ldu_analysis.cpp: check_layout_limits).  Every decoder takes the shift from the handle or from LduView.
    // Every load of an index or coefficient array is unit-stride across the wave; the symmetric
    // coefficient is stored once and re-read through the (nbr, slot) pair by the neighbour row.
    int nSlices = 0, upTotal = 0, loTotal = 0;
    int upWidthUniform = -1;                     // >= 0: every slice has this upper width
    int loWidthUniform = -1;
    int maxW = 0;                                // max slots (lower or upper) of any row
    int loShift = 4;                             // bits of the slot field of loEnt
    int *upOff = nullptr, *loOff = nullptr;      // [nSlices+1]
    int *upNbr = nullptr;                        // [upTotal]
    int *loEnt = nullptr;                        // [loTotal]
    int *flowOrder = nullptr;                    // [nOwned] cells by backward level (dataflow sweeps, ffm_solve.hip; level-scheduled mode)
    int *cellPerm = nullptr;                     // [N] new->old (only when !identity)
    int *faceSrc = nullptr;                      // [upTotal] native face -> caller face id (-1 padding)
    std::vector<int> h_callerToNative;           // [F] caller face id -> native face index
    std::vector<int> h_upOff, h_loOff, h_loEnt, h_upNbr;   // host copies for the sweep planners (entries freed after use)
    int *callerToNative = nullptr;               // device copy (on demand)

    // coefficients (internal numbering / native face index)
    double *diag = nullptr, *upper = nullptr, *lower = nullptr;  // lower==upper when symmetric
    double *lowerBuf = nullptr;                                  // storage for asymmetric lower

    // XCD-aware row schedule of the row kernels: list of 256-row chunks; entry i is processed by a workgroup with
    // blockIdx % 8 == i % 8, i.e. (observed round-robin dispatch) always on the same XCD, and chunks with the same i % 8
    // cover the same eighth of every dependency level, so a row's neighbours in the adjacent levels were touched by the
    // same XCD and are found in its L2.  Speed only; correctness does not depend on the placement.
    int *rowSched = nullptr; int nSched = 0;

    // preconditioner state
    double *rD = nullptr;          // reciprocal diagonal (DIC/DILU/diagonal)
    int rDKind = -1;               // which preconditioner rD currently holds
    unsigned long coeffEpoch = 0, rDEpoch = ~0ul;
    unsigned long offDiagEpoch = 0;       // bumped when upper / lower change (coeffEpoch: any coefficient, diag included)
    // the tile plan's coefficient arrays were written by the launch that wrote these native arrays (ffm_tile.hip: ffm_tile_coef_direct);
    // pending until the next set / bind, which adopts them if it binds exactly these arrays
    bool directPending = false;
    const double *directUpper = nullptr, *directLower = nullptr;
    unsigned long tileGathers = 0;        // k_tile_gather launches of this matrix (tests)
    double *diagBuf = nullptr, *upperBuf = nullptr;     // the library's own coefficient storage; diag/upper/lower may instead
                                                        // point at caller arrays (ffm_ldu_bind_coeffs_native_d)

    // work vectors (internal numbering), allocated on demand
    std::vector<double *> work;    // [nWork] each N doubles
    double *gsProd = nullptr;      // [3N] scratch of the tiled Gauss-Seidel sweep
    double *permIn[3] = {nullptr, nullptr, nullptr};  // staging for caller-order vectors

    // interfaces (processor patches), packed patch after patch
    std::vector<ffm_iface> ifaces;
    std::vector<int> ifaceTags, ghTags;   // pair tags: posting order of the point-to-point messages (ffm_ldu_set_exchange_tags)
    int haloTotal = 0;
    int *ifFaceCells = nullptr;    // [haloTotal] internal numbering
    double *ifBou = nullptr, *ifInt = nullptr;   // [haloTotal]
    double *haloSend = nullptr, *haloRecv = nullptr;
    double *haloSend_h = nullptr, *haloRecv_h = nullptr;   // pinned, host transport only
    // boundary cells grouped: cell ifCell[j] owns packed items ifItem[ifCellStart[j]..ifCellStart[j+1])
    // listed in (patch, face) order, so a cell's interface terms are added in the reference's order
    int nIfCells = 0;
    int *ifCell = nullptr, *ifCellStart = nullptr, *ifItem = nullptr;

    // ghost-cell halo plan (native decomposed path): for neighbour q, send x[ghSendCells[ghSendOff[q]..]] and receive
    // straight into x[nOwned + ghRecvOff[q] ..]
    std::vector<int> ghNbrRank, ghSendOff, ghRecvOff;   // offsets have nNbr+1 entries
    int *ghSendCells = nullptr;
    bool ghPending = false;        // an overlapped exchange is in flight on ctx->commStream (ffm_ghost_exchange_begin / _end)
    double *ghSendBuf = nullptr, *ghSendBuf_h = nullptr, *ghRecvBuf_h = nullptr;

    // ---- tiled sweep plan (sweepMode == 2): cells are numbered group-major, level-major inside a group;
    // group g = cells [grpCell[g], grpCell[g+1]); one workgroup sweeps one group level by level (ffm_tile.hip)
    int sweepMode = 0;              // 0: dataflow sweeps (level-major numbering); 2: tiled wavefront sweeps
    int nGroups = 0;
    bool bwdIsReverse = false;      // inside every group the backward order is the exact reverse of the forward order
    int *grpCell = nullptr;         // [G+1]
    unsigned int *sweepTicket = nullptr;          // [2]: ticket counter (zeroed on the stream before every sweep), abort flag
    ffm_tile_plan *tile = nullptr;                // tiled wavefront plan (sweepMode == 2)
};

struct LduView;
LduView ffm_view(const ffm_ldu *A);
const int *ffm_mesh_bcells(const ffm_mesh *m);                 // ffm_fv.hip: face cell of every boundary face (device)
const double *ffm_mesh_geom(const ffm_mesh *m, int which);     // ... and the mesh's device geometry arrays
// ---- internal helpers shared between translation units -------------------
int ffm_ldu_work(ffm_ldu *A, int idx, double **out);           // lazily allocated N-vectors
int ffm_to_internal(ffm_ldu *A, const double *x_d, int slot, const double **out);
int ffm_from_internal(ffm_ldu *A, const double *xin, double *x_d);
int ffm_k_spmv(ffm_ldu *A, const double *x, double *y, bool transpose);
int ffm_k_spmv_dot(ffm_ldu *A, const double *x, double *y, int slot, const ffm_scal_op &t = ffm_scal_op());  // y=Ax, scal[slot]=x.y (local)
int ffm_k_residual(ffm_ldu *A, const double *x, const double *b, double *r);
int ffm_k_sumA(ffm_ldu *A, double *s);
int ffm_k_spmv_sumA_rows(ffm_ldu *A, const double *x, double *y, double *s);   // this rank's rows, no ghost refresh
int ffm_k_residual_rows(ffm_ldu *A, const double *x, const double *b, double *r);
int ffm_k_spmv_sumA(ffm_ldu *A, const double *x, double *y, double *s);
int ffm_halo_update(ffm_ldu *A, const double *x, double *y, const double *coeffs, double sign);  // exchange + apply
int ffm_halo_apply(ffm_ldu *A, double *y, const double *coeffs, const double *vals /*null => 1*/, double sign);
int ffm_allreduce_slots(ffm_ctx *ctx, int firstSlot, int n);   // sum over ranks, in stream
int ffm_allreduce_minmax(ffm_ctx *ctx, int slot, int isMax, int n = 1);   // min or max over ranks of n slots, in stream
void ffm_comm_finalize_i(ffm_ctx *ctx);
int ffm_precond_setup_i(ffm_ldu *A, int precond);
int ffm_precond_apply_i(ffm_ldu *A, int precond, bool transpose, const double *r, double *w);
int ffm_tile_build(ffm_ldu *A, const std::vector<int> &lev, const std::vector<int> &bl, const std::vector<int> &grpCell);
int ffm_sweep_check_abort(ffm_ldu *A);                   // abort word of the tiled and the dataflow sweeps (ffm_solve.hip)
int ffm_tile_gs_ghost_terms(ffm_ldu *A, const double *psi, double *bP);
int ffm_ghost_exchange(ffm_ldu *A, double *x);
int ffm_ghost_exchange_begin(ffm_ldu *A, double *x);     // starts the refresh of x[nOwned..nCells); may return with it in flight
int ffm_ghost_exchange_split(ffm_ldu *A, const double *sendFrom, double *ghostInto);   // the same exchange: owned cells of one field out, the ghost layers [nGhost] of another in
int ffm_ghost_exchange_end(ffm_ldu *A);                  // the main stream waits for it
int ffm_tile_gs(ffm_ldu *A, bool sym, double *psi, const double *bP, double *bSave, double *prod3);
bool ffm_tile_amul_usable(const ffm_ldu *A);
int ffm_tile_amul(ffm_ldu *A, const double *x, double *y, int dotSlot, const ffm_scal_op &t = ffm_scal_op());     // returns 1 if the dot product is left to the caller
void ffm_tile_free(ffm_ldu *A);
bool ffm_tile_usable(const ffm_ldu *A);
struct FfmFvSegs { int nSeg; const int4 *seg; const int4 *rec; };
bool ffm_tile_fv_segments(ffm_ldu *A, int runLength, FfmFvSegs *out);   // single block, tile plan present: FV face passes through LDS (ffm_fused.hip)
bool ffm_tile_coef_direct_ok(const ffm_ldu *A);          // no ghost cells, a tile plan, rows of at most FFM_TILE_W entries per side
int ffm_tile_coef_direct(ffm_ldu *A, bool lower, double **fU, double **fL, double **bU);   // the plan's coefficient arrays, to be written by an assembly kernel
void ffm_tile_coef_written(ffm_ldu *A, const double *upper_d, const double *lower_d);
void ffm_tile_coef_adopt(ffm_ldu *A);
bool ffm_tile_pcg_fusable(const ffm_ldu *A);
int ffm_tile_pcg_fwd(ffm_ldu *A, double *rA, double *wA, int slot, const double *qA = nullptr, const ffm_scal_op &t = ffm_scal_op());
bool ffm_tile_amul_pcg_usable(const ffm_ldu *A);
bool ffm_tile_amul_asym_usable(const ffm_ldu *A);
int ffm_tile_amul_asym(ffm_ldu *A, const double *x, double *y);
int ffm_tile_amul_pcg(ffm_ldu *A, const double *w, const double *pin, double *pout, double *psi, double *y, int dotSlot, const ffm_scal_op &t = ffm_scal_op());
int ffm_tile_pcg_bwd(ffm_ldu *A, const double *rA, double *wA, int slot, const ffm_scal_op &t = ffm_scal_op());
// n = 1 .. FFM_TILE_MAXSYS systems with the matrix's off-diagonal coefficients in one sweep (ffm_tile.hip: k_tile); n = 1: the matrix's own
#define FFM_TILE_MAXSYS 5
bool ffm_tile_multi_fits(const ffm_ldu *A, int n);      // n systems fit the LDS rings of one sweep (five: the short ring)
int ffm_tile_precond(ffm_ldu *A, int precond, bool transpose, int n, const double *const *rD, const double *const *r, double *const *w);
int ffm_tile_calc_rD(ffm_ldu *A, int n, const double *const *diag, double *const *D);
int ffm_k_spmv_multi(ffm_ldu *A, int n, const double *const *diag, const double *const *x, double *const *y, double *const *sumA);
// ffm_solve_d on internal (native-order) vectors, no caller-order staging (ffm_solve.hip; GAMG's coarsest level)
extern "C" int ffm_solve_internal_i(ffm_ldu *A, int solver, int precond, double tol, double relTol, int minIter, int maxIter, int nSweeps,
                                    double *psi, const double *source, ffm_perf *perf);
int ffm_gs_smooth_i(ffm_ldu *A, bool sym, int nSweeps, double *psi, const double *b);
int ffm_halo_exchange(ffm_ldu *A, const double *x);
int ffm_ghost_exchange(ffm_ldu *A, double *x);                 // refresh x[nOwned..nCells) from the neighbour ranks          // pack x[faceCells], exchange into haloRecv
int ffm_read_scalars(ffm_ctx *ctx);  // scal_d -> scal_h, synchronises the stream

// reductions into device scalar slots (local partial sums; caller all-reduces); t: an operation for the summing launch to run
int ffm_k_dot(ffm_ctx *ctx, const double *x, const double *y, long n, int slot, const ffm_scal_op &t = ffm_scal_op());
int ffm_k_summag(ffm_ctx *ctx, const double *x, long n, int slot, const ffm_scal_op &t = ffm_scal_op());
int ffm_k_sum(ffm_ctx *ctx, const double *x, long n, int slot, const ffm_scal_op &t = ffm_scal_op());
int ffm_k_sumsqr(ffm_ctx *ctx, const double *x, long n, int slot, const ffm_scal_op &t = ffm_scal_op());

static inline int ffm_grid(long n, int threads) { return (int)((n + threads - 1) / threads); }
