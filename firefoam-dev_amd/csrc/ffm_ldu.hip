// ffm_ldu.hip -- device LDU container and the lduMatrix kernels Amul / Tmul / sumA / residual.
// (The lduAddressing analysis and the layout are host code: ffm_ldu_analysis.cpp.)
//
// Replaces (OpenFOAM-dev @940e28f, not vendored in the reference):
//   src/OpenFOAM/matrices/lduMatrix/lduAddressing/lduAddressing.C
//   src/OpenFOAM/matrices/lduMatrix/lduMatrix/lduMatrixATmul.C
// reached from the reference at solver/pEqn.H:5,39, solver/UEqn.H:19,
// solver/YEEqn.H:60,111.
//
// Data layout in HBM (all arrays in the *internal* cell numbering):
//   cells are ordered level-major: level(c) = longest path to c in the DAG
//   owner->neighbour, cells of one level contiguous and sorted by the caller's
//   index.  Every level-scheduled sweep (DIC/DILU/Gauss-Seidel) then touches a
//   contiguous cell range per level, and the SpMV runs in the same numbering so
//   no vector is permuted between SpMV and preconditioner.  The renumbering is a
//   topological order of the same DAG, so owner<neighbour is preserved and the
//   incomplete factorisations are the same operators as in the caller's
//   numbering.  A caller whose mesh is already level-major (ffm_renumber_levels)
//   pays no permutation pass at all.
//
//   Faces are stored as a sliced owner-ELL (slices of 64 cells = one wavefront,
//   slot-major inside a slice; see ffm_internal.hpp): every index / coefficient
//   load is unit-stride across the wave, the owner of a face is implicit, and a
//   symmetric coefficient is stored once -- the neighbour row re-reads it through
//   a packed (owner cell, slot) entry, which hits cache because neighbouring rows
//   are neighbours in memory.  HBM traffic of a symmetric Amul is therefore the
//   algorithmic 24 N + 16 F bytes plus padding.
//   Row form of the face loops: row c first adds its lower entries (faces whose
//   neighbour is c, in the caller's face order), then its upper slots (faces
//   owned by c, in the caller's face order) -- exactly the order in which the
//   serial face loop of the reference touches row c, so no atomics are needed
//   and every row sum is bitwise the reference's.
#include "ffm_internal.hpp"
#include "ffm_device.hpp"
#include <algorithm>

// ------------------------------------------------------------------ create ---
template <class T>
static int upload(ffm_ctx *c, T **dst, const std::vector<T> &v, size_t minCount = 1)
{
    size_t n = std::max(v.size(), minCount);
    FFM_HIP(hipMalloc((void **)dst, n * sizeof(T)));
    if (!v.empty()) FFM_HIP(hipMemcpyAsync(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return FFM_OK;
}

extern "C" int ffm_ldu_create(ffm_ctx *ctx, int N, int F, const int *l, const int *u, ffm_ldu **out)
{ return ffm_ldu_create_ext(ctx, N, 0, F, l, u, out); }

extern "C" int ffm_ldu_create_ext(ffm_ctx *ctx, int nOwn, int nGhost, int F, const int *l, const int *u, ffm_ldu **out)
{ return ffm_ldu_create_hint(ctx, nOwn, nGhost, F, l, u, nullptr, out); }

static int ldu_create_impl(ffm_ctx *ctx, int nOwn, int nGhost, int F, const int *l, const int *u, const int *groupHint, int forceMode,
                           ffm_ldu **out);

extern "C" int ffm_ldu_create_hint(ffm_ctx *ctx, int nOwn, int nGhost, int F, const int *l, const int *u, const int *groupHint,
                                   ffm_ldu **out)
{
    if (!ctx || !out || nOwn < 0 || nGhost < 0 || F < 0 || (F && (!l || !u))) { ffm_set_error("ffm_ldu_create: bad argument"); return FFM_ERR_ARG; }
    FFM_HIP(hipSetDevice(ctx->device));
    FFM_TRY(ldu_create_impl(ctx, nOwn, nGhost, F, l, u, groupHint, -1, out));
    if ((*out)->sweepMode == 2 && !ffm_tile_usable(*out)) {
        // the tile planner gave up on this grouping (entry order, external references per entry, ghost faces before owned
        // ones): the same matrix with level-scheduled sweeps instead
        if (getenv("FFM_VERBOSE")) fprintf(stderr, "ffm: no tile plan for this mesh / grouping: level-scheduled sweeps\n");
        ffm_ldu_destroy(*out); *out = nullptr;
        FFM_TRY(ldu_create_impl(ctx, nOwn, nGhost, F, l, u, nullptr, 0, out));
    }
    return FFM_OK;
}

// Everything of the handle that lives on the device, in stream order: the addressing, the tile plan, the row schedule, zeroed coefficients.
static int ldu_upload(ffm_ldu *A, const LduAnalysis &a, const LduLayout &L)
{
    ffm_ctx *ctx = A->ctx;
    const int N = A->nCells, nOwn = A->nOwned;
    FFM_TRY(upload(ctx, &A->upOff, L.upOff));
    FFM_TRY(upload(ctx, &A->loOff, L.loOff));
    FFM_TRY(upload(ctx, &A->upNbr, L.upNbr));
    FFM_TRY(upload(ctx, &A->loEnt, L.loEnt));
    FFM_TRY(upload(ctx, &A->faceSrc, L.faceSrc));
    if (A->sweepMode == 0) FFM_TRY(upload(ctx, &A->flowOrder, a.bwdOrder));
    if (A->sweepMode == 2) FFM_TRY(upload(ctx, &A->grpCell, a.grpCell));
    if (hipMalloc((void **)&A->sweepTicket, 2 * sizeof(unsigned int)) != hipSuccess) return FFM_ERR_HIP;
    hipMemsetAsync(A->sweepTicket, 0, 2 * sizeof(unsigned int), ctx->stream);
    if (!A->identity) FFM_TRY(upload(ctx, &A->cellPerm, a.newToOldCell));
    if (A->sweepMode == 2) {
        A->h_loEnt = L.loEnt; A->h_upNbr = L.upNbr;
        // Backward order of the tiled sweeps.  Where the backward dependency levels are the mirror image of the forward ones (a box)
        // the backward sweep walks the forward entries in reverse.  Where they are not (internal walls, unstructured graphs) it STILL
        // can: the reverse of a topological order is a topological order of the reversed graph, and the cells of one forward level are
        // never neighbours, so they form a valid backward entry as well -- neighbours that are then far away in the numbering go
        // through the mailboxes like any other external.  Such meshes take the backward levels mirrored from the forward ones.
        int rc;
        if (a.bwdIsReverse) rc = ffm_tile_build(A, a.levNew, a.blNew, a.grpCell);
        else {
            int maxLev = 0;
            for (int c = 0; c < nOwn; c++) maxLev = std::max(maxLev, a.levNew[c]);
            std::vector<int> blSym(nOwn);
            for (int c = 0; c < nOwn; c++) blSym[c] = maxLev - a.levNew[c];
            rc = ffm_tile_build(A, a.levNew, blSym, a.grpCell);
        }
        A->h_loEnt.clear(); A->h_loEnt.shrink_to_fit(); A->h_upNbr.clear(); A->h_upNbr.shrink_to_fit();
        FFM_TRY(rc);
    }
    A->nSched = (int)L.rowSched.size();
    FFM_TRY(upload(ctx, &A->rowSched, L.rowSched));
    size_t nb = sizeof(double) * (size_t)std::max(N, 1), fb = sizeof(double) * (size_t)std::max(A->upTotal, 1);
    if (hipMalloc((void **)&A->diag, nb) != hipSuccess || hipMalloc((void **)&A->upper, fb) != hipSuccess ||
        hipMalloc((void **)&A->rD, nb) != hipSuccess) { ffm_set_error("ffm_ldu_create: hipMalloc failed"); return FFM_ERR_HIP; }
    A->lower = A->upper; A->diagBuf = A->diag; A->upperBuf = A->upper;
    hipMemsetAsync(A->diag, 0, nb, ctx->stream); hipMemsetAsync(A->upper, 0, fb, ctx->stream);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { ffm_set_error("ffm_ldu_create: upload failed"); return FFM_ERR_HIP; }
    return FFM_OK;
}

// analysis, then layout (both on the host: ffm_ldu_analysis.cpp), then upload
static int ldu_create_impl(ffm_ctx *ctx, int nOwn, int nGhost, int F, const int *l, const int *u, const int *groupHint, int forceMode,
                           ffm_ldu **out)
{
    LduAnalysis a;
    { FfmStageTimer tm_("ldu_create: analyse");
      FFM_TRY(ffm_ldu_analysis(nOwn, nGhost, F, l, u, groupHint, forceMode, a)); }
    FfmStageTimer tmRest_("ldu_create: layout+upload+tile");
    LduLayout L;
    FFM_TRY(ffm_ldu_layout(a, nOwn, nGhost, F, L));
    ffm_ldu *A = new ffm_ldu();
    A->ctx = ctx; A->nCells = nOwn + nGhost; A->nOwned = nOwn; A->nFaces = F; A->globalCells = nOwn;
    A->identity = a.identity;
    A->sweepMode = a.mode; A->nGroups = a.nGroups; A->bwdIsReverse = a.bwdIsReverse;
    A->nLevels = std::max((int)a.fwdLevelStart.size() - 1, 0);
    A->h_newToOldCell = a.newToOldCell; A->h_newToOldFace = a.newToOldFace;
    A->nSlices = L.nSlices; A->upTotal = L.upTotal; A->loTotal = L.loTotal;
    A->upWidthUniform = L.upWidthUniform; A->loWidthUniform = L.loWidthUniform; A->maxW = L.maxW; A->loShift = L.loShift;
    A->h_upOff = L.upOff; A->h_loOff = L.loOff;
    A->h_callerToNative = std::move(L.callerToNative);
    const int rc = ldu_upload(A, a, L);
    if (rc) { ffm_ldu_destroy(A); return rc; }
    *out = A;
    return FFM_OK;
}

extern "C" int ffm_ldu_destroy(ffm_ldu *A)
{
    if (!A) return FFM_OK;
    hipSetDevice(A->ctx->device);
    hipStreamSynchronize(A->ctx->stream);
    for (double *w : A->work) hipFree(w);
    hipFree(A->gsProd);
    for (int i = 0; i < 3; i++) hipFree(A->permIn[i]);
    hipFree(A->upOff); hipFree(A->loOff); hipFree(A->upNbr); hipFree(A->loEnt); hipFree(A->faceSrc);
    hipFree(A->cellPerm); hipFree(A->callerToNative); hipFree(A->flowOrder);
    hipFree(A->grpCell); hipFree(A->sweepTicket); hipFree(A->rowSched);
    ffm_tile_free(A);
    hipFree(A->ghSendCells); hipFree(A->ghSendBuf); if (A->ghSendBuf_h) hipHostFree(A->ghSendBuf_h); if (A->ghRecvBuf_h) hipHostFree(A->ghRecvBuf_h);
    hipFree(A->diagBuf); hipFree(A->upperBuf); hipFree(A->lowerBuf); hipFree(A->rD);
    hipFree(A->ifFaceCells); hipFree(A->ifBou); hipFree(A->ifInt); hipFree(A->haloSend); hipFree(A->haloRecv);
    hipFree(A->ifCell); hipFree(A->ifCellStart); hipFree(A->ifItem);
    delete A;
    return FFM_OK;
}

extern "C" int ffm_ldu_ncells(const ffm_ldu *A) { return A ? A->nCells : FFM_ERR_ARG; }
extern "C" int ffm_ldu_sweep_mode(const ffm_ldu *A) { return !A ? FFM_ERR_ARG : A->sweepMode; }
extern "C" int ffm_ldu_nowned(const ffm_ldu *A) { return A ? A->nOwned : FFM_ERR_ARG; }
extern "C" int ffm_ldu_nfaces(const ffm_ldu *A) { return A ? A->nFaces : FFM_ERR_ARG; }
extern "C" int ffm_ldu_nlevels(const ffm_ldu *A) { return A ? A->nLevels : FFM_ERR_ARG; }
extern "C" int ffm_ldu_is_native_order(const ffm_ldu *A) { return A ? (A->identity ? 1 : 0) : FFM_ERR_ARG; }
extern "C" int ffm_ldu_get_cell_order(const ffm_ldu *A, int *newToOld)
{
    if (!A || !newToOld) return FFM_ERR_ARG;
    std::copy(A->h_newToOldCell.begin(), A->h_newToOldCell.end(), newToOld);
    return FFM_OK;
}
extern "C" int ffm_ldu_n_native_faces(const ffm_ldu *A) { return A ? A->upTotal : FFM_ERR_ARG; }
extern "C" int ffm_ldu_get_face_map(const ffm_ldu *A, int *callerToNative)
{
    if (!A || !callerToNative) return FFM_ERR_ARG;
    std::copy(A->h_callerToNative.begin(), A->h_callerToNative.end(), callerToNative);
    return FFM_OK;
}
extern "C" int ffm_ldu_set_global_cells(ffm_ldu *A, long g) { if (!A || g < A->nOwned) return FFM_ERR_ARG; A->globalCells = g; return FFM_OK; }
extern "C" long ffm_ldu_global_cells(const ffm_ldu *A) { return A ? A->globalCells : (long)FFM_ERR_ARG; }

int ffm_ldu_work(ffm_ldu *A, int idx, double **out)
{
    if (idx < 0 || idx > 31 + 9 * (FFM_TILE_MAXSYS - 1)) return FFM_ERR_ARG;          // 32 ..: the lanes of ffm_solve_multi_d
    if ((int)A->work.size() <= idx) A->work.resize(idx + 1, nullptr);
    if (!A->work[idx]) FFM_HIP(hipMalloc((void **)&A->work[idx], sizeof(double) * (size_t)std::max(A->nCells, 1)));
    *out = A->work[idx];
    return FFM_OK;
}

// ----------------------------------------------------- permutation kernels ---
__global__ void k_gather(long n, const int *__restrict__ perm, const double *__restrict__ src, double *__restrict__ dst)
{
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[perm[i]];
}
__global__ void k_scatter(long n, const int *__restrict__ perm, const double *__restrict__ src, double *__restrict__ dst)
{
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[perm[i]] = src[i];
}

static inline int stream_grid(long n) { long g = (n + 255) / 256; return (int)std::max(1L, std::min(g, (long)RED_BLOCKS)); }

int ffm_to_internal(ffm_ldu *A, const double *x_d, int slot, const double **out)
{
    if (A->identity) { *out = x_d; return FFM_OK; }
    if (!A->permIn[slot]) FFM_HIP(hipMalloc((void **)&A->permIn[slot], sizeof(double) * (size_t)std::max(A->nCells, 1)));
    hipLaunchKernelGGL(k_gather, dim3(stream_grid(A->nCells)), dim3(256), 0, A->ctx->stream, (long)A->nCells, A->cellPerm, x_d, A->permIn[slot]);
    *out = A->permIn[slot];
    return FFM_OK;
}
int ffm_from_internal(ffm_ldu *A, const double *xin, double *x_d)
{
    if (A->identity) {
        if (xin != x_d) FFM_HIP(hipMemcpyAsync(x_d, xin, sizeof(double) * A->nCells, hipMemcpyDeviceToDevice, A->ctx->stream));
        return FFM_OK;
    }
    hipLaunchKernelGGL(k_scatter, dim3(stream_grid(A->nCells)), dim3(256), 0, A->ctx->stream, (long)A->nCells, A->cellPerm, xin, x_d);
    return FFM_OK;
}

// gather with padding: dst[e] = (src_idx[e] >= 0) ? src[src_idx[e]] : 0   (LDU face order -> native faces)
__global__ void k_gather_faces(long n, const int *__restrict__ srcIdx, const double *__restrict__ src, double *__restrict__ dst)
{
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int f = srcIdx[i];
        dst[i] = (f >= 0) ? src[f] : 0.0;
    }
}

extern "C" int ffm_ldu_set_coeffs_d(ffm_ldu *A, const double *diag_d, const double *upper_d, const double *lower_d)
{
    if (!A || !diag_d || (A->nFaces && !upper_d)) return FFM_ERR_ARG;
    hipStream_t s = A->ctx->stream;
    const size_t nb = sizeof(double) * A->nCells, fb = sizeof(double) * std::max(A->upTotal, 1);
    A->diag = A->diagBuf; A->upper = A->upperBuf; A->directPending = false;
    if (lower_d && lower_d != upper_d) {
        if (!A->lowerBuf) FFM_HIP(hipMalloc((void **)&A->lowerBuf, fb));
        A->lower = A->lowerBuf; A->symmetric = false;
    } else { A->lower = A->upper; A->symmetric = true; }
    if (A->identity) { if (nb) FFM_HIP(hipMemcpyAsync(A->diag, diag_d, nb, hipMemcpyDeviceToDevice, s)); }
    else hipLaunchKernelGGL(k_gather, dim3(stream_grid(A->nCells)), dim3(256), 0, s, (long)A->nCells, A->cellPerm, diag_d, A->diag);
    if (A->upTotal) {
        hipLaunchKernelGGL(k_gather_faces, dim3(stream_grid(A->upTotal)), dim3(256), 0, s, (long)A->upTotal, A->faceSrc, upper_d, A->upper);
        if (!A->symmetric)
            hipLaunchKernelGGL(k_gather_faces, dim3(stream_grid(A->upTotal)), dim3(256), 0, s, (long)A->upTotal, A->faceSrc, lower_d, A->lower);
    }
    FFM_HIP(hipGetLastError());
    A->coeffEpoch++; A->offDiagEpoch++;
    return FFM_OK;
}

extern "C" int ffm_ldu_set_coeffs(ffm_ldu *A, const double *diag, const double *upper, const double *lower)
{
    if (!A || !diag || (A->nFaces && !upper)) return FFM_ERR_ARG;
    // stage through temporary device buffers (host pointers may be pageable)
    double *d = nullptr, *u = nullptr, *l = nullptr;
    const size_t nb = sizeof(double) * std::max(A->nCells, 1), fb = sizeof(double) * std::max(A->nFaces, 1);
    FFM_HIP(hipMalloc((void **)&d, nb)); FFM_HIP(hipMalloc((void **)&u, fb));
    if (lower) FFM_HIP(hipMalloc((void **)&l, fb));
    FFM_TRY(ffm_h2d(A->ctx, d, diag, sizeof(double) * A->nCells));
    if (A->nFaces) FFM_TRY(ffm_h2d(A->ctx, u, upper, sizeof(double) * A->nFaces));
    if (lower && A->nFaces) FFM_TRY(ffm_h2d(A->ctx, l, lower, sizeof(double) * A->nFaces));
    FFM_HIP(hipDeviceSynchronize());           // the null-stream uploads have landed before the context's (non-blocking) stream reads them
    int rc = ffm_ldu_set_coeffs_d(A, d, u, l);
    hipStreamSynchronize(A->ctx->stream);
    hipFree(d); hipFree(u); hipFree(l);
    return rc;
}

// native-layout entry for hosts that assemble directly in the library's face layout
extern "C" int ffm_ldu_set_coeffs_native_d(ffm_ldu *A, const double *diag_d, const double *upper_d, const double *lower_d)
{
    if (!A || !diag_d || (A->upTotal && !upper_d)) return FFM_ERR_ARG;
    if (!A->identity) { ffm_set_error("native coefficient layout needs the library's cell order (ffm_renumber_levels)"); return FFM_ERR_UNSUPPORTED; }
    hipStream_t s = A->ctx->stream;
    const size_t nb = sizeof(double) * A->nCells, fb = sizeof(double) * A->upTotal;
    A->diag = A->diagBuf; A->upper = A->upperBuf; A->directPending = false;
    if (lower_d && lower_d != upper_d) {
        if (!A->lowerBuf) FFM_HIP(hipMalloc((void **)&A->lowerBuf, std::max(fb, sizeof(double))));
        A->lower = A->lowerBuf; A->symmetric = false;
        if (fb) FFM_HIP(hipMemcpyAsync(A->lower, lower_d, fb, hipMemcpyDeviceToDevice, s));
    } else { A->lower = A->upper; A->symmetric = true; }
    if (nb) FFM_HIP(hipMemcpyAsync(A->diag, diag_d, nb, hipMemcpyDeviceToDevice, s));
    if (fb) FFM_HIP(hipMemcpyAsync(A->upper, upper_d, fb, hipMemcpyDeviceToDevice, s));
    A->coeffEpoch++; A->offDiagEpoch++;
    return FFM_OK;
}

// Zero-copy form: the matrix uses the caller's device arrays (native layout) until the next set / bind call; the caller keeps
// them alive and unchanged meanwhile.  offDiagUnchanged != 0: upper / lower hold the same values as at the previous call
// (e.g. the components of a vector equation, which differ in the boundary diagonal only), so layouts derived from them are kept.
// Arrays whose sweep layout the assembly kernel wrote beside them (ffm_tile_coef_written) bring it along: no gather for this epoch.
extern "C" int ffm_ldu_bind_coeffs_native_d(ffm_ldu *A, const double *diag_d, const double *upper_d, const double *lower_d,
                                            int offDiagUnchanged)
{
    if (!A || !diag_d || (A->upTotal && !upper_d)) return FFM_ERR_ARG;
    if (!A->identity) { ffm_set_error("native coefficient layout needs the library's cell order (ffm_renumber_levels)"); return FFM_ERR_UNSUPPORTED; }
    A->diag = const_cast<double *>(diag_d);
    A->upper = const_cast<double *>(upper_d ? upper_d : A->upperBuf);
    if (lower_d && lower_d != upper_d) { A->lower = const_cast<double *>(lower_d); A->symmetric = false; }
    else { A->lower = A->upper; A->symmetric = true; }
    A->coeffEpoch++;
    if (!offDiagUnchanged) A->offDiagEpoch++;
    const bool adopt = A->directPending && !offDiagUnchanged && upper_d == A->directUpper && (A->symmetric ? !A->directLower : lower_d == A->directLower);
    A->directPending = false;
    if (adopt) ffm_tile_coef_adopt(A);
    return FFM_OK;
}

// after a bind: the matrix points at its own coefficient buffers again (their contents are whatever the last set call left), so that
// nothing in the library refers to the caller's arrays once they are gone
extern "C" int ffm_ldu_unbind_coeffs(ffm_ldu *A)
{
    if (!A) return FFM_ERR_ARG;
    A->diag = A->diagBuf; A->upper = A->upperBuf; A->directPending = false;
    if (A->symmetric || !A->lowerBuf) { A->lower = A->upper; A->symmetric = true; } else A->lower = A->lowerBuf;
    // (the layouts derived from the off-diagonal coefficients stay as they are: a following bind with offDiagUnchanged != 0 -- the same
    // values again, e.g. the next specie sharing its coefficient arrays -- finds them current; any other set / bind renews them)
    A->coeffEpoch++;
    return FFM_OK;
}

extern "C" unsigned long ffm_ldu_offdiag_epoch(const ffm_ldu *A) { return A ? A->offDiagEpoch : 0ul; }

LduView ffm_view(const ffm_ldu *A)
{
    LduView v; v.N = A->nOwned; v.upOff = A->upOff; v.loOff = A->loOff; v.upNbr = A->upNbr; v.loEnt = A->loEnt; v.loShift = A->loShift;
    v.upW = A->upWidthUniform; v.loW = A->loWidthUniform; v.sched = A->rowSched; v.nSched = A->nSched;
    return v;
}

// ----------------------------------------------------------- lduMatrix::Amul ---
// One thread per row, grid-stride over a fixed grid; a wave = one slice, so all
// index/coefficient loads are unit-stride and the slot loops are wave-uniform.
// MODE 0: y = A x.  MODE 1: r = b - A x (lduMatrix::residual order).  MODE 2: s = sumA.
// MODE 3: y = A x and sumA (written through `partials`) in one pass over the coefficients -- the first two things every
// solver does with a freshly bound matrix (wA = A psi; normFactor needs sumA).
// DOT: additionally accumulates the block-partial of x[c]*y[c] (PCG's wApA).
template <int MODE, bool DOT, int W>
__global__ __launch_bounds__(256) void k_rows(LduView v, const double *__restrict__ diag,
                                              const double *__restrict__ upper, const double *__restrict__ lower,
                                              const double *__restrict__ x, const double *__restrict__ b,
                                              double *__restrict__ y, double *__restrict__ partials)
{
    __shared__ double sm[4];
    double dot = 0.0;
    for (int it = blockIdx.x; it < v.nSched; it += gridDim.x) {
        const int chunk = v.sched[it];
        const int c = chunk * 256 + (int)threadIdx.x;
        if (chunk < 0 || c >= v.N) continue;
        RowEnt<W> L, U;
        load_lower<W, true>(v, c, L);
        load_upper<W, false, true>(v, c, U);
        double al[W], au[W], xl[W], xu[W];
#pragma unroll
        for (int s = 0; s < W; s++) { al[s] = lower[L.f[s]]; au[s] = upper[U.f[s]]; }
        if (MODE != 2) {
#pragma unroll
            for (int s = 0; s < W; s++) { xl[s] = x[L.nb[s]]; xu[s] = x[U.nb[s]]; }
        }
        double xc = 0.0, acc;
        if (MODE != 2) xc = x[c];
        const double dc = __builtin_nontemporal_load(&diag[c]);
        double sum = dc;
        if (MODE == 0 || MODE == 3) acc = dc * xc;
        else if (MODE == 1) acc = __builtin_nontemporal_load(&b[c]) - dc * xc;
        else acc = dc;
#pragma unroll
        for (int s = 0; s < W; s++) if (L.on[s]) {
            if (MODE == 0 || MODE == 3) acc += al[s] * xl[s];
            else if (MODE == 1) acc -= al[s] * xl[s];
            else acc += al[s];
            if (MODE == 3) sum += al[s];
        }
#pragma unroll
        for (int s = 0; s < W; s++) if (U.on[s]) {
            if (MODE == 0 || MODE == 3) acc += au[s] * xu[s];
            else if (MODE == 1) acc -= au[s] * xu[s];
            else acc += au[s];
            if (MODE == 3) sum += au[s];
        }
        __builtin_nontemporal_store(acc, &y[c]);
        if (MODE == 3) __builtin_nontemporal_store(sum, &partials[c]);
        if (DOT) dot += acc * xc;
    }
    if (DOT) {
        double r = block_sum(dot, sm);
        if (threadIdx.x == 0) partials[blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(1024) void k_sum_partials(int n, const double *__restrict__ partials, double *__restrict__ scal, int slot, ffm_scal_op t)
{
    __shared__ double sm[16];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partials[i];
    double r = block_sum(acc, sm);
    if (threadIdx.x == 0) { scal[slot] = r; run_scal_op(scal, t); }
}

// grid of the row kernels: a multiple of 8 so that schedule entry i always meets blockIdx % 8 == i % 8
static inline int rows_grid(const ffm_ldu *A)
{
    // Fewer workgroups in flight on very large meshes: the rows in flight per XCD (grid/8 chunks of 256 rows, ~110 B each)
    // should not exceed the 4 MB L2 by much, or the neighbour gathers miss it (measured at 64 M rows: 1.16 ms with 1024
    // workgroups, 1.37 ms with 2048; below 10 M rows 2048 is marginally better)
    int g = std::min(A->nSched, A->nOwned >= (32 << 20) ? 1024 : RED_BLOCKS); g = (g + 7) & ~7; return std::max(g, 8);
}

// The Amul form of a matrix: the tiled kernel of a symmetric matrix, the tiled kernel of an asymmetric one (not for Tmul),
// or the row kernel.  FFM_NO_TILE_AMUL is read on every call: tests switch it between two Amuls of the same matrix.
enum AmulForm { AMUL_ROWS, AMUL_TILE_SYM, AMUL_TILE_ASYM };
static AmulForm amul_form(const ffm_ldu *A, bool transpose)
{
    if (ffm_tile_amul_usable(A) && !getenv("FFM_NO_TILE_AMUL")) return AMUL_TILE_SYM;
    if (!transpose && ffm_tile_amul_asym_usable(A)) return AMUL_TILE_ASYM;
    return AMUL_ROWS;
}

int ffm_k_spmv(ffm_ldu *A, const double *x, double *y, bool transpose)
{
    const double *up = transpose ? A->lower : A->upper, *lo = transpose ? A->upper : A->lower;
    const AmulForm form = amul_form(A, transpose);
    if (form == AMUL_TILE_SYM) {
        // the tiled kernel computes the rows without their ghost faces: the ghost refresh overlaps it and is waited for by the tail
        if (!A->ghNbrRank.empty()) FFM_TRY(ffm_ghost_exchange_begin(A, const_cast<double *>(x)));
        FFM_TRY(ffm_tile_amul(A, x, y, -1));
        return FFM_OK;
    }
    if (form == AMUL_TILE_ASYM) {
        if (!A->ghNbrRank.empty()) FFM_TRY(ffm_ghost_exchange_begin(A, const_cast<double *>(x)));
        return ffm_tile_amul_asym(A, x, y);
    }
    if (!A->ghNbrRank.empty()) FFM_TRY(ffm_ghost_exchange(A, const_cast<double *>(x)));   // refresh ghost columns
    FFM_DISPATCH_W(A->maxW, hipLaunchKernelGGL((k_rows<0, false, W>), dim3(rows_grid(A)), dim3(256), 0, A->ctx->stream, ffm_view(A),
                                               A->diag, up, lo, x, (const double *)nullptr, y, (double *)nullptr));
    FFM_HIP(hipGetLastError());
    if (!A->ifaces.empty()) FFM_TRY(ffm_halo_update(A, x, y, transpose ? A->ifInt : A->ifBou, -1.0));
    return FFM_OK;
}

// y_i = A_i x_i for NF matrices with the off-diagonal coefficients upper / lower and their own diagonals (the lanes of
// ffm_solve_multi_d): addressing and coefficients are read once per row; per system the row sum is k_rows<0> / <3>, term for term.
template <int NF> struct RowsMulti { const double *diag[NF], *x[NF]; double *y[NF], *sum[NF]; };
template <int MODE, int NF, int W>
__global__ __launch_bounds__(256) void k_rows_m(LduView v, const double *__restrict__ upper, const double *__restrict__ lower, RowsMulti<NF> m)
{
    for (int it = blockIdx.x; it < v.nSched; it += gridDim.x) {
        const int chunk = v.sched[it];
        const int c = chunk * 256 + (int)threadIdx.x;
        if (chunk < 0 || c >= v.N) continue;
        RowEnt<W> L, U;
        load_lower<W, true>(v, c, L);
        load_upper<W, false, true>(v, c, U);
        double al[W], au[W];
#pragma unroll
        for (int s = 0; s < W; s++) { al[s] = lower[L.f[s]]; au[s] = upper[U.f[s]]; }
#pragma unroll
        for (int i = 0; i < NF; i++) {
            const double *__restrict__ x = m.x[i];
            double xl[W], xu[W];
#pragma unroll
            for (int s = 0; s < W; s++) { xl[s] = x[L.nb[s]]; xu[s] = x[U.nb[s]]; }
            const double xc = x[c], dc = __builtin_nontemporal_load(&m.diag[i][c]);
            double acc = dc * xc, sum = dc;
#pragma unroll
            for (int s = 0; s < W; s++) if (L.on[s]) { acc += al[s] * xl[s]; if (MODE == 3) sum += al[s]; }
#pragma unroll
            for (int s = 0; s < W; s++) if (U.on[s]) { acc += au[s] * xu[s]; if (MODE == 3) sum += au[s]; }
            __builtin_nontemporal_store(acc, &m.y[i][c]);
            if (MODE == 3) __builtin_nontemporal_store(sum, &m.sum[i][c]);
        }
    }
}
template <int MODE, int NF>
static void rows_multi_launch(ffm_ldu *A, const double *const *diag, const double *const *x, double *const *y, double *const *sumA)
{
    RowsMulti<NF> m;
    for (int i = 0; i < NF; i++) { m.diag[i] = diag[i]; m.x[i] = x[i]; m.y[i] = y[i]; m.sum[i] = sumA ? sumA[i] : nullptr; }
    FFM_DISPATCH_W(A->maxW, hipLaunchKernelGGL((k_rows_m<MODE, NF, W>), dim3(rows_grid(A)), dim3(256), 0, A->ctx->stream, ffm_view(A),
                                               (const double *)A->upper, (const double *)A->lower, m));
}
// n = 2 .. FFM_TILE_MAXSYS systems; sumA != NULL: also sumA[i] = the row sums of system i (lduMatrix::sumA).  Matrices without coupled patches.
int ffm_k_spmv_multi(ffm_ldu *A, int n, const double *const *diag, const double *const *x, double *const *y, double *const *sumA)
{
    if (n < 2 || n > FFM_TILE_MAXSYS || !A->ifaces.empty()) return FFM_ERR_ARG;
    if (!A->ghNbrRank.empty()) for (int i = 0; i < n; i++) FFM_TRY(ffm_ghost_exchange(A, const_cast<double *>(x[i])));
    if (sumA) { if (n == 2) rows_multi_launch<3, 2>(A, diag, x, y, sumA); else if (n == 3) rows_multi_launch<3, 3>(A, diag, x, y, sumA); else if (n == 4) rows_multi_launch<3, 4>(A, diag, x, y, sumA); else rows_multi_launch<3, 5>(A, diag, x, y, sumA); }
    else { if (n == 2) rows_multi_launch<0, 2>(A, diag, x, y, sumA); else if (n == 3) rows_multi_launch<0, 3>(A, diag, x, y, sumA); else if (n == 4) rows_multi_launch<0, 4>(A, diag, x, y, sumA); else rows_multi_launch<0, 5>(A, diag, x, y, sumA); }
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

int ffm_k_spmv_dot(ffm_ldu *A, const double *x, double *y, int slot, const ffm_scal_op &t)
{
    if (!A->ifaces.empty()) {  // the halo term changes y after the row kernel: separate dot
        FFM_TRY(ffm_k_spmv(A, x, y, false));
        return ffm_k_dot(A->ctx, y, x, A->nOwned, slot, t);
    }
    if (amul_form(A, false) == AMUL_TILE_SYM) {
        if (!A->ghNbrRank.empty()) FFM_TRY(ffm_ghost_exchange_begin(A, const_cast<double *>(x)));
        const int rc = ffm_tile_amul(A, x, y, slot, t);
        if (rc == 1) return ffm_k_dot(A->ctx, y, x, A->nOwned, slot, t);      // ghost faces were added after the tiled kernel
        return rc;
    }
    if (!A->ghNbrRank.empty()) FFM_TRY(ffm_ghost_exchange(A, const_cast<double *>(x)));
    const int g = rows_grid(A);
    FFM_DISPATCH_W(A->maxW, hipLaunchKernelGGL((k_rows<0, true, W>), dim3(g), dim3(256), 0, A->ctx->stream, ffm_view(A), A->diag,
                                               A->upper, A->lower, x, (const double *)nullptr, y, A->ctx->partials_d));
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, A->ctx->stream, g, A->ctx->partials_d, A->ctx->scal_d, slot, t);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

int ffm_k_residual(ffm_ldu *A, const double *x, const double *b, double *r)
{
    if (!A->ghNbrRank.empty()) FFM_TRY(ffm_ghost_exchange(A, const_cast<double *>(x)));
    FFM_DISPATCH_W(A->maxW, hipLaunchKernelGGL((k_rows<1, false, W>), dim3(rows_grid(A)), dim3(256), 0, A->ctx->stream, ffm_view(A),
                                               A->diag, A->upper, A->lower, x, b, r, (double *)nullptr));
    FFM_HIP(hipGetLastError());
    if (!A->ifaces.empty()) FFM_TRY(ffm_halo_update(A, x, r, A->ifBou, +1.0));
    return FFM_OK;
}

// y = A x and s = sumA of the same matrix: one pass where the row kernel does the Amul, two where the tiled kernel does
int ffm_k_spmv_sumA(ffm_ldu *A, const double *x, double *y, double *s)
{
    if (amul_form(A, false) == AMUL_TILE_SYM) {
        FFM_TRY(ffm_k_spmv(A, x, y, false));
        return ffm_k_sumA(A, s);
    }
    if (!A->ghNbrRank.empty()) FFM_TRY(ffm_ghost_exchange(A, const_cast<double *>(x)));
    FFM_DISPATCH_W(A->maxW, hipLaunchKernelGGL((k_rows<3, false, W>), dim3(rows_grid(A)), dim3(256), 0, A->ctx->stream, ffm_view(A),
                                               A->diag, A->upper, A->lower, x, (const double *)nullptr, y, s));
    FFM_HIP(hipGetLastError());
    if (!A->ifaces.empty()) {
        FFM_TRY(ffm_halo_update(A, x, y, A->ifBou, -1.0));
        FFM_TRY(ffm_halo_apply(A, s, A->ifBou, nullptr, -1.0));
    }
    return FFM_OK;
}

// The row kernels over this rank's rows as they stand: no ghost refresh, so no rank waits for another.  For a matrix whose faces
// towards ghost cells carry zero coefficients (the staged fvDOM ray solves: their terms have been moved into the source).
int ffm_k_spmv_sumA_rows(ffm_ldu *A, const double *x, double *y, double *s)
{
    FFM_DISPATCH_W(A->maxW, hipLaunchKernelGGL((k_rows<3, false, W>), dim3(rows_grid(A)), dim3(256), 0, A->ctx->stream, ffm_view(A),
                                               A->diag, A->upper, A->lower, x, (const double *)nullptr, y, s));
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}
int ffm_k_residual_rows(ffm_ldu *A, const double *x, const double *b, double *r)
{
    FFM_DISPATCH_W(A->maxW, hipLaunchKernelGGL((k_rows<1, false, W>), dim3(rows_grid(A)), dim3(256), 0, A->ctx->stream, ffm_view(A),
                                               A->diag, A->upper, A->lower, x, b, r, (double *)nullptr));
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

int ffm_k_sumA(ffm_ldu *A, double *s)
{
    FFM_DISPATCH_W(A->maxW, hipLaunchKernelGGL((k_rows<2, false, W>), dim3(rows_grid(A)), dim3(256), 0, A->ctx->stream, ffm_view(A),
                                               A->diag, A->upper, A->lower, (const double *)nullptr, (const double *)nullptr, s,
                                               (double *)nullptr));
    FFM_HIP(hipGetLastError());
    // coupled patches: sumA[faceCells] -= interfaceBouCoeffs
    if (!A->ifaces.empty()) FFM_TRY(ffm_halo_apply(A, s, A->ifBou, nullptr, -1.0));
    return FFM_OK;
}

// ------------------------------------------------------------- public entry ---
extern "C" int ffm_spmv(ffm_ldu *A, const double *x_d, double *y_d)
{
    if (!A || !x_d || !y_d) return FFM_ERR_ARG;
    const double *xi; FFM_TRY(ffm_to_internal(A, x_d, 0, &xi));
    if (A->identity) return ffm_k_spmv(A, xi, y_d, false);
    double *yi; FFM_TRY(ffm_ldu_work(A, 0, &yi));
    FFM_TRY(ffm_k_spmv(A, xi, yi, false));
    return ffm_from_internal(A, yi, y_d);
}
extern "C" int ffm_tmul(ffm_ldu *A, const double *x_d, double *y_d)
{
    if (!A || !x_d || !y_d) return FFM_ERR_ARG;
    const double *xi; FFM_TRY(ffm_to_internal(A, x_d, 0, &xi));
    if (A->identity) return ffm_k_spmv(A, xi, y_d, true);
    double *yi; FFM_TRY(ffm_ldu_work(A, 0, &yi));
    FFM_TRY(ffm_k_spmv(A, xi, yi, true));
    return ffm_from_internal(A, yi, y_d);
}
extern "C" int ffm_sumA(ffm_ldu *A, double *s_d)
{
    if (!A || !s_d) return FFM_ERR_ARG;
    if (A->identity) return ffm_k_sumA(A, s_d);
    double *si; FFM_TRY(ffm_ldu_work(A, 0, &si));
    FFM_TRY(ffm_k_sumA(A, si));
    return ffm_from_internal(A, si, s_d);
}
extern "C" int ffm_residual(ffm_ldu *A, const double *x_d, const double *b_d, double *r_d)
{
    if (!A || !x_d || !b_d || !r_d) return FFM_ERR_ARG;
    const double *xi, *bi;
    FFM_TRY(ffm_to_internal(A, x_d, 0, &xi)); FFM_TRY(ffm_to_internal(A, b_d, 1, &bi));
    if (A->identity) return ffm_k_residual(A, xi, bi, r_d);
    double *ri; FFM_TRY(ffm_ldu_work(A, 0, &ri));
    FFM_TRY(ffm_k_residual(A, xi, bi, ri));
    return ffm_from_internal(A, ri, r_d);
}

extern "C" int ffm_bench_spmv(ffm_ldu *A, const double *x_d, double *y_d, int reps, double *avg_ms)
{
    if (!A || !x_d || !y_d || reps < 1 || !avg_ms) return FFM_ERR_ARG;
    if (!A->identity) { ffm_set_error("ffm_bench_spmv needs a level-major (native order) LDU"); return FFM_ERR_UNSUPPORTED; }
    hipEvent_t e0, e1;
    FFM_HIP(hipEventCreate(&e0)); FFM_HIP(hipEventCreate(&e1));
    FFM_TRY(ffm_k_spmv(A, x_d, y_d, false));  // warm-up
    FFM_HIP(hipEventRecord(e0, A->ctx->stream));
    for (int i = 0; i < reps; i++) FFM_TRY(ffm_k_spmv(A, x_d, y_d, false));
    FFM_HIP(hipEventRecord(e1, A->ctx->stream));
    FFM_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    FFM_HIP(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0); hipEventDestroy(e1);
    *avg_ms = (double)ms / reps;
    return FFM_OK;
}
