// ffm_device.hpp -- device-side helpers shared by the kernels (wave64 only), and the host-side launch grid of the element kernels.
#pragma once
#include <hip/hip_runtime.h>
#include "ffm_internal.hpp"

// grid of the grid-stride element kernels: 256 threads per block, at most RED_BLOCKS blocks
static inline int sgrid(long n) { long g = (n + 255) / 256; return (int)std::max(1L, std::min(g, (long)RED_BLOCKS)); }

// wave64 butterfly-free, order-fixed reductions: lane 0 ends with the result.
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_min(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_down(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    return v;
}

// Block reductions (blockDim.x a multiple of 64, <= 1024).  Result valid in
// thread 0.  sm must hold blockDim.x/64 doubles.  Waves are added in wave order.
__device__ __forceinline__ double block_sum(double v, double *sm)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        const int nw = blockDim.x >> 6;
        for (int i = 0; i < nw; i++) r += sm[i];
    }
    return r;
}
__device__ __forceinline__ double block_min(double v, double *sm)
{
    v = wave_min(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[w] = v;
    __syncthreads();
    double r = v;
    if (threadIdx.x == 0) {
        const int nw = blockDim.x >> 6;
        r = sm[0];
        for (int i = 1; i < nw; i++) r = fmin(r, sm[i]);
    }
    return r;
}
__device__ __forceinline__ double block_max(double v, double *sm)
{
    v = wave_max(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[w] = v;
    __syncthreads();
    double r = v;
    if (threadIdx.x == 0) {
        const int nw = blockDim.x >> 6;
        r = sm[0];
        for (int i = 1; i < nw; i++) r = fmax(r, sm[i]);
    }
    return r;
}

// --------------------------------------------------------------- scalar ops ---
// The solvers' scalar operations on the device scalar block (ffm_solve.hip).  One thread runs one: k_scalar_op as a launch of its
// own, or thread 0 of the one-workgroup launch that has just stored the sum the operation starts from (run_scal_op).
enum {
    OP_XREF = 1, OP_NORMF, OP_RES_INIT, OP_RES, OP_PCG_BETA, OP_PCG_ALPHA,
    OP_BS_RHO, OP_BS_ALPHA, OP_BS_OMEGA, OP_BICG_BETA, OP_BICG_ALPHA, OP_RESET
};

#define VSMALL_ 1e-300

// in: the slot the operation takes its sum from (the prologue kernel leaves three sums in S_TMP0..S_TMP2).  No __restrict__: the
// launches that sum partials store into s just before.
__device__ __forceinline__ void scalar_op_body(double *s, int op, double arg, int iter, int in)
{
    switch (op) {
    case OP_RESET:
        s[S_SING] = 0.0; s[S_WARA] = 1e+20; s[S_WARA_OLD] = 1e+20; s[S_RA0RA] = 0.0; s[S_ALPHA] = 0.0; s[S_OMEGA] = 0.0;
        s[S_BETA] = 0.0;
        break;
    case OP_XREF: s[S_XREF] = s[S_TMP0] / arg; break;                    // gAverage(psi)
    case OP_NORMF: s[S_NORMF] = s[S_TMP0] + 1e-20; break;                // + solverPerformance::small_
    case OP_RES_INIT: s[S_RES] = s[in] / s[S_NORMF]; s[S_RES0] = s[S_RES]; break;
    case OP_RES: if (s[S_SING] == 0.0) s[S_RES] = s[S_TMP0] / s[S_NORMF]; break;
    case OP_PCG_BETA: {                                                  // wArAold = wArA; wArA = (wA,rA)
        const double old = s[S_WARA], nw = s[S_TMP0];
        s[S_WARA_OLD] = old; s[S_WARA] = nw; s[S_BETA] = nw / old;
        break; }
    case OP_PCG_ALPHA: case OP_BICG_ALPHA: {                             // wApA; checkSingularity(|wApA|/normFactor)
        const double wApA = s[S_TMP0];
        s[S_WAPA] = wApA;
        if (fabs(wApA) / s[S_NORMF] > VSMALL_) { s[S_ALPHA] = s[S_WARA] / wApA; }
        else { s[S_SING] = 1.0; s[S_ALPHA] = 0.0; }
        break; }
    case OP_BS_RHO: {                                                    // rA0rAold = rA0rA; rA0rA = (rA0,rA)
        const double old = s[S_RA0RA], nw = s[in];
        s[S_RA0RA_OLD] = old; s[S_RA0RA] = nw;
        if (!(fabs(nw) > VSMALL_)) { s[S_SING] = 1.0; break; }
        if (iter > 0) {
            if (!(fabs(s[S_OMEGA]) > VSMALL_)) { s[S_SING] = 1.0; break; }
            s[S_BETA] = (nw / old) * (s[S_ALPHA] / s[S_OMEGA]);
        }
        break; }
    case OP_BS_ALPHA: if (s[S_SING] == 0.0) { s[S_RA0AYA] = s[S_TMP0]; s[S_ALPHA] = s[S_RA0RA] / s[S_TMP0]; } break;
    case OP_BS_OMEGA: if (s[S_SING] == 0.0) { s[S_TATA] = s[S_TMP0]; s[S_TASA] = s[S_TMP1]; s[S_OMEGA] = s[S_TMP1] / s[S_TMP0]; } break;
    case OP_BICG_BETA: {
        const double old = s[S_WARA], nw = s[S_TMP0];
        s[S_WARA_OLD] = old; s[S_WARA] = nw; s[S_BETA] = nw / old;
        break; }
    }
}
// the tail of a launch that sums partials into the scalar block: called by the thread that stored the sum(s), after the store
__device__ __forceinline__ void run_scal_op(double *scal, const ffm_scal_op &t)
{
    if (t.fused) scalar_op_body(scal, t.op, t.arg, t.iter, t.in);
}

// ------------------------------------------------------ sliced owner-ELL view ---
// Passed by value to every kernel that walks matrix rows (layout: ffm_internal.hpp).
struct LduView {
    int N;                      // number of ROWS (owned cells); column indices may reach the ghost cells beyond
    int loShift;                // bits of the slot field of a lower entry (4, or 5 for a matrix with more than 16 owned upper faces in a row)
    const int *upOff, *loOff;   // [nSlices+1]
    const int *upNbr;           // [upTotal]
    const int *loEnt;           // [loTotal]
    int upW;                    // uniform upper width of every slice, or -1
    int loW;                    // uniform lower width of every slice, or -1
    const int *sched; int nSched;   // XCD-aware chunk schedule of the row kernels (256 rows per chunk)
};

// first native face index of the slice of cell c
__device__ __forceinline__ int up_base(const LduView &v, int sl) { return v.upW >= 0 ? sl * v.upW * 64 : v.upOff[sl]; }
__device__ __forceinline__ int up_width(const LduView &v, int sl) { return v.upW >= 0 ? v.upW : (v.upOff[sl + 1] - v.upOff[sl]) >> 6; }
__device__ __forceinline__ int lo_base(const LduView &v, int sl) { return v.loW >= 0 ? sl * v.loW * 64 : v.loOff[sl]; }
__device__ __forceinline__ int lo_width(const LduView &v, int sl) { return v.loW >= 0 ? v.loW : (v.loOff[sl + 1] - v.loOff[sl]) >> 6; }
// native face index of slot `slot` in the row of cell `cell`
__device__ __forceinline__ int face_of(const LduView &v, int cell, int slot) { return up_base(v, cell >> 6) + slot * 64 + (cell & 63); }

// Row loaders: fetch all lower / upper entries of the row of cell c into registers with
// predicated, fully unrolled loads (W = compile-time bound on the slot count), so that the
// index loads of all slots are in flight together and the dependent gathers likewise: a row
// costs two memory round trips instead of two per slot.  Padding slots point at harmless
// addresses (own cell, face 0) and are masked out of the arithmetic.  s0: the first slot to load (a kernel that walks a wide row
// in chunks of W slots).
template <int W> struct RowEnt { int nb[W]; int f[W]; bool on[W]; };

// NT: index streams are read once per kernel -- load them non-temporally so they do not evict the gather targets
// (x, coefficients) from the XCD's L2
template <int W, bool NT = false>
__device__ __forceinline__ void load_lower(const LduView &v, int c, RowEnt<W> &R, int s0 = 0)
{
    const int sl = c >> 6, lane = c & 63;
    const int lb = lo_base(v, sl) + s0 * 64, lw = lo_width(v, sl) - s0;
    int e[W];
#pragma unroll
    for (int s = 0; s < W; s++) e[s] = (s < lw) ? (NT ? __builtin_nontemporal_load(&v.loEnt[lb + s * 64 + lane]) : v.loEnt[lb + s * 64 + lane]) : -1;
#pragma unroll
    for (int s = 0; s < W; s++) {
        R.on[s] = e[s] >= 0;
        R.nb[s] = R.on[s] ? (e[s] >> v.loShift) : c;
        R.f[s] = R.on[s] ? face_of(v, R.nb[s], (int)__builtin_amdgcn_ubfe((unsigned)e[s], 0u, (unsigned)v.loShift)) : 0;   // the low loShift bits
    }
}

// MASK_GHOST: drop upper neighbours that are ghost cells (index >= v.N): block-Jacobi sweeps
template <int W, bool MASK_GHOST = false, bool NT = false>
__device__ __forceinline__ void load_upper(const LduView &v, int c, RowEnt<W> &R, int s0 = 0)
{
    const int sl = c >> 6, lane = c & 63;
    const int ub = up_base(v, sl) + s0 * 64, uw = up_width(v, sl) - s0;
#pragma unroll
    for (int s = 0; s < W; s++) {
        const int idx = ub + s * 64 + lane;
        const int n = (s < uw) ? (NT ? __builtin_nontemporal_load(&v.upNbr[idx]) : v.upNbr[idx]) : -1;
        R.on[s] = n >= 0 && (!MASK_GHOST || n < v.N);
        R.nb[s] = R.on[s] ? n : c;
        R.f[s] = R.on[s] ? idx : 0;
    }
}

// The tiled sweeps read a matrix's off-diagonal coefficients as cell-major triples (ffm_tile.hip: TileDir::coefU / coefL): slot k of
// cell c holds the k-th PRESENT entry of the row, in row order, absent slots 0.0 (k_tile_gather's layout, byte for byte).  A kernel
// that assembles the matrix has a row's values in registers and stores the triple itself: v[s] is the coefficient of row slot s
// (anything where !on[s]).  Selects, no indexed temporaries; one 24-byte record per lane, consecutive lanes consecutive records.
struct TileCoefOut { double *fU, *fL, *bU; };       // forward upper / lower (fL null: symmetric), backward upper
__device__ __forceinline__ void store_triple(double *__restrict__ out, int c, const bool (&on)[FFM_TILE_W], const double (&v)[FFM_TILE_W])
{
    static_assert(FFM_TILE_W == 3, "three slots per direction");
    const double t12 = on[1] ? v[1] : (on[2] ? v[2] : 0.0);                    // first present of slots 1, 2
    const double k0 = on[0] ? v[0] : t12;
    const double k1 = on[0] ? t12 : ((on[1] && on[2]) ? v[2] : 0.0);
    const double k2 = (on[0] && on[1] && on[2]) ? v[2] : 0.0;
    double *o = out + 3 * (size_t)c;
    o[0] = k0; o[1] = k1; o[2] = k2;
}

// (W = 3: hexahedral meshes -- at most 3 lower and 3 upper neighbours per cell -- get their own instantiation: a quarter fewer
// predicated slot loads and registers than W = 4 in every row kernel)
#define FFM_DISPATCH_W(maxW, CALL)                      \
    do {                                                \
        if ((maxW) <= 3) { constexpr int W = 3; CALL; } \
        else if ((maxW) <= 4) { constexpr int W = 4; CALL; } \
        else if ((maxW) <= 8) { constexpr int W = 8; CALL; } \
        else if ((maxW) <= 16) { constexpr int W = 16; CALL; } \
        else { constexpr int W = 32; CALL; }            \
    } while (0)
