// ffm_solve.hip -- DIC / DILU / Gauss-Seidel sweeps of level-scheduled matrices and the
// PCG / PBiCGStab / PBiCG / smoothSolver / diagonalSolver drivers.
//
// Replaces (OpenFOAM-dev @940e28f, not vendored in the reference):
//   .../lduMatrix/preconditioners/{DIC,DILU}Preconditioner/*.C
//   .../lduMatrix/smoothers/{GaussSeidel,symGaussSeidel}/*.C
//   .../lduMatrix/solvers/{PCG,PBiCGStab,PBiCG,smoothSolver,diagonalSolver}/*.C
// selected by the reference in cases/steckler/system/fvSolution:21-61 and
// cases/wallFireSpread2D/system/fvSolution:115-152; entered from
// solver/pEqn.H:39, solver/UEqn.H:19, solver/YEEqn.H:60,111, solver/rhoEqn.H:43.
//
// Exactness: the serial face-order sweeps of the reference carry a dependency
// DAG (owner -> neighbour).  Every sweep has one form per sweep mode: matrices
// with a tile plan (sweepMode 2) take the tiled wavefront sweeps of
// ffm_tile.hip; all others -- unstructured meshes, GAMG coarse levels,
// FFM_SWEEP=levels -- the dataflow sweeps below: cells stored level-major, ONE
// launch per sweep (pair) in which every cell waits for the values it needs.
// Every row is accumulated in the reference's face order, and the library is
// compiled with -ffp-contract=off, so the sweeps are bitwise equal to the
// serial loops; only the dot products (two-stage tree sums instead of one
// serial sum) differ, in the last bits.
//
// Scalars (alpha, beta, residual norms) stay on the device; the host reads the
// residual back once per iteration (twice for PBiCGStab) to take the
// convergence decision, as SolverPerformance::checkConvergence does.
//
// PBiCGStab is written once, over lanes (pbicgstab_lanes): a lane is one system's solver state, a plain solve is the
// single lane that is the matrix's own state, and ffm_solve_multi_d runs up to FFM_TILE_MAXSYS lanes in lock step.
#include "ffm_internal.hpp"
#include "ffm_device.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>


// --------------------------------------------------------------- scalar ops ---
// (the operations: ffm_device.hpp, scalar_op_body)
__global__ void k_scalar_op(double *s, int op, double arg, int iter, int in)
{
    if (threadIdx.x || blockIdx.x) return;
    scalar_op_body(s, op, arg, iter, in);
}

static int scalar_op(ffm_ctx *c, int op, double arg = 0.0, int iter = 0, int in = S_TMP0)
{
    hipLaunchKernelGGL(k_scalar_op, dim3(1), dim3(64), 0, c->stream, c->scal_d, op, arg, iter, in);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}
// The operation that follows a reduction.  One rank: it rides on the reduction's one-workgroup launch that sums the partials (the
// reduction calls take it as their last argument) and finish_dot has nothing left to do.  More ranks: the local sum sits in
// S_TMP0(..S_TMP0+n-1), finish_dot adds the ranks' and then derives, in a launch of its own.
static ffm_scal_op tail_op(ffm_ctx *c, int op, double arg = 0.0, int iter = 0)
{
    ffm_scal_op t; t.op = op; t.arg = arg; t.iter = iter; t.fused = c->nRanks == 1 && !c->comm;
    return t;
}
static int finish_dot(ffm_ctx *c, const ffm_scal_op &t, int nSlots = 1)
{
    if (t.fused) return FFM_OK;
    FFM_TRY(ffm_allreduce_slots(c, S_TMP0, nSlots));
    return scalar_op(c, t.op, t.arg, t.iter);
}

// ----------------------------------------------------------- vector kernels ---
#define GRID_STRIDE(i, n) for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

__global__ void k_sub(long n, double *__restrict__ r, const double *__restrict__ b, const double *__restrict__ w)
{ GRID_STRIDE(i, n) r[i] = b[i] - w[i]; }


__global__ void k_copy(long n, double *__restrict__ d, const double *__restrict__ s)
{ GRID_STRIDE(i, n) d[i] = s[i]; }

// The prologue of a solve once xRef is known, one pass over Apsi, source and sumA:
//   r = source - Apsi;  partials[0..] = the normFactor sum |Apsi - xRef*sumA| + |source - xRef*sumA|;  partials[RED_BLOCKS..] = sum |r|;
//   BS (PBiCGStab): also partials[2*RED_BLOCKS..] = rA0.rA = sum r*r.  There r is rA0: at iteration 0 rA, rA0 and the search
//   direction pA are one vector, which is written once and read under all three names (pbicgstab_lanes).
// Grid, block, stride and block_sum are those of the reductions of ffm_ctx.hip (k_reduce1), so every sum keeps its partition and
// its tree.
template <bool BS>
__global__ __launch_bounds__(256) void k_prologue(long n, const double *__restrict__ Ax, const double *__restrict__ b,
                                                  const double *__restrict__ sumA, const double *__restrict__ scal, double *__restrict__ r,
                                                  double *__restrict__ partials)
{
    __shared__ double sm[4];
    const double xRef = scal[S_XREF];
    double accN = 0.0, accR = 0.0, accD = 0.0;
    GRID_STRIDE(i, n) {
        const double ax = Ax[i], bi = b[i], t = sumA[i] * xRef;
        const double ri = bi - ax;
        accN += fabs(ax - t) + fabs(bi - t);
        accR += fabs(ri);
        r[i] = ri;
        if (BS) accD += ri * ri;
    }
    const double sN = block_sum(accN, sm);
    const double sR = block_sum(accR, sm);
    const double sD = BS ? block_sum(accD, sm) : 0.0;
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = sN; partials[RED_BLOCKS + blockIdx.x] = sR;
        if (BS) partials[2 * RED_BLOCKS + blockIdx.x] = sD;
    }
}

// pA = first ? wA : wA + beta*pA
__global__ void k_p_update(long n, double *__restrict__ p, const double *__restrict__ w, const double *__restrict__ scal, int first)
{
    if (scal[S_SING] != 0.0) return;
    const double beta = scal[S_BETA];
    if (first) { GRID_STRIDE(i, n) p[i] = w[i]; }
    else { GRID_STRIDE(i, n) p[i] = w[i] + beta * p[i]; }
}

// fused PCG: psi += alpha*pA (the update left over from the iteration before), then pA = wA + beta*pA
__global__ void k_p_psi(long n, double *__restrict__ psi, double *__restrict__ p, const double *__restrict__ w, const double *__restrict__ scal)
{
    if (scal[S_SING] != 0.0) return;
    const double alpha = scal[S_ALPHA], beta = scal[S_BETA];
    GRID_STRIDE(i, n) { const double pi = p[i]; psi[i] += alpha * pi; p[i] = w[i] + beta * pi; }
}

// psi += alpha*pA; rA -= alpha*wA; partial sum |rA|      (PCG)
__global__ __launch_bounds__(256) void k_pcg_xr(long n, double *__restrict__ psi, double *__restrict__ r,
                                                const double *__restrict__ p, const double *__restrict__ w,
                                                const double *__restrict__ scal, double *__restrict__ partials)
{
    __shared__ double sm[4];
    const double alpha = scal[S_ALPHA];
    const bool sing = scal[S_SING] != 0.0;
    double acc = 0.0;
    GRID_STRIDE(i, n) {
        double ri = r[i];
        if (!sing) { psi[i] += alpha * p[i]; ri -= alpha * w[i]; r[i] = ri; }
        acc += fabs(ri);
    }
    const double s = block_sum(acc, sm);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// PBiCG extra: rT -= alpha*wT
__global__ void k_axmy_alpha(long n, double *__restrict__ r, const double *__restrict__ w, const double *__restrict__ scal)
{
    if (scal[S_SING] != 0.0) return;
    const double alpha = scal[S_ALPHA];
    GRID_STRIDE(i, n) r[i] -= alpha * w[i];
}

// PBiCGStab: pA = rA + beta*(pOld - omega*AyA).  pOld is pA itself (an element is loaded before it is stored: no __restrict__ on
// the two) except at iteration 1, where the direction of iteration 0 is rA0 (k_prologue).
__global__ void k_bs_p(long n, double *p, const double *pOld, const double *__restrict__ r, const double *__restrict__ AyA,
                       const double *__restrict__ scal)
{
    if (scal[S_SING] != 0.0) return;
    const double beta = scal[S_BETA], omega = scal[S_OMEGA];
    GRID_STRIDE(i, n) p[i] = r[i] + beta * (pOld[i] - omega * AyA[i]);
}

// sA = rA - alpha*AyA; partial |sA|
__global__ __launch_bounds__(256) void k_bs_s(long n, double *__restrict__ sA, const double *__restrict__ r,
                                              const double *__restrict__ AyA, const double *__restrict__ scal,
                                              double *__restrict__ partials)
{
    __shared__ double sm[4];
    const double alpha = scal[S_ALPHA];
    const bool sing = scal[S_SING] != 0.0;
    double acc = 0.0;
    if (!sing) GRID_STRIDE(i, n) { const double v = r[i] - alpha * AyA[i]; sA[i] = v; acc += fabs(v); }
    const double s = block_sum(acc, sm);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// psi += alpha*yA
__global__ void k_axpy_alpha(long n, double *__restrict__ psi, const double *__restrict__ y, const double *__restrict__ scal)
{
    const double alpha = scal[S_ALPHA];
    GRID_STRIDE(i, n) psi[i] += alpha * y[i];
}

// two dots in one pass: partials[0..] = tA.tA, partials[RED_BLOCKS..] = tA.sA
__global__ __launch_bounds__(256) void k_dot2(long n, const double *__restrict__ t, const double *__restrict__ s,
                                              double *__restrict__ partials)
{
    __shared__ double sm[4];
    double a = 0.0, b = 0.0;
    GRID_STRIDE(i, n) { const double ti = t[i]; a += ti * ti; b += ti * s[i]; }
    const double ra = block_sum(a, sm);
    const double rb = block_sum(b, sm);
    if (threadIdx.x == 0) { partials[blockIdx.x] = ra; partials[RED_BLOCKS + blockIdx.x] = rb; }
}

__global__ __launch_bounds__(1024) void k_sum_partials2(int n, const double *__restrict__ partials, double *__restrict__ scal,
                                                        int slot, int nSums, ffm_scal_op t)
{
    __shared__ double sm[16];
    for (int k = 0; k < nSums; k++) {
        double acc = 0.0;
        for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partials[k * RED_BLOCKS + i];
        const double r = block_sum(acc, sm);
        if (threadIdx.x == 0) scal[slot + k] = r;
    }
    if (threadIdx.x == 0) run_scal_op(scal, t);
}

// psi += alpha*yA + omega*zA; rA = sA - omega*tA; partial |rA|
__global__ __launch_bounds__(256) void k_bs_xr(long n, double *__restrict__ psi, double *__restrict__ r,
                                               const double *__restrict__ yA, const double *__restrict__ zA,
                                               const double *__restrict__ sA, const double *__restrict__ tA,
                                               const double *__restrict__ scal, double *__restrict__ partials)
{
    __shared__ double sm[4];
    const double alpha = scal[S_ALPHA], omega = scal[S_OMEGA];
    const bool sing = scal[S_SING] != 0.0;
    double acc = 0.0;
    if (!sing) GRID_STRIDE(i, n) {
        psi[i] += alpha * yA[i] + omega * zA[i];
        const double v = sA[i] - omega * tA[i];
        r[i] = v; acc += fabs(v);
    }
    const double s = block_sum(acc, sm);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// psi = source/diag (diagonalSolver)
__global__ void k_diag_solve(long n, double *__restrict__ psi, const double *__restrict__ b, const double *__restrict__ d)
{ GRID_STRIDE(i, n) psi[i] = b[i] / d[i]; }

__global__ void k_mul(long n, double *__restrict__ w, const double *__restrict__ a, const double *__restrict__ b)
{ GRID_STRIDE(i, n) w[i] = a[i] * b[i]; }

__global__ void k_recip(long n, double *__restrict__ d, const double *__restrict__ s)
{ GRID_STRIDE(i, n) d[i] = 1.0 / s[i]; }

static int partial_sum_to(ffm_ctx *c, int nb, int slot, int nSums = 1, const ffm_scal_op &t = ffm_scal_op())
{
    hipLaunchKernelGGL(k_sum_partials2, dim3(1), dim3(1024), 0, c->stream, nb, c->partials_d, c->scal_d, slot, nSums, t);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

// --------------------------------------------------------- dataflow sweeps ---
// Level-scheduled matrices (unstructured meshes, the coarse levels of a GAMG hierarchy): instead of one launch -- or one device-wide
// barrier -- per dependency level, ONE launch in which every cell waits for the values it needs.
// Workgroups take chunks of 256 cells by an atomic ticket, forward chunks in the level-major cell order, then backward chunks in
// backward-level order: every value a cell waits for belongs to a chunk with a lower ticket, i.e. to a workgroup that is running or
// has finished, so the grid drains whatever the dispatch order or the residency (the scheme of the tiled sweeps, ffm_tile.hip).
// Values are published in sentinel-filled arrays with agent-scope stores and polled with agent-scope loads: the value is its own
// flag.  A lane never blocks in front of its store: the wait is a retry loop with the store inside and a wave-uniform exit (a ballot
// over the lanes not yet done -- with a per-lane exit the compiler may sink the store behind the loop, where a finished lane would
// wait for the lanes that wait for it), so a chain of dependent cells in one wavefront advances one link per trip.  Every wait is bounded and raises the abort word (reported when the solve ends).
// Per-cell arithmetic is that of the serial face loops, term for term in the same order: results are bitwise equal.
// Measured on one MI355X against one launch per dependency level (the form this replaced): a DIC application (two sweeps) in
// level-major numbering 4.30 -> 2.36 ms at 200^3 (598 levels: 2.0 us per level and sweep, the store -> poll round trip between
// workgroups on different XCDs; the poll's s_sleep makes no difference), 1.66 -> 1.05 ms at 100^3; a GAMG V-cycle 29.0 -> 15.5 ms at
// 200^3 and 8.6 -> 5.8 ms at 96^3 (profiles/README.md)
constexpr int FLOW_T = 256;            // measured: 64 is slower at 200^3 (3.6 against 2.36 ms per DIC application), 1024 equal there and slower on the GAMG levels
constexpr unsigned FLOW_SPIN_LIMIT = 1u << 21;
constexpr unsigned long long FLOW_SENT = 0xFFF8C0DEFEEDF10Full;       // a NaN no computation produces
__device__ __forceinline__ bool f_pending(double v) { return (unsigned long long)__double_as_longlong(v) == FLOW_SENT; }
__device__ __forceinline__ void f_st(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double s_ld(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
enum { SM_RD = 0, SM_PRECOND = 1, SM_GS = 2, SM_SYMGS = 3 };
struct FlowArgs {
    LduView v;
    int N, nChunkF, nChunkB, nap;
    const int *order;                       // [N] cells by backward level
    const double *upper, *lower, *diag, *cf, *cb, *r, *bP;
    double *rD, *w, *psi;
    double *mf, *mb, *sv;                   // published values: forward, backward, bSave (sentinel-filled before the launch)
    unsigned int *ticket;                   // [0] ticket counter, [1] abort word
};
__global__ void k_flow_fill(long n, double *a, double *b, double *c, unsigned int *ticket)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) ticket[0] = 0u;
    const double sent = __longlong_as_double((long long)FLOW_SENT);
    GRID_STRIDE(i, n) { if (a) a[i] = sent; if (b) b[i] = sent; if (c) c[i] = sent; }
}
// one trip of a wait: false = keep waiting; raises / follows the abort word
__device__ __forceinline__ bool f_give_up(unsigned &spins, unsigned int *ticket, int nap)
{
    if (nap) __builtin_amdgcn_s_sleep(2);
    if ((++spins & 1023u) == 0u) {
        if (__hip_atomic_load(&ticket[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return true;
        if (spins > FLOW_SPIN_LIMIT) { __hip_atomic_store(&ticket[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return true; }
    }
    return false;
}
template <int MODE, int W>
__global__ __launch_bounds__(FLOW_T) void k_flow_sweep(FlowArgs a)
{
    __shared__ unsigned shTicket;
    if (threadIdx.x == 0) shTicket = atomicAdd(&a.ticket[0], 1u);
    __syncthreads();
    const unsigned tk = shTicket;
    unsigned spins = 0;
    if (tk < (unsigned)a.nChunkF) {
        // ---- forward
        const int c = (int)tk * FLOW_T + threadIdx.x;
        if (c >= a.N) return;
        if (MODE == SM_RD) {
            RowEnt<W> L; load_lower<W>(a.v, c, L);
            double au[W], al[W], rn[W];
#pragma unroll
            for (int s = 0; s < W; s++) { au[s] = a.upper[L.f[s]]; al[s] = a.lower[L.f[s]]; rn[s] = 1.0; }
            const double dg = a.diag[c];
            bool done = false; do { if (!done) {
                bool ready = true;
#pragma unroll
                for (int s = 0; s < W; s++) if (L.on[s]) { rn[s] = s_ld(&a.mf[L.nb[s]]); ready = ready && !f_pending(rn[s]); }
                if (ready) {
                    double d = dg;
#pragma unroll
                    for (int s = 0; s < W; s++) if (L.on[s]) d -= au[s] * al[s] / rn[s];
                    f_st(&a.mf[c], d);
                    a.rD[c] = 1.0 / d;              // k_recip
                    done = true;
                } else done = f_give_up(spins, a.ticket, a.nap);
            } } while (__ballot(!done) != 0ull);
        } else if (MODE == SM_PRECOND) {
            RowEnt<W> L; load_lower<W>(a.v, c, L);
            const double rd = a.rD[c], rc = a.r[c];
            double q[W], wn[W];
#pragma unroll
            for (int s = 0; s < W; s++) { q[s] = a.cf[L.f[s]]; wn[s] = 0.0; }
            bool done = false; do { if (!done) {
                bool ready = true;
#pragma unroll
                for (int s = 0; s < W; s++) if (L.on[s]) { wn[s] = s_ld(&a.mf[L.nb[s]]); ready = ready && !f_pending(wn[s]); }
                if (ready) {
                    double wc = rd * rc;
#pragma unroll
                    for (int s = 0; s < W; s++) if (L.on[s]) wc -= rd * q[s] * wn[s];
                    f_st(&a.mf[c], wc);
                    done = true;
                } else done = f_give_up(spins, a.ticket, a.nap);
            } } while (__ballot(!done) != 0ull);
        } else {
            RowEnt<W> L, U; load_lower<W>(a.v, c, L); load_upper<W>(a.v, c, U);
            double al[W], au[W], pl[W], pu[W];
#pragma unroll
            for (int s = 0; s < W; s++) {
                al[s] = a.lower[L.f[s]]; au[s] = a.upper[U.f[s]];
                pl[s] = 0.0; pu[s] = U.on[s] ? a.psi[U.nb[s]] : 0.0;          // upper neighbours: the values before this sweep
            }
            const double bc = a.bP[c], dg = a.diag[c];
            bool done = false; do { if (!done) {
                bool ready = true;
#pragma unroll
                for (int s = 0; s < W; s++) if (L.on[s]) { pl[s] = s_ld(&a.mf[L.nb[s]]); ready = ready && !f_pending(pl[s]); }
                if (ready) {
                    double val = bc;
#pragma unroll
                    for (int s = 0; s < W; s++) if (L.on[s]) val -= al[s] * pl[s];
                    const double save = val;
#pragma unroll
                    for (int s = 0; s < W; s++) if (U.on[s]) val -= au[s] * pu[s];
                    val /= dg;
                    if (MODE == SM_SYMGS) f_st(&a.sv[c], save); else a.psi[c] = val;
                    f_st(&a.mf[c], val);
                    done = true;
                } else done = f_give_up(spins, a.ticket, a.nap);
            } } while (__ballot(!done) != 0ull);
        }
        return;
    }
    // ---- backward (preconditioner application, symGaussSeidel)
    if (MODE == SM_RD || MODE == SM_GS) return;
    const int p = (int)(tk - (unsigned)a.nChunkF) * FLOW_T + threadIdx.x;
    if (p >= a.N) return;
    const int c = a.order[p];
    if (MODE == SM_PRECOND) {
        RowEnt<W> U; load_upper<W, true>(a.v, c, U);          // block-Jacobi: ghost neighbours are ignored
        const double rd = a.rD[c];
        double q[W], wn[W];
#pragma unroll
        for (int s = 0; s < W; s++) { q[s] = a.cb[U.f[s]]; wn[s] = 0.0; }
        bool done = false; do { if (!done) {
            double wc = s_ld(&a.mf[c]);
            bool ready = !f_pending(wc);
#pragma unroll
            for (int s = 0; s < W; s++) if (U.on[s]) { wn[s] = s_ld(&a.mb[U.nb[s]]); ready = ready && !f_pending(wn[s]); }
            if (ready) {
#pragma unroll
                for (int s = W - 1; s >= 0; s--) if (U.on[s]) wc -= rd * q[s] * wn[s];
                f_st(&a.mb[c], wc);
                a.w[c] = wc;
                done = true;
            } else done = f_give_up(spins, a.ticket, a.nap);
        } } while (__ballot(!done) != 0ull);
    } else {
        RowEnt<W> U; load_upper<W>(a.v, c, U);
        double au[W], pu[W];
        bool own[W];
#pragma unroll
        for (int s = 0; s < W; s++) {
            au[s] = a.upper[U.f[s]]; own[s] = U.on[s] && U.nb[s] < a.N;
            pu[s] = (U.on[s] && !own[s]) ? a.psi[U.nb[s]] : 0.0;              // ghost neighbours: unchanged by the sweep
        }
        const double dg = a.diag[c];
        bool done = false; do { if (!done) {
            double val = s_ld(&a.sv[c]);
            bool ready = !f_pending(val);
#pragma unroll
            for (int s = 0; s < W; s++) if (own[s]) { pu[s] = s_ld(&a.mb[U.nb[s]]); ready = ready && !f_pending(pu[s]); }
            if (ready) {
#pragma unroll
                for (int s = 0; s < W; s++) if (U.on[s]) val -= au[s] * pu[s];
                val /= dg;
                f_st(&a.mb[c], val);
                a.psi[c] = val;
                done = true;
            } else done = f_give_up(spins, a.ticket, a.nap);
        } } while (__ballot(!done) != 0ull);
    }
}

static int flow_args(ffm_ldu *A, int mode, FlowArgs &a)
{
    a = FlowArgs{};
    a.v = ffm_view(A); a.N = A->nOwned; a.nChunkF = (A->nOwned + FLOW_T - 1) / FLOW_T;
    a.nChunkB = (mode == SM_PRECOND || mode == SM_SYMGS) ? a.nChunkF : 0;
    a.nap = 1;
    a.order = A->flowOrder; a.upper = A->upper; a.lower = A->lower; a.diag = A->diag; a.rD = A->rD; a.ticket = A->sweepTicket;
    FFM_TRY(ffm_ldu_work(A, 20, &a.mf));
    if (a.nChunkB) FFM_TRY(ffm_ldu_work(A, 21, &a.mb));
    if (mode == SM_SYMGS) FFM_TRY(ffm_ldu_work(A, 22, &a.sv));
    hipLaunchKernelGGL(k_flow_fill, dim3(sgrid(A->nOwned)), dim3(256), 0, A->ctx->stream, (long)A->nOwned, a.mf, a.mb, a.sv, a.ticket);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}
// (a matrix without owned cells has nothing to sweep: no launch)
#define FLOW_LAUNCH(MODE, a) do { if ((a).nChunkF > 0) FFM_DISPATCH_W(A->maxW, hipLaunchKernelGGL((k_flow_sweep<MODE, W>), dim3((a).nChunkF + (a).nChunkB), dim3(FLOW_T), 0, A->ctx->stream, a)); } while (0)

// the abort word of the tiled and the dataflow sweeps (a bounded wait ran out): reported when a solve ends
int ffm_sweep_check_abort(ffm_ldu *A)
{
    unsigned int h[2] = {0, 0};
    FFM_HIP(hipMemcpyAsync(h, A->sweepTicket, sizeof(h), hipMemcpyDeviceToHost, A->ctx->stream));
    FFM_HIP(hipStreamSynchronize(A->ctx->stream));
    if (h[1]) {
        ffm_set_error(A->sweepMode == 2 ? "tiled sweep timed out waiting for a value of a predecessor group (abort word set)"
                                        : "dataflow sweep timed out waiting for the value of a predecessor cell (abort word set)");
        unsigned int z = 0;
        ffm_h2d(A->ctx, A->sweepTicket + 1, &z, sizeof(z));
        return FFM_ERR_HIP;
    }
    return FFM_OK;
}

// rD = 1/(diag - sum upper*lower/rD[l]) in face order (DIC: lower == upper)
static int calc_rD(ffm_ldu *A)
{
    if (A->sweepMode == 2) {
        const double *dg = A->diag;
        return ffm_tile_calc_rD(A, 1, &dg, &A->rD);          // (stores 1/D)
    }
    FlowArgs a; FFM_TRY(flow_args(A, SM_RD, a));
    FLOW_LAUNCH(SM_RD, a);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

int ffm_precond_setup_i(ffm_ldu *A, int precond)
{
    if (A->rDKind == precond && A->rDEpoch == A->coeffEpoch) return FFM_OK;
    hipStream_t s = A->ctx->stream;
    switch (precond) {
    case FFM_NONE: break;
    case FFM_DIC:
        if (!A->symmetric) { ffm_set_error("DIC needs a symmetric matrix"); return FFM_ERR_UNSUPPORTED; }
        FFM_TRY(calc_rD(A)); break;
    case FFM_DILU: FFM_TRY(calc_rD(A)); break;
    case FFM_DIAGONALP:
        hipLaunchKernelGGL(k_recip, dim3(sgrid(A->nOwned)), dim3(256), 0, s, (long)A->nOwned, A->rD, A->diag);
        FFM_HIP(hipGetLastError());
        break;
    default: ffm_set_error("unknown preconditioner %d", precond); return FFM_ERR_UNSUPPORTED;
    }
    A->rDKind = precond; A->rDEpoch = A->coeffEpoch;
    return FFM_OK;
}

int ffm_precond_apply_i(ffm_ldu *A, int precond, bool transpose, const double *r, double *w)
{
    hipStream_t s = A->ctx->stream;
    const long N = A->nOwned;
    if (precond == FFM_NONE) { hipLaunchKernelGGL(k_copy, dim3(sgrid(N)), dim3(256), 0, s, N, w, r); FFM_HIP(hipGetLastError()); return FFM_OK; }
    if (precond == FFM_DIAGONALP) { hipLaunchKernelGGL(k_mul, dim3(sgrid(N)), dim3(256), 0, s, N, w, A->rD, r); FFM_HIP(hipGetLastError()); return FFM_OK; }
    if (A->sweepMode == 2) { const double *rD = A->rD; return ffm_tile_precond(A, precond, transpose, 1, &rD, &r, &w); }
    // DIC: fwd upper / bwd upper.  DILU: fwd lower / bwd upper.  DILU^T: fwd upper / bwd lower.
    FlowArgs a; FFM_TRY(flow_args(A, SM_PRECOND, a));
    a.cf = (precond == FFM_DIC) ? A->upper : (transpose ? A->upper : A->lower);
    a.cb = (precond == FFM_DIC) ? A->upper : (transpose ? A->lower : A->upper);
    a.r = r; a.w = w;
    FLOW_LAUNCH(SM_PRECOND, a);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

// GaussSeidelSmoother::smooth / symGaussSeidelSmoother::smooth
int ffm_gs_smooth_i(ffm_ldu *A, bool sym, int nSweeps, double *psi, const double *b)
{
    hipStream_t s = A->ctx->stream;
    const long N = A->nOwned;
    double *bP, *bSave;
    FFM_TRY(ffm_ldu_work(A, 10, &bP)); FFM_TRY(ffm_ldu_work(A, 11, &bSave));
    for (int sw = 0; sw < nSweeps; sw++) {
        const double *bUse = b;
        if (!A->ifaces.empty()) {   // bPrime = source + bou*pnf (negated interface coefficients)
            hipLaunchKernelGGL(k_copy, dim3(sgrid(N)), dim3(256), 0, s, N, bP, b);
            FFM_TRY(ffm_halo_update(A, psi, bP, A->ifBou, +1.0));
            bUse = bP;
        }
        // decomposed block: every sweep starts from the neighbour ranks' current values, whatever form the sweep takes (the
        // reference's smoothers update the interfaces before every sweep: GaussSeidelSmoother.C, initMatrixInterfaces /
        // updateMatrixInterfaces inside the sweep loop) -- the dataflow sweeps read psi of the ghost cells
        if (!A->ghNbrRank.empty()) FFM_TRY(ffm_ghost_exchange(A, psi));
        if (A->sweepMode == 2) {
            if (!A->ghNbrRank.empty()) {        // move the ghost cells' terms into bPrime
                if (bUse == b) { hipLaunchKernelGGL(k_copy, dim3(sgrid(N)), dim3(256), 0, s, N, bP, b); bUse = bP; }
                FFM_TRY(ffm_tile_gs_ghost_terms(A, psi, bP));
            }
            if (!A->gsProd) FFM_HIP(hipMalloc((void **)&A->gsProd, sizeof(double) * 3 * (size_t)std::max(A->nCells, 1)));
            FFM_TRY(ffm_tile_gs(A, sym, psi, bUse, bSave, A->gsProd));
            continue;
        }
        FlowArgs a; FFM_TRY(flow_args(A, sym ? SM_SYMGS : SM_GS, a));
        a.bP = bUse; a.psi = psi;
        if (sym) FLOW_LAUNCH(SM_SYMGS, a); else FLOW_LAUNCH(SM_GS, a);
        FFM_HIP(hipGetLastError());
    }
    return FFM_OK;
}

// ------------------------------------------------------------------ solvers ---
struct Controls { double tol, relTol; int minIter, maxIter, nSweeps; };

static inline bool check_convergence(ffm_perf *p, const Controls &k)
{
    p->converged = (p->finalResidual < k.tol || (k.relTol > 1e-20 && p->finalResidual < k.relTol * p->initialResidual)) ? 1 : 0;
    return p->converged;
}

// rA = source - Apsi, normFactor and the initial residual: Apsi = A psi already computed, tmp holds sumA on entry
// (ffm_k_spmv_sumA at the top of every solver).  PBiCGStab (bs) passes its rA0 as rA: the one vector that is rA, rA0 and pA at
// iteration 0, and gets rA0.rA in S_TMP2 as well (k_prologue); tmp may be its pA, which is not written before iteration 1.
// The sums' ranks are added in one all-reduce.
static int norm_and_initial(ffm_ldu *A, const double *psi, const double *source, const double *Apsi, const double *tmp,
                            double *rA, ffm_perf *perf, bool bs = false, bool rowsOnly = false)
{
    ffm_ctx *c = A->ctx; hipStream_t s = c->stream; const long N = A->nOwned;
    if (rowsOnly) {
        FFM_TRY(ffm_k_sum(c, psi, N, S_TMP0));     // the norms of this rank's rows alone (ffm_solve_triangular_rows_d): no sum over ranks
        FFM_TRY(scalar_op(c, OP_XREF, (double)N));
        hipLaunchKernelGGL(k_prologue<false>, dim3(sgrid(N)), dim3(256), 0, s, N, Apsi, source, tmp, c->scal_d, rA, c->partials_d);
        FFM_TRY(partial_sum_to(c, sgrid(N), S_TMP0, 2));
        FFM_TRY(scalar_op(c, OP_NORMF));
        FFM_TRY(scalar_op(c, OP_RES_INIT, 0.0, 0, S_TMP1));
        return FFM_OK;
    }
    const ffm_scal_op xref = tail_op(c, OP_XREF, (double)A->globalCells), normf = tail_op(c, OP_NORMF);
    FFM_TRY(ffm_k_sum(c, psi, N, S_TMP0, xref));
    FFM_TRY(finish_dot(c, xref));
    const int g = sgrid(N), nSums = bs ? 3 : 2;
    if (bs) hipLaunchKernelGGL(k_prologue<true>, dim3(g), dim3(256), 0, s, N, Apsi, source, tmp, c->scal_d, rA, c->partials_d);
    else hipLaunchKernelGGL(k_prologue<false>, dim3(g), dim3(256), 0, s, N, Apsi, source, tmp, c->scal_d, rA, c->partials_d);
    FFM_TRY(partial_sum_to(c, g, S_TMP0, nSums, normf));
    FFM_TRY(finish_dot(c, normf, nSums));
    FFM_TRY(scalar_op(c, OP_RES_INIT, 0.0, 0, S_TMP1));
    FFM_TRY(ffm_read_scalars(c));
    perf->initialResidual = c->scal_h[S_RES0];
    perf->finalResidual = perf->initialResidual;
    perf->nIterations = 0; perf->singular = 0; perf->converged = 0;
    return FFM_OK;
}

// PCG::solve
static int pcg(ffm_ldu *A, int precond, const Controls &k, double *psi, const double *source, ffm_perf *perf)
{
    ffm_ctx *c = A->ctx; hipStream_t s = c->stream; const long N = A->nOwned; const int g = sgrid(N);
    double *pA, *wA, *rA;
    FFM_TRY(ffm_ldu_work(A, 1, &pA)); FFM_TRY(ffm_ldu_work(A, 2, &wA)); FFM_TRY(ffm_ldu_work(A, 3, &rA));
    FFM_TRY(scalar_op(c, OP_RESET));
    FFM_TRY(ffm_k_spmv_sumA(A, psi, wA, pA));
    FFM_TRY(norm_and_initial(A, psi, source, wA, pA, rA, perf));
    if (k.minIter > 0 || !check_convergence(perf, k)) {
        FFM_TRY(ffm_precond_setup_i(A, precond));
        const ffm_scal_op beta = tail_op(c, OP_PCG_BETA), alpha = tail_op(c, OP_PCG_ALPHA), res = tail_op(c, OP_RES);
        if (precond == FFM_DIC && A->sweepMode == 2 && ffm_tile_pcg_fusable(A)) {
            // The same iteration with the vector updates carried by the sweeps (ffm_tile.hip, k_tile<.., FUSE>): the residual
            // update and its norm ride on the forward sweep of the NEXT preconditioner application (which is therefore started
            // before the convergence check: one unused forward sweep per solve), wA.rA on the backward sweep, and psi += alpha pA
            // is deferred into the next search-direction update.  Per-cell arithmetic unchanged.
            // one more fusion where the tiled Amul runs without ghost faces: the direction update and the deferred solution update
            // ride on the Amul (k_tile_amul<true, true>: pNew = wA + beta*pOld, psi += alpha*pOld, qA = A pNew, pNew.qA), with
            // two direction buffers and the Amul result in a vector of its own (elsewhere: separate k_p_psi)
            const bool fuseP = ffm_tile_amul_pcg_usable(A);
            double *pB = nullptr, *qA = wA;
            if (fuseP) { FFM_TRY(ffm_ldu_work(A, 4, &pB)); FFM_TRY(ffm_ldu_work(A, 5, &qA)); }
            do {
                if (perf->nIterations == 0) {
                    FFM_TRY(ffm_precond_apply_i(A, precond, false, rA, wA));
                    FFM_TRY(ffm_k_dot(c, wA, rA, N, S_TMP0, beta));
                } else FFM_TRY(ffm_tile_pcg_bwd(A, rA, wA, S_TMP0, beta));
                FFM_TRY(finish_dot(c, beta));
                if (perf->nIterations == 0) {
                    hipLaunchKernelGGL(k_p_update, dim3(g), dim3(256), 0, s, N, pA, wA, c->scal_d, 1);
                    FFM_TRY(ffm_k_spmv_dot(A, pA, qA, S_TMP0, alpha));
                } else if (fuseP) {
                    FFM_TRY(ffm_tile_amul_pcg(A, wA, pA, pB, psi, qA, S_TMP0, alpha));
                    std::swap(pA, pB);
                } else {
                    hipLaunchKernelGGL(k_p_psi, dim3(g), dim3(256), 0, s, N, psi, pA, wA, c->scal_d);
                    FFM_TRY(ffm_k_spmv_dot(A, pA, qA, S_TMP0, alpha));
                }
                FFM_TRY(finish_dot(c, alpha));
                FFM_TRY(ffm_tile_pcg_fwd(A, rA, wA, S_TMP0, qA == wA ? nullptr : qA, res));
                FFM_TRY(finish_dot(c, res));
                FFM_TRY(ffm_read_scalars(c));
                if (c->scal_h[S_SING] != 0.0) { perf->singular = 1; break; }
                perf->finalResidual = c->scal_h[S_RES];
            } while ((++perf->nIterations < k.maxIter && !check_convergence(perf, k)) || perf->nIterations < k.minIter);
            if (!perf->singular) hipLaunchKernelGGL(k_axpy_alpha, dim3(g), dim3(256), 0, s, N, psi, pA, c->scal_d);
            FFM_HIP(hipGetLastError());
            return FFM_OK;
        }
        do {
            FFM_TRY(ffm_precond_apply_i(A, precond, false, rA, wA));
            FFM_TRY(ffm_k_dot(c, wA, rA, N, S_TMP0, beta));
            FFM_TRY(finish_dot(c, beta));
            hipLaunchKernelGGL(k_p_update, dim3(g), dim3(256), 0, s, N, pA, wA, c->scal_d, perf->nIterations == 0 ? 1 : 0);
            FFM_TRY(ffm_k_spmv_dot(A, pA, wA, S_TMP0, alpha));
            FFM_TRY(finish_dot(c, alpha));
            hipLaunchKernelGGL(k_pcg_xr, dim3(g), dim3(256), 0, s, N, psi, rA, pA, wA, c->scal_d, c->partials_d);
            FFM_TRY(partial_sum_to(c, g, S_TMP0, 1, res));
            FFM_TRY(finish_dot(c, res));
            FFM_TRY(ffm_read_scalars(c));
            if (c->scal_h[S_SING] != 0.0) { perf->singular = 1; break; }
            perf->finalResidual = c->scal_h[S_RES];
        } while ((++perf->nIterations < k.maxIter && !check_convergence(perf, k)) || perf->nIterations < k.minIter);
    }
    return FFM_OK;
}

// PBiCGStab::solve, of one system or of several in lock step.  fvMatrix::solveSegregated of a vector equation and the species loop
// under a multivariateSelection scheme solve systems that differ in the diagonal and the right-hand side only.  Every such system is
// a lane with its own solver state (scalars, work vectors, reciprocal diagonal); each lane goes through the operations of a solve
// of its own in the same order -- its numbers and its iteration count are those of a solve of its own -- but the preconditioner
// sweeps, the Amuls and calcReciprocalD of the lanes still iterating are ONE launch each (ffm_tile.hip: k_tile<.., NF>, ffm_ldu.hip:
// k_rows_m), and the host reads all residuals back with one synchronisation per half iteration.  A lane that is left alone takes
// the one-system calls; a single lane that is the matrix's own state (own_lane) is the plain solve: any matrix, any preconditioner.
namespace {
struct Lane {
    const double *diag, *source; double *psi; ffm_perf *perf;
    double *scal_d, *scal_h;
    int work;                   // its work vectors are ffm_ldu_work(work + 1 .. work + 8)
    double *rD, *pA, *yA, *rA, *AyA, *sA, *zA, *tA, *rA0;
    double *dir, *res;          // the search direction and the residual this iteration reads: pA and rA, at iteration 0 both rA0
    bool active;
};
struct LaneGuard {          // the context's scalar block and the matrix's diagonal / reciprocal diagonal are switched per lane
    ffm_ldu *A; bool several; double *scal_d, *scal_h, *diag, *rD;
    LaneGuard(ffm_ldu *a, bool sev) : A(a), several(sev), scal_d(a->ctx->scal_d), scal_h(a->ctx->scal_h), diag(a->diag), rD(a->rD) {}
    void use(const Lane &l) { A->ctx->scal_d = l.scal_d; A->ctx->scal_h = l.scal_h; A->diag = const_cast<double *>(l.diag); A->rD = l.rD; }
    ~LaneGuard()            // several lanes leave some lane's reciprocal diagonal behind: the matrix's own is stale
    { A->ctx->scal_d = scal_d; A->ctx->scal_h = scal_h; A->diag = diag; A->rD = rD; if (several) { A->rDKind = -1; A->rDEpoch = ~0ul; } }
};
}
// the matrix's own state as a lane: LaneGuard::use changes nothing for it
static Lane own_lane(ffm_ldu *A, double *psi, const double *source, ffm_perf *perf)
{
    Lane l{};
    l.diag = A->diag; l.source = source; l.psi = psi; l.perf = perf; l.scal_d = A->ctx->scal_d; l.scal_h = A->ctx->scal_h; l.work = 0; l.rD = A->rD;
    return l;
}
static int read_lane_scalars(ffm_ctx *c, Lane *L, int n)
{
    bool any = false;
    for (int i = 0; i < n; i++) if (L[i].active) {
        FFM_HIP(hipMemcpyAsync(L[i].scal_h, L[i].scal_d, sizeof(double) * NSCAL, hipMemcpyDeviceToHost, c->stream));
        any = true;
    }
    if (any) FFM_HIP(hipStreamSynchronize(c->stream));
    return FFM_OK;
}
static int precond_lanes(ffm_ldu *A, int precond, Lane *L, int n, double *Lane::*in, double *Lane::*out, LaneGuard &G)
{
    const double *rD[FFM_TILE_MAXSYS], *r[FFM_TILE_MAXSYS]; double *w[FFM_TILE_MAXSYS]; int m = 0, only = -1;
    for (int i = 0; i < n; i++) if (L[i].active) { rD[m] = L[i].rD; r[m] = L[i].*in; w[m] = L[i].*out; m++; only = i; }
    if (m >= 2) return ffm_tile_precond(A, precond, false, m, rD, r, w);
    if (m == 1) { G.use(L[only]); return ffm_precond_apply_i(A, precond, false, L[only].*in, L[only].*out); }
    return FFM_OK;
}
// out = A in for the lanes still iterating: one pass over the coefficients for all of them (ffm_ldu.hip: k_rows_m)
static int amul_lanes(ffm_ldu *A, Lane *L, int n, double *Lane::*in, double *Lane::*out, LaneGuard &G)
{
    const double *dg[FFM_TILE_MAXSYS], *x[FFM_TILE_MAXSYS]; double *y[FFM_TILE_MAXSYS]; int m = 0, only = -1;
    for (int i = 0; i < n; i++) if (L[i].active) { dg[m] = L[i].diag; x[m] = L[i].*in; y[m] = L[i].*out; m++; only = i; }
    if (m >= 2) return ffm_k_spmv_multi(A, m, dg, x, y, nullptr);
    if (m == 1) { G.use(L[only]); return ffm_k_spmv(A, L[only].*in, L[only].*out, false); }
    return FFM_OK;
}
static int pbicgstab_lanes(ffm_ldu *A, int precond, const Controls &k, int n, Lane *L)
{
    ffm_ctx *c = A->ctx; hipStream_t s = c->stream; const long N = A->nOwned; const int g = sgrid(N);
    LaneGuard G(A, n > 1);
    for (int i = 0; i < n; i++) {
        Lane &l = L[i]; G.use(l);
        FFM_TRY(ffm_ldu_work(A, l.work + 1, &l.pA)); FFM_TRY(ffm_ldu_work(A, l.work + 2, &l.yA)); FFM_TRY(ffm_ldu_work(A, l.work + 3, &l.rA));
        FFM_TRY(ffm_ldu_work(A, l.work + 8, &l.rA0));
        FFM_TRY(scalar_op(c, OP_RESET));
    }
    if (n == 1) FFM_TRY(ffm_k_spmv_sumA(A, L[0].psi, L[0].yA, L[0].pA));
    else {      // yA = A psi and sumA of every system in one pass
        const double *dg[FFM_TILE_MAXSYS], *x[FFM_TILE_MAXSYS]; double *y[FFM_TILE_MAXSYS], *sm[FFM_TILE_MAXSYS];
        for (int i = 0; i < n; i++) { dg[i] = L[i].diag; x[i] = L[i].psi; y[i] = L[i].yA; sm[i] = L[i].pA; }
        FFM_TRY(ffm_k_spmv_multi(A, n, dg, x, y, sm));
    }
    for (int i = 0; i < n; i++) {
        Lane &l = L[i]; G.use(l);
        FFM_TRY(norm_and_initial(A, l.psi, l.source, l.yA, l.pA, l.rA0, l.perf, true));          // (sumA in pA; reads this lane's scalars back)
        l.active = k.minIter > 0 || !check_convergence(l.perf, k);
        if (!l.active) continue;
        FFM_TRY(ffm_ldu_work(A, l.work + 4, &l.AyA)); FFM_TRY(ffm_ldu_work(A, l.work + 5, &l.sA)); FFM_TRY(ffm_ldu_work(A, l.work + 6, &l.zA));
        FFM_TRY(ffm_ldu_work(A, l.work + 7, &l.tA));
    }
    {   // calcReciprocalD of the systems that iterate.  Several lanes: every lane's rD is then current and the single-lane calls below
        // must not redo it, whatever the matrix's cache says of its own; the one lane of the matrix's own state keeps the cache check
        const double *dg[FFM_TILE_MAXSYS]; double *D[FFM_TILE_MAXSYS]; int m = 0, only = -1;
        for (int i = 0; i < n; i++) if (L[i].active) { dg[m] = L[i].diag; D[m] = L[i].rD; m++; only = i; }
        if (m >= 2) FFM_TRY(ffm_tile_calc_rD(A, m, dg, D));          // (stores 1/D)
        else if (m == 1) { G.use(L[only]); if (n > 1) A->rDKind = -1; FFM_TRY(ffm_precond_setup_i(A, precond)); }
        if (n > 1) { A->rDKind = precond; A->rDEpoch = A->coeffEpoch; }
    }
    // Iteration 0: rA, rA0 and pA are one vector, the rA0 that the prologue wrote, read wherever the iteration reads rA or pA.  It
    // ends with k_bs_xr writing rA; iteration 1 forms pA, with rA0 as the direction before it.
    const ffm_scal_op alpha = tail_op(c, OP_BS_ALPHA), res = tail_op(c, OP_RES), omega = tail_op(c, OP_BS_OMEGA);
    for (;;) {
        bool any = false;
        for (int i = 0; i < n; i++) if (L[i].active) {
            Lane &l = L[i]; G.use(l); any = true;
            const int it = l.perf->nIterations;
            if (it == 0) { l.dir = l.res = l.rA0; FFM_TRY(scalar_op(c, OP_BS_RHO, 0.0, 0, S_TMP2)); continue; }       // rA0.rA came with the prologue
            const ffm_scal_op rho = tail_op(c, OP_BS_RHO, 0.0, it);
            FFM_TRY(ffm_k_dot(c, l.rA0, l.rA, N, S_TMP0, rho));
            FFM_TRY(finish_dot(c, rho));
            hipLaunchKernelGGL(k_bs_p, dim3(g), dim3(256), 0, s, N, l.pA, (const double *)l.dir, l.rA, l.AyA, c->scal_d);
            l.dir = l.pA; l.res = l.rA;
        }
        if (!any) break;
        FFM_TRY(precond_lanes(A, precond, L, n, &Lane::dir, &Lane::yA, G));
        FFM_TRY(amul_lanes(A, L, n, &Lane::yA, &Lane::AyA, G));
        for (int i = 0; i < n; i++) if (L[i].active) {
            Lane &l = L[i]; G.use(l);
            FFM_TRY(ffm_k_dot(c, l.rA0, l.AyA, N, S_TMP0, alpha));
            FFM_TRY(finish_dot(c, alpha));
            hipLaunchKernelGGL(k_bs_s, dim3(g), dim3(256), 0, s, N, l.sA, (const double *)l.res, l.AyA, c->scal_d, c->partials_d);
            FFM_TRY(partial_sum_to(c, g, S_TMP0, 1, res));
            FFM_TRY(finish_dot(c, res));
        }
        FFM_TRY(read_lane_scalars(c, L, n));
        for (int i = 0; i < n; i++) if (L[i].active) {
            Lane &l = L[i]; G.use(l);
            if (l.scal_h[S_SING] != 0.0) { l.perf->singular = 1; l.active = false; continue; }
            l.perf->finalResidual = l.scal_h[S_RES];
            if (check_convergence(l.perf, k)) {
                hipLaunchKernelGGL(k_axpy_alpha, dim3(g), dim3(256), 0, s, N, l.psi, l.yA, c->scal_d);
                l.perf->nIterations++;
                l.active = false;
            }
        }
        FFM_TRY(precond_lanes(A, precond, L, n, &Lane::sA, &Lane::zA, G));
        FFM_TRY(amul_lanes(A, L, n, &Lane::zA, &Lane::tA, G));
        for (int i = 0; i < n; i++) if (L[i].active) {
            Lane &l = L[i]; G.use(l);
            hipLaunchKernelGGL(k_dot2, dim3(g), dim3(256), 0, s, N, l.tA, l.sA, c->partials_d);
            FFM_TRY(partial_sum_to(c, g, S_TMP0, 2, omega));
            FFM_TRY(finish_dot(c, omega, 2));
            hipLaunchKernelGGL(k_bs_xr, dim3(g), dim3(256), 0, s, N, l.psi, l.rA, l.yA, l.zA, l.sA, l.tA, c->scal_d, c->partials_d);
            FFM_TRY(partial_sum_to(c, g, S_TMP0, 1, res));
            FFM_TRY(finish_dot(c, res));
        }
        FFM_TRY(read_lane_scalars(c, L, n));
        for (int i = 0; i < n; i++) if (L[i].active) {
            Lane &l = L[i];
            l.perf->finalResidual = l.scal_h[S_RES];
            l.active = (++l.perf->nIterations < k.maxIter && !check_convergence(l.perf, k)) || l.perf->nIterations < k.minIter;
        }
    }
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}
static int pbicgstab(ffm_ldu *A, int precond, const Controls &k, double *psi, const double *source, ffm_perf *perf)
{
    Lane l = own_lane(A, psi, source, perf);
    return pbicgstab_lanes(A, precond, k, 1, &l);
}

// PBiCG::solve
static int pbicg(ffm_ldu *A, int precond, const Controls &k, double *psi, const double *source, ffm_perf *perf)
{
    ffm_ctx *c = A->ctx; hipStream_t s = c->stream; const long N = A->nOwned; const int g = sgrid(N);
    double *pA, *pT, *wA, *wT, *rA, *rT;
    FFM_TRY(ffm_ldu_work(A, 1, &pA)); FFM_TRY(ffm_ldu_work(A, 2, &wA)); FFM_TRY(ffm_ldu_work(A, 3, &rA));
    FFM_TRY(ffm_ldu_work(A, 4, &pT)); FFM_TRY(ffm_ldu_work(A, 5, &wT)); FFM_TRY(ffm_ldu_work(A, 6, &rT));
    FFM_TRY(scalar_op(c, OP_RESET));
    FFM_TRY(ffm_k_spmv_sumA(A, psi, wA, pA));
    FFM_TRY(ffm_k_spmv(A, psi, wT, true));
    hipLaunchKernelGGL(k_sub, dim3(g), dim3(256), 0, s, N, rT, source, wT);
    FFM_TRY(norm_and_initial(A, psi, source, wA, pA, rA, perf));
    if (k.minIter > 0 || !check_convergence(perf, k)) {
        FFM_TRY(ffm_precond_setup_i(A, precond));
        const ffm_scal_op beta = tail_op(c, OP_BICG_BETA), alpha = tail_op(c, OP_BICG_ALPHA), res = tail_op(c, OP_RES);
        do {
            FFM_TRY(ffm_precond_apply_i(A, precond, false, rA, wA));
            FFM_TRY(ffm_precond_apply_i(A, precond, true, rT, wT));
            FFM_TRY(ffm_k_dot(c, wA, rT, N, S_TMP0, beta));
            FFM_TRY(finish_dot(c, beta));
            const int first = perf->nIterations == 0 ? 1 : 0;
            hipLaunchKernelGGL(k_p_update, dim3(g), dim3(256), 0, s, N, pA, wA, c->scal_d, first);
            hipLaunchKernelGGL(k_p_update, dim3(g), dim3(256), 0, s, N, pT, wT, c->scal_d, first);
            FFM_TRY(ffm_k_spmv(A, pA, wA, false));
            FFM_TRY(ffm_k_spmv(A, pT, wT, true));
            FFM_TRY(ffm_k_dot(c, wA, pT, N, S_TMP0, alpha));
            FFM_TRY(finish_dot(c, alpha));
            hipLaunchKernelGGL(k_axmy_alpha, dim3(g), dim3(256), 0, s, N, rT, wT, c->scal_d);
            hipLaunchKernelGGL(k_pcg_xr, dim3(g), dim3(256), 0, s, N, psi, rA, pA, wA, c->scal_d, c->partials_d);
            FFM_TRY(partial_sum_to(c, g, S_TMP0, 1, res));
            FFM_TRY(finish_dot(c, res));
            FFM_TRY(ffm_read_scalars(c));
            if (c->scal_h[S_SING] != 0.0) { perf->singular = 1; break; }
            perf->finalResidual = c->scal_h[S_RES];
        } while ((++perf->nIterations < k.maxIter && !check_convergence(perf, k)) || perf->nIterations < k.minIter);
    }
    return FFM_OK;
}

// smoothSolver::solve
static int smooth(ffm_ldu *A, int smoother, const Controls &k, double *psi, const double *source, ffm_perf *perf)
{
    if (smoother != FFM_GS && smoother != FFM_SYMGS) { ffm_set_error("smoothSolver: smoother must be GaussSeidel or symGaussSeidel"); return FFM_ERR_UNSUPPORTED; }
    ffm_ctx *c = A->ctx; const long N = A->nOwned;
    const int nSweeps = k.nSweeps > 0 ? k.nSweeps : 1;
    double *Apsi, *tmp, *res;
    FFM_TRY(ffm_ldu_work(A, 1, &Apsi)); FFM_TRY(ffm_ldu_work(A, 2, &tmp)); FFM_TRY(ffm_ldu_work(A, 3, &res));
    FFM_TRY(scalar_op(c, OP_RESET));
    FFM_TRY(ffm_k_spmv_sumA(A, psi, Apsi, tmp));
    FFM_TRY(norm_and_initial(A, psi, source, Apsi, tmp, res, perf));
    if (k.minIter > 0 || !check_convergence(perf, k)) {
        const ffm_scal_op resOp = tail_op(c, OP_RES);
        do {
            FFM_TRY(ffm_gs_smooth_i(A, smoother == FFM_SYMGS, nSweeps, psi, source));
            FFM_TRY(ffm_k_residual(A, psi, source, res));
            FFM_TRY(ffm_k_summag(c, res, N, S_TMP0, resOp));
            FFM_TRY(finish_dot(c, resOp));
            FFM_TRY(ffm_read_scalars(c));
            perf->finalResidual = c->scal_h[S_RES];
        } while (((perf->nIterations += nSweeps) < k.maxIter && !check_convergence(perf, k)) || perf->nIterations < k.minIter);
    }
    return FFM_OK;
}

static int diagonal(ffm_ldu *A, double *psi, const double *source, ffm_perf *perf)
{
    hipLaunchKernelGGL(k_diag_solve, dim3(sgrid(A->nOwned)), dim3(256), 0, A->ctx->stream, (long)A->nOwned, psi, source, A->diag);
    FFM_HIP(hipGetLastError());
    perf->initialResidual = perf->finalResidual = 0.0; perf->nIterations = 0; perf->converged = 1; perf->singular = 0;
    return FFM_OK;
}

static int solve_internal(ffm_ldu *A, int solver, int precond, const Controls &k, double *psi, const double *source, ffm_perf *perf)
{
    switch (solver) {
    case FFM_PCG:
        if (!A->symmetric) { ffm_set_error("PCG needs a symmetric matrix"); return FFM_ERR_UNSUPPORTED; }
        return pcg(A, precond, k, psi, source, perf);
    case FFM_PBICGSTAB: return pbicgstab(A, precond, k, psi, source, perf);
    case FFM_PBICG: return pbicg(A, precond, k, psi, source, perf);
    case FFM_DIAGONAL: return diagonal(A, psi, source, perf);
    case FFM_SMOOTH: return smooth(A, precond, k, psi, source, perf);
    }
    ffm_set_error("unknown solver %d", solver);
    return FFM_ERR_UNSUPPORTED;
}

// library-internal: vectors in the matrix's internal cell order, no final synchronisation (ffm_gamg.hip: coarsest level)
extern "C" int ffm_solve_internal_i(ffm_ldu *A, int solver, int precond, double tol, double relTol, int minIter, int maxIter, int nSweeps,
                                    double *psi, const double *source, ffm_perf *perf)
{
    memset(perf, 0, sizeof(*perf));
    Controls k{tol, relTol, minIter, maxIter, nSweeps};
    return solve_internal(A, solver, precond, k, psi, source, perf);
}

extern "C" int ffm_solve_d(ffm_ldu *A, int solver, int precond, double tol, double relTol, int minIter, int maxIter,
                           int nSweeps, double *psi_d, const double *source_d, ffm_perf *out)
{
    if (!A || !psi_d || !source_d || !out) { ffm_set_error("ffm_solve_d: null argument"); return FFM_ERR_ARG; }
    if ((solver == FFM_PCG || solver == FFM_PBICGSTAB || solver == FFM_PBICG) &&
        !(precond == FFM_NONE || precond == FFM_DIC || precond == FFM_DILU || precond == FFM_DIAGONALP)) {
        ffm_set_error("solver %d: preconditioner %d not offered", solver, precond); return FFM_ERR_UNSUPPORTED;
    }
    memset(out, 0, sizeof(*out));
    Controls k{tol, relTol, minIter, maxIter, nSweeps};
    FFM_HIP(hipSetDevice(A->ctx->device));
    if (A->identity) {
        FFM_TRY(solve_internal(A, solver, precond, k, psi_d, source_d, out));
    } else {
        const double *si; double *pi;
        FFM_TRY(ffm_to_internal(A, source_d, 1, &si));
        const double *pin; FFM_TRY(ffm_to_internal(A, psi_d, 2, &pin)); pi = A->permIn[2];
        FFM_TRY(solve_internal(A, solver, precond, k, pi, si, out));
        FFM_TRY(ffm_from_internal(A, pi, psi_d));
    }
    FFM_HIP(hipStreamSynchronize(A->ctx->stream));
    FFM_TRY(ffm_sweep_check_abort(A));
    return FFM_OK;
}

// ------------------------------------------------------------------ exact one-sweep solves: what they share ---
// A solve that is one substitution sweep (ffm_solve_triangular_rows_d, the flow-ordered solves) still reports OpenFOAM's
// normalised residuals of the start value and of the result.  ranks: the sums are taken over all ranks (the Amul refreshes psi's
// ghost entries), else over this rank's rows as they stand -- nothing then reaches another rank: no ghost refresh, no all-reduce,
// and one host synchronisation fewer.  The single-rank path keeps the row kernel for the Amul with sumA (ffm_k_spmv_sumA may take
// the tiled kernel, another summation order).  Vectors in the internal numbering.
static int exact_solve_begin(ffm_ldu *A, bool ranks, const double *psi, const double *source, double **rA, ffm_perf *out)
{
    double *sumA, *Apsi;
    FFM_TRY(ffm_ldu_work(A, 1, &sumA)); FFM_TRY(ffm_ldu_work(A, 2, &Apsi)); FFM_TRY(ffm_ldu_work(A, 3, rA));
    FFM_TRY(scalar_op(A->ctx, OP_RESET));
    FFM_TRY(ranks ? ffm_k_spmv_sumA(A, psi, Apsi, sumA) : ffm_k_spmv_sumA_rows(A, psi, Apsi, sumA));
    return norm_and_initial(A, psi, source, Apsi, sumA, *rA, out, false, !ranks);
}
// v[0 .. n) -> their sum (isMax 0) or maximum (1) over the ranks; n <= 4
static int allreduce_host_values(ffm_ctx *c, double *v, int n, int isMax)
{
    if (c->nRanks <= 1 && !c->comm) return FFM_OK;
    FFM_TRY(ffm_h2d(c, c->scal_d + S_TMP0, v, sizeof(double) * n));
    FFM_TRY(isMax ? ffm_allreduce_minmax(c, S_TMP0, 1, n) : ffm_allreduce_slots(c, S_TMP0, n));
    return ffm_d2h(c, v, c->scal_d + S_TMP0, sizeof(double) * n);
}
// What the sweep left.  nIterations 1; converged says whether the substitution WAS the solve: sum |source - A psi| <= 1e-10
// sum |source| (an exact substitution leaves rounding, ~1e-15; a matrix that is not triangular in the order of the sweep leaves
// O(1)).  The test is on the unnormalised sums because OpenFOAM's normFactor is round-off wherever the solution is uniform over
// the rows.  psiCaller: where psi goes back to in the caller's numbering, or null.  The abort word of the dataflow sweeps is
// reported last, with ranks on every rank.
static int exact_solve_record(ffm_ldu *A, bool ranks, const char *who, double *psi, const double *source, double *rA, double *psiCaller, ffm_perf *out)
{
    ffm_ctx *c = A->ctx; const long N = A->nOwned;
    // ranks: the residual's Amul refreshes psi's ghost entries, which hold the neighbours' results on return.  (A matrix without a
    // ghost exchange and interfaces -- the single-rank ordered solve -- gets the same launch from either routine.)
    FFM_TRY(ranks ? ffm_k_residual(A, psi, source, rA) : ffm_k_residual_rows(A, psi, source, rA));
    FFM_TRY(ffm_k_summag(c, rA, N, S_TMP0));
    FFM_TRY(ffm_k_summag(c, source, N, S_TMP1));
    if (ranks) FFM_TRY(ffm_allreduce_slots(c, S_TMP0, 2));
    FFM_TRY(scalar_op(c, OP_RES));                                                  // (reads S_TMP0 only)
    if (psiCaller) FFM_TRY(ffm_from_internal(A, psi, psiCaller));
    FFM_TRY(ffm_read_scalars(c));
    out->initialResidual = c->scal_h[S_RES0]; out->finalResidual = c->scal_h[S_RES];
    out->nIterations = 1; out->singular = 0;
    out->converged = (c->scal_h[S_TMP0] <= 1e-10 * c->scal_h[S_TMP1]) ? 1 : 0;      // (false for NaN too)
    const int rcAbort = ffm_sweep_check_abort(A);
    if (!ranks) return rcAbort;
    double ab = rcAbort != FFM_OK ? 1.0 : 0.0;
    FFM_TRY(allreduce_host_values(c, &ab, 1, 1));
    if (rcAbort != FFM_OK) return rcAbort;
    if (ab != 0.0) { ffm_set_error("%s: a dataflow sweep timed out on another rank", who); return FFM_ERR_HIP; }
    return FFM_OK;
}

// The exact solve of a matrix that is triangular in the matrix's cell order, on this rank's rows alone: calcReciprocalD of a
// triangular matrix is 1/diag, and one DILU application is then the forward (lower-triangular) or the backward (upper-triangular)
// substitution in face order -- psi = A^-1 source, one sweep pair, no Krylov iteration.  Nothing here reaches another rank (no
// ghost refresh, no sum over ranks): faces towards ghost cells must carry zero coefficients, their terms belong in `source`.
// out: as exact_solve_record leaves it, the sums taken over this rank's rows (converged 0: a wrong renaming, a ghost face left
// in).  The matrix is the bound one (ffm_ldu_bind_coeffs_native_d), vectors in the library's cell order.
extern "C" int ffm_solve_triangular_rows_d(ffm_ldu *A, double *psi_d, const double *source_d, ffm_perf *out)
{
    if (!A || !psi_d || !source_d || !out) { ffm_set_error("ffm_solve_triangular_rows_d: null argument"); return FFM_ERR_ARG; }
    if (!A->identity || !A->ifaces.empty()) { ffm_set_error("ffm_solve_triangular_rows_d: needs the library's cell order and no coupled patches"); return FFM_ERR_UNSUPPORTED; }
    memset(out, 0, sizeof(*out));
    FFM_HIP(hipSetDevice(A->ctx->device));
    double *rA;
    FFM_TRY(exact_solve_begin(A, false, psi_d, source_d, &rA, out));
    FFM_TRY(ffm_precond_setup_i(A, FFM_DILU));
    FFM_TRY(ffm_precond_apply_i(A, FFM_DILU, false, source_d, psi_d));
    return exact_solve_record(A, false, "ffm_solve_triangular_rows_d", psi_d, source_d, rA, nullptr, out);
}

// ------------------------------------------------------------------ flow-ordered exact solve ---
// A matrix with at most one non-zero off-diagonal coefficient per face and no cycle among them (an upwind ray equation,
// fvm::div(Ji, Ii) + fvm::Sp(k omega, Ii), on any mesh with planar faces) is triangular under the level-major order of its own
// dependency graph (ffm_flow_levels, ffm_rays.cpp).  On a decomposed mesh the cells' graph is still acyclic, the ranks' is not
// (rank A feeds B across one cut face, B feeds A across another), so the order is staged by cells: stage = the largest number of
// rank crossings on any upstream path (ffm_flow_stages), and the order is stage-major.  The rows of stage s need owned cells of
// stage <= s and ghost cells of stage < s.  ffm_flow_order keeps the order on the device, int[N] in the matrix's internal cell
// numbering, and the stages' position ranges on the host; a single-rank order is the case of no ghost cells and one stage [0, N):
// it holds no stage arrays (4 N bytes of device memory), and neither making nor using it communicates.
// The solve, per stage: one dataflow sweep over the positions of the stage -- the machinery of k_flow_sweep: chunks of 256
// positions by ticket, published values, bounded waits -- in which a row waits for the owned cells of its non-zero entries only,
// lower faces then upper faces in face order, one division: bitwise the serial forward substitution.  A ghost column is read from
// psi's ghost entry, which the exchange behind the stage before filled; then all ranks refresh psi's ghost entries once and the
// next stage follows: nStages - 1 exchanges per solve, none on a single rank.
// The order is never trusted: a pass over the rows first checks, against the coefficients the matrix holds now, that the owned
// column of every non-zero entry stands earlier in the order than its row, in no later stage, and that a ghost column's stage is
// below the row's; the sweeps are launched only where no row fails on any rank -- a row then waits only for positions of its own
// or an earlier chunk, whose workgroups are running or done.  With ranks, every decision a rank takes on what it alone sees (a
// local cycle, a row the order does not fit, the abort word) is all-reduced first, so all ranks leave a call the same way.
struct ffm_flow_order {
    ffm_ctx *ctx = nullptr;
    bool staged = false;           // made by ffm_flow_order_create_staged: the entry point decides, not the matrix
    int N = 0, nGhost = 0, nLevels = 0;
    int nStages = 1;               // over all ranks, the same on every rank
    int *order = nullptr;          // [N] device: position -> internal cell
    std::vector<int> stageStart;   // [nStages + 1] host: stage s = the positions [stageStart[s], stageStart[s + 1]) of order
    // null in a single-rank order: every cell in stage 0, no ghost cells
    int *stage = nullptr;          // [N] device: stage of every owned cell (internal numbering)
    int *ghostStage = nullptr;     // [nGhost] device: stage of every ghost cell on the rank that owns it
};

struct OrderedArgs {
    LduView v;
    int N, nap;
    const int *order;
    const double *upper, *lower, *diag, *source;
    double *psi, *mf;
    unsigned int *ticket;
};

__global__ void k_order_pos(long n, const int *__restrict__ order, int *__restrict__ pos)
{ GRID_STRIDE(p, n) pos[order[p]] = (int)p; }

// non-zero entries whose owned column does not stand earlier in the order than the row or has a later stage, or whose ghost
// column's stage is not below the row's: block partial counts.  stage == null (a branch the whole grid takes alike): every cell in
// stage 0, and a ghost column fails
template <int W>
__global__ __launch_bounds__(256) void k_order_check(LduView v, const double *__restrict__ upper, const double *__restrict__ lower,
                                                     const int *__restrict__ pos, const int *__restrict__ stage,
                                                     const int *__restrict__ ghostStage, double *__restrict__ partials)
{
    __shared__ double sm[4];
    double bad = 0.0;
    GRID_STRIDE(i, (long)v.N) {
        const int c = (int)i;
        RowEnt<W> L, U; load_lower<W>(v, c, L); load_upper<W>(v, c, U);
        const int pc = pos[c], sc = stage ? stage[c] : 0;
#pragma unroll
        for (int s = 0; s < W; s++) {
            if (L.on[s] && lower[L.f[s]] != 0.0 && !(pos[L.nb[s]] < pc && (!stage || stage[L.nb[s]] <= sc))) bad += 1.0;
            if (U.on[s] && upper[U.f[s]] != 0.0) {
                const int n = U.nb[s];
                if (n < v.N ? !(pos[n] < pc && (!stage || stage[n] <= sc)) : !(stage && ghostStage[n - v.N] < sc)) bad += 1.0;
            }
        }
    }
    const double r = block_sum(bad, sm);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// the sweep over the positions [p0, p1) of one stage: a row waits on the published array for its owned columns only (cells of this
// launch's earlier positions, or of an earlier launch: published then); a ghost column is psi's ghost entry as the exchange behind
// an earlier stage left it, a plain load -- a kernel boundary lies in between.  GHOSTS false, a matrix without ghost cells: every
// column is owned, `own` folds into U.on
template <int W, bool GHOSTS>
__global__ __launch_bounds__(FLOW_T) void k_flow_ordered(OrderedArgs a, int p0, int p1)
{
    __shared__ unsigned shTicket;
    if (threadIdx.x == 0) shTicket = atomicAdd(&a.ticket[0], 1u);
    __syncthreads();
    const int p = p0 + (int)shTicket * FLOW_T + threadIdx.x;
    if (p >= p1) return;
    const int c = a.order[p];
    unsigned spins = 0;
    RowEnt<W> L, U; load_lower<W>(a.v, c, L); load_upper<W>(a.v, c, U);
    double al[W], au[W], pl[W], pu[W];
    bool own[W];
#pragma unroll
    for (int s = 0; s < W; s++) {
        al[s] = a.lower[L.f[s]]; au[s] = a.upper[U.f[s]];
        L.on[s] = L.on[s] && al[s] != 0.0; U.on[s] = U.on[s] && au[s] != 0.0;      // a zero entry is no dependency: not waited for
        own[s] = U.on[s] && (!GHOSTS || U.nb[s] < a.N);
        pl[s] = 0.0; pu[s] = (U.on[s] && !own[s]) ? a.psi[U.nb[s]] : 0.0;
    }
    const double bc = a.source[c], dg = a.diag[c];
    bool done = false; do { if (!done) {
        bool ready = true;
#pragma unroll
        for (int s = 0; s < W; s++) {
            if (L.on[s]) { pl[s] = s_ld(&a.mf[L.nb[s]]); ready = ready && !f_pending(pl[s]); }
            if (own[s]) { pu[s] = s_ld(&a.mf[U.nb[s]]); ready = ready && !f_pending(pu[s]); }
        }
        if (ready) {
            double val = bc;
#pragma unroll
            for (int s = 0; s < W; s++) if (L.on[s]) val -= al[s] * pl[s];
#pragma unroll
            for (int s = 0; s < W; s++) if (U.on[s]) val -= au[s] * pu[s];
            val /= dg;
            a.psi[c] = val;
            f_st(&a.mf[c], val);
            done = true;
        } else done = f_give_up(spins, a.ticket, a.nap);
    } } while (__ballot(!done) != 0ull);
}

static bool ordered_single_rank(const ffm_ldu *A)
{ return A->nOwned == A->nCells && A->ifaces.empty() && A->ghNbrRank.empty(); }
static bool ordered_decomposed(const ffm_ldu *A)
{
    // a ghost exchange, or a rank of several that has no neighbour (and then no ghost cell)
    return A->ifaces.empty() && (!A->ghNbrRank.empty() || (A->ctx->nRanks > 1 && A->nCells == A->nOwned));
}
// the refusal of a matrix that is not the entry point's kind (a matrix without ghost cells on a context of several ranks is both)
static int ordered_refuse(const ffm_ldu *A, bool ranks, const char *who)
{
    if (ranks ? ordered_decomposed(A) : ordered_single_rank(A)) return FFM_OK;
    if (ranks) ffm_set_error("%s: needs a matrix with a ghost exchange (ffm_ldu_set_ghost_exchange) and no processor interfaces; "
                             "ffm_flow_order_create and ffm_solve_ordered_d are the single-rank form", who);
    else ffm_set_error("%s: single rank only (the matrix has ghost cells, processor interfaces or a ghost exchange)", who);
    return FFM_ERR_UNSUPPORTED;
}

// the off-diagonals the matrix holds, once, as the faces of the internal numbering in the caller's face order of every row
// (columns >= nOwned: ghost cells)
static int download_faces(ffm_ldu *A, std::vector<int> &l, std::vector<int> &u, std::vector<double> &cu, std::vector<double> &cl)
{
    const int nS = A->nSlices, T = A->upTotal;
    std::vector<int> upOff((size_t)nS + 1, 0), upNbr((size_t)T);
    std::vector<double> up((size_t)T), lo((size_t)T);
    FFM_TRY(ffm_d2h(A->ctx, upOff.data(), A->upOff, sizeof(int) * ((size_t)nS + 1)));
    FFM_TRY(ffm_d2h(A->ctx, upNbr.data(), A->upNbr, sizeof(int) * (size_t)T));
    FFM_TRY(ffm_d2h(A->ctx, up.data(), A->upper, sizeof(double) * (size_t)T));
    if (A->lower != A->upper) FFM_TRY(ffm_d2h(A->ctx, lo.data(), A->lower, sizeof(double) * (size_t)T)); else lo = up;
    l.reserve(A->nFaces); u.reserve(A->nFaces); cu.reserve(A->nFaces); cl.reserve(A->nFaces);
    for (int sl = 0; sl < nS; sl++) {
        const int base = upOff[sl], w = (upOff[sl + 1] - base) >> 6;
        for (int lane = 0; lane < 64; lane++) for (int s = 0; s < w; s++) {
            const int e = base + s * 64 + lane, n = upNbr[e];
            if (n < 0) continue;
            l.push_back(sl * 64 + lane); u.push_back(n); cu.push_back(up[e]); cl.push_back(lo[e]);
        }
    }
    return FFM_OK;
}

__global__ void k_int_to_double(long n, const int *__restrict__ a, double *__restrict__ x)
{ GRID_STRIDE(i, n) x[i] = (double)a[i]; }
__global__ void k_double_to_int(long n, const double *__restrict__ x, int *__restrict__ a)
{ GRID_STRIDE(i, n) a[i] = (int)x[i]; }

static int flow_order_create(ffm_ldu *A, bool ranks, ffm_flow_order **out)
{
    const char *who = ranks ? "ffm_flow_order_create_staged" : "ffm_flow_order_create";
    if (!A || !out) { ffm_set_error("%s: null argument", who); return FFM_ERR_ARG; }
    *out = nullptr;
    FFM_TRY(ordered_refuse(A, ranks, who));
    FFM_HIP(hipSetDevice(A->ctx->device));
    ffm_ctx *c = A->ctx; hipStream_t s = c->stream;
    const int N = A->nOwned, nG = A->nCells - A->nOwned;
    std::vector<int> l, u; std::vector<double> cu, cl;
    FFM_TRY(download_faces(A, l, u, cu, cl));
    double *x = nullptr;                                   // the stages as a cell field: what the ghost exchange moves
    if (ranks) FFM_TRY(ffm_ldu_work(A, 23, &x));
    ffm_flow_order *o = new ffm_flow_order;
    o->ctx = c; o->staged = ranks; o->N = N; o->nGhost = nG;
    // from here on every rank takes every step: what fails locally is carried in `fail` to the all-reduce of the round
    int fail = FFM_OK, rc = FFM_OK;
    if (hipMalloc((void **)&o->order, sizeof(int) * (size_t)std::max(N, 1)) != hipSuccess ||
        (ranks && (hipMalloc((void **)&o->stage, sizeof(int) * (size_t)std::max(N, 1)) != hipSuccess ||
                   hipMalloc((void **)&o->ghostStage, sizeof(int) * (size_t)std::max(nG, 1)) != hipSuccess))) {
        ffm_set_error("%s: out of device memory", who); fail = FFM_ERR_HIP;
    }
    std::vector<int> order((size_t)std::max(N, 1)), stage((size_t)std::max(N, 1), 0);      // (a single rank: every stage 0)
    bool anyFail = false, cycle = false;
    double total = (double)nG;                             // a path with more rank crossings than there are ghost cells revisits one
    if (!ranks) {
        if (fail == FFM_OK) fail = ffm_flow_levels(N, (int)l.size(), l.data(), u.data(), cu.data(), cl.data(), order.data(), &o->nLevels);
    } else {
        // the fixpoint over the ranks: all ghost stages 0, then rounds of ffm_flow_stages, one ghost exchange of the stages and one
        // all-reduce of "some ghost stage changed", until none does
        rc = allreduce_host_values(c, &total, 1, 0);
        std::vector<int> ghostStage((size_t)std::max(nG, 1), 0), got((size_t)std::max(nG, 1), 0);
        while (rc == FFM_OK) {
            if (fail == FFM_OK) fail = ffm_flow_stages(N, nG, (int)l.size(), l.data(), u.data(), cu.data(), cl.data(), ghostStage.data(), stage.data(), order.data(), &o->nLevels);
            int top = -1;
            for (int i = 0; i < N; i++) top = std::max(top, stage[i]);
            // the owned cells' stages to the neighbours' ghost cells: one ghost exchange of a double field (small integers: exact)
            if (fail == FFM_OK) rc = ffm_h2d(c, o->stage, stage.data(), sizeof(int) * (size_t)N);
            if (rc != FFM_OK) break;
            if (fail == FFM_OK && N) hipLaunchKernelGGL(k_int_to_double, dim3(sgrid(N)), dim3(256), 0, s, (long)N, o->stage, x);
            else if ((rc = ffm_dzero(c, x, sizeof(double) * (size_t)A->nCells)) != FFM_OK) break;
            if ((rc = ffm_ghost_exchange(A, x)) != FFM_OK) break;
            bool changed = false;
            if (fail == FFM_OK && nG) {
                hipLaunchKernelGGL(k_double_to_int, dim3(sgrid(nG)), dim3(256), 0, s, (long)nG, x + N, o->ghostStage);
                if ((rc = ffm_d2h(c, got.data(), o->ghostStage, sizeof(int) * (size_t)nG)) != FFM_OK) break;
                changed = got != ghostStage;
                ghostStage = got;
            }
            double v[3] = {changed ? 1.0 : 0.0, fail != FFM_OK ? 1.0 : 0.0, (double)top};
            if ((rc = allreduce_host_values(c, v, 3, 1)) != FFM_OK) break;
            anyFail = v[1] != 0.0; cycle = v[2] > total; o->nStages = (int)v[2] + 1;
            if (anyFail || cycle || v[0] == 0.0) break;
        }
    }
    if (rc == FFM_OK && hipGetLastError() != hipSuccess) { ffm_set_error("%s: a kernel launch failed", who); rc = FFM_ERR_HIP; }
    if (rc == FFM_OK && fail != FFM_OK) rc = fail;        // (ffm_flow_levels, ffm_flow_stages or the allocation has set the message)
    else if (rc == FFM_OK && anyFail) { ffm_set_error("%s: refused on another rank (a cycle among its cells, or out of memory)", who); rc = FFM_ERR_UNSUPPORTED; }
    else if (rc == FFM_OK && cycle) {
        ffm_set_error("%s: a stage above the %.0f ghost cells of all ranks: the non-zero off-diagonal coefficients form a cycle through several ranks", who, total);
        rc = FFM_ERR_UNSUPPORTED;
    }
    if (rc == FFM_OK) {
        o->stageStart.assign((size_t)o->nStages + 1, 0);
        for (int i = 0; i < N; i++) o->stageStart[stage[i] + 1]++;
        for (int k = 0; k < o->nStages; k++) o->stageStart[k + 1] += o->stageStart[k];
        rc = ffm_h2d(c, o->order, order.data(), sizeof(int) * (size_t)N);
    }
    if (rc != FFM_OK) { ffm_flow_order_destroy(o); return rc; }
    *out = o;
    return FFM_OK;
}
extern "C" int ffm_flow_order_create(ffm_ldu *A, ffm_flow_order **out) { return flow_order_create(A, false, out); }
extern "C" int ffm_flow_order_create_staged(ffm_ldu *A, ffm_flow_order **out) { return flow_order_create(A, true, out); }
extern "C" int ffm_flow_order_nlevels(const ffm_flow_order *o) { return o ? o->nLevels : FFM_ERR_ARG; }
extern "C" int ffm_flow_order_nstages(const ffm_flow_order *o) { return o ? (o->staged ? o->nStages : 0) : FFM_ERR_ARG; }
extern "C" int ffm_flow_order_destroy(ffm_flow_order *o)
{
    if (!o) return FFM_OK;
    hipSetDevice(o->ctx->device);
    hipStreamSynchronize(o->ctx->stream);
    hipFree(o->order); hipFree(o->stage); hipFree(o->ghostStage);
    delete o;
    return FFM_OK;
}

// ranks false: the single-rank entry.  It may be called on a rank of several and never communicates: no all-reduce, no exchange
// (one stage), the norms of this rank's rows
static int solve_ordered(ffm_ldu *A, const ffm_flow_order *o, bool ranks, double *psi_d, const double *source_d, ffm_perf *out)
{
    const char *who = ranks ? "ffm_solve_ordered_staged_d" : "ffm_solve_ordered_d";
    if (!A || !o || !psi_d || !source_d || !out) { ffm_set_error("%s: null argument", who); return FFM_ERR_ARG; }
    FFM_TRY(ordered_refuse(A, ranks, who));
    memset(out, 0, sizeof(*out));
    FFM_HIP(hipSetDevice(A->ctx->device));
    ffm_ctx *c = A->ctx; hipStream_t s = c->stream; const long N = A->nOwned;
    // ---- 1. the order against the coefficients the matrix holds now, over all ranks; nothing else is launched or exchanged before
    const bool mine = o->ctx == A->ctx && o->staged == ranks && o->N == A->nOwned && o->nGhost == A->nCells - A->nOwned;
    const int g = sgrid(N);
    double v[3] = {1.0, (double)o->nStages, -(double)o->nStages};
    if (mine) {
        double *posBuf;
        FFM_TRY(ffm_ldu_work(A, 23, &posBuf));
        int *pos = (int *)posBuf;
        hipLaunchKernelGGL(k_order_pos, dim3(g), dim3(256), 0, s, N, o->order, pos);
        FFM_DISPATCH_W(A->maxW, hipLaunchKernelGGL(k_order_check<W>, dim3(g), dim3(256), 0, s, ffm_view(A), A->upper, A->lower, pos, o->stage, o->ghostStage, c->partials_d));
        FFM_HIP(hipGetLastError());
        FFM_TRY(partial_sum_to(c, g, S_TMP0));
        FFM_TRY(ffm_read_scalars(c));
        v[0] = c->scal_h[S_TMP0];
    }
    const double bad = v[0];
    if (ranks) FFM_TRY(allreduce_host_values(c, v, 3, 1));
    if (!(v[0] == 0.0) || v[1] != -v[2]) {
        if (!mine) ffm_set_error("%s: the order belongs to another matrix (%d cells, %d ghost cells, %d stages, made by ffm_flow_order_create%s; matrix %d, %d): nothing solved",
                                 who, o->N, o->nGhost, o->nStages, o->staged ? "_staged" : "", A->nOwned, A->nCells - A->nOwned);
        else if (!(bad == 0.0)) ffm_set_error("%s: %.0f non-zero entries do not precede their rows in this order or reach a ghost cell of a stage not below their "
                                              "row's (a stale order, the order of another matrix, or a matrix that is not triangular): nothing solved", who, bad);
        else if (v[1] != -v[2]) ffm_set_error("%s: the ranks' orders have %.0f to %.0f stages (orders of different matrices): nothing solved", who, -v[2], v[1]);
        else ffm_set_error("%s: the order was refused on another rank: nothing solved", who);
        return FFM_ERR_UNSUPPORTED;
    }
    // ---- 2. the stages, on the internal numbering
    const double *si = source_d; double *pi = psi_d;
    if (!A->identity) {
        FFM_TRY(ffm_to_internal(A, source_d, 1, &si));
        const double *pin; FFM_TRY(ffm_to_internal(A, psi_d, 2, &pin)); pi = A->permIn[2];
    }
    double *rA;
    FFM_TRY(exact_solve_begin(A, ranks, pi, si, &rA, out));
    OrderedArgs a{};
    a.v = ffm_view(A); a.N = A->nOwned; a.nap = 1; a.order = o->order;
    a.upper = A->upper; a.lower = A->lower; a.diag = A->diag; a.source = si; a.psi = pi; a.ticket = A->sweepTicket;
    FFM_TRY(ffm_ldu_work(A, 20, &a.mf));
    hipLaunchKernelGGL(k_flow_fill, dim3(g), dim3(256), 0, s, N, a.mf, (double *)nullptr, (double *)nullptr, a.ticket);
    for (int st = 0; st < o->nStages; st++) {
        const int p0 = o->stageStart[st], p1 = o->stageStart[st + 1], nChunk = (p1 - p0 + FLOW_T - 1) / FLOW_T;
        if (nChunk > 0) {
            if (st > 0) FFM_TRY(ffm_dzero(c, a.ticket, sizeof(unsigned int)));          // the ticket counter; the abort word stays
            if (o->nGhost) FFM_DISPATCH_W(A->maxW, hipLaunchKernelGGL((k_flow_ordered<W, true>), dim3(nChunk), dim3(FLOW_T), 0, s, a, p0, p1));
            else FFM_DISPATCH_W(A->maxW, hipLaunchKernelGGL((k_flow_ordered<W, false>), dim3(nChunk), dim3(FLOW_T), 0, s, a, p0, p1));
            FFM_HIP(hipGetLastError());
        }
        if (st + 1 < o->nStages) FFM_TRY(ffm_ghost_exchange(A, pi));                    // every rank, also one whose stage was empty
    }
    // ---- 3. what the solve left
    return exact_solve_record(A, ranks, who, pi, si, rA, A->identity ? nullptr : psi_d, out);
}
// `out` is zeroed before an order is refused (a null argument and a matrix of the other kind are refused before)
extern "C" int ffm_solve_ordered_d(ffm_ldu *A, const ffm_flow_order *o, double *psi_d, const double *source_d, ffm_perf *out)
{ return solve_ordered(A, o, false, psi_d, source_d, out); }
extern "C" int ffm_solve_ordered_staged_d(ffm_ldu *A, const ffm_flow_order *o, double *psi_d, const double *source_d, ffm_perf *out)
{ return solve_ordered(A, o, true, psi_d, source_d, out); }

// ------------------------------------------------------------------ several systems with common off-diagonals ---
// PBiCGStab + DILU (or DIC) of nSys <= FFM_TILE_MAXSYS systems as the lanes of one pbicgstab_lanes (above); one system is the matrix's
// own lane.  Everything else goes one system after the other through ffm_solve_d.
extern "C" int ffm_solve_multi_d(ffm_ldu *A, int nSys, int solver, int precond, double tol, double relTol, int minIter, int maxIter,
                                 const double *const *diag_d, const double *upper_d, const double *lower_d, double *const *psi_d,
                                 const double *const *source_d, ffm_perf *out)
{
    if (!A || nSys < 1 || !diag_d || !psi_d || !source_d || !out) { ffm_set_error("ffm_solve_multi_d: null argument"); return FFM_ERR_ARG; }
    for (int i = 0; i < nSys; i++) if (!diag_d[i] || !psi_d[i] || !source_d[i]) { ffm_set_error("ffm_solve_multi_d: null array"); return FFM_ERR_ARG; }
    FFM_HIP(hipSetDevice(A->ctx->device));
    Controls k{tol, relTol, minIter, maxIter, 1};
    // several lanes need the tiled sweeps of several systems (five systems the short LDS ring: a plan whose ring neighbours lie too far
    // apart for it solves them one after the other); one lane needs the vectors in the library's cell order only
    const bool lanes = nSys <= FFM_TILE_MAXSYS && solver == FFM_PBICGSTAB && (precond == FFM_DILU || precond == FFM_DIC) && A->identity &&
                       (nSys == 1 || (A->sweepMode == 2 && ffm_tile_multi_fits(A, nSys) && A->ifaces.empty()));
    if (!lanes) {          // one after the other (any solver, any matrix)
        for (int i = 0; i < nSys; i++) {
            FFM_TRY(ffm_ldu_bind_coeffs_native_d(A, diag_d[i], upper_d, lower_d, i > 0));
            FFM_TRY(ffm_solve_d(A, solver, precond, tol, relTol, minIter, maxIter, 1, psi_d[i], source_d[i], &out[i]));
        }
        return FFM_OK;
    }
    FFM_TRY(ffm_ldu_bind_coeffs_native_d(A, diag_d[0], upper_d, lower_d, 0));
    if (precond == FFM_DIC && !A->symmetric) { ffm_set_error("DIC needs a symmetric matrix"); return FFM_ERR_UNSUPPORTED; }
    ffm_ctx *c = A->ctx;
    if (nSys > 1 && !c->multiScal_d) {
        FFM_HIP(hipMalloc((void **)&c->multiScal_d, sizeof(double) * NSCAL * FFM_TILE_MAXSYS));
        FFM_HIP(hipHostMalloc((void **)&c->multiScal_h, sizeof(double) * NSCAL * FFM_TILE_MAXSYS, hipHostMallocDefault));
        FFM_HIP(hipMemsetAsync(c->multiScal_d, 0, sizeof(double) * NSCAL * FFM_TILE_MAXSYS, c->stream));
    }
    Lane L[FFM_TILE_MAXSYS];
    for (int i = 0; i < nSys; i++) {
        Lane &l = L[i];
        memset(&out[i], 0, sizeof(ffm_perf));
        l = own_lane(A, psi_d[i], source_d[i], &out[i]);            // lane 0 keeps the matrix's rD and the solvers' work vectors 1-8
        if (nSys > 1) { l.diag = diag_d[i]; l.scal_d = c->multiScal_d + (size_t)i * NSCAL; l.scal_h = c->multiScal_h + (size_t)i * NSCAL; }
        if (i > 0) { l.work = 32 + 9 * (i - 1); FFM_TRY(ffm_ldu_work(A, l.work, &l.rD)); }
    }
    FFM_TRY(pbicgstab_lanes(A, precond, k, nSys, L));
    FFM_HIP(hipStreamSynchronize(c->stream));
    FFM_TRY(ffm_sweep_check_abort(A));
    return FFM_OK;
}

extern "C" int ffm_solve(ffm_ldu *A, int solver, int precond, double tol, double relTol, int minIter, int maxIter,
                         int nSweeps, double *psi, const double *source, ffm_perf *out)
{
    if (!A || !psi || !source || !out) return FFM_ERR_ARG;
    double *p = nullptr, *b = nullptr;
    const size_t nb = sizeof(double) * (size_t)std::max(A->nCells, 1);
    FFM_HIP(hipMalloc((void **)&p, nb)); FFM_HIP(hipMalloc((void **)&b, nb));
    FFM_TRY(ffm_h2d(A->ctx, p, psi, sizeof(double) * A->nOwned));
    FFM_TRY(ffm_h2d(A->ctx, b, source, sizeof(double) * A->nOwned));
    int rc = ffm_solve_d(A, solver, precond, tol, relTol, minIter, maxIter, nSweeps, p, b, out);
    if (!rc) rc = ffm_d2h(A->ctx, psi, p, sizeof(double) * A->nOwned);
    hipFree(p); hipFree(b);
    return rc;
}

// ------------------------------------------- preconditioner entry (tests) ---
extern "C" int ffm_precond_setup(ffm_ldu *A, int precond, double *rD_out_d)
{
    if (!A) return FFM_ERR_ARG;
    FFM_TRY(ffm_precond_setup_i(A, precond));
    if (rD_out_d) FFM_TRY(ffm_from_internal(A, A->rD, rD_out_d));
    FFM_HIP(hipStreamSynchronize(A->ctx->stream));
    FFM_TRY(ffm_sweep_check_abort(A));
    return FFM_OK;
}

// the reciprocal diagonals of several systems from the one sweep of the lock-step solves (tests)
extern "C" int ffm_precond_setup_multi(ffm_ldu *A, int precond, int nSys, const double *const *diag_d, double *const *rD_out_d)
{
    if (!A || !diag_d || !rD_out_d || nSys < 2 || nSys > FFM_TILE_MAXSYS) { ffm_set_error("ffm_precond_setup_multi: bad argument"); return FFM_ERR_ARG; }
    if (precond != FFM_DIC && precond != FFM_DILU) { ffm_set_error("ffm_precond_setup_multi: DIC or DILU"); return FFM_ERR_UNSUPPORTED; }
    if (!(A->identity && A->sweepMode == 2 && ffm_tile_usable(A))) { ffm_set_error("ffm_precond_setup_multi needs a tiled matrix in the library's cell order"); return FFM_ERR_UNSUPPORTED; }
    if (!ffm_tile_multi_fits(A, nSys)) { ffm_set_error("ffm_precond_setup_multi: %d systems do not fit the LDS rings of this matrix's tile plan", nSys); return FFM_ERR_UNSUPPORTED; }
    if (precond == FFM_DIC && !A->symmetric) { ffm_set_error("DIC needs a symmetric matrix"); return FFM_ERR_UNSUPPORTED; }
    for (int i = 0; i < nSys; i++) if (!diag_d[i] || !rD_out_d[i]) { ffm_set_error("ffm_precond_setup_multi: null array"); return FFM_ERR_ARG; }
    FFM_HIP(hipSetDevice(A->ctx->device));
    FFM_TRY(ffm_tile_calc_rD(A, nSys, diag_d, rD_out_d));
    FFM_HIP(hipStreamSynchronize(A->ctx->stream));
    FFM_TRY(ffm_sweep_check_abort(A));
    return FFM_OK;
}

// timing helper for bench.py: `reps` preconditioner applications (DIC: a forward and a backward sweep each) on the matrix bound
// to the LDU, bracketed by HIP events on the context stream; average time of ONE application in milliseconds
extern "C" int ffm_bench_precond(ffm_ldu *A, int precond, const double *r_d, double *w_d, int reps, double *avg_ms)
{
    if (!A || !r_d || !w_d || reps < 1 || !avg_ms) return FFM_ERR_ARG;
    if (!A->identity) { ffm_set_error("ffm_bench_precond needs an LDU in the library's cell order"); return FFM_ERR_UNSUPPORTED; }
    FFM_TRY(ffm_precond_setup_i(A, precond));
    FFM_TRY(ffm_precond_apply_i(A, precond, false, r_d, w_d));      // warm-up
    hipEvent_t e0, e1;
    FFM_HIP(hipEventCreate(&e0)); FFM_HIP(hipEventCreate(&e1));
    FFM_HIP(hipEventRecord(e0, A->ctx->stream));
    for (int i = 0; i < reps; i++) FFM_TRY(ffm_precond_apply_i(A, precond, false, r_d, w_d));
    FFM_HIP(hipEventRecord(e1, A->ctx->stream));
    FFM_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    FFM_HIP(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0); hipEventDestroy(e1);
    *avg_ms = (double)ms / reps;
    return FFM_OK;
}

extern "C" int ffm_precond_apply(ffm_ldu *A, int precond, int transpose, const double *r_d, double *w_d)
{
    if (!A || !r_d || !w_d) return FFM_ERR_ARG;
    FFM_TRY(ffm_precond_setup_i(A, precond));
    const double *ri; FFM_TRY(ffm_to_internal(A, r_d, 0, &ri));
    if (A->identity) { FFM_TRY(ffm_precond_apply_i(A, precond, transpose != 0, ri, w_d)); }
    else {
        double *wi; FFM_TRY(ffm_ldu_work(A, 0, &wi));
        FFM_TRY(ffm_precond_apply_i(A, precond, transpose != 0, ri, wi));
        FFM_TRY(ffm_from_internal(A, wi, w_d));
    }
    FFM_HIP(hipStreamSynchronize(A->ctx->stream));
    FFM_TRY(ffm_sweep_check_abort(A));
    return FFM_OK;
}

extern "C" int ffm_gs_smooth(ffm_ldu *A, int symmetric_sweep, int nSweeps, double *psi_d, const double *b_d)
{
    if (!A || !psi_d || !b_d || nSweeps < 1) return FFM_ERR_ARG;
    if (A->identity) { FFM_TRY(ffm_gs_smooth_i(A, symmetric_sweep != 0, nSweeps, psi_d, b_d)); }
    else {
        const double *bi, *pin;
        FFM_TRY(ffm_to_internal(A, b_d, 1, &bi)); FFM_TRY(ffm_to_internal(A, psi_d, 2, &pin));
        FFM_TRY(ffm_gs_smooth_i(A, symmetric_sweep != 0, nSweeps, A->permIn[2], bi));
        FFM_TRY(ffm_from_internal(A, A->permIn[2], psi_d));
    }
    FFM_HIP(hipStreamSynchronize(A->ctx->stream));
    FFM_TRY(ffm_sweep_check_abort(A));
    return FFM_OK;
}
