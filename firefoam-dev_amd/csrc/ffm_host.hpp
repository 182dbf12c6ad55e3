// ffm_host.hpp -- the host-only part of libffm's private declarations: what a translation unit without device code and without a ROCm
// header (ffm_ldu_analysis.cpp) needs.  ffm_internal.hpp includes it, so the device translation units see the same definitions.
#pragma once
#include <ctime>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <thread>
#include <algorithm>

#include "../../include/ffm.h"

void ffm_set_error(const char *fmt, ...);

#define FFM_TRY(call)                                                            \
    do {                                                                         \
        int r_ = (call);                                                         \
        if (r_ != FFM_OK) return r_;                                             \
    } while (0)

// Host set-up loops over cells / faces (renumbered addressing, geometry in the native layout, the reconstruction tensors): independent
// iterations split over the host's cores (at most 16 threads; FFM_HOST_THREADS overrides; below 1M iterations: the caller's thread)
template <class Fn> inline void ffm_parallel_for(long n, Fn fn, long serialBelow = 1L << 20)
{
    static const int nT = [] { const char *e = getenv("FFM_HOST_THREADS"); int t = e ? atoi(e) : (int)std::thread::hardware_concurrency(); return std::max(1, std::min(t, 16)); }();
    if (n < serialBelow || nT == 1) { fn(0L, n); return; }
    std::vector<std::thread> th;
    const long chunk = (n + nT - 1) / nT;
    for (int t = 0; t < nT; t++) { const long lo = t * chunk, hi = std::min(n, lo + chunk); if (lo < hi) th.emplace_back([=] { fn(lo, hi); }); }
    for (auto &x : th) x.join();
}

// FFM_TIMING=1: wall time of the host-side set-up stages to stderr
struct FfmStageTimer {
    const char *what; double t0; bool on;
    static double now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
    explicit FfmStageTimer(const char *w) : what(w), t0(now()), on(getenv("FFM_TIMING") != nullptr) {}
    ~FfmStageTimer() { if (on) fprintf(stderr, "ffm timing: %-28s %.2f s\n", what, now() - t0); }
};
// the same in laps: lap("x") prints the time since the previous lap (FFM_TIMING=2)
struct FfmLapTimer {
    const char *what; double t0; bool on;
    explicit FfmLapTimer(const char *w) : what(w), t0(FfmStageTimer::now()), on(getenv("FFM_TIMING") != nullptr && atoi(getenv("FFM_TIMING")) >= 2) {}
    void lap(const char *stage) { if (!on) return; const double t = FfmStageTimer::now(); fprintf(stderr, "ffm timing:   %s: %-30s %.2f s\n", what, stage, t - t0); t0 = t; }
};
// edge of the 2-D tiles of cell columns, in cells: detected blockMesh boxes, the plume's group hint, ffm_tile_hint_from_centres
constexpr int TILE_EDGE = 16;
// label of the 2-D tile (a, b) of cell columns.  Ties between tiles that are ready at the same time are broken by label
// (ffm_ldu_analysis.cpp: rank_groups), so the label orders the tickets: anti-diagonal major = the order of the sweep's wavefront
static inline int ffm_tile_label(int a, int b)
{
    a = a < 2047 ? a : 2047; b = b < 2047 ? b : 2047;
    return (a + b) * 4096 + b;
}
constexpr int FFM_TILE_W = 3;       // tiled sweeps: neighbour slots per cell and direction (hexahedra: 3)

// ---- dependency analysis and layout of an LDU matrix (ffm_ldu_analysis.cpp) ----
// What the analysis decides about a matrix before any kernel runs: the internal cell and face numbering, the dependency levels of the
// sweeps and, for the tiled sweeps, the groups.
struct LduAnalysis {
    std::vector<int> newToOldCell, oldToNewCell, newToOldFace;
    std::vector<int> l, u;                 // new numbering, upper-triangular order
    std::vector<int> fwdLevelStart;        // [nLevels+1]
    std::vector<int> bwdLevelStart;        // [nBwd+1] into bwdOrder
    std::vector<int> bwdOrder;             // cells sorted by backward level (the order of the dataflow sweeps' backward chunks)
    bool identity = true;
    // group plan of the tiled sweeps (mode 2)
    int mode = 0, nGroups = 0; bool bwdIsReverse = false;
    std::vector<int> levNew, blNew;         // forward / backward level of every owned cell (new numbering)
    std::vector<int> grpCell;
};
// The sliced owner-ELL addressing of an analysed matrix (struct ffm_ldu in ffm_internal.hpp describes the arrays) and the XCD row
// schedule, on the host.
struct LduLayout {
    int nSlices = 0, upTotal = 0, loTotal = 0;
    int upWidthUniform = -1, loWidthUniform = -1, maxW = 0;
    int loShift = 4;                             // bits of the slot field of loEnt: 4, or 5 where a cell owns more than 16 faces towards owned cells
    std::vector<int> upOff, loOff;               // [nSlices+1]
    std::vector<int> upNbr, faceSrc;             // [max(upTotal, 1)]
    std::vector<int> loEnt;                      // [max(loTotal, 1)]
    std::vector<int> callerToNative;             // [F]
    std::vector<int> rowSched;
};
// the analysis of ffm_ldu_create*: the one the last ffm_renumber_hint left behind if it fits, a fresh one otherwise
int ffm_ldu_analysis(int nOwn, int nGhost, int F, const int *l, const int *u, const int *groupHint, int forceMode, LduAnalysis &a);
int ffm_ldu_layout(const LduAnalysis &a, int nOwn, int nGhost, int F, LduLayout &L);
bool ffm_tile_feasible(int nOwn, int F, const int *l, const int *u);

// ---- content sharing of the tile plans' neighbour-code blocks (ffm_tile_share.cpp) ----
int ffm_tile_share(std::vector<unsigned short> &codes, const std::vector<long> &start, const std::vector<int> &len, bool share, long padShorts,
                   std::vector<unsigned short> &pool, std::vector<unsigned> &off, long *uniqueBytes, long *totalBytes, const char *what);
bool ffm_tile_share_enabled(int reader);      // reader: 1 the sweeps, 2 the tiled Amul (FFM_TILE_CODE_SHARE)
