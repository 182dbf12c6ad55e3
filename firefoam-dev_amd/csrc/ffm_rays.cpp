// ffm_rays.cpp -- the tick schedule of the direction-ordered fvDOM ray solves on a box of blocks (pure host code, no HIP).
// For one ray direction the blocks of a box decomposition form a DAG: block b receives intensity from its face neighbour on
// the upstream side of every axis.  All rays of an octant share that DAG, so they are pipelined through it: the block at
// Manhattan distance s from the octant's upstream corner (its stage) solves the octant's r-th ray at tick r + s.  An octant
// with r > 0 rays on a grid with S = (px - 1) + (py - 1) + (pz - 1) + 1 stages takes r + S - 1 ticks (an octant without rays:
// none), and the octants follow one another in the order of their index.  Every rank computes the same tick count, so a
// sweep that enters one exchange per tick cannot hang.
#include "../../include/ffm.h"

// Octant index of a direction: bit a is set where component a is negative.  A component that is not negative -- +0.0 and
// -0.0 included -- counts as positive: the sign rule of the upwind weights (w = 1 where d & Sf >= 0) on a face whose normal
// points along +a.
static inline int octant_of(const double *d) { return (d[0] < 0 ? 1 : 0) | (d[1] < 0 ? 2 : 0) | (d[2] < 0 ? 4 : 0); }

extern "C" int ffm_ray_octant(const double *d3) { return d3 ? octant_of(d3) : FFM_ERR_ARG; }

extern "C" int ffm_ray_schedule(int px, int py, int pz, int bx, int by, int bz, int nRay, const double *dAve, int *tickRay, int cap)
{
    if (px < 1 || py < 1 || pz < 1 || bx < 0 || by < 0 || bz < 0 || bx >= px || by >= py || bz >= pz || nRay < 0 || (nRay && !dAve) || cap < 0 ||
        (cap && !tickRay)) return FFM_ERR_ARG;
    const int S = (px - 1) + (py - 1) + (pz - 1) + 1;
    int t0 = 0;                                                  // first tick of the octant
    for (int o = 0; o < 8; o++) {
        int r = 0;
        for (int i = 0; i < nRay; i++) r += octant_of(dAve + 3 * i) == o;
        if (!r) continue;
        // stage: blocks between this one and the upstream corner, axis by axis (upstream = block 0 where the rays run along +a)
        const int s = ((o & 1) ? px - 1 - bx : bx) + ((o & 2) ? py - 1 - by : by) + ((o & 4) ? pz - 1 - bz : bz);
        const int nTicks = r + S - 1;
        for (int t = 0; t < nTicks && t0 + t < cap; t++) tickRay[t0 + t] = -1;
        int k = 0;                                               // the octant's rays in ray-index order
        for (int i = 0; i < nRay; i++) if (octant_of(dAve + 3 * i) == o) {
            if (t0 + k + s < cap) tickRay[t0 + k + s] = i;
            k++;
        }
        t0 += nTicks;
    }
    return t0;
}

// ---------------------------------------------------------------------------------------------- flow order of a ray matrix ---
// An upwind ray matrix has at most one non-zero off-diagonal coefficient per face, so its rows form a dependency graph: row u[f]
// needs cell l[f] where lower[f] != 0, row l[f] needs cell u[f] where upper[f] != 0, a face with two zeros is no edge.  Where
// that graph has no cycle the matrix is triangular under the level-major cell order found here (level = longest dependency
// path; ascending cell index inside a level), and one forward substitution in that order is the exact solve
// (ffm_solve_ordered_d).  Kahn's algorithm, O(nCells + nFaces), one thread.  A cycle -- a face with two non-zero coefficients
// is the shortest -- is refused.
#include <vector>
void ffm_set_error(const char *fmt, ...);

// Kahn over one rank's rows: nOwned cells with rows, nGhost ghost cells (indices nOwned ..) that are sources of the stage another
// rank found.  Finds level (longest dependency path in the owned sub-graph) and stage (below) of every owned cell and the order
// stage-major, level-major inside a stage, ascending cell index inside a level.  Without ghost cells every stage is 0 and the order
// is the level-major one.  `who`: the public function, for the messages, which speak of ghost cells where `staged`; stage may be null.
static int flow_kahn(const char *who, bool staged, int nOwned, int nGhost, int nFaces, const int *lowerAddr, const int *upperAddr, const double *upper,
                     const double *lower, const int *ghostStage, int *stage, int *order, int *nLevels)
{
    const int N = nOwned, M = nOwned + nGhost, F = nFaces;
    for (int f = 0; f < F; f++)
        if (lowerAddr[f] < 0 || lowerAddr[f] >= M || upperAddr[f] < 0 || upperAddr[f] >= M) {
            if (staged) ffm_set_error("%s: face %d joins cells %d and %d of %d (+ %d ghost cells)", who, f, lowerAddr[f], upperAddr[f], N, nGhost);
            else ffm_set_error("%s: face %d joins cells %d and %d of %d", who, f, lowerAddr[f], upperAddr[f], N);
            return FFM_ERR_ARG;
        }
    for (int g = 0; g < nGhost; g++) if (ghostStage[g] < 0) { ffm_set_error("%s: ghost cell %d has stage %d", who, g, ghostStage[g]); return FFM_ERR_ARG; }
    // the owned sub-graph (successors of every owned cell, CSR) and what the ghost cells impose
    std::vector<int> start(N + 1, 0), indeg(N, 0), stg(N, 0);
    auto each_edge = [&](auto &&owned, auto &&ghost) {          // edge src -> dst: row dst needs cell src
        auto edge = [&](int src, int dst) { if (dst < N) { if (src < N) owned(src, dst); else ghost(src - N, dst); } };
        for (int f = 0; f < F; f++) {
            if (lower[f] != 0) edge(lowerAddr[f], upperAddr[f]);
            if (upper[f] != 0) edge(upperAddr[f], lowerAddr[f]);
        }
    };
    each_edge([&](int s, int d) { start[s + 1]++; indeg[d]++; },
              [&](int g, int d) { if (stg[d] < ghostStage[g] + 1) stg[d] = ghostStage[g] + 1; });
    for (int c = 0; c < N; c++) start[c + 1] += start[c];
    std::vector<int> succ(start[N]), fill(start.begin(), start.end() - 1);
    each_edge([&](int s, int d) { succ[fill[s]++] = d; }, [](int, int) {});
    std::vector<int> lev(N, 0), queue;
    queue.reserve(N);
    for (int c = 0; c < N; c++) if (!indeg[c]) queue.push_back(c);
    int nLev = 0, nStg = 0;
    for (size_t q = 0; q < queue.size(); q++) {
        const int c = queue[q];
        nLev = nLev > lev[c] + 1 ? nLev : lev[c] + 1;
        nStg = nStg > stg[c] + 1 ? nStg : stg[c] + 1;
        for (int k = start[c]; k < start[c + 1]; k++) {
            const int r = succ[k];
            if (lev[r] < lev[c] + 1) lev[r] = lev[c] + 1;
            if (nGhost && stg[r] < stg[c]) stg[r] = stg[c];          // (without ghost cells every stage stays 0)
            if (--indeg[r] == 0) queue.push_back(r);
        }
    }
    if ((int)queue.size() != N) {
        ffm_set_error("%s: the non-zero off-diagonal coefficients form a cycle through %d of %d %scells: "
                      "the matrix is not triangular under any cell order", who, N - (int)queue.size(), N, staged ? "owned " : "");
        return FFM_ERR_UNSUPPORTED;
    }
    // two stable counting sorts, by level, then by stage (the identity where there is one stage: left out)
    std::vector<int> pos(nLev + 1, 0);
    for (int c = 0; c < N; c++) pos[lev[c] + 1]++;
    for (int i = 0; i < nLev; i++) pos[i + 1] += pos[i];
    for (int c = 0; c < N; c++) order[pos[lev[c]]++] = c;
    if (nStg > 1) {
        const std::vector<int> byLev(order, order + N);
        pos.assign(nStg + 1, 0);
        for (int c = 0; c < N; c++) pos[stg[c] + 1]++;
        for (int i = 0; i < nStg; i++) pos[i + 1] += pos[i];
        for (int i = 0; i < N; i++) { const int c = byLev[i]; order[pos[stg[c]]++] = c; }
    }
    if (stage) for (int c = 0; c < N; c++) stage[c] = stg[c];
    *nLevels = nLev;
    return FFM_OK;
}

extern "C" int ffm_flow_levels(int nCells, int nFaces, const int *lowerAddr, const int *upperAddr, const double *upper, const double *lower,
                               int *order, int *nLevels)
{
    if (nCells < 0 || nFaces < 0 || (nFaces && (!lowerAddr || !upperAddr || !upper || !lower)) || (nCells && !order) || !nLevels) return FFM_ERR_ARG;
    return flow_kahn("ffm_flow_levels", false, nCells, 0, nFaces, lowerAddr, upperAddr, upper, lower, nullptr, nullptr, order, nLevels);
}

// ------------------------------------------------------------------------------- stages of a ray matrix on one rank's sub-domain ---
// The decomposed form of the order above.  A rank holds rows for its nOwned cells; its nGhost ghost cells (indices nOwned ..) are
// sources whose stage another rank found.  The stage of a cell is the largest number of rank crossings on any upstream path to it:
// stage[c] = max over the cells u that row c needs of stage[u] (u owned) or ghostStage[u] + 1 (u a ghost cell), 0 without any.  All
// rows of stage s then need owned cells of stage <= s and ghost cells of stage < s only: a rank solves them in one sweep once the
// ghost values of the stages before have arrived.  order: the owned cells stage-major, inside a stage level-major by the levels of
// ffm_flow_levels on the owned sub-graph (ascending cell index inside a level) -- a non-zero owned column has a stage no larger
// and a level smaller than its row's, so it stands before the row.  nLevels: the level count of the owned sub-graph.  Edges
// between two ghost cells, and the edge that a ghost cell's (absent) row would need, are no dependencies of this rank.  A cycle among
// the owned cells is refused; a cycle through several ranks is invisible here (ffm_flow_order_create_staged bounds the stages).
extern "C" int ffm_flow_stages(int nOwned, int nGhost, int nFaces, const int *lowerAddr, const int *upperAddr, const double *upper,
                               const double *lower, const int *ghostStage, int *stage, int *order, int *nLevels)
{
    if (nOwned < 0 || nGhost < 0 || nFaces < 0 || (nFaces && (!lowerAddr || !upperAddr || !upper || !lower)) || (nGhost && !ghostStage) ||
        (nOwned && (!stage || !order)) || !nLevels) return FFM_ERR_ARG;
    return flow_kahn("ffm_flow_stages", true, nOwned, nGhost, nFaces, lowerAddr, upperAddr, upper, lower, ghostStage, stage, order, nLevels);
}
