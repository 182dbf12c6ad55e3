// ffm_ldu_analysis.cpp -- what ffm_ldu_create* and ffm_renumber_* decide about a matrix before any kernel runs: cell order, dependency
// levels, groups of the tiled sweeps, backward order (analyse), and the sliced owner-ELL layout with the XCD row schedule
// (ffm_ldu_layout).  Host code only, no ROCm header: g++ builds it stand-alone too, to be stepped through or run under a sanitizer.
//
// Cells are ordered level-major: level(c) = longest path to c in the DAG owner->neighbour, cells of one level contiguous and sorted by
// the caller's index (or group-major, then level-major, for the tiled sweeps).  The renumbering is a topological order of the same
// DAG, so owner<neighbour is preserved and the incomplete factorisations are the same operators as in the caller's numbering.
#include "ffm_host.hpp"
#include <atomic>
#include <cmath>
#include <numeric>

// Sweep modes.  0 "levels": dataflow sweeps (level-major numbering, ffm_solve).  2 "tile": tiled wavefront sweep
// (ffm_tile).  Default (FFM_SWEEP unset or "auto"): tile when the caller gives a group hint or the mesh is a
// blockMesh-numbered box and the plan is feasible, levels otherwise.  FFM_SWEEP=tile also tiles un-hinted meshes (chunks of
// the cell order; tests).
enum { SWEEP_AUTO = 3 };
static int default_sweep_mode()
{
    const char *e = getenv("FFM_SWEEP");
    if (!e || e[0] == 'a' || e[0] == 'A') return SWEEP_AUTO;
    if (e[0] == 't' || e[0] == 'T' || e[0] == '2') return 2;
    return 0;
}

// The caller's addressing.  nOwn < N: cells [nOwn, N) are ghost cells (copies of neighbour-rank cells).  They own no faces, stay at
// the end of the numbering in their given order, take no part in the level structure, and faces towards them are ignored by the
// backward levels (block-Jacobi sweeps).
struct Addr { int N, nOwn, F; const int *l, *u; };

// blockMesh single-block numbering (c = i + nx*(j + ny*k), faces of c in the order +x, +y, +z): returns true and the box
static bool detect_box(int N, int F, const int *l, const int *u, int &nx, int &ny, int &nz)
{
    if (N < 8 || F < 3) return false;
    // nx: first cell without a face to c+1
    int f = 0; nx = 0;
    for (int c = 0; c < N; c++) {
        bool hasX = false;
        while (f < F && l[f] == c) { if (u[f] == c + 1) hasX = true; f++; }
        if (!hasX) { nx = c + 1; break; }
    }
    if (nx < 1 || N % nx) return false;
    // ny: number of rows until a row start has no face to c+nx
    std::vector<int> start(N + 1, 0);
    for (int q = 0; q < F; q++) start[l[q] + 1]++;
    for (int c = 0; c < N; c++) start[c + 1] += start[c];
    ny = 0;
    for (int j = 0; (long)j * nx < N; j++) {
        const int c = j * nx; bool hasY = false;
        for (int q = start[c]; q < start[c + 1]; q++) if (u[q] == c + nx) hasY = true;
        if (!hasY) { ny = j + 1; break; }
    }
    if (ny < 1 || (N / nx) % ny) return false;
    nz = N / nx / ny;
    if ((long)F != (long)(nx - 1) * ny * nz + (long)nx * (ny - 1) * nz + (long)nx * ny * (nz - 1)) return false;
    int q = 0;
    for (int k = 0; k < nz; k++) for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) {
        const int c = i + nx * (j + ny * k);
        if (i < nx - 1) { if (l[q] != c || u[q] != c + 1) return false; q++; }
        if (j < ny - 1) { if (l[q] != c || u[q] != c + nx) return false; q++; }
        if (k < nz - 1) { if (l[q] != c || u[q] != c + nx * ny) return false; q++; }
    }
    return q == F;
}

// ------------------------------------------- what a renumbering leaves behind ---
// ffm_renumber_* and ffm_ldu_create* are separate calls; two process-global memos carry the decisions of the first to the second.
//   Groups: every renumbering that chose tiled sweeps leaves its groups (contiguous cell ranges of the new numbering) under a
//     fingerprint of the renumbered addressing.  An analysis in automatic mode WITHOUT a hint takes them when its addressing has that
//     fingerprint, so creating the matrix from the renumbered mesh finds the groups again.  Eight lists; the oldest goes first; never
//     invalidated otherwise.
//   Analysis: ffm_renumber_hint without ghost cells that chose tiled sweeps leaves its whole analysis, in its own new numbering, with
//     the renumbered hint.  A caller that renumbers its mesh with it and then creates the matrix on the renumbered addressing with the
//     renumbered hint (the plume driver) would run the same analysis a second time and get identity permutations and the same levels,
//     groups and orders; ffm_ldu_analysis takes it instead, after checking that sizes, FFM_SWEEP, addressing and hint are exactly
//     those left behind.  One slot, emptied by its first use -- fitting or not -- and by the next ffm_renumber_hint / _levels_ext.
struct GroupMemo { unsigned long long key; int N, F; std::vector<int> grpCell; };
static std::vector<GroupMemo> g_groupMemo;
struct AnalysisMemo { bool valid = false; int N = 0, nOwn = 0, F = 0, sweepMode = 0; LduAnalysis a; std::vector<int> hint; };
static AnalysisMemo g_analysisMemo;

static unsigned long long addr_fingerprint(int N, int F, const int *l, const int *u)
{
    unsigned long long h = 0x9E3779B97F4A7C15ull ^ ((unsigned long long)N << 32) ^ (unsigned)F;
    for (int f = 0; f < F; f++) { h ^= (unsigned long long)(unsigned)l[f] | ((unsigned long long)(unsigned)u[f] << 32); h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 29; }
    return h;
}
static void memo_leave_groups(int N, int F, const LduAnalysis &a)
{
    if (a.mode != 2) return;
    GroupMemo m{addr_fingerprint(N, F, a.l.data(), a.u.data()), N, F, a.grpCell};
    for (auto &x : g_groupMemo) if (x.key == m.key && x.N == N && x.F == F) { x = m; return; }
    if (g_groupMemo.size() >= 8) g_groupMemo.erase(g_groupMemo.begin());
    g_groupMemo.push_back(std::move(m));
}
static const std::vector<int> *memo_groups(int N, int F, const int *l, const int *u)
{
    if (g_groupMemo.empty()) return nullptr;
    const unsigned long long key = addr_fingerprint(N, F, l, u);
    for (auto &x : g_groupMemo) if (x.key == key && x.N == N && x.F == F) return &x.grpCell;
    return nullptr;
}
// empties the slot; fills it (and takes a) when a is worth keeping
static void memo_leave_analysis(int nOwned, int nGhost, int nFaces, const int *groupHint, LduAnalysis &a)
{
    g_analysisMemo = AnalysisMemo();
    if (a.mode != 2 || !groupHint || nGhost != 0) return;
    AnalysisMemo &m = g_analysisMemo;
    m.N = nOwned; m.nOwn = nOwned; m.F = nFaces; m.sweepMode = default_sweep_mode();
    m.hint.resize(nOwned);
    { int *hp = m.hint.data(); const int *n2o = a.newToOldCell.data();
      ffm_parallel_for(nOwned, [=](long lo, long hi) { for (long c = lo; c < hi; c++) hp[c] = groupHint[n2o[c]]; }); }
    m.a = std::move(a);
    m.valid = true;
}
static bool same_ints(const int *x, const int *y, long n)
{
    std::atomic<int> differ(0);
    ffm_parallel_for(n, [&](long lo, long hi) { if (memcmp(x + lo, y + lo, sizeof(int) * (size_t)(hi - lo))) differ = 1; });
    return !differ;
}
static bool memo_take_analysis(int N, int nOwn, int F, const int *l, const int *u, const int *groupHint, LduAnalysis &a)
{
    AnalysisMemo m;
    std::swap(m, g_analysisMemo);
    if (!m.valid || !groupHint || m.N != N || m.nOwn != nOwn || m.F != F || m.sweepMode != default_sweep_mode()) return false;
    if (!same_ints(l, m.a.l.data(), F) || !same_ints(u, m.a.u.data(), F) || !same_ints(groupHint, m.hint.data(), nOwn)) return false;
    a = std::move(m.a);
    std::iota(a.newToOldCell.begin(), a.newToOldCell.end(), 0); a.oldToNewCell = a.newToOldCell;
    std::iota(a.newToOldFace.begin(), a.newToOldFace.end(), 0);
    a.identity = true;
    return true;
}

// ------------------------------------------------------ stages of analyse() ---
// Reads FFM_SWEEP / forceMode and the addressing; returns the sweep mode (0 or 2).  In automatic mode a mesh without a hint gets one in
// autoHint (groupHint then points at it): the groups a renumbering left for this addressing, or the 16 x 16 column tiles of a detected box.
static int pick_mode(const Addr &m, bool renumber, int forceMode, const int *&groupHint, std::vector<int> &autoHint)
{
    const int mode = forceMode >= 0 ? forceMode : default_sweep_mode();
    if (mode != SWEEP_AUTO) return mode;
    if (!renumber || m.nOwn <= 0 || (long)m.N * 24 >= (1L << 32)) return 0;      // (the tiled kernels use 32-bit byte offsets into their streams)
    int bx, by, bz;
    if (groupHint) return 2;
    if (const std::vector<int> *gc = memo_groups(m.N, m.F, m.l, m.u)) {
        autoHint.resize(m.nOwn);
        for (int g = 0; g + 1 < (int)gc->size(); g++) for (int c = (*gc)[g]; c < (*gc)[g + 1] && c < m.nOwn; c++) autoHint[c] = g;
    } else if (m.N == m.nOwn && detect_box(m.N, m.F, m.l, m.u, bx, by, bz)) {
        autoHint.resize(m.nOwn);
        for (int c = 0; c < m.nOwn; c++) autoHint[c] = ffm_tile_label(((c / bx) % by) / TILE_EDGE, (c / (bx * by)) / TILE_EDGE);
    } else return 0;
    groupHint = autoHint.data();
    return 2;
}

// Reads the addressing: 0 <= l < u < N, faces sorted by owner, no face owned by a ghost cell.
static int validate_addressing(const Addr &m)
{
    const int *l = m.l, *u = m.u;
    for (int f = 0; f < m.F; f++) {
        if (l[f] < 0 || u[f] >= m.N || l[f] >= u[f]) {
            ffm_set_error("LDU addressing: face %d has l=%d u=%d (need 0<=l<u<nCells=%d)", f, l[f], u[f], m.N);
            return FFM_ERR_ADDR;
        }
        if (f && l[f] < l[f - 1]) {
            ffm_set_error("LDU addressing: faces not sorted by owner at face %d", f);
            return FFM_ERR_ADDR;
        }
        if (l[f] >= m.nOwn) { ffm_set_error("LDU addressing: face %d is owned by a ghost cell", f); return FFM_ERR_ADDR; }
    }
    return FFM_OK;
}

// Reads the addressing; leaves the forward level of every cell (caller numbering) in lev and returns the number of levels.
static int forward_levels(const Addr &m, std::vector<int> &lev)
{
    lev.assign(m.N, 0);
    for (int f = 0; f < m.F; f++) if (m.u[f] < m.nOwn) lev[m.u[f]] = std::max(lev[m.u[f]], lev[m.l[f]] + 1);
    int nLev = 0;
    for (int c = 0; c < m.nOwn; c++) nLev = std::max(nLev, lev[c] + 1);
    return nLev;
}

// Reads the hint (one label per owned cell); leaves every cell's index into the distinct labels in ascending order in gid and
// returns their number: a presence table where the labels span a small range (tile labels do), a sort otherwise.
static int compact_labels(int nOwn, const int *groupHint, std::vector<int> &gid)
{
    std::vector<int> labels;
    int labMin = groupHint[0], labMax = groupHint[0];
    for (int c = 1; c < nOwn; c++) { labMin = std::min(labMin, groupHint[c]); labMax = std::max(labMax, groupHint[c]); }
    if ((long)labMax - labMin < (1L << 24)) {
        std::vector<int> idx((size_t)(labMax - labMin) + 1, 0);
        for (int c = 0; c < nOwn; c++) idx[groupHint[c] - labMin] = 1;
        for (size_t i = 0; i < idx.size(); i++) if (idx[i]) { idx[i] = (int)labels.size(); labels.push_back(labMin + (int)i); } else idx[i] = -1;
        ffm_parallel_for(nOwn, [&](long lo, long hi) { for (long c = lo; c < hi; c++) gid[c] = idx[groupHint[c] - labMin]; });
    } else {
        labels.assign(groupHint, groupHint + nOwn);
        std::sort(labels.begin(), labels.end()); labels.erase(std::unique(labels.begin(), labels.end()), labels.end());
        ffm_parallel_for(nOwn, [&](long lo, long hi) {
            for (long c = lo; c < hi; c++) gid[c] = (int)(std::lower_bound(labels.begin(), labels.end(), groupHint[c]) - labels.begin()); });
    }
    return (int)labels.size();
}

// Reads the addressing and the nl label classes in gid; gives the large connected pieces of a class ids of their own in gid and
// returns the number of ids.
// A label class that an internal wall (a sheet of baffle faces, cases/steckler/system/createBafflesDict) cuts into pieces that
// are not connected inside the class has dependency levels that restart behind the wall: a level then holds cells of two
// planes, is split over several entries, and the neighbours of a cell are no longer in the entries next to its own (the
// ring window of the tiled Amul; the sweeps' LDS ring).  Every connected component of a class becomes a group of its own:
// no new edges, so the group graph stays acyclic; classes in one piece (every tile of a box) are unchanged.
static int split_classes_at_walls(const Addr &m, int nl, std::vector<int> &gid)
{
    const int nOwn = m.nOwn, *l = m.l, *u = m.u;
    int nl2 = nl;
    std::vector<int> parent(nOwn);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    for (int f = 0; f < m.F; f++) if (u[f] < nOwn && gid[l[f]] == gid[u[f]]) { const int a_ = find(l[f]), b_ = find(u[f]); if (a_ != b_) parent[std::max(a_, b_)] = std::min(a_, b_); }
    // components of a class, numbered by their lowest cell; the first LARGE one keeps the class' id, the other large ones get
    // new ids; fragments (a few cells cut off by scattered baffle faces: fewer than 1024 cells or a sixteenth of the class)
    // stay with the class -- a group per fragment would only add tile hand-offs
    std::vector<int> compSize(nOwn, 0), classSize(nl, 0);
    for (int c = 0; c < nOwn; c++) { compSize[find(c)]++; classSize[gid[c]]++; }
    std::vector<int> firstRoot(nl, -1), newId(nOwn, -1);
    for (int c = 0; c < nOwn; c++) {
        const int r = find(c);
        if (newId[r] >= 0) continue;
        const int g = gid[r];
        const bool large = compSize[r] >= std::max(1024, classSize[g] / 16);
        if (!large) newId[r] = g;
        else if (firstRoot[g] < 0) { firstRoot[g] = r; newId[r] = g; }
        else newId[r] = nl2++;
    }
    if (nl2 > nl) {
        if (getenv("FFM_VERBOSE")) fprintf(stderr, "ffm: %d group labels in %d connected pieces (internal walls): one group per piece\n", nl, nl2);
        for (int c = 0; c < nOwn; c++) gid[c] = newId[find(c)];
    }
    return nl2;
}

// Reads the addressing and the nIds label classes in gid; leaves every cell's group in grpOfOld -- the classes ranked in a
// topological order of their dependency graph, ties by label -- and returns their number, or 0 (grpOfOld untouched) if that graph is cyclic.
static int rank_groups(const Addr &m, int nIds, const std::vector<int> &gid, std::vector<int> &grpOfOld)
{
    const int nOwn = m.nOwn, *l = m.l, *u = m.u;
    std::vector<std::pair<int, int>> edges;
    for (int f = 0; f < m.F; f++) if (u[f] < nOwn && gid[l[f]] != gid[u[f]]) edges.emplace_back(gid[l[f]], gid[u[f]]);
    std::sort(edges.begin(), edges.end()); edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    std::vector<int> indeg(nIds, 0), estart(nIds + 1, 0);
    for (auto &e : edges) { indeg[e.second]++; estart[e.first + 1]++; }
    for (int i = 0; i < nIds; i++) estart[i + 1] += estart[i];
    std::vector<int> rank(nIds, -1), heap;
    auto cmp = [](int x, int y) { return x > y; };
    for (int i = 0; i < nIds; i++) if (!indeg[i]) heap.push_back(i);
    std::make_heap(heap.begin(), heap.end(), cmp);
    int done = 0;
    while (!heap.empty()) {
        std::pop_heap(heap.begin(), heap.end(), cmp); const int x = heap.back(); heap.pop_back();
        rank[x] = done++;
        for (int k = estart[x]; k < estart[x + 1]; k++) { const int y = edges[k].second; if (--indeg[y] == 0) { heap.push_back(y); std::push_heap(heap.begin(), heap.end(), cmp); } }
    }
    if (done != nIds) return 0;
    for (int c = 0; c < nOwn; c++) grpOfOld[c] = rank[gid[c]];
    return nIds;
}

// Without a usable hint: leaves contiguous chunks of the caller's cell order in grpOfOld and returns their number.  The caller's order
// is a topological order of the DAG, so cross-group dependencies point from lower to higher groups by construction.
static int chunk_groups(int nOwn, std::vector<int> &grpOfOld)
{
    // at most 512 groups and at least 8192 cells per group
    int B = std::max(8192, (nOwn + 511) / 512);
    if (const char *e = getenv("FFM_PIPE_GROUP_CELLS")) B = std::max(1, atoi(e));     // tests: force many small groups
    for (int c = 0; c < nOwn; c++) grpOfOld[c] = c / B;
    return nOwn ? (nOwn + B - 1) / B : 0;
}

// Reads the groups and the forward levels; leaves a.nGroups, a.grpCell, the cell permutations and a zeroed a.fwdLevelStart.
// New numbering: group-major, then level, then "edge class", then caller index (stable counting passes, least
// significant key first).  Edge class: the cells of a level that have a neighbour in another group come first, grouped
// by the lowest-ranked such group, so that the values a neighbouring tile gathers from this one (Amul, the FV row
// kernels) are runs of consecutive cells instead of one 128-byte line per value (a 16 x 16 column tile: the two
// y-edges of a level were 16 cells with stride 16)
static void order_cells_grouped(const Addr &m, const std::vector<int> &lev, int nLev, const std::vector<int> &grpOfOld, int G, LduAnalysis &a)
{
    const int nOwn = m.nOwn, *l = m.l, *u = m.u;
    a.nGroups = G;
    a.grpCell.assign(G + 1, 0);
    for (int c = 0; c < nOwn; c++) a.grpCell[grpOfOld[c] + 1]++;
    for (int g = 0; g < G; g++) a.grpCell[g + 1] += a.grpCell[g];
    std::vector<int> first(nOwn);
    std::iota(first.begin(), first.end(), 0);
    if (G > 1) {
        std::vector<int> key(nOwn, G), cntK(G + 2, 0);
        for (int f = 0; f < m.F; f++) {
            if (u[f] >= nOwn) continue;
            const int gl = grpOfOld[l[f]], gu = grpOfOld[u[f]];
            if (gl != gu) { key[l[f]] = std::min(key[l[f]], gu); key[u[f]] = std::min(key[u[f]], gl); }
        }
        for (int c = 0; c < nOwn; c++) cntK[key[c] + 1]++;
        for (int i = 0; i <= G; i++) cntK[i + 1] += cntK[i];
        for (int c = 0; c < nOwn; c++) first[cntK[key[c]]++] = c;
    }
    std::vector<int> byLevel(nOwn), cnt(nLev + 1, 0);
    for (int c = 0; c < nOwn; c++) cnt[lev[c] + 1]++;
    for (int i = 0; i < nLev; i++) cnt[i + 1] += cnt[i];
    for (int i = 0; i < nOwn; i++) { const int c = first[i]; byLevel[cnt[lev[c]]++] = c; }
    std::vector<int>().swap(first);
    std::vector<int> pos(a.grpCell.begin(), a.grpCell.end() - (G ? 1 : 0));
    if (!G) pos.clear();
    for (int i = 0; i < nOwn; i++) { const int c = byLevel[i]; const int p = pos[grpOfOld[c]]++; a.newToOldCell[p] = c; a.oldToNewCell[c] = p; }
    a.fwdLevelStart.assign(nLev + 1, 0);
}

// Reads the forward levels; leaves the level-major cell permutations and a.fwdLevelStart.
static void order_cells_by_level(const Addr &m, const std::vector<int> &lev, int nLev, LduAnalysis &a)
{
    std::vector<int> start(nLev + 1, 0);
    for (int c = 0; c < m.nOwn; c++) start[lev[c] + 1]++;
    for (int i = 0; i < nLev; i++) start[i + 1] += start[i];
    a.fwdLevelStart = start;
    std::vector<int> pos(start.begin(), start.end() - (nLev ? 1 : 0));
    if (!nLev) pos.clear();
    for (int c = 0; c < m.nOwn; c++) { int p = pos[lev[c]]++; a.newToOldCell[p] = c; a.oldToNewCell[c] = p; }
}

// The caller insists on its numbering, which is only legal if it is level-major already: leaves identity permutations and a.fwdLevelStart.
static int keep_caller_order(const Addr &m, const std::vector<int> &lev, int nLev, LduAnalysis &a)
{
    std::iota(a.newToOldCell.begin(), a.newToOldCell.end(), 0);
    a.oldToNewCell = a.newToOldCell;
    a.fwdLevelStart.assign(nLev + 1, 0);
    for (int c = 0; c < m.nOwn; c++) a.fwdLevelStart[lev[c] + 1]++;
    for (int i = 0; i < nLev; i++) a.fwdLevelStart[i + 1] += a.fwdLevelStart[i];
    for (int c = 1; c < m.nOwn; c++) if (lev[c] < lev[c - 1]) { ffm_set_error("numbering is not level-major"); return FFM_ERR_ARG; }
    return FFM_OK;
}

// Reads the cell permutations; leaves a.identity and the faces in the new numbering, sorted by owner: a.l, a.u, a.newToOldFace.
static int renumber_faces(const Addr &m, bool sortByNewNeighbour, LduAnalysis &a)
{
    const int N = m.N, F = m.F, *l = m.l, *u = m.u;
    a.identity = true;
    for (int c = 0; c < N; c++) if (a.newToOldCell[c] != c) { a.identity = false; break; }
    a.l.resize(F); a.u.resize(F); a.newToOldFace.resize(F);
    if (a.identity) {
        std::copy(l, l + F, a.l.begin()); std::copy(u, u + F, a.u.begin());
        std::iota(a.newToOldFace.begin(), a.newToOldFace.end(), 0);
        return FFM_OK;
    }
    std::vector<int> cnt(N + 1, 0);
    for (int f = 0; f < F; f++) cnt[a.oldToNewCell[l[f]] + 1]++;
    for (int c = 0; c < N; c++) cnt[c + 1] += cnt[c];
    std::vector<int> pos(cnt.begin(), cnt.end() - 1);
    for (int f = 0; f < F; f++) a.newToOldFace[pos[a.oldToNewCell[l[f]]]++] = f;
    // The counting sort leaves the faces of one owner in the caller's face order.  The device
    // layout keeps that order so every row is accumulated exactly as in the caller's face loop;
    // the public renumbering sorts by the new neighbour (a proper upper-triangular mesh).
    if (sortByNewNeighbour) ffm_parallel_for(N, [&](long lo, long hi) {
        for (long c = lo; c < hi; c++)
            std::sort(a.newToOldFace.begin() + cnt[c], a.newToOldFace.begin() + cnt[c + 1],
                      [&](int f1, int f2) { return a.oldToNewCell[u[f1]] < a.oldToNewCell[u[f2]]; });
    });
    std::atomic<int> flipped(0);
    ffm_parallel_for(F, [&](long lo, long hi) {
        for (long f = lo; f < hi; f++) {
            const int of = a.newToOldFace[f];
            a.l[f] = a.oldToNewCell[l[of]]; a.u[f] = a.oldToNewCell[u[of]];
            if (a.l[f] >= a.u[f]) flipped = 1;
        }
    });
    if (flipped) { ffm_set_error("internal: renumbering flipped a face"); return FFM_ERR_ADDR; }
    return FFM_OK;
}

// Reads a.l, a.u; leaves the backward level of every cell (new numbering) in bl, and a.bwdLevelStart, a.bwdOrder.
static void backward_levels(const Addr &m, LduAnalysis &a, std::vector<int> &bl)
{
    const int nOwn = m.nOwn;
    bl.assign(m.N, 0);
    for (int f = m.F - 1; f >= 0; f--) if (a.u[f] < nOwn) bl[a.l[f]] = std::max(bl[a.l[f]], bl[a.u[f]] + 1);
    int nB = 0;
    for (int c = 0; c < nOwn; c++) nB = std::max(nB, bl[c] + 1);
    a.bwdLevelStart.assign(nB + 1, 0);
    for (int c = 0; c < nOwn; c++) a.bwdLevelStart[bl[c] + 1]++;
    for (int i = 0; i < nB; i++) a.bwdLevelStart[i + 1] += a.bwdLevelStart[i];
    a.bwdOrder.resize(nOwn);
    std::vector<int> pos(a.bwdLevelStart.begin(), a.bwdLevelStart.end() - (nB ? 1 : 0));
    if (!nB) pos.clear();
    for (int c = 0; c < nOwn; c++) a.bwdOrder[pos[bl[c]]++] = c;
}

// Reads the groups, both level sets and the renumbered faces; leaves a.levNew, a.blNew and a.bwdIsReverse, and fails if a
// cross-group face points from a higher to a lower group.
static int check_groups(const Addr &m, const std::vector<int> &lev, const std::vector<int> &bl, LduAnalysis &a)
{
    const int nOwn = m.nOwn, G = a.nGroups;
    a.levNew.resize(nOwn); a.blNew.assign(bl.begin(), bl.begin() + nOwn);
    ffm_parallel_for(nOwn, [&](long lo, long hi) { for (long c = lo; c < hi; c++) a.levNew[c] = lev[a.newToOldCell[c]]; });
    // the group graph must be acyclic in the new numbering: every cross-group face points from a lower to a higher group
    // (new numbering: the group of cell c is the one whose range [grpCell[g], grpCell[g + 1]) holds it)
    std::vector<int> grpOfNew(nOwn);
    ffm_parallel_for(G, [&](long lo, long hi) { for (long g = lo; g < hi; g++) std::fill(grpOfNew.begin() + a.grpCell[g], grpOfNew.begin() + a.grpCell[g + 1], (int)g); });
    std::atomic<int> cyclic(0);
    ffm_parallel_for(m.F, [&](long lo, long hi) {
        for (long f = lo; f < hi; f++) if (a.u[f] < nOwn && grpOfNew[a.l[f]] > grpOfNew[a.u[f]]) cyclic = 1;
    });
    if (cyclic) { ffm_set_error("internal: group graph not acyclic"); return FFM_ERR_ADDR; }
    // the backward order inside each group (by backward level, then descending cell index) is the exact reverse of the forward
    // order when the backward level never falls from one cell of a group to the cell before it
    std::atomic<int> notReverse(0);
    ffm_parallel_for(nOwn, [&](long lo, long hi) {
        for (long c = std::max(lo, 1L); c < hi; c++) if (grpOfNew[c - 1] == grpOfNew[c] && bl[c - 1] < bl[c]) notReverse = 1;
    });
    a.bwdIsReverse = !notReverse;
    return FFM_OK;
}

// The tiled sweeps need at most FFM_TILE_W lower and FFM_TILE_W upper neighbours per owned cell (ghost neighbours not counted) and,
// inside every group, a backward order that is the reverse of the forward order (LduAnalysis::bwdIsReverse).
bool ffm_tile_feasible(int nOwn, int F, const int *l, const int *u)
{
    std::vector<unsigned char> nl(nOwn, 0), nu(nOwn, 0);
    for (int f = 0; f < F; f++) {
        if (u[f] >= nOwn) continue;
        if (++nu[l[f]] > FFM_TILE_W || ++nl[u[f]] > FFM_TILE_W) return false;
    }
    return true;
}

static const char CYCLIC_HINT[] = "the group hint gives a cyclic group graph";
static const char TOO_MANY_NEIGHBOURS[] = "tiled sweeps not applicable (more than 3 lower or upper neighbours)";

// One attempt in the mode that FFM_SWEEP / forceMode and the hint ask for.  In automatic mode an attempt at tiled sweeps may end
// early with the reason in notTileable and a half filled: the hint's group graph is cyclic, or a cell has too many neighbours.
static int analyse_once(const Addr &m, bool renumber, bool sortByNewNeighbour, const int *groupHint, int forceMode, LduAnalysis &a,
                        FfmLapTimer &lap_, const char *&notTileable)
{
    const bool autoMode = (forceMode >= 0 ? forceMode : default_sweep_mode()) == SWEEP_AUTO;
    std::vector<int> autoHint, lev, bl;
    a.mode = pick_mode(m, renumber, forceMode, groupHint, autoHint);
    FFM_TRY(validate_addressing(m));
    lap_.lap("hint + validation");
    const int nLev = forward_levels(m, lev);
    a.newToOldCell.resize(m.N); a.oldToNewCell.resize(m.N);
    if (!renumber || a.mode < 1) a.mode = 0;
    if (a.mode >= 1) {
        // Groups.  With a hint (one label per owned cell, e.g. a 2-D tile of cell columns computed by the host from the cell
        // centres) the groups are the label classes, provided their dependency graph is acyclic.  Without a usable hint: chunks.
        std::vector<int> grpOfOld(m.nOwn, 0);
        int G = 0;
        if (groupHint && m.nOwn > 0) {
            std::vector<int> gid(m.nOwn);
            const int nl = compact_labels(m.nOwn, groupHint, gid);
            const int nIds = split_classes_at_walls(m, nl, gid);
            lap_.lap("labels + components");
            G = rank_groups(m, nIds, gid, grpOfOld);
            if (!G && autoMode) { notTileable = CYCLIC_HINT; return FFM_OK; }
        }
        if (!G) G = chunk_groups(m.nOwn, grpOfOld);
        lap_.lap("group graph");
        order_cells_grouped(m, lev, nLev, grpOfOld, G, a);
        lap_.lap("cell order");
    } else if (renumber) order_cells_by_level(m, lev, nLev, a);
    else FFM_TRY(keep_caller_order(m, lev, nLev, a));
    for (int c = m.nOwn; c < m.N; c++) { a.newToOldCell[c] = c; a.oldToNewCell[c] = c; }
    FFM_TRY(renumber_faces(m, sortByNewNeighbour, a));
    lap_.lap("faces");
    backward_levels(m, a, bl);
    lap_.lap("backward levels");
    if (a.mode >= 1) FFM_TRY(check_groups(m, lev, bl, a));
    lap_.lap("group checks + backward order");
    if (a.mode == 2 && !ffm_tile_feasible(m.nOwn, m.F, a.l.data(), a.u.data())) {
        notTileable = TOO_MANY_NEIGHBOURS;
        return FFM_OK;
    }
    lap_.lap("feasibility");
    return FFM_OK;
}

// The analysis proper.  A mesh / grouping that the tiled sweeps cannot take in automatic mode gets level-scheduled sweeps instead:
// the same analysis once more, without hint, in mode 0.
static int analyse(int N, int nOwn, int F, const int *l, const int *u, bool renumber, bool sortByNewNeighbour, LduAnalysis &a,
                   const int *groupHint = nullptr, int forceMode = -1)
{
    const Addr m{N, nOwn, F, l, u};
    const char *notTileable = nullptr;
    FfmLapTimer lap_("analyse");
    FFM_TRY(analyse_once(m, renumber, sortByNewNeighbour, groupHint, forceMode, a, lap_, notTileable));
    if (!notTileable) return FFM_OK;
    if (getenv("FFM_VERBOSE")) fprintf(stderr, "ffm: %s: level-scheduled sweeps\n", notTileable);
    const bool feasibilityLapOpen = notTileable == TOO_MANY_NEIGHBOURS;      // the first attempt ended inside its last lap
    a = LduAnalysis();
    FfmLapTimer lapLevels_("analyse");
    const char *ignored = nullptr;                                          // (mode 0 has nothing to refuse)
    FFM_TRY(analyse_once(m, renumber, sortByNewNeighbour, nullptr, 0, a, lapLevels_, ignored));
    if (feasibilityLapOpen) lap_.lap("feasibility");                        // ... which then covers the second attempt, as it always did
    return FFM_OK;
}

// ------------------------------------------------------------ entry points ---
// Group hint from cell centres, for hosts that have geometry but no structured indices (an OpenFOAM fvMesh): columns run
// along the axis that consecutive cell labels follow most often (the fastest index of a blockMesh block), the other two
// axes are cut into strips about `tileCells` cells wide (cell spacing estimated from the bounding box and the cell count).
// The result is only a hint: ffm_renumber_hint / ffm_ldu_create_hint check that the label classes form an acyclic group graph
// and fall back to the level-scheduled sweeps otherwise.
extern "C" int ffm_tile_hint_from_centres(int nCells, const double *C /* [3][nCells] */, int tileCells, int *hint)
{
    if (nCells < 0 || (nCells && (!C || !hint))) return FFM_ERR_ARG;
    if (nCells == 0) return FFM_OK;
    if (tileCells <= 0) tileCells = TILE_EDGE;
    double lo[3], hi[3];
    for (int d = 0; d < 3; d++) { lo[d] = hi[d] = C[(size_t)d * nCells]; }
    long votes[3] = {0, 0, 0};
    for (int c = 0; c < nCells; c++) {
        for (int d = 0; d < 3; d++) { const double v = C[(size_t)d * nCells + c]; lo[d] = std::min(lo[d], v); hi[d] = std::max(hi[d], v); }
        if (c + 1 < nCells) {
            double best = -1; int bd = 0;
            for (int d = 0; d < 3; d++) { const double dv = std::fabs(C[(size_t)d * nCells + c + 1] - C[(size_t)d * nCells + c]); if (dv > best) { best = dv; bd = d; } }
            votes[bd]++;
        }
    }
    // the axis that changes between most consecutive labels is the column axis... unless it is the row-wrap axis: take the
    // axis with the most votes (the fastest index changes N - N/nx times, the others far less)
    int col = 0;
    for (int d = 1; d < 3; d++) if (votes[d] > votes[col]) col = d;
    const int a = (col + 1) % 3, b = (col + 2) % 3;
    double L[3];
    for (int d = 0; d < 3; d++) L[d] = std::max(hi[d] - lo[d], 1e-300);
    // cells per axis from N and the aspect ratios (cell centres span L = (n-1) h): n_d ~ (N L_d^2/(L_e L_f))^(1/3)
    auto cellsAlong = [&](int d) { const int e = (d + 1) % 3, f = (d + 2) % 3; return std::max(1.0, std::cbrt((double)nCells * L[d] * L[d] / (L[e] * L[f]))); };
    double ha = L[a] / std::max(cellsAlong(a) - 1.0, 1.0), hb = L[b] / std::max(cellsAlong(b) - 1.0, 1.0);
    // better where the numbering allows it: the smallest step of the coordinate between consecutive cells (a structured block wraps
    // its rows by exactly one spacing).  The estimate above is off by a fraction of a percent (centres span (n-1) h, not n h), enough
    // to put a 17th cell row into a tile: levels of more than 256 cells, split entries, no ring plan for the tiled Amul
    {
        double sa = 1e300, sb = 1e300;
        for (int c = 0; c + 1 < nCells; c++) {
            const double da = std::fabs(C[(size_t)a * nCells + c + 1] - C[(size_t)a * nCells + c]);
            const double db = std::fabs(C[(size_t)b * nCells + c + 1] - C[(size_t)b * nCells + c]);
            if (da > 1e-9 * L[a] && da < sa) sa = da;
            if (db > 1e-9 * L[b] && db < sb) sb = db;
        }
        if (sa < 1e300 && sa >= 0.5 * ha) ha = sa;          // (a step far below the estimate: graded or unstructured, keep the estimate)
        if (sb < 1e300 && sb >= 0.5 * hb) hb = sb;
    }
    for (int c = 0; c < nCells; c++) {
        const int ta = (int)std::floor((C[(size_t)a * nCells + c] - lo[a]) / (tileCells * ha) + 1e-9);
        const int tb = (int)std::floor((C[(size_t)b * nCells + c] - lo[b]) / (tileCells * hb) + 1e-9);
        hint[c] = ffm_tile_label(ta, tb);
    }
    return FFM_OK;
}

extern "C" int ffm_renumber_levels_ext(int nOwned, int nGhost, int nFaces, const int *l, const int *u,
                                       int *newToOldCell, int *newToOldFace)
{ return ffm_renumber_hint(nOwned, nGhost, nFaces, l, u, nullptr, newToOldCell, newToOldFace); }

extern "C" int ffm_renumber_hint(int nOwned, int nGhost, int nFaces, const int *l, const int *u, const int *groupHint,
                                 int *newToOldCell, int *newToOldFace)
{
    if (nOwned < 0 || nGhost < 0 || nFaces < 0 || (nFaces && (!l || !u))) return FFM_ERR_ARG;
    LduAnalysis a;
    FFM_TRY(analyse(nOwned + nGhost, nOwned, nFaces, l, u, true, true, a, groupHint));
    if (newToOldCell) std::copy(a.newToOldCell.begin(), a.newToOldCell.end(), newToOldCell);
    if (newToOldFace) std::copy(a.newToOldFace.begin(), a.newToOldFace.end(), newToOldFace);
    memo_leave_groups(nOwned + nGhost, nFaces, a);
    memo_leave_analysis(nOwned, nGhost, nFaces, groupHint, a);
    return FFM_OK;
}

extern "C" int ffm_renumber_levels(int nCells, int nFaces, const int *l, const int *u,
                                   int *newToOldCell, int *newToOldFace)
{
    if (nCells < 0 || nFaces < 0 || (nFaces && (!l || !u))) return FFM_ERR_ARG;
    LduAnalysis a;
    FFM_TRY(analyse(nCells, nCells, nFaces, l, u, true, true, a));
    if (newToOldCell) std::copy(a.newToOldCell.begin(), a.newToOldCell.end(), newToOldCell);
    if (newToOldFace) std::copy(a.newToOldFace.begin(), a.newToOldFace.end(), newToOldFace);
    memo_leave_groups(nCells, nFaces, a);
    return FFM_OK;
}

int ffm_ldu_analysis(int nOwn, int nGhost, int F, const int *l, const int *u, const int *groupHint, int forceMode, LduAnalysis &a)
{
    const int N = nOwn + nGhost;
    if (forceMode < 0 && nGhost == 0 && memo_take_analysis(N, nOwn, F, l, u, groupHint, a)) return FFM_OK;
    return analyse(N, nOwn, F, l, u, true, false, a, groupHint, forceMode);
}

// ------------------------------------------------------------------ layout ---
// Reads a.l, a.u; leaves the widest upper and lower row of every slice of 64 owned cells in wu, wl.
static void slice_widths(const LduAnalysis &a, int nOwn, int N, int F, int nSl, std::vector<int> &wu, std::vector<int> &wl)
{
    std::vector<int> upCnt(N, 0), loCnt(N, 0);
    for (int f = 0; f < F; f++) { upCnt[a.l[f]]++; if (a.u[f] < nOwn) loCnt[a.u[f]]++; }
    wu.assign(nSl, 0); wl.assign(nSl, 0);
    for (int sl = 0; sl < nSl; sl++)
        for (int c = sl * 64; c < std::min(nOwn, sl * 64 + 64); c++) { wu[sl] = std::max(wu[sl], upCnt[c]); wl[sl] = std::max(wl[sl], loCnt[c]); }
}

// What the sliced layout cannot hold, and the width of the slot field of the packed lower entries (loShift).  At most 32 upper and 32
// lower faces per cell (the widest instantiation of the row kernels).  The packed entries are int32: a lower entry packs
// owner << loShift | slot.  Four bits hold the slot of every face that an owned cell reads through a lower entry unless some cell owns
// more than 16 faces towards OWNED cells (coarse GAMG levels of polyhedral and unstructured meshes): such a matrix takes five bits, and
// only such a matrix is limited to 2^26 cells instead of 2^27.  The faces towards ghost cells, which follow the owned ones in a
// decomposed matrix and have no lower entry, never count: they may use the slots above 16 of a four-bit matrix.
static int check_layout_limits(const LduAnalysis &a, int nOwn, int N, int F, const std::vector<int> &wu, const std::vector<int> &wl, int &loShift)
{
    const int nSl = (int)wu.size();
    int widest = 0;
    loShift = 4;
    for (int sl = 0; sl < nSl; sl++) {
        if (wu[sl] > 32 || wl[sl] > 32) { ffm_set_error("a cell has %d upper / %d lower faces (> 32): not supported by the sliced layout", wu[sl], wl[sl]); return FFM_ERR_UNSUPPORTED; }
        widest = std::max(widest, wu[sl]);
    }
    if ((long)nSl * 32 * 64 > 0x7fffffffL || N >= (1 << 27)) { ffm_set_error("mesh too large for int32 packed entries"); return FFM_ERR_UNSUPPORTED; }
    if (widest <= 16) return FFM_OK;                 // every slot is below 16
    int prev = -1, slot = 0;
    for (int f = 0; f < F; f++) {
        slot = (a.l[f] == prev) ? slot + 1 : 0; prev = a.l[f];
        if (slot >= 16 && a.u[f] < nOwn) { loShift = 5; break; }
    }
    if (loShift == 5 && N >= (1 << 26)) {
        ffm_set_error("mesh too large for int32 packed entries: a cell owns more than 16 faces towards owned cells, which limits the matrix to 2^26 cells");
        return FFM_ERR_UNSUPPORTED;
    }
    return FFM_OK;
}

// Reads the slice widths; leaves nSlices, the slice offsets and totals, the uniform widths and maxW.
static void slice_offsets(const std::vector<int> &wu, const std::vector<int> &wl, LduLayout &L)
{
    const int nSl = L.nSlices = (int)wu.size();
    L.upOff.assign(nSl + 1, 0); L.loOff.assign(nSl + 1, 0);
    int uniform = -2, uniformLo = -2;
    L.maxW = 0;
    for (int sl = 0; sl < nSl; sl++) {
        L.upOff[sl + 1] = L.upOff[sl] + wu[sl] * 64; L.loOff[sl + 1] = L.loOff[sl] + wl[sl] * 64;
        uniform = (uniform == -2) ? wu[sl] : (uniform == wu[sl] ? wu[sl] : -1);
        uniformLo = (uniformLo == -2) ? wl[sl] : (uniformLo == wl[sl] ? wl[sl] : -1);
        L.maxW = std::max(L.maxW, std::max(wu[sl], wl[sl]));
    }
    L.upTotal = L.upOff[nSl]; L.loTotal = L.loOff[nSl];
    L.upWidthUniform = (uniform >= 0) ? uniform : -1;
    L.loWidthUniform = (uniformLo >= 0) ? uniformLo : -1;
}

// Reads a.l, a.u, a.newToOldFace and the slice offsets; leaves upNbr, faceSrc, loEnt and callerToNative.
static void fill_entries(const LduAnalysis &a, int nOwn, int N, int F, LduLayout &L)
{
    L.upNbr.assign(std::max(L.upTotal, 1), -1); L.faceSrc.assign(std::max(L.upTotal, 1), -1); L.loEnt.assign(std::max(L.loTotal, 1), -1);
    L.callerToNative.assign(F, -1);
    // upper slots: faces of one owner are consecutive in a.l (owner-sorted), caller order inside (check_layout_limits walks the slots
    // the same way to choose the width of the slot field of the packed lower entries: change the slot order in both)
    std::vector<int> slotOfFace(F);
    int prev = -1, slot = 0;
    for (int f = 0; f < F; f++) {
        const int c = a.l[f];
        slot = (c == prev) ? slot + 1 : 0; prev = c;
        slotOfFace[f] = slot;
        const int e = L.upOff[c >> 6] + slot * 64 + (c & 63);
        L.upNbr[e] = a.u[f]; L.faceSrc[e] = a.newToOldFace[f];
        L.callerToNative[a.newToOldFace[f]] = e;
    }
    // lower entries in the CALLER's face order (losort of the caller's addressing)
    std::vector<int> oldToNewFace(F);
    for (int f = 0; f < F; f++) oldToNewFace[a.newToOldFace[f]] = f;
    std::vector<int> fill(N, 0);
    for (int of = 0; of < F; of++) {
        const int f = oldToNewFace[of], c = a.u[f];
        if (c >= nOwn) continue;                      // ghost cells have no rows
        const int q = L.loOff[c >> 6] + fill[c]++ * 64 + (c & 63);
        L.loEnt[q] = (a.l[f] << L.loShift) | slotOfFace[f];
    }
}

// Reads a.mode and a.fwdLevelStart; leaves the XCD-aware schedule of the row kernels (struct ffm_ldu): chunks of 256 rows, binned by the
// eighth of their dependency level.
static void row_schedule(const LduAnalysis &a, int nOwn, LduLayout &L)
{
    const int nChunks = (nOwn + 255) / 256, nLevels = std::max((int)a.fwdLevelStart.size() - 1, 0);
    std::vector<std::vector<int>> seq(8);
    if (a.mode == 0 && nLevels > 0) {
        int lv = 0;
        for (int ch = 0; ch < nChunks; ch++) {
            const int c0 = ch * 256;
            while (lv + 1 < nLevels && a.fwdLevelStart[lv + 1] <= c0) lv++;
            const long ls = a.fwdLevelStart[lv], le = a.fwdLevelStart[lv + 1];
            int eighth = (le > ls) ? (int)(8L * (c0 - ls) / (le - ls)) : 0;
            seq[std::min(std::max(eighth, 0), 7)].push_back(ch);
        }
    } else {
        // group-major numbering (tiles): each XCD streams through one contiguous eighth of the rows, so that the rows a
        // row gathers from (same or neighbouring tile) were fetched into the same L2
        for (int ch = 0; ch < nChunks; ch++) seq[std::min(7, (int)(8L * ch / std::max(nChunks, 1)))].push_back(ch);
    }
    size_t mx = 0;
    for (auto &q : seq) mx = std::max(mx, q.size());
    L.rowSched.assign(mx * 8, -1);
    for (int x = 0; x < 8; x++) for (size_t k = 0; k < seq[x].size(); k++) L.rowSched[k * 8 + x] = seq[x][k];
}

// The sliced owner-ELL of the analysed matrix: rows exist for owned cells only, in slices of 64 (one wavefront).
int ffm_ldu_layout(const LduAnalysis &a, int nOwn, int nGhost, int F, LduLayout &L)
{
    const int N = nOwn + nGhost, nSl = (nOwn + 63) / 64;
    std::vector<int> wu, wl;
    slice_widths(a, nOwn, N, F, nSl, wu, wl);
    FFM_TRY(check_layout_limits(a, nOwn, N, F, wu, wl, L.loShift));
    slice_offsets(wu, wl, L);
    fill_entries(a, nOwn, N, F, L);
    row_schedule(a, nOwn, L);
    return FFM_OK;
}

// Would ffm_ldu_create* accept this addressing?  The analysis and the layout of ffm_ldu_create_ext on the host, without a device or a
// context; the refusal's message is left in ffm_last_error.  (The size that no int32 entry can hold is refused before the analysis
// allocates its per-cell arrays.)
extern "C" int ffm_ldu_check_layout(int nOwned, int nGhost, int nFaces, const int *l, const int *u)
{
    if (nOwned < 0 || nGhost < 0 || nFaces < 0 || (nFaces && (!l || !u))) { ffm_set_error("ffm_ldu_check_layout: bad argument"); return FFM_ERR_ARG; }
    if ((long)nOwned + nGhost >= (1L << 27)) { ffm_set_error("mesh too large for int32 packed entries"); return FFM_ERR_UNSUPPORTED; }
    LduAnalysis a;
    FFM_TRY(analyse(nOwned + nGhost, nOwned, nFaces, l, u, true, false, a, nullptr, -1));
    LduLayout L;
    return ffm_ldu_layout(a, nOwned, nGhost, nFaces, L);
}
