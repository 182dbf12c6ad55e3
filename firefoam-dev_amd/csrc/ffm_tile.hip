// ffm_tile.hip -- tiled wavefront sweeps for DIC / DILU (calcReciprocalD, forward and backward substitution): one kernel template,
// k_tile<MODE, NF, R, FUSE>, for one system or NF systems with common off-diagonal coefficients; Gauss-Seidel row sweeps: k_tile_gs.
//
// Same operators, bitwise, as the level-scheduled kernels of ffm_solve.hip (OpenFOAM-dev DICPreconditioner /
// DILUPreconditioner::calcReciprocalD and ::precondition, reference selection cases/steckler/system/fvSolution:21-46).
// Motivation and measurements (MI355X, 400^3 box = 1198 dependency levels): a hand-off between workgroups costs about as
// much as a dependent kernel launch (3-5 us under load), so neither one launch per level nor a persistent kernel that
// publishes a progress word per level (tried in round 1, removed) gets under ~3.6 us per level.  Here
//   * cells are split into groups (2-D tiles of cell columns: a host hint or a detected blockMesh box) whose dependency
//     graph is acyclic; cells are numbered group-major and level-major inside a group; one workgroup sweeps one group,
//     one "entry" (<= 256 cells of one level) per step;
//   * inside a group the values of earlier levels are exchanged through an LDS ring: one workgroup barrier per level;
//   * a value another group needs (tile faces, ~12 % of the cells) is also stored to a "mailbox" slot with one 8-byte
//     agent-scope store.  Mailboxes are filled with a signalling-NaN sentinel before every sweep, and a sweep never
//     produces that bit pattern, so the value is its own ready flag: the consumer loads the slot with an agent-scope
//     load and re-loads it while it still reads the sentinel (cdna_hip_programming.md G16 form R2, "the data IS the
//     flag": one aligned 8-byte granule, no fence, no flag, no drain).  No progress words, no per-batch synchronisation;
//   * everything an entry needs from memory lives in streams private to this kernel whose addresses depend on the cell
//     index only (16-bit neighbour codes, coefficients gathered once per coefficient update) and is fetched T_PF entries
//     ahead into registers; entry records 2*T_PF ahead; mailbox values T_PM ahead.  The consumer therefore trails its
//     producers by a few levels and normally finds its values ready; the per-level critical path is LDS reads, a few
//     FMAs, one LDS write and one barrier;
//   * groups are handed out by an atomic ticket in topological order, so a workgroup only waits for groups that are
//     already running or finished (no residency assumption, no deadlock); every spin is bounded and raises the abort word
//     that ffm_sweep_check_abort() reports when the solve ends.
#include "ffm_internal.hpp"
#include "ffm_device.hpp"
#include <algorithm>
#include <atomic>
#include <climits>

constexpr int T_RING = 4096;        // doubles (power of two)
constexpr int T_ENT = 256;          // max cells per entry = workgroup size
constexpr int T_THREADS = 256;
constexpr int T_W = FFM_TILE_W;     // neighbour slots per cell and direction (ffm_host.hpp: ffm_tile_feasible tests it on the host)
constexpr int T_PF = 8;             // entries fetched ahead of the one being computed, at most (tile_pf)
constexpr int T_PM = 3;             // mailbox values are loaded this many entries ahead (2 <= T_PM < T_PF)
constexpr int T_XMAX = 64;          // max external references per entry (one lane of the mail wave each; power of two)
constexpr int T_RINGD = T_RING - 2 * T_ENT;     // largest cell distance served by the ring
constexpr unsigned T_SPIN_LIMIT = 1u << 22;
constexpr unsigned T_NONE = 0xFFFFu;               // absent neighbour / cell that publishes nothing
constexpr int T_LDS = T_RING + 2 * T_XMAX + 1;      // ring, two external buffers (entry parity), one dummy slot read by absent neighbours
constexpr unsigned long long T_SENT = 0x7FF4DEADBEEFCAFEull;    // signalling NaN: no arithmetic result has these bits
static_assert(T_LDS < (int)T_NONE && T_ENT <= 256, "neighbour codes are LDS slots");
static_assert(T_PM >= 2 && T_PM < T_PF, "read-ahead distances");

struct TileDir {            // one sweep direction (device arrays)
    int nEnt = 0, nPub = 0;
    int *grpEnt = nullptr;      // [G+1] entries of each group
    int4 *rec = nullptr;        // [nEnt + pad] {first cell, cells | externals << 16, first mailbox slot, byte offset of the entry's code block in `code`}
    int *extOff = nullptr;      // [nEnt + pad] first extSrc index of every entry (read by the mail wave only)
    int *extSrc = nullptr;      // mailbox slot of every external reference, entry by entry
    unsigned short *code = nullptr;   // pool of code blocks, one block = the cells of an entry in ascending order, 4 shorts per cell: 3 neighbour codes = the LDS
                                      // slot holding the neighbour's value when the cell is computed (ring slot (nb - group start) mod T_RING, or T_RING +
                                      // parity(entry)*T_XMAX + external index; T_NONE: no neighbour), publish slot | T_NONE.  No code depends on the cell's
                                      // absolute position, so entries with equal blocks share one (ffm_tile_share.cpp; FFM_TILE_CODE_SHARE=0: one block each; 1 / 2: only the sweeps' / the Amul's pool shared)
    long codeUnique = 0, codeTotal = 0;     // bytes of the pool's blocks / of all entries' blocks (host)
    int *src = nullptr;         // [3*nOwn] native coefficient index of each neighbour slot (-1: none)
    double *coefU = nullptr, *coefL = nullptr;        // [3*nOwn] gathered upper / lower coefficients (lazily allocated)
    unsigned long epochU = ~0ul, epochL = ~0ul;
    int reach = 0;              // largest cell distance of a neighbour served by the ring (host; <= T_RINGD)
    double *mail = nullptr;     // [nPub + 1] (inside ffm_tile_plan::mailAll)
};

struct ffm_tile_plan {
    bool usable = false;
    int G = 0;
    TileDir f, b;
    double *mailAll = nullptr;
    long nMail = 0;
    double *mailMulti = nullptr;    // [FFM_TILE_MAXSYS][nMail]: the mailboxes of the sweeps of several systems, allocated on first use
    // ---- tiled Amul (symmetric matrices): same groups and entries as the forward sweep
    bool amulUsable = false;
    bool gsTables = false;          // the upper-neighbour and tail tables below exist (Gauss-Seidel sweeps, Amul tail)
    std::vector<int> grpEntHost;    // forward entries of each group (host copy)
    int4 *arec = nullptr;           // [nEnt + pad] {first cell, cells | externals << 16, first index into aext, byte offset of the entry's code block in acode}
    uint4 *acode = nullptr;         // pool of code blocks (shared between equal entries as TileDir::code), per cell 8 x 16 bit: 3 lower codes, 3 upper codes
                                    // (A_* encoding below), 2 spare
    long acodeUnique = 0, acodeTotal = 0;
    int2 *aext = nullptr;           // per external reference {cell whose x is needed, native index of the coefficient or -1}
    // owned upper neighbours of every cell: the neighbour cell of slot k (the upper coefficients are the backward direction's)
    int *upNbrCell = nullptr;
    int nSeg = 0;                   // workgroups of the tiled Amul: a segment = a run of entries of one group
    int4 *aseg = nullptr;           // [nSeg] {group, first entry, end entry, end entry of the group}
    double *amulPartials = nullptr; // [nSeg]
    int4 *fvSeg = nullptr; int nFvSeg = 0, fvRun = 0;      // segments of the FV face passes (ffm_tile_fv_segments)
    int nTail = 0;                  // cells that own faces towards ghost cells (processed after the tiled kernel, in face order)
    int *tailCell = nullptr, *tailStart = nullptr, *tailFace = nullptr, *tailNbr = nullptr;
};

// ---- FV face passes on the tile numbering (ffm_fused.hip: k_mv_tile): runs of forward entries of one group, one workgroup each
// {first entry of the group, first entry of the run, end entry of the run, end entry of the group}; entry records = the forward plan's
bool ffm_tile_fv_segments(ffm_ldu *A, int runLength, FfmFvSegs *out)
{
    ffm_tile_plan *T = A->tile;
    if (!T || !T->usable || T->grpEntHost.empty() || A->nCells != A->nOwned) return false;
    if (!T->fvSeg || T->fvRun != runLength) {
        std::vector<int4> seg;
        const std::vector<int> &ge = T->grpEntHost;
        for (int g = 0; g < T->G; g++) for (int a = ge[g]; a < ge[g + 1]; a += runLength) seg.push_back(make_int4(ge[g], a, std::min(a + runLength, ge[g + 1]), ge[g + 1]));
        if (T->fvSeg) { hipFree(T->fvSeg); T->fvSeg = nullptr; }
        if (ffm_upload_vec(A->ctx, &T->fvSeg, seg) != FFM_OK) return false;
        T->nFvSeg = (int)seg.size(); T->fvRun = runLength;
    }
    out->nSeg = T->nFvSeg; out->seg = T->fvSeg; out->rec = T->f.rec;
    return true;
}

static void free_dir(TileDir &d)
{
    hipFree(d.grpEnt); hipFree(d.rec); hipFree(d.extOff); hipFree(d.extSrc); hipFree(d.code); hipFree(d.src); hipFree(d.coefU); hipFree(d.coefL);
    d = TileDir();
}
void ffm_tile_free(ffm_ldu *A)
{
    if (!A->tile) return;
    free_dir(A->tile->f); free_dir(A->tile->b);
    hipFree(A->tile->mailAll); hipFree(A->tile->mailMulti);
    hipFree(A->tile->arec); hipFree(A->tile->acode); hipFree(A->tile->aext); hipFree(A->tile->aseg); hipFree(A->tile->amulPartials);
    hipFree(A->tile->fvSeg); hipFree(A->tile->upNbrCell);
    hipFree(A->tile->tailCell); hipFree(A->tile->tailStart); hipFree(A->tile->tailFace); hipFree(A->tile->tailNbr);
    delete A->tile; A->tile = nullptr;
}
bool ffm_tile_usable(const ffm_ldu *A) { return A->tile && A->tile->usable; }

template <class T> static int upv(ffm_ctx *c, T **d, const std::vector<T> &v) { return ffm_upload_vec(c, d, v); }

// The per-cell codes (S shorts per cell) cut into the blocks of the entries `rec` and kept once per distinct content: rec[e].w becomes the
// byte offset of entry e's block in `pool` (its former value goes to wOut).  The pool ends in one entry's worth of padding, so that a
// record of the read-ahead padding (offset 0, no cells) and the idle lanes, which read position 0 of their entry, always have a block.
static int share_blocks(std::vector<unsigned short> &code, std::vector<int4> &rec, int S, const char *what, std::vector<unsigned short> &pool,
                        long *uniqueBytes, long *totalBytes, std::vector<int> *wOut)
{
    std::vector<long> start(rec.size());
    std::vector<int> len(rec.size());
    for (size_t e = 0; e < rec.size(); e++) { start[e] = (long)S * rec[e].x; len[e] = S * (rec[e].y & 0xFFFF); }
    std::vector<unsigned> off;
    FFM_TRY(ffm_tile_share(code, start, len, ffm_tile_share_enabled(S == 4 ? 1 : 2), (long)S * T_ENT, pool, off, uniqueBytes, totalBytes, what));
    for (size_t e = 0; e < rec.size(); e++) { if (wOut) (*wOut)[e] = rec[e].w; rec[e].w = (int)off[e]; }
    return FFM_OK;
}

// Build one direction.  fwd: neighbours = lower entries (cells with smaller index); bwd: upper slots.  Neighbours that are
// ghost cells are dropped (block-Jacobi sweeps ignore them); the remaining ones keep their order, which is the order of
// the reference's face loop.
static int build_dir(ffm_ldu *A, bool fwd, const std::vector<int> &lvl, const std::vector<int> &grpCell,
                     const std::vector<int> &grpOfCell, TileDir &D, bool &ok, std::vector<int4> *recOut = nullptr,
                     std::vector<int> *grpEntOut = nullptr)
{
    const int G = (int)grpCell.size() - 1, nOwn = A->nOwned, W = T_W, sh = A->loShift;
    const std::vector<int> &off = fwd ? A->h_loOff : A->h_upOff;
    const std::vector<int> &ent = fwd ? A->h_loEnt : A->h_upNbr;
    std::vector<int> nbr((size_t)W * nOwn, -1), src((size_t)W * nOwn, -1);
    std::vector<unsigned char> exposed(nOwn, 0);
    auto isExt = [&](int c, int nb) { return grpOfCell[nb] != grpOfCell[c] || std::abs(c - nb) > T_RINGD; };
    std::atomic<int> tooMany(0), reach(0);
    ffm_parallel_for(nOwn, [&](long c0_, long c1_) {
        int far = 0;
        for (long c = c0_; c < c1_; c++) {
            const int sl = (int)(c >> 6), lane = (int)(c & 63), wdt = (off[sl + 1] - off[sl]) / 64;
            int k = 0;
            for (int s = 0; s < wdt; s++) {
                const int q = off[sl] + s * 64 + lane, e = ent[q];
                if (e < 0) continue;
                const int nb = fwd ? (e >> sh) : e;
                if (nb >= nOwn) continue;
                if (k >= W) { tooMany = 1; break; }
                nbr[(size_t)W * c + k] = nb;
                src[(size_t)W * c + k] = fwd ? (A->h_upOff[nb >> 6] + (e & ((1 << sh) - 1)) * 64 + (nb & 63)) : q;
                if (isExt((int)c, nb)) exposed[nb] = 1;          // (several threads may store the same 1)
                else far = std::max(far, std::abs((int)c - nb));
                k++;
            }
        }
        int seen = reach.load();
        while (far > seen && !reach.compare_exchange_weak(seen, far)) {}
    });
    D.reach = reach;
    if (tooMany) { ok = false; return FFM_OK; }
    // entries: runs of one level, at most T_ENT cells and T_XMAX external references; forward ascending, backward descending
    std::vector<unsigned short> code((size_t)4 * nOwn, (unsigned short)T_NONE);
    std::vector<int> grpEnt(G + 1, 0), mailIdx(nOwn, -1);
    std::vector<int4> rec;
    int nPub = 0;
    auto extRefs = [&](int c) { int n = 0; for (int k = 0; k < W; k++) { const int nb = nbr[(size_t)W * c + k]; if (nb >= 0 && isExt(c, nb)) n++; } return n; };
    for (int g = 0; g < G; g++) {
        const int gs = grpCell[g], ge = grpCell[g + 1];
        int prevLevel = -1;
        auto close = [&](int c0, int c1, int nExt) {          // cells [c0,c1)
            if (lvl[c0] < prevLevel) ok = false;               // processing order must not go back in level
            prevLevel = lvl[c0];
            int slot = 0;
            for (int c = c0; c < c1; c++) if (exposed[c]) { code[(size_t)4 * c + 3] = (unsigned short)slot; mailIdx[c] = nPub + slot; slot++; }
            rec.push_back(make_int4(c0, (c1 - c0) | (nExt << 16), nPub, 0));
            nPub += slot;
        };
        if (fwd) {
            for (int c = gs; c < ge;) {
                int e = c, nx = 0;
                while (e < ge && lvl[e] == lvl[c] && e - c < T_ENT) { const int x = extRefs(e); if (e > c && nx + x > T_XMAX) break; nx += x; e++; }
                close(c, e, nx); c = e;
            }
        } else {
            for (int c = ge; c > gs;) {
                int e = c, nx = 0;
                while (e > gs && lvl[e - 1] == lvl[c - 1] && c - e < T_ENT) { const int x = extRefs(e - 1); if (e < c && nx + x > T_XMAX) break; nx += x; e--; }
                close(e, c, nx); c = e;
            }
        }
        if (!ok) return FFM_OK;
        grpEnt[g + 1] = (int)rec.size();
    }
    // neighbour codes and the external lists (mailbox slots are known for every group now)
    // (the entries' external lists start at the running sum of their external counts: the entries are independent of each other)
    size_t nExtAll = 0;
    for (int4 &R : rec) { R.w = (int)nExtAll; nExtAll += (size_t)(R.y >> 16); }
    std::vector<int> extSrc(nExtAll);
    std::atomic<int> bad(0);
    ffm_parallel_for((long)rec.size(), [&](long e0_, long e1_) {
        for (long ei = e0_; ei < e1_; ei++) {
            const int4 &R = rec[ei];
            const int c0 = R.x, cnt = R.y & 0xFFFF;
            const int gs = cnt ? grpCell[grpOfCell[c0]] : 0;
            int t = 0;
            for (int c = c0; c < c0 + cnt; c++) for (int k = 0; k < W; k++) {
                const int nb = nbr[(size_t)W * c + k];
                if (nb < 0) continue;
                if (isExt(c, nb)) {
                    if (mailIdx[nb] < 0 || t >= (R.y >> 16)) { bad = mailIdx[nb] < 0 ? 1 : 2; continue; }
                    code[(size_t)4 * c + k] = (unsigned short)(T_RING + (int)(ei & 1) * T_XMAX + t); extSrc[(size_t)R.w + t] = mailIdx[nb]; t++;
                } else code[(size_t)4 * c + k] = (unsigned short)((nb - gs) & (T_RING - 1));
            }
            if (t != (R.y >> 16)) bad = 2;
        }
    }, nOwn >= (1 << 20) ? 1024 : (1L << 40));
    if (bad == 1) { ffm_set_error("internal: tile plan references an unpublished cell"); return FFM_ERR_ADDR; }
    if (bad) { ffm_set_error("internal: tile plan external count mismatch"); return FFM_ERR_ADDR; }
    D.nEnt = (int)rec.size(); D.nPub = nPub;
    // the code blocks of the entries go to the pool; the record keeps the block's offset where it kept the first extSrc index
    std::vector<int> extOff(rec.size());
    std::vector<unsigned short> pool;
    FFM_TRY(share_blocks(code, rec, 4, fwd ? "tile: forward code sharing" : "tile: backward code sharing", pool, &D.codeUnique, &D.codeTotal, &extOff));
    if (recOut) *recOut = rec;
    if (grpEntOut) *grpEntOut = grpEnt;
    for (int k = 0; k < 2 * T_PF + 2; k++) { rec.push_back(make_int4(0, 0, 0, 0)); extOff.push_back(0); }      // read-ahead padding
    for (int k = 0; k < T_THREADS; k++) extSrc.push_back(0);
    FFM_TRY(upv(A->ctx, &D.grpEnt, grpEnt)); FFM_TRY(upv(A->ctx, &D.rec, rec)); FFM_TRY(upv(A->ctx, &D.extOff, extOff)); FFM_TRY(upv(A->ctx, &D.extSrc, extSrc));
    FFM_TRY(upv(A->ctx, &D.code, pool)); FFM_TRY(upv(A->ctx, &D.src, src));
    return FFM_OK;
}

// ------------------------------------------------------------------ tiled Amul: plan ---
// y = A x for a symmetric matrix on the tile numbering.  One workgroup streams through one group entry by entry (the
// forward sweep's entries); x and the upper coefficients of the entries [e-3, e+3] live in LDS rings, so a row finds its
// neighbours' x and, for its lower faces, the owner's coefficient there: every coefficient, x, diag is read from memory
// once (56 B per cell; the 16 B of codes come from the pool of entry blocks).  Neighbours outside the window or in another group ("externals", tile faces) are
// fetched by the mail wave from x / the native coefficient array.  Faces towards ghost cells come last in a row's face
// order and are added afterwards by k_amul_tail, so the sum of every row runs in the reference's face order.
constexpr int A_RING = 1024;            // cells in the x / coefficient rings (power of two; >= 8 entries of 256)
constexpr int A_WIN = 1;                // entries on either side served by the rings
constexpr int A_AHEAD = A_WIN + 1;      // the rings are filled this many entries ahead of the entry being computed
constexpr int A_XMAX = 128;             // externals per entry (two per lane of the mail wave)
constexpr int A_PF = 6;                 // read-ahead (entries), > A_AHEAD
constexpr unsigned A_NONE = 0xFFFFu, A_EXT = 0x8000u;      // in-ring code: bits 0-10 cell distance, bits 12-13 owner's slot
static_assert((A_WIN + A_AHEAD + 1) * T_ENT <= A_RING && A_PF > A_AHEAD, "ring window");

static int build_amul(ffm_ldu *A, const std::vector<int> &grpOfCell, const std::vector<int4> &recF)
{
    ffm_tile_plan *T = A->tile;
    const int nOwn = A->nOwned, nEnt = (int)recF.size();
    // ---- tables of the owned upper neighbours + the faces towards ghost cells (Gauss-Seidel sweeps, Amul tail):
    // structural requirements only (<= 3 owned upper neighbours, ghost neighbours after the owned ones in slot order)
    std::vector<int> tailCell, tailStart(1, 0), tailFace, tailNbr;
    std::vector<int> upNb((size_t)3 * nOwn, -1);
    for (int c = 0; c < nOwn; c++) {
        const int sl = c >> 6, lane = c & 63;
        const int uw = (A->h_upOff[sl + 1] - A->h_upOff[sl]) / 64;
        int k = 0;
        bool ghostSeen = false;
        for (int s = 0; s < uw; s++) {
            const int idx = A->h_upOff[sl] + s * 64 + lane, nb = A->h_upNbr[idx];
            if (nb < 0) continue;
            if (nb >= nOwn) {
                if (!ghostSeen) { tailCell.push_back(c); ghostSeen = true; }
                tailFace.push_back(idx); tailNbr.push_back(nb);
                continue;
            }
            if (ghostSeen || k >= 3) return FFM_OK;                      // owned after ghost, or too many: no tables
            upNb[(size_t)3 * c + k] = nb;
            k++;
        }
        if (ghostSeen) tailStart.push_back((int)tailFace.size());
    }
    FFM_TRY(upv(A->ctx, &T->upNbrCell, upNb));
    T->nTail = (int)tailCell.size();
    FFM_TRY(upv(A->ctx, &T->tailCell, tailCell)); FFM_TRY(upv(A->ctx, &T->tailStart, tailStart)); FFM_TRY(upv(A->ctx, &T->tailFace, tailFace)); FFM_TRY(upv(A->ctx, &T->tailNbr, tailNbr));
    T->gsTables = true;
#define AMUL_GIVE_UP(why) do { if (getenv("FFM_VERBOSE")) fprintf(stderr, "ffm: no ring plan for the tiled Amul (%s, entry %d of %d): row kernel\n", why, e, nEnt); return FFM_OK; } while (0)
    // ---- ring plan of the tiled Amul: may give up (too many out-of-window neighbours in one entry), Amul then runs on the row kernel
    std::vector<int> entOf(nOwn, -1);
    for (int e = 0; e < nEnt; e++) for (int c = recF[e].x; c < recF[e].x + (recF[e].y & 0xFFFF); c++) entOf[c] = e;
    std::vector<unsigned short> code((size_t)8 * nOwn, (unsigned short)A_NONE);
    std::vector<int4> arec(nEnt);
    std::vector<int2> aext;
    auto inRing = [&](int c, int nb) { return grpOfCell[nb] == grpOfCell[c] && std::abs(entOf[nb] - entOf[c]) <= A_WIN; };
    for (int e = 0; e < nEnt; e++) {
        const int c0 = recF[e].x, cnt = recF[e].y & 0xFFFF;
        const int extOff = (int)aext.size();
        int t = 0;
        for (int c = c0; c < c0 + cnt; c++) {
            const int sl = c >> 6, lane = c & 63;
            // lower entries in face order
            const int lw = (A->h_loOff[sl + 1] - A->h_loOff[sl]) / 64;
            int k = 0;
            for (int s = 0; s < lw; s++) {
                const int q = A->h_loEnt[A->h_loOff[sl] + s * 64 + lane];
                if (q < 0) continue;
                const int o = q >> A->loShift, os = q & ((1 << A->loShift) - 1);
                if (k >= 3) { AMUL_GIVE_UP("more than 3 lower neighbours"); }
                if (inRing(c, o) && os < 3 && c - o < 2048) code[(size_t)8 * c + k] = (unsigned short)((c - o) | (os << 12));
                else {
                    if (t >= A_XMAX) { AMUL_GIVE_UP("more than A_XMAX externals in one entry"); }
                    code[(size_t)8 * c + k] = (unsigned short)(A_EXT | t);
                    aext.push_back(make_int2(o, A->h_upOff[o >> 6] + os * 64 + (o & 63))); t++;
                }
                k++;
            }
            // owned upper neighbours in slot order (tables above)
            for (k = 0; k < 3; k++) {
                const int nb = upNb[(size_t)3 * c + k];
                if (nb < 0) break;
                if (inRing(c, nb) && nb - c < 2048) code[(size_t)8 * c + 3 + k] = (unsigned short)(nb - c);
                else {
                    if (t >= A_XMAX) { AMUL_GIVE_UP("more than A_XMAX externals in one entry"); }
                    code[(size_t)8 * c + 3 + k] = (unsigned short)(A_EXT | t);
                    aext.push_back(make_int2(nb, -1)); t++;
                }
            }
        }
        arec[e] = make_int4(c0, cnt | (t << 16), extOff, 0);
    }
    std::vector<unsigned short> pool;
    FFM_TRY(share_blocks(code, arec, 8, "tile: amul code sharing", pool, &T->acodeUnique, &T->acodeTotal, nullptr));
    for (int k = 0; k < 2 * A_PF + 2; k++) arec.push_back(make_int4(0, 0, 0, 0));
    for (int k = 0; k < 2 * A_XMAX; k++) aext.push_back(make_int2(0, -1));
    FFM_TRY(upv(A->ctx, &T->arec, arec)); FFM_TRY(upv(A->ctx, &T->aext, aext));
    FFM_HIP(hipMalloc((void **)&T->acode, sizeof(unsigned short) * pool.size()));
    FFM_TRY(ffm_h2d(A->ctx, T->acode, pool.data(), sizeof(unsigned short) * pool.size()));
    // segments: enough workgroups to fill the chip, each long enough to amortise the A_WIN entries read twice at either end
    {
        const std::vector<int> &grpEntH = T->grpEntHost;
        // measured at 400^3 (r02, scripts/tile_probe.py): 16 entries 0.82 ms, 24 0.83, 32 0.84, 64 0.87, a whole tile (430) 0.93, 8 0.94 --
        // short segments balance the 256 CUs better than their two extra ring entries cost
        const int L = std::min(20, std::max(16, nEnt / 2048));
        std::vector<int4> seg;
        for (int g = 0; g < T->G; g++) for (int a = grpEntH[g]; a < grpEntH[g + 1]; a += L) seg.push_back(make_int4(g, a, std::min(a + L, grpEntH[g + 1]), grpEntH[g + 1]));
        T->nSeg = (int)seg.size();
        FFM_TRY(upv(A->ctx, &T->aseg, seg));
        FFM_HIP(hipMalloc((void **)&T->amulPartials, sizeof(double) * std::max(T->nSeg, 1)));      // x.y of every segment (fused dot)
    }
    T->amulUsable = true;
    return FFM_OK;
}

int ffm_tile_build(ffm_ldu *A, const std::vector<int> &lev, const std::vector<int> &bl, const std::vector<int> &grpCell)
{
    A->tile = new ffm_tile_plan();
    ffm_tile_plan *T = A->tile;
    T->G = (int)grpCell.size() - 1;
    if (T->G <= 0) return FFM_OK;
    const int nOwn = A->nOwned;
    if ((long)A->nCells * 24 >= (1L << 32)) return FFM_OK;         // the kernel addresses its streams with 32-bit byte offsets
    std::vector<int> grpOfCell(nOwn);
    for (int g = 0; g < T->G; g++) for (int c = grpCell[g]; c < grpCell[g + 1]; c++) grpOfCell[c] = g;
    bool ok = true;
    std::vector<int4> recF;
    { FfmStageTimer tm_("tile: forward plan"); FFM_TRY(build_dir(A, true, lev, grpCell, grpOfCell, T->f, ok, &recF, &T->grpEntHost)); }
    if (ok) { FfmStageTimer tm_("tile: backward plan"); FFM_TRY(build_dir(A, false, bl, grpCell, grpOfCell, T->b, ok)); }
    T->usable = ok;
    if (ok) {
        T->nMail = (long)T->f.nPub + T->b.nPub + 2;
        FFM_HIP(hipMalloc((void **)&T->mailAll, sizeof(double) * T->nMail));
        T->f.mail = T->mailAll; T->b.mail = T->mailAll + T->f.nPub + 1;
        FfmStageTimer tm_("tile: amul plan");
        FFM_TRY(build_amul(A, grpOfCell, recF));
        // the Gauss-Seidel sweeps need the upper-neighbour tables: without them the matrix gets level-scheduled sweeps
        if (!T->gsTables) T->usable = false;
    }
    return FFM_OK;
}

// ------------------------------------------------------------------ device ---
struct TileView {
    int G;
    const int *grpCell, *grpEnt, *extOff, *extSrc;
    const int4 *rec;
    const uint2 *code;
    unsigned int *ticket;      // [0] ticket counter, [1] abort word
};

__device__ __forceinline__ double t_ld(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void t_st(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// workgroup barrier that only waits for this wave's LDS traffic: outstanding global loads (the read-ahead) stay in flight
__device__ __forceinline__ void t_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ bool t_pending(double v) { return (unsigned long long)__double_as_longlong(v) == T_SENT; }

enum { TM_FWD = 0, TM_BWD = 1, TM_RD = 2, TM_GSF = 3, TM_GSB = 4 };
struct __attribute__((aligned(8))) T3 { double a, b, c; };       // the three coefficients of a cell
static_assert(T_W == 3, "T3");

// slow path of a mailbox read: re-load until the producer's value has replaced the sentinel; bounded, watches the abort word
__device__ __noinline__ double t_wait_value(const double *addr, unsigned int *ticket, int *shAbort)
{
    double v = t_ld(addr);
    if (*(volatile int *)shAbort) return v;
    unsigned spins = 0;
    while (t_pending(v)) {
        __builtin_amdgcn_s_sleep(1);
        v = t_ld(addr);
        if ((++spins & 1023u) == 0u) {
            if (__hip_atomic_load(&ticket[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) { *shAbort = 1; break; }
            if (spins > T_SPIN_LIMIT) { __hip_atomic_store(&ticket[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); *shAbort = 1; break; }
        }
    }
    return v;
}

// One kernel sweeps NF systems that share the off-diagonal coefficients (NF = 1: the matrix's own system).  The segregated solves of
// a vector equation (fvMatrix::solveSegregated: the components of U differ in the boundary diagonal and the source only) and the
// species equations under a multivariateSelection scheme (solver/YEEqn.H:43-60: one set of face weights, one diffusivity) are such
// systems: neighbour codes and coefficients are read once, every system has its own ring in LDS, its own mailboxes and its own
// diagonal / right-hand side / result; a level costs one barrier for all of them and their dependency chains interleave.
// Per system i:
// TM_FWD: w[c] = rD[c]*r[c] - sum_k rD[c]*a[c][k]*w[l_k]           (k ascending: the reference's face order)
// TM_BWD: w[c] -= sum_k rD[c]*a[c][k]*w[u_k]                       (k descending)
// TM_RD : D[c] = diag[c] - sum_k a[c][k]*b[c][k]/D[l_k]            (k ascending); D stays in the ring and the mailboxes, w[c] = 1/D[c]
// (dg = rD for TM_FWD / TM_BWD, the diagonal for TM_RD)
// The per-level path is issue-bound (one wave per SIMD runs the whole entry), so
//   * waves 0-3 ("compute") are kept free of divergent branches: idle lanes work on a dummy cell, only stores are predicated;
//   * wave 4 ("mail") does nothing but bring the external values of the next entry into LDS: entry record -> mailbox slot
//     list -> mailbox values, each stage read ahead, re-loading a value while it still reads the sentinel.  Its few loads
//     have a vmcnt stream of their own, so waiting for a mailbox value never waits for the compute waves' read-ahead.
// Every wave executes the same number of workgroup barriers: one after the prologue, one per entry of the padded loop.
// FUSE (PCG, DIC; one system): the vector updates on either side of the preconditioner ride on the sweeps' own streams --
//   TM_FWD: aux = the residual, updated in place first: rA -= alpha*q (q = A pA: r when given, else w on entry; PCG.C "rA[cell] -= alpha*wA[cell]"),
//           partials[group] = sum |rA| (the residual norm of the iteration that just ended);
//   TM_BWD: partials[group] = sum wA*rA of the finished preconditioned residual (PCG.C wArA = gSumProd(wA, rA)).
// The per-cell arithmetic is that of k_pcg_xr / the unfused sweep; only the order of the two sums differs (as in any reduction).
// R: the ring length.  The plan's codes are LDS slots of a T_RING ring; a shorter ring (five rings of T_RING doubles do not fit the
// LDS) takes an in-ring code modulo R and an external code rebased from T_RING to R, and serves plans whose ring neighbours lie
// within R - 2*T_ENT cells (TileDir::reach, ffm_tile_multi_fits).
constexpr int TM_PF = 4;            // read-ahead of the sweeps of several systems (NF systems' operands per slot)
constexpr int TM_RING5 = 2048;
// entries fetched ahead of the one being computed (register budget: one system 8, 6 with a second coefficient triple)
constexpr int tile_pf(int NF, int MODE) { return NF > 1 ? TM_PF : (MODE == TM_RD || MODE == TM_GSF) ? 6 : T_PF; }
static_assert(T_PM < TM_PF && tile_pf(1, TM_RD) <= T_PF && TM_PF <= T_PF, "read-ahead distances");
template <int NF> struct TileSys { const double *dg[NF]; const double *r[NF]; double *w[NF]; double *mail[NF]; };

template <int MODE, int NF, int R = T_RING, bool FUSE = false>
__global__ __launch_bounds__(T_THREADS + 64) void k_tile(TileView t, const double *__restrict__ ca, const double *__restrict__ cb, TileSys<NF> m,
                                                         double *aux = nullptr, const double *__restrict__ scal = nullptr, double *__restrict__ partials = nullptr)
{
    static_assert(R <= T_RING && (R & (R - 1)) == 0 && R > 2 * T_ENT, "ring length");
    static_assert(!FUSE || MODE == TM_FWD || MODE == TM_BWD, "fused vector updates: DIC/DILU application only");
    static_assert(MODE == TM_FWD || MODE == TM_BWD || MODE == TM_RD, "DILU / DIC application and calcReciprocalD (Gauss-Seidel: k_tile_gs)");
    static_assert(NF == 1 || !FUSE, "fused vector updates: one system");
    constexpr int LDS = R + 2 * T_XMAX + 1;
    constexpr bool ASC = MODE != TM_BWD;
    constexpr bool TWO = MODE == TM_RD;                         // a second triple of per-cell doubles (cb)
    constexpr bool VEC = MODE != TM_RD;                         // a per-system vector operand (pv)
    constexpr int W = T_W, PF = tile_pf(NF, MODE);
    __shared__ double ring[NF][LDS];    // per system: ring of this group's values, the two halo buffers, the dummy slot
    __shared__ double shSum[4];
    __shared__ int4 shRec[4];           // entry records handed from the mail wave to the compute waves
    __shared__ int shG;
    __shared__ int shAbort;
    const unsigned tid = threadIdx.x;
    if (tid == 0) {
        const unsigned tk = atomicAdd(&t.ticket[0], 1u);
        const int k = (int)(tk % (unsigned)t.G);
        shG = ASC ? k : t.G - 1 - k; shAbort = 0;
    }
    __syncthreads();
    const int g = __builtin_amdgcn_readfirstlane(shG);
    const unsigned gs = (unsigned)__builtin_amdgcn_readfirstlane(t.grpCell[g]);
    const int e0 = __builtin_amdgcn_readfirstlane(t.grpEnt[g]), e1 = __builtin_amdgcn_readfirstlane(t.grpEnt[g + 1]);
    if (e0 >= e1) { if (FUSE && tid == 0) partials[g] = 0.0; return; }

    if (tid >= (unsigned)T_THREADS) {
        // ------------------------------------------------------------------ mail wave
        const unsigned lane = tid - (unsigned)T_THREADS;
        int4 qrec[PF];                  // record of entry e + 2*PF .. (slot = (e - e0) % PF)
        unsigned qne[PF], qxi[PF];      // externals and this lane's mailbox slot of entry e + PF ..
        unsigned qxo[PF];               // first extSrc index, with the record
        double qxv[PF][NF];             // mailbox values of entry e + T_PM ..
#define Q_REC(k, e) { const int e_ = min((e), e1); qrec[k] = t.rec[e_]; qxo[k] = (unsigned)t.extOff[e_]; }
#define Q_IDX(k, e) { const int4 R_ = qrec[k]; qne[k] = ((e) < e1) ? ((unsigned)R_.y >> 16) : 0u; qxi[k] = (unsigned)t.extSrc[qxo[k] + (lane < qne[k] ? lane : 0u)]; }
#define Q_MAIL(k) { _Pragma("unroll") for (int i_ = 0; i_ < NF; i_++) qxv[k][i_] = t_ld(&m.mail[i_][lane < qne[k] ? qxi[k] : 0u]); }
#define Q_PUT(k, e) {                                                                                    \
        if (lane < qne[k]) {                                                                              \
            _Pragma("unroll") for (int i_ = 0; i_ < NF; i_++) {                                           \
                double v_ = qxv[k][i_];                                                                   \
                if (__builtin_expect(t_pending(v_), 0)) v_ = t_wait_value(&m.mail[i_][qxi[k]], t.ticket, &shAbort); \
                ring[i_][R + (((e) & 1) * T_XMAX) + lane] = v_;                                           \
            }                                                                                             \
        }                                                                                                 \
    }
#pragma unroll
        for (int k = 0; k < PF; k++) Q_REC(k, e0 + k);
#pragma unroll
        for (int k = 0; k < PF; k++) { Q_IDX(k, e0 + k); Q_REC(k, e0 + PF + k); }
#pragma unroll
        for (int k = 0; k < T_PM; k++) Q_MAIL(k);
        Q_PUT(0, e0);
        if (lane == 0) shRec[(e0 + PF) & 3] = qrec[0];
        t_barrier();
        for (int e = e0; e < e1; e += PF) {
#pragma unroll
            for (int k = 0; k < PF; k++) {
                const int ee = e + k;
                Q_PUT((k + 1) % PF, ee + 1);            // externals of the next entry
                if (lane == 0) shRec[(ee + 1 + PF) & 3] = qrec[(k + 1) % PF];         // record the compute waves fetch from next
                Q_IDX(k, ee + PF);
                Q_REC(k, ee + 2 * PF);
                Q_MAIL((k + T_PM) % PF);
                t_barrier();
            }
        }
#undef Q_REC
#undef Q_IDX
#undef Q_MAIL
#undef Q_PUT
        return;             // (the fused sums are reduced by the compute waves alone)
    }

    // ---------------------------------------------------------------------- compute waves
    // read-ahead registers: slot k serves the entries e with (e - e0) % PF == k
    unsigned pc[PF], ppb[PF];
    bool pok[PF];
    uint2 pq[PF];
    double pa[PF][W], pb[PF][TWO ? W : 1], pd[PF][NF], pv[PF][VEC ? NF : 1], pv2[FUSE ? PF : 1];
    double fsum = 0.0;
    const double fAlpha = (FUSE && MODE == TM_FWD) ? scal[S_ALPHA] : 0.0;
    const bool fSing = (FUSE && MODE == TM_FWD) ? (scal[S_SING] != 0.0) : false;
#define T_FETCH(k, e, R_) {                                                                             \
        const unsigned cnt_ = ((e) < e1) ? ((unsigned)R_.y & 0xFFFFu) : 0u;                              \
        const bool ok_ = tid < cnt_;                                                                     \
        const unsigned ps_ = ok_ ? (ASC ? tid : cnt_ - 1u - tid) : 0u;      /* position in the entry's code block; idle lanes: its first cell */ \
        const unsigned cc_ = ok_ ? (unsigned)R_.x + ps_ : gs;                                            \
        const unsigned o8_ = cc_ * 8u, o24_ = cc_ * 24u;        /* 32-bit byte offsets: arrays < 4 GiB (host check) */  \
        pq[k] = *(const uint2 *)((const char *)t.code + ((unsigned)R_.w + ps_ * 8u));                    \
        { const T3 v_ = *(const T3 *)((const char *)ca + o24_); pa[k][0] = v_.a; pa[k][1] = v_.b; pa[k][2] = v_.c; }     \
        if (TWO) { const T3 v_ = *(const T3 *)((const char *)cb + o24_); pb[k][0] = v_.a; pb[k][TWO ? 1 : 0] = v_.b; pb[k][TWO ? 2 : 0] = v_.c; } \
        _Pragma("unroll") for (int i_ = 0; i_ < NF; i_++) {                                              \
            pd[k][i_] = *(const double *)((const char *)m.dg[i_] + o8_);                                 \
            if (VEC) pv[k][VEC ? i_ : 0] = *(const double *)((const char *)((FUSE && MODE == TM_FWD) ? (const double *)aux : MODE == TM_BWD ? (const double *)m.w[i_] : m.r[i_]) + o8_); \
        }                                                                                                \
        if (FUSE) pv2[FUSE ? k : 0] = *(const double *)((const char *)((MODE == TM_FWD && !m.r[0]) ? (const double *)m.w[0] : m.r[0]) + o8_); \
        pc[k] = cc_; pok[k] = ok_; ppb[k] = (unsigned)R_.z;                                              \
    }
#pragma unroll
    for (int k = 0; k < PF; k++) { const int4 R0 = t.rec[min(e0 + k, e1)]; T_FETCH(k, e0 + k, R0); }
    t_barrier();
    for (int e = e0; e < e1; e += PF) {
#pragma unroll
        for (int k = 0; k < PF; k++) {
            const int ee = e + k;                           // entries past e1 are padding of the unrolled loop: barriers only
            const int4 Rn = shRec[(ee + PF) & 3];           // record of the entry to fetch below (from the mail wave)
            // ---- entry ee from slot k (idle lanes work on the dummy cell gs; nothing of theirs is stored)
            {
                const unsigned c = pc[k];
                const unsigned cd[4] = {pq[k].x & 0xFFFFu, pq[k].x >> 16, pq[k].y & 0xFFFFu, pq[k].y >> 16};
                unsigned sl[W];                             // the plan stores the LDS slot itself (of a T_RING ring)
#pragma unroll
                for (int s = 0; s < W; s++)
                    sl[s] = (R == T_RING) ? min(cd[s], (unsigned)(LDS - 1))
                                          : (cd[s] < (unsigned)T_RING ? (cd[s] & (unsigned)(R - 1)) : min(cd[s] - (unsigned)(T_RING - R), (unsigned)(LDS - 1)));
                double val[NF];
#pragma unroll
                for (int i = 0; i < NF; i++) {
                    const double d = pd[k][i], v0 = VEC ? pv[k][VEC ? i : 0] : 0.0;
                    double x[W], v;         // one system: the three LDS reads are issued ahead of the arithmetic (issue-bound path)
                    if (NF == 1) {
#pragma unroll
                        for (int s = 0; s < W; s++) x[s] = ring[i][sl[s]];
                    }
#define T_X(s) (NF == 1 ? x[s] : ring[i][sl[s]])
                    if (MODE == TM_FWD) {
                        double ri = v0;
                        if (FUSE) {
                            if (!fSing) { ri -= fAlpha * pv2[FUSE ? k : 0]; if (pok[k]) *(double *)((char *)aux + c * 8u) = ri; }
                            fsum += pok[k] ? fabs(ri) : 0.0;
                        }
                        v = d * ri;
#pragma unroll
                        for (int s = 0; s < W; s++) { const double nv = v - d * pa[k][s] * T_X(s); v = (cd[s] != T_NONE) ? nv : v; }
                    } else if (MODE == TM_BWD) {
                        v = v0;
#pragma unroll
                        for (int s = W - 1; s >= 0; s--) { const double nv = v - d * pa[k][s] * T_X(s); v = (cd[s] != T_NONE) ? nv : v; }
                    } else {
                        v = d;
#pragma unroll
                        for (int s = 0; s < W; s++) { const double nv = v - pa[k][s] * pb[k][TWO ? s : 0] / T_X(s); v = (cd[s] != T_NONE) ? nv : v; }
                    }
                    val[i] = v;
#undef T_X
                }
                // the stores of an active lane.  One system: two predicated blocks, so that the arithmetic above stays outside them
                // (issue-bound path, see above); several: one block (the form their register budget was tuned with)
#define T_PUT(i) { *(double *)((char *)m.w[i] + c * 8u) = (MODE == TM_RD) ? 1.0 / val[i] : val[i]; ring[i][(c - gs) & (unsigned)(R - 1)] = val[i]; }
#define T_POST(i) { if (cd[3] != T_NONE) t_st(&m.mail[i][ppb[k] + cd[3]], val[i]); }
                if (NF == 1) {
                    if (pok[k]) T_PUT(0);
                    if (FUSE && MODE == TM_BWD) fsum += pok[k] ? val[0] * pv2[FUSE ? k : 0] : 0.0;
                    if (pok[k]) T_POST(0);
                } else if (pok[k]) {
#pragma unroll
                    for (int i = 0; i < NF; i++) { T_PUT(i); T_POST(i); }
                }
#undef T_PUT
#undef T_POST
            }
            // ---- refill slot k with entry ee + PF
            T_FETCH(k, ee + PF, Rn);
            t_barrier();                                    // one barrier per level: ring and halo are visible to the next entry
        }
    }
#undef T_FETCH
    if (FUSE) {             // the four compute waves (the mail wave has left): wave sums through LDS, lane 0 adds them in wave order
        double v = fsum;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((tid & 63u) == 0u) shSum[tid >> 6] = v;
        t_barrier();
        if (tid == 0) partials[g] = ((shSum[0] + shSum[1]) + shSum[2]) + shSum[3];
    }
}

// The Gauss-Seidel row sweeps of the matrix's own system keep a kernel of their own: as NF = 1 instantiations of k_tile the forward sweep
// ran 1.4 % slower at 200^3 than this form, whatever read-ahead depth or store order was tried (profiles/README.md), and the sweep is
// bound by its per-level issue path.  Same plan, same mailbox protocol, same wave roles and barrier discipline as k_tile.
// TM_GSF: forward row sweep: v = bPrime[c] - sum_k lower[c][k]*psi[l_k] (new values); aux[c] = v (kept for the reverse sweep of
//         symGaussSeidel); v -= b[c][k] for k = 0..2 (b = upper*psi_old of the upper neighbours, computed by k_tile_gs_products;
//         +0.0 where there is none); psi[c] = v/diag[c]
// TM_GSB: reverse row sweep: v = aux[c] - sum_k upper[c][k]*psi[u_k] (new values, k ascending); psi[c] = v/diag[c]
// (dg = the diagonal, r = bPrime / aux, w = psi)
template <int MODE>
__global__ __launch_bounds__(T_THREADS + 64) void k_tile_gs(TileView t, double *mail, const double *__restrict__ ca, const double *__restrict__ cb,
                                                            const double *__restrict__ dg, const double *__restrict__ r, double *w, double *aux)
{
    static_assert(MODE == TM_GSF || MODE == TM_GSB, "the Gauss-Seidel row sweeps");
    constexpr bool ASC = MODE != TM_GSB;
    constexpr bool TWO = MODE == TM_GSF;        // a second triple of per-cell doubles (cb)
    constexpr int W = T_W;
    constexpr int PF = tile_pf(1, MODE);
    __shared__ double ring[T_LDS];                    // ring of this group's values, the two halo buffers, the dummy slot
    double *const halo = ring + T_RING;
    __shared__ int4 shRec[4];           // entry records handed from the mail wave to the compute waves
    __shared__ int shG;
    __shared__ int shAbort;
    const unsigned tid = threadIdx.x;
    if (tid == 0) {
        const unsigned tk = atomicAdd(&t.ticket[0], 1u);
        const int k = (int)(tk % (unsigned)t.G);
        shG = ASC ? k : t.G - 1 - k; shAbort = 0;
    }
    __syncthreads();
    const int g = __builtin_amdgcn_readfirstlane(shG);
    const unsigned gs = (unsigned)__builtin_amdgcn_readfirstlane(t.grpCell[g]);
    const int e0 = __builtin_amdgcn_readfirstlane(t.grpEnt[g]), e1 = __builtin_amdgcn_readfirstlane(t.grpEnt[g + 1]);
    if (e0 >= e1) return;

    if (tid >= (unsigned)T_THREADS) {
        // ------------------------------------------------------------------ mail wave
        const unsigned lane = tid - (unsigned)T_THREADS;
        int4 qrec[PF];                // record of entry e + 2*PF .. (slot = (e - e0) % PF)
        unsigned qne[PF], qxi[PF];  // externals and this lane's mailbox slot of entry e + PF ..
        unsigned qxo[PF];           // first extSrc index, with the record
        double qxv[PF];               // mailbox value of entry e + T_PM ..
#define Q_REC(k, e) { const int e_ = min((e), e1); qrec[k] = t.rec[e_]; qxo[k] = (unsigned)t.extOff[e_]; }
#define Q_IDX(k, e) { const int4 R_ = qrec[k]; qne[k] = ((e) < e1) ? ((unsigned)R_.y >> 16) : 0u; qxi[k] = (unsigned)t.extSrc[qxo[k] + (lane < qne[k] ? lane : 0u)]; }
#define Q_MAIL(k) { qxv[k] = t_ld(&mail[lane < qne[k] ? qxi[k] : 0u]); }
#define Q_PUT(k, e) {                                                                                    \
        if (lane < qne[k]) {                                                                              \
            double v_ = qxv[k];                                                                           \
            if (__builtin_expect(t_pending(v_), 0)) v_ = t_wait_value(&mail[qxi[k]], t.ticket, &shAbort); \
            halo[(((e) & 1) * T_XMAX) + lane] = v_;                                                       \
        }                                                                                                 \
    }
#pragma unroll
        for (int k = 0; k < PF; k++) Q_REC(k, e0 + k);
#pragma unroll
        for (int k = 0; k < PF; k++) { Q_IDX(k, e0 + k); Q_REC(k, e0 + PF + k); }
#pragma unroll
        for (int k = 0; k < T_PM; k++) Q_MAIL(k);
        Q_PUT(0, e0);
        if (lane == 0) shRec[(e0 + PF) & 3] = qrec[0];
        t_barrier();
        for (int e = e0; e < e1; e += PF) {
#pragma unroll
            for (int k = 0; k < PF; k++) {
                const int ee = e + k;
                Q_PUT((k + 1) % PF, ee + 1);          // externals of the next entry
                if (lane == 0) shRec[(ee + 1 + PF) & 3] = qrec[(k + 1) % PF];     // record the compute waves fetch from next
                Q_IDX(k, ee + PF);
                Q_REC(k, ee + 2 * PF);
                Q_MAIL((k + T_PM) % PF);
                t_barrier();
            }
        }
#undef Q_REC
#undef Q_IDX
#undef Q_MAIL
#undef Q_PUT
        return;
    }

    // ---------------------------------------------------------------------- compute waves
    // read-ahead registers: slot k serves the entries e with (e - e0) % PF == k
    unsigned pc[PF], ppb[PF];
    bool pok[PF];
    uint2 pq[PF];
    double pa[PF][W], pb[PF][TWO ? W : 1], pd[PF], pv[PF];
#define T_FETCH(k, e, R_) {                                                                             \
        const unsigned cnt_ = ((e) < e1) ? ((unsigned)R_.y & 0xFFFFu) : 0u;                              \
        const bool ok_ = tid < cnt_;                                                                     \
        const unsigned ps_ = ok_ ? (ASC ? tid : cnt_ - 1u - tid) : 0u;      /* position in the entry's code block; idle lanes: its first cell */ \
        const unsigned cc_ = ok_ ? (unsigned)R_.x + ps_ : gs;                                            \
        const unsigned o8_ = cc_ * 8u, o24_ = cc_ * 24u;        /* 32-bit byte offsets: arrays < 4 GiB (host check) */  \
        pq[k] = *(const uint2 *)((const char *)t.code + ((unsigned)R_.w + ps_ * 8u));                    \
        { const T3 v_ = *(const T3 *)((const char *)ca + o24_); pa[k][0] = v_.a; pa[k][1] = v_.b; pa[k][2] = v_.c; }     \
        if (TWO) { const T3 v_ = *(const T3 *)((const char *)cb + o24_); pb[k][0] = v_.a; pb[k][TWO ? 1 : 0] = v_.b; pb[k][TWO ? 2 : 0] = v_.c; } \
        pd[k] = *(const double *)((const char *)dg + o8_);                                               \
        pv[k] = *(const double *)((const char *)r + o8_);                                                \
        pc[k] = cc_; pok[k] = ok_; ppb[k] = (unsigned)R_.z;                                              \
    }
#pragma unroll
    for (int k = 0; k < PF; k++) { const int4 R0 = t.rec[min(e0 + k, e1)]; T_FETCH(k, e0 + k, R0); }
    t_barrier();
    for (int e = e0; e < e1; e += PF) {
#pragma unroll
        for (int k = 0; k < PF; k++) {
            const int ee = e + k;                           // entries past e1 are padding of the unrolled loop: barriers only
            const int4 Rn = shRec[(ee + PF) & 3];         // record of the entry to fetch below (from the mail wave)
            // ---- entry ee from slot k (idle lanes work on the dummy cell gs; nothing of theirs is stored)
            {
                const unsigned c = pc[k];
                const unsigned cd[4] = {pq[k].x & 0xFFFFu, pq[k].x >> 16, pq[k].y & 0xFFFFu, pq[k].y >> 16};
                double x[W];
#pragma unroll
                for (int s = 0; s < W; s++) x[s] = ring[min(cd[s], (unsigned)(T_LDS - 1))];     // the plan stores the LDS slot itself
                const double d = pd[k];
                double val;
                if (MODE == TM_GSF) {
                    val = pv[k];
#pragma unroll
                    for (int s = 0; s < W; s++) { const double nv = val - pa[k][s] * x[s]; val = (cd[s] != T_NONE) ? nv : val; }
                    if (pok[k]) *(double *)((char *)aux + c * 8u) = val;
#pragma unroll
                    for (int s = 0; s < W; s++) val -= pb[k][TWO ? s : 0];
                    val = val / d;
                } else {
                    val = pv[k];
#pragma unroll
                    for (int s = 0; s < W; s++) { const double nv = val - pa[k][s] * x[s]; val = (cd[s] != T_NONE) ? nv : val; }
                    val = val / d;
                }
                if (pok[k]) { *(double *)((char *)w + c * 8u) = val; ring[(c - gs) & (unsigned)(T_RING - 1)] = val; }
                if (pok[k] && cd[3] != T_NONE) t_st(&mail[ppb[k] + cd[3]], val);
            }
            // ---- refill slot k with entry ee + PF
            T_FETCH(k, ee + PF, Rn);
            t_barrier();                                    // one barrier per level: ring and halo are visible to the next entry
        }
    }
#undef T_FETCH
}

// out[i] = native[src[i]] (0 where a cell has fewer than T_W neighbours): coefficients in the kernel's cell-major layout
__global__ void k_tile_gather(long n, const int *__restrict__ src, const double *__restrict__ native, double *__restrict__ out)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int q = src[i];
        out[i] = (q >= 0) ? native[q] : 0.0;
    }
}
// mailbox fill before a sweep (pair); it also zeroes the group ticket counter, so that the 32-bit counter never wraps and every
// launch hands its groups out as ticket % G with ticket < 2 G (forward sweep 0..G-1, backward sweep G..2G-1)
__global__ void k_tile_fill(long n, unsigned long long *p, unsigned long long v, unsigned int *ticket)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) ticket[0] = 0u;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = v;
}

static TileView tview(const ffm_ldu *A, const TileDir &d)
{
    TileView t; t.G = A->tile->G; t.grpCell = A->grpCell; t.grpEnt = d.grpEnt; t.extOff = d.extOff; t.extSrc = d.extSrc; t.rec = d.rec;
    t.code = (const uint2 *)d.code; t.ticket = A->sweepTicket;
    return t;
}

// gathered coefficients of one direction, refreshed when the matrix coefficients changed
static int tile_coef(ffm_ldu *A, TileDir &d, bool upper, const double **out)
{
    const long n = (long)T_W * A->nOwned;
    double *&buf = upper ? d.coefU : d.coefL;
    unsigned long &ep = upper ? d.epochU : d.epochL;
    if (!buf) { FFM_HIP(hipMalloc((void **)&buf, sizeof(double) * std::max<long>(n, 1))); ep = ~0ul; }
    if (ep != A->offDiagEpoch) {
        const int g = std::max(1, std::min(ffm_grid(n, 256), 8 * RED_BLOCKS));
        hipLaunchKernelGGL(k_tile_gather, dim3(g), dim3(256), 0, A->ctx->stream, n, d.src, upper ? A->upper : A->lower, buf);
        ep = A->offDiagEpoch;
        A->tileGathers++;
    }
    *out = buf;
    return FFM_OK;
}

// The same arrays written by the kernel that assembles the matrix (ffm_device.hpp: store_triple) instead of gathered from its native
// coefficients: the forward direction's upper (and, lower: lower) coefficients and the backward direction's upper ones, handed out
// for writing.  They count as stale from here on; ffm_tile_coef_written declares them current for native arrays that the same
// launch wrote, and the bind of exactly those arrays (ffm_ldu_bind_coeffs_native_d) adopts them for the epoch it opens.  Any
// other set / bind, and any plain assembly entry point of the mesh (it may refill the same arrays), drops the declaration and the
// next sweep gathers.  b.coefL (transposed DILU) is always gathered.
// FFM_ERR_UNSUPPORTED, nothing touched: a block with ghost cells (their faces are dropped from the triples), no tile plan, rows
// wider than T_W (the assembly kernel's slots would not be the plan's).
bool ffm_tile_coef_direct_ok(const ffm_ldu *A) { return ffm_tile_usable(A) && A->nCells == A->nOwned && A->maxW <= T_W && A->identity; }
int ffm_tile_coef_direct(ffm_ldu *A, bool lower, double **fU, double **fL, double **bU)
{
    if (!ffm_tile_coef_direct_ok(A)) {
        ffm_set_error("sweep-layout coefficients cannot be written directly: ghost cells, no tile plan or rows wider than %d", T_W);
        return FFM_ERR_UNSUPPORTED;
    }
    ffm_tile_plan *T = A->tile;
    const size_t bytes = sizeof(double) * std::max<long>((long)T_W * A->nOwned, 1);
    double **buf[3] = {&T->f.coefU, lower ? &T->f.coefL : nullptr, &T->b.coefU};
    for (double **b : buf) if (b && !*b) FFM_HIP(hipMalloc((void **)b, bytes));
    T->f.epochU = T->b.epochU = ~0ul;
    if (lower) T->f.epochL = ~0ul;
    A->directPending = false;
    *fU = T->f.coefU; *fL = lower ? T->f.coefL : nullptr; *bU = T->b.coefU;
    return FFM_OK;
}
void ffm_tile_coef_written(ffm_ldu *A, const double *upper_d, const double *lower_d)
{
    A->directPending = true; A->directUpper = upper_d; A->directLower = (lower_d && lower_d != upper_d) ? lower_d : nullptr;
}
// (called by the bind that found its arrays declared: the epoch is the one it has just opened)
void ffm_tile_coef_adopt(ffm_ldu *A)
{
    ffm_tile_plan *T = A->tile;
    T->f.epochU = T->b.epochU = A->offDiagEpoch;
    if (A->directLower) T->f.epochL = A->offDiagEpoch;
}
// tests: one of the plan's arrays as a sweep would find it -- made current first -- on the host; which: 0 f.coefU, 1 f.coefL,
// 2 b.coefU, 3 b.coefL; out_h [3*nOwned].  And the number of gathers this matrix has launched.
extern "C" int ffm_ldu_tile_coef_read(ffm_ldu *A, int which, double *out_h)
{
    if (!A || !out_h || which < 0 || which > 3) return FFM_ERR_ARG;
    if (!ffm_tile_usable(A)) { ffm_set_error("ffm_ldu_tile_coef_read: the matrix has no tile plan"); return FFM_ERR_UNSUPPORTED; }
    const double *p;
    FFM_TRY(tile_coef(A, which < 2 ? A->tile->f : A->tile->b, !(which & 1), &p));
    return ffm_d2h(A->ctx, out_h, p, sizeof(double) * (size_t)T_W * A->nOwned);
}
extern "C" long ffm_ldu_tile_gathers(const ffm_ldu *A) { return A ? (long)A->tileGathers : -1; }
// bytes of neighbour codes the plan keeps (the pool's blocks) and bytes its entries refer to (what per-cell arrays would hold);
// which: 0 forward sweep, 1 backward sweep, 2 tiled Amul (0 / 0 where the matrix has no ring plan for it)
extern "C" int ffm_ldu_tile_code_bytes(const ffm_ldu *A, int which, long *uniqueBytes, long *totalBytes)
{
    if (!A || !uniqueBytes || !totalBytes || which < 0 || which > 2) return FFM_ERR_ARG;
    if (!ffm_tile_usable(A)) { ffm_set_error("ffm_ldu_tile_code_bytes: the matrix has no tile plan"); return FFM_ERR_UNSUPPORTED; }
    const ffm_tile_plan *T = A->tile;
    *uniqueBytes = which == 0 ? T->f.codeUnique : which == 1 ? T->b.codeUnique : T->acodeUnique;
    *totalBytes = which == 0 ? T->f.codeTotal : which == 1 ? T->b.codeTotal : T->acodeTotal;
    return FFM_OK;
}

static void tile_fill(ffm_ldu *A, double *p, long n)
{
    const int g = std::max(1, std::min(ffm_grid(n, 256), 8 * RED_BLOCKS));
    hipLaunchKernelGGL(k_tile_fill, dim3(g), dim3(256), 0, A->ctx->stream, n, (unsigned long long *)p, T_SENT, A->sweepTicket);
}

// n systems in one sweep: up to four on the plan's own ring, five on the short one where the plan's ring neighbours are near enough
bool ffm_tile_multi_fits(const ffm_ldu *A, int n)
{
    if (n < 1 || n > FFM_TILE_MAXSYS || !ffm_tile_usable(A)) return false;
    return n <= 4 || std::max(A->tile->f.reach, A->tile->b.reach) <= TM_RING5 - 2 * T_ENT;
}
extern "C" int ffm_ldu_tile_reach(const ffm_ldu *A, int *reach, int *limit, int *limit5)
{
    if (!A || !reach || !limit || !limit5) return FFM_ERR_ARG;
    if (!ffm_tile_usable(A)) { ffm_set_error("ffm_ldu_tile_reach: the matrix has no tile plan"); return FFM_ERR_UNSUPPORTED; }
    *reach = std::max(A->tile->f.reach, A->tile->b.reach); *limit = T_RINGD; *limit5 = TM_RING5 - 2 * T_ENT;
    return FFM_OK;
}
// The mailboxes of n systems, filled with the sentinel for the next sweep (pair): system i's are (*mail) + i*nMail.  One system has
// the plan's own (fwdOnly: only the forward direction's are filled); several have [FFM_TILE_MAXSYS][nMail] of their own
static int tile_mail(ffm_ldu *A, int n, bool fwdOnly, double **mail)
{
    ffm_tile_plan *T = A->tile;
    if (n > 1 && !T->mailMulti) FFM_HIP(hipMalloc((void **)&T->mailMulti, sizeof(double) * (size_t)FFM_TILE_MAXSYS * (size_t)T->nMail));
    *mail = (n == 1) ? T->mailAll : T->mailMulti;
    tile_fill(A, *mail, (n == 1 && fwdOnly) ? (long)T->f.nPub + 1 : (long)n * T->nMail);
    return FFM_OK;
}
// one sweep of direction d over NF systems (r: null where the mode has no right-hand side; r[0] null in a fused forward sweep: q = w)
template <int MODE, int NF, int R = T_RING, bool FUSE = false>
static void tile_launch(ffm_ldu *A, const TileDir &d, double *mail, const double *ca, const double *cb, const double *const *dg, const double *const *r,
                        double *const *w, double *aux = nullptr, const double *scal = nullptr, double *partials = nullptr)
{
    ffm_tile_plan *T = A->tile;
    TileSys<NF> m;
    for (int i = 0; i < NF; i++) { m.dg[i] = dg[i]; m.r[i] = r ? r[i] : nullptr; m.w[i] = w[i]; m.mail[i] = mail + (size_t)i * T->nMail + (d.mail - T->mailAll); }
    hipLaunchKernelGGL((k_tile<MODE, NF, R, FUSE>), dim3(T->G), dim3(T_THREADS + 64), 0, A->ctx->stream, tview(A, d), ca, cb, m, aux, scal, partials);
}
#define TILE_SWEEP(MODE, n, ...) switch (n) { case 1: tile_launch<MODE, 1>(__VA_ARGS__); break; case 2: tile_launch<MODE, 2>(__VA_ARGS__); break; \
                                             case 3: tile_launch<MODE, 3>(__VA_ARGS__); break; case 4: tile_launch<MODE, 4>(__VA_ARGS__); break; \
                                             default: tile_launch<MODE, 5, TM_RING5>(__VA_ARGS__); break; }
// DILU / DIC application of n = 1 .. FFM_TILE_MAXSYS systems with the matrix's off-diagonal coefficients and their own reciprocal
// diagonals: w[i] = precondition(r[i])
int ffm_tile_precond(ffm_ldu *A, int precond, bool transpose, int n, const double *const *rD, const double *const *r, double *const *w)
{
    ffm_tile_plan *T = A->tile;
    if (!ffm_tile_multi_fits(A, n)) { ffm_set_error("ffm_tile_precond: %d systems do not fit this matrix's tile plan", n); return FFM_ERR_ARG; }
    // forward coefficient: DIC upper; DILU lower; DILU^T upper.  backward: DIC upper; DILU upper; DILU^T lower.
    const bool fwdUpper = (precond == FFM_DIC) || transpose;
    const bool bwdUpper = (precond == FFM_DIC) || !transpose;
    const double *cf, *cb; double *mail;
    FFM_TRY(tile_coef(A, T->f, fwdUpper, &cf));
    FFM_TRY(tile_coef(A, T->b, bwdUpper, &cb));
    FFM_TRY(tile_mail(A, n, false, &mail));
    TILE_SWEEP(TM_FWD, n, A, T->f, mail, cf, nullptr, rD, r, w);
    TILE_SWEEP(TM_BWD, n, A, T->b, mail, cb, nullptr, rD, nullptr, w);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}
// D[i] = 1/(diag[i] - sum upper*lower/D[i][l]) in face order for n systems
int ffm_tile_calc_rD(ffm_ldu *A, int n, const double *const *diag, double *const *D)
{
    ffm_tile_plan *T = A->tile;
    if (!ffm_tile_multi_fits(A, n)) { ffm_set_error("ffm_tile_calc_rD: %d systems do not fit this matrix's tile plan", n); return FFM_ERR_ARG; }
    const double *cu, *cl; double *mail;
    FFM_TRY(tile_coef(A, T->f, true, &cu));
    if (A->lower == A->upper) cl = cu; else FFM_TRY(tile_coef(A, T->f, false, &cl));
    FFM_TRY(tile_mail(A, n, true, &mail));
    TILE_SWEEP(TM_RD, n, A, T->f, mail, cu, cl, diag, nullptr, D);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

__global__ void k_tile_sum_partials(int n, const double *__restrict__ partials, double *__restrict__ scal, int slot, ffm_scal_op t);
// PCG with DIC on a tile plan: the two halves of the preconditioner application with the neighbouring vector
// updates fused in (k_tile<.., FUSE>).  Forward: rA -= scal[S_ALPHA]*wA, scal[slot] = sum |rA| (local), wA = forward sweep of rA.
// Backward: finishes wA, scal[slot] = sum wA*rA (local).  t: the scalar operation that follows the sum, run by the launch that sums.
bool ffm_tile_pcg_fusable(const ffm_ldu *A)
{
    const char *e = getenv("FFM_PCG_UNFUSED");
    const bool off = e && atoi(e) != 0;
    return !off && ffm_tile_usable(A) && A->tile->G <= 4 * RED_BLOCKS;
}
int ffm_tile_pcg_fwd(ffm_ldu *A, double *rA, double *wA, int slot, const double *qA, const ffm_scal_op &t)
{
    ffm_tile_plan *T = A->tile;
    hipStream_t s = A->ctx->stream;
    const double *cf, *cb, *rD = A->rD; double *mail;
    FFM_TRY(tile_coef(A, T->f, true, &cf));
    FFM_TRY(tile_coef(A, T->b, true, &cb));
    FFM_TRY(tile_mail(A, 1, false, &mail));
    tile_launch<TM_FWD, 1, T_RING, true>(A, T->f, mail, cf, nullptr, &rD, &qA, &wA, rA, A->ctx->scal_d, A->ctx->partials_d);
    hipLaunchKernelGGL(k_tile_sum_partials, dim3(1), dim3(1024), 0, s, T->G, (const double *)A->ctx->partials_d, A->ctx->scal_d, slot, t);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}
int ffm_tile_pcg_bwd(ffm_ldu *A, const double *rA, double *wA, int slot, const ffm_scal_op &t)
{
    ffm_tile_plan *T = A->tile;
    hipStream_t s = A->ctx->stream;
    const double *cb, *rD = A->rD;
    FFM_TRY(tile_coef(A, T->b, true, &cb));
    tile_launch<TM_BWD, 1, T_RING, true>(A, T->b, T->mailAll, cb, nullptr, &rD, &rA, &wA, nullptr, A->ctx->scal_d, A->ctx->partials_d);      // (mailboxes: filled by the forward half)
    hipLaunchKernelGGL(k_tile_sum_partials, dim3(1), dim3(1024), 0, s, T->G, (const double *)A->ctx->partials_d, A->ctx->scal_d, slot, t);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

// upper*psi_old of the (owned) upper neighbours of every cell, slot by slot; +0.0 where a cell has fewer than three
__global__ void k_tile_gs_products(long n3, const int *__restrict__ nbrCell, const double *__restrict__ coef, const double *__restrict__ psi,
                                   double *__restrict__ out)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n3; i += (long)gridDim.x * blockDim.x) {
        const int nb = nbrCell[i];
        out[i] = (nb >= 0) ? coef[i] * psi[nb] : 0.0;
    }
}

// One GaussSeidelSmoother / symGaussSeidelSmoother sweep (forward rows, then reverse rows when sym): psi in place, bP = bPrime
// (source with the lagged interface terms), bSave = scratch [nCells].  prod = scratch [3*nCells].
int ffm_tile_gs(ffm_ldu *A, bool sym, double *psi, const double *bP, double *bSave, double *prod)
{
    ffm_tile_plan *T = A->tile;
    hipStream_t s = A->ctx->stream;
    const double *cl, *cu; double *mail;
    FFM_TRY(tile_coef(A, T->f, A->lower == A->upper, &cl));        // lower coefficients, lower-neighbour layout
    FFM_TRY(tile_coef(A, T->b, true, &cu));                         // upper coefficients, upper-neighbour layout
    const long n3 = (long)T_W * A->nOwned;
    hipLaunchKernelGGL(k_tile_gs_products, dim3(std::max(1, std::min(ffm_grid(n3, 256), 8 * RED_BLOCKS))), dim3(256), 0, s, n3,
                       (const int *)T->upNbrCell, cu, (const double *)psi, prod);
    FFM_TRY(tile_mail(A, 1, false, &mail));
    hipLaunchKernelGGL(k_tile_gs<TM_GSF>, dim3(T->G), dim3(T_THREADS + 64), 0, s, tview(A, T->f), T->f.mail, cl, (const double *)prod, (const double *)A->diag, bP, psi, bSave);
    if (sym)
        hipLaunchKernelGGL(k_tile_gs<TM_GSB>, dim3(T->G), dim3(T_THREADS + 64), 0, s, tview(A, T->b), T->b.mail, cu, (const double *)nullptr, (const double *)A->diag,
                           (const double *)bSave, psi, (double *)nullptr);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

// ------------------------------------------------------------------ tiled Amul: kernels ---
struct AmulView {
    int G;
    const int *grpCell, *grpEnt;
    const int4 *rec, *seg;
    const uint4 *code;
    const int2 *ext;
};

// y[c] = diag[c]*x[c] + sum_lower coef*x[l] + sum_upper(owned) coef*x[u]   (lduMatrix::Amul row order); DOT: partial of x.y
// FUSEP (PCG): x is not read but formed on the way into the rings, x = w + beta*pin (PCG.C "pA = wA + beta*pA"), and stored to pout
// by the segment that owns the row, together with psi += alpha*pin (the solution update left over from the iteration before);
// pin / pout are two buffers (a neighbouring workgroup may still need the old direction), y must not alias w.
// ASYM (asymmetric matrices: the transport equations): the coefficient of a lower face is not the owner's upper coefficient from
// the ring but the cell's own triple lc[3c + k] of lower coefficients (the array the forward DILU sweep streams, gathered once
// per coefficient update); x still comes through the rings / external buffers.
template <bool DOT, bool FUSEP = false, bool ASYM = false>
__global__ __launch_bounds__(T_THREADS + 64) void k_tile_amul(AmulView t, const double *__restrict__ bc, const double *__restrict__ upper,
                                                              const double *__restrict__ diag, const double *__restrict__ x,
                                                              double *__restrict__ y, double *__restrict__ partials,
                                                              const double *__restrict__ pin = nullptr, double *__restrict__ pout = nullptr,
                                                              double *__restrict__ psi = nullptr, const double *__restrict__ scal = nullptr,
                                                              const double *__restrict__ lc = nullptr)
{
    // FUSEP: x = w on entry.  A singular flag leaves direction and solution as they are (k_p_psi's guard)
    const bool fSing = FUSEP ? (scal[S_SING] != 0.0) : false;
    const double fBeta = FUSEP ? scal[S_BETA] : 0.0, fAlpha = FUSEP ? scal[S_ALPHA] : 0.0;
    __shared__ double xring[A_RING + 2 * A_XMAX];           // x of the window, then the two external-x buffers
    __shared__ double cring[3 * A_RING + 2 * A_XMAX];       // upper coefficients of the window, then the external coefficients
    __shared__ int4 shRec[4];
    __shared__ double sm[8];
    const unsigned tid = threadIdx.x;
    // segment [sa, sb) of group g: rows of these entries are computed; the rings also need the A_WIN entries on either side
    const int4 S = t.seg[blockIdx.x];
    const int g = S.x, sa = S.y, sb = S.z;
    const unsigned gs = (unsigned)t.grpCell[g];
    const int e0 = max(t.grpEnt[g], sa - A_WIN), e1 = min(S.w, sb + A_WIN);     // entries loaded
    double dot = 0.0;
    if (sa < sb) {
        if (tid >= (unsigned)T_THREADS) {
            // ---------------------------------------------------------------- mail wave: externals of the next entry
            const unsigned lane = tid - (unsigned)T_THREADS;
            int4 qrec[A_PF];
            unsigned qne[A_PF];
            int2 qi0[A_PF], qi1[A_PF];
            double qx0[A_PF], qx1[A_PF], qc0[A_PF], qc1[A_PF], qp0[FUSEP ? A_PF : 1], qp1[FUSEP ? A_PF : 1];
#define Q_REC(k, e) { qrec[k] = t.rec[min((e), e1)]; }
#define Q_IDX(k, e) { const int4 R_ = qrec[k]; qne[k] = ((e) < e1) ? ((unsigned)R_.y >> 16) : 0u;                       \
                      qi0[k] = t.ext[(unsigned)R_.z + (lane < qne[k] ? lane : 0u)];                                     \
                      qi1[k] = t.ext[(unsigned)R_.z + (lane + 64u < qne[k] ? lane + 64u : 0u)]; }
#define Q_VAL(k) { qx0[k] = x[qi0[k].x]; qx1[k] = x[qi1[k].x]; qc0[k] = upper[max(qi0[k].y, 0)]; qc1[k] = upper[max(qi1[k].y, 0)];     \
                   if (FUSEP) { qp0[FUSEP ? k : 0] = pin[qi0[k].x]; qp1[FUSEP ? k : 0] = pin[qi1[k].x]; } }
#define Q_X0(k) (FUSEP ? (fSing ? qp0[FUSEP ? k : 0] : qx0[k] + fBeta * qp0[FUSEP ? k : 0]) : qx0[k])
#define Q_X1(k) (FUSEP ? (fSing ? qp1[FUSEP ? k : 0] : qx1[k] + fBeta * qp1[FUSEP ? k : 0]) : qx1[k])
#define Q_PUT(k, e) { const unsigned hb_ = (unsigned)((e) & 1) * (unsigned)A_XMAX;                                      \
                      if (lane < qne[k]) { xring[A_RING + hb_ + lane] = Q_X0(k); cring[3 * A_RING + hb_ + lane] = qc0[k]; } \
                      if (lane + 64u < qne[k]) { xring[A_RING + hb_ + lane + 64u] = Q_X1(k); cring[3 * A_RING + hb_ + lane + 64u] = qc1[k]; } }
#pragma unroll
            for (int k = 0; k < A_PF; k++) Q_REC(k, e0 + k);
#pragma unroll
            for (int k = 0; k < A_PF; k++) { Q_IDX(k, e0 + k); Q_REC(k, e0 + A_PF + k); }
#pragma unroll
            for (int k = 0; k < T_PM; k++) Q_VAL(k);
            Q_PUT(0, e0);
            if (lane == 0) shRec[(e0 + A_PF) & 3] = qrec[0];
            t_barrier();
            for (int e = e0; e < sb; e += A_PF) {
#pragma unroll
                for (int k = 0; k < A_PF; k++) {
                    const int ee = e + k;
                    Q_PUT((k + 1) % A_PF, ee + 1);
                    if (lane == 0) shRec[(ee + 1 + A_PF) & 3] = qrec[(k + 1) % A_PF];
                    Q_IDX(k, ee + A_PF);
                    Q_REC(k, ee + 2 * A_PF);
                    Q_VAL((k + T_PM) % A_PF);
                    t_barrier();
                }
            }
#undef Q_REC
#undef Q_IDX
#undef Q_VAL
#undef Q_PUT
#undef Q_X0
#undef Q_X1
        } else {
            // ---------------------------------------------------------------- compute waves
            unsigned pc[A_PF];
            bool pok[A_PF], pst[A_PF];
            uint4 pq[A_PF];
            double pb[A_PF][3], pd[A_PF], px[A_PF], pp[FUSEP ? A_PF : 1], ps[FUSEP ? A_PF : 1], pl[ASYM ? A_PF : 1][3];
#define A_FETCH(k, e, R_) {                                                                              \
        const unsigned cnt_ = ((e) < e1) ? ((unsigned)(R_).y & 0xFFFFu) : 0u;                            \
        const bool ok_ = tid < cnt_;                                                                     \
        const unsigned cc_ = ok_ ? (unsigned)(R_).x + tid : gs;                                          \
        const unsigned o8_ = cc_ * 8u;                                                                   \
        pq[k] = *(const uint4 *)((const char *)t.code + ((unsigned)(R_).w + (ok_ ? tid : 0u) * 16u));     /* the entry's code block; idle lanes: its first cell */ \
        { const T3 v_ = *(const T3 *)((const char *)bc + cc_ * 24u); pb[k][0] = v_.a; pb[k][1] = v_.b; pb[k][2] = v_.c; } \
        pd[k] = *(const double *)((const char *)diag + o8_);                                             \
        px[k] = *(const double *)((const char *)x + o8_);                                                \
        if (FUSEP) { pp[FUSEP ? k : 0] = *(const double *)((const char *)pin + o8_); ps[FUSEP ? k : 0] = *(const double *)((const char *)psi + o8_); } \
        if (ASYM) { const T3 v_ = *(const T3 *)((const char *)lc + cc_ * 24u); pl[ASYM ? k : 0][0] = v_.a; pl[ASYM ? k : 0][1] = v_.b; pl[ASYM ? k : 0][2] = v_.c; } \
        pc[k] = cc_; pok[k] = ok_; pst[k] = ok_ && (e) >= sa && (e) < sb;                                \
    }
#define A_FILL(k) { if (FUSEP) px[k] = fSing ? pp[FUSEP ? k : 0] : px[k] + fBeta * pp[FUSEP ? k : 0];                      \
                    if (pok[k]) { const unsigned i_ = (pc[k] - gs) & (unsigned)(A_RING - 1); xring[i_] = px[k];    \
                                   cring[3u * i_] = pb[k][0]; cring[3u * i_ + 1u] = pb[k][1]; cring[3u * i_ + 2u] = pb[k][2]; } }
#pragma unroll
            for (int k = 0; k < A_PF; k++) { const int4 R0 = t.rec[min(e0 + k, e1)]; A_FETCH(k, e0 + k, R0); }
#pragma unroll
            for (int k = 0; k < A_AHEAD; k++) A_FILL(k);
            t_barrier();
            for (int e = e0; e < sb; e += A_PF) {
#pragma unroll
                for (int k = 0; k < A_PF; k++) {
                    const int ee = e + k;
                    const int4 Rn = shRec[(ee + A_PF) & 3];
                    {
                        const unsigned c = pc[k];
                        const unsigned hb = (unsigned)(ee & 1) * (unsigned)A_XMAX;
                        const unsigned cd[6] = {pq[k].x & 0xFFFFu, pq[k].x >> 16, pq[k].y & 0xFFFFu, pq[k].y >> 16, pq[k].z & 0xFFFFu, pq[k].z >> 16};
                        const double xc = px[k];
                        double acc = pd[k] * xc;
#pragma unroll
                        for (int s = 0; s < 3; s++) {       // lower faces: x and the coefficient from the owner's ring slot
                            const unsigned m = (unsigned)((int)(cd[s] << 16) >> 31);
                            const unsigned ri = (c - (cd[s] & 0x7FFu) - gs) & (unsigned)(A_RING - 1);
                            const unsigned hi = hb + (cd[s] & (unsigned)(A_XMAX - 1));
                            const unsigned xi = ri ^ ((ri ^ ((unsigned)A_RING + hi)) & m);
                            const unsigned ci = (3u * ri + ((cd[s] >> 12) & 3u)) ^ (((3u * ri + ((cd[s] >> 12) & 3u)) ^ (3u * (unsigned)A_RING + hi)) & m);
                            const double nv = acc + (ASYM ? pl[ASYM ? k : 0][s] : cring[ci]) * xring[xi];
                            acc = (cd[s] != A_NONE) ? nv : acc;
                        }
#pragma unroll
                        for (int s = 0; s < 3; s++) {       // upper faces: own coefficient
                            const unsigned u = cd[3 + s];
                            const unsigned m = (unsigned)((int)(u << 16) >> 31);
                            const unsigned ri = (c + (u & 0x7FFu) - gs) & (unsigned)(A_RING - 1);
                            const unsigned xi = ri ^ ((ri ^ ((unsigned)A_RING + hb + (u & (unsigned)(A_XMAX - 1)))) & m);
                            const double nv = acc + pb[k][s] * xring[xi];
                            acc = (u != A_NONE) ? nv : acc;
                        }
                        if (pst[k]) __builtin_nontemporal_store(acc, (double *)((char *)y + c * 8u));
                        if (FUSEP && pst[k]) {
                            *(double *)((char *)pout + c * 8u) = xc;
                            if (!fSing) *(double *)((char *)psi + c * 8u) = ps[FUSEP ? k : 0] + fAlpha * pp[FUSEP ? k : 0];
                        }
                        if (DOT) dot += pst[k] ? acc * xc : 0.0;
                    }
                    A_FILL((k + A_AHEAD) % A_PF);           // rings: entry ee + A_AHEAD
                    A_FETCH(k, ee + A_PF, Rn);
                    t_barrier();
                }
            }
#undef A_FETCH
#undef A_FILL
        }
    }
    if (DOT) {
        const double rsum = block_sum(dot, sm);
        if (tid == 0) partials[blockIdx.x] = rsum;
    }
}

// faces towards ghost cells, in slot order, added to the finished owned part of the row
template <bool SUB>
__global__ void k_amul_tail(int n, const int *__restrict__ cell, const int *__restrict__ start, const int *__restrict__ face,
                            const int *__restrict__ nbr, const double *__restrict__ upper, const double *__restrict__ x, double *__restrict__ y)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = cell[i];
    double acc = y[c];
    for (int q = start[i]; q < start[i + 1]; q++) { const double t = upper[face[q]] * x[nbr[q]]; acc = SUB ? acc - t : acc + t; }
    y[c] = acc;
}

// Gauss-Seidel on a block with ghost cells: bPrime = source - (faces towards ghost cells)*psi_ghost, the lagged explicit
// treatment OpenFOAM gives coupled patches (GaussSeidelSmoother: bPrime = source; updateMatrixInterfaces with negated coeffs)
int ffm_tile_gs_ghost_terms(ffm_ldu *A, const double *psi, double *bP)
{
    ffm_tile_plan *T = A->tile;
    if (T->nTail > 0)
        hipLaunchKernelGGL(k_amul_tail<true>, dim3((T->nTail + 255) / 256), dim3(256), 0, A->ctx->stream, T->nTail, (const int *)T->tailCell,
                           (const int *)T->tailStart, (const int *)T->tailFace, (const int *)T->tailNbr, (const double *)A->upper, psi, bP);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

__global__ __launch_bounds__(1024) void k_tile_sum_partials(int n, const double *__restrict__ partials, double *__restrict__ scal, int slot, ffm_scal_op t)
{
    __shared__ double sm[16];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partials[i];
    const double r = block_sum(acc, sm);
    if (threadIdx.x == 0) { scal[slot] = r; run_scal_op(scal, t); }
}

bool ffm_tile_amul_usable(const ffm_ldu *A) { return ffm_tile_usable(A) && A->tile->amulUsable && A->symmetric && A->ifaces.empty(); }

// y = A x for an asymmetric matrix on the tile plan (transport equations): upper coefficients from the backward sweep's gathered
// array, lower coefficients from the forward sweep's; ghost faces by the tail kernel as in the symmetric case
bool ffm_tile_amul_asym_usable(const ffm_ldu *A)
{
    return ffm_tile_usable(A) && A->tile->amulUsable && !A->symmetric && A->ifaces.empty();
}
int ffm_tile_amul_asym(ffm_ldu *A, const double *x, double *y)
{
    ffm_tile_plan *T = A->tile;
    hipStream_t s = A->ctx->stream;
    const double *bcoef, *lcoef;
    FFM_TRY(tile_coef(A, T->b, true, &bcoef));
    FFM_TRY(tile_coef(A, T->f, false, &lcoef));
    AmulView v; v.G = T->G; v.grpCell = A->grpCell; v.grpEnt = T->f.grpEnt; v.rec = T->arec; v.seg = T->aseg; v.code = T->acode; v.ext = T->aext;
    hipLaunchKernelGGL((k_tile_amul<false, false, true>), dim3(T->nSeg), dim3(T_THREADS + 64), 0, s, v, bcoef, (const double *)A->upper, (const double *)A->diag, x, y,
                       (double *)nullptr, (const double *)nullptr, (double *)nullptr, (double *)nullptr, (const double *)nullptr, lcoef);
    FFM_TRY(ffm_ghost_exchange_end(A));
    if (T->nTail > 0)
        hipLaunchKernelGGL(k_amul_tail<false>, dim3((T->nTail + 255) / 256), dim3(256), 0, s, T->nTail, (const int *)T->tailCell, (const int *)T->tailStart,
                           (const int *)T->tailFace, (const int *)T->tailNbr, (const double *)A->upper, x, y);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

// PCG: pout = w + beta*pin, psi += alpha*pin, y = A pout, scal[dotSlot] = pout.y (local), in one pass (k_tile_amul<true, true>)
bool ffm_tile_amul_pcg_usable(const ffm_ldu *A)
{
    return ffm_tile_amul_usable(A) && A->tile->nTail == 0 && A->ghNbrRank.empty();
}
int ffm_tile_amul_pcg(ffm_ldu *A, const double *w, const double *pin, double *pout, double *psi, double *y, int dotSlot, const ffm_scal_op &t)
{
    ffm_tile_plan *T = A->tile;
    hipStream_t s = A->ctx->stream;
    const double *bcoef;
    FFM_TRY(tile_coef(A, T->b, true, &bcoef));
    AmulView v; v.G = T->G; v.grpCell = A->grpCell; v.grpEnt = T->f.grpEnt; v.rec = T->arec; v.seg = T->aseg; v.code = T->acode; v.ext = T->aext;
    hipLaunchKernelGGL((k_tile_amul<true, true>), dim3(T->nSeg), dim3(T_THREADS + 64), 0, s, v, bcoef, (const double *)A->upper, (const double *)A->diag, w, y,
                       T->amulPartials, pin, pout, psi, (const double *)A->ctx->scal_d);
    hipLaunchKernelGGL(k_tile_sum_partials, dim3(1), dim3(1024), 0, s, T->nSeg, (const double *)T->amulPartials, A->ctx->scal_d, dotSlot, t);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

// y = A x (symmetric A); dotSlot >= 0: also scal[dotSlot] = x.y over the owned rows (local part), followed by the operation t
int ffm_tile_amul(ffm_ldu *A, const double *x, double *y, int dotSlot, const ffm_scal_op &t)
{
    ffm_tile_plan *T = A->tile;
    hipStream_t s = A->ctx->stream;
    const double *bcoef;
    FFM_TRY(tile_coef(A, T->b, true, &bcoef));
    AmulView v; v.G = T->G; v.grpCell = A->grpCell; v.grpEnt = T->f.grpEnt; v.rec = T->arec; v.seg = T->aseg; v.code = T->acode; v.ext = T->aext;
    const bool fusedDot = dotSlot >= 0 && T->nTail == 0;
    if (fusedDot) {
        FFM_TRY(ffm_ghost_exchange_end(A));          // (no ghost faces on this rank: nothing in flight that the kernel would need)
        hipLaunchKernelGGL((k_tile_amul<true>), dim3(T->nSeg), dim3(T_THREADS + 64), 0, s, v, bcoef, (const double *)A->upper, (const double *)A->diag, x, y, T->amulPartials);
        hipLaunchKernelGGL(k_tile_sum_partials, dim3(1), dim3(1024), 0, s, T->nSeg, (const double *)T->amulPartials, A->ctx->scal_d, dotSlot, t);
    } else {
        hipLaunchKernelGGL((k_tile_amul<false>), dim3(T->nSeg), dim3(T_THREADS + 64), 0, s, v, bcoef, (const double *)A->upper, (const double *)A->diag, x, y, (double *)nullptr);
        FFM_TRY(ffm_ghost_exchange_end(A));          // an overlapped ghost refresh (ffm_ghost_exchange_begin) must have landed before the tail
        if (T->nTail > 0)
            hipLaunchKernelGGL(k_amul_tail<false>, dim3((T->nTail + 255) / 256), dim3(256), 0, s, T->nTail, (const int *)T->tailCell, (const int *)T->tailStart,
                               (const int *)T->tailFace, (const int *)T->tailNbr, (const double *)A->upper, x, y);
    }
    FFM_HIP(hipGetLastError());
    return fusedDot || dotSlot < 0 ? FFM_OK : 1;       // 1: the caller still has to take the dot product
}

extern "C" int ffm_debug_set_sweep_ticket(ffm_ldu *A, unsigned int value)
{
    if (!A || !A->sweepTicket) return FFM_ERR_ARG;
    FFM_HIP(hipStreamSynchronize(A->ctx->stream));
    FFM_TRY(ffm_h2d(A->ctx, A->sweepTicket, &value, sizeof(value)));
    return FFM_OK;
}

// Diagnostics: resident workgroups per CU the runtime predicts for the forward / backward sweep kernels and the tiled Amul
extern "C" int ffm_debug_tile_occupancy(int *out3)
{
    if (!out3) return FFM_ERR_ARG;
    FFM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&out3[0], (k_tile<TM_FWD, 1>), T_THREADS + 64, 0));
    FFM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&out3[1], (k_tile<TM_BWD, 1>), T_THREADS + 64, 0));
    FFM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&out3[2], k_tile_amul<true>, T_THREADS + 64, 0));
    return FFM_OK;
}
