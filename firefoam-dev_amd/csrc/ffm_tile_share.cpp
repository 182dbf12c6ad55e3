// ffm_tile_share.cpp -- content sharing of the tile plans' neighbour-code blocks (host only, no ROCm header: g++ builds it as well).
//
// The tiled sweeps and the tiled Amul (ffm_tile.hip) read, per cell, a few 16-bit neighbour codes that never change after the plan is
// built.  A code names an LDS slot or a cell distance, never an absolute cell, so the codes of one entry (<= 256 cells of one level)
// are the same bytes for every entry in the same position of a structured tile: on a box of 16 x 16 column tiles a full level has
// 256 cells in one fixed order, the ring slots repeat every T_RING/256 levels, and all interior tiles look alike.  The plan therefore
// keeps every distinct block of codes once, in a pool, and gives each entry the byte offset of its block; the pool of a large box is
// about 1 MB and stays in the L2 where the per-cell arrays were streamed from memory by every sweep.  Nothing here knows a mesh: blocks
// are compared by content, and a plan without repeating entries gets a pool as large as its per-cell array.
#include "ffm_host.hpp"
#include <cstdint>
#include <unordered_map>

static inline uint64_t share_hash(const unsigned short *p, size_t n)
{
    uint64_t h = 0x9E3779B97F4A7C15ull * (uint64_t)(n + 1);
    size_t i = 0;
    for (; i + 4 <= n; i += 4) { uint64_t w; memcpy(&w, p + i, 8); h = (h ^ w) * 0xFF51AFD7ED558CCDull; h ^= h >> 29; }
    for (; i < n; i++) { h = (h ^ p[i]) * 0xC4CEB9FE1A85EC53ull; h ^= h >> 31; }
    return h;
}

// Block i = codes[start[i], start[i] + len[i]) (shorts).  share: the pool holds every distinct block once, in the order of first
// appearance; else the pool IS the code array and block i stays where it was (offset 2*start[i]): the per-cell layout, byte for byte.
// off[i]: byte offset of block i in the pool (an empty block: 0).  The pool is extended by padShorts shorts of 0xFFFF that belong to
// no block.  uniqueBytes / totalBytes: the blocks of the pool / of the input, without the padding.  `codes` is consumed.
int ffm_tile_share(std::vector<unsigned short> &codes, const std::vector<long> &start, const std::vector<int> &len, bool share, long padShorts,
                   std::vector<unsigned short> &pool, std::vector<unsigned> &off, long *uniqueBytes, long *totalBytes, const char *what)
{
    FfmStageTimer tm_(what ? what : "tile: code sharing");
    const long nB = (long)start.size();
    long total = 0;
    for (long i = 0; i < nB; i++) {
        if (len[i] < 0 || start[i] < 0 || start[i] + len[i] > (long)codes.size()) { ffm_set_error("internal: code block %ld outside the code array", i); return FFM_ERR_ARG; }
        total += len[i];
    }
    off.assign(nB, 0u);
    pool.clear();
    long unique = 0;
    if (!share) {
        pool.swap(codes);
        for (long i = 0; i < nB; i++) off[i] = len[i] ? (unsigned)(2 * start[i]) : 0u;
        unique = total;
        if (2 * (long)pool.size() + 2 * padShorts >= (1L << 32)) { ffm_set_error("tile plan: neighbour codes of 4 GiB or more"); return FFM_ERR_UNSUPPORTED; }
    } else {
        std::vector<uint64_t> hash(nB);
        ffm_parallel_for(nB, [&](long a, long b) { for (long i = a; i < b; i++) hash[i] = share_hash(codes.data() + start[i], (size_t)len[i]); }, 4096);
        // hash -> blocks already in the pool with that hash (chained through `next`); equal hashes are settled by comparing the bytes
        std::unordered_map<uint64_t, long> head;
        head.reserve((size_t)std::min<long>(nB, 1L << 16));
        std::vector<long> next(nB, -1);
        std::vector<long> poolAt(nB, -1);          // first short of block i's copy in the pool (representatives only)
        for (long i = 0; i < nB; i++) {
            if (!len[i]) continue;
            const unsigned short *p = codes.data() + start[i];
            auto it = head.find(hash[i]);
            long rep = -1;
            if (it != head.end())
                for (long j = it->second; j >= 0; j = next[j])
                    if (len[j] == len[i] && memcmp(pool.data() + poolAt[j], p, sizeof(unsigned short) * (size_t)len[i]) == 0) { rep = j; break; }
            if (rep < 0) {
                if (2 * ((long)pool.size() + len[i] + padShorts) >= (1L << 32)) { ffm_set_error("tile plan: neighbour codes of 4 GiB or more"); return FFM_ERR_UNSUPPORTED; }
                poolAt[i] = (long)pool.size();
                pool.insert(pool.end(), p, p + len[i]);
                if (it != head.end()) { next[i] = it->second; it->second = i; } else head.emplace(hash[i], i);
                rep = i;
            }
            off[i] = (unsigned)(2 * poolAt[rep]);
        }
        unique = (long)pool.size();
        std::vector<unsigned short>().swap(codes);
    }
    pool.insert(pool.end(), (size_t)std::max<long>(padShorts, 0), (unsigned short)0xFFFFu);
    if (uniqueBytes) *uniqueBytes = 2 * unique;
    if (totalBytes) *totalBytes = 2 * total;
    return FFM_OK;
}

// FFM_TILE_CODE_SHARE, read when a plan is built: 0 = every entry keeps a block of its own; otherwise a mask of the readers whose
// pools are shared, 1 = the sweeps (both directions), 2 = the tiled Amul (A/B runs of one reader); unset = 3, both
bool ffm_tile_share_enabled(int reader)
{
    const char *e = getenv("FFM_TILE_CODE_SHARE");
    const int mask = (e && *e) ? atoi(e) : 3;
    return (mask & reader) != 0;
}

// tests / tools: the routine on host arrays.  offset_out [nBlocks] byte offsets; pool_out [poolCapacity] shorts, at least
// (share ? sum of len : nCodes) + padShorts; *poolShorts: shorts written to pool_out (padding included); *uniqueShorts: without it
extern "C" int ffm_tile_share_codes(int nBlocks, const long *start, const int *len, const unsigned short *codes, long nCodes, int share, long padShorts,
                                    unsigned int *offset_out, unsigned short *pool_out, long poolCapacity, long *uniqueShorts, long *poolShorts)
{
    if (nBlocks < 0 || nCodes < 0 || padShorts < 0 || (nBlocks && (!start || !len || !offset_out)) || (nCodes && !codes) || !uniqueShorts || !poolShorts) {
        ffm_set_error("ffm_tile_share_codes: bad argument");
        return FFM_ERR_ARG;
    }
    std::vector<unsigned short> c(codes, codes + nCodes), pool;
    std::vector<long> s(start, start + nBlocks);
    std::vector<int> l(len, len + nBlocks);
    std::vector<unsigned> off;
    long ub = 0, tb = 0;
    FFM_TRY(ffm_tile_share(c, s, l, share != 0, padShorts, pool, off, &ub, &tb, nullptr));
    if ((long)pool.size() > poolCapacity || (pool.size() && !pool_out)) { ffm_set_error("ffm_tile_share_codes: the pool needs %ld shorts, %ld given", (long)pool.size(), poolCapacity); return FFM_ERR_ARG; }
    if (!pool.empty()) memcpy(pool_out, pool.data(), sizeof(unsigned short) * pool.size());
    for (int i = 0; i < nBlocks; i++) offset_out[i] = off[i];
    *uniqueShorts = ub / 2; *poolShorts = (long)pool.size();
    return FFM_OK;
}
