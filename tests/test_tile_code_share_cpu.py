"""The content sharing of the tile plans' neighbour-code blocks (csrc/ffm_tile_share.cpp) without a GPU, through its C entry point
ffm_tile_share_codes, on designed inputs: expanding the pool by the offsets gives back every input short, the pool holds no block twice,
blocks are told apart by content (last short, length, common prefix), and the switch-off form is the code array itself."""
import ctypes as C

import numpy as np
import pytest

PAD = 24


def _share(ffm, blocks, share=1, pad=PAD, gaps=False):
    """blocks: list of uint16 arrays -> (offsets [bytes], pool [shorts, padding included], unique shorts)"""
    L = ffm.lib()
    parts, start, pos = [], [], 0
    for b in blocks:
        if gaps:                    # shorts between the blocks that belong to none
            parts.append(np.full(3, 0xABCD, np.uint16)); pos += 3
        start.append(pos); parts.append(np.asarray(b, np.uint16)); pos += len(b)
    codes = np.concatenate(parts) if parts else np.zeros(0, np.uint16)
    n = len(blocks)
    start = np.asarray(start, np.int64); ln = np.asarray([len(b) for b in blocks], np.int32)
    off = np.zeros(max(n, 1), np.uint32)
    cap = len(codes) + pad
    pool = np.zeros(max(cap, 1), np.uint16)
    uniq, used = C.c_long(-1), C.c_long(-1)
    rc = L.ffm_tile_share_codes(n, start.ctypes.data_as(C.POINTER(C.c_long)), ln.ctypes.data_as(C.POINTER(C.c_int)),
                                codes.ctypes.data_as(C.POINTER(C.c_ushort)), len(codes), share, pad, off.ctypes.data_as(C.POINTER(C.c_uint)),
                                pool.ctypes.data_as(C.POINTER(C.c_ushort)), cap, C.byref(uniq), C.byref(used))
    assert rc == 0, L.ffm_last_error()
    return off[:n], pool[:used.value], uniq.value, codes


def _check(blocks, off, pool, uniq, pad=PAD):
    assert len(pool) == uniq + pad and np.all(pool[uniq:] == 0xFFFF)            # the padding belongs to no block
    seen = {}
    for b, o in zip(blocks, off):
        b = np.asarray(b, np.uint16)
        if len(b) == 0:
            assert o == 0
            continue
        assert o % 2 == 0 and o // 2 + len(b) <= uniq
        assert np.array_equal(pool[o // 2: o // 2 + len(b)], b)                  # every input short comes back
        key = b.tobytes()
        assert seen.setdefault(key, int(o)) == o                                 # equal blocks: one offset
    assert len({v for v in seen.values()}) == len(seen)                          # distinct blocks: distinct offsets
    assert uniq == sum(len(k) // 2 for k in seen)                                # and the pool holds nothing else: no block twice
    return seen


def test_repeated_blocks_are_kept_once(ffm):
    rng = np.random.default_rng(1)
    kinds = [rng.integers(0, 0xFFFF, 4 * 256, dtype=np.uint16) for _ in range(16)]
    blocks = [kinds[(3 * i) % 16] for i in range(200)]
    off, pool, uniq, _ = _share(ffm, blocks)
    seen = _check(blocks, off, pool, uniq)
    assert len(seen) == 16 and uniq == 16 * 4 * 256
    first = [int(off[[(3 * i) % 16 for i in range(200)].index(k)]) for k in range(16)]
    assert sorted(first) == [2 * 4 * 256 * j for j in range(16)]                 # order of first appearance, back to back


def test_blocks_that_differ_in_the_last_short_only(ffm):
    a = np.arange(1000, 1000 + 4 * 37, dtype=np.uint16)
    b = a.copy(); b[-1] ^= 1
    c = a.copy(); c[0] ^= 0x8000
    blocks = [a, b, a, c, b, a.copy()]
    off, pool, uniq, _ = _share(ffm, blocks)
    seen = _check(blocks, off, pool, uniq)
    assert len(seen) == 3 and off[0] == off[2] == off[5] and off[1] == off[4] and len({off[0], off[1], off[3]}) == 3


def test_blocks_of_different_lengths_with_a_common_prefix(ffm):
    base = np.arange(1, 1 + 8 * 40, dtype=np.uint16)
    blocks = [base[:8 * 40], base[:8 * 39], base[:8], base[:8 * 40], base[:8 * 39], base[:4], base[:1], base[:8]]
    off, pool, uniq, _ = _share(ffm, blocks)
    seen = _check(blocks, off, pool, uniq)
    assert len(seen) == 5 and uniq == 8 * 40 + 8 * 39 + 8 + 4 + 1                # a prefix is a block of its own, never an alias


def test_empty_plan_and_one_entry(ffm):
    off, pool, uniq, _ = _share(ffm, [])
    assert len(off) == 0 and uniq == 0 and len(pool) == PAD and np.all(pool == 0xFFFF)
    one = [np.arange(4 * 200, dtype=np.uint16)]
    off, pool, uniq, _ = _share(ffm, one)
    _check(one, off, pool, uniq)
    assert off[0] == 0 and uniq == 800
    off, pool, uniq, _ = _share(ffm, [np.zeros(0, np.uint16), one[0], np.zeros(0, np.uint16)])          # entries without cells
    assert list(off) == [0, 0, 0] and uniq == 800


@pytest.mark.parametrize("n", [5000, 70000])          # 70000 blocks: the hashing runs on several threads
def test_many_blocks_some_equal(ffm, n):
    rng = np.random.default_rng(n)
    kind = rng.integers(0, 300, n)
    length = 4 * (1 + kind % 7)
    blocks = [((np.arange(length[i]) * 31 + 7 * kind[i]) & 0xFFFF).astype(np.uint16) for i in range(n)]
    off, pool, uniq, _ = _share(ffm, blocks, gaps=True)
    seen = _check(blocks, off, pool, uniq)
    assert len(seen) == len(set(kind))


def test_switched_off_every_block_stays_where_it_was(ffm):
    a = np.arange(64, dtype=np.uint16)
    blocks = [a, a, a[:32], a]
    off, pool, uniq, codes = _share(ffm, blocks, share=0, gaps=True)
    assert uniq == sum(len(b) for b in blocks)                                   # unique == total
    assert np.array_equal(pool[:len(codes)], codes) and np.all(pool[len(codes):] == 0xFFFF) and len(pool) == len(codes) + PAD
    pos = 0
    for b, o in zip(blocks, off):
        pos += 3
        assert o == 2 * pos
        pos += len(b)


def test_pool_too_small_is_refused(ffm):
    L = ffm.lib()
    codes = np.arange(16, dtype=np.uint16); start = np.array([0, 8], np.int64); ln = np.array([8, 8], np.int32)
    off = np.zeros(2, np.uint32); pool = np.zeros(8, np.uint16); u, p = C.c_long(), C.c_long()
    rc = L.ffm_tile_share_codes(2, start.ctypes.data_as(C.POINTER(C.c_long)), ln.ctypes.data_as(C.POINTER(C.c_int)),
                                codes.ctypes.data_as(C.POINTER(C.c_ushort)), 16, 1, 0, off.ctypes.data_as(C.POINTER(C.c_uint)),
                                pool.ctypes.data_as(C.POINTER(C.c_ushort)), 8, C.byref(u), C.byref(p))
    assert rc == -1 and b"pool needs 16 shorts" in L.ffm_last_error()           # FFM_ERR_ARG
    ln[1] = 9                                                                    # a block that runs past the code array
    rc = L.ffm_tile_share_codes(2, start.ctypes.data_as(C.POINTER(C.c_long)), ln.ctypes.data_as(C.POINTER(C.c_int)),
                                codes.ctypes.data_as(C.POINTER(C.c_ushort)), 16, 1, 0, off.ctypes.data_as(C.POINTER(C.c_uint)),
                                pool.ctypes.data_as(C.POINTER(C.c_ushort)), 8, C.byref(u), C.byref(p))
    assert rc == -1
