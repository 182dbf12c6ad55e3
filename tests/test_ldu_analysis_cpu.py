"""The dependency analysis behind ffm_renumber_* (csrc/ffm_ldu_analysis.cpp) without a GPU: every branch of analyse() -- detected box,
level-major order, chunk groups, hinted groups and their ranking, classes cut by internal walls, the two fall-backs to level-scheduled
sweeps, ghost cells, refused addressing -- must give exactly the numbering the library gave before the analysis was split into stages.

(a) DIGESTS: SHA-256 of newToOldCell followed by newToOldFace (int32 bytes), recorded from the library of commit 89df91d with
    `python tests/test_ldu_analysis_cpu.py` (the __main__ block prints the tables below).
(b) invariants that need no recording: permutations, l < u and owner-sorted faces after the renumbering, ghost cells in place, and for
    hinted meshes: renumbering the renumbered mesh with the renumbered hint is the identity (what the analysis memo relies on).
The FFM_VERBOSE line of the fall-back and split cases is read from the stderr of a child process."""
import contextlib
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

# recorded from commit 89df91d
DIGESTS = {
    "box_auto": "53743ed65b57c338c89a510532a4e3e291b621a2aea4135c00d9611901035839",
    "box_levels": "d64a98308e15f03e1c636c3816ea9efaf65a79b7a74a597bd228dc2a708b4b12",
    "box_chunks37": "2e782f3200548ab7b9bfba4a2d9d6a40b4c6496038b21476f2567de06d330ce1",
    "hint_tiles": "238e4b433c192661cab3ff5eedd2f5cd32bac3cca493b925dd4a728d7c8057dd",
    "hint_baffled": "6be1c9e2a4dad40ff7f6b5a1beaaad01a369070d221b59c7663ad559f57a3303",
    "hint_cyclic_auto": "9ac9c32e88bbeffdb7c9a5e5acc51074d54c1da42a611f175e43b5418b12d504",
    "hint_cyclic_tile": "c896abb787b489e2c9eaffc22cef5fa3ad99d8073394faa775799278b30a3d34",
    "wall_split": "4b0be005b93f3b44cf2fde7075a8ba964137a5ebcc1b5b771506b43ec76c4db2",
    "centres_hint": "93e34409667cee2d2e133c056373cba8c55ff6e24d73ba5e4b3a39d43ff8d604",
    "merged_hint": "9b0e3cc1dfb65f97ae5cf7e5de93fa9a95d5daf9df1781ae152d0f667e8c3c98",
    "ghost_block": "542b134d1d3448333a013b3a60ec5bedf4c83a9c1cd364c2fabf71a9bbef6e8a",
    "ghost_block_chunks17": "e448d4bacb7f6d95114f2c30f9f06851bae5725d5560260cc0ef040f1c75368a",
}
HINT_DIGESTS = {       # the labels of ffm_tile_hint_from_centres
    "centres_hint": "1db0276706b0fd3e9aec5bb6659db58982ee1ea405ae7066a9401a7e4ffb31e0",
}
VERBOSE = {            # the line a fall-back or split case prints to stderr under FFM_VERBOSE=1 (None: chunk groups, silently)
    "hint_cyclic_auto": "ffm: the group hint gives a cyclic group graph: level-scheduled sweeps",
    "wall_split": "ffm: 2 group labels in 4 connected pieces (internal walls): one group per piece",
    "merged_hint": "ffm: tiled sweeps not applicable (more than 3 lower or upper neighbours): level-scheduled sweeps",
    "hint_cyclic_tile": None,
}
BAD_ADDR = {           # (return code, ffm_last_error) of the two cases of test_abi_cpu.test_bad_addressing_is_rejected
    "unsorted": (-2, "LDU addressing: faces not sorted by owner at face 1"),
    "l_equals_u": (-2, "LDU addressing: face 0 has l=0 u=0 (need 0<=l<u<nCells=3)"),
}


def _ffm():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from ffm_import import ffm
    return ffm


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in ("FFM_SWEEP", "FFM_PIPE_GROUP_CELLS")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _box(ffm, n, hint=None, env=None):
    N, l, u = ffm.hexmesh.hex_ldu(*n)
    return dict(nOwn=N, nGhost=0, l=l, u=u, hint=None if hint is None else hint(np.arange(N), *n), env=env or {})


def _tiles3(c, nx, ny, nz):            # 3 x 3 tiles of cell columns (j, k)
    return ((c // nx) % ny) // 3 + 10 * ((c // (nx * ny)) // 3)


def _walled(ffm):
    """8 x 32 x 16 without the y-faces between j = 15 and 16: an internal wall across the whole box"""
    nx, ny, nz = 8, 32, 16
    m = _box(ffm, (nx, ny, nz))
    l, u = m["l"], m["u"]
    keep = ~((u - l == nx) & ((l // nx) % ny == 15))
    m["l"], m["u"] = l[keep], u[keep]
    return m, (nx, ny, nz)


def _ghost_block(ffm, env=None):
    N, l, u = ffm.hexmesh.hex_ldu(6, 5, 4)
    S = ffm.decompose.SubDomain(N, l, u, ffm.decompose.partition_graph(N, l, u, 2), 2, 0)
    assert S.nGhost > 0
    return dict(nOwn=S.nOwned, nGhost=S.nGhost, l=S.l, u=S.u, hint=None, env=env or {})


def _build(ffm, name):
    """the mesh, hint and switches of a case"""
    if name == "box_auto":
        return _box(ffm, (20, 18, 17))
    if name == "box_levels":
        return _box(ffm, (20, 18, 17), env={"FFM_SWEEP": "levels"})
    if name == "box_chunks37":
        return _box(ffm, (20, 18, 17), env={"FFM_SWEEP": "tile", "FFM_PIPE_GROUP_CELLS": "37"})
    if name == "hint_tiles":
        return _box(ffm, (11, 13, 12), _tiles3)
    if name == "hint_baffled":
        m = _box(ffm, (11, 13, 12), _tiles3)
        keep = ffm.hexmesh.hash_u(0xBAF, np.arange(len(m["l"]))) > 0.2
        m["l"], m["u"] = m["l"][keep], m["u"][keep]
        return m
    if name == "hint_cyclic_auto":
        return _box(ffm, (11, 13, 12), lambda c, *n: c % 2)
    if name == "hint_cyclic_tile":
        return _box(ffm, (11, 13, 12), lambda c, *n: c % 2, env={"FFM_SWEEP": "tile", "FFM_PIPE_GROUP_CELLS": "64"})
    if name == "wall_split":
        m, (nx, ny, nz) = _walled(ffm)
        m["hint"] = (np.arange(m["nOwn"]) // (nx * ny)) // 8
        return m
    if name == "centres_hint":
        m, (nx, ny, nz) = _walled(ffm)
        c = np.arange(m["nOwn"])
        centres = 0.1 * (np.stack([c % nx, (c // nx) % ny, c // (nx * ny)]) + 0.5)
        m["hint"] = ffm.tile_hint_from_centres(centres, tileCells=8)
        return m
    if name == "merged_hint":
        import merged_mesh as MM
        mm = MM.case("w16u14")
        j, k = np.floor(mm.C[:, 1] / 0.1).astype(int), np.floor(mm.C[:, 2] / 0.1).astype(int)
        return dict(nOwn=mm.nCells, nGhost=0, l=mm.l.astype(np.int32), u=mm.u.astype(np.int32), hint=j // 3 + 10 * (k // 3), env={})
    if name == "ghost_block":
        return _ghost_block(ffm)
    if name == "ghost_block_chunks17":
        return _ghost_block(ffm, {"FFM_SWEEP": "tile", "FFM_PIPE_GROUP_CELLS": "17"})
    raise KeyError(name)


CASES = ["box_auto", "box_levels", "box_chunks37", "hint_tiles", "hint_baffled", "hint_cyclic_auto", "hint_cyclic_tile", "wall_split",
         "centres_hint", "merged_hint", "ghost_block", "ghost_block_chunks17"]


def _renumber(ffm, m):
    with _env(m["env"]):
        return ffm.renumber_levels(m["nOwn"], m["l"], m["u"], groupHint=m["hint"], nGhost=m["nGhost"])


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, np.int32).tobytes())
    return h.hexdigest()


def _bad_addr(ffm, which):
    L = ffm.lib()
    l, u, F = {"unsorted": ([1, 0], [2, 1], 2), "l_equals_u": ([0], [0], 1)}[which]
    l, u = np.array(l, np.int32), np.array(u, np.int32)
    c, f = np.empty(3, np.int32), np.empty(2, np.int32)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    rc = L.ffm_renumber_levels(3, F, ip(l), ip(u), ip(c), ip(f))
    return rc, L.ffm_last_error().decode()


@pytest.mark.parametrize("name", CASES)
def test_numbering_is_the_recorded_one(ffm, name):
    m = _build(ffm, name)
    cOrd, fOrd = _renumber(ffm, m)
    nOwn, N, F = m["nOwn"], m["nOwn"] + m["nGhost"], len(m["l"])
    # (b) what holds for every numbering the library may choose
    assert np.array_equal(np.sort(cOrd), np.arange(N)) and np.array_equal(np.sort(fOrd), np.arange(F))
    assert np.array_equal(cOrd[nOwn:], np.arange(nOwn, N))                   # ghost cells keep their places
    l2, u2, oldToNew = ffm.hexmesh.apply_renumbering(N, m["l"], m["u"], cOrd, fOrd)
    assert (l2 < u2).all() and (np.diff(l2) >= 0).all()
    if m["hint"] is not None:
        again = dict(m, l=l2, u=u2, hint=np.asarray(m["hint"])[cOrd[:nOwn]])
        c3, f3 = _renumber(ffm, again)
        assert np.array_equal(c3, np.arange(N)) and np.array_equal(f3, np.arange(F))
    # (a) the numbering of the parent commit
    if name in HINT_DIGESTS:
        assert len(np.unique(m["hint"])) == 8
        assert _digest(m["hint"]) == HINT_DIGESTS[name]
    assert _digest(cOrd, fOrd) == DIGESTS[name]


@pytest.mark.parametrize("which", sorted(BAD_ADDR))
def test_bad_addressing_code_and_message(ffm, which):
    assert _bad_addr(ffm, which) == BAD_ADDR[which]


@pytest.fixture(scope="module")
def verbose_lines():
    """stderr of one child process that runs the cases of VERBOSE under FFM_VERBOSE=1, split by case"""
    env = dict(os.environ, FFM_VERBOSE="1")
    for k in ("FFM_SWEEP", "FFM_PIPE_GROUP_CELLS", "FFM_TIMING"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--verbose-child"] + sorted(VERBOSE), env=env, text=True,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr
    out, cur = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("== "):
            cur = out.setdefault(line[3:], [])
        elif cur is not None and line.startswith("ffm:"):
            cur.append(line)
    return out


@pytest.mark.parametrize("name", sorted(VERBOSE))
def test_verbose_line(verbose_lines, name):
    assert verbose_lines[name] == ([VERBOSE[name]] if VERBOSE[name] else [])


def _verbose_child(names):
    ffm = _ffm()
    for name in names:
        m = _build(ffm, name)
        sys.stderr.write("== %s\n" % name); sys.stderr.flush()
        _renumber(ffm, m)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--verbose-child"]:
        _verbose_child(sys.argv[2:])
    else:
        ffm = _ffm()
        print("DIGESTS = {")
        for name in CASES:
            print('    "%s": "%s",' % (name, _digest(*_renumber(ffm, _build(ffm, name)))))
        print("}\nHINT_DIGESTS = {")
        print('    "centres_hint": "%s",' % _digest(_build(ffm, "centres_hint")["hint"]))
        print("}\nBAD_ADDR = {")
        for which in sorted(BAD_ADDR):
            print('    "%s": %r,' % (which, _bad_addr(ffm, which)))
        print("}")
