"""Meshes whose GAMG hierarchy has coarse rows wider than a fine cell's (a helper, not a test): shared by tests/test_gamg_levels_cpu.py
and tests/test_gamg_wide_rows_gpu.py.

Pair agglomeration widens rows: a coarse cell of a 3-D mesh settles at 20 - 25 neighbours, and how they split into upper and lower faces
is an accident of the coarse numbering.  On the merged meshes of tests/merged_mesh.py and on randomly relabelled boxes some coarse cell
then owns more than 16 faces towards owned cells, which the packed lower entries of the row layout hold only with a five-bit slot field
(csrc/ffm_ldu_analysis.cpp: check_layout_limits).  A hex box and the steckler room with their real face areas stay blocky and never get
there.

ROWS: name -> (mesh, weights, cells, widths).  `widths` lists (max owned upper, max lower) faces of a cell for every level of the oracle's
hierarchy (oracle/gamg.py: Agglomeration), level 0 first.  The widths were computed once from the oracle and are asserted by both tests, so that a change of a mesh helper cannot
quietly turn a wide case into a narrow one.  WIDE names the rows with a level of more than 16 owned upper faces."""
import numpy as np

import common

ROWS = {
    "w32multi-Sf": ("w32multi", "Sf", 211, [(4, 24), (17, 19), (17, 17), (15, 13), (10, 8)]),
    "w32multi-hashed": ("w32multi", "hashed", 211, [(4, 24), (17, 10), (15, 17), (9, 12), (6, 7)]),
    "w32l30-hashed": ("w32l30", "hashed", 174, [(4, 30), (22, 8), (12, 13), (8, 9)]),
    "w32l30-Sf": ("w32l30", "Sf", 174, [(4, 30), (4, 23), (6, 23), (6, 9)]),
    "w16u14-hashed": ("w16u14", "hashed", 118, [(14, 4), (16, 7), (12, 8), (6, 8)]),
    "dag12s3-hashed": ("dag12s3", "hashed", 1728, [(6, 6), (14, 13), (15, 17), (20, 14), (15, 15), (16, 13), (10, 12)]),
    "dag14s5-hashed": ("dag14s5", "hashed", 2744, [(6, 6), (16, 12), (16, 17), (20, 16), (17, 17), (16, 13), (10, 12), (6, 9)]),
    "dag30s9-hashed": ("dag30s9", "hashed", 27000, [(6, 6), (14, 15), (19, 21), (22, 19), (23, 20), (19, 21), (19, 21), (19, 18), (17, 17), (14, 13), (14, 9)]),
    "steckler-Sf": ("steckler", "Sf", 9000, [(3, 3), (4, 7), (6, 7), (8, 9), (8, 8), (8, 12), (10, 10), (9, 10), (10, 9), (8, 7)]),
    "steckler-hashed": ("steckler", "hashed", 9000, [(3, 3), (8, 9), (11, 11), (13, 13), (14, 15), (13, 15), (13, 15), (10, 12), (9, 8), (7, 8)]),
}
SMALL = list(ROWS)[:7]               # at most 2744 cells: the rows of the GPU test
WIDE = ["w32multi-Sf", "w32multi-hashed", "w32l30-hashed", "dag12s3-hashed", "dag14s5-hashed", "dag30s9-hashed"]

_cache = {}


def build(O, name):
    """(N, l, u, face weights, Agglomeration) of a row: computed once, never changed"""
    if name in _cache:
        return _cache[name]
    from oracle import gamg
    mesh, weights, cells, _ = ROWS[name]
    Sf = None
    if mesh.startswith("dag"):
        n, seed = (int(x) for x in mesh[3:].split("s"))
        N, l, u = common.random_dag_mesh(O, n, seed=seed)
    elif mesh == "steckler":
        from oracle import steckler
        m = steckler.build_mesh()
        N, l, u, Sf = m.nCells, m.l.astype(np.int32), m.u.astype(np.int32), m.Sf
    else:
        import merged_mesh as MM
        m = MM.case(mesh)
        N, l, u, Sf = m.nCells, m.l.astype(np.int32), m.u.astype(np.int32), m.Sf
    assert N == cells
    w = gamg.face_area_pair_weights(Sf) if weights == "Sf" else 0.5 + O.hash_u(0x5F, np.arange(len(l)))
    _cache[name] = (N, l, u, w, gamg.Agglomeration(N, l, u, w))
    return _cache[name]


def level_widths(agg):
    """[(max owned upper, max lower) faces of a cell] per level of the hierarchy (one rank: every face is towards an owned cell)"""
    return [(int(np.bincount(agg.l[k]).max()), int(np.bincount(agg.u[k]).max())) for k in range(agg.nLevels + 1)]


def check_widths(name, agg):
    """the row's widths still hold"""
    want, got = ROWS[name][3], level_widths(agg)
    assert got == want, (name, got)
    assert (max(a for a, _ in got) > 16) == (name in WIDE), (name, got)
