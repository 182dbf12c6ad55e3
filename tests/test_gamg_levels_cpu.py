"""The row layout's limits against the coarse levels GAMG really makes, without a GPU: ffm_ldu_check_layout (host code, the analysis and
the layout of ffm_ldu_create_ext) must accept every level of the oracle's hierarchy (oracle/gamg.py: Agglomeration, which the GPU tests
assert equal to the library's level by level) on the meshes of tests/gamg_wide_cases.py -- merged polyhedral meshes and relabelled boxes
whose coarse cells own 17 to 23 faces towards owned cells -- and must go on refusing what the layout cannot hold, with a message that
says why: more than 32 faces on one side, 2^27 cells, and 2^26 cells where a row needs the five-bit slot field."""
import re

import numpy as np
import pytest

import gamg_wide_cases as GW
import merged_mesh as MM

UNSUPPORTED = -5


@pytest.mark.parametrize("name", list(GW.ROWS))
def test_every_level_of_the_hierarchy_is_accepted(O, ffm, name):
    N, l, u, w, agg = GW.build(O, name)
    GW.check_widths(name, agg)
    assert agg.nLevels >= 3
    for lev in range(agg.nLevels + 1):
        assert ffm.check_layout(agg.nCells[lev], agg.l[lev], agg.u[lev]) == (0, ""), (name, lev)


def test_ghost_faces_do_not_count_towards_the_slot_field(ffm):
    """a row of 20 upper faces, 12 towards owned cells followed by 8 towards ghost cells (a coarse cell at a rank boundary), and the same
    row with 18 owned faces: both accepted"""
    for nOwnedFaces in (12, 18):
        nOwn = nOwnedFaces + 1
        l = np.zeros(20, np.int32); u = np.arange(1, 21, dtype=np.int32)
        assert ffm.check_layout(nOwn, l, u, nGhost=21 - nOwn) == (0, "")


@pytest.mark.parametrize("name,message", [("u34", r"a cell has 34 upper / \d+ lower faces \(> 32\): not supported by the sliced layout"),
                                          ("l34", r"a cell has \d+ upper / 34 lower faces \(> 32\): not supported by the sliced layout")])
def test_more_than_32_faces_on_a_side_are_refused(ffm, name, message):
    m = MM.case(name)
    assert MM.widths(m.l, m.u) == MM.REFUSED[name][4:6]
    rc, msg = ffm.check_layout(m.nCells, m.l, m.u)
    assert rc == UNSUPPORTED and re.fullmatch(message, msg), (rc, msg)


def test_an_index_range_of_2_to_the_27_is_refused(ffm):
    """the packed entries are int32: owner << 4 | slot"""
    l = np.array([0, 0, 1], np.int32); u = np.array([1, 2, 2], np.int32)
    assert ffm.check_layout(3, l, u) == (0, "")
    rc, msg = ffm.check_layout(2 ** 27, l, u)
    assert rc == UNSUPPORTED and msg == "mesh too large for int32 packed entries", (rc, msg)
    rc, msg = ffm.check_layout(3, l, u, nGhost=2 ** 27 - 3)
    assert rc == UNSUPPORTED and msg == "mesh too large for int32 packed entries", (rc, msg)


def test_a_wide_matrix_is_limited_to_2_to_the_26_cells(ffm):
    """owner << 5 | slot where a cell owns more than 16 faces towards owned cells: only such a matrix loses a bit of index range, and the
    message says so.  (The index range is made of ghost cells: 2^26 rows are refused before that for the size of their slices, wide or
    not.  Each call allocates the analysis' per-cell arrays, 2 GB for a second or two: the one slow test of this file.)"""
    N = 2 ** 26
    l = np.zeros(17, np.int32); u = np.arange(1, 18, dtype=np.int32)
    rc, msg = ffm.check_layout(18, l, u, nGhost=N - 18)
    assert rc == UNSUPPORTED and msg.startswith("mesh too large for int32 packed entries: a cell owns more than 16 faces towards owned cells") \
        and "2^26 cells" in msg, (rc, msg)
    assert ffm.check_layout(18, l[:16], u[:16], nGhost=N - 18) == (0, "")            # 16 owned upper faces: four bits, 2^27
    assert ffm.check_layout(17, l, u, nGhost=N - 17) == (0, "")                      # the 17th face is towards a ghost cell


def test_bad_arguments_are_refused(ffm):
    l = np.array([0], np.int32); u = np.array([1], np.int32)
    assert ffm.check_layout(-1, l, u)[0] == -1
    rc, msg = ffm.check_layout(1, l, u)                   # the neighbour is no cell
    assert rc != 0 and "face 0" in msg, (rc, msg)
