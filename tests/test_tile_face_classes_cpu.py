"""Host-only: the designed fluxes of tests/fv_edge_inputs.py (tiled_fields) reach every class of face of the tile walk (csrc/ffm_fused.hip:
k_mv_tile) on the boxes tests/test_tile_face_chains_gpu.py runs it on.  A box's tile hint makes 16 x 16 tiles in (y, z) with the columns
along x (csrc/ffm_ldu_analysis.cpp: pick_mode); a dependency level of a tile, i + y % 16 + z % 16, is one entry of at most 256 cells, and
32 entries are one run, which one workgroup walks with the entries e-1, e, e+1 in its LDS window."""
import numpy as np
import pytest

import fv_edge_inputs as E

TILE, RUN = 16, 32
BOXES = [(20, 18, 40), (40, 20, 18)]


def face_classes(m, phi):
    """(upwind, place of the other cell) of every internal face.  Upwind as the kernels decide it: the owner where phi > 0, else the
    neighbour, zero fluxes (which the neighbour evaluates) apart.  The other cell: in the same tile and run (the LDS window), in another
    tile (read from memory), or in the same tile across a run boundary (the halo entry that the workgroup stages beside its own run)"""
    i, j, k = m.ijk
    tile = (j // TILE) * 4096 + k // TILE
    run = (i + j % TILE + k % TILE) // RUN
    up = np.where(phi == 0, "zero", np.where(phi > 0, "owner", "neighbour"))
    same = tile[m.l] == tile[m.u]
    place = np.where(~same, "other tile", np.where(run[m.l] == run[m.u], "window", "run boundary"))
    return up, place


@pytest.mark.parametrize("n", BOXES, ids=lambda n: "x".join(map(str, n)))
def test_every_class_of_face_is_reached(n):
    from oracle import plume
    m = plume.make_mesh(n, h=E.H)
    i, j, k = m.ijk
    assert np.array_equal(np.arange(m.nCells), i + n[0] * (j + n[1] * k))          # x runs fastest: the order the hint is taken from
    levels = (i + j % TILE + k % TILE)[(j < TILE) & (k < TILE)].max() + 1
    assert levels == n[0] + 2 * TILE - 2 and levels > RUN                            # a full tile has more than one run
    up, place = face_classes(m, E.tiled_fields(m, 1)["phi"])
    for a in ("owner", "neighbour", "zero"):
        for b in ("window", "other tile", "run boundary"):
            assert ((up == a) & (place == b)).any(), (a, b)
