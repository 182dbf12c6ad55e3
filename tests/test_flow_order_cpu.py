"""The flow order of an upwind ray matrix (csrc/ffm_rays.cpp: ffm_flow_levels, host code): on every test mesh -- the polyhedral
meshes of tests/merged_mesh.py, the boxes of tests/test_fvdom_gpu.py, the steckler room with its baffles -- and for the 32 rays of
nPhi 2, nTheta 4 plus the axis direction (1,0,0), the order is a permutation under which the matrix is triangular, level-major with
the level count of Kahn's algorithm restated here; cyclic matrices are refused."""
import numpy as np
import pytest

import merged_mesh
import ray_matrix as R

MESHES = sorted(merged_mesh.CASES) + ["box7x8x6", "box14x18x1", "steckler"]


@pytest.mark.parametrize("name", MESHES)
def test_order_makes_every_ray_matrix_triangular(ffm, name):
    m = R.mesh(name)
    N = m.nCells
    l, u = np.asarray(m.l, np.int64), np.asarray(m.u, np.int64)
    for tag, d, omega in R.directions():
        _, upper, lower = R.ray_matrix(m, d, omega)
        assert not np.any((upper != 0) & (lower != 0))
        if tag == "x" and name != "steckler" and name.startswith("box"):
            assert np.any((upper == 0) & (lower == 0))                 # the transverse faces: no edges
        order, nLevels = ffm.flow_levels(N, l, u, upper, lower)
        assert sorted(order.tolist()) == list(range(N)), (name, tag)
        pos = np.empty(N, np.int64); pos[order] = np.arange(N)
        src, dst = R.edges(l, u, upper, lower)
        assert np.all(pos[src] < pos[dst]), (name, tag)
        lev, k, acyclic = R.kahn_levels(N, src, dst)
        assert acyclic and nLevels == k, (name, tag, nLevels, k)
        along = lev[order]
        assert np.all(np.diff(along) >= 0), (name, tag)
        same = np.diff(along) == 0
        assert np.all(np.diff(order)[same] > 0), (name, tag)          # ascending cell index inside a level


def test_a_ring_is_refused(ffm):
    # a -> b -> c -> a: row 1 needs cell 0, row 2 needs cell 1, row 0 needs cell 2
    l, u = np.array([0, 0, 1]), np.array([1, 2, 2])
    lower, upper = np.array([-1.0, 0.0, -1.0]), np.array([0.0, -1.0, 0.0])
    with pytest.raises(ffm.FfmError, match=r"\(-5\).*cycle"):
        ffm.flow_levels(3, l, u, upper, lower)
    order, n = ffm.flow_levels(3, l, u, np.zeros(3), lower)            # without the closing edge: a chain
    assert order.tolist() == [0, 1, 2] and n == 3


def test_a_face_with_both_coefficients_is_refused(ffm):
    l, u = np.array([0, 1]), np.array([1, 2])
    with pytest.raises(ffm.FfmError, match=r"\(-5\)"):
        ffm.flow_levels(3, l, u, np.array([-1.0, 0.0]), np.array([-0.5, -1.0]))
