"""The stages of an upwind ray matrix on a decomposed mesh (csrc/ffm_rays.cpp: ffm_flow_stages, host code): called per simulated
rank in one process on the sub-domains of the product's partitioners (decompose.SubDomain; rcb and graph growing into 2 and 4),
with the ghost stages carried between the "ranks" in numpy until nothing changes -- the fixpoint ffm_flow_order_create_staged
takes over the communicator.  The stages equal the restatement on the merged mesh (tests/ray_stages.py: the longest path counting
rank crossings), every rank's order is a permutation, stage-major, with every non-zero owned column before its row.  A ring
through two ranks that neither sees locally exceeds the ghost-count bound within a few rounds; a cycle among a rank's own cells is
refused by the call itself.  Without ghost cells ffm_flow_stages is ffm_flow_levels: both are one Kahn pass."""
import numpy as np
import pytest

import ray_matrix as R
import ray_stages as S

MESHES = ["box7x8x6", "box14x18x1", "steckler", "w16u14", "w32multi"]
PARTITIONS = [("rcb", 2), ("rcb", 4), ("graph", 2), ("graph", 4)]


@pytest.mark.parametrize("partitioner,world", PARTITIONS)
@pytest.mark.parametrize("name", MESHES)
def test_stages_equal_the_merged_restatement(ffm, name, partitioner, world):
    m = R.mesh(name)
    N = m.nCells
    l, u = np.asarray(m.l, np.int64), np.asarray(m.u, np.int64)
    part = ffm.decompose.partition_rcb(m.C, world) if partitioner == "rcb" else ffm.decompose.partition_graph(N, l, u, world)
    subs = [ffm.decompose.SubDomain(N, l, u, part, world, r) for r in range(world)]
    assert all(s.nGhost > 0 for s in subs)
    counts = []
    for tag, d, omega in R.five_directions():
        diag, upper, lower = R.ray_matrix(m, d, omega)
        want = S.merged_stages(N, l, u, upper, lower, part)
        out, rounds = S.fixpoint(ffm, subs, [s.coeffs(diag, upper, lower)[1:] for s in subs])
        assert rounds <= want.max() + 2, (name, tag, rounds, want.max())          # stages only grow: at most (stage count + 1) rounds
        for s, (stage, order, nLevels), (_, up, lo) in zip(subs, out, (s.coeffs(diag, upper, lower) for s in subs)):
            n = s.nOwned
            assert np.array_equal(stage, want[s.gcell[:n]]), (name, partitioner, world, tag, s.rank)
            assert sorted(order.tolist()) == list(range(n)), (name, tag, s.rank)
            assert np.all(np.diff(stage[order]) >= 0), (name, tag, s.rank)      # stage-major
            own = s.u < n                                                         # faces between two owned cells
            src, dst = R.edges(s.l[own].astype(np.int64), s.u[own].astype(np.int64), up[own], lo[own])
            pos = np.empty(n, np.int64); pos[order] = np.arange(n)
            assert np.all(pos[src] < pos[dst]), (name, tag, s.rank)
            lev, k, acyclic = R.kahn_levels(n, src, dst)
            assert acyclic and nLevels == k, (name, tag, s.rank, nLevels, k)
            key = stage[order].astype(np.int64) * k + lev[order]                  # level-major inside a stage, ascending cells inside a level
            assert np.all(np.diff(key) >= 0) and np.all(np.diff(order)[np.diff(key) == 0] > 0), (name, tag, s.rank)
        counts.append(int(want.max()) + 1)
    print("%s %s into %d: stages of the five directions %r" % (name, partitioner, world, counts))


@pytest.mark.parametrize("name", MESHES + ["w8", "w32l30"])
def test_without_ghost_cells_the_stages_are_the_levels(ffm, name):
    m = R.mesh(name)
    N = m.nCells
    l, u = np.asarray(m.l, np.int64), np.asarray(m.u, np.int64)
    for tag, d, omega in R.five_directions():
        _, upper, lower = R.ray_matrix(m, d, omega)
        want, nLevels = ffm.flow_levels(N, l, u, upper, lower)
        stage, order, n = ffm.flow_stages(N, 0, l, u, upper, lower, np.zeros(0, np.int32))
        assert not stage.any(), (name, tag)
        assert np.array_equal(order, want), (name, tag)
        assert n == nLevels, (name, tag)


def test_a_ring_through_two_ranks_exceeds_the_ghost_count_bound(ffm):
    # cells 0 -> 1 | 2 -> 3 with the cut edges 1 -> 2 and 3 -> 0: acyclic on either rank, a cycle over both
    l, u = np.array([0, 0, 1, 2]), np.array([1, 3, 2, 3])
    lower, upper = np.array([-1.0, 0.0, -1.0, -1.0]), np.array([0.0, -1.0, 0.0, 0.0])     # face (0,3): row 0 needs cell 3
    part = np.array([0, 0, 1, 1], np.int32)
    subs = [ffm.decompose.SubDomain(4, l, u, part, 2, r) for r in range(2)]
    diag = np.ones(4)
    coeffs = [s.coeffs(diag, upper, lower)[1:] for s in subs]
    for s, (up, lo) in zip(subs, coeffs):                                        # every rank alone: fine
        stage, order, _ = ffm.flow_stages(s.nOwned, s.nGhost, s.l, s.u, up, lo, np.zeros(s.nGhost, np.int32))
        assert sorted(order.tolist()) == [0, 1]
    total = sum(s.nGhost for s in subs)
    out, rounds = S.fixpoint(ffm, subs, coeffs, maxRounds=total + 3)
    assert out is None and rounds <= total + 2, rounds
    # without the closing edge: a chain through both ranks, two stages
    out, rounds = S.fixpoint(ffm, subs, [s.coeffs(diag, np.zeros(4), lower)[1:] for s in subs])
    assert [o[0].tolist() for o in out] == [[0, 0], [1, 1]] and rounds <= 3


def test_a_cycle_among_the_owned_cells_is_refused_by_the_call(ffm):
    # a -> b -> c -> a among three owned cells, one ghost cell feeding a
    l, u = np.array([0, 0, 0, 1]), np.array([1, 2, 3, 2])
    lower, upper = np.array([-1.0, 0.0, 0.0, -1.0]), np.array([0.0, -1.0, -1.0, 0.0])
    with pytest.raises(ffm.FfmError, match=r"\(-5\).*cycle"):
        ffm.flow_stages(3, 1, l, u, upper, lower, np.array([4], np.int32))
    stage, order, n = ffm.flow_stages(3, 1, l, u, np.array([0.0, 0.0, -1.0, 0.0]), lower, np.array([4], np.int32))
    assert stage.tolist() == [5, 5, 5] and order.tolist() == [0, 1, 2] and n == 3
    with pytest.raises(ffm.FfmError, match=r"\(-2\)|\(-1\)"):
        ffm.flow_stages(3, 1, l, np.array([1, 2, 4, 2]), upper, lower, np.array([0], np.int32))
