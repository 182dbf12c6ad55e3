"""The staged flow-ordered solve on decomposed meshes (csrc/ffm_solve.hip: ffm_flow_order_create_staged,
ffm_solve_ordered_staged_d) on upwind ray matrices (tests/ray_matrix.py), partitions of the product's partitioners, one process
per rank sharing cuda:0 over the host / gloo transport (tests/workers/ordered_rank.py): the 7 x 8 x 6 box (336 cells), w32multi
(211 cells, rows of up to 24 faces, a cyclic rank graph under RCB) and the steckler room (9000 cells, baffles), (2, rcb) and
(4, graph), the five directions of ray_matrix.five_directions(), hashed sources, NaN-laced start values.

(a) the gathered psi against the serial forward substitution of the MERGED matrix: rel-L2 <= 1e-8, the project's parity bound
    (as tests/test_plume_rays_decomposed_gpu.py).  Not bitwise: a cut face whose global owner is the ghost
    cell is a local upper face, so a row subtracts its terms in another order than the merged row.  Measured on an MI355X: at most
    1.4e-16 over all cases and directions.
(b) bitwise: every rank's rows recomputed in numpy from the ghost entries psi holds after the solve, stage by stage in an order of
    ffm_flow_stages, lower then upper faces in the rank's face order -- by induction over the stages the whole algorithm.
(c) nIterations 1, converged 1; the stage count is the same on all ranks and the merged restatement's (tests/ray_stages.py); the
    exchange callback is called the same number of times on every rank during a solve, at most nStages - 1 plus the two of the
    residuals' Amuls.
(d) only rank 0 holds the opposite ray's coefficients: every rank's call fails with (-5) before any exchange, every rank's psi is bit
    for bit its start value, all workers exit 0; with the right coefficients back the same order solves again, bitwise as before.
(e) the box under (2, rcb): the rank below the cut has a matrix whose widest row is in the W = 3 bucket (the hex instantiation of the
    kernels; above the cut the flipped cut faces make a fourth upper face), and 42 ghost cells -- no multiple of 64."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import ray_matrix as R
from common import rel_l2, free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MESHES = ["box7x8x6", "w32multi", "steckler"]
PARTITIONS = [(2, "rcb"), (4, "graph")]
CASES = [(name, world, partitioner) for name in MESHES for world, partitioner in PARTITIONS]
BOUND = 1e-8
_RUNS, _MERGED = {}, {}


def merged(ffm, O, name):
    """the serial solutions of the five rays on the merged mesh: computed once, never changed"""
    if name not in _MERGED:
        m = R.mesh(name)
        N = m.nCells
        l, u = np.asarray(m.l, np.int64), np.asarray(m.u, np.int64)
        want = []
        for i, (tag, d, omega) in enumerate(R.five_directions()):
            diag, upper, lower = R.ray_matrix(m, d, omega)
            order, _ = ffm.flow_levels(N, l, u, upper, lower)
            want.append(R.forward_substitution(N, l, u, diag, upper, lower, 0.5 + O.hash_u(40 + i, np.arange(N)), order))
            assert np.isfinite(want[-1]).all()
        _MERGED[name] = (N, want)
    return _MERGED[name]


def run(name, world, partitioner):
    """one launch of the workers per case for the whole module: the ranks' result files"""
    key = (name, world, partitioner)
    if key in _RUNS:
        return _RUNS[key]
    port = free_port()
    with tempfile.TemporaryDirectory() as tmp:
        procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "workers", "ordered_rank.py"), str(r), str(world), str(port), name, partitioner, tmp],
                                  stdout=subprocess.DEVNULL, stderr=subprocess.PIPE) for r in range(world)]
        try:
            outs = [p.communicate(timeout=120) for p in procs]
        finally:
            for p in procs:                      # never leave a rank behind (the others wait for it in gloo)
                if p.poll() is None:
                    p.kill()
        assert [p.returncode for p in procs] == [0] * world, [o[1][-1500:] for o in outs]
        _RUNS[key] = [dict(np.load(os.path.join(tmp, "rank%d.npz" % r))) for r in range(world)]
    return _RUNS[key]


@pytest.mark.parametrize("name,world,partitioner", CASES)
def test_gathered_psi_against_the_merged_forward_substitution(O, ffm, ctx, name, world, partitioner):
    N, want = merged(ffm, O, name)
    parts = run(name, world, partitioner)
    assert sorted(np.concatenate([p["gcell"] for p in parts]).tolist()) == list(range(N)) and all(int(p["nGhost"]) > 0 for p in parts)
    for i in range(5):
        psi = np.full(N, np.nan)
        for p in parts:
            psi[p["gcell"]] = p["psi%d" % i]
        e = rel_l2(psi, want[i])
        print("%s %s into %d, direction %d: rel-L2 against the merged solve %.3e (%d stages)" % (name, partitioner, world, i, e, int(parts[0]["nStages%d" % i])))
        assert e <= BOUND, (name, world, partitioner, i, e)


@pytest.mark.parametrize("name,world,partitioner", CASES)
def test_every_rank_is_bitwise_its_own_rows_recomputed(ctx, name, world, partitioner):
    for r, p in enumerate(run(name, world, partitioner)):
        assert [int(p["bitwise%d" % i]) for i in range(5)] == [1] * 5, (name, world, partitioner, r)


@pytest.mark.parametrize("name,world,partitioner", CASES)
def test_perf_record_stage_counts_and_exchanges(ctx, name, world, partitioner):
    parts = run(name, world, partitioner)
    for i in range(5):
        S = int(parts[0]["nStages%d" % i])
        for r, p in enumerate(parts):
            assert int(p["nIter%d" % i]) == 1 and int(p["conv%d" % i]) == 1, (name, i, r)
            assert int(p["nStages%d" % i]) == S == int(p["wantStages%d" % i]) and int(p["stagesMatch%d" % i]) == 1, (name, i, r)
            # sums over all ranks: the same record everywhere (NaN where the NaN-laced start value makes OpenFOAM's normFactor NaN)
            assert np.array_equal(p["res%d" % i], parts[0]["res%d" % i], equal_nan=True), (name, i, r)
        ex = {int(p["exchanges%d" % i]) for p in parts}
        assert len(ex) == 1 and ex.pop() <= S - 1 + 2, (name, i, S, [int(p["exchanges%d" % i]) for p in parts])


@pytest.mark.parametrize("name,world,partitioner", CASES)
def test_all_ranks_refuse_together_when_one_holds_another_matrix(ctx, name, world, partitioner):
    for r, p in enumerate(run(name, world, partitioner)):
        assert int(p["refused"]) == 1 and int(p["untouched"]) == 1 and int(p["refusedExchanges"]) == 0, (name, r)
        assert int(p["conv_after"]) == 1 and int(p["bitwise_after"]) == 1, (name, r)


def test_the_box_runs_the_hex_width_with_a_ragged_ghost_count(ctx):
    parts = run("box7x8x6", 2, "rcb")
    assert min(int(p["maxW"]) for p in parts) <= 3                  # the W = 3 instantiation of the check and the stage kernel
    assert all(int(p["nGhost"]) % 64 != 0 for p in parts)
