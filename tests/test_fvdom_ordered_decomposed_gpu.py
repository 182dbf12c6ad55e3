"""The fvDOM handle with setOrderedSolves(true) on a DECOMPOSED mesh (include/fireFoamHandles.H; every ray by fvScalarMatrix::
solveOrdered, on a sub-domain the staged exact solve of ffm_solve_ordered_staged_d) through b1_fvdom_ordered of examples/b1_demo.C.
Mesh, inputs and partitions of tests/test_foam_layer_decomposed_gpu.py::test_fvdom_with_reflecting_walls_on_a_decomposed_mesh: the
10 x 9 x 8 box, foam_case.fvdom_inputs (wall emissivities < 1: the rays are coupled through the walls of every rank), 16 rays, three
iterations per call, two calls, (2, rcb) and (4, graph), one process per rank sharing cuda:0 over the host / gloo transport
(tests/workers/fvdom_ordered_rank.py); div(Ji,Ii_h) upwind and linearUpwind.  I of all rays, G and qin against the single-rank
b1_fvdom_ordered run of this process within 1e-8, the bound of that test; every ray solve of every call is logged as `ordered` with one
iteration, and the stage count is printed once."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import foam_case
import fvdom_ordered_case
from common import rel_l2, free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (10, 9, 8)
BOUND = 1e-8
SCHEMES = {"upwind": 0, "linearUpwind": 5}
_single, _runs = {}, {}


def single(ffm, ctx, scheme):
    """the single-rank run of the same code (tests/test_fvdom_ordered_gpu.py compares it with the oracle): once per scheme"""
    if scheme not in _single:
        from oracle import plume
        m = plume.make_mesh(SHAPE, h=0.1)
        T, Tb, E, emis = foam_case.fvdom_inputs(m)
        res = fvdom_ordered_case.run(ffm, ctx, m, T, Tb, E, emis, scheme=scheme, quiet=True)
        assert np.array_equal(res[1], np.arange(m.nCells)) and res[2] == [3, 3] and res[4] == 1
        _single[scheme] = (m, res)
    return _single[scheme]


def decomposed(world, partitioner):
    """one launch of the workers per partition for the whole module: (the ranks' result files, their logs)"""
    if (world, partitioner) not in _runs:
        port = free_port()
        with tempfile.TemporaryDirectory() as tmp:
            procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "workers", "fvdom_ordered_rank.py"), str(r), str(world), str(port)]
                                      + [str(v) for v in SHAPE] + [partitioner, tmp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                     for r in range(world)]
            try:
                outs = [p.communicate(timeout=120) for p in procs]
            finally:
                for p in procs:                      # never leave a rank behind (the others wait for it in gloo)
                    if p.poll() is None:
                        p.kill()
            assert [p.returncode for p in procs] == [0] * world, [o[1][-1500:] for o in outs]
            parts = [dict(np.load(os.path.join(tmp, "rank%d.npz" % r))) for r in range(world)]
        _runs[(world, partitioner)] = (parts, [o[0] for o in outs])
    return _runs[(world, partitioner)]


@pytest.mark.parametrize("schemeName", sorted(SCHEMES))
@pytest.mark.parametrize("world,partitioner", [(2, "rcb"), (4, "graph")])
def test_fields_equal_the_single_rank_ordered_run(ffm, ctx, world, partitioner, schemeName):
    scheme = SCHEMES[schemeName]
    m, ((I1, G1, q1), _, its1, nSolves1, _) = single(ffm, ctx, scheme)
    parts, _ = decomposed(world, partitioner)
    assert sorted(np.concatenate([p["cells"] for p in parts]).tolist()) == list(range(m.nCells))
    assert all(p["its_%d" % scheme].tolist() == its1 for p in parts) and all(int(p["nGhost"]) > 0 for p in parts)
    assert all(int(p["nSolves_%d" % scheme]) == nSolves1 and int(p["maxIts_%d" % scheme]) == 1 for p in parts)
    I = np.full_like(I1, np.nan); G = np.full_like(G1, np.nan)
    for p in parts:
        I[:, p["cells"]] = p["I_%d" % scheme]; G[p["cells"]] = p["G_%d" % scheme]
    errI = max(rel_l2(I[i], I1[i]) for i in range(I.shape[0]))
    errQ = 0.0
    for pt in m.patches:
        full = np.full(pt.size, np.nan)
        for p in parts:
            full[p["pos_" + pt.name]] = p["qin_%d_%s" % (scheme, pt.name)]
        errQ = max(errQ, np.abs(full - q1[pt.name][1]).max() / max(np.abs(q1[pt.name][1]).max(), 1e-300))
    print("%s into %d, %s: I %.3e  G %.3e  qin %.3e" % (partitioner, world, schemeName, errI, rel_l2(G, G1), errQ))
    assert errI < BOUND and rel_l2(G, G1) < BOUND and errQ <= BOUND


@pytest.mark.parametrize("world,partitioner", [(2, "rcb"), (4, "graph")])
def test_every_ray_solve_is_logged_as_ordered_with_one_iteration(ffm, ctx, world, partitioner):
    parts, logs = decomposed(world, partitioner)
    stages = set()
    for r, log in enumerate(logs):
        runs = log.split("== scheme ")[1:]
        assert [x.split("\n", 1)[0] for x in runs] == ["0", "5"], r
        for scheme, text in zip((0, 5), runs):
            solves = [ln for ln in text.splitlines() if "Solving for" in ln]
            assert len(solves) == 16 * 3 * 2, (r, scheme, len(solves))          # 16 rays, three iterations per call, two calls
            assert all(re.match(r"ordered:  Solving for ILambda_\d+_0, .*, No Iterations 1$", ln) for ln in solves), (r, scheme)
            said = re.findall(r"^fvDOM: ordered ray solves, up to (\d+) stages per ray$", text, flags=re.M)
            assert len(said) == 1 and int(said[0]) >= 2, (r, scheme, said)      # once, after the first correct(); a cut mesh has two stages at least
            stages.add((scheme, int(said[0])))
    assert len(stages) == 2                                                      # the same count on every rank
