"""SURVEY 8(e) / VERDICT r1 item 5 on the device: the baffled steckler room and a randomly relabelled box, partitioned by the
product's RCB / graph-growing partitioners into 2 and 4 sub-domains, solved by the HIP library in its ghost-cell form
(ffm_ldu_create_ext + ffm_ldu_set_ghost_exchange + pair tags) -- one process per rank sharing cuda:0 through the host (gloo)
transport.  The assembled Amul equals the global operator (1e-14), the converged fields equal the serial oracle solve to 1e-10
at tolerance 1e-12 (block-Jacobi DIC / DILU differ from the serial preconditioner only in the iteration path)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import part_cases
from common import rel_l2, free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("meshName,partitioner,world,solver,precond,asym", [
    ("steckler", "rcb", 4, "PCG", "DIC", 0.0), ("steckler", "graph", 2, "PBICGSTAB", "DILU", 0.3),
    ("dag_random", "graph", 4, "PCG", "DIC", 0.0), ("dag_random", "rcb", 2, "SMOOTH", "SYMGS", 0.3)])
def test_partitioned_mesh_on_the_device(O, ffm, ctx, meshName, partitioner, world, solver, precond, asym):
    N, l, u, centres, diag, up, lo, source = part_cases.build(O, meshName, asym)
    Ao = O.Ldu(N, l, u).set_coeffs(diag, up, lo)
    ref, perf = Ao.solve(getattr(O, solver), getattr(O, precond), np.zeros(N), source, tolerance=1e-12, maxIter=1000)
    yref = Ao.amul(O.hash_u(0xF4, np.arange(N)))
    port = free_port()
    with tempfile.TemporaryDirectory() as tmp:
        procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "workers", "part_rank.py"), "gpu", str(r), str(world), str(port),
                                   meshName, partitioner, solver, precond, str(asym), tmp], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
                 for r in range(world)]
        try:
            outs = [p.communicate(timeout=120) for p in procs]
        finally:
            for p in procs:                      # a rank that failed leaves the others waiting in gloo: never leave them behind
                if p.poll() is None:
                    p.kill()
        assert [p.returncode for p in procs] == [0] * world, [o[1][-800:] for o in outs]
        parts = [np.load(os.path.join(tmp, "rank%d.npz" % r)) for r in range(world)]
        ys = [np.load(os.path.join(tmp, "amul%d.npy" % r)) for r in range(world)]
    assert len({int(p["nIter"]) for p in parts}) == 1
    full, y = np.empty(N), np.empty(N)
    for p, yy in zip(parts, ys):
        full[p["gcell"]] = p["psi"]; y[p["gcell"]] = yy
    assert rel_l2(y, yref) < 1e-14
    assert rel_l2(full, ref) < (1e-10 if solver != "SMOOTH" else 1e-9)


def _run_ranks(mode, world, port, args, tmp, env=None):
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "workers", "part_rank.py"), mode, str(r), str(world), str(port)] + args + [tmp],
                              env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE) for r in range(world)]
    outs = [None] * world
    import time
    t0 = time.time()
    try:
        # a rank that fails leaves the others waiting in a collective: stop all of them as soon as one has exited with an error
        while any(p.poll() is None for p in procs):
            if any(p.poll() not in (None, 0) for p in procs) or time.time() - t0 > 120:
                break
            time.sleep(0.2)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for r, p in enumerate(procs):
            outs[r] = p.communicate()[1]
    codes = [p.returncode for p in procs]
    assert codes == [0] * world, (codes, [o[-700:] for o, c in zip(outs, codes) if c not in (0, -9)] or [o[-300:] for o in outs])
    return [dict(np.load(os.path.join(tmp, "rank%d.npz" % r))) for r in range(world)]


@pytest.mark.parametrize("meshName,precond", [("dag_random", "SYMGS"), ("dag_random", "GS"), ("steckler", "SYMGS")])
def test_every_smoother_sweep_sees_the_neighbour_ranks_current_values(O, ffm, ctx, meshName, precond):
    """ONE call of the (sym)GaussSeidel smoother with nSweeps = 2 from a non-zero start on a decomposed, level-scheduled matrix,
    psi after the call against the oracle's smoother with OpenFOAM's processor patches on the same decomposition (interfaces
    updated before every sweep, GaussSeidelSmoother.C).  Not a converged answer: a second sweep that used the ghost values of the
    first would be off by the size of one sweep's update (~1e-2), not by rounding."""
    world = 2
    args = [meshName, "graph", "GS2", precond, "0.3"]
    port = free_port()
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        ref = _run_ranks("oracle", world, port, args, t1, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
        got = _run_ranks("gpu", world, port + 1, args, t2)
    N = sum(len(p["gcell"]) for p in ref)
    a, b = np.empty(N), np.empty(N)
    for p in ref:
        a[p["gcell"]] = p["psi"]
    for p in got:
        b[p["gcell"]] = p["psi"]
    assert all(int(p["nGhost"]) > 0 for p in got)
    # one sweep moves psi by O(1e-1) of its size here; the two codes differ in the place of the ghost terms in a row's sum only
    start = O.hash_u(0xF5, np.arange(N))
    assert rel_l2(a, start) > 1e-2
    assert rel_l2(b, a) < 1e-13, rel_l2(b, a)


@pytest.mark.parametrize("meshName,world,precond,asym,part", [
    pytest.param("steckler", 2, "GS", 0.0, "rcb", id="steckler-2-GS-0.0"), pytest.param("steckler", 4, "GS", 0.0, "rcb", id="steckler-4-GS-0.0"),
    pytest.param("dag_random", 2, "DILU", 0.3, "rcb", id="dag_random-2-DILU-0.3"), pytest.param("steckler", 4, "SYMGS", 0.0, "rcb", id="steckler-4-SYMGS-0.0"),
    pytest.param("dag_random", 4, "DIC", 0.0, "rcb", id="dag_random-4-DIC-0.0"),
    pytest.param("dag_random", 2, "DILU", 0.3, "graph", id="dag_random-2-DILU-0.3-graph"), pytest.param("dag_random", 4, "DIC", 0.0, "graph", id="dag_random-4-DIC-0.0-graph")])
def test_gamg_on_a_decomposed_mesh(O, ffm, ctx, meshName, world, precond, asym, part):
    """GAMG over 2 and 4 ranks the way OpenFOAM runs it without a processorAgglomerator (BASELINE config 5: p_rgh by GAMG + GaussSeidel on
    four ranks, cases/wallFireSpread2D/system/fvSolution:36-60): every rank agglomerates its own cells, the processor interfaces are
    agglomerated with them, smoothers refresh the interfaces before every sweep, the coarsest level is solved over all ranks, the
    stopping rule and the scale factors are global.  The device (ghost-cell form, ffm_gamg_* on ffm_ldu_create_ext matrices, ranks
    sharing cuda:0 through the host transport) against the oracle in OpenFOAM's processor-patch form (oracle/gamg_multi.py) on the same
    decomposition: the same hierarchy (cells per level on every rank), the same number of V-cycles, the same residuals and solution
    (the two forms add a row's interface terms at different places of its sum: rounding level)."""
    args = [meshName, part, "GAMG", precond, str(asym)]           # (rcb: coordinate bisection, box-like sub-domains; graph: sub-domains of any shape, wider coarse rows)
    port = free_port()
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        ref = _run_ranks("oracle", world, port, args, t1, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
        got = _run_ranks("gpu", world, port + 1, args, t2)
    assert len({int(p["nIter"]) for p in got}) == 1 and len({int(p["nLevels"]) for p in got}) == 1
    for r in range(world):
        assert int(got[r]["nLevels"]) == int(ref[r]["nLevels"]) and int(ref[r]["nLevels"]) >= 3
        assert np.array_equal(got[r]["levelCells"], ref[r]["levelCells"]), (r, got[r]["levelCells"], ref[r]["levelCells"])
        assert int(got[r]["nIter"]) == int(ref[r]["nIter"]) and 2 <= int(ref[r]["nIter"]) < 60, (int(got[r]["nIter"]), int(ref[r]["nIter"]))
        assert abs(float(got[r]["initialResidual"]) - float(ref[r]["initialResidual"])) <= 1e-10
        assert abs(float(got[r]["finalResidual"]) - float(ref[r]["finalResidual"])) <= 1e-6 * float(ref[r]["finalResidual"]) + 1e-14
    N = sum(len(p["gcell"]) for p in ref)
    a, b = np.empty(N), np.empty(N)
    for p in ref:
        a[p["gcell"]] = p["psi"]
    for p in got:
        b[p["gcell"]] = p["psi"]
    assert rel_l2(b, a) < 1e-9, rel_l2(b, a)
