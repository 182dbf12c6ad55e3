"""Direction-ordered fvDOM ray solves across block boundaries (ffm_plume_set_radiation_ordering 1): on a decomposed box the ranks
walk the ticks of ffm_ray_schedule, a rank solves a ray once its upstream neighbours' intensities sit in its ghost cells -- the
ghost inflow goes to the source, the rest is the one-block triangular system, solved exactly on the rank's own rows -- and every
tick ends with one ghost exchange.  2 and 4 ranks (one process each, sharing cuda:0 through the host / gloo transport) run the
12 x 16 x 12 plume with the rays on in every step: one step, then a second one with the absorption / emission model coupled
into h.  All runs (the references too) with FFM_PLUME_TIGHT, as tests/test_plume_decomposed_gpu.py: the non-ray solves then
differ between a decomposed and a single-rank run by 1e-13, not by their stopping tolerances.

Measured on an MI355X (rel-L2; bound 1e-8, the parity bound of BASELINE.md section 2): G and the 32 rays over both steps
agree with the single-rank ordered run to 1.2e-15 and with the oracle to 6.1e-11 on all three grids (DESIGN.md row f / N1)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from common import rel_l2, free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GLOB = (12, 16, 12)
GRIDS = [(2, 1, 1), (1, 1, 2), (2, 2, 1)]          # 2 x 2 x 1: stages 0, 1, 1, 2
FIELDS = ["T", "p_rgh", "Ux", "Uy", "Uz", "O2", "C3H8", "CO2", "H2O"]
RAYS = ["I%d" % i for i in range(32)]
BOUND = 1e-8

# I<i> iteration counts of ordering 0 (every ray a block-Jacobi PBiCGStab + DILU solve over all ranks) on these grids WITH
# FFM_PLUME_TIGHT, i.e. every solve to 1e-13 as in all runs of this file -- not the counts of the default 1e-4 tolerance -- step 1 and step 2, rays 0 .. 31: recorded from a run of this worker on commit cbdeb84 ("Fuse the step's leftover
# passes; swap old-time buffers"), the parent of the commit that added the staged sweep
MODE0_RAY_ITERS = {
    (2, 1, 1): [[2, 2, 10, 12, 12, 11, 11, 10, 2, 2, 12, 13, 12, 12, 11, 12, 12, 12, 11, 12, 2, 2, 12, 13, 12, 11, 11, 10, 2, 2, 10, 12],
                [2, 2, 3, 2, 6, 7, 9, 8, 2, 2, 3, 2, 6, 7, 9, 11, 10, 9, 7, 6, 2, 2, 10, 11, 10, 9, 7, 6, 2, 2, 9, 10]],
    (1, 1, 2): [[2, 2, 10, 12, 11, 11, 11, 11, 2, 2, 12, 13, 12, 11, 12, 12, 12, 11, 12, 12, 2, 2, 12, 13, 11, 11, 11, 11, 2, 2, 10, 12],
                [2, 2, 3, 3, 6, 8, 9, 9, 2, 2, 3, 2, 6, 6, 9, 11, 10, 8, 6, 6, 2, 2, 10, 11, 9, 10, 8, 6, 2, 2, 9, 10]],
    (2, 2, 1): [[3, 3, 10, 12, 12, 11, 11, 10, 3, 3, 12, 13, 13, 12, 12, 12, 13, 12, 12, 12, 3, 3, 12, 13, 12, 11, 11, 10, 3, 3, 10, 12],
                [2, 2, 3, 2, 6, 7, 8, 8, 2, 2, 3, 3, 6, 7, 10, 11, 11, 10, 7, 6, 2, 2, 11, 12, 10, 9, 7, 6, 2, 2, 9, 10]],
}


def _tight_plume(ffm, ctx):
    os.environ["FFM_PLUME_TIGHT"] = "1"
    try:
        return ffm.Plume(ctx, GLOB)
    finally:
        del os.environ["FFM_PLUME_TIGHT"]


@pytest.fixture(scope="module")
def single(ffm, ctx):
    """the single-rank ordered run of the same driver: per step G, the 32 rays, the solve log; after step 2 the other fields"""
    from oracle import plume
    case = _tight_plume(ffm, ctx)
    case.set_radiation(solverFreq=1, rays=plume.ray_set())
    out = []
    for step in range(2):
        if step == 1:
            case.set_radiation_model(0.08, 0.3, 0.3)
        case.step()
        d = {name: case.field(name) for name in ["G"] + RAYS + (FIELDS if step == 1 else [])}
        d["iters"] = [(n, p["nIterations"]) for n, p in case.solves()]
        out.append(d)
    case.close()
    return out


@pytest.fixture(scope="module")
def oracle_run(O):
    """oracle.plume.Plume(n) with set_radiation(solverFreq=1): G and the rays of the two steps"""
    from oracle import plume
    ref = plume.Plume(GLOB); ref.set_radiation(solverFreq=1)
    out = []
    for step in range(2):
        if step == 1:
            ref.set_radiation_model(0.08, 0.3, 0.3)
        ref.step()
        d = {"I%d" % i: ref.I[i].copy() for i in range(32)}
        d["G"] = ref.G.copy()
        out.append(d)
    return out


_RUNS = {}


def _decomposed(grid):
    """both orderings on `grid`, one launch of the workers per grid for the whole module: {key: field gathered over the ranks},
    the per-rank solve logs under 'iters' and the rays' residuals under 'res'"""
    if grid in _RUNS:
        return _RUNS[grid]
    world = grid[0] * grid[1] * grid[2]
    port = free_port()
    with tempfile.TemporaryDirectory() as tmp:
        procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "workers", "plume_rays_rank.py"), str(r), str(world), str(port),
                                   *map(str, GLOB), *map(str, grid), "01", tmp], env=dict(os.environ, FFM_PLUME_TIGHT="1"))
                 for r in range(world)]
        try:
            rcs = [p.wait(timeout=240) for p in procs]
        finally:
            for p in procs:                      # never leave a rank behind (the others wait for it in gloo)
                if p.poll() is None:
                    p.kill()
        assert rcs == [0] * world
        parts = [dict(np.load(os.path.join(tmp, "rank%d.npz" % r), allow_pickle=True)) for r in range(world)]
    nx, ny, nz = GLOB
    run = {"iters": {}, "res": {}}
    for key in parts[0]:
        if key in ("lo", "hi"):
            continue
        if key.endswith("_iters") or key.endswith("_res"):
            run["iters" if key.endswith("_iters") else "res"][key.rsplit("_", 1)[0]] = [pt[key] for pt in parts]
            continue
        full = np.empty((nz, ny, nx))
        for pt in parts:
            lo, hi = pt["lo"], pt["hi"]
            full[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = pt[key].reshape(hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])
        run[key] = full.ravel()
    _RUNS[grid] = run
    return run


def _ray_counts(log):
    got = dict((n, int(it)) for n, it in log if n.startswith("I"))
    assert len(got) == 32
    return [got["I%d" % i] for i in range(32)]


@pytest.mark.parametrize("grid", GRIDS)
def test_staged_rays_take_one_iteration_on_every_rank(ffm, ctx, grid):
    run = _decomposed(grid)
    for step in range(2):
        for r, log in enumerate(run["iters"]["m1_s%d" % step]):
            assert _ray_counts(log) == [1] * 32, (grid, step, r)
        for r, res in enumerate(run["res"]["m1_s%d" % step]):
            print("grid %s step %d rank %d: max final residual of a staged ray solve %.3e (initial: max %.3e)"
                  % (grid, step + 1, r, res[:, 1].max(), res[:, 0].max()))
            # every solve reports that its substitution was the solve: sum |source - A psi| <= 1e-10 sum |source| over the rank's rows
            # (ffm_solve_triangular_rows_d; the driver turns a solve that is not into an error).  OpenFOAM's NORMALISED final residual
            # is printed, not bounded: its normFactor is round-off where a block's solution is uniform (DESIGN.md row f / N1)
            assert res.shape == (32, 3) and np.all(np.isfinite(res)) and np.all(res[:, 0] > 0) and np.all(res[:, 2] == 1)


@pytest.mark.parametrize("grid", GRIDS)
def test_staged_rays_match_the_single_rank_ordered_run_and_the_oracle(ffm, ctx, single, oracle_run, grid):
    run = _decomposed(grid)
    worst = {"single": 0.0, "oracle": 0.0}
    for step in range(2):
        for name in ["G"] + RAYS:
            a = run["m1_s%d_%s" % (step, name)]
            for what, ref in (("single", single[step][name]), ("oracle", oracle_run[step][name])):
                worst[what] = max(worst[what], rel_l2(a, ref))
    print("grid %s: max rel-L2 of G and the 32 rays over two steps: vs single-rank ordered %.3e, vs oracle %.3e" % (grid, worst["single"], worst["oracle"]))
    assert worst["single"] < BOUND and worst["oracle"] < BOUND, (grid, worst)


@pytest.mark.parametrize("grid", GRIDS)
def test_coupled_step_keeps_the_other_fields_and_their_iteration_counts(ffm, ctx, single, grid):
    run = _decomposed(grid)
    for name in FIELDS:
        a, b = run["m1_s1_%s" % name], single[1][name]
        e = rel_l2(a, b) if np.linalg.norm(b) > 1e-30 else float(np.abs(a).max())
        print("grid %s %s: staged %.3e (ordering 0 on the same grid: %.3e)" % (grid, name, e, rel_l2(run["m0_s1_%s" % name], b)))
        assert e < BOUND, (grid, name, e)
    for step in range(2):
        for l0, l1 in zip(run["iters"]["m0_s%d" % step], run["iters"]["m1_s%d" % step]):
            other = lambda log: [(n, int(it)) for n, it in log if not n.startswith("I")]      # noqa: E731
            assert other(l0) == other(l1), (grid, step)


@pytest.mark.parametrize("grid", GRIDS)
def test_ordering_0_keeps_its_ray_iteration_counts(ffm, ctx, grid):
    run = _decomposed(grid)
    logs = [run["iters"]["m0_s%d" % step] for step in range(2)]
    for step in range(2):
        for log in logs[step][1:]:
            assert _ray_counts(log) == _ray_counts(logs[step][0])          # a global solve: every rank counts the same
    got = [_ray_counts(logs[step][0]) for step in range(2)]
    print("grid %s ordering 0 ray iterations: %r" % (grid, got))
    assert got == MODE0_RAY_ITERS[grid], grid
    assert min(min(g) for g in got) > 1                                     # ... and they are many: what the staged sweep removes


def test_single_block_ordering_1_is_bitwise_ordering_0(ffm, ctx, single):
    from oracle import plume
    case = _tight_plume(ffm, ctx)
    case.set_radiation(solverFreq=1, rays=plume.ray_set())
    case.set_radiation_ordering(1)
    for step in range(2):
        if step == 1:
            case.set_radiation_model(0.08, 0.3, 0.3)
        case.step()
        assert [(n, p["nIterations"]) for n, p in case.solves()] == single[step]["iters"]
        for name in ["G"] + RAYS + (FIELDS if step == 1 else []):
            assert np.array_equal(case.field(name), single[step][name]), (step, name)
    with pytest.raises(ffm.FfmError):
        case.set_radiation_ordering(2)
    case.close()


def test_fused_ray_assembly_is_bitwise_the_operator_chain(ffm, ctx):
    """ffm_fvdom_ray_assemble_d against the six launches + ffm_fvm_add_boundary it replaces, on the plume box (inlet, floor, top and
    side patches: inflow and outflow faces of every kind), in a state with a flame (T not uniform) and the emission term on"""
    from oracle import plume
    rays = plume.ray_set()
    case = ffm.Plume(ctx, GLOB)
    case.set_radiation(solverFreq=1, rays=rays)
    case.step()
    case.set_radiation_model(0.08, 0.3, 0.3)
    case.step()
    signs = [tuple(bool(c < 0) for c in d) for d, _ in rays]
    allPos, mixed = signs.index((False, False, False)), next(i for i, s in enumerate(signs) if len(set(s)) == 2)
    for ray in (allPos, mixed):
        chain, fused = case.ray_system(ray, fused=False), case.ray_system(ray, fused=True)
        for what, a, b in zip(("diag", "upper", "lower", "source"), fused, chain):
            assert np.all(np.isfinite(b)) and (what in ("upper", "lower") or np.abs(b).max() > 0), (ray, what)
            assert np.array_equal(a, b), (ray, what, np.abs(a - b).max())
    case.close()
