"""The plume step with kEqn, the janaf thermo, the reference's EDC AND the coupled fvDOM rays (ffm_plume_set_radiation_thermo) on a
decomposed box: 2 ranks (2 x 1 x 1, one process each, sharing cuda:0 over the host / gloo transport) against the single-rank device
run from the default start state (the only one a block can be given), both ray orderings, every solve to 1e-13 (FFM_PLUME_TIGHT=1, as
in tests/test_plume_thermo_decomposed_gpu.py and tests/test_plume_rays_decomposed_gpu.py).  radiation->Sh reads the Cp field of the
ghost cells too, and the rays the thermo package's T there.

The protocol of tests/test_plume_rays_decomposed_gpu.py: one step with the rays on, then a second one with the absorption / emission
model coupled into h, compared after it.  That step has the ray sweep with E = RadFraction*Qdot (the flame burns by then), G, the Sh
pass with the Cp field and the enthalpy solve with it.  Steps after it are not compared: with absorption the ambient cells are heated
from an enthalpy that is rounding noise, and limitedLinear's weights of such a field multiply the new O(1) enthalpies
(tests/test_plume_gpu.py::test_plume_with_the_reference_radiation_model_coupled_into_h,
tests/test_plume_cpu.py::test_limited_weights_of_a_noise_field_are_ill_conditioned): the differences of a decomposed run's sums are
amplified like any other perturbation.  Measured on an MI355X, both orderings alike: after the compared step h 1.1e-9, U 1.7e-10,
T 3.4e-12, G 1.4e-15, ShSu 2.0e-14, rays <= 7.3e-15; one step later h 4.7e-7, U 1.3e-7, T 3.0e-9 while G 4.0e-14, ShSu 8.5e-14,
Cp 1.2e-10, rays <= 1.1e-13; two coupled steps without absorption (a = 0): h 1.1e-9, U 1.7e-10.

Bounds: 1e-8 rel-L2, the BOUND of tests/test_plume_rays_decomposed_gpu.py -- for the staged sweep (ordering 1), whose rays take one
iteration on every rank, and for the block-Jacobi solves of ordering 0 alike; p_rgh at 1e-6 of its own variation, as in every
decomposed test with the thermo package.  Each rank runs under a time limit of its own; the parent checks every exit status."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from common import rel_l2, free_port
from oracle import thermo as TH
from plume_keqn_ref import smooth_k0
from plume_radiation_ref import RAD_MODEL
from plume_thermo_ref import DATA, TABLE, single_step

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT = 200         # seconds per rank
BOUND = 1e-8
GLOB, GRID, NSTEPS, COUPLE_AT = (12, 16, 12), (2, 1, 1), 2, 1
NAMES = ["rho", "p", "T", "h", "Ux", "Uy", "Uz", "O2", "C3H8", "CO2", "p_rgh", "k", "nut", "alphat", "psi", "mu", "alpha", "Cp", "wFuel", "Qdot",
         "G", "ShSu", "ShSp"] + ["I%d" % i for i in range(32)]


def _run(ffm, ctx, nSteps, coupleAt, model):
    """the single-rank run's fields and one launch of the two ranks that runs both orderings"""
    from oracle import plume
    os.environ["FFM_PLUME_TIGHT"] = "1"
    try:
        ref = ffm.Plume(ctx, GLOB)
    finally:
        del os.environ["FFM_PLUME_TIGHT"]
    th = ffm.Thermo(ctx, DATA["species"], TABLE, TH.RR)
    rx = single_step()
    ref.set_turbulence(k0=smooth_k0(plume.make_mesh(GLOB)))
    ref.set_thermo(th)
    ref.set_combustion(s=rx.s, qFuel=rx.qFuel)
    ref.set_radiation_thermo(True)
    ref.set_radiation(solverFreq=1)
    for step in range(nSteps):
        if step == coupleAt:
            ref.set_radiation_model(*model)
        ref.step()
    single = {name: ref.field(name) for name in NAMES}
    ref.close(); th.close()
    world = GRID[0] * GRID[1] * GRID[2]
    port = free_port()
    with tempfile.TemporaryDirectory() as tmp:
        # the ranks are one collective run: started together, each under its own limit, nothing started after them
        procs = [subprocess.Popen(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.join(HERE, "workers", "plume_radiation_rank.py"),
                                   str(r), str(world), str(port), *map(str, GLOB), *map(str, GRID), str(nSteps), "01", tmp, str(coupleAt), *map(repr, model)],
                                  env=dict(os.environ, FFM_PLUME_TIGHT="1")) for r in range(world)]
        try:
            rcs = [p.wait(timeout=LIMIT + 30) for p in procs]
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
        assert rcs == [0] * world
        parts = [dict(np.load(os.path.join(tmp, "rank%d.npz" % r))) for r in range(world)]
    return single, parts


@pytest.fixture(scope="module")
def runs(ffm, ctx):
    return _run(ffm, ctx, NSTEPS, COUPLE_AT, RAD_MODEL)


def _gather(parts, key):
    nx, ny, nz = GLOB
    full = np.empty((nz, ny, nx))
    for pt in parts:
        lo, hi = pt["lo"], pt["hi"]
        full[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = pt[key].reshape(hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])
    return full.ravel()


def _errors(single, parts, mode):
    errs = {}
    for name in NAMES:
        a, b = _gather(parts, "m%d_%s" % (mode, name)), single[name]
        if name == "p_rgh":             # a small fluctuation on top of p (held to 1e-8): against the scale of its own variation
            errs[name] = np.linalg.norm(a - b) / max(np.linalg.norm(b - b.mean()), 1e-30)
        else:
            errs[name] = np.abs(a).max() if np.linalg.norm(b) < 1e-30 else rel_l2(a, b)
    rays = [errs["I%d" % i] for i in range(32)]
    print("ordering %d: %s, worst ray %.1e" % (mode, ", ".join("%s %.1e" % (k, v) for k, v in errs.items() if not k.startswith("I")), max(rays)))
    return errs


@pytest.mark.parametrize("mode", [1, 0])
def test_two_ranks_match_the_single_rank_run_with_radiation_and_every_model_on(runs, mode):
    single, parts = runs
    assert single["wFuel"].max() > 0.0 and single["G"].min() > 0.0 and np.abs(single["ShSu"]).max() > 0.0
    # Cp is a field and nowhere the stand-in's constant: by 1e-3 of it, five decades above the bound below
    assert single["Cp"].max() - single["Cp"].min() > 1.0 and np.abs(single["Cp"] - 1005.0).min() > 1.0
    for pt in parts:
        it = pt["m%d_rayIters" % mode]
        assert len(it) == 32 and (np.all(it == 1) if mode == 1 else it.min() > 1)       # staged: exact; block-Jacobi: iterated
    for name, e in _errors(single, parts, mode).items():
        assert e < (1e-6 if name == "p_rgh" else BOUND), (mode, name, e)
