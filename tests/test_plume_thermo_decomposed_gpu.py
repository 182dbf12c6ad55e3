"""The plume step with kEqn, the janaf thermo and the reference's EDC on a decomposed box: 2 ranks (2 x 1 x 1, one process each,
sharing cuda:0 over the host / gloo transport) against the single-rank run from the default start state, every solve to 1e-13
(FFM_PLUME_TIGHT=1: what is left is block-Jacobi preconditioning and the order of the global sums, as in
tests/test_plume_keqn_decomposed_gpu.py, whose figure on this set-up is 3e-9).  thermo.correct() and the EDC run over the ghost cells
too, from refreshed Y, h, k and rho: mu, alpha and wFuel there must be the neighbour rank's -- a stale ghost layer shows at the cut at
1e-3, not at 1e-8.  set_thermo's hydrostatic start is a collective of its own.  Each rank runs under a time limit of its own.
p_rgh is held to 1e-6 of its own variation, as in both existing decomposed tests (p itself meets 1e-8)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from common import rel_l2, free_port
from oracle import thermo as TH
from plume_keqn_ref import smooth_k0
from plume_thermo_ref import DATA, TABLE, single_step

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT = 200         # seconds per rank
NAMES = ["rho", "p", "T", "h", "Ux", "Uy", "Uz", "O2", "C3H8", "CO2", "p_rgh", "k", "nut", "alphat", "psi", "mu", "alpha", "Cp", "wFuel", "Qdot"]


def test_two_ranks_match_the_single_rank_run_with_every_model_on(ffm, ctx):
    from oracle import plume
    glob, grid, nSteps = (12, 16, 12), (2, 1, 1), 2
    world = grid[0] * grid[1] * grid[2]
    os.environ["FFM_PLUME_TIGHT"] = "1"
    try:
        ref = ffm.Plume(ctx, glob)
    finally:
        del os.environ["FFM_PLUME_TIGHT"]
    th = ffm.Thermo(ctx, DATA["species"], TABLE, TH.RR)
    rx = single_step()
    ref.set_turbulence(k0=smooth_k0(plume.make_mesh(glob)))
    ref.set_thermo(th)
    ref.set_combustion(s=rx.s, qFuel=rx.qFuel)
    for _ in range(nSteps):
        ref.step()
    assert ref.field("wFuel").max() > 0.0
    port = free_port()
    with tempfile.TemporaryDirectory() as tmp:
        # the ranks are one collective run: started together, each under its own limit, nothing started after them
        procs = [subprocess.Popen(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.join(HERE, "workers", "plume_thermo_rank.py"),
                                   str(r), str(world), str(port), *map(str, glob), *map(str, grid), str(nSteps), tmp],
                                  env=dict(os.environ, FFM_PLUME_TIGHT="1")) for r in range(world)]
        try:
            rcs = [p.wait(timeout=LIMIT + 30) for p in procs]
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
        assert rcs == [0] * world
        parts = [np.load(os.path.join(tmp, "rank%d.npz" % r)) for r in range(world)]
    nx, ny, nz = glob
    errs = {}
    for name in NAMES:
        full = np.empty((nz, ny, nx))
        for pt in parts:
            lo, hi = pt["lo"], pt["hi"]
            full[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = pt[name].reshape(hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])
        a, b = full.ravel(), ref.field(name)
        if name == "p_rgh":             # a small fluctuation on top of p (held to 1e-8): against the scale of its own variation
            errs[name] = np.linalg.norm(a - b) / max(np.linalg.norm(b - b.mean()), 1e-30)
        else:
            errs[name] = np.abs(a).max() if np.linalg.norm(b) < 1e-30 else rel_l2(a, b)
    print(", ".join("%s %.1e" % kv for kv in errs.items()))
    for name, e in errs.items():
        assert e < (1e-6 if name == "p_rgh" else 1e-8), (name, e)
    ref.close(); th.close()
