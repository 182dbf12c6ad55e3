"""The CPU restatement of the plume step with the kEqn model (tests/plume_keqn_ref.py) and the inputs of the GPU tests
(tests/test_plume_keqn_gpu.py): a closed form, the signs the model guarantees, and that the model matters on the start state the
device is compared on -- a device that ignores it cannot pass the parity test."""
import numpy as np
import pytest

from common import rel_l2
from plume_keqn_ref import CE, SMALL, PlumeKEqn, smooth_k0

N = (12, 16, 12)


def start(n=N, turbulence=True, k0=True, **kw):
    """the GPU tests' start state: conditioned=True and the smooth non-uniform k0"""
    from oracle import plume
    ref = PlumeKEqn(n, conditioned=True, **kw)
    if turbulence:
        ref.set_turbulence(k0=smooth_k0(ref.m) if k0 else None)
    return ref, plume


def test_gas_at_rest_with_uniform_k_decays_by_the_closed_form(O, monkeypatch):
    """No gravity, no inflow, inflow values equal to the ambient ones: the gas stays at rest and uniform up to the rounding noise of the
    solves of uniform fields, G = 0, convection and diffusion of the uniform k vanish, and the k equation is, row by row,
    (rdt rho + Ce rho sqrt(k0)/delta) k1 = rdt rho0 k0 -- in the cells on the inlet with the patch's diffusion towards the fixed
    kInlet on both sides.  Every solve runs to 1e-14 of the normalised residual; the bound is worked out below, three orders below
    the decay itself (Ce sqrt(k0)/delta/rdt = 1.3e-3 here)."""
    from oracle import plume
    monkeypatch.setattr(plume, "G", np.zeros(3))

    class Tight(plume.Solvers):
        CONTROLS = {kind: dict(c, tolerance=1e-14, relTol=0.0) for kind, c in plume.Solvers.CONTROLS.items()}

    n = (6, 7, 5)
    ref = PlumeKEqn(n, solvers=Tight())
    ref.Y_in = ref.Y_amb.copy()
    inlet = ref.m.patches[ref.names.index("inlet")]
    ref.inlet_U, ref.inlet_h = np.zeros((inlet.size, 3)), 0.0
    k0 = 4.0e-3
    ref.set_turbulence(kInlet=k0)
    rho0 = ref.rho.copy()
    ref.step()
    assert np.abs(ref.U).max() < 1e-9 and np.abs(ref.Gk).max() < 1e-20
    rdt = ref.rDeltaT
    sp = CE * rho0 * np.sqrt(k0) / ref.delta
    # the inlet holds k at kInlet = k0 while the cells decay: its cells gain the patch's diffusion a (kInlet - k1), a = gamma_b delta_b |Sf|/V
    a = np.zeros(ref.m.nCells)
    nut0 = 0.094 * np.sqrt(k0) * ref.delta
    np.add.at(a, inlet.faceCells, (rho0 * (nut0 + plume.MU / rho0))[inlet.faceCells] * inlet.deltaCoeffs * inlet.magSf / ref.m.V[inlet.faceCells])
    closed = (rdt * rho0 * k0 + a * k0) / (rdt * rho0 + sp + a)
    assert np.array_equal(ref.rho0, rho0)
    err = np.abs(ref.k / closed - 1.0)
    # the inlet cells then differ from their neighbours by nu_eff dt (2/h^2) (1 - k1/k0) ~ 3e-7 relative, which diffusion carries on
    # with the weight nu_eff dt/h^2 ~ 1e-4 per ring of cells: 4e-11 in the first ring, below 1e-9 everywhere
    assert err.max() < 1e-9, err.max()
    away = np.ones(ref.m.nCells, bool); away[inlet.faceCells] = False
    assert np.array_equal(closed[away], (rdt * rho0 * k0 / (rdt * rho0 + sp))[away])
    assert abs(1.0 - closed[0] / k0) > 1e-3                    # the decay is there to be seen


def test_production_is_non_negative_and_k_stays_bounded(O):
    ref, _ = start()
    for step in range(3):
        ref.step()
        assert (ref.Gk >= 0.0).all(), (step, ref.Gk.min())
        assert (ref.k >= SMALL).all() and np.isfinite(ref.k).all(), step
        assert (ref.nut >= 0.0).all() and (ref.alphat >= 0.0).all(), step
    assert ref.Gk.max() > 0.0


def test_the_model_moves_the_start_state_of_the_gpu_tests_far_beyond_the_parity_bound(O):
    """1e-8 is the parity bound; with the model the velocity differs from the model-free step's by orders of magnitude more after
    the three steps the GPU tests take, nut is of the order of mu/rho or larger, and k0 varies far above rounding everywhere"""
    on, plume = start()
    off, _ = start(turbulence=False)
    k0 = smooth_k0(on.m)
    assert k0.min() > 0 and (k0.max() - k0.min()) / k0.mean() > 0.1
    d = np.abs(k0[on.m.u] - k0[on.m.l]) / k0.mean()
    assert d.min() > 1e-6, d.min()                              # no two neighbours equal: limitedLinear's r is well-conditioned
    assert (on.nut / (plume.MU / on.rho)).max() >= 1.0
    for _ in range(3):
        on.step(); off.step()
    for c in range(3):
        assert rel_l2(on.U[c], off.U[c]) > 1e-5, (c, rel_l2(on.U[c], off.U[c]))
    assert rel_l2(on.h, off.h) > 1e-6
    assert [nme for nme, _ in on.sol.log][-2:] == ["p_rgh", "k"] and "k" not in [nme for nme, _ in off.sol.log]


def test_the_model_off_is_the_oracles_own_step(O):
    a, plume = start(turbulence=False)
    b = plume.Plume(N, conditioned=True)
    for _ in range(2):
        a.step(); b.step()
    for name, v in b.fields().items():
        assert np.array_equal(a.fields()[name], v), name
