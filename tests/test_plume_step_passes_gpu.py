"""The time step's fused passes and pointer-swapped old-time fields (ffm_plume.hip): every check is a byte comparison.

* the default step (div(phi,K) in one cell pass, the species tail in one pass, rhoEqn with the solve as the epilogue of the surface
  integral, rAU inside UEqn.A(), ddtCorr inside the old-time flux pass) against FFM_PLUME_UNFUSED=1 (one kernel per operator), from the
  conditioned start state of oracle/plume.py, after 1, 2, 3 and 4 steps, with both solver selections;
* rho0, K0 and psi0 trade buffers with rho, K and psi at every step: after an odd and after an even number of steps they are the
  previous step's fields;
* ffm_plume_set_initial_state after three steps starts the case again: two more steps equal those of a fresh case.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = (24, 24, 24)
FIELDS = ["rho", "p", "p_rgh", "T", "h", "Ux", "Uy", "Uz", "O2", "H2O", "C3H8", "CO2", "N2", "K", "psi", "ph_rgh"]


def _case(ffm, ctx, n=N, unfused=False, steckler=False):
    if unfused:
        os.environ["FFM_PLUME_UNFUSED"] = "1"
    try:
        case = ffm.Plume(ctx, n)
    finally:
        os.environ.pop("FFM_PLUME_UNFUSED", None)
    if steckler:
        case.set_solvers(True)
    _start(case, n)
    return case


def _start(case, n):
    from oracle import plume
    m = plume.make_mesh(n)
    Y0, h0 = plume.conditioned_state(m, plume.Y_AMB_COND, plume.H_AMB_COND)
    case.set_initial_state(Y0, h0, plume.Y_AMB_COND, plume.Y_IN_COND, plume.H_AMB_COND)


def _solves(case):
    return [(name, sorted(pf.items())) for name, pf in case.solves()]


@pytest.mark.parametrize("steckler", [False, True])
def test_fused_step_equals_the_per_operator_step(ffm, ctx, steckler):
    fused = _case(ffm, ctx, steckler=steckler)
    plain = _case(ffm, ctx, unfused=True, steckler=steckler)
    for name in FIELDS:
        assert fused.field(name).tobytes() == plain.field(name).tobytes(), ("start", name)
    for step in range(1, 5):
        fused.step(); plain.step()
        assert _solves(fused) == _solves(plain), step
        for name in FIELDS:
            assert fused.field(name).tobytes() == plain.field(name).tobytes(), (step, name)
    fused.close(); plain.close()


def test_old_time_fields_after_odd_and_even_step_counts(ffm, ctx):
    case = _case(ffm, ctx)
    pairs = [("rho0", "rho"), ("K0", "K"), ("psi0", "psi"), ("h0", "h"), ("p0", "p"), ("p_rgh0", "p_rgh"), ("U0x", "Ux"), ("U0y", "Uy"),
             ("U0z", "Uz"), ("O2_0", "O2"), ("H2O_0", "H2O"), ("C3H8_0", "C3H8"), ("CO2_0", "CO2")]
    nC = case.nCells
    prev = {new: case.raw(new)[:nC].copy() for _, new in pairs}
    for step in range(1, 5):
        case.step()
        for old, new in pairs:
            assert case.raw(old)[:nC].tobytes() == prev[new].tobytes(), (step, old)
        now = {new: case.raw(new)[:nC].copy() for _, new in pairs}
        assert any(now[k].tobytes() != prev[k].tobytes() for k in ("rho", "K", "psi")), step      # the fields do move
        prev = now
    case.close()


@pytest.mark.parametrize("steckler", [False, True])
def test_restart_after_three_steps_equals_a_fresh_case(ffm, ctx, steckler):
    again = _case(ffm, ctx, steckler=steckler)
    for _ in range(3):
        again.step()
    _start(again, N)
    fresh = _case(ffm, ctx, steckler=steckler)
    assert _solves(again) == _solves(fresh)                    # the hydrostatic solves
    for step in range(1, 3):
        again.step(); fresh.step()
        assert _solves(again) == _solves(fresh), step
        for name in FIELDS:
            assert again.field(name).tobytes() == fresh.field(name).tobytes(), (step, name)
    again.close(); fresh.close()
