"""The plume step with h as the fifth system of the species (one assembly pass, one lock-step solve of five lanes: ffm_plume_step.hip,
species_eqns) against FFM_PLUME_SEPARATE_H=1 (h assembled and solved after the species), from the conditioned start state of
oracle/plume.py on a 24^3 box, four steps.  Every check is a byte comparison: the fields, the old-time fields and the solve log.

* default selection: every step takes the joint form;
* coupled radiation every 2nd step: the steps with radiation->correct() between the species and h keep the separate sequence, the
  others take the joint form with radiation->Sh among h's sources;
* steckler solvers, one limiter per field: the joint form is off (no step counted, the same solve log);
* one run with the allocator's blocks handed out NaN-filled.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = (24, 24, 24)
FIELDS = ["rho", "p", "p_rgh", "T", "h", "Ux", "Uy", "Uz", "O2", "H2O", "C3H8", "CO2", "N2", "K", "psi", "ph_rgh"]
OLD = ["rho0", "K0", "psi0", "h0", "p0", "p_rgh0", "U0x", "U0y", "U0z", "O2_0", "H2O_0", "C3H8_0", "CO2_0"]
TRANSPORT = ["O2", "H2O", "C3H8", "CO2", "h"]


def _case(ffm, ctx, separate=False, steckler=False, independent=False, radiation=False):
    env = {"FFM_PLUME_SEPARATE_H": separate, "FFM_PLUME_INDEPENDENT_LIMITERS": independent}
    for k, on in env.items():
        if on:
            os.environ[k] = "1"
    try:
        case = ffm.Plume(ctx, N)
    finally:
        for k in env:
            os.environ.pop(k, None)
    if steckler:
        case.set_solvers(True)
    if radiation:
        case.set_radiation(solverFreq=2)
        case.set_radiation_model(0.08, 0.3, 0.3)
    from oracle import plume
    m = plume.make_mesh(N)
    Y0, h0 = plume.conditioned_state(m, plume.Y_AMB_COND, plume.H_AMB_COND)
    case.set_initial_state(Y0, h0, plume.Y_AMB_COND, plume.Y_IN_COND, plume.H_AMB_COND)
    return case


def _solves(case):
    return [(name, sorted(pf.items())) for name, pf in case.solves()]


def _same_four_steps(a, b, jointSteps):
    """a: the default sequence, b: FFM_PLUME_SEPARATE_H; jointSteps[i]: step i of `a` takes the joint form"""
    nC = a.nCells
    for step in range(4):
        before = a.joint_steps()
        a.step(); b.step()
        assert a.joint_steps() - before == (1 if jointSteps[step] else 0), step
        assert b.joint_steps() == 0
        log = _solves(a)
        assert log == _solves(b), step
        names = [nm for nm, _ in log]
        i = names.index("O2")
        assert names[i:i + 4] == TRANSPORT[:4] and "h" in names[i + 4:], names         # the log keeps the reference's order
        for name in FIELDS:
            assert a.field(name).tobytes() == b.field(name).tobytes(), (step, name)
        for name in OLD:
            assert a.raw(name)[:nC].tobytes() == b.raw(name)[:nC].tobytes(), (step, name)
    its = {nm: pf["nIterations"] for nm, pf in a.solves() if nm in TRANSPORT}
    print("iterations of the last step", its)
    a.close(); b.close()


def test_joint_step_equals_the_separate_sequence(ffm, ctx):
    _same_four_steps(_case(ffm, ctx), _case(ffm, ctx, separate=True), [True] * 4)


def test_with_coupled_radiation_every_second_step(ffm, ctx):
    _same_four_steps(_case(ffm, ctx, radiation=True), _case(ffm, ctx, separate=True, radiation=True), [False, True, False, True])


@pytest.mark.parametrize("kw", [dict(steckler=True), dict(independent=True)], ids=["steckler", "independent-limiters"])
def test_joint_form_is_off_for_other_selections(ffm, ctx, kw):
    _same_four_steps(_case(ffm, ctx, **kw), _case(ffm, ctx, separate=True, **kw), [False] * 4)


def test_joint_step_with_a_poisoned_pool(ffm, ctx):
    ref = _case(ffm, ctx, separate=True)
    ctx.debug_pool_poison(True)
    try:
        case = _case(ffm, ctx)
        for _ in range(2):
            case.step(); ref.step()
    finally:
        ctx.debug_pool_poison(False)
    assert case.joint_steps() == 2
    assert _solves(case) == _solves(ref)
    for name in FIELDS:
        f = case.field(name)
        assert np.isfinite(f).all() and f.tobytes() == ref.field(name).tobytes(), name
    case.close(); ref.close()
