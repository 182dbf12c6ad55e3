"""The plume step whose LUST correction of UEqn and div(phi,K) of EEqn run as tile passes without gradient arrays (ffm_plume_step.hip:
u_sources, mv_weights, e_K_terms) against the per-operator step (FFM_PLUME_UNFUSED=1), from the conditioned start state of
oracle/plume.py on a 24^3 box, three steps, byte for byte: the fields, the old-time fields and the solve log.

* the default selection (both tile passes, h with the species);
* the kEqn model selected: the gradients of U are wanted by the stress divergence and by kEqn, the step keeps their arrays;
* coupled radiation every 2nd step: the face products of div(phi,K) live over the species solves and radiation->correct();
* weights handed in on one step (ffm_plume_override_mv_weights): that step's e_K_terms runs the gradient form, the others the sum;
* one run with the allocator's blocks handed out NaN-filled."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = (24, 24, 24)
FIELDS = ["rho", "p", "p_rgh", "T", "h", "Ux", "Uy", "Uz", "O2", "H2O", "C3H8", "CO2", "N2", "K", "psi", "ph_rgh"]
OLD = ["rho0", "K0", "psi0", "h0", "p0", "p_rgh0", "U0x", "U0y", "U0z", "O2_0", "H2O_0", "C3H8_0", "CO2_0"]


def _case(ffm, ctx, unfused=False, keqn=False, radiation=False):
    if unfused:
        os.environ["FFM_PLUME_UNFUSED"] = "1"
    try:
        case = ffm.Plume(ctx, N)
    finally:
        os.environ.pop("FFM_PLUME_UNFUSED", None)
    from oracle import plume
    m = plume.make_mesh(N)
    if radiation:
        case.set_radiation(solverFreq=2)
        case.set_radiation_model(0.08, 0.3, 0.3)
    Y0, h0 = plume.conditioned_state(m, plume.Y_AMB_COND, plume.H_AMB_COND)
    case.set_initial_state(Y0, h0, plume.Y_AMB_COND, plume.Y_IN_COND, plume.H_AMB_COND)
    if keqn:
        from plume_keqn_ref import smooth_k0
        case.set_turbulence(k0=smooth_k0(m))
    return case


def _solves(case):
    return [(name, sorted(pf.items())) for name, pf in case.solves()]


def _same(a, b, step):
    nC = a.nCells
    assert _solves(a) == _solves(b), step
    for name in FIELDS:
        fa = a.field(name)
        assert np.isfinite(fa).all() and fa.tobytes() == b.field(name).tobytes(), (step, name)
    for name in OLD:
        assert a.raw(name)[:nC].tobytes() == b.raw(name)[:nC].tobytes(), (step, name)


def _three_steps(a, b, before_step=None):
    for step in range(3):
        if before_step:
            before_step(step, a, b)
        a.step(); b.step()
        _same(a, b, step)
    a.close(); b.close()


@pytest.mark.parametrize("kw", [dict(), dict(keqn=True), dict(radiation=True)], ids=["default", "kEqn", "radiation"])
def test_fused_step_equals_the_per_operator_step(ffm, ctx, kw):
    _three_steps(_case(ffm, ctx, **kw), _case(ffm, ctx, unfused=True, **kw))


def test_weights_handed_in_on_one_step(ffm, ctx):
    """step 1 convects the species and h with the linear weights handed in: mv_weights forms no face products in that step"""
    def hand_in(step, a, b):
        if step == 1:
            w = np.full(a.nFaces, 0.5)
            a.override_mv_weights(w); b.override_mv_weights(w)
    _three_steps(_case(ffm, ctx), _case(ffm, ctx, unfused=True), hand_in)


def test_with_a_poisoned_pool(ffm, ctx):
    ref = _case(ffm, ctx, unfused=True)
    ctx.debug_pool_poison(True)
    try:
        case = _case(ffm, ctx)
        for step in range(3):
            case.step(); ref.step()
            _same(case, ref, step)
    finally:
        ctx.debug_pool_poison(False)
    case.close(); ref.close()
