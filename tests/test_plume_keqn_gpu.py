"""The compiled plume step with the LES kEqn sub-grid model (ffm_plume_set_turbulence) against its CPU restatement
(tests/plume_keqn_ref.py), from the start state tests/test_plume_keqn_cpu.py shows the model to matter on: the conditioned state of
oracle/plume.py and a smooth, nowhere-uniform k0.

  (a) parity: after every step every field tests/test_plume_multistep_gpu.py compares, and k, nut, alphat, within 1e-8 rel-L2, with
      identical iteration counts of every solve, k's included;
  (b) the fused step == the per-operator step (FFM_PLUME_UNFUSED=1), byte for byte, every field and solve, three steps;
  (c) (a) with the solver selection of cases/steckler/system/fvSolution:49-62;
  (d) the model switched on and off again: the steps that follow are those of a handle that never had it, byte for byte; refused
      arguments leave the handle as it was;
  (e) three steps with a NaN-poisoned pool equal the unpoisoned run byte for byte.
"""
import os

import numpy as np
import pytest

from common import rel_l2
from plume_keqn_ref import PlumeKEqn, smooth_k0
from test_plume_multistep_gpu import FIELDS as STEP_FIELDS, _compare

pytestmark = pytest.mark.gpu

LES_FIELDS = ["k", "nut", "alphat"]
BYTE_FIELDS = ["rho", "p", "p_rgh", "T", "h", "Ux", "Uy", "Uz", "O2", "H2O", "C3H8", "CO2", "N2", "K", "psi"]


def _gpu_case(ffm, ctx, n, unfused=False, steckler=False, turbulence=True):
    from oracle import plume
    if unfused:
        os.environ["FFM_PLUME_UNFUSED"] = "1"
    try:
        case = ffm.Plume(ctx, n)
    finally:
        os.environ.pop("FFM_PLUME_UNFUSED", None)
    if steckler:
        case.set_solvers(True)
    m = plume.make_mesh(n)
    Y0, h0 = plume.conditioned_state(m, plume.Y_AMB_COND, plume.H_AMB_COND)
    case.set_initial_state(Y0, h0, plume.Y_AMB_COND, plume.Y_IN_COND, plume.H_AMB_COND)
    if turbulence:
        case.set_turbulence(k0=smooth_k0(m))
    return case


def _ref_case(n, steckler=False):
    from oracle import plume
    ref = PlumeKEqn(n, conditioned=True, solvers=plume.StecklerSolvers() if steckler else None)
    ref.set_turbulence(k0=smooth_k0(ref.m))
    return ref


def _solves(case):
    return [(name, sorted(pf.items())) for name, pf in case.solves()]


def _parity(ffm, ctx, n, steps, steckler=False):
    ref, gpu = _ref_case(n, steckler), _gpu_case(ffm, ctx, n, steckler=steckler)
    for name in LES_FIELDS:                                     # correctNut() at set_turbulence
        assert rel_l2(gpu.field(name), ref.fields()[name]) < 1e-13, name
    for step in range(steps):
        ref.step(); gpu.step()
        assert [nme for nme, _ in gpu.solves()][-2:] == ["p_rgh", "k"]
        errs = {name: rel_l2(gpu.field(name), ref.fields()[name]) for name in LES_FIELDS}
        print("step %d: %s" % (step, ", ".join("%s %.2e" % kv for kv in errs.items())))
        worst = _compare(step, gpu, ref)                        # iteration counts of every solve and the step's fields at 1e-8
        print("step %d: worst of %s: %.2e" % (step, "/".join(STEP_FIELDS), worst))
        bad = {k: v for k, v in errs.items() if not v < 1e-8}
        assert not bad, (step, bad)
    gpu.close()


@pytest.mark.parametrize("n", [(12, 16, 12), (16, 20, 14)])
def test_parity_with_the_restatement_at_1e8(O, ffm, ctx, n):
    _parity(ffm, ctx, n, 4)


def test_parity_with_the_steckler_solver_selection(O, ffm, ctx):
    _parity(ffm, ctx, (12, 16, 12), 3, steckler=True)


def test_fused_step_equals_the_per_operator_step_with_the_model_on(ffm, ctx):
    n = (24, 24, 24)
    fused, plain = _gpu_case(ffm, ctx, n), _gpu_case(ffm, ctx, n, unfused=True)
    for name in BYTE_FIELDS + LES_FIELDS:
        assert fused.field(name).tobytes() == plain.field(name).tobytes(), ("start", name)
    for step in range(1, 4):
        fused.step(); plain.step()
        assert _solves(fused) == _solves(plain), step
        for name in BYTE_FIELDS + LES_FIELDS:
            assert fused.field(name).tobytes() == plain.field(name).tobytes(), (step, name)
    fused.close(); plain.close()


def test_model_switched_on_then_off_and_refused_arguments(ffm, ctx):
    n = (12, 16, 12)
    never, case = _gpu_case(ffm, ctx, n, turbulence=False), _gpu_case(ffm, ctx, n, turbulence=False)
    with pytest.raises(ffm.FfmError):
        case.field("k")
    from oracle import plume
    k0 = smooth_k0(plume.make_mesh(n))
    bad_k0 = [k0.copy() for _ in range(3)]
    bad_k0[0][7] = np.nan; bad_k0[1][0] = 0.0; bad_k0[2][-1] = -1e-4
    refused = [dict(Ck=-0.1), dict(Ce=-1.0), dict(Prt=0.0), dict(Prt=-1.0), dict(kInlet=0.0), dict(kInlet=-1e-4), dict(Ck=float("nan")),
               dict(k0=bad_k0[0]), dict(k0=bad_k0[1]), dict(k0=bad_k0[2])]
    for kw in refused:
        with pytest.raises(ffm.FfmError):
            case.set_turbulence(**kw)
    assert ffm.lib().ffm_plume_set_turbulence(case.h, 2, 0.094, 1.048, 1.0, 1e-4, None) != 0       # unknown model
    with pytest.raises(ffm.FfmError):
        case.field("nut")
    never.step(); case.step()                                    # the refusals changed nothing
    for name in BYTE_FIELDS:
        assert case.field(name).tobytes() == never.field(name).tobytes(), ("refused", name)
    assert _solves(case) == _solves(never)
    case.set_turbulence(k0=k0)
    assert case.field("k").tobytes() == k0.tobytes()
    for kw in refused:                                           # ... and with the model on they leave it on and as it was
        with pytest.raises(ffm.FfmError):
            case.set_turbulence(**kw)
    assert case.field("k").tobytes() == k0.tobytes()
    case.set_turbulence(model=None)
    with pytest.raises(ffm.FfmError):
        case.field("k")
    for step in range(2):
        never.step(); case.step()
        assert _solves(case) == _solves(never), step
        for name in BYTE_FIELDS:
            assert case.field(name).tobytes() == never.field(name).tobytes(), (step, name)
    # and the model on does change the step
    case.set_turbulence(k0=k0)
    never.step(); case.step()
    assert case.field("Uy").tobytes() != never.field("Uy").tobytes()
    never.close(); case.close()


def test_three_steps_with_a_poisoned_pool(ffm, ctx):
    n = (12, 16, 12)
    ref = _gpu_case(ffm, ctx, n)
    for _ in range(3):
        ref.step()
    ctx.sync(); ctx.trim()
    ctx.debug_pool_poison(True)
    try:
        case = _gpu_case(ffm, ctx, n)
        for _ in range(3):
            case.step()
        ctx.sync()
    finally:
        ctx.debug_pool_poison(False)
        ctx.trim()
    assert _solves(case) == _solves(ref)
    for name in BYTE_FIELDS + LES_FIELDS:
        f = case.field(name)
        assert np.isfinite(f).all(), name
        assert f.tobytes() == ref.field(name).tobytes(), name
    ref.close(); case.close()
