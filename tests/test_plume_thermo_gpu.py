"""The compiled plume step with the janaf / sutherland thermo and the reference's EDC (ffm_plume_set_thermo, ffm_plume_set_combustion)
against its CPU restatement (tests/plume_thermo_ref.py), from the start states tests/test_plume_thermo_cpu.py shows the models to
matter on: the conditioned state of oracle/plume.py and the blob state, with the smooth k0 of tests/plume_keqn_ref.py.

  (a) parity: after each of 4 steps every field tests/test_plume_multistep_gpu.py compares, and k, nut, alphat, T, psi, mu, alpha, Cp,
      wFuel, Qdot, within 1e-8 rel-L2 with identical iteration counts of every solve -- not bitwise: exp comes from two maths libraries;
  (b) the fused step == the per-operator step (FFM_PLUME_UNFUSED=1), byte for byte, every field and solve, start + three steps;
  (c) (a)'s second configuration with the solver selection of cases/steckler/system/fvSolution:49-62;
  (d) switching: models set, unset and restarted == a handle that never had them; the two call orders of set_thermo and
      set_initial_state; every refusal leaves the handle as it was;
  (e) three steps with a NaN-poisoned pool equal the unpoisoned run byte for byte.
"""
import os

import numpy as np
import pytest

from common import rel_l2
from oracle import thermo as TH
from plume_keqn_ref import smooth_k0
from plume_thermo_ref import CONFIGS, DATA, STATES, TABLE, ref_case, single_step, start_state
from test_plume_multistep_gpu import FIELDS as STEP_FIELDS, _compare

pytestmark = pytest.mark.gpu

LES_FIELDS = ["k", "nut", "alphat"]
THERMO_FIELDS = ["T", "psi", "mu", "alpha", "Cp"]
SOURCE_FIELDS = ["wFuel", "Qdot"]
BYTE_FIELDS = ["rho", "p", "p_rgh", "T", "h", "Ux", "Uy", "Uz", "O2", "H2O", "C3H8", "CO2", "N2", "K", "psi"]


@pytest.fixture(scope="module")
def thermo(ffm, ctx):
    th = ffm.Thermo(ctx, DATA["species"], TABLE, TH.RR)
    yield th
    th.close()


def _edc_kw(edc):
    rx = single_step()
    return dict(edc, s=rx.s, qFuel=rx.qFuel)


def _gpu_case(ffm, ctx, n, state="blob", config="thermo+kEqn+EDC", thermo=None, unfused=False, steckler=False):
    """the device set up in the restatement's order (plume_thermo_ref.ref_case): start state, kEqn, thermo, EDC; thermo None: the stand-in"""
    from oracle import plume
    cfg = CONFIGS[config]
    if unfused:
        os.environ["FFM_PLUME_UNFUSED"] = "1"
    try:
        case = ffm.Plume(ctx, n)
    finally:
        os.environ.pop("FFM_PLUME_UNFUSED", None)
    if steckler:
        case.set_solvers(True)
    m = plume.make_mesh(n)
    Y0, h0 = start_state(m, state)
    case.set_initial_state(Y0, h0, plume.Y_AMB_COND, plume.Y_IN_COND, plume.H_AMB_COND)
    if cfg["turbulence"]:
        case.set_turbulence(k0=smooth_k0(m))
    if thermo is not None:
        case.set_thermo(thermo)
    if cfg["edc"]:
        case.set_combustion(**_edc_kw(cfg["edc"]))
    return case


def _solves(case):
    return [(name, sorted(pf.items())) for name, pf in case.solves()]


def _extra_fields(config, thermo=True):
    return (LES_FIELDS if CONFIGS[config]["turbulence"] else []) + (THERMO_FIELDS if thermo else []) + SOURCE_FIELDS


def _parity(ffm, ctx, thermo, n, state, config, steps, steckler=False):
    from oracle import plume
    ref = ref_case(n, state, config, solvers=plume.StecklerSolvers() if steckler else None)
    gpu = _gpu_case(ffm, ctx, n, state, config, thermo, steckler=steckler)
    start = THERMO_FIELDS + ["rho", "p"] + (LES_FIELDS if CONFIGS[config]["turbulence"] else [])
    for name in start:                                            # the start-up: thermo.correct(), the hydrostatic start, correctNut()
        assert rel_l2(gpu.field(name), ref.fields()[name]) < 1e-8, ("start", name)
    assert [pf["nIterations"] for _, pf in gpu.solves()] == [pf["nIterations"] for _, pf in ref.sol.log]      # the hydrostatic solves
    extra = _extra_fields(config)
    for step in range(steps):
        ref.step(); gpu.step()
        errs = {name: rel_l2(gpu.field(name), ref.fields()[name]) for name in extra}
        print("step %d: %s" % (step, ", ".join("%s %.2e" % kv for kv in errs.items())))
        worst = _compare(step, gpu, ref)                          # iteration counts of every solve and the step's fields at 1e-8
        print("step %d: worst of %s: %.2e; worst of the models' fields: %.2e" % (step, "/".join(STEP_FIELDS), worst or 0.0, max(errs.values())))
        bad = {k: v for k, v in errs.items() if not v < 1e-8}
        assert not bad, (step, bad)
    gpu.close()


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("n", [(12, 16, 12), (16, 20, 14)])
def test_parity_with_the_restatement_at_1e8(O, ffm, ctx, thermo, n, state, config):
    _parity(ffm, ctx, thermo, n, state, config, 4)


@pytest.mark.parametrize("state", STATES)
def test_parity_with_the_steckler_solver_selection(O, ffm, ctx, thermo, state):
    _parity(ffm, ctx, thermo, (12, 16, 12), state, "thermo+kEqn+EDC", 3, steckler=True)


@pytest.mark.parametrize("config,with_thermo", [("thermo", True), ("thermo+kEqn+EDC", True), ("thermo+kEqn+EDC,C_Diff", True), ("thermo+kEqn+EDC", False)])
def test_fused_step_equals_the_per_operator_step_with_the_models_on(ffm, ctx, thermo, config, with_thermo):
    n = (24, 24, 24)
    th = thermo if with_thermo else None
    fused, plain = _gpu_case(ffm, ctx, n, "blob", config, th), _gpu_case(ffm, ctx, n, "blob", config, th, unfused=True)
    names = BYTE_FIELDS + _extra_fields(config, with_thermo)
    assert _solves(fused) == _solves(plain)                       # the hydrostatic solves
    for name in names:
        if name not in SOURCE_FIELDS:                             # (written by the first step)
            assert fused.field(name).tobytes() == plain.field(name).tobytes(), ("start", name)
    for step in range(1, 4):
        fused.step(); plain.step()
        assert _solves(fused) == _solves(plain), step
        for name in names:
            assert fused.field(name).tobytes() == plain.field(name).tobytes(), (step, name)
    if config == "thermo":
        assert fused.joint_steps() == 3                           # the joint species + h lock-step solve stays available
    fused.close(); plain.close()


def _same_steps(a, b, steps, what, names=BYTE_FIELDS):
    for step in range(steps):
        a.step(); b.step()
        assert _solves(a) == _solves(b), (what, step)
        for name in names:
            assert a.field(name).tobytes() == b.field(name).tobytes(), (what, step, name)


def test_models_set_then_unset_and_restarted_step_as_a_handle_that_never_had_them(ffm, ctx, thermo):
    from oracle import plume
    n = (12, 16, 12)
    never = _gpu_case(ffm, ctx, n, "blob", "thermo", None)
    case = _gpu_case(ffm, ctx, n, "blob", "thermo+kEqn+EDC", thermo)
    for name in THERMO_FIELDS + SOURCE_FIELDS:
        case.field(name)
    case.step(); case.step()
    on_Uy = case.field("Uy")
    case.set_combustion(model=None); case.set_turbulence(model=None)
    Y0, h0 = start_state(plume.make_mesh(n), "blob")
    case.set_initial_state(Y0, h0, plume.Y_AMB_COND, plume.Y_IN_COND, plume.H_AMB_COND)      # restart: set_thermo is allowed again
    case.set_thermo(None)
    for name in ("mu", "alpha", "Cp", "wFuel", "Qdot"):
        with pytest.raises(ffm.FfmError):
            case.field(name)
    for name in BYTE_FIELDS:
        assert case.field(name).tobytes() == never.field(name).tobytes(), ("restart", name)
    _same_steps(case, never, 2, "unset")
    assert on_Uy.tobytes() != never.field("Uy").tobytes()        # ... and the models on do change Uy
    never.close(); case.close()


@pytest.mark.parametrize("config", ["thermo", "thermo+kEqn+EDC"])
def test_set_thermo_then_set_initial_state_gives_the_bytes_of_the_opposite_order(ffm, ctx, thermo, config):
    from oracle import plume
    n = (12, 16, 12)
    a = _gpu_case(ffm, ctx, n, "blob", config, thermo)           # set_initial_state, (set_turbulence,) set_thermo
    b = ffm.Plume(ctx, n)
    m = plume.make_mesh(n)
    if CONFIGS[config]["turbulence"]:
        b.set_turbulence(k0=smooth_k0(m))
    b.set_thermo(thermo)
    Y0, h0 = start_state(m, "blob")
    b.set_initial_state(Y0, h0, plume.Y_AMB_COND, plume.Y_IN_COND, plume.H_AMB_COND)
    if CONFIGS[config]["edc"]:
        b.set_combustion(**_edc_kw(CONFIGS[config]["edc"]))
    names = BYTE_FIELDS + _extra_fields(config)
    assert _solves(a) == _solves(b)
    for name in names:
        if name not in SOURCE_FIELDS:
            assert a.field(name).tobytes() == b.field(name).tobytes(), ("start", name)
    _same_steps(a, b, 2, "order", names)
    a.close(); b.close()


def test_refusals_leave_the_handle_as_it_was(ffm, ctx, thermo):
    n = (12, 16, 12)
    rx = single_step()
    L = ffm.lib()
    # ---- a handle with the stand-ins: a wrong species table, EDC without kEqn, bad EDC arguments, thermo after radiation
    plain, case = _gpu_case(ffm, ctx, n, "blob", "thermo", None), _gpu_case(ffm, ctx, n, "blob", "thermo", None)
    four = ffm.Thermo(ctx, DATA["species"][:4], TABLE, TH.RR)
    swapped = ffm.Thermo(ctx, DATA["species"][::-1], TABLE, TH.RR)
    for th in (four, swapped):
        with pytest.raises(ffm.FfmError):
            case.set_thermo(th)
    with pytest.raises(ffm.FfmError):
        case.set_combustion(s=rx.s, qFuel=rx.qFuel)                              # EDC without kEqn
    assert L.ffm_plume_set_combustion(case.h, 1, 4.0, 0.0, 1.0, rx.s, rx.qFuel) == -5       # FFM_ERR_UNSUPPORTED
    assert L.ffm_plume_set_thermo(case.h, four.h) == -1                                     # FFM_ERR_ARG
    _same_steps(case, plain, 1, "refused on a plain handle")
    with pytest.raises(ffm.FfmError):
        case.set_thermo(thermo)                                                  # after a step
    with pytest.raises(ffm.FfmError):
        case.field("Cp")
    _same_steps(case, plain, 1, "set_thermo after a step")
    plain.close(); case.close()
    # ---- radiation first, then thermo
    rad, case = _gpu_case(ffm, ctx, n, "blob", "thermo", None), _gpu_case(ffm, ctx, n, "blob", "thermo", None)
    for c in (rad, case):
        c.set_radiation(solverFreq=2)
    with pytest.raises(ffm.FfmError):
        case.set_thermo(thermo)
    assert L.ffm_plume_set_thermo(case.h, thermo.h) == -5                                    # FFM_ERR_UNSUPPORTED
    _same_steps(case, rad, 2, "thermo after radiation")
    rad.close(); case.close()
    # ---- a handle with every model on: radiation after thermo, kEqn off under EDC, every bad EDC argument, an unknown model
    full, case = _gpu_case(ffm, ctx, n, "blob", "thermo+kEqn+EDC", thermo), _gpu_case(ffm, ctx, n, "blob", "thermo+kEqn+EDC", thermo)
    with pytest.raises(ffm.FfmError):
        case.set_radiation(solverFreq=2)
    with pytest.raises(ffm.FfmError):
        case.set_radiation_model(0.1, 0.5, 0.22)
    with pytest.raises(ffm.FfmError):
        case.set_turbulence(model=None)
    assert L.ffm_plume_set_radiation(case.h, 2, 2, 4, None, None) == -5 and L.ffm_plume_set_turbulence(case.h, 0, 0.094, 1.048, 1.0, 1e-4, None) == -5
    good = dict(C_EDC=4.0, C_Diff=0.0, C_Stiff=1.0, s=rx.s, qFuel=rx.qFuel)
    bad = [dict(s=0.0), dict(s=-1.0), dict(C_Stiff=0.0), dict(C_Stiff=-1.0), dict(C_EDC=-1.0), dict(C_Diff=-1.0), dict(qFuel=0.0), dict(qFuel=-1.0)]
    bad += [{key: v} for key in good for v in (float("nan"), float("inf"))]
    for kw in bad:
        with pytest.raises(ffm.FfmError):
            case.set_combustion(**dict(good, **kw))
    assert L.ffm_plume_set_combustion(case.h, 2, 4.0, 0.0, 1.0, rx.s, rx.qFuel) != 0          # unknown model
    _same_steps(case, full, 2, "refused with the models on", BYTE_FIELDS + _extra_fields("thermo+kEqn+EDC"))
    full.close(); case.close(); four.close(); swapped.close()


def test_three_steps_with_a_poisoned_pool(ffm, ctx, thermo):
    n = (12, 16, 12)
    ref = _gpu_case(ffm, ctx, n, "blob", "thermo+kEqn+EDC", thermo)
    for _ in range(3):
        ref.step()
    ctx.sync(); ctx.trim()
    ctx.debug_pool_poison(True)
    try:
        case = _gpu_case(ffm, ctx, n, "blob", "thermo+kEqn+EDC", thermo)
        for _ in range(3):
            case.step()
        ctx.sync()
    finally:
        ctx.debug_pool_poison(False)
        ctx.trim()
    assert _solves(case) == _solves(ref)
    for name in BYTE_FIELDS + _extra_fields("thermo+kEqn+EDC"):
        f = case.field(name)
        assert np.isfinite(f).all(), name
        assert f.tobytes() == ref.field(name).tobytes(), name
    ref.close(); case.close()
