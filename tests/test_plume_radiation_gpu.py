"""The compiled plume step with the fvDOM rays and radiation->Sh TOGETHER with the janaf / sutherland thermo and the reference's EDC
(ffm_plume_set_radiation_thermo) against its CPU restatement (tests/plume_radiation_ref.py); modelled on tests/test_plume_thermo_gpu.py,
whose device set-up, field lists and start states it shares.  tests/test_plume_radiation_cpu.py shows that these inputs cannot be met
with the constant Cp the source pass had: ShSp moves by 0.76, ShSu by 1.7e-2, h after step 2 by 3e-6 rel-L2.

  (a) parity: 4 steps with solverFreq 2 -- steps 0 and 2 a ray sweep and the separate EEqn, steps 1 and 3 h as the fifth lock-step system
      with the Sh source -- every field tests/test_plume_thermo_gpu.py compares plus ShSu, ShSp within 1e-8 rel-L2, identical iteration
      counts of every solve; G and the rays within the bound of tests/test_plume_gpu.py's coupled-radiation test (rtol there);
  (b) the fused step == the per-operator step (FFM_PLUME_UNFUSED=1) byte for byte: every field, G, I0, I13, I31, ShSu, ShSp, every solve
      record, at (24,24,24) over the start and 3 steps -- with the thermo package and, the constant-Cp path having the same new launches,
      without it;
  (c) switching: both call orders of set_thermo and set_radiation* give the same bytes; switch on and thermo off == a handle without the
      switch; the switch cannot be turned off with both on; without it the three radiation setters return -5 as before;
  (d) 3 steps with a NaN-poisoned pool equal the unpoisoned run byte for byte.
"""
import numpy as np
import pytest

from common import rel_l2
from plume_radiation_ref import RAD_FREQ, RAD_MODEL, ref_case
from plume_thermo_ref import CONFIGS, STATES
from test_plume_multistep_gpu import _compare
from test_plume_thermo_gpu import (BYTE_FIELDS, LES_FIELDS, THERMO_FIELDS, _extra_fields, _gpu_case, _same_steps, _solves,
                                   thermo)  # noqa: F401  (thermo: the module fixture)

pytestmark = pytest.mark.gpu

RAD_FIELDS = ["G", "I0", "I13", "I31", "ShSu", "ShSp"]
UNSUPPORTED = -5


def _rad_case(ffm, ctx, n, state, config, thermo, unfused=False, rays=None, order="thermo first"):  # noqa: F811
    """tests/test_plume_thermo_gpu.py's device case with the switch on and the radiation of plume_radiation_ref.ref_case.  order: the
    thermo package before the radiation setters (as the restatement) or after them"""
    if order == "thermo first" or thermo is None:
        case = _gpu_case(ffm, ctx, n, state, config, thermo, unfused=unfused)
        case.set_radiation_thermo(True)
        case.set_radiation(solverFreq=RAD_FREQ, rays=rays)
        case.set_radiation_model(*RAD_MODEL)
        return case
    from test_plume_thermo_gpu import _edc_kw
    case = _gpu_case(ffm, ctx, n, state, config, None, unfused=unfused)       # start state, kEqn, (EDC: needs kEqn only)
    case.set_radiation_thermo(True)
    case.set_radiation_model(*RAD_MODEL)
    case.set_radiation(solverFreq=RAD_FREQ, rays=rays)
    case.set_radiation_ordering(0)
    case.set_thermo(thermo)
    if CONFIGS[config]["edc"]:
        case.set_combustion(**_edc_kw(CONFIGS[config]["edc"]))
    return case


@pytest.mark.parametrize("config", ["thermo", "thermo+kEqn+EDC"])
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("n", [(12, 16, 12), (16, 20, 14)])
def test_parity_with_the_restatement_at_1e8(O, ffm, ctx, thermo, n, state, config):  # noqa: F811
    ref = ref_case(n, state, config)
    gpu = _rad_case(ffm, ctx, n, state, config, thermo, rays=ref.rays)
    for name in THERMO_FIELDS + ["rho", "p"] + (LES_FIELDS if CONFIGS[config]["turbulence"] else []):
        assert rel_l2(gpu.field(name), ref.fields()[name]) < 1e-8, ("start", name)
    with pytest.raises(ffm.FfmError):
        gpu.field("ShSu")                                         # no source pass yet
    extra = _extra_fields(config) + ["ShSu", "ShSp"]
    for step in range(4):
        ref.step(); gpu.step()
        sweep = step % RAD_FREQ == 0
        names = [nme for nme, _ in gpu.solves()]
        assert sum(1 for nme in names if nme.startswith("I")) == (32 if sweep else 0), step
        f = ref.fields()
        errs = {name: rel_l2(gpu.field(name), f[name]) for name in extra}
        # the bound of tests/test_plume_gpu.py::test_plume_with_the_reference_radiation_model_coupled_into_h on G and the rays
        tol = 1e-8 if step == 0 else 1e-5
        rtol = 1e-11 if step < 2 else 1e-3 * tol                  # the rays see T^4 of the step before
        rerr = {"I%d" % i: rel_l2(gpu.field("I%d" % i), ref.I[i]) for i in range(32)}
        rerr["G"] = rel_l2(gpu.field("G"), ref.G)
        print("step %d (%s): %s" % (step, "sweep + EEqn" if sweep else "five systems", ", ".join("%s %.2e" % kv for kv in errs.items())))
        print("step %d: G %.2e, worst ray %.2e (bound %.0e)" % (step, rerr["G"], max(v for k, v in rerr.items() if k != "G"), rtol))
        worst = _compare(step, gpu, ref)                          # iteration counts of every solve and the step's fields at 1e-8
        print("step %d: worst of the step's fields %.2e" % (step, worst or 0.0))
        bad = {k: v for k, v in errs.items() if not v < 1e-8}
        assert not bad, (step, bad)
        bad = {k: v for k, v in rerr.items() if not v < rtol}
        assert not bad, (step, rtol, bad)
    assert gpu.joint_steps() == 2                                 # steps 1 and 3: h was the fifth system
    gpu.close()


@pytest.mark.parametrize("config,with_thermo", [("thermo", True), ("thermo+kEqn+EDC", True), ("thermo+kEqn+EDC", False)])
def test_fused_step_equals_the_per_operator_step_with_radiation(ffm, ctx, thermo, config, with_thermo):  # noqa: F811
    n = (24, 24, 24)
    th = thermo if with_thermo else None
    fused, plain = _rad_case(ffm, ctx, n, "blob", config, th), _rad_case(ffm, ctx, n, "blob", config, th, unfused=True)
    names = BYTE_FIELDS + _extra_fields(config, with_thermo)
    assert _solves(fused) == _solves(plain)                       # the hydrostatic solves
    for name in BYTE_FIELDS + (THERMO_FIELDS if with_thermo else []):
        assert fused.field(name).tobytes() == plain.field(name).tobytes(), ("start", name)
    for step in range(1, 4):
        fused.step(); plain.step()
        assert _solves(fused) == _solves(plain), step
        for name in names + RAD_FIELDS:
            a = fused.field(name)
            assert np.isfinite(a).all(), (step, name)
            assert a.tobytes() == plain.field(name).tobytes(), (step, name)
    assert np.abs(fused.field("G")).min() > 0.0 and np.abs(fused.field("ShSp")).min() > 0.0
    assert fused.joint_steps() == 1 and plain.joint_steps() == 0  # the second of the three steps has no sweep
    fused.close(); plain.close()


def test_call_orders_of_set_thermo_and_the_radiation_setters_give_the_same_bytes(ffm, ctx, thermo):  # noqa: F811
    n, config = (12, 16, 12), "thermo+kEqn+EDC"
    a = _rad_case(ffm, ctx, n, "blob", config, thermo)
    b = _rad_case(ffm, ctx, n, "blob", config, thermo, order="radiation first")
    names = BYTE_FIELDS + _extra_fields(config)
    assert _solves(a) == _solves(b)
    for name in BYTE_FIELDS + THERMO_FIELDS:
        assert a.field(name).tobytes() == b.field(name).tobytes(), ("start", name)
    _same_steps(a, b, 3, "order", names + RAD_FIELDS)
    a.close(); b.close()


def test_switch_on_and_thermo_off_is_a_handle_without_the_switch(ffm, ctx):
    n, config = (12, 16, 12), "thermo+kEqn+EDC"
    never = _gpu_case(ffm, ctx, n, "blob", config, None)
    never.set_radiation(solverFreq=RAD_FREQ); never.set_radiation_model(*RAD_MODEL)
    case = _rad_case(ffm, ctx, n, "blob", config, None)
    _same_steps(case, never, 3, "switch without thermo", BYTE_FIELDS + _extra_fields(config, False) + RAD_FIELDS)
    case.set_radiation_thermo(False)                              # thermo off: allowed, and nothing moves
    _same_steps(case, never, 1, "switch off again", BYTE_FIELDS + RAD_FIELDS)
    never.close(); case.close()


def test_refusals_with_and_without_the_switch(ffm, ctx, thermo):  # noqa: F811
    n, config = (12, 16, 12), "thermo+kEqn+EDC"
    L = ffm.lib()
    # ---- both on: the switch cannot be turned off, and the handle steps as its twin
    full, case = _rad_case(ffm, ctx, n, "blob", config, thermo), _rad_case(ffm, ctx, n, "blob", config, thermo)
    with pytest.raises(ffm.FfmError):
        case.set_radiation_thermo(False)
    assert L.ffm_plume_set_radiation_thermo(case.h, 0) == UNSUPPORTED
    assert L.ffm_plume_set_radiation_thermo(None, 1) == -1
    _same_steps(case, full, 2, "switch off refused", BYTE_FIELDS + _extra_fields(config) + RAD_FIELDS)
    full.close(); case.close()
    # ---- without the switch: the three setters refuse a handle with the thermo package, as before
    plain, case = _gpu_case(ffm, ctx, n, "blob", config, thermo), _gpu_case(ffm, ctx, n, "blob", config, thermo)
    assert L.ffm_plume_set_radiation(case.h, 2, 2, 4, None, None) == UNSUPPORTED
    assert L.ffm_plume_set_radiation_model(case.h, 0.1, 0.5, 0.22) == UNSUPPORTED
    assert L.ffm_plume_set_radiation_ordering(case.h, 0) == UNSUPPORTED
    with pytest.raises(ffm.FfmError):
        case.field("G")
    _same_steps(case, plain, 2, "refused without the switch", BYTE_FIELDS + _extra_fields(config))
    plain.close(); case.close()
    # ---- ... and set_thermo a handle with rays
    case = _gpu_case(ffm, ctx, n, "blob", config, None)
    case.set_radiation(solverFreq=RAD_FREQ)
    assert L.ffm_plume_set_thermo(case.h, thermo.h) == UNSUPPORTED
    case.close()


def test_three_steps_with_a_poisoned_pool(ffm, ctx, thermo):  # noqa: F811
    n, config = (12, 16, 12), "thermo+kEqn+EDC"
    ref = _rad_case(ffm, ctx, n, "blob", config, thermo)
    for _ in range(3):
        ref.step()
    ctx.sync(); ctx.trim()
    ctx.debug_pool_poison(True)
    try:
        case = _rad_case(ffm, ctx, n, "blob", config, thermo)
        for _ in range(3):
            case.step()
        ctx.sync()
    finally:
        ctx.debug_pool_poison(False)
        ctx.trim()
    assert _solves(case) == _solves(ref)
    for name in BYTE_FIELDS + _extra_fields(config) + RAD_FIELDS:
        f = case.field(name)
        assert np.isfinite(f).all(), name
        assert f.tobytes() == ref.field(name).tobytes(), name
    ref.close(); case.close()
