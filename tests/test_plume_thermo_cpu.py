"""The CPU restatement of the plume step with the janaf thermo and the reference's EDC (tests/plume_thermo_ref.py) and the inputs of
the GPU tests (tests/test_plume_thermo_gpu.py): the conditions those tests rest on, asserted on the restatement alone -- the blob state
reaches both janaf coefficient sets, more than one Newton iteration, both arms of the EDC's min and of its max, never janaf::limit; the
models matter far beyond the parity bound; with every model off the class is PlumeKEqn."""
import numpy as np
import pytest

from common import rel_l2
from plume_keqn_ref import PlumeKEqn, smooth_k0
from plume_thermo_ref import C_DIFF_2, CONFIGS, PlumeThermo, blob_state, ref_case, species

SIZES = [(12, 16, 12), (16, 20, 14)]
STEPS = 4                       # the most any GPU test takes


@pytest.mark.parametrize("n", SIZES)
def test_blob_state_reaches_both_coefficient_sets_both_limits_and_never_the_clamp(O, n):
    ref = ref_case(n, "blob", "thermo+kEqn+EDC")
    mix = ref.mix
    Tc = mix.Tcommon
    moved, o2lim, fuellim = False, False, False
    for step in range(STEPS + 1):
        if step:
            ref.step()
            moved = moved or bool(ref.newton_moved.any())
            o2lim = o2lim or bool(ref.o2_limited.any()); fuellim = fuellim or bool((~ref.o2_limited).any())
            assert ref.wFuel.max() > 0.0, step
        assert (ref.T < Tc).any() and (ref.T > Tc).any(), step                     # both janaf coefficient sets, the branch at Tcommon
        assert (ref.T > ref.mix.Tlow).all() and (ref.T < ref.mix.Thigh).all(), step     # janaf::limit never active
    assert moved                                                                 # thermo::T: more than one iteration in some cell
    assert o2lim and fuellim
    print("T %.1f - %.1f K, %d cells above Tcommon, %d O2-limited" % (ref.T.min(), ref.T.max(), (ref.T > Tc).sum(), ref.o2_limited.sum()))


@pytest.mark.parametrize("n", SIZES)
def test_the_second_edc_set_has_cells_on_both_sides_of_the_max(O, n):
    """C_Diff = 60 (plume_thermo_ref.C_DIFF_2): rtDiff > rtTurb in some cells and rtDiff < rtTurb in others, at the start and after every step"""
    assert CONFIGS["thermo+kEqn+EDC,C_Diff"]["edc"]["C_Diff"] == C_DIFF_2 == 60.0
    ref = ref_case(n, "blob", "thermo+kEqn+EDC,C_Diff")
    ref.combustion_correct()
    for step in range(STEPS + 1):
        if step:
            ref.step()
        assert (ref.rtDiff > ref.rtTurb).any() and (ref.rtDiff < ref.rtTurb).any(), step
    # ... and with C_Diff = 0 the turbulent rate decides everywhere
    ref = ref_case(n, "blob", "thermo+kEqn+EDC")
    ref.step()
    assert (ref.rtDiff == 0.0).all() and (ref.rtTurb > 0.0).all()


@pytest.mark.parametrize("config", list(CONFIGS))
def test_the_models_move_the_step_far_beyond_the_parity_bound(O, config):
    """1e-8 is the parity bound: T, Uy and h of the run with the models differ from the stand-in run's by orders of magnitude more"""
    n = SIZES[0]
    on, off = ref_case(n, "blob", config), ref_case(n, "blob", "thermo", thermo=False)
    assert off.thermo is None and off.edc is None
    for _ in range(STEPS):
        on.step(); off.step()
    assert rel_l2(on.T, off.T) > 1e-4, rel_l2(on.T, off.T)
    assert rel_l2(on.U[1], off.U[1]) > 1e-4, rel_l2(on.U[1], off.U[1])
    assert rel_l2(on.h, off.h) > 1e-6, rel_l2(on.h, off.h)
    assert 1000.0 < on.Cp.min() < 1100.0 and on.Cp.max() > 1200.0, (on.Cp.min(), on.Cp.max())     # one constant Cp it is not


def test_inlet_enthalpy_is_the_mixtures_at_the_inlet_temperature(O):
    from oracle import plume
    ref = ref_case(SIZES[0], "conditioned", "thermo")
    sp = species()
    one = sp.mixture(np.asarray(plume.Y_IN_COND, float))
    assert ref.inlet_enthalpy() == float(one.Hs(0.0, np.array([plume.T_IN]))[0])
    assert abs(float(one.THs(np.array([ref.inlet_enthalpy()]), 0.0, np.array([400.0]))[0]) - plume.T_IN) < 1e-6
    assert abs(ref.inlet_enthalpy() / (plume.CP * (plume.T_IN - plume.TREF)) - 1.0) > 0.05      # not the stand-in's


@pytest.mark.parametrize("turbulence", [False, True])
def test_every_model_off_is_plume_keqn_byte_for_byte(O, turbulence):
    n = SIZES[0]
    a, b = PlumeThermo(n, conditioned=True), PlumeKEqn(n, conditioned=True)
    if turbulence:
        a.set_turbulence(k0=smooth_k0(a.m)); b.set_turbulence(k0=smooth_k0(b.m))
    for _ in range(2):
        a.step(); b.step()
        assert [(nm, sorted(p.items())) for nm, p in a.sol.log] == [(nm, sorted(p.items())) for nm, p in b.sol.log]
        for name, v in b.fields().items():
            assert a.fields()[name].tobytes() == v.tobytes(), name
    # set_state with the conditioned state is the constructor's start, and switching the models on and off again leaves nothing behind
    c = ref_case(n, "conditioned", "thermo+kEqn+EDC" if turbulence else "thermo")
    c.set_combustion(on=False); c.set_thermo(None)
    d = PlumeKEqn(n, conditioned=True)
    if turbulence:
        d.set_turbulence(k0=smooth_k0(d.m))
    c.step(); d.step()
    for name, v in d.fields().items():
        assert c.fields()[name].tobytes() == v.tobytes(), name
