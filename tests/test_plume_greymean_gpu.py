"""The compiled plume step with greyMeanAbsorptionEmission as its absorption / emission model (ffm_plume_set_absorption_emission), on the
box of tests/test_plume_p1_gpu.py (12, 16, 12), 4 steps at solverFreq 2, with kEqn + the janaf thermo + the EDC, for the rays and for P1.

  (a) the fused step (ffm_fvdom_ray_assemble_v_d or ffm_p1_assemble_d with a_d / e_d / a_b, ffm_radiation_sh_greymean_d every step) ==
      the per-operator step (FFM_PLUME_UNFUSED=1: the operator chains and ffm_greymean_a_d, ffm_greymean_E_d, ffm_radiation_sh_v_d) byte
      for byte on every field, aRad, G, ShSu, ShSp (and qr for P1) included, with the same solve records;
  (b) both follow tests/plume_greymean_ref.py: identical iteration counts, every field within 1e-8 (the plume tests' bound);
  (c) the model matters: G differs from the constant-a run's by far more than that bound, so a driver that ignored the handle fails;
  (d) switching off: a handle with the model set and unset -- before its first step and again between steps -- steps bit for bit like
      one that never had it; after a run WITH the model, set_absorption_emission(None) takes aRad away and the next correct() gives
      another G than a twin's that kept the model;
  (e) refusals: a block of a decomposed box FFM_ERR_UNSUPPORTED with a message, a model with other molecular weights FFM_ERR_ARG, no
      radiation model selected FFM_ERR_UNSUPPORTED; the handle then steps like one that never got the call.
Unpinned by reference data: the reference ships no output of a run with this model."""
import numpy as np
import pytest

import plume_greymean_ref as R
from common import rel_l2
from test_plume_multistep_gpu import _compare
from test_plume_thermo_gpu import BYTE_FIELDS, _extra_fields, _gpu_case, _same_steps, _solves, thermo  # noqa: F401  (thermo: the module fixture)

pytestmark = pytest.mark.gpu

N = (12, 16, 12)
CONFIG = "thermo+kEqn+EDC"
UNSUPPORTED, ERR_ARG = -5, -1
RAD_FIELDS = {"rays": ["aRad", "G", "I0", "I13", "I31", "ShSu", "ShSp"], "P1": ["aRad", "G", "qr", "ShSu", "ShSp"]}


@pytest.fixture(scope="module")
def model(ffm, ctx):
    from oracle import plume
    coeffs, order = R.participating()
    gm = ffm.GreyMean(ctx, plume.SPECIES, R.weights(True), coeffs, R.EHRR, order=order)
    yield gm
    gm.close()


def _case(ffm, ctx, which, thermo, gm, unfused=False):  # noqa: F811
    case = _gpu_case(ffm, ctx, N, "blob", CONFIG, thermo, unfused=unfused)
    case.set_radiation_thermo(True)
    if which == "rays":
        case.set_radiation(solverFreq=R.FREQ)
        case.set_radiation_model(*R.RAY_MODEL)
    else:
        case.set_radiation_p1(R.FREQ, *R.P1_MODEL, wallEmissivity=R.EMISSIVITY)
    if gm is not None:
        case.set_absorption_emission(gm)
    return case


@pytest.mark.parametrize("which", ["rays", "P1"])
def test_fused_equals_per_operator_and_both_follow_the_restatement(O, ffm, ctx, thermo, model, which):  # noqa: F811
    fused, plain = _case(ffm, ctx, which, thermo, model), _case(ffm, ctx, which, thermo, model, unfused=True)
    const = _case(ffm, ctx, which, thermo, None)
    ref = R.ref_case(N, which)
    names = BYTE_FIELDS + _extra_fields(CONFIG) + RAD_FIELDS[which]
    with pytest.raises(ffm.FfmError):
        fused.field("aRad")                                       # not evaluated yet
    worst_all = {}
    for step in range(4):
        fused.step(); plain.step(); const.step(); ref.step()
        assert _solves(fused) == _solves(plain), step
        for name in names:
            a = fused.field(name)
            assert np.isfinite(a).all(), (step, name)
            assert a.tobytes() == plain.field(name).tobytes(), (step, name)
        sweep = step % R.FREQ == 0
        solved = [nme for nme, _ in fused.solves()]
        assert (sum(1 for nme in solved if nme.startswith("I")) == 32 if which == "rays" else ("G" in solved)) == sweep, (step, solved)
        f = ref.fields()
        errs = {name: rel_l2(fused.field(name), f[name]) for name in _extra_fields(CONFIG) + [k for k in RAD_FIELDS[which] if not k.startswith("I")]}
        if which == "rays":
            errs.update({"I%d" % i: rel_l2(fused.field("I%d" % i), ref.I[i]) for i in range(32)})
        worst = _compare(step, fused, ref)                        # iteration counts of every solve and the step's fields at 1e-8
        shown = {k: v for k, v in errs.items() if not k.startswith("I")}
        print("%s step %d (%s): %s; worst ray %.2e; worst of the step's fields %.2e" % (
            which, step, "correct() + EEqn" if sweep else "EEqn, no correct()", ", ".join("%s %.2e" % kv for kv in shown.items()),
            max([v for k, v in errs.items() if k.startswith("I")] or [0.0]), worst or 0.0))
        bad = {k: v for k, v in errs.items() if not v < 1e-8}
        assert not bad, (step, bad)
        for k, v in errs.items():
            worst_all[k] = max(worst_all.get(k, 0.0), v)
        # (c) the model matters
        dG = rel_l2(fused.field("G"), const.field("G"))
        assert dG > 1e-3, (step, dG)
    print("%s maxima over 4 steps: %s" % (which, ", ".join("%s %.2e" % kv for kv in worst_all.items() if not kv[0].startswith("I"))))
    a = fused.field("aRad")
    assert a.min() > 0 and a.max() > 2 * a.min()
    # with the model on h keeps its own EEqn in every step: Sh reads a of the species just solved, which five systems assembled
    # together cannot give it (the constant-a handle beside them does take h as the fifth system in steps 1 and 3)
    assert fused.joint_steps() == 0 and plain.joint_steps() == 0 and const.joint_steps() == 2
    for c in (fused, plain, const):
        c.close()


@pytest.mark.parametrize("which", ["rays", "P1"])
def test_switching_off_gives_the_constants_bits(ffm, ctx, thermo, model, which):  # noqa: F811
    """`never` never has the model.  `case` has it set and unset before its first step, and set and unset again between steps: from
    those (equal) states it steps bit for bit like `never`.  Then `case` runs two steps WITH the model beside a twin, is switched off,
    and runs on: aRad is gone, its solves and fields part from the twin's that kept the model (the next sweep's G by far more than 1e-8),
    and it stays finite -- the constant's launches run again.  (No handle without the model can reach the state after a run with it, so
    the bitwise comparison is made at the states both kinds of handle can reach.)"""
    never, case = _case(ffm, ctx, which, thermo, None), _case(ffm, ctx, which, thermo, model)
    case.set_absorption_emission(None)
    names = BYTE_FIELDS + _extra_fields(CONFIG) + [k for k in RAD_FIELDS[which] if k != "aRad"]
    _same_steps(case, never, 2, "model unset before the first step", names)
    case.set_absorption_emission(model); case.set_absorption_emission(None)
    _same_steps(case, never, 2, "model set and unset between steps", names)
    with pytest.raises(ffm.FfmError):
        case.field("aRad")
    never.close(); case.close()
    case, twin = _case(ffm, ctx, which, thermo, model), _case(ffm, ctx, which, thermo, model)
    _same_steps(case, twin, 2, "both with the model", names + ["aRad"])
    case.set_absorption_emission(None)
    case.step(); twin.step()                                      # step 2: a correct()
    with pytest.raises(ffm.FfmError):
        case.field("aRad")
    assert np.isfinite(case.field("G")).all() and rel_l2(case.field("G"), twin.field("G")) > 1e-3
    assert case.field("ShSp").tobytes() != twin.field("ShSp").tobytes()
    case.close(); twin.close()


def test_refusals(ffm, ctx, thermo, model):  # noqa: F811
    from oracle import plume
    L = ffm.lib()
    # no radiation model selected
    bare = _gpu_case(ffm, ctx, N, "blob", CONFIG, thermo)
    assert L.ffm_plume_set_absorption_emission(bare.h, model.h) == UNSUPPORTED
    assert L.ffm_plume_set_absorption_emission(None, model.h) == ERR_ARG
    assert L.ffm_plume_set_absorption_emission(bare.h, None) == 0
    bare.close()
    # other molecular weights than the thermo package's
    coeffs, order = R.participating()
    W = dict(R.weights(True)); W["CO2"] = 44.0
    other = ffm.GreyMean(ctx, plume.SPECIES, W, coeffs, R.EHRR, order=order)
    case, same = _case(ffm, ctx, "rays", thermo, None), _case(ffm, ctx, "rays", thermo, None)
    assert L.ffm_plume_set_absorption_emission(case.h, other.h) == ERR_ARG
    assert b"molecular weights" in L.ffm_last_error()
    with pytest.raises(ffm.FfmError):
        case.set_absorption_emission(other)
    _same_steps(case, same, 2, "model refused", BYTE_FIELDS + ["G", "ShSu", "ShSp"])
    case.close(); same.close(); other.close()


def test_a_decomposed_block_refuses_the_model(ffm, model):
    """the lower x half of the box as rank 0 of 2 in one process, as tests/test_plume_p1_gpu.py builds it (the communicator's callbacks
    play the mirror-image neighbour); the rays are on with the coupling, the setter refuses the handle, NULL stays accepted"""
    own = ffm.Context(0)

    def allreduce(vals, op=0):
        if op == 0:
            vals *= 2.0

    def exchange(sizes, ranks, offs, send, recv):
        recv[:] = send
    own.comm_init_host(0, 2, allreduce, exchange)
    blk = ffm.Plume(own, N, lo=(0, 0, 0), hi=(6, 16, 12), nbrRank=(-1, 1, -1, -1, -1, -1))
    blk.set_radiation(solverFreq=2); blk.set_radiation_model(*R.RAY_MODEL)
    assert ffm.lib().ffm_plume_set_absorption_emission(blk.h, model.h) == UNSUPPORTED
    assert b"decomposed" in ffm.lib().ffm_last_error()
    assert ffm.lib().ffm_plume_set_absorption_emission(blk.h, None) == 0
    with pytest.raises(ffm.FfmError):
        blk.field("aRad")
    blk.close(); own.close()
