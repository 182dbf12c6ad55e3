"""The compiled plume step with the P1 radiation model (ffm_plume_set_radiation_p1) in place of the rays.

  (a) the fused step (ffm_p1_assemble_d, ffm_p1_wall_flux_d) == the per-operator step (FFM_PLUME_UNFUSED=1: the chain of entry points they
      restate) byte for byte over 4 steps with solverFreq 2: every field of tests/test_fused_gpu.py's FIELDS plus G, qr, ShSu, ShSp, and the
      iteration count of every solve, the G solve included -- at (12, 16, 12) and at (40, 36, 33) (several tiles);
  (b) against the CPU restatement tests/plume_p1_ref.py over 4 steps: identical iteration counts, every field within 1e-8 rel-L2;
  (c) off means unchanged: a handle with set_radiation_p1(0, ...) and a fresh one give the same bytes and the same solve records;
  (d) refusals: the rays on, then P1 (and the other way round) -- FFM_ERR_UNSUPPORTED, and the handle steps like one that never got
      the call; a block of a decomposed box -- FFM_ERR_UNSUPPORTED."""
import os

import numpy as np
import pytest

from common import rel_l2
from plume_p1_ref import P1_FREQ, P1_MODEL, ref_case
from plume_thermo_ref import start_state
from test_plume_multistep_gpu import _compare

pytestmark = pytest.mark.gpu

FIELDS = ["rho", "p", "p_rgh", "T", "h", "Ux", "Uy", "Uz", "O2", "H2O", "C3H8", "CO2", "N2", "K"]      # tests/test_fused_gpu.py's
P1_FIELDS = ["G", "qr", "ShSu", "ShSp"]
UNSUPPORTED = -5
EMISSIVITY = 0.8


def _case(ffm, ctx, n, unfused=False, state="blob"):
    from oracle import plume
    if unfused:
        os.environ["FFM_PLUME_UNFUSED"] = "1"
    try:
        case = ffm.Plume(ctx, n)
    finally:
        os.environ.pop("FFM_PLUME_UNFUSED", None)
    Y0, h0 = start_state(plume.make_mesh(n), state)
    case.set_initial_state(Y0, h0, plume.Y_AMB_COND, plume.Y_IN_COND, plume.H_AMB_COND)
    return case


def _solves(case):
    return [(name, sorted(pf.items())) for name, pf in case.solves()]


def _same_steps(a, b, steps, what, names):
    for step in range(steps):
        a.step(); b.step()
        assert _solves(a) == _solves(b), (what, step)
        for name in names:
            assert a.field(name).tobytes() == b.field(name).tobytes(), (what, step, name)


@pytest.mark.parametrize("n", [(12, 16, 12), (40, 36, 33)])
def test_fused_step_equals_the_per_operator_step_with_p1(ffm, ctx, n):
    fused, plain = _case(ffm, ctx, n), _case(ffm, ctx, n, unfused=True)
    for c in (fused, plain):
        c.set_radiation_p1(P1_FREQ, *P1_MODEL, wallEmissivity=EMISSIVITY)
    for step in range(4):
        fused.step(); plain.step()
        its = [(a, p["nIterations"]) for a, p in fused.solves()]
        assert its == [(a, p["nIterations"]) for a, p in plain.solves()], step
        assert sum(1 for a, _ in its if a == "G") == (1 if step % P1_FREQ == 0 else 0), (step, its)
        for name in FIELDS + P1_FIELDS:
            a = fused.field(name)
            assert np.isfinite(a).all(), (step, name)
            assert np.array_equal(a, plain.field(name)), (step, name)
    assert np.abs(fused.field("G")).min() > 0.0 and np.abs(fused.field("qr")).max() > 0.0 and np.abs(fused.field("ShSp")).min() > 0.0
    assert fused.joint_steps() == 2 and plain.joint_steps() == 0      # steps 1 and 3 have no correct(): h is the fifth lock-step system
    fused.close(); plain.close()


def test_parity_with_the_restatement_at_1e8(O, ffm, ctx):
    n = (12, 16, 12)
    ref = ref_case(n, wallEmissivity=EMISSIVITY)
    gpu = _case(ffm, ctx, n)
    gpu.set_radiation_p1(P1_FREQ, *P1_MODEL, wallEmissivity=EMISSIVITY)
    with pytest.raises(ffm.FfmError):
        gpu.field("qr")                                           # no correct() yet
    worst_all = {}
    for step in range(4):
        ref.step(); gpu.step()
        f = ref.fields()
        errs = {name: rel_l2(gpu.field(name), f[name]) for name in P1_FIELDS}
        worst = _compare(step, gpu, ref)                          # iteration counts of every solve (G among them) and the step's fields at 1e-8
        print("step %d (%s): %s; worst of the step's fields %.2e" % (step, "P1 solve + EEqn" if step % P1_FREQ == 0 else "five systems",
                                                                    ", ".join("%s %.2e" % kv for kv in errs.items()), worst or 0.0))
        assert ("G" in [nme for nme, _ in gpu.solves()]) == (step % P1_FREQ == 0)
        bad = {k: v for k, v in errs.items() if not v < 1e-8}
        assert not bad, (step, bad)
        for k, v in list(errs.items()) + [("step fields", worst or 0.0)]:
            worst_all[k] = max(worst_all.get(k, 0.0), v)
    print("maxima over 4 steps: " + ", ".join("%s %.2e" % kv for kv in worst_all.items()))
    gpu.close()


def test_off_means_unchanged(ffm, ctx):
    n = (12, 16, 12)
    fresh, off = _case(ffm, ctx, n), _case(ffm, ctx, n)
    off.set_radiation_p1(0, *P1_MODEL, wallEmissivity=EMISSIVITY)
    _same_steps(off, fresh, 3, "P1 off", FIELDS)
    assert all(nme != "G" for nme, _ in off.solves())
    with pytest.raises(ffm.FfmError):
        off.field("G")
    fresh.close(); off.close()


def test_p1_and_the_rays_refuse_each_other(ffm, ctx):
    n = (12, 16, 12)
    L = ffm.lib()
    # ---- the rays on, then P1
    rays, case = _case(ffm, ctx, n), _case(ffm, ctx, n)
    for c in (rays, case):
        c.set_radiation(solverFreq=2); c.set_radiation_model(0.1, 0.3, 0.3)
    assert L.ffm_plume_set_radiation_p1(case.h, 2, 0.1, 0.3, 0.3, 1.0) == UNSUPPORTED
    with pytest.raises(ffm.FfmError):
        case.set_radiation_p1(2, 0.1, 0.3, 0.3)
    _same_steps(case, rays, 2, "P1 refused", FIELDS + ["G", "I0", "I31", "ShSu", "ShSp"])
    rays.close(); case.close()
    # ---- P1 on, then the rays
    p1, case = _case(ffm, ctx, n), _case(ffm, ctx, n)
    for c in (p1, case):
        c.set_radiation_p1(P1_FREQ, *P1_MODEL, wallEmissivity=EMISSIVITY)
    assert L.ffm_plume_set_radiation(case.h, 2, 2, 4, None, None) == UNSUPPORTED
    with pytest.raises(ffm.FfmError):
        case.set_radiation(solverFreq=2)
    _same_steps(case, p1, 2, "rays refused", FIELDS + P1_FIELDS)
    p1.close(); case.close()
    # ---- bad arguments
    case = _case(ffm, ctx, n)
    assert L.ffm_plume_set_radiation_p1(None, 1, 0.1, 0.3, 0.3, 1.0) == -1
    assert L.ffm_plume_set_radiation_p1(case.h, -1, 0.1, 0.3, 0.3, 1.0) == -1
    assert L.ffm_plume_set_radiation_p1(case.h, 1, -0.1, 0.3, 0.3, 1.0) == -1
    assert L.ffm_plume_set_radiation_p1(case.h, 1, 0.1, 0.3, 0.3, 1.5) == -1
    case.close()


def test_a_decomposed_handle_refuses_p1(ffm):
    """the lower x half of the box as rank 0 of 2, in ONE process: the communicator's callbacks play a neighbour that is this block's
    mirror image (what it sends comes back as the ghost values; a sum over the ranks is twice this rank's share), which is all the
    hydrostatic start-up of the block needs.  The setter refuses the handle; off stays accepted."""
    own = ffm.Context(0)                                          # a context of its own: the communicator stays off the shared one

    def allreduce(vals, op=0):
        if op == 0:
            vals *= 2.0

    def exchange(sizes, ranks, offs, send, recv):
        recv[:] = send
    own.comm_init_host(0, 2, allreduce, exchange)
    blk = ffm.Plume(own, (12, 16, 12), lo=(0, 0, 0), hi=(6, 16, 12), nbrRank=(-1, 1, -1, -1, -1, -1))
    assert ffm.lib().ffm_plume_set_radiation_p1(blk.h, 2, 0.1, 0.3, 0.3, 1.0) == UNSUPPORTED
    assert b"decomposed" in ffm.lib().ffm_last_error()
    assert ffm.lib().ffm_plume_set_radiation_p1(blk.h, 0, 0.1, 0.3, 0.3, 1.0) == 0        # off is off everywhere
    with pytest.raises(ffm.FfmError):
        blk.field("qr")
    blk.close(); own.close()
