"""csrc/ffm_pyro.hip at its template and range edges, against oracle/pyrolysis.py and tests/pyro_incident_ref.py: every layer count the
kernels are instantiated for (2: no interior row, the first row is the last; 16: the `default:` label, the largest register arrays) and
the refusal of 1 and 17; another material and another reaction (ffm_pyro_set_solids, ffm_pyro_set_reaction with a reaction that runs);
a partly charred start, also below the 0.001 floor of c0; a burnt-out column (Yw clipped to exactly 0).  Panels of 70 columns: two
waves, the second ragged.  Inputs: tests/physics_edge_inputs.py, whose edges tests/test_physics_edge_inputs_cpu.py checks on the
oracle.  Tolerances as tests/test_pyrolysis_gpu.py: 1e-11 of the field's maximum (device exp / pow against libm), phiGas 1e-10; a run
inside one launch against single steps is bitwise."""
import numpy as np
import pytest

import physics_edge_inputs as E

pytestmark = pytest.mark.gpu

FIELDS = ("rho", "Yw", "T", "h", "alpha")
NCOL = 70
GEO = dict(thickness=0.0127, area=0.01)
SEL21 = dict(model="reactingOneDim21", alphaScheme="harmonic", kappaScheme="harmonic", back=("constH", 25.0, 298.15))


def _compare(dev, ref, what, tol=1e-11):
    for name in FIELDS:
        r, d = getattr(ref, name), dev.field(name)
        err = np.abs(d - r).max() / max(np.abs(r).max(), 1e-300)
        print("%s %s: %.2e" % (what, name, err))
        assert err <= tol, (what, name, err)
    errg = np.abs(dev.field("phiGas") - ref.massGas).max() / max(np.abs(ref.massGas).max(), 1e-300)
    print("%s phiGas: %.2e" % (what, errg))
    assert errg <= 1e-10, (what, errg)
    assert np.abs(dev.field("Tsurf") - ref.T[:, 0]).max() <= tol * np.abs(ref.T).max(), what


def _run_given_flux(ffm, ctx, nLay, sel, nSteps=600):
    from oracle import pyrolysis as PY
    ref = PY.Panel(NCOL, nLay, **GEO, **sel)
    dev = ffm.PyrolysisPanel(ctx, NCOL, nLay, **GEO)
    if sel:
        dev.set_model(**sel)
    q = E.column_flux(NCOL); qd = ctx.to_device(q)
    gas = np.zeros(NCOL); m0 = (ref.rho * ref.V).sum(axis=1)
    for step in range(nSteps):
        ref.step(0.05, q); dev.step(0.05, qd)
        if step % 100 == 99 or step == 0:
            _compare(dev, ref, "nLay=%d step %d" % (nLay, step))
        gas += dev.field("phiGas") * 0.05
    assert ref.Yw.min() < 0.5                                   # the run reached charring
    assert np.allclose(m0 - (dev.field("rho") * ref.V).sum(axis=1), gas, rtol=1e-9)
    dev.close()


@pytest.mark.parametrize("nLay", range(2, 17))
def test_every_layer_count_matches_oracle(ffm, ctx, nLay):
    _run_given_flux(ffm, ctx, nLay, {})


@pytest.mark.parametrize("nLay", [2, 3, 16])
def test_model21_harmonic_and_constH_back_at_the_end_layer_counts(ffm, ctx, nLay):
    """with 2 layers the exposed and the back condition act on adjacent rows"""
    _run_given_flux(ffm, ctx, nLay, SEL21)


def _incident(ffm, ctx, nLay, qr):
    import pyro_incident_ref as R
    case = R.case_data()
    sel = R.case_selections(case)
    geo = dict(thickness=case["pyrolysis"]["thickness"], area=0.01, T0=case["panelT"]["internalField"])
    Qr = 3.0e4 + 6.0e4 * np.sin(0.37 * np.arange(NCOL)) ** 2
    qr0 = 2.0e4 * np.cos(0.11 * np.arange(NCOL)) - 2.0e3 if qr else None      # some columns emit: clipped to no source
    ref = R.IncidentPanel(NCOL, nLay, QrIncident=Qr, qr0=qr0, **geo, **sel)
    dev = ffm.PyrolysisPanel(ctx, NCOL, nLay, **geo)
    dev.set_model(**sel)
    dev.set_incident_radiation(Qr)
    if qr:
        dev.set_qr_source(qr0)
    return ref, dev, E.incident_deltaT(case["controls"]["deltaT"], nLay)


@pytest.mark.parametrize("qr", [False, True])
@pytest.mark.parametrize("nLay", [2, 3, 15, 16])
def test_step_incident_at_the_end_layer_counts(ffm, ctx, nLay, qr):
    ref, dev, dt = _incident(ffm, ctx, nLay, qr)
    n = int(round(80.0 / dt))                                   # 80 s: through the charring of the exposed layers
    for step in range(n):
        ref.step_incident(dt); dev.step_incident(dt)
        if step % (n // 4) == n // 4 - 1 or step == 0:
            _compare(dev, ref, "incident nLay=%d qr=%d step %d" % (nLay, qr, step))
            for name in ("Twall", "qSurf"):
                r, d = getattr(ref, name), dev.field(name)
                assert np.abs(d - r).max() <= 1e-11 * np.abs(r).max(), (step, name)
    assert ref.Yw.min() < 0.5
    dev.close()


@pytest.mark.parametrize("qr", [False, True])
@pytest.mark.parametrize("nLay", [2, 16])
def test_run_incident_is_bitwise_the_stepped_run_and_its_history_the_restatement(ffm, ctx, nLay, qr):
    ref, stepped, dt = _incident(ffm, ctx, nLay, qr)
    every = int(round(2.0 / dt)); nSteps = 10 * every + 3 * every // 10     # 20.6 s; the last steps give no sample
    assert nSteps % every != 0
    _, one, _ = _incident(ffm, ctx, nLay, qr)
    samples = []
    for s in range(nSteps):
        stepped.step_incident(dt)
        if (s + 1) % every == 0:
            samples.append({k: stepped.field(k) for k in ("Twall", "phiGas", "T", "rho", "Yw")})
    H = one.run_incident(dt, nSteps, sampleEvery=every)
    for k in FIELDS + ("Twall", "qSurf", "phiGas", "Tsurf"):
        assert np.array_equal(one.field(k), stepped.field(k)), k
    nS = nSteps // every
    assert nS == 10 and len(samples) == nS
    assert H["Twall"].shape == H["phiGas"].shape == (nS, NCOL)
    assert all(H[k].shape == (nS, NCOL, nLay) for k in ("T", "rho", "Yw", "chemistryQdot"))     # (nS, 2 + 4 nLay, nCol) on the device
    for i, smp in enumerate(samples):
        for k, v in smp.items():
            assert np.array_equal(H[k][i], v), (i, k)
    Hr = ref.run_incident(dt, nSteps, sampleEvery=every)
    for k in ("Twall", "T", "rho", "Yw"):
        assert Hr[k].shape == H[k].shape
        assert np.abs(H[k] - Hr[k]).max() <= 1e-11 * np.abs(Hr[k]).max(), k
    assert np.abs(H["phiGas"] - Hr["phiGas"]).max() <= 1e-10 * max(Hr["phiGas"].max(), 1e-300)
    # chemistryQdot relative to the layer's largest: a rate of exp and pow, as phiGas
    assert np.abs(H["chemistryQdot"] - Hr["chemistryQdot"]).max() <= 1e-10 * max(np.abs(Hr["chemistryQdot"]).max(), 1e-300)
    assert np.abs(Hr["chemistryQdot"]).max() > 0
    stepped.close(); one.close()


@pytest.mark.parametrize("nLay", [1, 17])
def test_layer_counts_outside_the_instantiated_range_are_refused(ffm, ctx, nLay):
    import ctypes as C
    from oracle import pyrolysis as PY
    h = C.c_void_p()
    assert ffm.lib().ffm_pyro_create(ctx.h, NCOL, nLay, 0.0127, 0.01, 298.15, 1.0, C.byref(h)) == -1      # FFM_ERR_ARG
    assert not h.value
    with pytest.raises(ffm.FfmError, match=r"ffm_pyro_create failed \(-1\)"):
        ffm.PyrolysisPanel(ctx, NCOL, nLay, **GEO)
    # a panel created on the same context afterwards steps correctly
    ref = PY.Panel(NCOL, 4, **GEO, T0=600.0); dev = ffm.PyrolysisPanel(ctx, NCOL, 4, **GEO, T0=600.0)
    q = E.column_flux(NCOL); qd = ctx.to_device(q)
    for step in range(20):
        ref.step(0.05, q); dev.step(0.05, qd)
    _compare(dev, ref, "after the refusal of %d layers" % nLay)
    assert ref.massGas.max() > 0
    dev.close()


@pytest.mark.parametrize("sel", [{}, SEL21])
def test_other_material_and_reaction(ffm, ctx, sel):
    """ffm_pyro_set_solids and ffm_pyro_set_reaction with a reaction that runs: the start state follows the solids (rho, h, alpha, and
    c0 through the reacting steps), then 300 steps through the charring of a material with a char heat of formation"""
    from oracle import pyrolysis as PY
    mat = dict(wood=E.OTHER_WOOD, char=E.OTHER_CHAR, reaction=E.OTHER_REACTION)
    ref = PY.Panel(NCOL, 8, **GEO, T0=320.0, **sel, **mat)
    dev = ffm.PyrolysisPanel(ctx, NCOL, 8, **GEO, T0=320.0)
    if sel:
        dev.set_model(**sel)
    wood_state = {k: dev.field(k) for k in FIELDS}
    dev.set_solids(E.solid4(E.OTHER_WOOD), E.solid4(E.OTHER_CHAR))
    R = E.OTHER_REACTION
    dev.set_reaction(R["A"], R["Ta"], R["Tcrit"], R["n"])
    for k in ("rho", "h", "alpha"):
        assert np.array_equal(dev.field(k), getattr(ref, k)), k           # formed from + - * / alone: bitwise
        assert not np.array_equal(dev.field(k), wood_state[k]), k
    assert np.all(dev.field("Yw") == 1.0) and np.all(dev.field("T") == 320.0) and np.all(dev.field("Twall") == 320.0)
    q = E.column_flux(NCOL); qd = ctx.to_device(q)
    for step in range(300):
        ref.step(0.05, q); dev.step(0.05, qd)
        if step % 50 == 49 or step == 0:
            _compare(dev, ref, "other material step %d" % step)
    assert ref.Yw.min() < 0.5 and ref.massGas.max() > 0
    dev.close()


def test_set_solids_after_steps_starts_the_panel_again(ffm, ctx):
    """ffm_pyro_set_solids re-initialises the state: a panel that has run, given the solids again, repeats its run bit for bit"""
    dev = ffm.PyrolysisPanel(ctx, NCOL, 5, **GEO, T0=600.0)
    solids = (E.solid4(E.OTHER_WOOD), E.solid4(E.OTHER_CHAR))
    dev.set_solids(*solids)
    qd = ctx.to_device(E.column_flux(NCOL))

    def run():
        for _ in range(30):
            dev.step(0.05, qd)
        return {k: dev.field(k) for k in FIELDS + ("phiGas", "Tsurf")}
    first = run()
    assert first["Yw"].max() < 1.0
    dev.set_solids(*solids)
    assert np.all(dev.field("Yw") == 1.0) and np.all(dev.field("phiGas") == 0.0) and np.all(dev.field("Tsurf") == 600.0)
    second = run()
    assert all(np.array_equal(first[k], second[k]) for k in first)
    dev.close()


@pytest.mark.parametrize("Yw0", [0.6, 0.0005])
def test_partly_charred_start(ffm, ctx, Yw0):
    """Yw0 < 1: rho0 of the mixture and c0 = rho0 max(Yw0, 0.001); 0.0005 lies below that floor"""
    from oracle import pyrolysis as PY
    ref = PY.Panel(NCOL, 8, **GEO, Yw0=Yw0); dev = ffm.PyrolysisPanel(ctx, NCOL, 8, **GEO, Yw0=Yw0)
    for k in FIELDS:
        assert np.array_equal(dev.field(k), getattr(ref, k)), k
    q = E.column_flux(NCOL); qd = ctx.to_device(q)
    for step in range(50):
        ref.step(0.05, q); dev.step(0.05, qd)
        if step % 10 == 9 or step == 0:
            _compare(dev, ref, "Yw0=%g step %d" % (Yw0, step))
    assert ref.massGas.max() > 0 and ref.Yw.max() < Yw0
    dev.close()


def test_burnout_clips_Yw_to_zero_and_the_charred_column_goes_on(ffm, ctx):
    """first-order reaction at 693 K, kf deltaT = 1.048: the first step clips Yw to exactly 0 in every cell (the unclipped value is
    -0.84: tests/test_physics_edge_inputs_cpu.py), 20 more steps run on the fully charred column (X = 0, omega = 0).  The temperatures
    are unphysical, the whole heat of reaction landing in one step: a test of the arithmetic at Yw = 0, not of a fire."""
    from oracle import pyrolysis as PY
    B = E.BURNOUT
    ref = PY.Panel(NCOL, 8, **GEO, T0=B["T0"], reaction=B["reaction"])
    dev = ffm.PyrolysisPanel(ctx, NCOL, 8, **GEO, T0=B["T0"])
    R = B["reaction"]
    dev.set_reaction(R["A"], R["Ta"], R["Tcrit"], R["n"])
    qd = ctx.to_device(np.zeros(NCOL))
    m0 = (dev.field("rho") * ref.V).sum(axis=1); gas = np.zeros(NCOL)
    for step in range(B["nSteps"]):
        ref.step(B["dt"], np.zeros(NCOL)); dev.step(B["dt"], qd)
        assert np.all(dev.field("Yw") == 0.0), step
        _compare(dev, ref, "burnout step %d" % step)
        assert all(np.isfinite(dev.field(k)).all() for k in FIELDS)
        assert step == 0 or np.all(dev.field("phiGas") == 0.0)
        gas += dev.field("phiGas") * B["dt"]
    assert dev.field("rho").min() > 6.0 and gas.min() > 0
    assert np.allclose(m0 - (dev.field("rho") * ref.V).sum(axis=1), gas, rtol=1e-12)      # mass lost = gas released
    dev.close()
