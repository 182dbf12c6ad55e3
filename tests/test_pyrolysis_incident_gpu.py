"""BASELINE config 1 on the device: ffm_pyro_step_incident (fixedIncidentRadiation inside the column kernel), qrHSource and
ffm_pyro_run_incident (the whole run in one launch, state in registers) against tests/pyro_incident_ref.py with the selections of
tests/golden/pyrolysis1d_case_data.json.  Tolerances of the per-step comparison are those of tests/test_pyrolysis_gpu.py for this
kernel (device exp / pow against libm): 1e-11 relative, phiGas 1e-10; the run against single steps is bitwise."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("rho", "Yw", "T", "h", "alpha")


def _config1(ffm, ctx, nCol, Qr, area=0.01, **override):
    import pyro_incident_ref as R
    case = R.case_data()
    sel = dict(R.case_selections(case), **override)
    geo = dict(thickness=case["pyrolysis"]["thickness"], area=area, T0=case["panelT"]["internalField"])
    ref = R.IncidentPanel(nCol, case["pyrolysis"]["nLayers"], QrIncident=Qr, **geo, **sel)
    dev = ffm.PyrolysisPanel(ctx, nCol, case["pyrolysis"]["nLayers"], **geo)
    dev.set_model(**sel)
    dev.set_incident_radiation(Qr)
    ctl = case["controls"]
    return ref, dev, ctl["deltaT"], int(round(ctl["endTime"] / ctl["deltaT"])), ctl["sampleInterval"]


def _columns_Qr(nCol):
    return 3.0e4 + 6.0e4 * np.sin(0.37 * np.arange(nCol)) ** 2 if nCol > 1 else np.array([6.0e4])      # 30 ... 90 kW/m2


@pytest.mark.parametrize("nCol,variant", [(1, "config1"), (257, "config1"), (5000, "config1"), (257, "reactingOneDim21"), (257, "qrHSource")])
def test_step_incident_matches_the_restatement(ffm, ctx, nCol, variant):
    over = dict(model="reactingOneDim21", alphaScheme="linear") if variant == "reactingOneDim21" else {}
    ref, dev, dt, n, _ = _config1(ffm, ctx, nCol, _columns_Qr(nCol), **over)
    if variant == "qrHSource":
        ref.qr0 = 2.0e4 * np.cos(0.11 * np.arange(nCol)) - 2.0e3          # some columns emit: clipped to no source
        dev.set_qr_source(ref.qr0)
    assert n == 500
    for step in range(n):
        ref.step_incident(dt); dev.step_incident(dt)
        if step % 100 == 99 or step == 0:
            for name in FIELDS + ("Twall", "qSurf"):
                r, d = getattr(ref, name), dev.field(name)
                err = np.abs(d - r).max() / np.abs(r).max()
                print("%s nCol=%d step %d %s: %.2e" % (variant, nCol, step, name, err))
                assert err <= 1e-11, (step, name, err)
            errg = np.abs(dev.field("phiGas") - ref.massGas).max() / max(ref.massGas.max(), 1e-300)
            print("%s nCol=%d step %d phiGas: %.2e" % (variant, nCol, step, errg))
            assert errg <= 1e-10, (step, errg)
            assert np.array_equal(dev.field("Tsurf"), dev.field("T")[:, 0])
    assert ref.Yw.min() < 0.5                                   # the run reached charring
    dev.close()


@pytest.mark.parametrize("qr", [False, True])
def test_run_incident_is_bitwise_the_stepped_run(ffm, ctx, qr):
    nCol = 5000
    mk = lambda: _config1(ffm, ctx, nCol, _columns_Qr(nCol))
    _, stepped, dt, n, every = mk()
    _, one, _, _, _ = mk()
    _, two, _, _, _ = mk()
    panels = (stepped, one, two)
    if qr:
        for p in panels:
            p.set_qr_source(2.0e4 * np.cos(0.11 * np.arange(nCol)) - 2.0e3)
    assert (n, every) == (500, 10)
    names = FIELDS + ("Twall", "qSurf", "phiGas", "Tsurf")
    samples = []
    for s in range(n):
        stepped.step_incident(dt)
        if (s + 1) % every == 0:
            samples.append({k: stepped.field(k) for k in ("Twall", "phiGas", "T", "rho", "Yw")})
    H = one.run_incident(dt, n, sampleEvery=every)
    assert two.run_incident(dt, n // 2) is None
    two.run_incident(dt, n - n // 2)
    final = {k: stepped.field(k) for k in names}
    assert final["Yw"].min() < 0.5 and final["phiGas"].max() > 0
    for k in names:
        assert np.array_equal(one.field(k), final[k]), k
        assert np.array_equal(two.field(k), final[k]), k
    assert H["T"].shape == (n // every, nCol, 8) and H["Twall"].shape == (n // every, nCol)
    for i, smp in enumerate(samples):
        for k, v in smp.items():
            assert np.array_equal(H[k][i], v), (i, k)
    # chemistryQdot has no field to fetch: Qdot = -Hf_wood RRs_wood and RRg = (1 - rho_char/rho_wood) omega, so the column's heat
    # release and its pyrolysate release are proportional
    from oracle import pyrolysis as PY
    V = 0.01 * 0.0234 / 8
    gas = H["chemistryQdot"].sum(axis=2) * V * (1.0 - PY.CHAR.rho / PY.WOOD.rho) / PY.WOOD.Hf
    assert np.allclose(gas, H["phiGas"], rtol=1e-12, atol=0) and H["chemistryQdot"].min() < 0
    for p in panels:
        p.close()


@pytest.mark.parametrize("e", [0.17, 0.85])
def test_radiative_equilibrium_in_one_launch(ffm, ctx, e):
    """the equilibrium of tests/test_pyrolysis_incident_cpu.py on the device, the whole run one ffm_pyro_run_incident"""
    from pyro_incident_ref import NO_REACTION, equilibrium_setup
    from oracle import pyrolysis as PY
    Qr, L, Teq, tau, n, dt = equilibrium_setup(e)
    dev = ffm.PyrolysisPanel(ctx, 3, 8, thickness=L, area=0.01)
    dev.set_model(alphaScheme="harmonic", kappaScheme="harmonic", radiation=dict(v=(e, e), char=(0.9, 0.9)))
    R = PY.REACTION
    dev.set_reaction(R["A"], R["Ta"], NO_REACTION, R["n"])
    dev.set_incident_radiation(Qr)
    assert n * dt >= 20.0 * tau
    dev.run_incident(dt, n)
    T, Tw = dev.field("T"), dev.field("Twall")
    print("device equilibrium e=%g: max |T/Teq - 1| = %.3e after %d steps" % (e, np.abs(T / Teq - 1.0).max(), n))
    assert np.all(dev.field("Yw") == 1.0) and np.all(dev.field("phiGas") == 0.0)
    assert np.abs(T / Teq - 1.0).max() <= 1e-6 and np.abs(Tw / Teq - 1.0).max() <= 1e-6
    dev.close()


def test_incident_argument_checks(ffm, ctx):
    nCol = 100
    dev = ffm.PyrolysisPanel(ctx, nCol, 8, thickness=0.0234, area=0.01)
    dev.set_model(alphaScheme="harmonic", kappaScheme="harmonic")
    dev.set_incident_radiation(6.0e4)
    before = {k: dev.field(k) for k in FIELDS + ("Twall", "qSurf", "phiGas", "Tsurf")}

    def unchanged():
        return all(np.array_equal(dev.field(k), v) for k, v in before.items())
    # no surface radiation model: an error with a message, not a constant emissivity
    with pytest.raises(ffm.FfmError, match="surface radiation"):
        dev.step_incident(0.2)
    with pytest.raises(ffm.FfmError, match="surface radiation"):
        dev.run_incident(0.2, 10)
    assert unchanged()
    dev.set_model(alphaScheme="harmonic", kappaScheme="harmonic", radiation=dict(v=(0.17, 0.17), char=(0.85, 0.85)))
    with pytest.raises(ffm.FfmError):
        dev.run_incident(0.2, 0)
    with pytest.raises(ffm.FfmError):
        dev.run_incident(0.2, 10, sampleEvery=0)
    need = (20 // 5) * (2 + 4 * 8) * nCol
    hist = ctx.zeros(need)
    L = ffm.lib()
    assert L.ffm_pyro_run_incident(dev.h, 0.2, 20, 5, C.c_void_p(hist.data_ptr()), need - 1) == -1          # FFM_ERR_ARG
    assert b"history" in L.ffm_last_error()
    ctx.sync()
    assert unchanged() and not hist.cpu().numpy().any()
    assert L.ffm_pyro_run_incident(dev.h, 0.2, 20, 5, C.c_void_p(hist.data_ptr()), need) == 0
    ctx.sync()
    h = hist.cpu().numpy().reshape(4, 34, nCol)
    assert np.all(h[:, 0] > 298.15) and np.all(h[:, 2:10] > 298.0) and not unchanged()
    # a panel without QrIncident
    other = ffm.PyrolysisPanel(ctx, 4, 8, thickness=0.0234, area=0.01)
    other.set_model(radiation=dict(v=(0.17, 0.17), char=(0.85, 0.85)))
    with pytest.raises(ffm.FfmError, match="QrIncident"):
        other.step_incident(0.2)
    other.close(); dev.close()
