"""BASELINE config 1 (cases/pyrolysis1D on its own dictionaries): tests/pyro_incident_ref.py -- fixedIncidentRadiation on the exposed
face and qrHSource over oracle/pyrolysis.py's Panel -- pinned to what the equations imply.  The reference ships no output of this
case (cases/pyrolysis1D/mlr.plot:4 plots ./referenceResult, which is not in the tree), so nothing here is reference data:
 * radiative equilibrium: with no reaction and an adiabatic back face every layer tends to (QrIncident/sigma)^(1/4), whatever e is;
 * energy: the enthalpy gained is the recorded qSurf A dt summed over the steps;
 * qrHSource: the source sums to A (qr0 - qr_{N-1}); an opaque solid takes it all in layer 0, like a surface flux; qr0 <= 0 is no source;
 * config 1 from tests/golden/pyrolysis1d_case_data.json: the case's 500 steps of 0.2 s char the exposed layer first, the wood
   fraction only falls, the mass lost is the pyrolysate released;
 * the fixture regenerates byte-identically from the case files where the reference tree is present."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

@pytest.mark.parametrize("e", [0.17, 0.85])
def test_radiative_equilibrium(e):
    from pyro_incident_ref import NO_REACTION, IncidentPanel, equilibrium_setup
    Qr, L, Teq, tau, n, dt = equilibrium_setup(e)
    assert abs(Teq - 1014.2) < 0.05 and n * dt >= 20.0 * tau
    P = IncidentPanel(2, 8, QrIncident=Qr, Tcrit=NO_REACTION, thickness=L, area=0.01, alphaScheme="harmonic", kappaScheme="harmonic",
                      radiation=dict(v=(e, e), char=(0.9, 0.9)))
    for _ in range(n):
        P.step_incident(dt)
    assert np.all(P.Yw == 1.0) and np.all(P.massGas == 0.0)
    print("equilibrium e=%g: max |T/Teq - 1| = %.3e after %d steps" % (e, np.abs(P.T / Teq - 1.0).max(), n))
    assert np.abs(P.T / Teq - 1.0).max() <= 1e-6
    assert np.abs(P.Twall / Teq - 1.0).max() <= 1e-6


def test_incident_energy_balance():
    """no reaction, zero-gradient back face: sum(rho h V) gains the recorded e (Qr - sigma T^4) A dt of every step"""
    from oracle import pyrolysis as PY
    from pyro_incident_ref import NO_REACTION, IncidentPanel
    Qr = np.array([3.0e4, 6.0e4, 9.0e4])
    P = IncidentPanel(3, 8, QrIncident=Qr, Tcrit=NO_REACTION, thickness=0.0234, area=0.04, alphaScheme="harmonic", kappaScheme="harmonic",
                      radiation=dict(v=(0.17, 0.17), char=(0.85, 0.85)))
    E0 = (P.rho * P.h * P.V).sum(axis=1)
    dt, put = 0.2, np.zeros(3)
    for _ in range(200):
        T0 = P.T[:, 0].copy()
        res = P.step_incident(dt)
        assert np.array_equal(P.qSurf, 0.17 * (Qr - PY.SIGMA_SB * ((T0 * T0) * (T0 * T0)))) and np.all(res["emissivity"] == 0.17)
        put += P.qSurf * P.A * dt
    assert P.T[:, 0].min() > 400.0 and np.all(P.Yw == 1.0)             # hot enough to react, had the reaction been on
    E1 = (P.rho * P.h * P.V).sum(axis=1)
    assert np.allclose(E1 - E0, put, rtol=1e-12, atol=0)
    # the wall value: the cell value plus the gradient over half a layer, q = kappa refGrad
    assert np.allclose((P.Twall - P.T[:, 0]) * (2.0 / P.dx) * PY.WOOD.kappa, P.qSurf, rtol=1e-12)


def test_qr_source_sums_and_limits():
    from pyro_incident_ref import IncidentPanel
    rad = dict(v=(0.17, 0.17), char=(0.85, 0.85))
    kw = dict(thickness=0.0234, area=0.04, T0=500.0, alphaScheme="harmonic", kappaScheme="harmonic")
    q = np.array([1.0e3, 2.0e4, 5.0e4])
    qr0 = np.array([4.0e4, 1.0e4, 2.5e4])
    # the source sums to A (qr0 - qr_{N-1}), also where the composition varies over the depth
    P = IncidentPanel(3, 8, qr0=qr0, radiation=rad, **kw)
    P.Yw[:] = np.linspace(0.3, 1.0, 8)[None, :]
    for _ in range(5):
        res = P.step(0.2, q)
        assert np.allclose(res["qrSource"].sum(axis=1), P.A * (qr0 - res["qr"][:, -1]), rtol=1e-13, atol=0)
        assert np.all(res["qrSource"] > 0) and np.all(np.diff(res["qr"], axis=1) < 0) and np.all(res["qr"][:, 0] < qr0)
    # an opaque solid: everything lands in layer 0, which is a surface flux of qr0 on top of q
    big = dict(v=(1.0e9, 0.17), char=(1.0e9, 0.85))
    a = IncidentPanel(3, 8, qr0=qr0, radiation=big, **kw)
    b = IncidentPanel(3, 8, radiation=big, **kw)
    worst = 0.0
    for _ in range(50):              # every step from the same state: the two differ in where q A and qr0 A are added, i.e. by round-off
        for name in ("h", "T", "rho", "Yw", "alpha"):
            setattr(b, name, getattr(a, name).copy())
        ra = a.step(0.2, q); b.step(0.2, q + qr0)
        assert np.all(ra["qr"] == 0.0) and np.array_equal(ra["qrSource"][:, 0], a.A * qr0) and np.all(ra["qrSource"][:, 1:] == 0.0)
        assert np.array_equal(a.rho, b.rho) and np.array_equal(a.Yw, b.Yw)
        worst = max(worst, np.abs(a.h / b.h - 1.0).max(), np.abs(a.T / b.T - 1.0).max())
    print("opaque solid against a surface flux: largest relative difference of a step %.2e" % worst)
    assert a.Yw.min() < 1.0                                              # through the onset of the reaction
    assert worst <= 64 * np.finfo(float).eps                             # a few roundings through an 8 x 8 diagonally dominant solve
    # an emitting surface (qr0 <= 0) is no source: bitwise the step without it, with each closure of the exposed face
    c = IncidentPanel(3, 8, qr0=np.array([0.0, -5.0e3, -1.0]), QrIncident=6.0e4, radiation=rad, **kw)
    d = IncidentPanel(3, 8, QrIncident=6.0e4, radiation=rad, **kw)
    for s in range(40):
        if s % 2:
            rc = c.step(0.2, q); d.step(0.2, q)
        else:
            rc = c.step_incident(0.2); d.step_incident(0.2)
        assert np.all(rc["qrSource"] == 0.0)
        for name in ("h", "T", "rho", "Yw", "alpha", "Twall", "qSurf", "massGas"):
            assert np.array_equal(getattr(c, name), getattr(d, name)), (s, name)


def test_config1_from_the_fixture():
    """cases/pyrolysis1D with its own selections: reactingOneDim, both laplacians harmonic, constHTemperature h 0 at the back,
    fixedIncidentRadiation 60 kW/m2 with the emissivity of greyMeanSolidAbsorptionEmission, 8 layers over 0.0234 m, 500 steps of 0.2 s"""
    import pyro_incident_ref as R
    case = R.case_data()
    sel = R.case_selections(case)
    assert sel == dict(model="reactingOneDim", alphaScheme="harmonic", kappaScheme="harmonic", back=("constH", 0.0, 298.15),
                       radiation=dict(v=(0.17, 0.17), char=(0.85, 0.85)))
    assert case["pyrolysis"]["qrHSource"] == "no" and case["pyrolysis"]["gasHSource"] == "no" and case["solvePrimaryRegion"] == "false"
    ctl = case["controls"]
    dt, n = ctl["deltaT"], int(round(ctl["endTime"] / ctl["deltaT"]))
    assert (dt, n, ctl["sampleInterval"], ctl["adjustTimeStep"]) == (0.2, 500, 10, "no")
    P = R.IncidentPanel(1, case["pyrolysis"]["nLayers"], QrIncident=case["panelT"]["exposed"]["QrIncident"], thickness=case["pyrolysis"]["thickness"],
                        area=1.0, T0=case["panelT"]["internalField"], **sel)
    m0 = (P.rho * P.V).sum(axis=1)
    gas = np.zeros(1)
    first = {}
    for s in range(n):
        yw0 = P.Yw.copy()
        res = P.step_incident(dt)
        gas += P.massGas * dt
        assert np.isfinite(P.T).all() and np.isfinite(P.h).all() and np.isfinite(P.rho).all()
        assert np.all(P.Yw <= yw0) and np.all(P.Yw >= 0.0)              # the wood fraction only falls
        for i in np.nonzero(P.Yw[0] < 0.99)[0]:
            first.setdefault(int(i), s)
    print("config 1 after %d steps: Yw[0]=%.4f T[0]=%.2f Twall=%.2f emissivity=%.4f" % (n, P.Yw[0, 0], P.T[0, 0], P.Twall[0], res["emissivity"][0]))
    assert P.Yw.min() < 0.5                                             # reached charring
    assert np.all(np.diff(P.Yw[0]) >= 0) and P.Yw[0, 0] < P.Yw[0, -1] and first[0] == min(first.values())     # the exposed layer chars first
    assert np.all(np.diff(P.T[0]) < 0) and P.Twall[0] > P.T[0, 0]
    lost = m0 - (P.rho * P.V).sum(axis=1)
    assert lost[0] > 0 and np.allclose(lost, gas, rtol=1e-9, atol=0)
    assert 0.17 < res["emissivity"][0] <= 0.85


def test_fixture_regenerates_from_the_case_files():
    spec = importlib.util.spec_from_file_location("make_pyrolysis1d_case_data", os.path.join(HERE, "golden", "make_pyrolysis1d_case_data.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    if not os.path.isdir(gen.CASE):
        pytest.skip("the reference tree is not present")
    assert gen.dumps() == open(gen.OUT).read()
