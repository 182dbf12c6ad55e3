"""The inputs of the edge tests of the per-cell physics kernels (tests/physics_edge_inputs.py) reach, on the oracle alone, the edge each
is meant to reach: the burnout run clips Yw with a margin that rounding cannot cross, the EDC fields take both branches of the rate, the
synthetic thermo table has neither its first nor its last species at an extreme and the oracle handles absent leading species, the
limits of the temperature range, T = Tcommon, a NaN enthalpy and an enthalpy no temperature has.  The GPU modules
tests/test_pyrolysis_edges_gpu.py and tests/test_thermo_edges_gpu.py run the same inputs through the kernels."""
import numpy as np
import pytest

import physics_edge_inputs as E
from oracle import pyrolysis as PY
from oracle import thermo as TH


def _burnout_panel(T0):
    return PY.Panel(70, 8, thickness=0.0127, area=0.01, T0=T0, reaction=E.BURNOUT["reaction"])


def test_burnout_clips_every_cell_with_a_margin_and_keeps_rho_positive():
    B = E.BURNOUT
    p = _burnout_panel(B["T0"])
    Yun, rho, kf = E.burnout_unclipped_Yw(p, B["dt"])
    assert abs(kf.max() * B["dt"] - 1.048) < 1e-3
    assert Yun.max() < -1e-3 and rho.min() > 6.0               # clipped everywhere, far from the decision; rho = 6.55
    m0 = (p.rho * p.V).sum(axis=1); gas = np.zeros(p.nCol)
    for s in range(B["nSteps"]):
        p.step(B["dt"], np.zeros(p.nCol)); gas += p.massGas * B["dt"]
        assert np.all(p.Yw == 0.0) and p.rho.min() > 6.0
        assert all(np.isfinite(f).all() for f in (p.T, p.h, p.alpha, p.massGas))
        assert s == 0 or np.all(p.massGas == 0.0)               # nothing is left to react
    assert np.allclose(m0 - (p.rho * p.V).sum(axis=1), gas, rtol=1e-12)


def test_burnout_window_of_the_start_temperature():
    """690 K does not clip, 695 K drives rho negative: 693 K lies inside the window"""
    B = E.BURNOUT
    Yun, rho, _ = E.burnout_unclipped_Yw(_burnout_panel(690.0), B["dt"])
    assert Yun.min() > 0.1 and rho.min() > 0
    _, rho, _ = E.burnout_unclipped_Yw(_burnout_panel(695.0), B["dt"])
    assert rho.max() < 0


@pytest.mark.parametrize("Yw0,c0", [(0.6, 14.99), (0.0005, None)])
def test_partly_charred_start_is_finite_and_uses_the_floor_of_c0(Yw0, c0):
    p = PY.Panel(70, 8, thickness=0.0127, area=0.01, Yw0=Yw0)
    rho0 = 1.0 / (Yw0 / PY.WOOD.rho + (1 - Yw0) / PY.CHAR.rho)
    assert p.c0 == rho0 * max(Yw0, 0.001) and (c0 is None or abs(p.c0 - c0) < 0.01)
    assert (Yw0 < 0.001) == (p.c0 > rho0 * Yw0)                 # below the floor the floor decides
    for _ in range(50):
        p.step(0.05, E.column_flux(70))
    assert all(np.isfinite(f).all() for f in (p.rho, p.Yw, p.T, p.h)) and p.massGas.max() > 0


def test_other_material_differs_in_every_number_and_chars():
    a = E.solid4(E.OTHER_WOOD) + E.solid4(E.OTHER_CHAR); b = E.solid4(PY.WOOD) + E.solid4(PY.CHAR)
    assert len(set(a)) == 8 and not set(a) & set(b) and E.OTHER_CHAR.Hf != 0.0
    assert all(E.OTHER_REACTION[k] != PY.REACTION[k] for k in PY.REACTION)
    p = PY.Panel(70, 8, thickness=0.0127, area=0.01, wood=E.OTHER_WOOD, char=E.OTHER_CHAR, reaction=E.OTHER_REACTION)
    d = PY.Panel(70, 8, thickness=0.0127, area=0.01)
    assert p.rho[0, 0] == E.OTHER_WOOD.rho and p.alpha[0, 0] == E.OTHER_WOOD.kappa / E.OTHER_WOOD.Cp and p.c0 == E.OTHER_WOOD.rho
    for _ in range(300):
        p.step(0.05, E.column_flux(70)); d.step(0.05, E.column_flux(70))
    assert p.Yw.min() < 0.5 and np.isfinite(p.T).all()
    assert np.abs(p.T - d.T).max() > 1.0                        # the keyword arguments are what the step uses


def test_module_constants_are_the_default_material():
    p = PY.Panel(3, 4)
    assert p.wood is PY.WOOD and p.char is PY.CHAR and p.reaction == PY.REACTION


@pytest.mark.parametrize("nLay", [2, 16])
def test_end_layer_counts_reach_charring_on_the_oracle(nLay):
    p = PY.Panel(70, nLay, thickness=0.0127, area=0.01)
    for _ in range(600):
        p.step(0.05, E.column_flux(70))
    assert p.Yw.min() < 0.15


@pytest.mark.parametrize("nLay", [2, 16])
def test_incident_runs_do_not_amplify_rounding_at_their_time_step(nLay):
    """the condition of comparing the fixedIncidentRadiation runs to 1e-11: a change of QrIncident in the last place stays small"""
    import pyro_incident_ref as R
    case = R.case_data()
    geo = dict(thickness=case["pyrolysis"]["thickness"], area=0.01, T0=case["panelT"]["internalField"])
    Qr = 3.0e4 + 6.0e4 * np.sin(0.37 * np.arange(70)) ** 2
    dt = E.incident_deltaT(case["controls"]["deltaT"], nLay)
    assert dt == (0.2 if nLay == 2 else 0.1)
    a = R.IncidentPanel(70, nLay, QrIncident=Qr, **geo, **R.case_selections(case))
    b = R.IncidentPanel(70, nLay, QrIncident=Qr * (1.0 + 2.3e-16 * np.sign(np.sin(1.0 + np.arange(70)))), **geo, **R.case_selections(case))
    worst = 0.0
    for s in range(int(round(80.0 / dt))):
        a.step_incident(dt); b.step_incident(dt)
        if s % 50 == 49:
            worst = max(worst, np.abs(a.rho - b.rho).max() / a.rho.max(), np.abs(a.T - b.T).max() / a.T.max())
    assert not np.array_equal(a.QrIncident, b.QrIncident) and worst < 1e-12 and a.Yw.min() < 0.5


# ------------------------------------------------------------------------------------------------------------------- thermo
def test_synthetic_table_has_no_extreme_at_its_ends():
    for n in (2, 8):
        names, tab = E.synthetic_table(n)
        for key, pick in (("Tlow", max), ("Thigh", min), ("As", max), ("As", min), ("Ts", max), ("Ts", min)):
            v = [tab[s][key] for s in names]
            assert len(set(v)) == n
            if n == 8:
                assert pick(v) not in (v[0], v[-1]), key


@pytest.mark.parametrize("nSp", [1, 2, 8])
def test_oracle_handles_absent_leading_species_and_the_range_edges(nSp):
    names, tab = E.synthetic_table(nSp)
    sp = TH.Species(names, tab)
    n = 300
    Y = E.compositions(nSp, n, seed=5)
    assert np.allclose(Y.sum(axis=0), 1.0)
    if nSp > 1:
        assert Y[0, 0] == 0 and Y[1, 0] > 0 and Y[0, 2] == 0 and Y[-1, 2] == 1.0
    if nSp > 2:
        assert np.all(Y[:2, 1] == 0) and Y[2, 1] > 0 and np.all(Y[:-1, 2] == 0)
        assert 0.25 < (Y == 0).mean() < 0.45
    mx = sp.mixture(Y)
    if nSp > 1:                                                 # a cell of the last species alone has that species' properties
        last = sp.single(nSp - 1)
        assert mx.W[2] == last.W and mx.As[2] == last.As and np.array_equal(mx.high[2], last.high)
    T = E.hashed(3, n, 300.0, 2500.0)
    he = mx.Hs(0.0, T)
    for T0 in (250.0, 3000.0, 5900.0):
        assert np.abs(mx.THs(he, 0.0, np.full(n, T0)) - T).max() < 1e-3
        assert np.array_equal(mx.THs(mx.Hs(0.0, mx.Tlow) - 1.0e5, 0.0, np.full(n, T0)), mx.Tlow * np.ones(n))
        assert np.array_equal(mx.THs(mx.Hs(0.0, mx.Thigh) + 1.0e5, 0.0, np.full(n, T0)), mx.Thigh * np.ones(n))
    if nSp == 8:
        assert len(np.unique(mx.Tlow)) > 1 and len(np.unique(mx.Thigh)) > 1
    Tc = np.full(n, 1000.0)
    assert np.array_equal(mx._coeffs(Tc), mx.high * np.ones((n, 7)))            # at T == Tcommon the high set applies
    assert np.abs(mx.THs(mx.Hs(0.0, Tc), 0.0, np.full(n, 900.0)) - 1000.0).max() < 1e-6


def test_oracle_passes_a_nan_enthalpy_on_to_that_cell_only():
    names, tab = E.synthetic_table(8)
    mx = TH.Species(names, tab).mixture(E.compositions(8, 300, seed=5))
    T = E.hashed(3, 300, 300.0, 2500.0)
    he = mx.Hs(0.0, T)
    clean = mx.THs(he, 0.0, np.full(300, 900.0))
    he[7] = np.nan
    Tn = mx.THs(he, 0.0, np.full(300, 900.0))
    assert np.isnan(Tn[7]) and np.isnan(Tn).sum() == 1
    assert np.array_equal(np.delete(Tn, 7), np.delete(clean, 7))
    assert np.isnan(mx.mu(0.0, Tn)[7]) and np.isnan(mx.psi(0.0, Tn)[7]) and np.isnan(mx.alphah(0.0, Tn)[7])


def test_oracle_fails_on_an_enthalpy_inside_the_jump():
    names, tab, hmid, (below, above) = E.jump_table()
    R = TH.RR / tab["N2"]["W"]
    assert abs((above - below) / R - 50.0) < 0.01 and below < hmid < above
    mx = TH.Species(names, tab).single(0)
    with pytest.raises(RuntimeError, match="maximum number of iterations exceeded"):
        mx.THs(np.array([hmid]), 0.0, np.array([900.0]))
    assert abs(mx.THs(np.array([below - 1.0e4]), 0.0, np.array([900.0]))[0] - 1000.0) < 20.0   # next to the jump it converges


# ---------------------------------------------------------------------------------------------------------------- EDC / nut
def test_edc_fields_take_both_branches_and_both_limits():
    rho, k, d, al, Yf, Yo = E.edc_fields(1000)
    w, rtT, rtD = E.edc_reference(rho, k, d, al, Yf, Yo)
    assert E.EDC["C_Diff"] > 0
    assert ((rtD > rtT) & (k > 0)).sum() > 20 and (rtT > rtD).sum() > 20       # the diffusion branch wins, and not only where k = 0
    assert (k == 0).sum() > 20 and np.all(rtT[k == 0] == 0.0) and np.all(rtD[k == 0] > 0)
    assert ((Yf < Yo / E.EDC["s"]) & (Yf > 0)).sum() > 20 and (Yf > Yo / E.EDC["s"]).sum() > 20   # fuel- and oxygen-limited
    assert np.isfinite(w).all() and (w[k == 0] > 0).any()
