"""Inputs (test infrastructure) of the edge tests of the per-cell physics kernels -- csrc/ffm_pyro.hip, csrc/ffm_thermo.hip and the wall
kernel of csrc/ffm_rad.hip -- shared by tests/test_physics_edge_inputs_cpu.py, which checks on the oracle alone that every input reaches
the edge it is meant to reach, and by the GPU modules tests/test_pyrolysis_edges_gpu.py and tests/test_thermo_edges_gpu.py, which run
the same inputs through the kernels.  Only tests/ may import this module."""
import json
import os

import numpy as np

from oracle import pyrolysis as PY
from oracle import thermo as TH

# ---------------------------------------------------------------------------------------------------------------- pyrolysis
# a material whose eight numbers all differ from the built-in wood / char (oracle/pyrolysis.py), with a char heat of formation, and a
# reaction whose four constants differ from the built-in ones
OTHER_WOOD = PY.Solid(310.0, 1420.0, 0.21, -3.1e5)
OTHER_CHAR = PY.Solid(73.0, 1010.0, 0.09, 1.2e5)
OTHER_REACTION = dict(A=2.5e7, Ta=9800.0, Tcrit=450.0, n=1.7)


def solid4(s):
    """(rho, Cp, kappa, Hf): the argument of PyrolysisPanel.set_solids"""
    return (s.rho, s.Cp, s.kappa, s.Hf)


def column_flux(nCol, q0=3.0e4):
    """a different heat flux into every column [W/m2], as tests/test_pyrolysis_gpu.py's panel test"""
    return q0 * (1.0 + 0.7 * np.sin(0.37 * np.arange(nCol)) ** 2)


def incident_deltaT(caseDeltaT, nLay):
    """deltaT of the fixedIncidentRadiation runs: the case's (0.2 s, for 8 layers) up to 8 layers, half of it above.  The patch is explicit
    (T^4 of the old cell temperature), stable while deltaT stays below twice the exposed layer's time constant, which falls as 1/nLay and,
    once the layer has charred, with char's rho Cp.  With 15 or 16 layers and 0.2 s the restatement itself turns a change of QrIncident
    by one unit in the last place into 1e-8 of rho while the exposed layer chars -- nothing can be compared to 1e-11 there; with 0.1 s
    it stays at 1e-13 (tests/test_physics_edge_inputs_cpu.py)."""
    return caseDeltaT if nLay <= 8 else 0.5 * caseDeltaT


# burnout: first-order reaction at T0 = 693 K, deltaT = 0.05 s: kf deltaT = 1.048 > 1, so the first step's species update is negative in
# every cell and is clipped to Yw = 0, while rho stays positive.  The window: 690 K does not clip, 695 K drives rho negative.
BURNOUT = dict(T0=693.0, dt=0.05, nSteps=21, reaction=dict(PY.REACTION, n=1.0))


def burnout_unclipped_Yw(panel, dt):
    """what solveSpeciesMass gives before Yi.max(0), and the new rho, for the panel's present state (Panel._evolve's expressions)"""
    R = panel.reaction
    rdt = 1.0 / dt
    kf = np.where(panel.T < R["Tcrit"], 0.0, R["A"] * np.exp(-R["Ta"] / panel.T))
    omega = kf * np.power(panel.rho * panel.Yw / panel.c0, R["n"]) * panel.c0
    rho = (rdt * panel.rho * panel.V - panel.V * ((1.0 - panel.char.rho / panel.wood.rho) * omega)) / (rdt * panel.V)
    return (rdt * panel.rho * panel.Yw * panel.V + panel.V * (-omega)) / (rdt * rho * panel.V), rho, kf


# ------------------------------------------------------------------------------------------------------------------- thermo
STECKLER = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "steckler_case_data.json")))

# per-species limits and sutherland constants of the synthetic table: all distinct, and in no monotone order, so that neither the first
# nor the last species holds the largest Tlow, the smallest Thigh or an extreme As / Ts
SYN_TLOW = [215.0, 260.0, 230.0, 290.0, 205.0, 280.0, 220.0, 250.0]
SYN_THIGH = [4800.0, 4300.0, 4700.0, 3900.0, 4900.0, 4000.0, 4600.0, 4400.0]
SYN_AS = [1.60e-06, 1.95e-06, 1.35e-06, 2.10e-06, 1.50e-06, 1.20e-06, 1.85e-06, 1.70e-06]
SYN_TS = [150.0, 90.0, 210.0, 120.0, 240.0, 110.0, 180.0, 135.0]


def golden_table():
    return {n: {k: (np.array(v) if isinstance(v, list) else v) for k, v in d.items()} for n, d in STECKLER["table"].items()}


def synthetic_table(nSpecies):
    """(names, table) of nSpecies <= 9 species: the golden five, repeated, entry k with its molecular weight and both coefficient sets
    scaled by 1 + 0.03 k (one factor for both sets: Cp and Ha stay as continuous at Tcommon as the golden ones are) and the limits and
    sutherland constants above.  Tcommon stays 1000 K for all (janafThermo::operator+= demands equal Tcommon)."""
    gold, base = golden_table(), STECKLER["species"]
    names, tab = [], {}
    for k in range(nSpecies):
        g = gold[base[k % len(base)]]
        f = 1.0 + 0.03 * k
        name = "%s_%d" % (base[k % len(base)], k)
        names.append(name)
        tab[name] = dict(W=g["W"] * (1.0 + 0.011 * k), Tlow=SYN_TLOW[k % 8], Thigh=SYN_THIGH[k % 8], Tcommon=g["Tcommon"],
                         high=np.asarray(g["high"], float) * f, low=np.asarray(g["low"], float) * f, As=SYN_AS[k % 8], Ts=SYN_TS[k % 8])
    return names, tab


def compositions(nSpecies, n, seed):
    """Y[nSpecies][n]: random compositions summing to 1 in which about a third of the entries are exactly 0; cell 0 lacks the first
    species, cell 1 the first two, cell 2 all but the last (the leading species of cellMixture's progressive sum are absent)"""
    rng = np.random.default_rng(seed)
    Y = rng.random((nSpecies, n)) * (rng.random((nSpecies, n)) > 1.0 / 3.0)
    Y[-1] += (Y.sum(axis=0) == 0.0)                     # no empty cell
    if nSpecies > 1 and n > 0:
        Y[0, 0:1] = 0.0; Y[1, 0:1] = np.maximum(Y[1, 0:1], 0.25)
    if nSpecies > 2 and n > 1:
        Y[0:2, 1] = 0.0; Y[2, 1] = max(Y[2, 1], 0.25)
    if nSpecies > 1 and n > 2:
        Y[:-1, 2] = 0.0; Y[-1, 2] = 1.0
    return Y / Y.sum(axis=0)


def hashed(seed, n, lo=0.0, hi=1.0):
    """n values in [lo, hi) without a period: entry i and entry i + 524288 differ"""
    return lo + (hi - lo) * np.random.default_rng(seed).random(n)


def jump_table():
    """one species whose lowCpCoeffs[5] is lowered by 50: Ha jumps by 50 R at Tcommon; returns (names, table, he in the middle of the
    jump [J/kg]).  No temperature has that enthalpy: the Newton iteration started at 900 K alternates across Tcommon for ever."""
    g = golden_table()["N2"]
    low = np.asarray(g["low"], float).copy(); low[5] -= 50.0
    tab = {"N2": dict(g, low=low)}
    mx = TH.Species(["N2"], tab).single(0)
    Tc = float(g["Tcommon"])
    below, above = float(mx.Hs(0.0, np.nextafter(Tc, 0.0))), float(mx.Hs(0.0, Tc))
    return ["N2"], tab, 0.5 * (below + above), (below, above)


# ---------------------------------------------------------------------------------------------------------------- EDC / nut
EDC = dict(s=3.6282945, dt=2.0e-2, Ce=1.048, C_EDC=4.0, C_Diff=25.0, C_Stiff=1.0, qFuel=4.6357151e7, Ck=0.094, Prt=0.85)


def edc_fields(n, seed=11):
    """rho, k, delta, alpha, Yfuel, YO2 of n cells: k spans decades and is exactly 0 in every seventh cell (the max(k, SMALL) guard: there
    the turbulent rate is 0 and the diffusion rate decides); fuel-limited and oxygen-limited cells, and cells without fuel"""
    rng = np.random.default_rng(seed)
    rho = 0.2 + rng.random(n)
    k = 10.0 ** (-4.0 + 5.0 * rng.random(n)); k[::7] = 0.0
    delta = 0.01 + 0.05 * rng.random(n)
    alpha = 2.0e-5 * (1.0 + 4.0 * rng.random(n))
    Yf = 0.2 * rng.random(n) * (rng.random(n) > 0.2)
    Yo = 0.233 * rng.random(n)
    Yf[0], Yo[0] = 0.05, 0.2                            # the leading cell (k = 0) burns: a launch of one cell has a rate to compare
    return rho, k, delta, alpha, Yf, Yo


def edc_reference(rho, k, delta, alpha, Yf, Yo, c=EDC):
    """eddyDissipationModel::correct in numpy, the formulas of tests/test_thermo_gpu.py; returns (wFuel, rtTurb, rtDiff)"""
    eps = c["Ce"] * k * np.sqrt(k) / delta
    rtTurb = c["C_EDC"] * eps / np.maximum(k, 1e-15)
    rtDiff = c["C_Diff"] * alpha / rho / delta ** 2
    rt = np.maximum(rtTurb, rtDiff)
    w = rho * np.minimum(Yf, Yo / c["s"]) / c["dt"] / c["C_Stiff"] * (1.0 - np.exp(-c["C_Stiff"] * c["dt"] * rt))
    return w, rtTurb, rtDiff
