"""greyMeanAbsorptionEmission::aCont restated in numpy (test infrastructure, not a test): the arithmetic of csrc/ffm_greymean.hpp in the
same operation order -- only + * / occur, correctly rounded in IEEE double on both sides, so the device result equals this one bit for bit.

    invWt = ((0 + Y_0/W_0) + Y_1/W_1) + ...                      all species, index order
    a = 0; for the participating species in list order:
        Xk = Y_s/(W_s*invWt); Xipi = Xk*(p/101325.0); b = lo where T < Tcommon else hi; Ti = 1.0/T where invTemp else T
        a = a + Xipi*(((((b5*Ti + b4)*Ti + b3)*Ti + b2)*Ti + b1)*Ti + b0)

The order over the participating species is the list's (the case file's), not the reference's HashTable order: unpinned by reference data."""
import json
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "greymean_case_data.json")
# molecular weights [kg/kmol] of the species of the tests' mixtures (cases/steckler/constant/thermo.compressibleGas; CH4 = 12.011 + 4*1.00794)
W = {"O2": 31.9988, "N2": 28.0134, "CO2": 44.01, "H2O": 18.0153, "CH4": 16.04276, "C3H8": 44.0962}


def fixture():
    return json.load(open(FIXTURE))


def polynomial(c, T):
    """one species' polynomial at T [array]: absorption per atm of partial pressure"""
    T = np.asarray(T, np.float64)
    low = T < c["Tcommon"]
    b = [np.where(low, c["loTcoeffs"][k], c["hiTcoeffs"][k]) for k in range(6)]
    Ti = 1.0 / T if c["invTemp"] else T
    return ((((b[5] * Ti + b[4]) * Ti + b[3]) * Ti + b[2]) * Ti + b[1]) * Ti + b[0]


def aCont(species, Wd, coeffs, order, Y, p, T):
    """species: all species (the order of Y, a list of arrays); Wd: {specie: W}; coeffs: {specie: dict}; order: the participating species"""
    invWt = np.zeros_like(T)
    for s, name in enumerate(species):
        invWt = invWt + Y[s] / Wd[name]
    a = np.zeros_like(T)
    for name in order:
        s = species.index(name)
        Xk = Y[s] / (Wd[name] * invWt)
        Xipi = Xk * (p / 101325.0)
        a = a + Xipi * polynomial(coeffs[name], T)
    return a


def outside(coeffs, order, T):
    """True where the device pass raises its flag: some T outside [Tlow, Thigh] of a participating species"""
    return bool(any(((T < coeffs[s]["Tlow"]) | (T > coeffs[s]["Thigh"])).any() for s in order))


def radiation_sh(a, e, sigma, E, G, T, he, Cp):
    """ffm_radiation_sh_v_d: the order of k_radiation_sh with field a, e, E"""
    Rp = 4.0 * e * sigma
    T3 = T * T * T
    Ru = a * G - E
    return Ru - Rp * T3 * (T - 4.0 * he / Cp), 4.0 * Rp * T3 / Cp


# ------------------------------------------------------------------ the designed inputs of the kernel tests ---
SPECIES5 = ["CH4", "O2", "N2", "H2O", "CO2"]


def edge_coeffs():
    """the fixture's three species with CH4's table altered so that every branch is live: a loTcoeffs set that is not zero, a Tcommon
    (650 K) different from the others' (300 K), a narrower [Tlow, Thigh]"""
    fx = fixture()
    co = {k: dict(v) for k, v in fx["coeffs"].items()}
    co["CH4"].update(Tcommon=650.0, Tlow=250.0, Thigh=2400.0, loTcoeffs=[5.9, -2.1e-3, 3.0e-7, -1.0e-10, 2.0e-14, -1.0e-18])
    return co


def edge_inputs(n, seed=5, in_range=False):
    """Y (5 arrays, summing to 1), p, T for n cells.  The first cells are designed: T just below, at and above each Tcommon (nextafter),
    a participating species with Y == 0, a non-participating species (N2) carrying most of the mass, and -- unless in_range -- T below
    every Tlow and above every Thigh.  Returns (Y, p, T, names of the designed cells)."""
    r = np.random.RandomState(seed)
    Y = r.uniform(0.02, 1.0, (5, n))
    T = r.uniform(260.0, 2390.0, n)
    p = r.uniform(0.9e5, 1.1e5, n)
    marks = {}
    cells = [("below300", np.nextafter(300.0, 0.0)), ("at300", 300.0), ("above300", np.nextafter(300.0, 1e9)),
             ("below650", np.nextafter(650.0, 0.0)), ("at650", 650.0), ("above650", np.nextafter(650.0, 1e9)),
             ("zeroY", 1234.5), ("mostlyN2", 1800.0)]
    if not in_range:
        cells += [("tooCold", 150.0), ("tooHot", 2600.0), ("coldForCH4only", 225.0), ("hotForCH4only", 2450.0)]
    for i, (name, t) in enumerate(cells):
        if i < n:
            T[i] = t; marks[name] = i
    if "zeroY" in marks:
        Y[4, marks["zeroY"]] = 0.0                      # CO2 participates and is absent
    if "mostlyN2" in marks:
        Y[:, marks["mostlyN2"]] = [1e-3, 2e-3, 0.99, 4e-3, 3e-3]
    Y = Y / Y.sum(axis=0)
    return [np.ascontiguousarray(y) for y in Y], p, T, marks
