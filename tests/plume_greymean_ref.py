"""CPU restatement (test infrastructure, a helper, not a test) of the plume step with greyMeanAbsorptionEmission as the absorption /
emission model (ffm_plume_set_absorption_emission): tests/plume_radiation_ref.py (the rays) and tests/plume_p1_ref.py (P1) with the model
where they have the constant.  Neither is edited; the two classes here differ from them in three places:

 * the absorption coefficient is the cell field a = aCont() of tests/greymean_ref.py from the step's Y, p, T, formed afresh at every
   radiation->correct() and at every radiation->Sh (the reference's Rp() / Ru() call aCont() each time); e = a; P1 takes its patch values
   as the adjacent cells' (extrapolatedCalculated);
 * E = EhrrCoeff*Qdot in place of RadFraction*Qdot: rad_fraction() returns EhrrCoeff, the burner-patch sum drops out;
 * fields() carries aRad, the last a.
The parents' expressions take an array where they had the scalar, in the same operation order: V*(a*omega), (a*sigma)*T^4,
Rp = 4.0*a*sigma, Ru = a*G - E.  The participating species are those of the case data that the plume has (CO2, H2O; the plume has no CH4),
summed in the data's order.  Unpinned by reference data.  Only tests/ may import this module."""
import numpy as np

from oracle import oracle as O
from oracle import plume

import greymean_ref as GM
import p1_ref as P1
from plume_p1_ref import PlumeP1
from plume_radiation_ref import PlumeRadiation
from plume_thermo_ref import CONFIGS, TABLE, species, start_state

EHRR = 0.25                           # EhrrCoeff of the tests (the case data has 0: no emission term)
FREQ = 2
RAY_MODEL = (0.1, 0.5, 0.22)          # the constant model the opt-in replaces (plume_radiation_ref.RAD_MODEL)
P1_MODEL = (0.1, 0.3, 0.3)
EMISSIVITY = 0.8


def participating():
    """(coeffs, order): the case data's species that the plume transports"""
    fx = GM.fixture()
    order = [s for s in fx["species"] if s in plume.SPECIES]
    return {s: fx["coeffs"][s] for s in order}, order


def weights(thermo=True):
    return {s: float(TABLE[s]["W"]) for s in plume.SPECIES} if thermo else {s: float(w) for s, w in zip(plume.SPECIES, plume.WMOL)}


class _GreyMean:
    gm = None

    def set_absorption_emission(self, coeffs, order, EhrrCoeff, W):
        self.gm = dict(coeffs=coeffs, order=order, Ehrr=float(EhrrCoeff), W=W)

    def a_field(self):
        g = self.gm
        self.aRad = GM.aCont(plume.SPECIES, g["W"], g["coeffs"], g["order"], [np.ascontiguousarray(y) for y in self.Y], self.p, self.T)
        return self.aRad

    def rad_fraction(self):
        return self.gm["Ehrr"] if self.gm else super().rad_fraction()

    def radiation_sh(self, Qdot):
        if self.gm:
            self.rad_a = self.a_field()
        return super().radiation_sh(Qdot)

    def fields(self):
        out = super().fields()
        if self.gm and hasattr(self, "aRad"):
            out["aRad"] = self.aRad
        return out


class PlumeGreyMeanRays(_GreyMean, PlumeRadiation):
    def _radiation_correct_standin(self):
        if self.gm:
            self.rad_a = self.a_field()
        PlumeRadiation._radiation_correct_standin(self)


class PlumeGreyMeanP1(_GreyMean, PlumeP1):
    def _radiation_correct_standin(self):
        if not self.gm:
            return PlumeP1._radiation_correct_standin(self)
        m = self.m
        a = self.rad_a = self.a_field()
        self.radE = self.rad_fraction() * self.Qdot_field
        S = P1.system(m, a, a, self.radE, self.T, self.zg(self.T), self.p1_emissivity, sigma=plume.SIGMA_SB, a_b=self.zg(a))
        self.G, perf = P1.solve(O, m, S, self.G, tolerance=1e-6)
        self.sol.log.append(("G", perf))
        self.G_b, self.qr = P1.wall(m, S, self.G)


def ref_case(n, model, greymean=True, state="blob", config="thermo+kEqn+EDC"):
    """model "rays" or "P1"; kEqn + janaf thermo + EDC from the blob state, set up in the order the GPU test sets the device up"""
    from plume_keqn_ref import smooth_k0
    cfg = CONFIGS[config]
    ref = (PlumeGreyMeanRays if model == "rays" else PlumeGreyMeanP1)(n, conditioned=True)
    Y, h = start_state(ref.m, state)
    ref.set_state(Y, h)
    if cfg["turbulence"]:
        ref.set_turbulence(k0=smooth_k0(ref.m))
    ref.set_thermo(species())
    if cfg["edc"]:
        ref.set_combustion(**cfg["edc"])
    if model == "rays":
        ref.set_radiation(solverFreq=FREQ)
        ref.set_radiation_model(*RAY_MODEL)
    else:
        ref.set_radiation_p1(FREQ, *P1_MODEL, wallEmissivity=EMISSIVITY)
    if greymean:
        coeffs, order = participating()
        ref.set_absorption_emission(coeffs, order, EHRR, weights(True))
    return ref
