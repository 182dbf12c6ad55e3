"""CPU restatement (test infrastructure, a helper, not a test) of the plume step with the P1 radiation model (ffm_plume_set_radiation_p1):
tests/plume_radiation_ref.py's PlumeRadiation with radiation->correct() replaced by the P1 solve of tests/p1_ref.py.  Nothing else
differs: E = RadFraction*Qdot, radiation->Sh with the one constant for a and e, whether a step has a correct() -- all as for the rays.

radiation->correct() (solver/YEEqn.H:80): P1::calculate() with a = e = the absorption constant, no scattering, MarshakRadiation with the
one wall emissivity on every patch at the zero-gradient patch values of T, PCG + DIC at the `G` entry's controls (tolerance 1e-6, relTol 0;
cases/steckler/system/fvSolution:75-81) from the previous G, logged as "G"; then qr.

Unpinned by reference data: the reference ships no output of a P1 run.  Only tests/ may import this module."""
import numpy as np

from oracle import oracle as O
from oracle import plume

import p1_ref as P1
from plume_radiation_ref import PlumeRadiation
from plume_thermo_ref import start_state

P1_MODEL = (0.1, 0.3, 0.3)            # absorption [1/m], Ehrr1, Ehrr2
P1_FREQ = 2                           # steps 0 and 2: a P1 solve and the separate EEqn; steps 1 and 3: h with the Sh source, no solve


class PlumeP1(PlumeRadiation):
    p1_emissivity = 1.0

    def set_radiation_p1(self, solverFreq=1, absorption=0.1, Ehrr1=0.0, Ehrr2=0.0, wallEmissivity=1.0):
        if solverFreq <= 0:
            return
        self.set_radiation_model(absorption, Ehrr1, Ehrr2)
        self.radFreq = solverFreq
        self.rays, self.I = ("P1",), []          # (non-empty: radiation->Sh is on and fields() carries G)
        self.p1_emissivity = float(wallEmissivity)
        self.G = np.zeros(self.m.nCells)

    def _radiation_correct_standin(self):
        m = self.m
        self.radE = self.rad_fraction() * self.Qdot_field        # absorptionEmission->ECont(): RadFraction*Qdot
        S = P1.system(m, self.rad_a, self.rad_a, self.radE, self.T, self.zg(self.T), self.p1_emissivity, sigma=plume.SIGMA_SB)
        self.G, perf = P1.solve(O, m, S, self.G, tolerance=1e-6)
        self.sol.log.append(("G", perf))
        self.G_b, self.qr = P1.wall(m, S, self.G)

    def fields(self):
        out = PlumeRadiation.fields(self)
        if hasattr(self, "qr"):
            out["qr"] = np.concatenate(self.qr)
        return out


def ref_case(n, state="blob", solverFreq=P1_FREQ, model=P1_MODEL, wallEmissivity=1.0):
    """the stand-in physics from the start state of tests/plume_thermo_ref.py with P1 on"""
    ref = PlumeP1(n, conditioned=True)
    Y, h = start_state(ref.m, state)
    ref.set_state(Y, h)
    ref.set_radiation_p1(solverFreq, *model, wallEmissivity=wallEmissivity)
    return ref
