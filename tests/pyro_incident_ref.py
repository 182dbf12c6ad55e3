"""CPU restatement (test infrastructure) of what BASELINE config 1 (cases/pyrolysis1D) adds to oracle/pyrolysis.py's Panel, in the
operation order of csrc/ffm_pyro.hip:

 * fixedIncidentRadiation on the exposed face (lib/fvPatchFieldsPyrolysis/fixedIncidentRadiation/
   fixedIncidentRadiationFvPatchScalarField.C:155-213): gradient = e (QrIncident - sigma pow4(intFld))/kappa(*this), intFld the cell
   temperature before the step, e = absorptionEmission().e() of the exposed layer's composition after solveSpeciesMass; evaluated
   where Panel._evolve calls its `flux` closure (construction of hEqn).  The look-up of pyroCUPOneDimV1 models (:168-185) finds none
   for reactingOneDim(21) and does nothing.
 * qrHSource (reactingOneDim.C:95-144 updateqr, :335-339 solveEnergy; the same text in reactingOneDim21.C:96-145, 350-354): qr0 =
   max(qr0, 0) enters through the exposed face and is attenuated with kappaRad() = absorptionEmission().a() of the composition
   BEFORE the step (updateFields() runs before solveSpeciesMass, :686-705) over delta_0 = dx/2, delta_i = dx; hEqn gains
   fvc::div(fvc::interpolate(qr)*nMagSf()): face values qr0 | linear | zeroGradient back face, cell i gains A (qf_{i-1/2} - qf_{i+1/2}).
   The sign rests on regionModel1D::nMagSf (upstream OpenFOAM, not in the reference tree); it is the only one for which the column
   absorbs A (qr0 - qr_{N-1}) in total.  The source is added to the assembled right-hand side Panel._evolve returns, the system is
   solved again with oracle.pyrolysis.thomas and solidThermo.correct() repeated.

Tcrit: replaces the reaction's critical temperature for this panel (a value above every temperature reached switches it off).
Only tests/ may import this module."""
import json
import os

import numpy as np

from oracle import pyrolysis as PY

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pyrolysis1d_case_data.json")


def case_data():
    return json.load(open(FIXTURE))


def case_selections(case):
    """the fixture's selections as the keyword arguments of Panel / PyrolysisPanel.set_model"""
    s, b = case["solids"], case["panelT"]["back"]
    for name, ref in (("wood", PY.WOOD), ("char", PY.CHAR)):        # the solids and the reaction are the restatement's built-in ones
        assert (s[name]["rho"], s[name]["Cp"], s[name]["kappa"], s[name]["Hf"]) == (ref.rho, ref.Cp, ref.kappa, ref.Hf)
    r = case["reaction"]
    assert dict(A=r["A"], Ta=r["Ta"], Tcrit=r["Tcrit"], n=r["order"]) == PY.REACTION
    assert b["type"] == "constHTemperature" and case["panelT"]["exposed"]["type"] == "fixedIncidentRadiation"
    assert case["absorptionEmissionModel"] == "greyMeanSolidAbsorptionEmission" and case["panelSchemes"]["interpolationDefault"] == "linear"
    return dict(model=case["pyrolysis"]["pyrolysisModel"], alphaScheme=case["panelSchemes"]["laplacian(thermo:alpha,h)"],
                kappaScheme=case["panelSchemes"]["laplacian(kappa,T)"], back=("constH", b["h"], b["Tinf"]),
                radiation=dict(v=(s["wood"]["absorptivity"], s["wood"]["emissivity"]), char=(s["char"]["absorptivity"], s["char"]["emissivity"])))


class IncidentPanel(PY.Panel):
    def __init__(self, nCol, nLay=8, QrIncident=None, qr0=None, Tcrit=None, **kw):
        if Tcrit is not None:
            kw["reaction"] = dict(kw.get("reaction") or PY.REACTION, Tcrit=Tcrit)
        super().__init__(nCol, nLay, **kw)
        self.QrIncident = None if QrIncident is None else np.broadcast_to(np.asarray(QrIncident, float), (nCol,)).copy()
        self.qr0 = None if qr0 is None else np.broadcast_to(np.asarray(qr0, float), (nCol,)).copy()
        self.Tcrit = Tcrit

    def qr_field(self):
        """updateqr(): (qr at the cell centres [nCol][nLay], clipped qr0 [nCol]) from the present composition"""
        (aV, _), (aC, _) = self.radiation["v"], self.radiation["char"]
        X = self.Xw()
        kapR = X * aV + (1.0 - X) * aC
        q0 = np.maximum(self.qr0, 0.0)
        qr = np.empty((self.nCol, self.nLay))
        kappaInt = np.zeros(self.nCol)
        for i in range(self.nLay):
            kappaInt = kappaInt + kapR[:, i] * (0.5 * self.dx if i == 0 else self.dx)
            qr[:, i] = q0 * np.exp(-kappaInt)
        return qr, q0

    def _evolve(self, dt, flux, Tback):
        if self.qr0 is None:
            return super()._evolve(dt, flux, Tback)
        qr, q0 = self.qr_field()                               # before solveSpeciesMass
        res = super()._evolve(dt, flux, Tback)
        qf = np.empty((self.nCol, self.nLay + 1))
        qf[:, 0] = q0
        qf[:, 1:-1] = 0.5 * (qr[:, :-1] + qr[:, 1:])
        qf[:, -1] = qr[:, -1]
        S = self.A * (qf[:, :-1] - qf[:, 1:])
        res["src"] = res["src"] + S
        self.h = PY.thomas(res["lower"], res["diag"], res["upper"], res["src"])
        Cp = self.Cp()
        self.T = PY.TSTD + self.h / Cp
        self.alpha = self.kappa_vol() / Cp
        res["qr"], res["qrSource"] = qr, S
        return res

    def step_incident(self, dt):
        out = {}
        T_old0 = self.T[:, 0].copy()

        def flux(kap):
            _, e = self.surface_radiation()                         # the composition after solveSpeciesMass
            q = e * (self.QrIncident - PY.SIGMA_SB * ((T_old0 * T_old0) * (T_old0 * T_old0)))
            out["refGrad"] = q / kap
            out["e"] = e
            return q
        res = self._evolve(dt, flux, None)
        self.Twall = self.T[:, 0] + out["refGrad"] / (2.0 / self.dx)
        res["emissivity"] = out["e"]
        return res

    def run_incident(self, dt, nSteps, sampleEvery=None):
        """nSteps of step_incident; the history PyrolysisPanel.run_incident returns"""
        H = {k: [] for k in ("Twall", "phiGas", "T", "rho", "Yw", "chemistryQdot")}
        for s in range(nSteps):
            res = self.step_incident(dt)
            if sampleEvery and (s + 1) % sampleEvery == 0:
                for k, v in (("Twall", self.Twall), ("phiGas", self.massGas), ("T", self.T), ("rho", self.rho), ("Yw", self.Yw), ("chemistryQdot", res["Qdot"])):
                    H[k].append(np.array(v))
        return {k: np.array(v) for k, v in H.items()} if sampleEvery else None


NO_REACTION = 1.0e9          # Tcrit above any temperature: kf = 0


def equilibrium_setup(e):
    """Equilibrium temperature, run time and step of the equilibrium test, from its inputs.  The surface relaxes with the lumped time
    constant tau = rho Cp L/(4 e sigma Teq^3) (46 s for the case's wood at e = 0.17), but the slab is not lumped (Biot number
    4 e sigma Teq^3 L/kappa = 7 ... 35): the slowest mode of a slab with a Robin face and an adiabatic back decays with
    tau_1 = tcond/zeta_1^2, zeta_1 tan zeta_1 = Bi, tcond = L^2 rho Cp/kappa, and 1/zeta_1^2 <= 1/Bi + 4/pi^2, i.e. tau_1 <= tau +
    0.41 tcond.  The run lasts 20 (tau + tcond) >= 20 tau_1: the distance to equilibrium falls by e^-20 = 2e-9 of the initial 716 K,
    far below the bound of 1e-6 relative.  The patch is evaluated explicitly (T^4 of the old temperature), stable for deltaT below
    twice the exposed layer's own time constant tau/nLay (1.2 s at e = 0.85): deltaT = 0.5 s."""
    Qr, L = 60000.0, 0.0234
    Teq = (Qr / PY.SIGMA_SB) ** 0.25
    tau = PY.WOOD.rho * PY.WOOD.Cp * L / (4.0 * e * PY.SIGMA_SB * Teq ** 3)
    tcond = L * L * PY.WOOD.rho * PY.WOOD.Cp / PY.WOOD.kappa
    dt = 0.5
    return Qr, L, Teq, tau, int(np.ceil(20.0 * (tau + tcond) / dt)), dt
