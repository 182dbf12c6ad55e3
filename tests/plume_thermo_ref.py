"""CPU restatement (test infrastructure) of the plume step with the janaf / sutherland thermo package and the reference's EDC selected
(ffm_plume_set_thermo, ffm_plume_set_combustion): tests/plume_keqn_ref.py's PlumeKEqn with the places where the stand-in physics sat
taken by oracle/thermo.py -- pinned on the numbers the reference prints at start-up -- and by the expression of oracle/steckler_case.py's
edc_correct, which the golden log pins:

 * thermo.correct() (solver/YEEqn.H:114, solver/phrghEqn.H, set-up): Species.mixture by progressive mass-fraction sum, T = THs(h) by
   Newton from the old T, psi, sutherland mu, modified-Eucken alpha = kappa/Cp and Cp at the new T;
 * UEqn: laminar interpolate(mu) with zero-gradient patch values; with kEqn rho nuEff = rho (nut + mu/rho), mu the cell field;
 * alphaEff = alpha (+ alphat), one diffusivity for the species and h; patch alpha zero-gradient;
 * inlet enthalpy Hs(inlet mixture, T_IN); hAmb stays the case's;
 * combustion->correct(): eddyDissipationModel::correct with the step's deltaT, kEqn's Ce and delta, the thermo model's alpha (mu/Pr with
   the stand-in thermo); s and qFuel from thermo.SingleStep, the species' stoichiometric factors the plume's NU.
set_thermo redoes the start-up as the device does: T = TREF (the Newton start), thermo.correct(), rho = psi p, the hydrostatic
initialisation, correctNut() with the new rho where kEqn is on.  With every model off the class is PlumeKEqn unchanged.

The plume with these models is unpinned by reference data, as the plume itself is.  Only tests/ may import this module."""
import json
import os

import numpy as np

from oracle import fv, plume
from oracle import steckler_case as SC
from oracle import thermo as TH
from plume_keqn_ref import PlumeKEqn, SMALL

DATA = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "steckler_case_data.json")))
TABLE = {n: {k: (np.array(v) if isinstance(v, list) else v) for k, v in d.items()} for n, d in DATA["table"].items()}
assert DATA["species"] == plume.SPECIES


def species():
    return TH.Species(DATA["species"], TABLE)


def single_step(sp=None):
    rx = DATA["reaction"]
    return TH.SingleStep(sp or species(), [tuple(t) for t in rx["lhs"]], [tuple(t) for t in rx["rhs"]], fuel=DATA["fuel"], inert=DATA["inertSpecie"])


def blob_state(m, sp=None):
    """plume.conditioned_state with a hot fuel blob in the middle of the box: g = exp(-|s - 0.5|^2/0.05), s the cell centre in unit-box
    coordinates; Y[C3H8] += 0.3 g, Y[N2] -= 0.3 g, h = Hs(mixture, 300 + 1100 g).  Cells on both sides of Tcommon = 1000 K, O2-limited
    cells in the blob and fuel-limited ones around it (tests/test_plume_thermo_cpu.py)"""
    sp = sp or species()
    Y, _ = plume.conditioned_state(m, plume.Y_AMB_COND, plume.H_AMB_COND)
    lo, hi = m.C.min(axis=0), m.C.max(axis=0)
    s = (m.C - lo) / np.where(hi > lo, hi - lo, 1.0)
    g = np.exp(-((s - 0.5) ** 2).sum(axis=1) / 0.05)
    Y = Y.copy()
    Y[2] += 0.3 * g; Y[plume.INERT] -= 0.3 * g
    return Y, sp.mixture(Y).Hs(0.0, 300.0 + 1100.0 * g)


class PlumeThermo(PlumeKEqn):
    thermo = None           # a thermo.Species: the janaf package on
    edc = None              # dict(C_EDC, C_Diff, C_Stiff, s, qFuel): the reference's EDC on

    # ---- selection ------------------------------------------------------------------------------------------------
    def set_thermo(self, sp):
        assert self.stepNo == 0
        self.thermo = sp
        self.inlet_h = None if sp is None else float(sp.mixture(np.asarray(self.Y_in, float)).Hs(0.0, np.array([plume.T_IN]))[0])
        self.start_up()

    def set_state(self, Y, h):
        """ffm_plume_set_initial_state with the case's own ambient / inlet values: a restart from time 0"""
        N = self.m.nCells
        self.Y, self.h = np.array(Y, dtype=np.float64), np.array(h, dtype=np.float64)
        self.U = np.zeros((3, N)); self.K = np.zeros(N); self.dpdt = np.zeros(N)
        self.phi = np.zeros(self.m.nFaces); self.phib = [np.zeros(p.size) for p in self.m.patches]
        self.stepNo, self.time = 0, 0.0
        self.start_up(renut=self.thermo is not None)

    def start_up(self, renut=True):
        N = self.m.nCells
        self.p = np.full(N, plume.PREF)
        if self.thermo is not None:
            self.T = np.full(N, plume.TREF)
        self.sol.log = []
        self.thermo_correct()
        self.rho = self.psi * self.p
        self.hydrostatic_init()
        if renut and self.turb:
            self.kb = self.bc_k().values(self.m, self.k)
            self.correct_nut()

    def set_combustion(self, C_EDC=4.0, C_Diff=0.0, C_Stiff=1.0, s=None, qFuel=None, on=True):
        if not on:
            self.edc = None
            return
        assert self.turb
        rx = single_step()
        self.edc = dict(C_EDC=C_EDC, C_Diff=C_Diff, C_Stiff=C_Stiff, s=rx.s if s is None else s, qFuel=rx.qFuel if qFuel is None else qFuel)

    # ---- the thermo package ---------------------------------------------------------------------------------------
    def calc_psi(self):
        if self.thermo is None:
            return PlumeKEqn.calc_psi(self)
        return self.thermo.mixture(self.Y).psi(self.p, self.T)

    def thermo_correct(self):
        if self.thermo is None:
            return PlumeKEqn.thermo_correct(self)
        mix = self.thermo.mixture(self.Y)
        Told = self.T
        self.T = mix.THs(self.h, self.p, Told)
        self.newton_moved = np.abs(self.T - Told) > Told * 1.0e-4          # cells whose first iterate was not accepted
        self.psi = mix.psi(self.p, self.T)
        self.mu = mix.mu(self.p, self.T)
        self.alpha = mix.alphah(self.p, self.T)
        self.Cp = mix.Cp(self.p, self.T)
        self.mix = mix

    def mu_cells(self):
        return np.full(self.m.nCells, plume.MU) if self.thermo is None else self.mu

    def alpha_cells(self):
        return np.full(self.m.nCells, plume.MU / plume.PR) if self.thermo is None else self.alpha

    def rho_nuEff(self):
        if self.thermo is None:
            return PlumeKEqn.rho_nuEff(self)
        rhob, mub = self.zg(self.rho), self.zg(self.mu)
        return self.rho * (self.nut + self.mu / self.rho), [r * (n + mb / r) for r, n, mb in zip(rhob, self.nutb, mub)]

    def alpha_eff_faces(self):
        m, a = self.m, self.alpha_cells()
        if self.turb:
            return fv.interpolate(m, a + self.alphat, [ab + t for ab, t in zip(self.zg(a), self.alphatb)])
        return fv.interpolate(m, a, self.zg(a))

    def inlet_enthalpy(self):
        return plume.CP * (plume.T_IN - plume.TREF) if self.inlet_h is None else self.inlet_h

    # ---- combustion->correct() ------------------------------------------------------------------------------------
    def combustion_correct(self):
        fuel, o2 = self.Y[2], self.Y[0]
        if self.edc is None:
            self.wFuel = self.rho * np.minimum(fuel, o2 / plume.S_O2) / plume.TAU
            self.Qdot = self.wFuel * plume.HC
            return
        c = self.edc
        eps = self.Ce * self.k * np.sqrt(self.k) / self.delta                                  # oracle/steckler_case.py: edc_correct
        self.rtTurb = c["C_EDC"] * eps / np.maximum(self.k, SMALL)
        self.rtDiff = c["C_Diff"] * self.alpha_cells() / self.rho / self.delta ** 2
        rt = np.maximum(self.rtTurb, self.rtDiff)
        self.wFuel = self.rho * np.minimum(fuel, o2 / c["s"]) / self.dt / c["C_Stiff"] * (1.0 - np.exp(-c["C_Stiff"] * self.dt * rt))
        self.Qdot = c["qFuel"] * self.wFuel
        self.o2_limited = o2 / c["s"] < fuel

    # ---- one time step: PlumeKEqn.step() with the selected models ----------------------------------------------------
    def step(self):
        if self.thermo is None and self.edc is None:
            return PlumeKEqn.step(self)
        assert self.radFreq == 0 and not getattr(self, "adjust", False) and not getattr(self, "divU_scheme", None) and self.mv_selection
        m, rdt = self.m, self.rDeltaT
        self.sol.log = []
        self.rho0, self.U0, self.h0, self.Y0 = self.rho.copy(), self.U.copy(), self.h.copy(), self.Y.copy()
        self.K0, self.p0, self.psi0, self.p_rgh0 = self.K.copy(), self.p.copy(), self.psi.copy(), self.p_rgh.copy()
        self.phi0, self.phib0 = self.phi.copy(), [b.copy() for b in self.phib]
        self.rho_eqn()
        # ---- UEqn.H
        bcU = self.bc_U()
        Ub, Ub3 = self._Ub3(bcU)
        if self.turb:
            gam, gamb = self.rho_nuEff()
        else:
            gam = self.mu_cells(); gamb = self.zg(gam)
        muf, _ = fv.interpolate(m, gam, gamb)
        UEqn = fv.fvm_ddt(m, rdt, self.rho, self.rho0, self.U0)
        zb = [np.zeros(p.size) for p in m.patches]
        divU = fv.fvm_div(m, self.phi, self.phib, fv.lust_weights(m, self.phi), bcU)
        divU.add_vol(np.stack([fv.surface_integrate(m, self.phi * fv.lust_correction(m, self.phi, fv.grad(m, self.U[c], Ub[c])), zb)
                               for c in range(3)]))
        UEqn += divU
        UEqn -= fv.fvm_laplacian(m, muf, gamb, bcU)
        if self.turb:
            gU, gUb = SC.grad_vector(m, self.U.T.copy(), Ub3)
            X = gam[:, None, None] * SC.dev2T(gU); Xb = [g[:, None, None] * SC.dev2T(t) for g, t in zip(gamb, gUb)]
            UEqn.add_vol(-SC.div_tensor(m, X, Xb).T)
        rhob = self.zg(self.rho)
        sgr, _ = fv.snGrad(m, self.rho, rhob)
        bcp = self.bc_p_rgh([np.zeros(p.size) for p in m.patches])
        sgp, sgpb = fv.snGrad(m, self.p_rgh, self.p_rgh_b if self.stored_bc else bcp.values(m, self.p_rgh))
        rec = fv.reconstruct(m, (-self.ghf * sgr - sgp) * m.magSf, [-s * p.magSf for s, p in zip(sgpb, m.patches)])
        for c in range(3):
            d, s = UEqn.solve_system(c)
            s = s + m.V * rec[:, c]
            self.U[c] = self.sol.solve("U", "U" + "xyz"[c], m, d, UEqn.upper, UEqn.lower, s, self.U[c])
        self.K = 0.5 * (self.U ** 2).sum(axis=0)
        # ---- YEEqn.H
        af, afb = self.alpha_eff_faces()
        self.combustion_correct()
        wFuel, Qdot = self.wFuel, self.Qdot
        self.Qdot_field = Qdot
        nsp = len(plume.SPECIES)
        bch = self.bc_scalar(self.inlet_enthalpy(), self.h_amb, floor_fixed=0.0)
        lim = fv.limited_limiter(m, "limitedLinear", self.phi, self.h, fv.grad(m, self.h, bch.values(m, self.h)), 1.0)
        Ytb = [np.zeros(p.size) for p in m.patches]
        for i in range(nsp):
            if i == plume.INERT:
                continue
            Yb = self.bc_scalar(self.Y_in[i], self.Y_amb[i]).values(m, self.Y[i])
            Ytb = [a + np.maximum(b, 0.0) for a, b in zip(Ytb, Yb)]
            lim = np.minimum(lim, fv.limited_limiter(m, "limitedLinear01", self.phi, self.Y[i], fv.grad(m, self.Y[i], Yb), 1.0))
        Nb = [np.maximum(1.0 - b, 0.0) for b in Ytb]
        lim = np.minimum(lim, fv.limited_limiter(m, "limitedLinear01", self.phi, self.Y[plume.INERT], fv.grad(m, self.Y[plume.INERT], Nb), 1.0))
        w_mv = lim * m.weights + (1.0 - lim) * fv.pos0(self.phi)
        self.w_mv_last = w_mv
        Yt = np.zeros(m.nCells)
        for i in range(nsp):
            if i == plume.INERT:
                continue
            bc = self.bc_scalar(self.Y_in[i], self.Y_amb[i])
            E = fv.fvm_ddt(m, rdt, self.rho, self.rho0, self.Y0[i])
            E += fv.fvm_div(m, self.phi, self.phib, w_mv, [bc])
            E -= fv.fvm_laplacian(m, af, afb, [bc])
            E.add_su(plume.NU[i] * wFuel)
            d, s = E.solve_system()
            self.Y[i] = np.maximum(self.sol.solve("Yi", plume.SPECIES[i], m, d, E.upper, E.lower, s, self.Y[i]), 0.0)
            Yt += self.Y[i]
        self.Y[plume.INERT] = np.maximum(1.0 - Yt, 0.0)
        Ub = [b.values(m, self.U[c]) for c, b in enumerate(bcU)]
        Kb = [0.5 * sum(Ub[c][q] ** 2 for c in range(3)) for q in range(len(m.patches))]
        wK = fv.limited_weights(m, "limitedLinear", self.phi, self.K, fv.grad(m, self.K, Kb), 1.0)
        Kf = wK * self.K[m.l] + (1.0 - wK) * self.K[m.u]
        E = fv.fvm_ddt(m, rdt, self.rho, self.rho0, self.h0)
        E += fv.fvm_div(m, self.phi, self.phib, w_mv, [bch])
        E -= fv.fvm_laplacian(m, af, afb, [bch])
        E.add_vol(rdt * (self.rho * self.K - self.rho0 * self.K0))
        E.add_vol(fv.surface_integrate(m, self.phi * Kf, [pb * kb for pb, kb in zip(self.phib, Kb)]))
        E.add_vol(-self.dpdt)
        E.add_su(Qdot)
        d, s = E.solve_system()
        self.h = self.sol.solve("h", "h", m, d, E.upper, E.lower, s, self.h)
        self.thermo_correct()
        # ---- pEqn.H, nCorrectors = 2
        for corr in range(2):
            self.p_corrector(UEqn, final=(corr == 1))
        if self.turb:
            self.k_eqn()                                 # turbulence->correct()
        self.rho = self.psi * self.p
        self.time += self.dt
        self.stepNo += 1

    def fields(self):
        out = PlumeKEqn.fields(self)
        out["psi"] = self.psi
        if self.thermo is not None:
            out.update(mu=self.mu, alpha=self.alpha, Cp=self.Cp)
        if self.thermo is not None or self.edc is not None:
            if hasattr(self, "wFuel"):
                out.update(wFuel=self.wFuel, Qdot=self.Qdot)
        return out


# ---- the cases the CPU and GPU tests share ---------------------------------------------------------------------------------------
# C_Diff of the second EDC parameter set: with the blob state's alpha/rho/delta^2 of 0.009 - 0.096 1/s and rtTurb = C_EDC Ce sqrt(k)/delta
# of 3.7 - 4.8 1/s, 60 puts rtDiff at 0.55 - 5.8 1/s: above rtTurb in the hot cells, below it in the cold ones
# (tests/test_plume_thermo_cpu.py asserts both)
C_DIFF_2 = 60.0
CONFIGS = {"thermo": dict(turbulence=False, edc=None),
           "thermo+kEqn+EDC": dict(turbulence=True, edc=dict(C_EDC=4.0, C_Diff=0.0, C_Stiff=1.0)),
           "thermo+kEqn+EDC,C_Diff": dict(turbulence=True, edc=dict(C_EDC=4.0, C_Diff=C_DIFF_2, C_Stiff=1.0))}
STATES = ("conditioned", "blob")


def start_state(m, state):
    return blob_state(m) if state == "blob" else plume.conditioned_state(m, plume.Y_AMB_COND, plume.H_AMB_COND)


def ref_case(n, state, config, thermo=True, solvers=None):
    """the restatement set up in the order the GPU tests set the device up: start state, kEqn with the smooth k0, thermo, EDC"""
    from plume_keqn_ref import smooth_k0
    cfg = CONFIGS[config]
    ref = PlumeThermo(n, conditioned=True, solvers=solvers)
    Y, h = start_state(ref.m, state)
    ref.set_state(Y, h)
    if cfg["turbulence"]:
        ref.set_turbulence(k0=smooth_k0(ref.m))
    if thermo:
        ref.set_thermo(species())
    if cfg["edc"]:
        ref.set_combustion(**cfg["edc"])
    return ref
