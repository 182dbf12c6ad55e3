"""CPU restatement (test infrastructure) of the plume step with the LES kEqn sub-grid model (ffm_plume_set_turbulence): oracle/plume.py's
Plume with the three places where oracle/steckler_case.py -- which the golden log pins -- has the model, composed from oracle/fv.py and
that module's tensor helpers:

 * UEqn (solver/UEqn.H:7, StecklerCase.U_eqn / nuEff_rho): turbulence->divDevRhoReff(U) = - fvm::laplacian(rho nuEff, U)
   - fvc::div(rho nuEff dev2(T(grad U))), rho nuEff = rho (nut + mu/rho) with the rho of rhoEqn and zero-gradient patch values of rho;
 * YEEqn (solver/YEEqn.H:12, StecklerCase.alphaEff): alphaEff = alpha + alphat for the species and h, alphat of the last correctNut();
 * turbulence->correct() after the second corrector (solver/fireFoam.C:113-116, StecklerCase.k_eqn / correct_nut), before
   rho = thermo.rho(): the k equation solved by the controls of h, bound(k, SMALL), correctNut().
The plume's constants (MU, PR) and patches: k fixed kInlet on the inlet, inletOutlet(kInlet) on top / sides, zeroGradient on the floor
(the pattern of the species); nut and alphat zeroGradient, 0 on the floor.  k keeps the patch values evaluated after its last solve
(before bounding); at the start they are its condition's with the present phib.  The two implicit sources of the k equation enter the
diagonal as ONE sum, max(s, 0) + Ce rho sqrt(k)/delta, the order the device fixes for both of its forms.

The plume with kEqn is unpinned by reference data, as the plume itself is.  Only tests/ may import this module."""
import numpy as np

from oracle import fv, plume
from oracle import steckler_case as SC

SMALL = 1.0e-15
CK, CE, PRT, K_INLET = 0.094, 1.048, 1.0, 1.0e-4            # cases/steckler/constant/turbulenceProperties:18-30, cases/steckler/0/k


def smooth_k0(m, base=2.0e-3, amp=0.5):
    """a smooth, nowhere-uniform start field for k (amplitude far above rounding: limitedLinear's r is then formed from differences of
    the field, not of solver noise), large enough for nut to be of the order of mu/rho on a 5 cm mesh"""
    lo, hi = m.C.min(axis=0), m.C.max(axis=0)
    s = (m.C - lo) / (hi - lo)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    return base * (1.0 + amp * ((0.7 * x + 1.0 * y + 0.5 * z) / 2.2 + 0.25 * (0.5 * x * x + 0.7 * y * y + z * z) / 2.2))


class PlumeKEqn(plume.Plume):
    turb = False

    def set_turbulence(self, Ck=CK, Ce=CE, Prt=PRT, kInlet=K_INLET, k0=None):
        m = self.m
        self.Ck, self.Ce, self.Prt, self.kInlet = Ck, Ce, Prt, kInlet
        self.delta = np.cbrt(m.V)
        self.k = np.full(m.nCells, kInlet) if k0 is None else np.array(k0, dtype=np.float64)
        self.kb = self.bc_k().values(m, self.k)
        self.correct_nut()
        self.turb = True

    def bc_k(self):
        return self.bc_scalar(self.kInlet, self.kInlet)

    def _zg0(self, vf):
        """zeroGradient, fixedValue 0 on the floor"""
        return [np.zeros(p.size) if p.name == "floor" else vf[p.faceCells].copy() for p in self.m.patches]

    def correct_nut(self):
        self.nut = self.Ck * np.sqrt(self.k) * self.delta
        self.nutb = self._zg0(self.nut)
        self.alphat = self.rho * self.nut / self.Prt
        self.alphatb = self._zg0(self.alphat)

    def rho_nuEff(self):
        rhob = self.zg(self.rho)
        return self.rho * (self.nut + plume.MU / self.rho), [r * (n + plume.MU / r) for r, n in zip(rhob, self.nutb)]

    def _Ub3(self, bcU):
        Ub = [b.values(self.m, self.U[c]) for c, b in enumerate(bcU)]
        return Ub, [np.stack([Ub[c][q] for c in range(3)], axis=1) for q in range(len(self.m.patches))]

    # ---- one time step: Plume.step() with the model's terms (no radiation, LUST for div(phi,U)) -----------------
    def step(self):
        if not self.turb:
            return plume.Plume.step(self)
        assert self.radFreq == 0 and not getattr(self, "adjust", False) and not getattr(self, "divU_scheme", None) and self.mv_selection
        m, rdt = self.m, self.rDeltaT
        MU, PR, CP, TREF, T_IN = plume.MU, plume.PR, plume.CP, plume.TREF, plume.T_IN
        self.sol.log = []
        self.rho0, self.U0, self.h0, self.Y0 = self.rho.copy(), self.U.copy(), self.h.copy(), self.Y.copy()
        self.K0, self.p0, self.psi0, self.p_rgh0 = self.K.copy(), self.p.copy(), self.psi.copy(), self.p_rgh.copy()
        self.phi0, self.phib0 = self.phi.copy(), [b.copy() for b in self.phib]
        self.rho_eqn()
        # ---- UEqn.H
        bcU = self.bc_U()
        Ub, Ub3 = self._Ub3(bcU)
        gam, gamb = self.rho_nuEff()
        muf, _ = fv.interpolate(m, gam, gamb)
        UEqn = fv.fvm_ddt(m, rdt, self.rho, self.rho0, self.U0)
        zb = [np.zeros(p.size) for p in m.patches]
        divU = fv.fvm_div(m, self.phi, self.phib, fv.lust_weights(m, self.phi), bcU)
        divU.add_vol(np.stack([fv.surface_integrate(m, self.phi * fv.lust_correction(m, self.phi, fv.grad(m, self.U[c], Ub[c])), zb)
                               for c in range(3)]))
        UEqn += divU
        UEqn -= fv.fvm_laplacian(m, muf, gamb, bcU)
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
        alphaEff = MU / PR + self.alphat
        af, afb = fv.interpolate(m, alphaEff, [MU / PR + b for b in self.alphatb])
        fuel, o2 = self.Y[2], self.Y[0]
        wFuel = self.rho * np.minimum(fuel, o2 / plume.S_O2) / plume.TAU
        Qdot = wFuel * plume.HC
        self.Qdot_field = Qdot
        nsp = len(plume.SPECIES)
        bch = self.bc_scalar(CP * (T_IN - TREF) if self.inlet_h is None else self.inlet_h, self.h_amb, floor_fixed=0.0)
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
        self.k_eqn()                                     # turbulence->correct()
        self.rho = self.psi * self.p
        self.time += self.dt
        self.stepNo += 1

    def k_eqn(self):
        """StecklerCase.k_eqn on the plume"""
        m, rdt = self.m, self.rDeltaT
        rhob = self.zg(self.rho)
        rhof, _ = fv.interpolate(m, self.rho, rhob)
        divU = fv.surface_integrate(m, self.phi / rhof, [a / b for a, b in zip(self.phib, rhob)])
        _, Ub3 = self._Ub3(self.bc_U())
        gU, _ = SC.grad_vector(m, self.U.T.copy(), Ub3)
        twoSymm = gU + np.swapaxes(gU, 1, 2)
        tr = (twoSymm[:, 0, 0] + twoSymm[:, 1, 1]) + twoSymm[:, 2, 2]
        dev = twoSymm.copy()
        for a in range(3):
            dev[:, a, a] = dev[:, a, a] - (1.0 / 3.0) * tr
        self.Gk = Gk = self.nut * np.einsum("nij,nij->n", gU, dev)
        bck = self.bc_k()
        Dk, Dkb = self.rho_nuEff()
        Dkf, _ = fv.interpolate(m, Dk, Dkb)
        w = fv.limited_weights(m, "limitedLinear", self.phi, self.k, fv.grad(m, self.k, self.kb), 1.0)
        self.wk_last = w
        k0 = self.k.copy()
        E = fv.fvm_ddt(m, rdt, self.rho, self.rho0, k0)
        E += fv.fvm_div(m, self.phi, self.phib, w, [bck])
        E -= fv.fvm_laplacian(m, Dkf, Dkb, [bck])
        E.add_su(self.rho * Gk)
        ss = (2.0 / 3.0) * self.rho * divU
        E.source[0] -= m.V * np.minimum(ss, 0.0) * k0
        E.diag += m.V * (np.maximum(ss, 0.0) + self.Ce * self.rho * np.sqrt(k0) / self.delta)
        d, s = E.solve_system()
        self.k = self.sol.solve("h", "k", m, d, E.upper, E.lower, s, self.k)
        self.kb = bck.values(m, self.k)
        self.k = np.maximum(self.k, SMALL)
        self.correct_nut()

    def fields(self):
        out = plume.Plume.fields(self)
        if self.turb:
            out.update(k=self.k, nut=self.nut, alphat=self.alphat)
        return out
