"""CPU restatement (test infrastructure) of the plume step with the fvDOM stand-in and radiation->Sh TOGETHER with the janaf / sutherland
thermo package and the reference's EDC (ffm_plume_set_radiation_thermo): tests/plume_thermo_ref.py's PlumeThermo with
radiation->correct() and radiation->Sh(thermo, he) put into its step where oracle/plume.py:445-446,462-470 has them:

 * radiation->correct() (solver/YEEqn.H:80) is the inherited _radiation_correct_standin: it reads self.T -- the thermo package's --
   and E = RadFraction*Qdot with Qdot of whichever combustion model is selected (self.Qdot_field); RadFraction, the ambient black-body
   inflow and the zero-gradient outflow are the stand-in's;
 * radiation->Sh (solver/YEEqn.H:101): Ru - fvm::Sp(4 Rp T^3/Cpv, he) - Rp T^3 (T - 4 he/Cpv) in the operation order of
   oracle/plume.py:464-468, Cpv = self.Cp (thermo.correct()'s cell field, at the T read here) where the thermo package is on, the
   constant plume.CP where it is not.
PlumeThermo.step asserts radFreq == 0, so this class carries a step of its own: PlumeThermo.step statement for statement plus the two
places above; with radiation off it reproduces PlumeThermo.step bitwise (tests/test_plume_radiation_cpu.py).

The plume with these models is unpinned by reference data, as the plume itself is.  Only tests/ may import this module."""
import numpy as np

from oracle import fv, plume
from oracle import steckler_case as SC
from plume_keqn_ref import PlumeKEqn
from plume_thermo_ref import CONFIGS, PlumeThermo, species, start_state


class PlumeRadiation(PlumeThermo):
    sh_constant_cp = False          # tests: radiation->Sh with plume.CP although the thermo package is on (what the new ground replaces)

    def sh_cp(self):
        return plume.CP if (self.thermo is None or self.sh_constant_cp) else self.Cp

    def radiation_sh(self, Qdot):
        """(ShSu, ShSp) of radiation->Sh(thermo, he) from the present G, T, h"""
        Cp = self.sh_cp()
        Rp = 4.0 * self.rad_a * plume.SIGMA_SB
        T3 = self.T * self.T * self.T
        Ru = self.rad_a * self.G - self.rad_fraction() * Qdot
        ShSp = 4.0 * Rp * T3 / Cp
        ShSu = Ru - Rp * T3 * (self.T - 4.0 * self.h / Cp)
        return ShSu, ShSp

    def step(self):
        if self.thermo is None and self.edc is None:
            # the stand-in physics: oracle/plume.py's own step has the radiation (without kEqn), PlumeKEqn's has none
            return PlumeKEqn.step(self) if self.turb else plume.Plume.step(self)
        assert not getattr(self, "adjust", False) and not getattr(self, "divU_scheme", None) and self.mv_selection and self.fvdom is None
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
        if self.radFreq > 0 and self.stepNo % self.radFreq == 0:          # radiation->correct(), solver/YEEqn.H:80 (oracle/plume.py:445-446)
            self._radiation_correct_standin()
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
        if self.rad_coupled and self.rays and hasattr(self, "radE"):      # + radiation->Sh(thermo, he) (oracle/plume.py:462-470)
            self.ShSu, self.ShSp = self.radiation_sh(Qdot)
            E.diag += m.V * self.ShSp
            E.add_su(self.ShSu)
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
        out = PlumeThermo.fields(self)
        if self.rays:
            out["G"] = self.G
        if hasattr(self, "ShSu"):
            out.update(ShSu=self.ShSu, ShSp=self.ShSp)
        return out


# ---- the case the CPU and GPU tests share ----------------------------------------------------------------------------------------
RAD_MODEL = (0.1, 0.5, 0.22)          # absorption [1/m], Ehrr1, Ehrr2 (cases/steckler/constant/radiationProperties:42-52 with a grey medium)
RAD_FREQ = 2                          # steps 0 and 2: a ray sweep and the separate EEqn; steps 1 and 3: h with the Sh source, no sweep


def ref_case(n, state, config, thermo=True, radiation=True, solvers=None):
    """the restatement set up in the order the GPU tests set the device up: start state, kEqn with the smooth k0, thermo, EDC, radiation"""
    from plume_keqn_ref import smooth_k0
    cfg = CONFIGS[config]
    ref = PlumeRadiation(n, conditioned=True, solvers=solvers)
    Y, h = start_state(ref.m, state)
    ref.set_state(Y, h)
    if cfg["turbulence"]:
        ref.set_turbulence(k0=smooth_k0(ref.m))
    if thermo:
        ref.set_thermo(species())
    if cfg["edc"]:
        ref.set_combustion(**cfg["edc"])
    if radiation:
        ref.set_radiation(solverFreq=RAD_FREQ)
        ref.set_radiation_model(*RAD_MODEL)
    return ref
