"""CPU restatement (test infrastructure, a helper, not a test) of the reference's P1 radiation model on any mesh oracle/fv.py handles
(oracle.plume.make_mesh, tests/merged_mesh.py), written from the C++ statement by statement:

  P1::calculate()  packages/thermophysicalModels/radiation/radiationModels/P1/P1.C:213-258
      gamma = 1.0/(3.0*a + 3.0*sigmaEff + a0)                      a0 = ROOTVSMALL (OpenFOAM's 1.0e-150 for doubles: upstream's
      solve(fvm::laplacian(gamma, G) - fvm::Sp(a, G)                constant, restated from knowledge, not in the reference tree)
            == -4.0*(e*sigma*pow4(T)) - E)
      qr_b = -gamma_b*G_b.snGrad()
  sigmaEff = sigma_s*(3.0 - C)                                     submodels/scatterModel/constantScatter/constantScatter.C:87
  P1::Rp() = 4.0*e*sigma,  P1::Ru() = a*G - E                      P1.C:261-293
  MarshakRadiationFvPatchScalarField::updateCoeffs()               derivedFvPatchFields/MarshakRadiation/...C:156-190
      refValue = 4.0*sigma*pow4(T_b), refGrad = 0, Ep = emissivity/(2*(2 - emissivity)),
      valueFraction = 1.0/(1.0 + gamma_b*deltaCoeffs/Ep)

in the operation order the device kernels keep: pow4(x) = (x*x)*(x*x); the denominator (3.0*a + 3.0*sigmaEff) + a0; the source
(-(4.0*((e*sigma)*T4))) - E; the fraction 1.0/(1.0 + (gamma_b*delta_b)/Ep) -- emissivity 0 gives Ep = 0, +inf and the fraction 0 exactly.
Built on oracle.fv (interpolate, fvm_laplacian, MixedBC) and solved with the oracle's PCG + DIC.  Only tests/ may import this module."""
import numpy as np

from oracle import fv

SIGMA = 5.670367e-8
A0 = 1.0e-150


def pow4(x):
    return (x * x) * (x * x)


def gamma(a, sigmaEff):
    return 1.0 / ((3.0 * a + 3.0 * sigmaEff) + A0)


def per_patch(m, v):
    """a scalar, or a list with one array per patch -> the list"""
    return [np.asarray(x, np.float64) for x in v] if isinstance(v, (list, tuple)) else [np.full(p.size, float(v)) for p in m.patches]


def marshak(m, sigma, gamma_b, T_b, emissivity):
    """(valueFraction, refValue) per patch"""
    f, ref = [], []
    for p, gb, tb, e in zip(m.patches, gamma_b, T_b, emissivity):
        with np.errstate(divide="ignore"):
            Ep = e / (2.0 * (2.0 - e))
            f.append(1.0 / (1.0 + (gb * p.deltaCoeffs) / Ep))
        ref.append((4.0 * sigma) * pow4(tb))
    return f, ref


class System:
    """the equation of P1::calculate() for given fields: M (oracle.fv.Matrix before the boundary coefficients are added), d / s (what the
    solver takes), upper, bc (the Marshak condition as an oracle.fv.MixedBC), gamma_b per patch"""


def system(m, a, e, E, T, T_b, emissivity, sigma_s=0.0, C=0.0, sigma=SIGMA, a_b=None):
    """a, e, E: scalars or cell arrays; a_b: the patch values of a (default: the scalar a; a cell array needs them given)"""
    N = m.nCells
    cells = lambda v: np.full(N, float(v)) if np.ndim(v) == 0 else np.asarray(v, np.float64)
    if a_b is None:
        assert np.ndim(a) == 0, "patch values of the absorption field wanted"
        a_b = a
    ac, ec, Ec = cells(a), cells(e), cells(E)
    sigmaEff = sigma_s * (3.0 - C)
    S = System()
    gam = gamma(ac, sigmaEff)
    S.gamma_b = [gamma(x, sigmaEff) for x in per_patch(m, a_b)]
    f, ref = marshak(m, sigma, S.gamma_b, per_patch(m, T_b), per_patch(m, emissivity))
    S.bc = fv.MixedBC(m, f=f, ref=ref)
    gf, _ = fv.interpolate(m, gam, S.gamma_b)
    M = fv.fvm_laplacian(m, gf, S.gamma_b, [S.bc])
    M.diag = M.diag - m.V * ac                                       # - fvm::Sp(a, G)
    M.add_su((-(4.0 * ((ec * sigma) * pow4(np.asarray(T, np.float64))))) - Ec)
    S.M, S.upper = M, M.upper
    S.d, S.s = M.solve_system()
    return S


def solve(O, m, S, G0, tolerance=1e-6):
    """PCG + DIC, relTol 0 (the `G` entry of cases/steckler/system/fvSolution:75-81); returns (G, perf)"""
    return O.Ldu(m.nCells, m.l, m.u).set_coeffs(S.d, S.upper, None).solve(O.PCG, O.DIC, G0, S.s, tolerance=tolerance, relTol=0.0, maxIter=1000)


def wall(m, S, G):
    """(G_b, qr) per patch: the mixed evaluate and qr = -gamma_b*snGrad"""
    Gb = S.bc.values(m, G)
    _, sn = fv.snGrad(m, G, Gb)
    return Gb, [-gb * s for gb, s in zip(S.gamma_b, sn)]


def residual(m, S, G):
    """b - A G of the assembled system"""
    r = S.s - S.d * G
    np.subtract.at(r, m.l, S.upper * G[m.u])
    np.subtract.at(r, m.u, S.upper * G[m.l])
    return r


def Ru(a, G, E):
    return a * G - E


def Rp(e, sigma=SIGMA):
    return 4.0 * e * sigma


class P1:
    """the model as a handle: correct() every solverFreq-th call from the previous G, as radiationModel::correct() (radiationModel.C:209-226)"""

    def __init__(self, O, m, a, e, sigma_s=0.0, C=0.0, sigma=SIGMA, solverFreq=1, tolerance=1e-6, emissivity=1.0):
        self.O, self.m, self.a, self.e, self.sigma_s, self.C, self.sigma = O, m, a, e, sigma_s, C, sigma
        self.solverFreq, self.tolerance, self.emissivity = solverFreq, tolerance, emissivity
        self.G = np.zeros(m.nCells)
        self.calls, self.log = 0, []

    def correct(self, T, T_b, E=0.0):
        self.calls += 1
        if self.solverFreq <= 0 or (self.calls - 1) % self.solverFreq != 0:
            return False
        self.S = system(self.m, self.a, self.e, E, T, T_b, self.emissivity, self.sigma_s, self.C, self.sigma)
        self.G, perf = solve(self.O, self.m, self.S, self.G, self.tolerance)
        self.G_b, self.qr = wall(self.m, self.S, self.G)
        self.log.append(perf)
        return True
