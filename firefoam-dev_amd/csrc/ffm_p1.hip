// ffm_p1.hip -- SURVEY row 25: the P1 radiation model (reference packages/thermophysicalModels/radiation/radiationModels/P1/P1.C:213-258)
// and its wall condition, MarshakRadiationFvPatchScalarField::updateCoeffs (derivedFvPatchFields/MarshakRadiation/
// MarshakRadiationFvPatchScalarField.C:156-190).  One symmetric Helmholtz-type equation for the incident radiation G,
//   gamma = 1/(3 a + 3 sigmaEff + a0);  fvm::laplacian(gamma, G) - fvm::Sp(a, G) == -4 e sigma T^4 - E,
// every patch a `mixed` one with refValue 4 sigma T_b^4, refGrad 0, valueFraction 1/(1 + gamma_b deltaCoeffs/Ep),
// Ep = emissivity/(2 (2 - emissivity)); the wall flux is qr_b = -gamma_b snGrad(G)_b.  The solve is the library's PCG + DIC
// (cases/steckler/system/fvSolution:75-81); the matrix is negative definite like the hydrostatic Laplacians.
// Operation order (the per-operator chain is the specification, every entry point here equals it bit for bit):
//   pow4(x) = (x*x)*(x*x);  gamma = 1.0/((3.0*a + 3.0*sigmaEff) + a0);  su = (-(4.0*((e*sigma)*T4))) - E;
//   valueFraction = 1.0/(1.0 + (gamma_b*delta_b)/Ep): emissivity 0 gives Ep = 0, a quotient of +inf and the fraction 0 exactly,
//   a reflecting wall -- IEEE arithmetic, kept as it is.
#include "ffm_mesh.hpp"

// a0 of P1.C:222, ROOTVSMALL: OpenFOAM's 1.0e-150 for doubles.  The constant is upstream's (src/OpenFOAM/primitives/Scalar), not in
// the reference tree: restated from knowledge of OpenFOAM.
#define P1_A0 1.0e-150

__device__ __forceinline__ double p1_gamma(double a, double s3) { return 1.0 / ((3.0 * a + s3) + P1_A0); }
__device__ __forceinline__ double p1_pow4(double t) { return (t * t) * (t * t); }
// the Marshak coefficients of one boundary face
__device__ __forceinline__ void p1_marshak(double sigma, double gb, double dk, double tb, double eps, double &f, double &ref)
{
    const double Ep = eps / (2.0 * (2.0 - eps));
    ref = (4.0 * sigma) * p1_pow4(tb);
    f = 1.0 / (1.0 + (gb * dk) / Ep);
}

__global__ void k_p1_gamma(long n, const double *__restrict__ a, double aConst, double s3, double *__restrict__ gamma)
{ GRID_STRIDE(i, n) gamma[i] = p1_gamma(a ? a[i] : aConst, s3); }

extern "C" int ffm_p1_gamma_d(ffm_ctx *ctx, long n, const double *a_d, double aConst, double sigmaEff, double *gamma_d)
{
    if (!ctx || n < 0 || !gamma_d) return FFM_ERR_ARG;
    if (n == 0) return FFM_OK;
    FFM_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_p1_gamma, dim3(sgrid(n)), dim3(256), 0, ctx->stream, n, a_d, aConst, 3.0 * sigmaEff, gamma_d);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

__global__ void k_p1_marshak(int B, double sigma, const double *__restrict__ gb, const double *__restrict__ delta, const double *__restrict__ Tb,
                             const double *__restrict__ emis, double *__restrict__ f, double *__restrict__ ref)
{
    GRID_STRIDE(k, B) {
        double fk, rk;
        p1_marshak(sigma, gb[k], delta[k], Tb[k], emis ? emis[k] : 1.0, fk, rk);
        f[k] = fk; ref[k] = rk;
    }
}

extern "C" int ffm_p1_marshak_coeffs_d(ffm_mesh *m, double sigma, const double *gamma_b, const double *T_b, const double *emissivity_b,
                                       double *valueFraction_b, double *refValue_b)
{
    if (!m) return FFM_ERR_ARG;
    if (m->B == 0) return FFM_OK;
    if (!gamma_b || !T_b || !valueFraction_b || !refValue_b) return FFM_ERR_ARG;
    LAUNCH(k_p1_marshak, m->B, m->B, sigma, gamma_b, m->bDelta, T_b, emissivity_b, valueFraction_b, refValue_b);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

// ------------------------------------------------------------------ the system of P1::calculate() in one pass ---
// What the per-operator chain
//   ffm_p1_gamma_d (cells, patches) | ffm_fvc_interpolate | ffm_fvm_transport (laplacian alone, sign +1) | ffm_p1_marshak_coeffs_d |
//   ffm_fvm_boundary_coeffs | diag -= V a | source = 0 + V su | ffm_fvm_add_boundary
// leaves in upper / diag / source, every term rounded as there, from one walk over the rows (the structure of k_ray_assemble,
// ffm_rad.hip): a row forms gamma of itself and of its neighbours in registers -- a lower face's gamma_f from the same operands in the
// same order as its owner's row forms it, so both get the same bits -- the owner writes the face coefficient, and the cell's boundary
// faces are folded in with the Marshak coefficients formed in place (each boundary face has one cell: it is written once).
// (the launch bound is the block size of LAUNCH_CELLS: without it the 32-slot rows spill 476 bytes per lane under the default cap of 128 registers)
template <int W>
__global__ __launch_bounds__(256) void k_p1_assemble(MeshView q, double s3, double sigma, const double *__restrict__ a, double aConst, const double *__restrict__ ab,
                              const double *__restrict__ ee, double eConst, const double *__restrict__ E, const double *__restrict__ T,
                              const double *__restrict__ Tb, const double *__restrict__ emis, const double *__restrict__ bMag,
                              const double *__restrict__ bDelta, double *__restrict__ upper, double *__restrict__ diag,
                              double *__restrict__ source, double *__restrict__ gammaB, double *__restrict__ fB, double *__restrict__ refB)
{
    CELL_SCHED(ci, q) {
        const int c = (int)ci;
        RowEnt<W> L, U; load_lower<W>(q.v, c, L); load_upper<W>(q.v, c, U);
        const double ac = a ? a[c] : aConst, gP = p1_gamma(ac, s3);
        double dLap = 0.0;
        // faces where c is the neighbour: the owner's gamma is the P of the interpolate
#pragma unroll
        for (int s = 0; s < W; s++) if (L.on[s]) {
            const int e = L.f[s];
            const double w = q.w[e], gO = a ? p1_gamma(a[L.nb[s]], s3) : gP;
            const double gf = w * gO + (1.0 - w) * gP;
            dLap -= gf * q.magSf[e] * q.delta[e];
        }
        // faces owned by c: write the coefficient
#pragma unroll
        for (int s = 0; s < W; s++) if (U.on[s]) {
            const int e = U.f[s];
            const double w = q.w[e], gN = a ? p1_gamma(a[U.nb[s]], s3) : gP;
            const double gf = w * gP + (1.0 - w) * gN;
            const double g = gf * q.magSf[e] * q.delta[e];
            dLap -= g;
            upper[e] = g;
        }
        const double Vc = q.V[c], t = T[c];
        double d = dLap - Vc * ac;
        const double su = E ? (-(4.0 * (((ee ? ee[c] : eConst) * sigma) * p1_pow4(t)))) - E[c] : -(4.0 * (((ee ? ee[c] : eConst) * sigma) * p1_pow4(t)));
        double sr = 0.0 + Vc * su;
        const int jb = q.cellB[c];
        if (jb >= 0) for (int it = q.bcStart[jb]; it < q.bcStart[jb + 1]; it++) {
            const int k = q.bcItem[it];
            const double gb = p1_gamma(ab ? ab[k] : aConst, s3), dk = bDelta[k], gk = 0.0;
            double fk, rk;
            p1_marshak(sigma, gb, dk, Tb[k], emis ? emis[k] : 1.0, fk, rk);
            gammaB[k] = gb; fB[k] = fk; refB[k] = rk;
            const double pG = gb * bMag[k];
            d += pG * (-fk * dk);                                            // internalCoeffs
            sr += -pG * (fk * dk * rk + (1.0 - fk) * gk);                    // boundaryCoeffs
        }
        diag[c] = d; source[c] = sr;
    }
}

extern "C" int ffm_p1_assemble_d(ffm_mesh *m, double sigmaEff, double sigma, const double *a_d, double aConst, const double *a_b, const double *e_d,
                                 double eConst, const double *E_d, const double *T_d, const double *T_b, const double *emissivity_b,
                                 double *upper, double *diag, double *source, double *gamma_b, double *valueFraction_b, double *refValue_b)
{
    if (!m || !T_d || !upper || !diag || !source || (m->B && (!T_b || !gamma_b || !valueFraction_b || !refValue_b))) return FFM_ERR_ARG;
    m->A->directPending = false;        // (as in ffm_fvm_transport: the off-diagonal array is being rewritten)
    FFM_DISPATCH_W(m->A->maxW, LAUNCH_CELLS(k_p1_assemble<W>, mview(m), 3.0 * sigmaEff, sigma, a_d, aConst, a_b, e_d, eConst, E_d, T_d, T_b, emissivity_b,
                                            m->bMagSf, m->bDelta, upper, diag, source, gamma_b, valueFraction_b, refValue_b));
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

// The mixed evaluate of the solved G on the patches and P1.C:251-257, qr_b = -gamma_b*G_b.snGrad(): ffm_bc_values (refGrad 0) +
// ffm_fvc_snGrad_b + one multiply, bit for bit
__global__ void k_p1_wall_flux(int B, const int *__restrict__ fc, const double *__restrict__ delta, const double *__restrict__ gb,
                               const double *__restrict__ f, const double *__restrict__ ref, const double *__restrict__ G,
                               double *__restrict__ Gb, double *__restrict__ qr)
{
    GRID_STRIDE(k, B) {
        const double gc = G[fc[k]], dk = delta[k], gk = 0.0;
        const double v = f[k] * ref[k] + (1.0 - f[k]) * (gc + gk / dk);
        Gb[k] = v;
        qr[k] = -gb[k] * (dk * (v - gc));
    }
}

extern "C" int ffm_p1_wall_flux_d(ffm_mesh *m, const double *gamma_b, const double *valueFraction_b, const double *refValue_b, const double *G_d,
                                  double *G_b, double *qr_b)
{
    if (!m) return FFM_ERR_ARG;
    if (m->B == 0) return FFM_OK;
    if (!gamma_b || !valueFraction_b || !refValue_b || !G_d || !G_b || !qr_b) return FFM_ERR_ARG;
    LAUNCH(k_p1_wall_flux, m->B, m->B, m->bCells, m->bDelta, gamma_b, valueFraction_b, refValue_b, G_d, G_b, qr_b);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}
