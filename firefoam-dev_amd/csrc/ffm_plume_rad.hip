// ffm_plume_rad.hip -- the radiation models of the plume case: the fvDOM stand-in (the rays' set-up), P1, radiation->correct() and the radiation setters.
#include "ffm_plume.hpp"
#include "ffm_greymean.hpp"

// ---- fvDOM stand-in: radiation->correct() of solver/YEEqn.H:80 -------------------------------------------------------
// per ray i (direction dAve_i, solid angle omega_i; fvDOM.C:55-90, radiativeIntensityRay.C:126-143):
//   fvm::div(Ji, Ii) + fvm::Sp(k*omega, Ii) == 1/pi*omega*(k*sigma*T^4),  Ji = dAve & Sf, div scheme upwind
// (radiativeIntensityRay.C:267-322), inflow faces at the ambient black-body intensity, outflow zero-gradient; then
// G = sum Ii*omega (fvDOM::updateG).  Constant k, no scattering, no coupling back into the enthalpy equation.
// RadFraction of constRadFractionEmission::ECont with radScaling (reference lib/thermophysicalModels/radiation/submodels/
// absorptionEmissionModel/constRadFractionEmission/constRadFractionEmission.C): both patch lists name the burner
// (cases/steckler/constant/radiationProperties:44-52) -> mlr1 = mlr2 = -gSum(phi_burner)
int plume_rad_fraction(ffm_plume *P, double *out)
{
    const double *kind = P->kind_d, *pb = P->phib; double *t = P->wB[0];
    forN(P, P->B, [=] __device__(long k) { t[k] = kind[k] < 0.5 ? pb[k] : 0.0; });
    double sum = 0.0;
    FFM_TRY(ffm_reduce_sum(P->ctx, t, P->B, &sum));          // gSum: every rank takes part, also one without boundary faces
    const double mlr = -sum, e1 = P->Ehrr1, e2 = P->Ehrr2;
    *out = std::max(std::min(e1, e2), (mlr * e1 + mlr * e2) / std::max(1e-15, mlr + mlr));
    return FFM_OK;
}
// the system of ray i, one operator per launch: Ji and the upwind weights, the boundary flux and value fractions, the transport
// matrix, its boundary coefficients, the absorption and the source, addBoundaryDiag / addBoundarySource
// -> P->upper, P->lower, P->dWork, P->sWork
static int ray_assemble_ops(ffm_plume *P, int i, const double *Ee)
{
    ffm_mesh *m = P->mesh; const int N = P->N, B = P->B; const long nNat = P->nNat;
    const double *V = ffm_mesh_geom(m, 0);
    const double *sx = ffm_mesh_geom(m, 9), *sy = ffm_mesh_geom(m, 10), *sz = ffm_mesh_geom(m, 11);
    const double *bx = ffm_mesh_geom(m, 6), *by = ffm_mesh_geom(m, 7), *bz = ffm_mesh_geom(m, 8);
    double *J = P->radJ, *w = P->radW, *Jb = P->radJb, *f = P->radF, *ref = P->radRef, *su = P->radSrc;
    const double *T = P->T; const double KA = P->radA;
    const double *aF = P->gm ? P->aRad : nullptr;                 // greyMeanAbsorptionEmission: a[c]*omega and a[c]*sigma per cell
    const double d0 = P->rayD[3 * i], d1 = P->rayD[3 * i + 1], d2 = P->rayD[3 * i + 2], omega = P->rayOmega[i];
    forN(P, nNat, [=] __device__(long e) { const double j = (d0 * sx[e] + d1 * sy[e]) + d2 * sz[e]; J[e] = j; w[e] = j >= 0 ? 1.0 : 0.0; });
    forN(P, B, [=] __device__(long k) { const double j = (d0 * bx[k] + d1 * by[k]) + d2 * bz[k]; Jb[k] = j; f[k] = 1.0 - (j >= 0 ? 1.0 : 0.0); });
    FFM_TRY(ffm_fvm_transport(m, 0.0, nullptr, J, w, nullptr, -1, P->diag, P->upper, P->lower));
    FFM_TRY(ffm_fvm_boundary_coeffs(m, Jb, nullptr, -1, f, ref, P->zeroB, P->ic[0], P->bc[0]));
    double *dg = P->diag; const double kO = KA * omega, cS = 1.0 / M_PI * omega, kS = KA * SIGMA_SB;
    forN(P, N, [=] __device__(long c) {
        const double kOc = aF ? aF[c] * omega : kO, kSc = aF ? aF[c] * SIGMA_SB : kS;
        dg[c] = dg[c] + V[c] * kOc;
        const double t = T[c];
        // 1/pi*omega*(k sigma T^4 [+ E/4]) (radiativeIntensityRay.C:286-300)
        su[c] = Ee ? V[c] * (cS * (kSc * ((t * t) * (t * t)) + Ee[c] / 4.0)) : V[c] * (cS * (kSc * ((t * t) * (t * t))));
    });
    return ffm_fvm_add_boundary(m, P->ic[0], P->bc[0], P->diag, su, nullptr, P->dWork, P->sWork);
}
// the system of ray i in one pass (ffm_fvdom_ray_assemble_v_d with greyMean's a of the cells, else ffm_fvdom_ray_assemble_d) or by
// the operator chain above: the same bytes
static int ray_assemble(ffm_plume *P, int i, const double *Ee, bool onePass)
{
    if (!onePass) return ray_assemble_ops(P, i, Ee);
    if (P->gm) return ffm_fvdom_ray_assemble_v_d(P->mesh, &P->rayD[3 * i], P->rayOmega[i], P->aRad, SIGMA_SB, P->T, Ee, P->radRef, nullptr, nullptr, P->upper,
                                                 P->lower, P->dWork, P->sWork);
    return ffm_fvdom_ray_assemble_d(P->mesh, &P->rayD[3 * i], P->rayOmega[i], P->radA, SIGMA_SB, P->T, Ee, P->radRef, nullptr, nullptr, P->upper, P->lower,
                                    P->dWork, P->sWork);
}

// fvDOM::updateG over the cells (ghost cells included: every rank holds its neighbours' rays there) in one pass
static int rad_update_G(ffm_plume *P)
{
    return ffm_fvdom_G_d(P->ctx, P->N, (int)P->rayOmega.size(), P->radIdd, P->radOmegaD, P->G);
}

// the axis whose direction component has the minority sign; none (-1) when all three agree (the cell order is then already
// an upwind or a downwind order of the ray and DILU is exact)
static int ray_flip_axis(const ffm_plume *P, int i)
{
    const double d0 = P->rayD[3 * i], d1 = P->rayD[3 * i + 1], d2 = P->rayD[3 * i + 2];
    const int neg = (d0 < 0) + (d1 < 0) + (d2 < 0);
    if (neg == 1) return d0 < 0 ? 0 : d1 < 0 ? 1 : 2;
    if (neg == 2) return d0 >= 0 ? 0 : d1 >= 0 ? 1 : 2;
    return -1;
}

// The solve of a ray's system in dWork, sWork, upper, lower: as it stands (flip < 0), or with the first n cells renamed by the flip of
// that axis -- same sparsity, triangular -- gathered into radDB/SB/PsiB/UB/LB, solved, and the solution scattered back into Ii.
// solve(diag, upper, lower, psi, source) is the caller's.
template <class Solve> static int solve_ray(ffm_plume *P, int flip, int n, double *Ii, Solve solve)
{
    if (flip < 0) return solve(P->dWork, P->upper, P->lower, Ii, P->sWork);
    const int *cm = P->radCm[flip], *fm = P->radFm[flip];
    const double *dW = P->dWork, *sW = P->sWork, *up = P->upper, *lo = P->lower;
    double *dB = P->radDB, *sB = P->radSB, *pB = P->radPsiB, *uB = P->radUB, *lB = P->radLB;
    forN(P, n, [=] __device__(long c) { const int s = cm[c]; dB[c] = dW[s]; sB[c] = sW[s]; pB[c] = Ii[s]; });
    forN(P, P->nNat, [=] __device__(long e) {
        const int q = fm[e];
        if (q >= 0) { uB[e] = up[q]; lB[e] = lo[q]; } else { uB[e] = lo[~q]; lB[e] = up[~q]; }
    });
    FFM_TRY(solve(dB, uB, lB, pB, sB));
    forN(P, n, [=] __device__(long c) { Ii[cm[c]] = pB[c]; });
    return FFM_OK;
}

// The staged sweep of the rays over the blocks of a decomposed box (ffm_plume_set_radiation_ordering 1).  The ticks come from
// ffm_ray_schedule and are the same in number on every rank.  In a tick a rank solves at most one ray: its upstream neighbours
// solved that ray in earlier ticks and their values sit in the ghost cells, so the ghost inflow moves into the source and what
// is left is the one-block system -- triangular after the axis-flip renaming, solved exactly by one DILU application on this
// rank's rows, nothing inside reaching another rank.  Every tick then ends with ONE ghost exchange that all ranks enter, a rank
// without a ray too: it carries the ray each rank solved in the tick into the neighbours' ghost cells of that ray.  No rank ever
// waits for another outside that exchange.
static int radiation_correct_staged(ffm_plume *P, const double *Ee)
{
    ffm_mesh *m = P->mesh; const int nOwn = P->nOwn;
    const int nTicks = (int)P->radTick.size();
    const bool timing = getenv("FFM_TIMING") != nullptr;          // wall time of the ticks' exchanges (ghost exchange + the copies into the rays' ghost layers)
    double tExch = 0.0;
    for (int t = 0; t < nTicks; t++) {
        const int i = P->radTick[t];
        if (i >= 0) {
            FFM_TRY(ffm_fvdom_ray_assemble_d(m, &P->rayD[3 * i], P->rayOmega[i], P->radA, SIGMA_SB, P->T, Ee, P->radRef, nullptr, nullptr,
                                             P->upper, P->lower, P->dWork, P->sWork));
            FFM_TRY(ffm_fvdom_fold_ghost_inflow_d(m, P->nRadHaloCells, P->radHaloCells, P->I[i], P->upper, P->lower, P->sWork));
            SolveLog L; memset(&L, 0, sizeof(L)); snprintf(L.name, sizeof(L.name), "I%d", i);
            FFM_TRY(solve_ray(P, ray_flip_axis(P, i), nOwn, P->I[i], [&](const double *d, const double *up, const double *lo, double *psi, const double *src) {
                FFM_TRY(ffm_ldu_bind_coeffs_native_d(P->A, d, up, lo, 0));
                return ffm_solve_triangular_rows_d(P->A, psi, src, &L.perf);
            }));
            P->log.push_back(L);
            if (!L.perf.converged) {
                ffm_set_error("plume radiation: the staged solve of ray %d left sum|residual| above 1e-10 sum|source| (normalised %g): its rows are not triangular in the renamed order", i, L.perf.finalResidual);
                return FFM_ERR_ADDR;
            }
        }
        // the tick's exchange: out goes the ray solved here (a rank without one sends a field nobody reads), in come the rays
        // the face neighbours solved, each into the ghost layer of its own ray
        double tx0 = 0.0;
        if (timing) { PL_HIP(hipStreamSynchronize(P->ctx->stream)); tx0 = FfmStageTimer::now(); }
        FFM_TRY(ffm_ghost_exchange_split(P->A, i >= 0 ? P->I[i] : P->G, P->radGhostBuf));
        for (int s6 = 0; s6 < 6; s6++) {
            const int r = P->radNbrTick[s6][t], n = P->gOff[s6 + 1] - P->gOff[s6];
            if (r >= 0 && n > 0) dcopy(P, P->I[r] + nOwn + P->gOff[s6], P->radGhostBuf + P->gOff[s6], n);
        }
        if (timing) { PL_HIP(hipStreamSynchronize(P->ctx->stream)); tExch += FfmStageTimer::now() - tx0; }
    }
    if (timing) fprintf(stderr, "ffm timing: staged ray sweep rank %d: %d ticks, exchanges %.4f s in all (%.3f ms per tick)\n", P->ctx->rank, nTicks, tExch, nTicks ? 1e3 * tExch / nTicks : 0.0);
    // G = sum Ii omega in ray-index order from zero, as the unstaged sweep adds it: one pass over the rays
    return rad_update_G(P);
}

// greyMeanAbsorptionEmission at a radiation->correct(): a of the cells once (ffm_greymean_a_d) and E = EhrrCoeff*Qdot; the RadFraction
// reduction over the burner patch and its host read-back drop out in this mode
static int absem_correct(ffm_plume *P)
{
    FFM_TRY(ffm_greymean_a_d(P->gm, P->N, P->Y, P->p, P->T, P->aRad, P->gmFlag));
    FFM_TRY(ffm_greymean_E_d(P->gm, P->N, P->Qdot, P->radE));
    P->gmHaveA = true;
    return FFM_OK;
}
// absorptionEmission->ECont() of this radiation->correct() into radE: greyMean's, else constRadFractionEmission's RadFraction*Qdot
// (constRadFractionEmission.C, radScaling)
static int rad_emission(ffm_plume *P)
{
    if (P->gm) return absem_correct(P);
    double frac = 0.0;
    FFM_TRY(plume_rad_fraction(P, &frac));
    double *E = P->radE; const double *Qd = P->Qdot;
    forN(P, P->N, [=] __device__(long c) { E[c] = frac * Qd[c]; });
    return FFM_OK;
}

// ---- P1 in place of the rays (ffm_plume_set_radiation_p1): P1::calculate() of P1.C:213-258 -------------------------------------
// gamma = 1/(3 a + a0) (no scattering), fvm::laplacian(gamma, G) - fvm::Sp(a, G) == -4 a sigma T^4 - E with E = RadFraction*Qdot,
// MarshakRadiation with the one wall emissivity on every patch at the zero-gradient patch values of T, PCG + DIC at the `G` entry's
// controls (cases/steckler/system/fvSolution:75-81) from the previous G, then qr.  The fused step: ffm_p1_assemble_d and
// ffm_p1_wall_flux_d; the per-operator step: the chain of entry points they restate, the same bytes.
static int p1_correct(ffm_plume *P)
{
    ffm_mesh *m = P->mesh; const int N = P->N;
    const double *E = P->radE;
    const double *aF = nullptr, *aB = nullptr;                    // greyMeanAbsorptionEmission: a = e as a cell field, its patch values the adjacent cells'
    FFM_TRY(rad_emission(P));
    if (P->gm) { aF = P->aRad; aB = P->aRadB; zg(P, P->aRadB, P->aRad); }
    zg(P, P->p1Tb, P->T);
    const double a = P->radA;
    if (P->fused) {
        FFM_TRY(ffm_p1_assemble_d(m, 0.0, SIGMA_SB, aF, a, aB, aF, a, E, P->T, P->p1Tb, P->p1EmisB, P->upper, P->dWork, P->sWork,
                                  P->p1GammaB, P->p1F, P->p1Ref));
    } else {
        FFM_TRY(ffm_p1_gamma_d(P->ctx, N, aF, a, 0.0, P->p1GammaC));
        FFM_TRY(ffm_p1_gamma_d(P->ctx, P->B, aB, a, 0.0, P->p1GammaB));
        FFM_TRY(ffm_fvc_interpolate(m, nullptr, P->p1GammaC, P->p1GammaF));
        FFM_TRY(ffm_fvm_transport(m, 0.0, nullptr, nullptr, nullptr, P->p1GammaF, +1, P->diag, P->upper, nullptr));
        FFM_TRY(ffm_p1_marshak_coeffs_d(m, SIGMA_SB, P->p1GammaB, P->p1Tb, P->p1EmisB, P->p1F, P->p1Ref));
        FFM_TRY(ffm_fvm_boundary_coeffs(m, nullptr, P->p1GammaB, +1, P->p1F, P->p1Ref, P->zeroB, P->ic[0], P->bc[0]));
        const double *V = ffm_mesh_geom(m, 0), *T = P->T; double *dg = P->diag, *su = P->p1Su;
        forN(P, N, [=] __device__(long c) {
            const double ac = aF ? aF[c] : a;
            dg[c] = dg[c] - V[c] * ac;
            const double t = T[c];
            su[c] = 0.0 + V[c] * ((-(4.0 * ((ac * SIGMA_SB) * ((t * t) * (t * t))))) - E[c]);
        });
        FFM_TRY(ffm_fvm_add_boundary(m, P->ic[0], P->bc[0], P->diag, su, nullptr, P->dWork, P->sWork));
    }
    FFM_TRY(solve_named(P, "G", FFM_PCG, FFM_DIC, 1e-6, 0.0, P->dWork, P->upper, nullptr, P->p1G, P->sWork));
    if (P->fused) FFM_TRY(ffm_p1_wall_flux_d(m, P->p1GammaB, P->p1F, P->p1Ref, P->p1G, P->p1Gb, P->p1Qr));
    else {
        FFM_TRY(ffm_bc_values(m, P->p1F, P->p1Ref, P->zeroB, P->p1G, P->p1Gb));
        FFM_TRY(ffm_fvc_snGrad_b(m, P->p1G, P->p1Gb, P->p1Sn));
        const double *gb = P->p1GammaB, *sn = P->p1Sn; double *qr = P->p1Qr;
        forN(P, P->B, [=] __device__(long k) { qr[k] = -gb[k] * sn[k]; });
    }
    P->radHaveG = true; P->p1HaveQr = true;
    return FFM_OK;
}

extern "C" int ffm_plume_set_radiation_p1(ffm_plume *P, int solverFreq, double absorption, double Ehrr1, double Ehrr2, double wallEmissivity)
{
    if (!P || solverFreq < 0 || !(absorption >= 0) || !(Ehrr1 >= 0) || !(Ehrr2 >= 0) || !(wallEmissivity >= 0 && wallEmissivity <= 1)) return FFM_ERR_ARG;
    if (solverFreq == 0) {          // off: the step of a handle that never saw P1
        if (P->p1Freq > 0) { P->p1Freq = 0; P->radCoupled = false; P->radHaveG = false; P->radHaveSh = false; P->p1HaveQr = false; }
        return FFM_OK;
    }
    if (!P->oneBlock) { ffm_set_error("ffm_plume_set_radiation_p1: a block of a decomposed box (P1 runs on a single block only)"); return FFM_ERR_UNSUPPORTED; }
    if (P->radFreq > 0) { ffm_set_error("ffm_plume_set_radiation_p1: the fvDOM rays are on (ffm_plume_set_radiation); one radiation model at a time"); return FFM_ERR_UNSUPPORTED; }
    if (P->thermo && !P->radThermo) { ffm_set_error("ffm_plume_set_radiation_p1: not with ffm_plume_set_thermo on (ffm_plume_set_radiation_thermo is off)"); return FFM_ERR_UNSUPPORTED; }
    PL_HIP(hipSetDevice(P->ctx->device));
    if (!P->p1G) {
        const size_t nPool = P->pool.size(); const int N = P->N, B = P->B;
        P->p1G = dalloc(P, N); P->p1GammaB = dalloc(P, B); P->p1F = dalloc(P, B); P->p1Ref = dalloc(P, B); P->p1Gb = dalloc(P, B); P->p1Qr = dalloc(P, B);
        P->p1Tb = dalloc(P, B); P->p1EmisB = dalloc(P, B);
        if (!P->fused) { P->p1GammaC = dalloc(P, N); P->p1GammaF = dalloc(P, P->nNat); P->p1Su = dalloc(P, N); P->p1Sn = dalloc(P, B); }
        if (P->pool.size() != nPool + (P->fused ? 8 : 12)) { ffm_set_error("plume: out of device memory"); return FFM_ERR_HIP; }
    }
    if (!P->radE) { P->radE = dalloc(P, P->N); P->radShSu = dalloc(P, P->N); P->radShSp = dalloc(P, P->N); }
    if (!P->radE || !P->radShSu || !P->radShSp) return FFM_ERR_HIP;
    double *eb = P->p1EmisB; const double eps = wallEmissivity;
    forN(P, P->B, [=] __device__(long k) { eb[k] = eps; });
    P->radA = absorption; P->Ehrr1 = Ehrr1; P->Ehrr2 = Ehrr2; P->radCoupled = true;
    P->p1Freq = solverFreq;
    return FFM_OK;
}

int radiation_correct(ffm_plume *P)
{
    if (P->p1Freq > 0) return p1_correct(P);
    const int N = P->N;
    // the fused step on one block: every ray assembled in one pass, G formed once after the last ray.  The per-operator step, and
    // the block-Jacobi solves of a decomposed box, keep the operator chain and add each ray to G as it is solved -- the same bytes
    const bool onePass = P->fused && P->oneBlock;
    double *G = P->G;
    if (!onePass && !P->radStaged) forN(P, N, [=] __device__(long c) { G[c] = 0.0; });
    const double *Ee = nullptr;
    if (P->gm || P->radCoupled) { FFM_TRY(rad_emission(P)); Ee = P->radE; }
    if (P->radStaged) { FFM_TRY(radiation_correct_staged(P, Ee)); P->radHaveG = true; return FFM_OK; }
    const int nRay = (int)P->rayOmega.size();
    for (int i = 0; i < nRay; i++) {
        FFM_TRY(ray_assemble(P, i, Ee, onePass));
        char nm[16]; snprintf(nm, sizeof(nm), "I%d", i);
        FFM_TRY(solve_ray(P, P->radOrdered ? ray_flip_axis(P, i) : -1, N, P->I[i], [&](const double *d, const double *up, const double *lo, double *psi, const double *src) {
            return solve_named(P, nm, FFM_PBICGSTAB, FFM_DILU, 1e-4, 0.0, d, up, lo, psi, src, false, true);
        }));
        FFM_TRY(HX(P, P->I[i]));
        const double *Ii = P->I[i]; const double omega = P->rayOmega[i];
        if (!onePass) forN(P, N, [=] __device__(long c) { G[c] = G[c] + Ii[c] * omega; });
    }
    if (onePass) FFM_TRY(rad_update_G(P));
    P->radHaveG = true;
    return FFM_OK;
}

// Tests: the system of ray `ray` as the solver would take it in the state the case is in, assembled by the chain of operators
// (fused == 0) or by the one-pass kernel ffm_fvdom_ray_assemble_d (fused != 0).  diag, source [owned cells] in natural cell
// order, upper, lower [faces] in the case's face order; the two forms are to agree bit for bit.
extern "C" int ffm_plume_ray_system(ffm_plume *P, int ray, int fused, double *diag, double *upper, double *lower, double *source)
{
    if (!P || !diag || !upper || !lower || !source || !P->G || ray < 0 || ray >= (int)P->rayOmega.size()) return FFM_ERR_ARG;
    PL_HIP(hipSetDevice(P->ctx->device));
    const double *Ee = P->radCoupled ? P->radE : nullptr;
    if (P->gm && !P->gmHaveA) { ffm_set_error("ffm_plume_ray_system: greyMeanAbsorptionEmission is on and has not been evaluated yet (step first)"); return FFM_ERR_ARG; }
    FFM_TRY(ray_assemble(P, ray, Ee, fused != 0));
    std::vector<double> c(P->N), fu(std::max<long>(P->nNat, 1)), fl(std::max<long>(P->nNat, 1));
    FFM_TRY(ffm_d2h(P->ctx, c.data(), P->dWork, sizeof(double) * P->N));
    for (int k = 0; k < P->nOwn; k++) diag[P->newToOld[k]] = c[k];
    FFM_TRY(ffm_d2h(P->ctx, c.data(), P->sWork, sizeof(double) * P->N));
    for (int k = 0; k < P->nOwn; k++) source[P->newToOld[k]] = c[k];
    FFM_TRY(ffm_d2h(P->ctx, fu.data(), P->upper, sizeof(double) * P->nNat));
    FFM_TRY(ffm_d2h(P->ctx, fl.data(), P->lower, sizeof(double) * P->nNat));
    const std::vector<int> &c2n = P->A->h_callerToNative;
    for (int f = 0; f < P->F; f++) { upper[f] = fu[c2n[f]]; lower[f] = fl[c2n[f]]; }
    return FFM_OK;
}

// The direction-ordered ray solves need the axis-flip maps of the block (struct ffm_plume: radCm / radFm): built once the rays
// exist, on a single block (where every ray is then one exact DILU application) and, for the staged sweep, on a block of a
// decomposed box.  There the maps rename the owned cells only: ghost cells and cut faces keep their place -- the staged sweep has
// moved the cut faces' terms into the source and zeroed their coefficients before it renames anything.
// the block's renumbered LDU addressing on the host (hL2, hU2, hOldToNew), made again from the block's shape and the kept
// renumbering: a decomposed block does not hold these after creation, only the staged ray sweep wants them
static void plume_host_addressing(ffm_plume *P)
{
    if (!P->hL2.empty()) return;
    const int nx = P->nx, ny = P->ny, nz = P->nz, nOwn = P->nOwn, N = P->N, F = P->F; const int *gOff = P->gOff;
    auto cellOf = [&](int i, int j, int k) { return i + nx * (j + ny * k); };
    auto ghostOf = [&](int side, int i, int j, int k) -> int {
        switch (side >> 1) {
        case 0: return nOwn + gOff[side] + j + ny * k;
        case 1: return nOwn + gOff[side] + i + nx * k;
        default: return nOwn + gOff[side] + i + nx * j;
        }
    };
    std::vector<int> l, u; l.reserve(F); u.reserve(F);           // natural order, as ffm_plume_create_block builds it
    for (int k = 0; k < nz; k++) for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) {
        const int c = cellOf(i, j, k);
        if (i < nx - 1) { l.push_back(c); u.push_back(c + 1); }
        if (j < ny - 1) { l.push_back(c); u.push_back(c + nx); }
        if (k < nz - 1) { l.push_back(c); u.push_back(c + nx * ny); }
        const int at[6] = {i == 0, i == nx - 1, j == 0, j == ny - 1, k == 0, k == nz - 1};
        for (int s6 = 0; s6 < 6; s6++) if (at[s6] && P->nbrRank[s6] >= 0) { l.push_back(c); u.push_back(ghostOf(s6, i, j, k)); }
    }
    P->hOldToNew.assign(N, 0);
    for (int c = 0; c < N; c++) P->hOldToNew[P->newToOld[c]] = c;
    P->hL2.resize(F); P->hU2.resize(F);
    for (int f = 0; f < F; f++) { P->hL2[f] = P->hOldToNew[l[P->faceNewToOld[f]]]; P->hU2[f] = P->hOldToNew[u[P->faceNewToOld[f]]]; }
}

static int rad_prepare(ffm_plume *P)
{
    if (!P->G) return FFM_OK;                                   // no rays yet: ffm_plume_set_radiation comes back here
    const bool single = P->oneBlock;
    if (!single && P->radOrdering == 1 && (!P->radMaps || !P->radGhostBuf)) {
        plume_host_addressing(P);
        if ((int)P->hL2.size() != P->F) { ffm_set_error("plume radiation: the block's addressing could not be rebuilt"); return FFM_ERR_ADDR; }
    }
    if (!P->radMaps && (single || P->radOrdering == 1)) {
        const int N = P->N, nOwn = P->nOwn, F = P->F, nx = P->nx, ny = P->ny, nz = P->nz; const long nNat = P->nNat;
        std::vector<int> ownerStart(N + 1, 0);
        for (int f = 0; f < F; f++) ownerStart[P->hL2[f] + 1]++;
        for (int c = 0; c < N; c++) ownerStart[c + 1] += ownerStart[c];            // faces are sorted by owner (upper-triangular order)
        const std::vector<int> &c2n = P->A->h_callerToNative;
        for (int a = 0; a < 3; a++) {
            std::vector<int> cm(N), fm(std::max<long>(nNat, 1));
            for (long e = 0; e < nNat; e++) fm[e] = (int)e;                        // padding entries and cut faces map to themselves
            for (int c = 0; c < N; c++) {
                const int o = P->newToOld[c];
                if (o >= nOwn) { cm[c] = c; continue; }                            // ghost cell
                int i = o % nx, j = (o / nx) % ny, k = o / (nx * ny);
                if (a == 0) i = nx - 1 - i; else if (a == 1) j = ny - 1 - j; else k = nz - 1 - k;
                cm[c] = P->hOldToNew[i + nx * (j + ny * k)];
            }
            for (int f = 0; f < F; f++) {
                if (P->hU2[f] >= nOwn) continue;                                   // cut face
                int o = cm[P->hL2[f]], n = cm[P->hU2[f]]; bool swap = false;
                if (o > n) { std::swap(o, n); swap = true; }
                int fp = -1;
                for (int g = ownerStart[o]; g < ownerStart[o + 1]; g++) if (P->hU2[g] == n) { fp = g; break; }
                if (fp < 0) { ffm_set_error("plume radiation: the flipped image of a face is not a face"); return FFM_ERR_ADDR; }
                fm[c2n[f]] = swap ? ~c2n[fp] : c2n[fp];
            }
            PL_HIP(hipMalloc((void **)&P->radCm[a], sizeof(int) * N)); PL_HIP(hipMalloc((void **)&P->radFm[a], sizeof(int) * std::max<long>(nNat, 1)));
            FFM_TRY(ffm_h2d(P->ctx, P->radCm[a], cm.data(), sizeof(int) * N));
            FFM_TRY(ffm_h2d(P->ctx, P->radFm[a], fm.data(), sizeof(int) * std::max<long>(nNat, 1)));
        }
        P->radDB = dalloc(P, N); P->radSB = dalloc(P, N); P->radPsiB = dalloc(P, N); P->radUB = dalloc(P, nNat); P->radLB = dalloc(P, nNat);
        if (!P->radDB || !P->radSB || !P->radPsiB || !P->radUB || !P->radLB) return FFM_ERR_HIP;
        P->radMaps = true;
        P->radOrdered = single;
    }
    if (!single && P->radOrdering == 1) {
        if (!P->radGhostBuf) {
            // the owned cells with a cut face, and the ghost layers where the exchange puts them: side after side behind the owned cells
            std::vector<int> halo;
            for (int f = 0; f < P->F; f++) if (P->hU2[f] >= P->nOwn && (halo.empty() || halo.back() != P->hL2[f])) halo.push_back(P->hL2[f]);
            for (int g = P->nOwn; g < P->N; g++) if (P->newToOld[g] != g) { ffm_set_error("plume radiation: ghost cells are not in exchange order"); return FFM_ERR_ADDR; }
            P->nRadHaloCells = (int)halo.size();
            FFM_TRY(ffm_upload_vec(P->ctx, &P->radHaloCells, halo));
            P->radGhostBuf = dalloc(P, P->N - P->nOwn);
            if (!P->radGhostBuf) return FFM_ERR_HIP;
        }
        // the ticks of this rank and of its face neighbours (a neighbour's ray of a tick is what its message of that tick carries)
        const int nRay = (int)P->rayOmega.size(); const int *g = P->blkGrid, *b = P->blkAt;
        const int nTicks = ffm_ray_schedule(g[0], g[1], g[2], b[0], b[1], b[2], nRay, P->rayD.data(), nullptr, 0);
        if (nTicks < 0) return nTicks;
        P->radTick.assign(nTicks, -1);
        FFM_TRY(std::min(0, ffm_ray_schedule(g[0], g[1], g[2], b[0], b[1], b[2], nRay, P->rayD.data(), P->radTick.data(), nTicks)));
        for (int s6 = 0; s6 < 6; s6++) {
            P->radNbrTick[s6].assign(nTicks, -1);
            if (P->nbrRank[s6] < 0) continue;
            int nb[3] = {b[0], b[1], b[2]}; nb[s6 >> 1] += (s6 & 1) ? 1 : -1;
            const int nT = ffm_ray_schedule(g[0], g[1], g[2], nb[0], nb[1], nb[2], nRay, P->rayD.data(), P->radNbrTick[s6].data(), nTicks);
            if (nT != nTicks) { ffm_set_error("plume radiation: tick counts differ between blocks"); return FFM_ERR_ARG; }
        }
        P->radStaged = true;
        std::vector<int>().swap(P->hL2); std::vector<int>().swap(P->hU2); std::vector<int>().swap(P->hOldToNew);      // maps and lists are on the device now
    }
    return FFM_OK;
}

// Switch the fvDOM stand-in on: every `solverFreq` steps (cases/steckler/constant/radiationProperties:32-40: solverFreq 100,
// nPhi 2, nTheta 4 -> 32 rays) the step solves one upwind transport equation per ray before the enthalpy equation.
// dAve[3*nRay] / omega[nRay] may be given by the caller (the shim passes fvDOM's own); null -> built here from nPhi, nTheta.
extern "C" int ffm_plume_set_radiation(ffm_plume *P, int solverFreq, int nPhi, int nTheta, const double *dAve, const double *omega)
{
    if (!P || solverFreq < 0 || nPhi < 1 || nTheta < 1 || ((dAve == nullptr) != (omega == nullptr))) return FFM_ERR_ARG;
    if (P->thermo && !P->radThermo) { ffm_set_error("ffm_plume_set_radiation: not with ffm_plume_set_thermo on (ffm_plume_set_radiation_thermo is off)"); return FFM_ERR_UNSUPPORTED; }
    if (P->p1Freq > 0) { ffm_set_error("ffm_plume_set_radiation: the P1 model is on (ffm_plume_set_radiation_p1); one radiation model at a time"); return FFM_ERR_UNSUPPORTED; }
    PL_HIP(hipSetDevice(P->ctx->device));
    const int nRay = 4 * nPhi * nTheta;
    P->rayD.assign(3 * (size_t)nRay, 0.0); P->rayOmega.assign(nRay, 0.0);
    if (dAve) { std::copy(dAve, dAve + 3 * nRay, P->rayD.begin()); std::copy(omega, omega + nRay, P->rayOmega.begin()); }
    else {
        const double dPhi = M_PI / (2.0 * nPhi), dTheta = M_PI / nTheta; int i = 0;
        for (int n = 1; n <= nTheta; n++) for (int mm = 1; mm <= 4 * nPhi; mm++, i++) {
            const double theta = (2.0 * n - 1.0) * dTheta / 2.0, phi = (2.0 * mm - 1.0) * dPhi / 2.0;
            const double a = sin(0.5 * dPhi) * (dTheta - cos(2.0 * theta) * sin(dTheta));
            P->rayOmega[i] = 2.0 * sin(theta) * sin(dTheta / 2.0) * dPhi;
            P->rayD[3 * i] = sin(phi) * a; P->rayD[3 * i + 1] = cos(phi) * a; P->rayD[3 * i + 2] = 0.5 * dPhi * sin(2.0 * theta) * sin(dTheta);
        }
    }
    if ((int)P->I.size() < nRay) {
        for (int i = (int)P->I.size(); i < nRay; i++) { double *p = dalloc(P, P->N); if (!p) return FFM_ERR_HIP; P->I.push_back(p); }
    }
    if (!P->G) {
        P->G = dalloc(P, P->N); P->radSrc = dalloc(P, P->N); P->radJ = dalloc(P, P->nNat); P->radW = dalloc(P, P->nNat);
        // black inflow at the ambient temperature: the rays' refValue, written here and nowhere else
        P->radJb = dalloc(P, P->B); P->radF = dalloc(P, P->B); P->radRef = dfill(P, P->B, SIGMA_SB * ((TREF * TREF) * (TREF * TREF)) / M_PI);
        if (!P->G || !P->radSrc || !P->radJ || !P->radW || !P->radJb || !P->radF || !P->radRef) return FFM_ERR_HIP;
    }
    // the rays' pointers and solid angles for ffm_fvdom_G_d
    static_assert(sizeof(double *) == sizeof(double), "the pointer table is taken from the pool of doubles");
    if (P->radTabRays < nRay) {
        P->radIdd = (double **)dalloc(P, nRay); P->radOmegaD = dalloc(P, nRay);
        if (!P->radIdd || !P->radOmegaD) return FFM_ERR_HIP;
        P->radTabRays = nRay;
    }
    FFM_TRY(ffm_h2d(P->ctx, P->radIdd, P->I.data(), sizeof(double *) * nRay));
    FFM_TRY(ffm_h2d(P->ctx, P->radOmegaD, P->rayOmega.data(), sizeof(double) * nRay));
    FFM_TRY(rad_prepare(P));
    P->radFreq = solverFreq;
    return FFM_OK;
}

// How the rays of a decomposed block are solved (see include/ffm.h): 0 every ray a block-Jacobi PBiCGStab solve over all ranks,
// 1 the staged, direction-ordered sweep.  The place of the block in the block grid is read off the neighbour ranks: ranks number
// the blocks x fastest (rank = bx + px (by + py bz)), so the rank stride across a y side is px and across a z side px py.
extern "C" int ffm_plume_set_radiation_ordering(ffm_plume *P, int mode)
{
    if (!P || (mode != 0 && mode != 1)) return FFM_ERR_ARG;
    if (P->thermo && !P->radThermo) { ffm_set_error("ffm_plume_set_radiation_ordering: not with ffm_plume_set_thermo on (ffm_plume_set_radiation_thermo is off)"); return FFM_ERR_UNSUPPORTED; }
    PL_HIP(hipSetDevice(P->ctx->device));
    if (mode == 1 && !P->oneBlock) {
        const int *nb = P->nbrRank; const int rank = P->ctx->rank, world = P->ctx->nRanks;
        const int sy = nb[2] >= 0 ? rank - nb[2] : nb[3] >= 0 ? nb[3] - rank : 0, sz = nb[4] >= 0 ? rank - nb[4] : nb[5] >= 0 ? nb[5] - rank : 0;
        const int px = sy > 0 ? sy : sz > 0 ? sz : world;
        const int py = sy > 0 ? (sz > 0 ? sz / px : world / px) : 1;
        const int pz = px > 0 && py > 0 ? world / (px * py) : 0;
        bool ok = px > 0 && py > 0 && pz > 0 && px * py * pz == world && sy >= 0 && sz >= 0 && (sz == 0 || sz == px * py);
        int b[3] = {0, 0, 0};
        if (ok) {
            b[0] = rank % px; b[1] = (rank / px) % py; b[2] = rank / (px * py);
            const int g[3] = {px, py, pz}, stride[3] = {1, px, px * py};
            for (int s6 = 0; s6 < 6 && ok; s6++) {
                const int d = s6 >> 1, at = b[d] + ((s6 & 1) ? 1 : -1);
                ok = nb[s6] == ((at < 0 || at >= g[d]) ? -1 : rank + ((s6 & 1) ? stride[d] : -stride[d]));
            }
        }
        if (!ok) {
            ffm_set_error("plume radiation ordering 1: the neighbour ranks are not those of a box of blocks numbered x fastest (rank %d of %d)", rank, world);
            return FFM_ERR_UNSUPPORTED;
        }
        P->blkGrid[0] = px; P->blkGrid[1] = py; P->blkGrid[2] = pz;
        for (int d = 0; d < 3; d++) P->blkAt[d] = b[d];
    }
    P->radOrdering = mode;
    P->radStaged = false;
    return rad_prepare(P);
}

// the reference's absorption / emission model + radiation->Sh coupling (see include/ffm.h)
extern "C" int ffm_plume_set_radiation_model(ffm_plume *P, double absorption, double Ehrr1, double Ehrr2)
{
    if (!P || absorption < 0 || Ehrr1 < 0 || Ehrr2 < 0) return FFM_ERR_ARG;
    if (P->thermo && !P->radThermo) { ffm_set_error("ffm_plume_set_radiation_model: not with ffm_plume_set_thermo on (ffm_plume_set_radiation_thermo is off)"); return FFM_ERR_UNSUPPORTED; }
    if (P->p1Freq > 0) { ffm_set_error("ffm_plume_set_radiation_model: the P1 model is on and has its own constants (ffm_plume_set_radiation_p1)"); return FFM_ERR_UNSUPPORTED; }
    PL_HIP(hipSetDevice(P->ctx->device));
    if (!P->radE) { P->radE = dalloc(P, P->N); P->radShSu = dalloc(P, P->N); P->radShSp = dalloc(P, P->N); }
    if (!P->radE || !P->radShSu || !P->radShSp) return FFM_ERR_HIP;
    P->radA = absorption; P->Ehrr1 = Ehrr1; P->Ehrr2 = Ehrr2; P->radCoupled = true;
    return FFM_OK;
}

// greyMeanAbsorptionEmission in place of the constant absorption coefficient and of constRadFractionEmission's E (see include/ffm.h).
// The handle is borrowed, as ffm_plume_set_thermo's is; NULL: the constant again, the step of a handle that never had the model.
extern "C" int ffm_plume_set_absorption_emission(ffm_plume *P, ffm_greymean *gm)
{
    if (!P) return FFM_ERR_ARG;
    if (!gm) { P->gm = nullptr; P->gmHaveA = false; return FFM_OK; }
    if (!P->oneBlock) { ffm_set_error("ffm_plume_set_absorption_emission: a block of a decomposed box (the model runs on a single block only)"); return FFM_ERR_UNSUPPORTED; }
    if (!((P->radFreq > 0 || P->p1Freq > 0) && P->radCoupled)) {
        ffm_set_error("ffm_plume_set_absorption_emission: needs ffm_plume_set_radiation with ffm_plume_set_radiation_model, or ffm_plume_set_radiation_p1, first");
        return FFM_ERR_UNSUPPORTED;
    }
    // the model's species are the plume's, with the molecular weights of the selected thermo package (the stand-in's WMOL)
    double W[NSP]; int nS = NSP;
    if (P->thermo) FFM_TRY(ffm_thermo_species(P->thermo, &nS, nullptr));
    if (P->thermo && nS == NSP) FFM_TRY(ffm_thermo_species(P->thermo, &nS, W)); else for (int i = 0; i < NSP; i++) W[i] = WMOL[i];
    bool same = gm->t.n == NSP && nS == NSP;
    for (int i = 0; same && i < NSP; i++) same = gm->t.W[i] == W[i];
    if (!same) { ffm_set_error("ffm_plume_set_absorption_emission: the model's species or molecular weights are not the %s", P->thermo ? "thermo package's" : "plume's"); return FFM_ERR_ARG; }
    PL_HIP(hipSetDevice(P->ctx->device));
    if (!P->aRad) {
        P->aRad = dalloc(P, P->N); P->aRadB = dalloc(P, P->B);
        if (!P->aRad || !P->aRadB) return FFM_ERR_HIP;
        PL_HIP(hipMalloc((void **)&P->gmFlag, sizeof(int)));
        PL_HIP(hipMemsetAsync(P->gmFlag, 0, sizeof(int), P->ctx->stream));
        PL_HIP(hipHostMalloc((void **)&P->gmFlagH, sizeof(int), hipHostMallocDefault));
        *P->gmFlagH = 0;
    }
    P->gm = gm; P->gmHaveA = false;
    return FFM_OK;
}
