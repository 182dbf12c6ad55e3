// ffm_plume_step.hip -- one fireFoam time step of the plume case (solver/fireFoam.C:76-121 with PIMPLE 1/2/0, cases/steckler/system/
// fvSolution:84-89) against the C ABI of include/ffm.h: ffm_plume_step at the end of the file is the reference's sequence, one stage per snippet
//   rhoEqn  solver/rhoEqn.H:33-43      UEqn  solver/UEqn.H:3-33      YEEqn   solver/YEEqn.H:37-118      pEqn  solver/pEqn.H:1-60 (x2)
//   turbulence->correct()  solver/fireFoam.C:113-116: k_eqn, only with the LES kEqn model selected (ffm_plume_set_turbulence; oracle:
//   tests/plume_keqn_ref.py); without it the step is the stand-in's constant mu and mu/Pr and launches nothing more than before
//   thermo.correct(), mu, alpha: the janaf / sutherland package, and combustion->correct(): the reference's EDC, where selected
//   (ffm_plume_set_thermo, ffm_plume_set_combustion; oracle: tests/plume_thermo_ref.py); with nothing selected, the stand-ins' launches
// bench.py's workload and the subject of tests/test_plume_gpu.py (oracle: oracle/plume.py, same sequence in numpy).  A stage whose assembly has
// a fused pass (ffm_fused.hip) reads P->fused once; its per-operator form, one launch per fvc:: / fvm:: operator (FFM_PLUME_UNFUSED, bitwise
// equal), is the function <stage>_ops next to it, and what both forms run is in the stage.  Scratch slots: the table in ffm_plume.hpp.
#include "ffm_plume.hpp"

// dynamic part of the mixed BCs: inletOutlet / pressureInletOutletVelocity value fraction f = 1 - pos0(phi_b)
static void bc_update_f(ffm_plume *P, double *f, const double *fStatic)
{ const double *pb = P->phib; forN(P, P->B, [=] __device__(long k) { f[k] = fStatic[k] < 0 ? 1.0 - (pb[k] >= 0 ? 1.0 : 0.0) : fStatic[k]; }); }

static int update_bcs(ffm_plume *P)
{
    for (int c = 0; c < 3; c++) bc_update_f(P, P->fU[c], P->fStaticU[c]);
    bc_update_f(P, P->fS, P->fStaticS);
    bc_update_f(P, P->fH, P->fStaticH);
    return FFM_OK;
}

// ---- boundary values of U from its mixed BC (per component) -> P->Ub -----------------------------------
static int U_boundary(ffm_plume *P)
{
    for (int c = 0; c < 3; c++) FFM_TRY(ffm_bc_values(P->mesh, P->fU[c], P->refU[c], P->zeroB, P->U[c], P->Ub[c]));
    return FFM_OK;
}

// p_rgh BC: fixedFluxPressure gradient on inlet/floor, prghTotalHydrostaticPressure value on top/sides (reads P->Ub)
static int bc_p_rgh(ffm_plume *P, const double *grad /*[B] or null*/, const double *rhob)
{
    const double *kind = P->kind_d, *pb = P->phib, *phb = P->ph_rgh_b;
    const double *u0 = P->Ub[0], *u1 = P->Ub[1], *u2 = P->Ub[2];
    double *f = P->fP, *ref = P->refP, *g = P->gradP;
    forN(P, P->B, [=] __device__(long k) {
        if (kind[k] < 1.5) { f[k] = 0.0; ref[k] = 0.0; g[k] = grad ? grad[k] : 0.0; }
        else {
            f[k] = 1.0; g[k] = 0.0;
            ref[k] = phb[k] - 0.5 * rhob[k] * (1.0 - (pb[k] >= 0 ? 1.0 : 0.0)) * ((u0[k] * u0[k] + u1[k] * u1[k]) + u2[k] * u2[k]);
        }
    });
    return FFM_OK;
}

// oldTime fields.  rho, K and psi are rewritten in full before their first read (rho by rhoEqn next, K after the momentum solve,
// psi by the thermo update after EEqn): the old-time field takes the buffer, no copy.  Every kernel gets its pointers from P at
// launch.  phi's old-time value is read where phi still holds it (ddtCorr, first corrector), and nothing reads the inert specie's.
static void store_old_time(ffm_plume *P)
{
    const int N = P->N;
    std::swap(P->rho0, P->rho); std::swap(P->K0, P->K); std::swap(P->psi0, P->psi);
    dcopy(P, P->hs0, P->hs, N); dcopy(P, P->p0, P->p, N); dcopy(P, P->p_rgh0, P->p_rgh, N);
    for (int c = 0; c < 3; c++) dcopy(P, P->U0[c], P->U[c], N);
    for (int i = 0; i < NSP; i++) if (i != INERT) dcopy(P, P->Y0[i], P->Y[i], N);
}

static int rho_eqn_ops(ffm_plume *P)
{
    double *div = P->wN[0];
    FFM_TRY(ffm_fvc_surface_integrate(P->mesh, P->phi, P->phib, div));
    const double *V = ffm_mesh_geom(P->mesh, 0), *rho0 = P->rho0; double *rho = P->rho; const double rdt = P->rdt;
    forN(P, P->nOwn, [=] __device__(long i) { rho[i] = (rdt * rho0[i] * V[i] - V[i] * div[i]) / (rdt * V[i]); });
    return FFM_OK;
}
// fvm::ddt(rho) + fvc::div(phi) == 0  -> diagonal: rho = (rdt*rho0*V - V*div(phi))/(rdt*V).  The one-pass kernel refuses only rows
// wider than 16 entries; the rows of a hex block have at most 6 (three faces towards owned cells and one cut face per coupled side
// that a corner cell touches: ffm_ldu_analysis.cpp counts both into maxW), so no FFM_ERR_UNSUPPORTED comes back from it here.
static int rho_eqn(ffm_plume *P)
{
    FFM_TRY(P->fused ? ffm_fvc_rho_eqn(P->mesh, P->rdt, P->phi, P->phib, P->rho0, P->rho) : rho_eqn_ops(P));
    return HX(P, P->rho);
}

// ---------------- UEqn.H
// rec = reconstruct((-ghf*snGrad(rho) - snGrad(p_rgh))*magSf); the per-operator form's three launches stand between the patch kernels.
// The fused form stops at the patch part tb: u_eqn forms the face flux, reconstructs it and adds it to the sources in one cell pass
// (ffm_ue_buoyancy_source3), after u_sources
static int u_buoyancy(ffm_plume *P, double *const rec[3])
{
    ffm_mesh *m = P->mesh; const bool ops = !P->fused;
    double *sgr = P->wF[1], *sgp = P->wF[2], *t = P->wF[4], *tb = P->wB[5], *rhob = P->wB[6], *pb = P->wB[7];
    const double *ghf = P->ghf, *magSf = ffm_mesh_geom(m, 1), *bMag = ffm_mesh_geom(m, 4);
    if (ops) FFM_TRY(ffm_fvc_snGrad(m, P->rho, sgr));
    zg(P, rhob, P->rho);
    FFM_TRY(bc_p_rgh(P, nullptr, rhob));
    FFM_TRY(ffm_bc_values(m, P->fP, P->refP, P->gradP, P->p_rgh, pb));
    if (ops) FFM_TRY(ffm_fvc_snGrad(m, P->p_rgh, sgp));
    FFM_TRY(ffm_fvc_snGrad_b(m, P->p_rgh, pb, tb));
    if (ops) forN(P, P->nNat, [=] __device__(long e) { t[e] = (-ghf[e] * sgr[e] - sgp[e]) * magSf[e]; });
    forN(P, P->B, [=] __device__(long k) { tb[k] = -tb[k] * bMag[k]; });
    return ops ? ffm_fvc_reconstruct(m, t, tb, rec[0], rec[1], rec[2]) : FFM_OK;
}

// ddt + the explicit LUST correction of component c, one operator per launch: gaussConvectionScheme::fvmDiv with a corrected() scheme,
// fvm += fvc::surfaceIntegrate(phi*LUST::correction(U_c))
static int u_source_ops(ffm_plume *P, int c)
{
    ffm_mesh *m = P->mesh; const double rdt = P->rdt; const double *V = ffm_mesh_geom(m, 0);
    // (with the kEqn model the three gradients live on for the stress divergence: u_stress_divergence)
    double *gx = P->turbModel ? P->lesG[c][0] : P->wN[1], *gy = P->turbModel ? P->lesG[c][1] : P->wN[2], *gz = P->turbModel ? P->lesG[c][2] : P->wN[3];
    double *corr = P->wF[4], *divc = P->wN[4];
    FFM_TRY(ffm_fvc_grad(m, P->U[c], P->Ub[c], gx, gy, gz));
    FFM_TRY(HX(P, gx)); FFM_TRY(HX(P, gy)); FFM_TRY(HX(P, gz));
    FFM_TRY(ffm_fv_lust_correction(m, P->phi, gx, gy, gz, corr));
    { const double *phi = P->phi; forN(P, P->nNat, [=] __device__(long e) { corr[e] = phi[e] * corr[e]; }); }
    FFM_TRY(ffm_fvc_surface_integrate(m, corr, P->zeroB, divc));
    double *s = P->Usrc[c]; const double *rho0 = P->rho0, *u0 = P->U0[c];
    forN(P, P->N, [=] __device__(long i) { s[i] = rdt * rho0[i] * u0[i] * V[i] - V[i] * divc[i]; });
    return FFM_OK;
}
// the patch coefficients of the three components and their sources; the per-operator form finishes a component before the next
static int u_sources(ffm_plume *P, const double *mub)
{
    ffm_mesh *m = P->mesh; const bool ops = !P->fused;
    for (int c = 0; c < 3; c++) {
        FFM_TRY(ffm_fvm_boundary_coeffs(m, P->phib, mub, -1, P->fU[c], P->refU[c], P->zeroB, P->Uic[c], P->Ubc[c]));
        if (ops) FFM_TRY(u_source_ops(P, c));
    }
    if (ops) return FFM_OK;
    const double *uf[3] = {P->U[0], P->U[1], P->U[2]}, *ub[3] = {P->Ub[0], P->Ub[1], P->Ub[2]}, *u0[3] = {P->U0[0], P->U0[1], P->U0[2]};
    // Single block, no sub-grid model (whose stress divergence and kEqn want the gradients): every face's phi*correction by its upwind cell
    // on the tile walk, then one row pass for the sums and the ddt source -- no gradient arrays (ffm_fused.hip: k_mv_tile<MVT_LUST>,
    // k_lust_sum; bit for bit the two passes below, which take over where ffm_tile_fv_segments refuses the box)
    if (P->oneBlock && !P->turbModel) {
        double *qf[3] = {P->wF[1], P->wF[2], P->wF[4]};
        const int rc = ffm_fv_lust_phi_correction3_tiled(m, P->phi, uf, ub, qf);
        if (rc == FFM_OK) return ffm_fvm_lust_source3_sum(m, P->rdt, P->rho0, u0, qf, P->Usrc);
        if (rc != FFM_ERR_UNSUPPORTED) return rc;
    }
    // one gradient pass for the three components, one pass for the LUST correction + the ddt source (ffm_fused.hip)
    double *ggx[3] = {P->gM[0][0], P->gM[1][0], P->gM[2][0]}, *ggy[3] = {P->gM[0][1], P->gM[1][1], P->gM[2][1]}, *ggz[3] = {P->gM[0][2], P->gM[1][2], P->gM[2][2]};
    FFM_TRY(ffm_fvc_grad_multi(m, 3, uf, ub, ggx, ggy, ggz));
    for (int c = 0; c < 3; c++) { FFM_TRY(HX(P, ggx[c])); FFM_TRY(HX(P, ggy[c])); FFM_TRY(HX(P, ggz[c])); }
    return ffm_fvm_lust_source3(m, P->rdt, P->phi, P->rho0, u0, ggx, ggy, ggz, P->Usrc);
}

// A fused assembly pass on a single block writes the sweeps' coefficient layout beside the native one (the *_direct entry points:
// the solve that binds the arrays next gathers nothing); where the matrix's tile plan cannot take it, the plain form and the gather
// (asked of the matrix first: a block that would be refused is not put to the call, and no refusal text is left behind a good step)
#define DIRECT_OR(P, direct, plain) \
    do { int rc_ = ((P)->oneBlock && ffm_tile_coef_direct_ok((P)->A)) ? (direct) : FFM_ERR_UNSUPPORTED; \
         if (rc_ == FFM_ERR_UNSUPPORTED) rc_ = (plain); FFM_TRY(rc_); } while (0)

// ---------------- the kEqn model's parts of UEqn.H and YEEqn.H (ffm_plume_set_turbulence; oracle: tests/plume_keqn_ref.py) ----------
// the nine cell gradients g[3*i + j] = d_i U_j where the form in use keeps them: gM[c] (fused), lesG[c] (per-operator)
static void les_gradU(ffm_plume *P, const double *g9[9])
{ for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) g9[3 * i + j] = P->fused ? P->gM[j][i] : P->lesG[j][i]; }

// rho*nuEff = rho*(nut + mu/rho) with the present rho: linear interpolation -> gf, patch values -> gb (rho_b: the zero-gradient copy).
// The fused form is one owner-row pass from rho and nut (ffm_les_face_diffusivity); the per-operator form goes through the cell field,
// which the fused form writes only where a later pass wants it (wantCell: the stress divergence of u_eqn)
static int les_rho_nuEff_faces(ffm_plume *P, double *gamCell, bool wantCell, double *rhob, double *gf, double *gb)
{
    ffm_mesh *m = P->mesh;
    const double *rho = P->rho, *nut = P->nut, *nutb = P->nutb;
    zg(P, rhob, rho);
    if (P->thermo) {                // mu: thermo.correct()'s cell field, zero-gradient on the patches (ffm_les_face_diffusivity_v)
        const double *mu = P->mu; const int *fc = ffm_mesh_bcells(m);
        if (!P->fused || wantCell) forN(P, P->N, [=] __device__(long i) { gamCell[i] = rho[i] * (nut[i] + mu[i] / rho[i]); });
        if (P->fused) return ffm_les_face_diffusivity_v(m, 0, mu, rho, rhob, nut, nutb, gf, gb);
        FFM_TRY(ffm_fvc_interpolate(m, nullptr, gamCell, gf));
        forN(P, P->B, [=] __device__(long k) { gb[k] = rhob[k] * (nutb[k] + mu[fc[k]] / rhob[k]); });
        return FFM_OK;
    }
    if (!P->fused || wantCell) forN(P, P->N, [=] __device__(long i) { gamCell[i] = rho[i] * (nut[i] + MU / rho[i]); });
    if (P->fused) return ffm_les_face_diffusivity(m, 0, MU, rho, rhob, nut, nutb, gf, gb);
    FFM_TRY(ffm_fvc_interpolate(m, nullptr, gamCell, gf));
    forN(P, P->B, [=] __device__(long k) { gb[k] = rhob[k] * (nutb[k] + MU / rhob[k]); });
    return FFM_OK;
}

// turbulence->divDevRhoReff(U), explicit part (solver/UEqn.H:7): Usrc_c += V*fvc::div(rho nuEff dev2(T(grad U)))_c from the gradients
// u_sources formed for LUST and U's patch values; the same two launches in both forms
static int u_stress_divergence(ffm_plume *P, const double *gam, const double *gamb)
{
    const double *g9[9]; les_gradU(P, g9);
    const double *U[3] = {P->U[0], P->U[1], P->U[2]}, *Ub[3] = {P->Ub[0], P->Ub[1], P->Ub[2]};
    double *dv[3] = {P->wN[9], P->wN[10], P->wN[11]};
    FFM_TRY(ffm_fvc_div_dev2T_gradU(P->mesh, g9, gam, gamb, U, Ub, dv));
    const double *V = ffm_mesh_geom(P->mesh, 0), *d0 = dv[0], *d1 = dv[1], *d2 = dv[2]; double *s0 = P->Usrc[0], *s1 = P->Usrc[1], *s2 = P->Usrc[2];
    forN(P, P->nOwn, [=] __device__(long i) { s0[i] = s0[i] + V[i] * d0[i]; s1[i] = s1[i] + V[i] * d1[i]; s2[i] = s2[i] + V[i] * d2[i]; });
    return FFM_OK;
}

// a laminar diffusivity of the janaf thermo on the faces: interpolate(c), zero-gradient patch values (c = mu: UEqn; c = alpha: YEEqn)
static int thermo_laminar_faces(ffm_plume *P, const double *c, double *cf, double *cb)
{
    if (P->fused) return ffm_les_face_diffusivity_v(P->mesh, 1, c, nullptr, nullptr, nullptr, nullptr, cf, cb);
    FFM_TRY(ffm_fvc_interpolate(P->mesh, nullptr, c, cf));
    zg(P, cb, c);
    return FFM_OK;
}

// turbulence->alphaEff() (solver/YEEqn.H:12): alpha + alphat with the alphat of the last correctNut(), one diffusivity for species and h
static int les_alpha_eff(ffm_plume *P)
{
    ffm_mesh *m = P->mesh;
    double *af = P->alphaEff_f, *afb = P->alphaEff_b, *a = P->wN[11]; const double *alphat = P->alphat, *alphatb = P->alphatb;
    if (P->thermo) {                // alpha: thermo.correct()'s cell field, zero-gradient on the patches
        const double *alpha = P->alpha; const int *fc = ffm_mesh_bcells(m);
        if (P->fused) return ffm_les_face_diffusivity_v(m, 1, alpha, nullptr, nullptr, alphat, alphatb, af, afb);
        forN(P, P->N, [=] __device__(long i) { a[i] = alpha[i] + alphat[i]; });
        FFM_TRY(ffm_fvc_interpolate(m, nullptr, a, af));
        forN(P, P->B, [=] __device__(long k) { afb[k] = alpha[fc[k]] + alphatb[k]; });
        return FFM_OK;
    }
    if (P->fused) return ffm_les_face_diffusivity(m, 1, MU / PR, nullptr, nullptr, alphat, alphatb, af, afb);
    forN(P, P->N, [=] __device__(long i) { a[i] = MU / PR + alphat[i]; });
    FFM_TRY(ffm_fvc_interpolate(m, nullptr, a, af));
    forN(P, P->B, [=] __device__(long k) { afb[k] = MU / PR + alphatb[k]; });
    return FFM_OK;
}

static int u_eqn(ffm_plume *P)
{
    ffm_mesh *m = P->mesh; const int N = P->N; const bool ops = !P->fused;
    double *wU = P->wF[3], *muf = P->wF[0], *mub = P->wB[4], *rec[3] = {P->wN[5], P->wN[6], P->wN[7]};
    FFM_TRY(update_bcs(P));
    FFM_TRY(U_boundary(P));
    // div(phi,U) Gauss LUST grad(U) (cases/steckler/system/fvSchemes:32): LUST weights for the implicit part -- a function of phi and the
    // mesh weights alone, formed inside the assembly pass by the fused form; the explicit correction goes into the source (u_sources)
    if (ops) FFM_TRY(ffm_fv_limited_weights(m, 4, 1.0, 0.0, 1.0, P->phi, nullptr, nullptr, nullptr, nullptr, wU));
    double *gam = P->wN[8];         // kEqn: rho*nuEff on the cells, for the stress divergence (wB[6] is u_buoyancy's rhob next)
    if (P->turbModel) FFM_TRY(les_rho_nuEff_faces(P, gam, true, P->wB[6], muf, mub));
    else if (P->thermo) FFM_TRY(thermo_laminar_faces(P, P->mu, muf, mub));
    else {
        forN(P, P->nNat, [=] __device__(long e) { muf[e] = MU; });
        forN(P, P->B, [=] __device__(long k) { mub[k] = MU; });
    }
    if (ops) FFM_TRY(ffm_fvm_transport(m, P->rdt, P->rho, P->phi, wU, muf, -1, P->Udiag, P->Uupper, P->Ulower));
    else DIRECT_OR(P, ffm_fvm_transport_scheme_direct(m, P->rdt, P->rho, P->phi, 4, muf, -1, P->Udiag, P->Uupper, P->Ulower),
                   ffm_fvm_transport_scheme(m, P->rdt, P->rho, P->phi, 4, muf, -1, P->Udiag, P->Uupper, P->Ulower));
    FFM_TRY(u_buoyancy(P, rec));
    FFM_TRY(u_sources(P, mub));
    if (P->turbModel) FFM_TRY(u_stress_divergence(P, gam, mub));
    // fvMatrix::solveSegregated: the three components share the face coefficients -- one lock-step solve (ffm_solve_multi_d).
    // UdW = Udiag + sum ic, UsW = Usrc + sum bc + V*rec; Usrc, Uic and Ubc stay as they are for the correctors.  The fused form: one
    // cell pass from rho, p_rgh and u_buoyancy's patch part, no face flux and no rec (a hex block's rows have at most 6 entries, see
    // rho_eqn: no FFM_ERR_UNSUPPORTED from it here)
    const char *nm[3] = {"Ux", "Uy", "Uz"};
    if (ops) { for (int c = 0; c < 3; c++) FFM_TRY(ffm_fvm_add_boundary(m, P->Uic[c], P->Ubc[c], P->Udiag, P->Usrc[c], rec[c], P->UdW[c], P->UsW[c])); }
    else FFM_TRY(ffm_ue_buoyancy_source3(m, P->ghf, P->rho, P->p_rgh, P->wB[5], P->Uic, P->Ubc, P->Udiag, P->Usrc, P->UdW, P->UsW));
    FFM_TRY(solve_named_multi(P, 3, nm, 1e-6, P->UdW, P->Uupper, P->Ulower, P->U, P->UsW));
    for (int c = 0; c < 3; c++) FFM_TRY(HX(P, P->U[c]));
    double *K = P->K; const double *U0 = P->U[0], *U1 = P->U[1], *U2 = P->U[2];
    forN(P, N, [=] __device__(long i) { K[i] = 0.5 * ((U0[i] * U0[i] + U1[i] * U1[i]) + U2[i] * U2[i]); });
    return FFM_OK;
}

// ---------------- YEEqn.H
// turbulence->alphaEff() without a sub-grid model and combustion->correct().  The stand-ins: constant alphaEff, EDC-shaped single-step
// fuel consumption rate.  The selected models: interpolate(alpha) of the janaf thermo; the reference's eddyDissipationModel::correct
// (ffm_plume_set_combustion: ffm_edc_correct_d, one cell pass in both forms, ghosts included) with the step's deltaT, kEqn's Ce and delta
// and the thermo model's alpha
static int combustion_correct(ffm_plume *P)
{
    double *af = P->alphaEff_f, *afb = P->alphaEff_b, *wFuel = P->wFuel, *Qdot = P->Qdot, *Yt = P->Yt;
    if (!P->turbModel && P->thermo) FFM_TRY(thermo_laminar_faces(P, P->alpha, af, afb));
    else if (!P->turbModel) {       // (kEqn: les_alpha_eff, called next)
        forN(P, P->nNat, [=] __device__(long e) { af[e] = 0.5 * (MU / PR) + (1.0 - 0.5) * (MU / PR); });
        forN(P, P->B, [=] __device__(long k) { afb[k] = MU / PR; });
    }
    const double *rho = P->rho, *fuel = P->Y[2], *o2 = P->Y[0];
    // (the per-operator species loop sums Yt as it goes and wants it zero)
    if (P->combModel == 1) {
        if (!P->fused) forN(P, P->N, [=] __device__(long i) { Yt[i] = 0.0; });
        return ffm_edc_correct_d(P->ctx, P->N, rho, P->kSgs, P->lesDelta, P->thermo ? P->alpha : P->alphaStd, fuel, o2, P->edcS, P->dt, P->Ce,
                                 P->C_EDC, P->C_Diff, P->C_Stiff, P->qFuel, wFuel, Qdot);
    }
    if (P->fused) forN(P, P->N, [=] __device__(long i) { const double w = rho[i] * fmin(fuel[i], o2[i] / S_O2) / TAU; wFuel[i] = w; Qdot[i] = w * HC; });
    else forN(P, P->N, [=] __device__(long i) { const double w = rho[i] * fmin(fuel[i], o2[i] / S_O2) / TAU; wFuel[i] = w; Qdot[i] = w * HC; Yt[i] = 0.0; });
    return FFM_OK;
}

// the six fields under the common limiter and their patch values: h first, then the transported species, then the inert one
// (the minimum does not depend on the order); limitedLinear for h, limitedLinear01 for the species
struct MvFields { const double *vf[6], *vb[6]; };
static const int MV_SCHEMES[6] = {2, 3, 3, 3, 3, 3};

static int mv_weights_grad_multi(ffm_plume *P, const MvFields &f)
{
    ffm_mesh *m = P->mesh;
    const double *vf2[2] = {f.vf[0], f.vf[5]}, *vb2[2] = {f.vb[0], f.vb[5]}, *cgx[6], *cgy[6], *cgz[6];
    double *g2x[2] = {P->mvG[0][0], P->mvG[1][0]}, *g2y[2] = {P->mvG[0][1], P->mvG[1][1]}, *g2z[2] = {P->mvG[0][2], P->mvG[1][2]};
    double *ggx[4], *ggy[4], *ggz[4];
    for (int j = 0; j < 4; j++) { ggx[j] = P->gM[j][0]; ggy[j] = P->gM[j][1]; ggz[j] = P->gM[j][2]; }
    FFM_TRY(ffm_fvc_grad_multi(m, 2, vf2, vb2, g2x, g2y, g2z));
    FFM_TRY(ffm_fvc_grad_multi(m, 4, f.vf + 1, f.vb + 1, ggx, ggy, ggz));
    for (int j = 0; j < 2; j++) { FFM_TRY(HX(P, g2x[j])); FFM_TRY(HX(P, g2y[j])); FFM_TRY(HX(P, g2z[j])); }
    for (int j = 0; j < 4; j++) { FFM_TRY(HX(P, ggx[j])); FFM_TRY(HX(P, ggy[j])); FFM_TRY(HX(P, ggz[j])); }
    cgx[0] = g2x[0]; cgy[0] = g2y[0]; cgz[0] = g2z[0]; cgx[5] = g2x[1]; cgy[5] = g2y[1]; cgz[5] = g2z[1];
    for (int j = 0; j < 4; j++) { cgx[1 + j] = ggx[j]; cgy[1 + j] = ggy[j]; cgz[1 + j] = ggz[j]; }
    return ffm_fv_multivariate_weights(m, 6, MV_SCHEMES, 1.0, 0.0, 1.0, P->phi, f.vf, cgx, cgy, cgz, P->wMv);
}

static int mv_weights_ops(ffm_plume *P, const MvFields &f)
{
    ffm_mesh *m = P->mesh;
    double *gx = P->wN[1], *gy = P->wN[2], *gz = P->wN[3], *lim = P->wF[1];
    for (int j = 0; j < 6; j++) {
        FFM_TRY(ffm_fvc_grad(m, f.vf[j], f.vb[j], gx, gy, gz));
        FFM_TRY(HX(P, gx)); FFM_TRY(HX(P, gy)); FFM_TRY(HX(P, gz));
        FFM_TRY(ffm_fv_limited_limiter(m, MV_SCHEMES[j], 1.0, 0.0, 1.0, P->phi, f.vf[j], gx, gy, gz, lim, j == 0 ? 0 : 1));
    }
    return ffm_fv_weights_from_limiter(m, P->phi, lim, P->wMv);
}

// mvConvection (solver/YEEqn.H:1-10): the common limiter over the five species and h, from the fields as they are now -> P->wMv
static int mv_weights(ffm_plume *P)
{
    P->phiKValid = false;
    if (!P->mvSelection) return FFM_OK;                                  // one limiter per field: the equations evaluate their own
    if (P->mvOverride) { P->mvOverride = false; return FFM_OK; }         // weights of this step were handed in: wMv stays as uploaded
    ffm_mesh *m = P->mesh;
    // K rides on the tile pass below (fused single block): its patch values first -- U.correctBoundaryConditions() after the momentum solve;
    // nothing between here and e_K_terms writes U, phi or U's patch conditions -- into a member, Ub's slots being Nb's and hb's next
    const bool withK = P->fused && P->oneBlock && P->phiKf;
    if (withK) {
        FFM_TRY(U_boundary(P));
        double *Kb = P->KbM; const double *b0 = P->Ub[0], *b1 = P->Ub[1], *b2 = P->Ub[2];
        forN(P, P->B, [=] __device__(long k) { Kb[k] = 0.5 * ((b0[k] * b0[k] + b1[k] * b1[k]) + b2[k] * b2[k]); });
    }
    double *Nb = P->wB[1], *hb = P->wB[3];
    MvFields f = {{P->hs, nullptr, nullptr, nullptr, nullptr, P->Y[INERT]}, {hb, nullptr, nullptr, nullptr, nullptr, Nb}};
    for (int i = 0, j = 0; i < NSP; i++) if (i != INERT) {
        FFM_TRY(ffm_bc_values(m, P->fS, P->refY[i], P->zeroB, P->Y[i], P->spB[j]));
        f.vf[1 + j] = P->Y[i]; f.vb[1 + j] = P->spB[j]; j++;
    }
    {   // the inert specie's patch values: Y[inertIndex] == 1 - Yt; .max(0) on the patch faces too
        const double *b0 = P->spB[0], *b1 = P->spB[1], *b2 = P->spB[2], *b3 = P->spB[3];
        forN(P, P->B, [=] __device__(long k) { const double t = ((fmax(b0[k], 0.0) + fmax(b1[k], 0.0)) + fmax(b2[k], 0.0)) + fmax(b3[k], 0.0); Nb[k] = fmax(1.0 - t, 0.0); });
    }
    FFM_TRY(ffm_bc_values(m, P->fH, P->refH, P->zeroB, P->hs, hb));
    if (!P->fused) return mv_weights_ops(P, f);
    // gradients of the six fields + the common limiter in ONE pass with the cell values staged through LDS on the tile numbering
    // (ffm_fused.hip: k_mv_tile; bit for bit mv_weights_grad_multi, which takes over where ffm_tile_fv_segments refuses the box)
    // With K as the seventh staged field the pass also leaves phi_f*Kf of fvc::div(phi,K) per face for e_K_terms (`Gauss limitedLinear 1`)
    const int rc = withK ? ffm_fv_multivariate_weights_phiK_tiled(m, 6, MV_SCHEMES, 1.0, 0.0, 1.0, P->phi, f.vf, f.vb, P->wMv, 2, 1.0, 0.0, 1.0, P->K,
                                                                  P->KbM, P->phiKf)
                         : ffm_fv_multivariate_weights_tiled(m, 6, MV_SCHEMES, 1.0, 0.0, 1.0, P->phi, f.vf, f.vb, P->wMv);
    if (rc == FFM_OK) P->phiKValid = withK;
    return rc == FFM_ERR_UNSUPPORTED ? mv_weights_grad_multi(P, f) : rc;
}

// transport equation of a scalar, one operator per launch: ddt(rho,vf) + div(phi,vf) - laplacian(gamma,vf) == su (+ explicit LHS
// terms in `expl`); convected with the weights wGiven, or with those of its own limiter where wGiven is null
static int scalar_transport(ffm_plume *P, const char *name, int scheme, double *vf, const double *vf0, const double *fBC, const double *ref,
                            const double *gamma_f, const double *gamma_b, const double *su, const double *const *expl, double tol,
                            const double *su2, const double *sp, const double *wGiven, const double *vbStored = nullptr)
{
    ffm_mesh *m = P->mesh; const int N = P->N;
    double *vb = P->wB[2], *gx = P->wN[1], *gy = P->wN[2], *gz = P->wN[3], *wOwn = P->wF[3], *sSu = P->wN[4];
    const double *w = wGiven;
    if (!wGiven) {
        // (vbStored: the field keeps the patch values of its last evaluation -- k -- instead of evaluating its condition again)
        if (!vbStored) FFM_TRY(ffm_bc_values(m, fBC, ref, P->zeroB, vf, vb));
        FFM_TRY(ffm_fvc_grad(m, vf, vbStored ? vbStored : vb, gx, gy, gz));
        FFM_TRY(HX(P, gx)); FFM_TRY(HX(P, gy)); FFM_TRY(HX(P, gz));
        FFM_TRY(ffm_fv_limited_weights(m, scheme, 1.0, 0.0, 1.0, P->phi, vf, gx, gy, gz, wOwn));
        w = wOwn;
    }
    FFM_TRY(ffm_fvm_transport(m, P->rdt, P->rho, P->phi, w, gamma_f, -1, P->diag, P->upper, P->lower));
    FFM_TRY(ffm_fvm_boundary_coeffs(m, P->phib, gamma_b, -1, fBC, ref, P->zeroB, P->ic[0], P->bc[0]));
    // source = rdt*rho0*vf0*V (- V*expl) ; then + boundaryCoeffs + V*su
    const double *V = ffm_mesh_geom(m, 0), *rho0 = P->rho0; double *s = P->src[0]; const double rdt = P->rdt;
    // explicit volume terms on the left-hand side: one `source -= V*term` each, in the order given (fvMatrix + volField)
    if (expl) { const double *e0 = expl[0], *e1 = expl[1], *e2 = expl[2];
                forN(P, N, [=] __device__(long i) { s[i] = ((rdt * rho0[i] * vf0[i] * V[i] - V[i] * e0[i]) - V[i] * e1[i]) - V[i] * e2[i]; }); }
    else forN(P, N, [=] __device__(long i) { s[i] = rdt * rho0[i] * vf0[i] * V[i]; });
    double *s2 = sSu;
    if (su) { forN(P, N, [=] __device__(long i) { s2[i] = s[i] + V[i] * su[i]; }); }
    else s2 = s;
    if (sp) { double *dg = P->diag; forN(P, N, [=] __device__(long i) { dg[i] = dg[i] + V[i] * sp[i]; }); }      // - fvm::Sp(sp, vf) on the RHS
    if (su2) { double *s3 = P->src[1]; const double *sIn = s2; forN(P, N, [=] __device__(long i) { s3[i] = sIn[i] + V[i] * su2[i]; }); s2 = s3; }
    FFM_TRY(ffm_fvm_add_boundary(m, P->ic[0], P->bc[0], P->diag, s2, nullptr, P->dWork, P->sWork));
    FFM_TRY(solve_named(P, name, FFM_PBICGSTAB, FFM_DILU, tol, 0.0, P->dWork, P->upper, P->lower, vf, P->sWork));
    return HX(P, vf);
}

static int species_eqns_ops(ffm_plume *P)
{
    double *su = P->wN[11], *Yt = P->Yt; const double *wFuel = P->wFuel;
    for (int i = 0; i < NSP; i++) {
        if (i == INERT) continue;
        const double nu = NU[i];
        forN(P, P->N, [=] __device__(long c) { su[c] = nu * wFuel[c]; });
        // (P->wMv is null with one limiter per field)
        FFM_TRY(scalar_transport(P, SPN[i], 3, P->Y[i], P->Y0[i], P->fS, P->refY[i], P->alphaEff_f, P->alphaEff_b, su, nullptr, 1e-8, nullptr, nullptr, P->wMv));
        double *Yi = P->Y[i];
        forN(P, P->N, [=] __device__(long c) { const double v = fmax(Yi[c], 0.0); Yi[c] = v; Yt[c] += v; });
    }
    double *Yn = P->Y[INERT];
    forN(P, P->N, [=] __device__(long c) { Yn[c] = fmax(1.0 - Yt[c], 0.0); });
    return FFM_OK;
}

// (defined with e_eqn below)
struct KTerms { double *ddtK, *divK, *ndpdt; };
static int e_K_terms(ffm_plume *P, const KTerms &kt);
static int e_radiation_source(ffm_plume *P, const double **shSu, const double **shSp);

// withH (the common limiter, PBiCGStab + DILU, one block, no radiation->correct() in this step): h is the fifth field of the assembly
// pass and the fifth lane of the lock-step solve.  Nothing the enthalpy matrix reads is written by the species solves -- Qdot is
// combustion_correct's, the K terms come from U, wMv is formed before, T, hs and G are old values -- so its explicit terms are formed
// first; the solve log keeps the reference's order, every lane the numbers of a solve of its own.
static int species_eqns(ffm_plume *P, bool *offDiagBound, bool withH)
{
    *offDiagBound = false;
    if (!P->fused) return species_eqns_ops(P);
    ffm_mesh *m = P->mesh; const int N = P->N, ns = NSP - 1; const double rdt = P->rdt;
    const double *af = P->alphaEff_f, *afb = P->alphaEff_b, *wFuel = P->wFuel;
    int sp[ns];
    const double *vf0[ns], *fq[ns], *rq[ns], *gq[ns], *suq[ns]; double nuq[ns];
    for (int i = 0, j = 0; i < NSP; i++) if (i != INERT) {
        sp[j] = i; vf0[j] = P->Y0[i]; fq[j] = P->fS; rq[j] = P->refY[i]; gq[j] = P->zeroB; suq[j] = wFuel; nuq[j] = NU[i]; j++;
    }
    if (withH) {
        const KTerms kt = {P->wN[0], P->wN[4], P->wN[5]};
        FFM_TRY(e_K_terms(P, kt));
        const double *shSu, *shSp;
        FFM_TRY(e_radiation_source(P, &shSu, &shSp));
        constexpr int nq = ns + 1;
        const double *vf0q[nq], *fq5[nq], *rq5[nq], *gq5[nq], *suq5[nq], *su2q[nq], *spq[nq], *expl[3 * nq]; double fac[nq];
        double *dd[nq], *ss[nq], *uu[nq] = {P->spU[0], nullptr, nullptr, nullptr, nullptr}, *ll[nq] = {P->spL[0], nullptr, nullptr, nullptr, nullptr};
        const char *nmq[nq]; double *pq[nq];
        for (int j = 0; j < ns; j++) {
            vf0q[j] = vf0[j]; fq5[j] = fq[j]; rq5[j] = rq[j]; gq5[j] = gq[j]; suq5[j] = suq[j]; fac[j] = nuq[j]; su2q[j] = spq[j] = nullptr;
            for (int e = 0; e < 3; e++) expl[3 * j + e] = nullptr;
            dd[j] = P->spD[j]; ss[j] = P->spS[j]; nmq[j] = SPN[sp[j]]; pq[j] = P->Y[sp[j]];
        }
        vf0q[ns] = P->hs0; fq5[ns] = P->fH; rq5[ns] = P->refH; gq5[ns] = P->zeroB; suq5[ns] = P->Qdot; fac[ns] = 1.0; su2q[ns] = shSu; spq[ns] = shSp;
        expl[3 * ns] = kt.ddtK; expl[3 * ns + 1] = kt.divK; expl[3 * ns + 2] = kt.ndpdt;
        dd[ns] = P->dWork; ss[ns] = P->sWork; nmq[ns] = "h"; pq[ns] = P->hs;
        DIRECT_OR(P, ffm_fvm_scalar_transport_multi_ws_direct(m, nq, P->wMv, rdt, P->rho, P->rho0, P->phi, P->phib, af, afb, vf0q, fq5, rq5, gq5, suq5, fac,
                                                              su2q, spq, expl, dd, uu, ll, ss),
                  ffm_fvm_scalar_transport_multi_ws(m, nq, P->wMv, rdt, P->rho, P->rho0, P->phi, P->phib, af, afb, vf0q, fq5, rq5, gq5, suq5, fac, su2q,
                                                    spq, expl, dd, uu, ll, ss));
        FFM_TRY(solve_named_multi(P, nq, nmq, 1e-8, dd, P->spU[0], P->spL[0], pq, ss));
        for (int j = 0; j < nq; j++) FFM_TRY(HX(P, pq[j]));
        P->jointSteps++;
    } else if (P->mvSelection) {
        // with the common weights and one diffusivity the four species have the SAME off-diagonal coefficients (only diag and source
        // differ, through the patch conditions and the sources): written once, gathered into the sweeps' layout once; the assembly
        // pass forms nu_i*wFuel itself
        double *uShared[ns] = {P->spU[0], nullptr, nullptr, nullptr}, *lShared[ns] = {P->spL[0], nullptr, nullptr, nullptr};
        DIRECT_OR(P, ffm_fvm_scalar_transport_multi_ws_direct(m, ns, P->wMv, rdt, P->rho, P->rho0, P->phi, P->phib, af, afb, vf0, fq, rq, gq, suq, nuq,
                                                              nullptr, nullptr, nullptr, P->spD, uShared, lShared, P->spS),
                  ffm_fvm_scalar_transport_multi_ws(m, ns, P->wMv, rdt, P->rho, P->rho0, P->phi, P->phib, af, afb, vf0, fq, rq, gq, suq, nuq, nullptr,
                                                    nullptr, nullptr, P->spD, uShared, lShared, P->spS));
        const char *nmq[ns]; double *pq[ns];
        for (int j = 0; j < ns; j++) { nmq[j] = SPN[sp[j]]; pq[j] = P->Y[sp[j]]; }
        FFM_TRY(solve_named_multi(P, ns, nmq, 1e-8, P->spD, P->spU[0], P->spL[0], pq, P->spS));
        for (int j = 0; j < ns; j++) FFM_TRY(HX(P, P->Y[sp[j]]));
        *offDiagBound = true;           // spU[0], spL[0] are now the matrix' bound (and gathered) off-diagonals
    } else {
        // one limiter per field: the source is the product field nu_i*wFuel, as before; each species has its own matrix
        const double *vf[ns], *vb[ns], *cgx[ns], *cgy[ns], *cgz[ns]; double *ggx[ns], *ggy[ns], *ggz[ns];
        for (int j = 0; j < ns; j++) {
            const int i = sp[j]; const double nu = nuq[j]; double *sm = P->suM[j];
            forN(P, N, [=] __device__(long c) { sm[c] = nu * wFuel[c]; });
            FFM_TRY(ffm_bc_values(m, P->fS, P->refY[i], P->zeroB, P->Y[i], P->spB[j]));
            vf[j] = P->Y[i]; vb[j] = P->spB[j]; suq[j] = sm;
            ggx[j] = P->gM[j][0]; ggy[j] = P->gM[j][1]; ggz[j] = P->gM[j][2]; cgx[j] = ggx[j]; cgy[j] = ggy[j]; cgz[j] = ggz[j];
        }
        FFM_TRY(ffm_fvc_grad_multi(m, ns, vf, vb, ggx, ggy, ggz));
        for (int j = 0; j < ns; j++) { FFM_TRY(HX(P, ggx[j])); FFM_TRY(HX(P, ggy[j])); FFM_TRY(HX(P, ggz[j])); }
        FFM_TRY(ffm_fvm_scalar_transport_multi(m, ns, 3, 1.0, 0.0, 1.0, rdt, P->rho, P->rho0, P->phi, P->phib, af, afb, vf, cgx, cgy, cgz, vf0,
                                               fq, rq, gq, suq, nullptr, nullptr, nullptr, P->spD, P->spU, P->spL, P->spS));
        for (int j = 0; j < ns; j++) {
            FFM_TRY(solve_named(P, SPN[sp[j]], FFM_PBICGSTAB, FFM_DILU, 1e-8, 0.0, P->spD[j], P->spU[j], P->spL[j], P->Y[sp[j]], P->spS[j]));
            FFM_TRY(HX(P, P->Y[sp[j]]));
        }
    }
    // Yi.max(0), Yt = sum Yi in the species' order starting from zero, Y[inertIndex] = max(1 - Yt, 0): one pass (solver/YEEqn.H:60-66)
    double *y0 = P->Y[sp[0]], *y1 = P->Y[sp[1]], *y2 = P->Y[sp[2]], *y3 = P->Y[sp[3]], *Yn = P->Y[INERT];
    forN(P, N, [=] __device__(long c) {
        const double a = fmax(y0[c], 0.0), b = fmax(y1[c], 0.0), d = fmax(y2[c], 0.0), e = fmax(y3[c], 0.0);
        y0[c] = a; y1[c] = b; y2[c] = d; y3[c] = e;
        const double t = (((0.0 + a) + b) + d) + e;
        Yn[c] = fmax(1.0 - t, 0.0);
    });
    return FFM_OK;
}

// ---- EEqn: the explicit LHS terms fvc::ddt(rho,K) + fvc::div(phi,K) - dpdt (solver/YEEqn.H:89-101)
static int e_K_terms_ops(ffm_plume *P, const double *Kb, const double *kgx, const double *kgy, const double *kgz, const KTerms &kt)
{
    ffm_mesh *m = P->mesh; const double rdt = P->rdt;
    double *wK = P->wF[3], *Kf = P->wF[4], *KfB = P->wB[5];
    FFM_TRY(ffm_fv_limited_weights(m, 2, 1.0, 0.0, 1.0, P->phi, P->K, kgx, kgy, kgz, wK));
    FFM_TRY(ffm_fvc_interpolate(m, wK, P->K, Kf));
    const double *phi = P->phi, *phib = P->phib;
    forN(P, P->nNat, [=] __device__(long e) { Kf[e] = phi[e] * Kf[e]; });
    forN(P, P->B, [=] __device__(long k) { KfB[k] = phib[k] * Kb[k]; });
    FFM_TRY(ffm_fvc_surface_integrate(m, Kf, KfB, kt.divK));
    const double *rho = P->rho, *rho0 = P->rho0, *K = P->K, *K0 = P->K0, *dpdt = P->dpdt; double *ddtK = kt.ddtK, *ndpdt = kt.ndpdt;
    forN(P, P->N, [=] __device__(long c) { ddtK[c] = rdt * (rho[c] * K[c] - rho0[c] * K0[c]); ndpdt[c] = -dpdt[c]; });
    return FFM_OK;
}
// The fused form: limitedLinear weights, interpolate(K), *phi, surfaceIntegrate and the two cell terms in one cell-centred pass,
// no wK, no Kf.  ffm_fvc_div_phiK_terms refuses only rows wider than 8 entries; a hex block's have at most 6 (see rho_eqn).
static int e_K_terms(ffm_plume *P, const KTerms &kt)
{
    ffm_mesh *m = P->mesh;
    // this step's mv_weights left phi_f*Kf on the faces (k_mv_tile<MVT_WK>): one row pass sums them -- no grad(K), no limiter here
    if (P->phiKValid)
        return ffm_fvc_div_phiK_sum(m, P->rdt, P->phiKf, P->phib, P->K, P->KbM, P->rho, P->rho0, P->K0, P->dpdt, kt.divK, kt.ddtK, kt.ndpdt);
    double *Kb = P->wB[0], *kgx = P->wN[1], *kgy = P->wN[2], *kgz = P->wN[3];
    FFM_TRY(U_boundary(P));     // U.correctBoundaryConditions() after the momentum solve
    const double *b0 = P->Ub[0], *b1 = P->Ub[1], *b2 = P->Ub[2];
    forN(P, P->B, [=] __device__(long k) { Kb[k] = 0.5 * ((b0[k] * b0[k] + b1[k] * b1[k]) + b2[k] * b2[k]); });
    FFM_TRY(ffm_fvc_grad(m, P->K, Kb, kgx, kgy, kgz));
    FFM_TRY(HX(P, kgx)); FFM_TRY(HX(P, kgy)); FFM_TRY(HX(P, kgz));
    return P->fused ? ffm_fvc_div_phiK_terms(m, 2, 1.0, 0.0, 1.0, P->rdt, P->phi, P->phib, P->K, Kb, kgx, kgy, kgz, P->rho, P->rho0, P->K0, P->dpdt,
                                             kt.divK, kt.ddtK, kt.ndpdt)
                    : e_K_terms_ops(P, Kb, kgx, kgy, kgz, kt);
}

// + radiation->Sh(thermo, he) = Ru - fvm::Sp(4 Rp T^3/Cpv, he) - Rp T^3 (T - 4 he/Cpv), Rp = 4 a sigma, Ru = a G - E
// (radiationModel.C:229-244, fvDOM.C Rp / Ru), E of the current Qdot; both null where radiation is not coupled
static int e_radiation_source(ffm_plume *P, const double **shSu, const double **shSp)
{
    *shSu = *shSp = nullptr;
    if (!(P->radCoupled && P->radHaveG)) return FFM_OK;
    if (P->gm) {
        // greyMeanAbsorptionEmission: a follows T and Y every step (Rp() / Ru() call aCont() afresh), E = EhrrCoeff*Qdot.  Fused: one pass
        // with a in registers; per-operator: the three entry points it restates, the same bytes
        double *su = P->radShSu, *sp = P->radShSp; const double *Cpv = P->thermo ? P->Cp : nullptr;
        if (P->fused) FFM_TRY(ffm_radiation_sh_greymean_d(P->gm, P->N, P->Y, P->p, P->T, SIGMA_SB, P->radG(), P->hs, P->Qdot, Cpv, CP, P->aRad, su, sp, P->gmFlag));
        else {
            FFM_TRY(ffm_greymean_a_d(P->gm, P->N, P->Y, P->p, P->T, P->aRad, P->gmFlag));
            FFM_TRY(ffm_greymean_E_d(P->gm, P->N, P->Qdot, P->radE));
            FFM_TRY(ffm_radiation_sh_v_d(P->ctx, P->N, P->aRad, P->aRad, SIGMA_SB, P->radE, P->radG(), P->T, P->hs, Cpv, CP, su, sp));
        }
        P->gmHaveA = true; P->radHaveSh = true;
        *shSu = su; *shSp = sp;
        return FFM_OK;
    }
    double frac = 0.0;
    FFM_TRY(plume_rad_fraction(P, &frac));
    const double Rp = 4.0 * P->radA * SIGMA_SB, KA = P->radA;
    // Cpv: the thermo package's cell field (thermo.correct() of the step before wrote it at the T read here), else the stand-in's constant
    double *su2 = P->radShSu, *sp2 = P->radShSp; const double *G = P->radG(), *T = P->T, *hh = P->hs, *Qd = P->Qdot, *Cpf = P->thermo ? P->Cp : nullptr;
    if (P->fused) FFM_TRY(ffm_radiation_sh_d(P->ctx, P->N, KA, SIGMA_SB, frac, G, T, hh, Qd, Cpf, CP, su2, sp2));
    else forN(P, P->N, [=] __device__(long c) {
        const double t = T[c], T3 = t * t * t, cp = Cpf ? Cpf[c] : CP;
        const double Ru = KA * G[c] - frac * Qd[c];
        sp2[c] = 4.0 * Rp * T3 / cp;
        su2[c] = Ru - Rp * T3 * (t - 4.0 * hh[c] / cp);
    });
    P->radHaveSh = true;
    *shSu = su2; *shSp = sp2;
    return FFM_OK;
}

// The four transported species share phi, rho and dEff: boundary values, gradients and matrices of all four in one pass each, then
// the solves in the reference's order (nothing a later equation reads changes in an earlier solve)
static int e_eqn(ffm_plume *P, bool shareH)
{
    ffm_mesh *m = P->mesh; const double rdt = P->rdt;
    const KTerms kt = {P->wN[0], P->wN[4], P->wN[5]};
    FFM_TRY(e_K_terms(P, kt));
    const double *expl[3] = {kt.ddtK, kt.divK, kt.ndpdt};
    const double *shSu, *shSp;
    FFM_TRY(e_radiation_source(P, &shSu, &shSp));
    if (!P->fused) return scalar_transport(P, "h", 2, P->hs, P->hs0, P->fH, P->refH, P->alphaEff_f, P->alphaEff_b, P->Qdot, expl, 1e-8, shSu, shSp, P->wMv);
    const double *af = P->alphaEff_f, *afb = P->alphaEff_b;
    const double *vf[1] = {P->hs}, *vb[1] = {P->spB[0]}, *vf0[1] = {P->hs0}, *fq[1] = {P->fH}, *rq[1] = {P->refH}, *gq[1] = {P->zeroB}, *suq[1] = {P->Qdot};
    double *ggx[1] = {P->gM[0][0]}, *ggy[1] = {P->gM[0][1]}, *ggz[1] = {P->gM[0][2]};
    const double *cgx[1] = {ggx[0]}, *cgy[1] = {ggy[0]}, *cgz[1] = {ggz[0]}, *su2q[1] = {shSu}, *spq[1] = {shSp};
    double *dd[1] = {P->dWork}, *uu[1] = {P->upper}, *ll[1] = {P->lower}, *ss[1] = {P->sWork};
    // h is convected with the same weights and diffuses with the same alphaEff (Le = 1) as the species: where their off-diagonals
    // are still the bound ones (common limiter, no ray solve in between) the enthalpy matrix shares them as well
    if (shareH) { uu[0] = nullptr; ll[0] = nullptr; }
    if (P->mvSelection)
        FFM_TRY(ffm_fvm_scalar_transport_multi_w(m, 1, P->wMv, rdt, P->rho, P->rho0, P->phi, P->phib, af, afb, vf0, fq, rq, gq, suq, su2q, spq, expl,
                                                 dd, uu, ll, ss));
    else {
        FFM_TRY(ffm_bc_values(m, P->fH, P->refH, P->zeroB, P->hs, P->spB[0]));
        FFM_TRY(ffm_fvc_grad_multi(m, 1, vf, vb, ggx, ggy, ggz));
        FFM_TRY(HX(P, ggx[0])); FFM_TRY(HX(P, ggy[0])); FFM_TRY(HX(P, ggz[0]));
        FFM_TRY(ffm_fvm_scalar_transport_multi(m, 1, 2, 1.0, 0.0, 1.0, rdt, P->rho, P->rho0, P->phi, P->phib, af, afb, vf, cgx, cgy, cgz, vf0,
                                               fq, rq, gq, suq, su2q, spq, expl, dd, uu, ll, ss));
    }
    if (shareH) FFM_TRY(solve_named(P, "h", FFM_PBICGSTAB, FFM_DILU, 1e-8, 0.0, P->dWork, P->spU[0], P->spL[0], P->hs, P->sWork, true));
    else FFM_TRY(solve_named(P, "h", FFM_PBICGSTAB, FFM_DILU, 1e-8, 0.0, P->dWork, P->upper, P->lower, P->hs, P->sWork));
    return HX(P, P->hs);
}

// ---------------- pEqn.H: what one statement hands to the next
struct PCorr {
    double *rAU, *rhorAU, *HbyA[3], *rec[3];             // cells
    double *rhorAUf, *phig, *phiHbyA, *fl;               // faces: fl = p_rghEqn.flux()
    double *rhorAUfb, *rhob, *phiHbyAb, *flb;            // patch faces
};

static int pc_rAU_ops(ffm_plume *P, const PCorr &w)
{
    double *rho = P->rho, *rAU = w.rAU, *rhorAU = w.rhorAU;
    FFM_TRY(ffm_fvm_A(P->mesh, 3, P->Udiag, P->Uic[0], P->Uic[1], P->Uic[2], rAU));
    mul(P, rho, P->psi, P->p, P->N);                                                        // rho = thermo.rho()
    forN(P, P->nOwn, [=] __device__(long i) { rAU[i] = 1.0 / rAU[i]; });
    FFM_TRY(HX(P, rAU));
    forN(P, P->N, [=] __device__(long i) { rhorAU[i] = rho[i] * rAU[i]; });
    return FFM_OK;
}
static int pc_HbyA_ops(ffm_plume *P, const PCorr &w)
{
    const double *rAU = w.rAU;
    for (int c = 0; c < 3; c++) {
        FFM_TRY(ffm_fvm_H(P->mesh, 3, c, P->Uupper, P->Ulower, P->Usrc[c], P->Uic[0], P->Uic[1], P->Uic[2], P->Ubc[c], P->U[c], w.HbyA[c]));
        double *Hc = w.HbyA[c];
        forN(P, P->nOwn, [=] __device__(long i) { Hc[i] = rAU[i] * Hc[i]; });
        FFM_TRY(HX(P, Hc));
    }
    return FFM_OK;
}
// rho = thermo.rho(); rAU = 1/UEqn.A(); rhorAUf = interpolate(rho*rAU); HbyA = rAU*UEqn.H().  On a single block (no ghost refresh of rAU
// in between) the first three are one pass, inside that of UEqn.A().  The fused form leaves rhorAUf to pc_phiHbyA's face pass
static int pc_rAU_HbyA(ffm_plume *P, const PCorr &w)
{
    ffm_mesh *m = P->mesh; const bool ops = !P->fused;
    if (ops || !P->oneBlock) FFM_TRY(pc_rAU_ops(P, w));
    else FFM_TRY(ffm_fvm_rAU(m, 3, P->Udiag, P->Uic[0], P->Uic[1], P->Uic[2], P->psi, P->p, P->rho, w.rAU, w.rhorAU));
    if (ops) FFM_TRY(ffm_fvc_interpolate(m, nullptr, w.rhorAU, w.rhorAUf));
    zg(P, w.rhorAUfb, w.rhorAU);
    if (ops) return pc_HbyA_ops(P, w);
    FFM_TRY(ffm_fvm_HbyA3(m, P->Uupper, P->Ulower, P->Usrc, P->Uic, P->Ubc, P->U, w.rAU, w.HbyA));
    for (int c = 0; c < 3; c++) FFM_TRY(HX(P, w.HbyA[c]));
    return FFM_OK;
}

// phig and fvc::flux(rho*HbyA), one operator per launch
static int pc_phig_flux_ops(ffm_plume *P, const PCorr &w)
{
    ffm_mesh *m = P->mesh;
    double *sg = P->wF[1], *phig = w.phig, *rH[3] = {P->wN[5], P->wN[6], P->wN[7]};
    const double *ghf = P->ghf, *magSf = ffm_mesh_geom(m, 1), *rhorAUf = w.rhorAUf;
    FFM_TRY(ffm_fvc_snGrad(m, P->rho, sg));
    forN(P, P->nNat, [=] __device__(long e) { phig[e] = -rhorAUf[e] * ghf[e] * sg[e] * magSf[e]; });
    for (int c = 0; c < 3; c++) mul(P, rH[c], P->rho, w.HbyA[c], P->N);
    return ffm_fvc_flux(m, rH[0], rH[1], rH[2], w.phiHbyA);
}
static int pc_ddtCorr_ops(ffm_plume *P, const PCorr &w, bool evalDdtCorr)
{
    ffm_mesh *m = P->mesh; const int N = P->N; const long nNat = P->nNat; const double rdt = P->rdt;
    double *rU0[3] = {P->wN[8], P->wN[9], P->wN[10]}, *fl0 = P->wF[4];
    double *phiHbyA = w.phiHbyA, *dc = P->ddtCorrF; const double *rhorAUf = w.rhorAUf, *phig = w.phig;
    if (evalDdtCorr) {
        const double *phi0 = P->phi;
        for (int c = 0; c < 3; c++) mul(P, rU0[c], P->rho0, P->U0[c], N);
        FFM_TRY(ffm_fvc_flux(m, rU0[0], rU0[1], rU0[2], fl0));
        forN(P, nNat, [=] __device__(long e) {
            const double phiCorr = phi0[e] - fl0[e];
            const double coeff = 1.0 - fmin(fabs(phiCorr) / (fabs(phi0[e]) + 1e-15), 1.0);
            dc[e] = coeff * rdt * phiCorr;
        });
    }
    forN(P, nNat, [=] __device__(long e) { phiHbyA[e] = (phiHbyA[e] + rhorAUf[e] * dc[e]) + phig[e]; });
    return FFM_OK;
}
// phig = -rhorAUf*ghf*snGrad(rho)*magSf; phiHbyA = fvc::flux(rho*HbyA) + rhorAUf*fvc::ddtCorr(rho, U, phi) + phig: interior by linear interpolation; boundary
// rho_b*HbyA_b.Sf with constrainHbyA.  ddtCorr reads old-time fields only: evaluated in the first corrector of a step, while phi
// still holds the old-time flux (pc_flux overwrites it), and reused by the second.  The fused form: rhorAUf, phig and phiHbyA of the
// internal faces in one owner-row pass (ffm_pc_face_fluxes), after the patch part
static int pc_phiHbyA(ffm_plume *P, const PCorr &w)
{
    ffm_mesh *m = P->mesh; const bool ops = !P->fused;
    if (ops) FFM_TRY(pc_phig_flux_ops(P, w));
    {
        const double *bSx = ffm_mesh_geom(m, 6), *bSy = ffm_mesh_geom(m, 7), *bSz = ffm_mesh_geom(m, 8);
        const int *fc = ffm_mesh_bcells(m); const double *kind = P->kind_d, *rhob = w.rhob; double *phiHbyAb = w.phiHbyAb;
        const double *h0 = w.HbyA[0], *h1 = w.HbyA[1], *h2 = w.HbyA[2], *u0 = P->Ub[0], *u1 = P->Ub[1], *u2 = P->Ub[2];
        forN(P, P->B, [=] __device__(long k) {
            const bool fixed = kind[k] < 1.5; const int c = fc[k];
            const double a0 = fixed ? u0[k] : h0[c], a1 = fixed ? u1[k] : h1[c], a2 = fixed ? u2[k] : h2[c];
            phiHbyAb[k] = (rhob[k] * a0 * bSx[k] + rhob[k] * a1 * bSy[k]) + rhob[k] * a2 * bSz[k];
        });
    }
    const bool evalDdtCorr = !P->ddtCorrValid;
    P->ddtCorrValid = true;
    if (ops) return pc_ddtCorr_ops(P, w, evalDdtCorr);
    if (evalDdtCorr) FFM_TRY(ffm_fvc_ddt_corr(m, P->rdt, P->rho0, P->U0[0], P->U0[1], P->U0[2], P->phi, P->ddtCorrF));
    return ffm_pc_face_fluxes(m, w.rhorAU, P->ghf, P->rho, w.HbyA[0], w.HbyA[1], w.HbyA[2], P->ddtCorrF, w.rhorAUf, w.phig, w.phiHbyA);
}

static int pc_p_rgh_eqn_ops(ffm_plume *P, const PCorr &w)
{
    ffm_mesh *m = P->mesh; const double rdt = P->rdt;
    double *div = P->wN[8];
    FFM_TRY(ffm_fvc_surface_integrate(m, w.phiHbyA, w.phiHbyAb, div));
    double *s = P->src[0]; const double *V = ffm_mesh_geom(m, 0), *psi = P->psi, *rho = P->rho;
    const double *psi0 = P->psi0, *prgh0 = P->p_rgh0, *rho0 = P->rho0, *gh = P->gh;
    forN(P, P->N, [=] __device__(long i) {
        // fvc::ddt(psi,rho)*gh, fvc::ddt(psi)*pRef, fvc::div(phiHbyA): one source update each (solver/pEqn.H:30-33)
        s[i] = ((rdt * psi0[i] * prgh0[i] * V[i] - V[i] * (rdt * (psi[i] * rho[i] - psi0[i] * rho0[i]) * gh[i]))
                - V[i] * (rdt * (psi[i] - psi0[i]) * PREF)) - V[i] * div[i];
    });
    return ffm_fvm_add_boundary(m, P->ic[0], P->bc[0], P->diag, P->src[0], nullptr, P->dWork, P->sWork);
}
// constrainPressure: gradient on fixedFluxPressure patches; then
// p_rghEqn = fvm::ddt(psi,p_rgh) + fvc::ddt(psi,rho)*gh + fvc::ddt(psi)*pRef + fvc::div(phiHbyA) - fvm::laplacian(rhorAUf,p_rgh)
static int pc_p_rgh_eqn(ffm_plume *P, const PCorr &w, bool final)
{
    ffm_mesh *m = P->mesh; const bool ops = !P->fused;
    double *grads = P->wB[6];
    {
        const double *bMag = ffm_mesh_geom(m, 4), *bSx = ffm_mesh_geom(m, 6), *bSy = ffm_mesh_geom(m, 7), *bSz = ffm_mesh_geom(m, 8);
        const double *u0 = P->Ub[0], *u1 = P->Ub[1], *u2 = P->Ub[2], *phiHbyAb = w.phiHbyAb, *rhob = w.rhob, *rhorAUfb = w.rhorAUfb;
        forN(P, P->B, [=] __device__(long k) {
            grads[k] = (phiHbyAb[k] - rhob[k] * ((bSx[k] * u0[k] + bSy[k] * u1[k]) + bSz[k] * u2[k])) / (bMag[k] * rhorAUfb[k]);
        });
    }
    FFM_TRY(bc_p_rgh(P, grads, w.rhob));
    if (ops) FFM_TRY(ffm_fvm_transport(m, P->rdt, P->psi, nullptr, nullptr, w.rhorAUf, -1, P->diag, P->upper, P->lower));
    FFM_TRY(ffm_fvm_boundary_coeffs(m, nullptr, w.rhorAUfb, -1, P->fP, P->refP, P->gradP, P->ic[0], P->bc[0]));
    // (the fused form writes no `lower`: the matrix is symmetric, the solve and pc_flux_U read `upper` in both roles)
    if (ops) FFM_TRY(pc_p_rgh_eqn_ops(P, w));
    else DIRECT_OR(P, ffm_fvm_pressure_eqn_direct(m, P->rdt, P->psi, P->psi0, P->p_rgh0, P->rho, P->rho0, P->gh, PREF, w.rhorAUf, w.phiHbyA, w.phiHbyAb,
                                                  P->ic[0], P->bc[0], P->upper, nullptr, P->dWork, P->sWork),
                   ffm_fvm_pressure_eqn(m, P->rdt, P->psi, P->psi0, P->p_rgh0, P->rho, P->rho0, P->gh, PREF, w.rhorAUf, w.phiHbyA, w.phiHbyAb,
                                        P->ic[0], P->bc[0], P->upper, nullptr, P->dWork, P->sWork));
    FFM_TRY(solve_named(P, "p_rgh", FFM_PCG, FFM_DIC, 1e-6, final ? 0.0 : 0.01, P->dWork, P->upper, nullptr, P->p_rgh, P->sWork));
    return HX(P, P->p_rgh);
}

// phi = phiHbyA + p_rghEqn.flux(); U = HbyA + rAU*reconstruct((p_rghEqn.flux() + phig)/rhorAUf), K = 0.5 magSqr(U), p = p_rgh + rho*gh + pRef,
// dpdt = fvc::ddt(p), and rhoEqn.H after p.  On a single block the fused form is one pass over the cells after the patch part
// (ffm_pc_finish: the flux, phi, reconstruct, U, K, p, dpdt and rhoEqn.H, which reads none of them; no flux, t or rec field; a hex
// block's rows have at most 6 entries, see rho_eqn); on a decomposed block U's ghost cells are refreshed before K.  The per-operator
// form takes K and dpdt after rhoEqn.H
static int pc_flux_U(ffm_plume *P, const PCorr &w)
{
    ffm_mesh *m = P->mesh; const int N = P->N; const double rdt = P->rdt; const bool ops = !P->fused;
    double *t = P->wF[5], *tb = P->wB[6];
    double *phi = P->phi, *phib = P->phib; const double *phiHbyA = w.phiHbyA, *fl = w.fl, *phig = w.phig, *rhorAUf = w.rhorAUf;
    const double *phiHbyAb = w.phiHbyAb, *flb = w.flb, *rhorAUfb = w.rhorAUfb;
    const double *lower = ops ? P->lower : P->upper;
    FFM_TRY(ffm_fvm_flux(m, P->upper, lower, P->ic[0], P->bc[0], P->p_rgh, ops ? w.fl : nullptr, w.flb));
    if (!ops && P->oneBlock) {
        forN(P, P->B, [=] __device__(long k) { phib[k] = phiHbyAb[k] + flb[k]; tb[k] = flb[k] / rhorAUfb[k]; });
        return ffm_pc_finish(m, rdt, PREF, P->upper, lower, P->p_rgh, phiHbyA, phig, rhorAUf, phib, tb, w.rAU, w.HbyA, P->gh, P->p0, P->rho0,
                             phi, P->U, P->K, P->p, P->dpdt, P->rho);
    }
    if (ops) forN(P, P->nNat, [=] __device__(long e) { phi[e] = phiHbyA[e] + fl[e]; t[e] = rhorAUf[e] != 0.0 ? (fl[e] + phig[e]) / rhorAUf[e] : 0.0; });
    else FFM_TRY(ffm_pc_flux(m, P->upper, lower, P->p_rgh, phiHbyA, phig, rhorAUf, w.fl, phi, t));
    forN(P, P->B, [=] __device__(long k) { phib[k] = phiHbyAb[k] + flb[k]; tb[k] = flb[k] / rhorAUfb[k]; });
    FFM_TRY(ffm_fvc_reconstruct(m, t, tb, w.rec[0], w.rec[1], w.rec[2]));
    const double *rAU = w.rAU, *rx = w.rec[0], *ry = w.rec[1], *rz = w.rec[2], *h0 = w.HbyA[0], *h1 = w.HbyA[1], *h2 = w.HbyA[2];
    double *U0 = P->U[0], *U1 = P->U[1], *U2 = P->U[2], *K = P->K, *dpdt = P->dpdt, *p = P->p;
    const double *rho = P->rho, *p_rgh = P->p_rgh, *gh = P->gh, *p0 = P->p0;
    forN(P, P->nOwn, [=] __device__(long i) {
        const double a = h0[i] + rAU[i] * rx[i], b = h1[i] + rAU[i] * ry[i], c = h2[i] + rAU[i] * rz[i];
        U0[i] = a; U1[i] = b; U2[i] = c;
    });
    FFM_TRY(HX(P, U0)); FFM_TRY(HX(P, U1)); FFM_TRY(HX(P, U2));
    forN(P, N, [=] __device__(long i) { p[i] = p_rgh[i] + rho[i] * gh[i] + PREF; });
    FFM_TRY(rho_eqn(P));
    forN(P, N, [=] __device__(long i) {
        K[i] = 0.5 * ((U0[i] * U0[i] + U1[i] * U1[i]) + U2[i] * U2[i]);
        dpdt[i] = rdt * (p[i] - p0[i]);
    });
    return FFM_OK;
}

static int p_corrector(ffm_plume *P, bool final)
{
    const PCorr w = {P->wN[0], P->wN[1], {P->wN[2], P->wN[3], P->wN[4]}, {P->wN[5], P->wN[6], P->wN[7]},
                     P->wF[0], P->wF[2], P->wF[3], P->wF[4],
                     P->wB[0], P->wB[4], P->wB[5], P->wB[7]};
    FFM_TRY(pc_rAU_HbyA(P, w));
    FFM_TRY(update_bcs(P));
    FFM_TRY(U_boundary(P));
    zg(P, w.rhob, P->rho);
    FFM_TRY(pc_phiHbyA(P, w));
    FFM_TRY(pc_p_rgh_eqn(P, w, final));
    return pc_flux_U(P, w);
}

// ---------------- turbulence->correct() (solver/fireFoam.C:113-116): kEqn::correct
// bound(k, kMin) and correctNut(): nut = Ck sqrt(k) delta, alphat = rho nut/Prt with the present rho, over the ghost cells too (k and rho
// are refreshed there and delta is theirs: the values a refresh of nut and alphat would bring); then the patch values, zeroGradient
// and 0 on the floor.  The fused form is one cell pass (ffm_les_keqn_update)
static int correct_nut(ffm_plume *P)
{
    double *k = P->kSgs, *nut = P->nut, *alphat = P->alphat, *nutb = P->nutb, *alphatb = P->alphatb;
    if (P->fused) FFM_TRY(ffm_les_keqn_update(P->mesh, P->N, K_MIN, P->Ck, P->Prt, k, P->lesDelta, P->rho, nut, alphat));
    else {
        forN(P, P->N, [=] __device__(long i) { k[i] = fmax(k[i], K_MIN); });
        FFM_TRY(ffm_les_keqn_nut_d(P->ctx, P->N, P->Ck, P->Prt, k, P->lesDelta, P->rho, nut, alphat));
    }
    const int *fc = ffm_mesh_bcells(P->mesh); const double *kind = P->kind_d;
    forN(P, P->B, [=] __device__(long q) {
        const bool floor = kind[q] > 0.5 && kind[q] < 1.5;
        nutb[q] = floor ? 0.0 : nut[fc[q]]; alphatb[q] = floor ? 0.0 : alphat[fc[q]];
    });
    return FFM_OK;
}

int plume_turbulence_init(ffm_plume *P)
{
    bc_update_f(P, P->fS, P->fStaticS);
    FFM_TRY(ffm_bc_values(P->mesh, P->fS, P->refK, P->zeroB, P->kSgs, P->kb));
    return correct_nut(P);
}

// divU = surfaceIntegrate(phi/interpolate(rho)), G = nut (grad U && dev(twoSymm(grad U))) and the three source arrays, one operator per launch
static int k_eqn_terms_ops(ffm_plume *P, const double *const *g9, const double *rhob, double *su, double *su2, double *sp)
{
    ffm_mesh *m = P->mesh;
    double *G = P->wN[8], *divU = P->wN[9], *rhof = P->wF[1], *pr = P->wF[2], *prb = P->wB[5];
    const double *phi = P->phi, *phib = P->phib, *rho = P->rho, *k = P->kSgs, *delta = P->lesDelta; const double Ce = P->Ce;
    FFM_TRY(ffm_fvc_interpolate(m, nullptr, rho, rhof));
    forN(P, P->nNat, [=] __device__(long e) { pr[e] = phi[e] / rhof[e]; });
    forN(P, P->B, [=] __device__(long q) { prb[q] = phib[q] / rhob[q]; });
    FFM_TRY(ffm_fvc_surface_integrate(m, pr, prb, divU));
    FFM_TRY(ffm_les_keqn_G(m, g9, P->nut, G));
    forN(P, P->nOwn, [=] __device__(long i) { su[i] = rho[i] * G[i]; });
    forN(P, P->nOwn, [=] __device__(long i) { const double ss = (2.0 / 3.0) * rho[i] * divU[i]; su2[i] = -(fmin(ss, 0.0) * k[i]); });
    forN(P, P->nOwn, [=] __device__(long i) { const double ss = (2.0 / 3.0) * rho[i] * divU[i]; sp[i] = fmax(ss, 0.0) + Ce * rho[i] * sqrt(k[i]) / delta[i]; });
    return FFM_OK;
}

// ddt(rho,k) + div(phi,k) [Gauss limitedLinear 1, the limiter from grad(k) with k's stored patch values] - laplacian(rho nuEff, k)
//   == rho G - SuSp(2/3 rho divU, k) - Sp(Ce rho sqrt(k)/delta, k);  bound(k, SMALL);  correctNut()
// after the second corrector, with its phi, U and rho (rhoEqn.H's, before rho = thermo.rho()) and the nut of the last correctNut().  k's
// condition is the species' pattern (fS).  The fused form: the explicit terms in one owner-row pass (ffm_les_keqn_terms), the face
// diffusivity in one (ffm_les_face_diffusivity), the assembly in one (ffm_fvm_scalar_transport_multi, as e_eqn with a limiter of its own).
// grad(U) is read at a row's own cell only and is not refreshed; grad(k) and k are
static int k_eqn(ffm_plume *P)
{
    ffm_mesh *m = P->mesh; const bool ops = !P->fused;
    double *su = P->wN[5], *su2 = P->wN[6], *sp = P->wN[7], *Dkf = P->wF[0], *Dkb = P->wB[4], *rhob = P->wB[6], *k = P->kSgs;
    FFM_TRY(update_bcs(P));
    FFM_TRY(U_boundary(P));
    const double *g9[9]; les_gradU(P, g9);
    if (ops) { for (int c = 0; c < 3; c++) FFM_TRY(ffm_fvc_grad(m, P->U[c], P->Ub[c], P->lesG[c][0], P->lesG[c][1], P->lesG[c][2])); }
    else {
        const double *uf[3] = {P->U[0], P->U[1], P->U[2]}, *ub[3] = {P->Ub[0], P->Ub[1], P->Ub[2]};
        double *ggx[3] = {P->gM[0][0], P->gM[1][0], P->gM[2][0]}, *ggy[3] = {P->gM[0][1], P->gM[1][1], P->gM[2][1]}, *ggz[3] = {P->gM[0][2], P->gM[1][2], P->gM[2][2]};
        FFM_TRY(ffm_fvc_grad_multi(m, 3, uf, ub, ggx, ggy, ggz));
    }
    FFM_TRY(les_rho_nuEff_faces(P, P->wN[10], false, rhob, Dkf, Dkb));
    if (ops) FFM_TRY(k_eqn_terms_ops(P, g9, rhob, su, su2, sp));
    else FFM_TRY(ffm_les_keqn_terms(m, g9, P->nut, P->rho, rhob, k, P->lesDelta, P->phi, P->phib, P->Ce, su, su2, sp));
    if (ops) FFM_TRY(scalar_transport(P, "k", 2, k, k, P->fS, P->refK, Dkf, Dkb, su, nullptr, 1e-8, su2, sp, nullptr, P->kb));
    else {
        const double *vf[1] = {k}, *vb[1] = {P->kb}, *fq[1] = {P->fS}, *rq[1] = {P->refK}, *gq[1] = {P->zeroB}, *suq[1] = {su}, *su2q[1] = {su2}, *spq[1] = {sp};
        double *ggx[1] = {P->gM[3][0]}, *ggy[1] = {P->gM[3][1]}, *ggz[1] = {P->gM[3][2]};
        const double *cgx[1] = {ggx[0]}, *cgy[1] = {ggy[0]}, *cgz[1] = {ggz[0]};
        double *dd[1] = {P->dWork}, *uu[1] = {P->upper}, *ll[1] = {P->lower}, *ss[1] = {P->sWork};
        FFM_TRY(ffm_fvc_grad_multi(m, 1, vf, vb, ggx, ggy, ggz));
        FFM_TRY(HX(P, ggx[0])); FFM_TRY(HX(P, ggy[0])); FFM_TRY(HX(P, ggz[0]));
        // (the old-time k is k itself until the solve: nothing has written it since the last step's correct())
        FFM_TRY(ffm_fvm_scalar_transport_multi(m, 1, 2, 1.0, 0.0, 1.0, P->rdt, P->rho, P->rho0, P->phi, P->phib, Dkf, Dkb, vf, cgx, cgy, cgz, vf,
                                               fq, rq, gq, suq, su2q, spq, nullptr, dd, uu, ll, ss));
        FFM_TRY(solve_named(P, "k", FFM_PBICGSTAB, FFM_DILU, 1e-8, 0.0, P->dWork, P->upper, P->lower, k, P->sWork));
        FFM_TRY(HX(P, k));
    }
    FFM_TRY(ffm_bc_values(m, P->fS, P->refK, P->zeroB, k, P->kb));
    return correct_nut(P);
}

extern "C" int ffm_plume_step(ffm_plume *P)
{
    if (!P) return FFM_ERR_ARG;
    P->log.clear();
    P->ddtCorrValid = false;
    store_old_time(P);
    FFM_TRY(rho_eqn(P));
    FFM_TRY(u_eqn(P));
    FFM_TRY(combustion_correct(P));
    if (P->turbModel) FFM_TRY(les_alpha_eff(P));
    FFM_TRY(mv_weights(P));
    bool spOffDiagBound;
    const bool radNow = (P->radFreq > 0 && P->stepNo % P->radFreq == 0) || (P->p1Freq > 0 && P->stepNo % P->p1Freq == 0);
    // (with greyMeanAbsorptionEmission h keeps its own EEqn in every step: radiation->Sh reads a of the species the Yi equations have just
    // solved, solver/YEEqn.H:43-60 before :101, which the five lock-step systems, assembled together, cannot give it)
    const bool jointYh = P->fused && P->mvSelection && !P->stecklerSolvers && P->oneBlock && !radNow && !P->separateH && !P->gm;
    FFM_TRY(species_eqns(P, &spOffDiagBound, jointYh));
    if (radNow) { FFM_TRY(radiation_correct(P)); spOffDiagBound = false; }     // radiation->correct(), solver/YEEqn.H:80: its ray solves bind other coefficients
    if (!jointYh) FFM_TRY(e_eqn(P, spOffDiagBound));
    FFM_TRY(thermo_correct(P));
    FFM_TRY(p_corrector(P, false));
    FFM_TRY(p_corrector(P, true));
    if (P->turbModel) FFM_TRY(k_eqn(P));
    mul(P, P->rho, P->psi, P->p, P->N);
    P->time += P->dt; P->stepNo++;
    thermo_flag_fetch(P);           // thermo::T's iteration-limit flag travels with the synchronisation that closes the step
    absem_flag_fetch(P);
    PL_HIP(hipStreamSynchronize(P->ctx->stream));
    absem_flag_check(P);
    return thermo_flag_check(P);
}
