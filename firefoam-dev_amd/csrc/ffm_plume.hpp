// ffm_plume.hpp -- the handle of the synthetic buoyant-plume case and what its translation units share: ffm_plume.hip (create / destroy,
// setters, getters, hydrostatic initialisation), ffm_plume_step.hip (the time step), ffm_plume_rad.hip (the fvDOM stand-in and P1).  The physics
// plug-ins that the reference takes from other libraries are replaced by the stand-ins listed in oracle/plume.py (perfect gas / constant
// Cp, constant mu, Pr, EDC-shaped single-step source, zero-gradient thermo boundary values); their constants are below.
// Opt-in, the reference's own models take their place: LES kEqn (ffm_plume_set_turbulence), janaf / sutherland thermo (ffm_plume_set_thermo), EDC
// (ffm_plume_set_combustion); the patch values of the thermo fields stay zero-gradient copies.
#pragma once
#include "ffm_internal.hpp"
#include "ffm_device.hpp"
#include <algorithm>
#include <cmath>
#include <string>

namespace {
constexpr double RR = 8314.47, CP = 1005.0, TREF = 298.15, PREF = 101325.0, MU = 1.8e-5, PR = 0.7;
constexpr double S_O2 = 3.6282945, HC = 46357151.0, TAU = 0.05, T_IN = 600.0, U_IN = 0.5, SIGMA_SB = 5.670367e-8;
constexpr int NSP = 5, INERT = 4;
const double WMOL[NSP] = {31.9988, 18.0153, 44.0962, 44.01, 28.0134};
const double Y_AMB[NSP] = {0.23301, 0.0, 0.0, 0.0, 0.76699};
const double Y_IN[NSP] = {0.0, 0.0, 1.0, 0.0, 0.0};
const double NU[NSP] = {-S_O2, 4 * 18.0153 / 44.0962, -1.0, 3 * 44.01 / 44.0962, 0.0};
const char *const SPN[NSP] = {"O2", "H2O", "C3H8", "CO2", "N2"};
enum { P_INLET = 0, P_FLOOR = 1, P_TOP = 2, P_SIDES = 3 };

template <class F> __global__ void k_for(long n, F f)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) f(i);
}
}  // namespace

struct SolveLog { char name[16]; ffm_perf perf; };

struct ffm_plume {
    ffm_ctx *ctx = nullptr; ffm_ldu *A = nullptr; ffm_mesh *mesh = nullptr;
    int nx = 0, ny = 0, nz = 0, N = 0, nOwn = 0, F = 0, nNat = 0, B = 0;   // N = owned + ghost cells
    bool oneBlock = true;                  // the whole box on this rank: no ghost cells (N == nOwn), no ghost refresh between passes
    double h = 0.05, dt = 1e-3, rdt = 1e3, time = 0.0;
    std::vector<int> newToOld;             // library cell order -> natural blockMesh cell id
    std::vector<int> faceNewToOld;         // library (caller-side) face order -> natural blockMesh face id
    bool mvOverride = false;               // tests: the next step convects the species and h with weights handed in (ffm_plume_override_mv_weights)
    double hAmb = 0.0;                     // inletOutlet reference value of h on the open patches
    std::vector<double *> pool;            // every device buffer, for destroy
    // fields
    double *Y[NSP], *Y0[NSP], *T, *hs, *hs0, *U[3], *U0[3], *p, *p0, *p_rgh, *p_rgh0, *psi, *psi0, *rho, *rho0, *K, *K0, *dpdt;
    double *phi, *phib, *gh, *ghf, *ph_rgh, *ph_rgh_b;      // (phi's old-time value is read from phi itself: pc_phiHbyA)
    // boundary-condition data [B]
    double *kind_d;                        // patch kind per boundary face (as double for simple kernels)
    double *fU[3], *refU[3], *fS, *refS, *fP, *refP, *gradP, *zeroB, *oneB;
    double *fStaticU[3], *fStaticS, *fStaticH, *fH, *refY[NSP], *refH;      // static templates (-1 = inletOutlet)
    // matrix + work
    double *diag, *upper, *lower, *src[3], *ic[3], *bc[3], *dWork, *sWork;       // (the fused p_rghEqn is symmetric and writes no `lower`)
    double *UdW[3], *UsW[3];               // diagonal + source of the three components (one lock-step solve)
    // Scratch: cell [N], face [nNat] and patch-face [B] fields.  A stage names the slots it uses in one block at its head; a value that
    // lives from one stage into a later one has a member of its own (next line).  `->`: must survive calls into other stages / the library.
    // (ops): the per-operator form only (FFM_PLUME_UNFUSED); (ops, blocks): that form and the fused one on a decomposed box -- the fused
    // single-block step forms the value where it is used and leaves the slot alone.
    //   wN[0]    hydrostatic_init, rho_eqn_ops: div | e_eqn (or species_eqns with h): ddtK -> | p_corrector: rAU -> (read for the last time before pc_flux_U's rho_eqn)
    //   wN[1-3]  u_source_ops, scalar_transport, mv_weights_ops, e_K_terms: a gradient | p_corrector: rhorAU, HbyA[0-1] ->
    //   wN[4]    u_source_ops: divc | e_eqn: divK -> (scalar_transport reads it before it writes its source sum here) | p_corrector: HbyA[2] ->
    //   wN[5-7]  u_eqn (ops), pc_flux_U (ops, blocks): reconstruct(...) -> | e_eqn: [5] -dpdt -> | pc_phig_flux_ops: rho*HbyA
    //   wN[8-10] wFuel, Qdot, Yt: combustion_correct -> species_eqns, radiation_correct, e_eqn | pc_ddtCorr_ops: rho0*U0 | pc_p_rgh_eqn_ops: [8] div
    //   wN[11]   species_eqns_ops: nu_i*wFuel
    //   wF[0]    hydrostatic_init: rhof | u_eqn: muf | alphaEff_f: combustion_correct -> species_eqns, e_eqn | p_corrector: rhorAUf ->
    //   wF[1]    hydrostatic_init, u_buoyancy, pc_phig_flux_ops: snGrad(rho) | u_sources (fused single block): phi*LUST correction of Ux |
    //            mv_weights_ops: limiter
    //   wF[2]    hydrostatic_init: phig | u_buoyancy: snGrad(p_rgh) | u_sources (fused single block): phi*LUST correction of Uy | p_corrector: phig ->
    //   wF[3]    u_eqn (ops): LUST weights -> | scalar_transport, e_K_terms_ops: a field's own weights | p_corrector: phiHbyA ->
    //   wF[4]    u_buoyancy (ops): reconstruct's argument, then u_source_ops: phi*correction (fused single block: of Uz) | e_K_terms_ops: phi*Kf | pc_ddtCorr_ops: flux(rho0*U0),
    //            then p_corrector (ops, blocks): p_rghEqn.flux() ->      wF[5]  pc_flux_U (ops, blocks): reconstruct's argument
    //   wB[0]    hydrostatic_init: rhob | e_K_terms: Kb, then (after Kb's last reader) plume_rad_fraction: burner flux | p_corrector: rhorAUfb ->
    //   wB[1-3]  Ub: U_boundary -> the end of the stage that called it (u_eqn, e_K_terms, p_corrector); in between hydrostatic_init: [1] fTop |
    //            mv_weights: [1] inert specie's, [3] h's patch values | scalar_transport: [2] patch values
    //   wB[4]    u_eqn: mub -> | alphaEff_b: combustion_correct -> species_eqns, e_eqn | p_corrector: rhob ->
    //   wB[5]    u_buoyancy: reconstruct's argument -> u_eqn's source pass (after u_sources) | e_K_terms_ops: phib*Kb | p_corrector: phiHbyAb ->
    //   wB[6]    u_buoyancy: rhob | pc_p_rgh_eqn: constrainPressure gradient (until bc_p_rgh), then pc_flux_U: reconstruct's argument
    //   wB[7]    u_buoyancy: p_rgh patch values | p_corrector: p_rghEqn.flux() on the patches
    double *wN[12], *wF[6], *wB[8];
    double *wFuel, *Qdot, *Yt, *alphaEff_f, *alphaEff_b, *Ub[3];
    double *ddtCorrF = nullptr; bool ddtCorrValid = false;      // coeff*rDeltaT*phiCorr of fvc::ddtCorr(rho, U, phi): old-time fields only, the same in both correctors of a step
    // fused assembly (ffm_fused.hip): gradients of up to 4 fields, the matrices of the 4 transported species, their patch values
    double *gM[4][3], *spD[4], *spU[4], *spL[4], *spS[4], *spB[4], *suM[4];
    // mvConvection of solver/YEEqn.H:1-10 (`Gauss multivariateSelection`): the weights of the ONE limiter all species and h are
    // convected with -- the minimum of the member schemes' limiters over the five species and h (FFM_PLUME_INDEPENDENT_LIMITERS=1:
    // one limiter per field, as round 1 had it; wMv is then null)
    bool mvSelection = true;
    double *wMv = nullptr, *mvG[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    // fvc::div(phi,K) of EEqn on the fused single block: the tile pass of mv_weights also forms phi_f*Kf per face (phiKf [nNat]) from K's
    // patch values (KbM [B]), and e_K_terms sums them.  Both live from mv_weights over the species solves and radiation_correct to
    // e_K_terms; phiKValid: this step's mv_weights wrote them (not with weights handed in, one limiter per field, a refused tile form)
    double *phiKf = nullptr, *KbM = nullptr; bool phiKValid = false;
    bool fused = true;                     // FFM_PLUME_UNFUSED: one kernel per operator (tests compare the two paths)
    bool separateH = false;                // FFM_PLUME_SEPARATE_H: h assembled and solved after the species, never as their fifth system
    int jointSteps = 0;                    // steps in which h was the fifth system of the species' pass and solve (ffm_plume_joint_steps)
    // UEqn kept for pEqn (A, H)
    double *Udiag, *Uupper, *Ulower, *Usrc[3], *Uic[3], *Ubc[3];
    std::vector<SolveLog> log;
    bool tight = false;                    // tests: every solve to 1e-13 / relTol 0 (removes the stopping-rule noise)
    // fvDOM stand-in: off unless ffm_plume_set_radiation() was called
    int stepNo = 0, radFreq = 0;
    std::vector<double> rayD, rayOmega;    // dAve[3] and omega per ray
    // direction-ordered ray solves (single block): for the flip of axis a, radCm[a][c] = cell that takes c's place and
    // radFm[a][e] = native face that takes e's place (bit-complemented where owner and neighbour change roles); the permuted
    // system has the sparsity of A and is triangular for every ray whose minority-sign axis is a, so DILU solves it exactly
    // (solve_ray gathers it into radDB .. radLB).  hL2, hU2, hOldToNew: the renumbered addressing on the host the maps are made from
    std::vector<int> hL2, hU2, hOldToNew;
    int *radCm[3] = {nullptr, nullptr, nullptr}, *radFm[3] = {nullptr, nullptr, nullptr};
    double *radDB = nullptr, *radSB = nullptr, *radPsiB = nullptr, *radUB = nullptr, *radLB = nullptr;
    bool radOrdered = false;               // single block with the flip maps: every ray is one exact DILU application
    // staged sweep over the blocks of a box decomposition (ffm_plume_set_radiation_ordering 1): the flip maps of the owned cells,
    // the owned cells that have a cut face, this block's place in the block grid, the ghost layers' offsets, and per tick the
    // ray this rank solves / the ray each face neighbour solves (ffm_ray_schedule; -1: none)
    int radOrdering = 0; bool radMaps = false, radStaged = false;
    int nbrRank[6] = {-1, -1, -1, -1, -1, -1}, gOff[7] = {0, 0, 0, 0, 0, 0, 0}, blkGrid[3] = {1, 1, 1}, blkAt[3] = {0, 0, 0};
    int *radHaloCells = nullptr; int nRadHaloCells = 0; double *radGhostBuf = nullptr;
    std::vector<int> radTick, radNbrTick[6];
    // the rays, G, and the per-operator assembly's face and patch arrays; radRef [B] is the black inflow at the ambient temperature,
    // filled where it is allocated (ffm_plume_set_radiation) and only read after that
    std::vector<double *> I; double *G = nullptr, *radJ = nullptr, *radW = nullptr, *radJb = nullptr, *radF = nullptr, *radRef = nullptr, *radSrc = nullptr;
    // the reference's absorption / emission model and radiation->Sh (ffm_plume_set_radiation_model): constant absorption
    // coefficient, emission E = RadFraction*Qdot with the radScaling of constRadFractionEmission::ECont
    bool radCoupled = false; double radA = 0.1, Ehrr1 = 0.0, Ehrr2 = 0.0;
    double *radE = nullptr, *radShSu = nullptr, *radShSp = nullptr; bool radHaveG = false;
    // greyMeanAbsorptionEmission in place of the constant a and of RadFraction*Qdot (ffm_plume_set_absorption_emission): the borrowed
    // handle, a of the cells (current at every radiation->correct() and every radiation->Sh) and its zero-gradient patch copy (P1), the
    // temperature-range flag on the device and its pinned host copy
    ffm_greymean *gm = nullptr; double *aRad = nullptr, *aRadB = nullptr; bool gmHaveA = false;
    int *gmFlag = nullptr, *gmFlagH = nullptr;
    bool radHaveSh = false;                // radShSu / radShSp hold a source pass ("ShSu", "ShSp" are readable)
    // fvDOM::updateG as one pass (ffm_fvdom_G_d): the rays' pointers and solid angles on the device, for radTabRays rays
    double **radIdd = nullptr, *radOmegaD = nullptr; int radTabRays = 0;
    // ffm_plume_set_radiation_thermo: the rays and radiation->Sh accepted together with the thermo package (Sh then reads the Cp field)
    bool radThermo = false;
    // P1 in place of the rays (ffm_plume_set_radiation_p1; off: p1Freq 0, every pointer null): its G (the rays keep theirs), the patch
    // arrays gamma_b, valueFraction, refValue, G_b, qr, T_b, the wall emissivity [B], and -- the per-operator form only -- gamma on cells and faces, su
    int p1Freq = 0;
    double *p1G = nullptr, *p1GammaB = nullptr, *p1F = nullptr, *p1Ref = nullptr, *p1Gb = nullptr, *p1Qr = nullptr, *p1Tb = nullptr, *p1EmisB = nullptr;
    double *p1GammaC = nullptr, *p1GammaF = nullptr, *p1Su = nullptr, *p1Sn = nullptr;
    bool p1HaveQr = false;
    const double *radG() const { return p1Freq > 0 ? p1G : G; }      // the G radiation->Sh reads
    bool stecklerSolvers = false;         // transport equations with smoothSolver + symGaussSeidel, maxIter 10
                                           // (cases/steckler/system/fvSolution:49-62) instead of PBiCGStab + DILU
    // LES kEqn sub-grid model (ffm_plume_set_turbulence; cases/steckler/constant/turbulenceProperties:18-30): 0 = none, every pointer null
    int turbModel = 0;
    double Ck = 0.094, Ce = 1.048, Prt = 1.0, kInlet = 1e-4;
    double *kSgs = nullptr, *nut = nullptr, *alphat = nullptr, *lesDelta = nullptr;      // cells; delta = cbrt(V)
    double *kb = nullptr, *nutb = nullptr, *alphatb = nullptr, *refK = nullptr;           // patch faces; kb: k's values after its last solve, before bound()
    double *lesG[3][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};   // (ops) grad(U_c)[d]; the fused form has gM[c][d]
    // Scratch of the model's passes, beside the table above:
    //   u_eqn: wN[8] rho*nuEff, wN[9-11] div(rho nuEff dev2(T(grad U)))
    //   combustion_correct (ops): wN[11] alpha + alphat
    //   k_eqn: wN[5-7] su, su2, sp -> the assembly | wF[0], wB[4] rho*nuEff on faces / patch faces -> | wB[6] rhob | fused: gM[0-2] grad(U), gM[3] grad(k) |
    //          (ops) wN[8] G, wN[9] divU, wN[10] rho*nuEff, wF[1] rhof, wF[2] phi/rhof, wB[5] phib/rhob, then scalar_transport's own slots
    // janaf / sutherland thermo (ffm_plume_set_thermo): the borrowed handle, or null = the stand-in; every pointer null with it
    ffm_thermo *thermo = nullptr;
    double *mu = nullptr, *alpha = nullptr, *Cp = nullptr;     // cells, ghosts included: thermo.correct()'s
    int *thermoFail = nullptr, *thermoFailH = nullptr;         // thermo::T's iteration-limit flag on the device; its pinned host copy
    // the reference's EDC (ffm_plume_set_combustion): 0 = the stand-in rate
    int combModel = 0;
    double C_EDC = 4.0, C_Diff = 0.0, C_Stiff = 1.0, edcS = S_O2, qFuel = HC;
    double *alphaStd = nullptr;            // cells: mu/Pr, the alpha EDC reads while the stand-in thermo is on
    double *wFuelOwn = nullptr, *QdotOwn = nullptr;      // wFuel and Qdot outside the scratch table while either model is on ("wFuel", "Qdot" stay readable)
    // Scratch of the two models' passes, beside the tables above:
    //   combustion_correct (ops, laminar thermo): nothing | (ops, kEqn) wN[11] alpha + alphat, as before
    //   plume_inlet_enthalpy: wB[0] T_IN, wB[2] Hs(refY, T_IN) (between stages: set-up only)
};

constexpr double K_MIN = 1.0e-15;          // bound(k, kMin): kMin = SMALL

#define PL_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { ffm_set_error("%s:%d %s", __FILE__, __LINE__, hipGetErrorString(e_)); return FFM_ERR_HIP; } } while (0)

static inline double *dalloc(ffm_plume *P, size_t n)
{
    double *p = nullptr;
    if (hipMalloc((void **)&p, sizeof(double) * std::max<size_t>(n, 1)) != hipSuccess) return nullptr;
    if (ffm_dzero(P->ctx, p, sizeof(double) * std::max<size_t>(n, 1)) != FFM_OK) { hipFree(p); return nullptr; }
    P->pool.push_back(p);
    return p;
}
static inline double *dupload(ffm_plume *P, const std::vector<double> &v)
{
    double *p = dalloc(P, v.size());
    if (p && !v.empty() && ffm_h2d(P->ctx, p, v.data(), sizeof(double) * v.size()) != FFM_OK) return nullptr;
    return p;
}
template <class Fn> static void forN(ffm_plume *P, long n, Fn f)
{
    if (n > 0) hipLaunchKernelGGL(k_for<Fn>, dim3(sgrid(n)), dim3(256), 0, P->ctx->stream, n, f);
}
static inline double *dfill(ffm_plume *P, size_t n, double value)          // a field with one value everywhere, filled on the device
{
    double *p = dalloc(P, n);
    if (p && n) forN(P, (long)n, [=] __device__(long i) { p[i] = value; });
    return p;
}
static inline void dcopy(ffm_plume *P, double *d, const double *s, long n)
{ hipMemcpyAsync(d, s, sizeof(double) * n, hipMemcpyDeviceToDevice, P->ctx->stream); }

// refresh the ghost-cell entries of a cell field from the neighbour ranks (no-op on a single rank)
static inline int HX(ffm_plume *P, double *f) { return P->oneBlock ? FFM_OK : ffm_halo_refresh_d(P->A, f); }

// ---- stand-in physics (not part of the reproduced hot path) -----------------------------------
static inline void standin_thermo(ffm_plume *P)
{   // T = Tref + h/Cp ; psi = 1/(R T sum(Y_i/W_i))
    double *T = P->T, *psi = P->psi; const double *h = P->hs;
    const double *y0 = P->Y[0], *y1 = P->Y[1], *y2 = P->Y[2], *y3 = P->Y[3], *y4 = P->Y[4];
    const double w0 = WMOL[0], w1 = WMOL[1], w2 = WMOL[2], w3 = WMOL[3], w4 = WMOL[4];
    forN(P, P->N, [=] __device__(long i) {
        const double t = TREF + h[i] / CP;
        T[i] = t;
        psi[i] = 1.0 / (RR * t * ((((y0[i] / w0 + y1[i] / w1) + y2[i] / w2) + y3[i] / w3) + y4[i] / w4));
    });
}
// thermo.correct() with the selected model over all N cells.  The stand-in: standin_thermo, the launch it always was.  The janaf
// model: fused, ONE pass without a read-back (ffm_thermo_step_d; the failure flag is read where the caller next synchronises:
// thermo_flag_fetch / thermo_flag_check); per-operator, the two public passes it replaces (ffm_thermo_correct_d reads its own flag back)
static inline int thermo_correct(ffm_plume *P)
{
    if (!P->thermo) { standin_thermo(P); return FFM_OK; }
    if (P->fused) return ffm_thermo_step_d(P->thermo, P->N, P->Y, P->hs, P->T, P->psi, P->mu, P->alpha, P->Cp, P->thermoFail);
    FFM_TRY(ffm_thermo_correct_d(P->thermo, P->N, P->Y, P->hs, P->p, P->T, P->psi, P->mu, P->alpha));
    return ffm_thermo_Cp_d(P->thermo, P->N, P->Y, P->T, P->Cp);
}
// before / after a synchronisation the caller does anyway: copy the flag to its pinned host word; report and clear it
static inline void thermo_flag_fetch(ffm_plume *P)
{ if (P->thermo && P->fused) hipMemcpyAsync(P->thermoFailH, P->thermoFail, sizeof(int), hipMemcpyDeviceToHost, P->ctx->stream); }
static inline int thermo_flag_check(ffm_plume *P)
{
    if (!P->thermo || !P->fused || !*P->thermoFailH) return FFM_OK;
    *P->thermoFailH = 0;
    hipMemsetAsync(P->thermoFail, 0, sizeof(int), P->ctx->stream);
    ffm_set_error("thermo::T: maximum number of iterations exceeded");
    return FFM_ERR_ARG;
}
// the same for greyMeanAbsorptionEmission's temperature-range flag: the reference only warns (absorptionCoeffs::checkT), so does this
static inline void absem_flag_fetch(ffm_plume *P)
{ if (P->gm) hipMemcpyAsync(P->gmFlagH, P->gmFlag, sizeof(int), hipMemcpyDeviceToHost, P->ctx->stream); }
static inline void absem_flag_check(ffm_plume *P)
{
    if (!P->gm || !*P->gmFlagH) return;
    *P->gmFlagH = 0;
    hipMemsetAsync(P->gmFlag, 0, sizeof(int), P->ctx->stream);
    ffm_set_error("greyMeanAbsorptionEmission: a temperature left a participating species' [Tlow, Thigh] in step %d", P->stepNo);
    fprintf(stderr, "--> ffm WARNING: %s\n", ffm_last_error());
}
static inline void mul(ffm_plume *P, double *o, const double *a, const double *b, long n) { forN(P, n, [=] __device__(long i) { o[i] = a[i] * b[i]; }); }

// boundary zero-gradient copy of a cell field
static inline void zg(ffm_plume *P, double *ob, const double *vf)
{ const int *fc = ffm_mesh_bcells(P->mesh); forN(P, P->B, [=] __device__(long k) { ob[k] = vf[fc[k]]; }); }

static inline int solve_named(ffm_plume *P, const char *name, int solver, int pre, double tol, double relTol, const double *d,
                              const double *up, const double *lo, double *psi, const double *src, bool sameOffDiag = false, bool keepSolver = false)
{
    // zero-copy: the driver's coefficient arrays stay untouched until the solve has returned
    FFM_TRY(ffm_ldu_bind_coeffs_native_d(P->A, d, up, lo, sameOffDiag ? 1 : 0));
    SolveLog L; memset(&L, 0, sizeof(L)); strncpy(L.name, name, sizeof(L.name) - 1);
    if (P->tight) { tol = 1e-13; relTol = 0.0; }
    int maxIter = 1000;
    if (P->stecklerSolvers && solver == FFM_PBICGSTAB && !keepSolver) { solver = FFM_SMOOTH; pre = FFM_SYMGS; maxIter = P->tight ? 1000 : 10; }
    FFM_TRY(ffm_solve_d(P->A, solver, pre, tol, relTol, 0, maxIter, 1, psi, src, &L.perf));
    P->log.push_back(L);
    return FFM_OK;
}

// n systems with the off-diagonal coefficients up / lo (the components of U; the species under the common limiter): ffm_solve_multi_d
static inline int solve_named_multi(ffm_plume *P, int n, const char *const *names, double tol, const double *const *d, const double *up, const double *lo,
                                    double *const *psi, const double *const *src)
{
    if (P->stecklerSolvers || n < 2) {
        for (int i = 0; i < n; i++) FFM_TRY(solve_named(P, names[i], FFM_PBICGSTAB, FFM_DILU, tol, 0.0, d[i], up, lo, psi[i], src[i], i > 0));
        return FFM_OK;
    }
    double relTol = 0.0;
    if (P->tight) { tol = 1e-13; relTol = 0.0; }
    std::vector<ffm_perf> pf(n);
    FFM_TRY(ffm_solve_multi_d(P->A, n, FFM_PBICGSTAB, FFM_DILU, tol, relTol, 0, 1000, d, up, lo, psi, src, pf.data()));
    for (int i = 0; i < n; i++) { SolveLog L; memset(&L, 0, sizeof(L)); strncpy(L.name, names[i], sizeof(L.name) - 1); L.perf = pf[i]; P->log.push_back(L); }
    return FFM_OK;
}

// ffm_plume_rad.hip: radiation->correct() of solver/YEEqn.H:80, and RadFraction of constRadFractionEmission (e_eqn's radiation->Sh wants it too)
int radiation_correct(ffm_plume *P);
int plume_rad_fraction(ffm_plume *P, double *out);
// ffm_plume_step.hip: k's patch values from its condition with the present phib, then bound(k) + correctNut() (ffm_plume_set_turbulence)
int plume_turbulence_init(ffm_plume *P);
