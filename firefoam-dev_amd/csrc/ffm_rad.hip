// ffm_rad.hip -- SURVEY 8(f) N1: the wall condition of the fvDOM rays, greyDiffusiveRadiationMixedFvPatchScalarField::updateCoeffs
// (reference packages/thermophysicalModels/radiation/derivedFvPatchFields/greyDiffusiveRadiation/
// greyDiffusiveRadiationMixedFvPatchScalarField.C:150-230), for ALL boundary faces of the mesh in one pass per ray solve.
// The ray equations themselves are assembled and solved by the transport kernels (ffm_fv.hip) and the LDU solvers; what is
// specific to the radiation model is this coupling of the rays through the walls: a wall of emissivity e sends back
// (1 - e) of the radiation the OTHER rays deposit on it (their qin), which is what fvDOM::calculate iterates on
// (fvDOM/fvDOM.C:547-584; cases/wallFireSpread2D/constant/radiationProperties:39-46: maxIter 5, convergence 1e-3).
#include "ffm_mesh.hpp"
#include "ffm_greymean.hpp"

// one thread per boundary face k; ray arrays are [nRay][B].  Order of the Ir sum: rays 0 .. nRay-1, the ray's own qin counted as
// the zero it was reset to (radiativeIntensityRay::correct: qin_.boundaryFieldRef() = 0 before the matrix is built).
__global__ void k_grey_diffusive(int B, int nRay, int ray, double dx, double dy, double dz, double ax, double ay, double az, double sigma,
                                 const double *__restrict__ bSx, const double *__restrict__ bSy, const double *__restrict__ bSz,
                                 const double *__restrict__ bMag, const double *__restrict__ Iw, const double *__restrict__ emis,
                                 const double *__restrict__ Tb, double *__restrict__ qinAll, double *__restrict__ qemAll,
                                 double *__restrict__ qrAll, double *__restrict__ f, double *__restrict__ ref)
{
    GRID_STRIDE(k, B) {
        const double nx = bSx[k] / bMag[k], ny = bSy[k] / bMag[k], nz = bSz[k] / bMag[k];
        const double nAve = (nx * ax + ny * ay) + nz * az;
        const double iw = Iw[k];
        qrAll[(size_t)ray * B + k] = 0.0 + iw * nAve;
        double Ir = ray == 0 ? 0.0 : qinAll[k];
        for (int j = 1; j < nRay; j++) Ir = Ir + (j == ray ? 0.0 : qinAll[(size_t)j * B + k]);
        const bool out = -((nx * dx + ny * dy) + nz * dz) > 0.0;
        const double e = emis ? emis[k] : 1.0, t = Tb[k];
        const double val = (Ir * (1.0 - e) + e * sigma * ((t * t) * (t * t))) / M_PI;
        f[k] = out ? 1.0 : 0.0;
        ref[k] = out ? val : 0.0;
        qemAll[(size_t)ray * B + k] = out ? val * nAve : 0.0;
        qinAll[(size_t)ray * B + k] = out ? 0.0 : iw * nAve;
    }
}

extern "C" int ffm_fvdom_wall_coeffs_d(ffm_mesh *m, int nRay, int ray, const double *d3, const double *dAve3, double sigma, const double *Iw_b,
                                       const double *emissivity_b, const double *T_b, double *qin_all, double *qem_all, double *qr_all,
                                       double *f_b, double *ref_b)
{
    if (!m || !d3 || !dAve3 || !Iw_b || !T_b || !qin_all || !qem_all || !qr_all || !f_b || !ref_b || nRay < 1 || ray < 0 || ray >= nRay) return FFM_ERR_ARG;
    if (m->B == 0) return FFM_OK;
    LAUNCH(k_grey_diffusive, m->B, m->B, nRay, ray, d3[0], d3[1], d3[2], dAve3[0], dAve3[1], dAve3[2], sigma, m->bSf[0], m->bSf[1], m->bSf[2], m->bMagSf,
           Iw_b, emissivity_b, T_b, qin_all, qem_all, qr_all, f_b, ref_b);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

// fvDOM::updateG, boundary part: out[k] = sum over the rays (in ray order) of all[ray][k]
__global__ void k_sum_rays(int B, int nRay, const double *__restrict__ all, double *__restrict__ out)
{
    GRID_STRIDE(k, B) {
        double s = 0.0;
        for (int j = 0; j < nRay; j++) s = s + all[(size_t)j * B + k];
        out[k] = s;
    }
}
extern "C" int ffm_fvdom_sum_rays_d(ffm_mesh *m, int nRay, const double *all, double *out_b)
{
    if (!m || !all || !out_b || nRay < 1) return FFM_ERR_ARG;
    if (m->B == 0) return FFM_OK;
    LAUNCH(k_sum_rays, m->B, m->B, nRay, all, out_b);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

// ------------------------------------------------------------------ one ray's system in one pass ---
// The equation of one fvDOM ray (radiativeIntensityRay.C:267-322 with `div(Ji,Ii_h) Gauss upwind`),
//   fvm::div(Ji, Ii) + fvm::Sp(k omega, Ii) == omega/pi (k sigma T^4 [+ E/4]),  Ji = dAve & Sf,
// inflow boundary faces at ref_b, outflow zero-gradient, as the solver takes it: what the per-operator chain
//   Ji, w (faces) | Jb, f (boundary) | ffm_fvm_transport | ffm_fvm_boundary_coeffs | diag += V k omega, source | ffm_fvm_add_boundary
// leaves in upper / lower / diag / source, every term rounded as there (so the coefficients are those of the chain bit for
// bit), from one walk over the rows: a row forms Ji of its own faces in registers, the owner writes the face coefficients.
// FIELD: the absorption coefficient is the cell field aF (an absorptionEmissionModel's aCont()) and kO, kS arrive as omega and
// sigma: the row forms a[c]*omega and a[c]*sigma, the products the host forms once for a constant.
template <int W, bool FIELD>
__global__ void k_ray_assemble(MeshView q, double d0, double d1, double d2, double kO, double cS, double kS, const double *__restrict__ aF,
                               const double *__restrict__ T, const double *__restrict__ E, const double *__restrict__ refB,
                               const double *__restrict__ bDelta, double *__restrict__ Jf, double *__restrict__ wf,
                               double *__restrict__ upper, double *__restrict__ lower, double *__restrict__ diag,
                               double *__restrict__ source)
{
    CELL_SCHED(ci, q) {
        const int c = (int)ci;
        RowEnt<W> L, U; load_lower<W>(q.v, c, L); load_upper<W>(q.v, c, U);
        double dDiv = 0.0;
        // faces where c is the neighbour: diag -= upper[f]
#pragma unroll
        for (int s = 0; s < W; s++) if (L.on[s]) {
            const int e = L.f[s];
            const double j = (d0 * q.Sfx[e] + d1 * q.Sfy[e]) + d2 * q.Sfz[e];
            const double w = j >= 0 ? 1.0 : 0.0, lo = -w * j;
            dDiv -= (lo + j);
        }
        // faces owned by c: write coefficients, diag -= lower[f]
#pragma unroll
        for (int s = 0; s < W; s++) if (U.on[s]) {
            const int e = U.f[s];
            const double j = (d0 * q.Sfx[e] + d1 * q.Sfy[e]) + d2 * q.Sfz[e];
            const double w = j >= 0 ? 1.0 : 0.0, lo = -w * j, up = lo + j;
            dDiv -= lo;
            upper[e] = up; lower[e] = lo;
            if (Jf) Jf[e] = j;
            if (wf) wf[e] = w;
        }
        const double Vc = q.V[c], t = T[c];
        const double kOc = FIELD ? aF[c] * kO : kO, kSc = FIELD ? aF[c] * kS : kS;
        double d = dDiv + Vc * kOc;
        double s = E ? Vc * (cS * (kSc * ((t * t) * (t * t)) + E[c] / 4.0)) : Vc * (cS * (kSc * ((t * t) * (t * t))));
        const int jb = q.cellB[c];
        if (jb >= 0) for (int it = q.bcStart[jb]; it < q.bcStart[jb + 1]; it++) {
            const int k = q.bcItem[it];
            const double j = (d0 * q.bSfx[k] + d1 * q.bSfy[k]) + d2 * q.bSfz[k];
            const double fk = 1.0 - (j >= 0 ? 1.0 : 0.0), rk = refB[k], gk = 0.0, dk = bDelta[k];
            d += j * (1.0 - fk);                                             // internalCoeffs
            s += -j * (fk * rk + (1.0 - fk) * gk / dk);                      // boundaryCoeffs
        }
        diag[c] = d; source[c] = s;
    }
}

extern "C" int ffm_fvdom_ray_assemble_d(ffm_mesh *m, const double *dAve3, double omega, double absorption, double sigma, const double *T,
                                        const double *E, const double *ref_b, double *J_f, double *w_f, double *upper, double *lower,
                                        double *diag, double *source)
{
    if (!m || !dAve3 || !T || !upper || !lower || !diag || !source || (m->B && !ref_b)) return FFM_ERR_ARG;
    const double kO = absorption * omega, cS = 1.0 / M_PI * omega, kS = absorption * sigma;
    FFM_DISPATCH_W(m->A->maxW, LAUNCH_CELLS((k_ray_assemble<W, false>), mview(m), dAve3[0], dAve3[1], dAve3[2], kO, cS, kS, nullptr, T, E, ref_b, m->bDelta,
                                            J_f, w_f, upper, lower, diag, source));
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}
// the same system with the absorption coefficient as a cell field: kO = a[c]*omega, kS = a[c]*sigma per row
extern "C" int ffm_fvdom_ray_assemble_v_d(ffm_mesh *m, const double *dAve3, double omega, const double *a_d, double sigma, const double *T,
                                          const double *E, const double *ref_b, double *J_f, double *w_f, double *upper, double *lower,
                                          double *diag, double *source)
{
    if (!m || !dAve3 || !a_d || !T || !upper || !lower || !diag || !source || (m->B && !ref_b)) return FFM_ERR_ARG;
    const double cS = 1.0 / M_PI * omega;
    FFM_DISPATCH_W(m->A->maxW, LAUNCH_CELLS((k_ray_assemble<W, true>), mview(m), dAve3[0], dAve3[1], dAve3[2], omega, cS, sigma, a_d, T, E, ref_b, m->bDelta,
                                            J_f, w_f, upper, lower, diag, source));
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

// The upstream ghost inflow of a ray on one block of a decomposed mesh: a cut face is an upper face of its owned cell c towards
// a ghost cell g, and upper[e] I_g is the term of row c that lies on the neighbour rank.  With I_g final (the neighbour is
// upstream of this block and has solved the ray) the term moves to the right-hand side, source_c -= upper[e] I_g in the
// row's face order, and the face leaves the matrix (both coefficients 0): what remains couples owned cells only.  On the
// downstream cut faces upper[e] is already 0.  One thread per owned cell that has a cut face (cells[n]).
__global__ void k_ray_fold_ghosts(MeshView q, int n, const int *__restrict__ cells, const double *__restrict__ I,
                                  double *__restrict__ upper, double *__restrict__ lower, double *__restrict__ source)
{
    GRID_STRIDE(i, n) {
        const int c = cells[i];
        double s = source[c];
        FOR_OWN_FACES(q, c, e, nb) if (nb >= q.v.N) {
            s = s - upper[e] * I[nb];
            upper[e] = 0.0; lower[e] = 0.0;
        }
        source[c] = s;
    }
}

extern "C" int ffm_fvdom_fold_ghost_inflow_d(ffm_mesh *m, int nCells, const int *cells, const double *I, double *upper, double *lower,
                                             double *source)
{
    if (!m || nCells < 0 || (nCells && (!cells || !I || !upper || !lower || !source))) return FFM_ERR_ARG;
    if (nCells == 0) return FFM_OK;
    LAUNCH(k_ray_fold_ghosts, nCells, mview(m), nCells, cells, I, upper, lower, source);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

// ------------------------------------------------------------------ radiation->Sh and fvDOM::updateG as cell passes ---
// radiation->Sh(thermo, he) of solver/YEEqn.H:101 (radiationModel.C:229-244 with fvDOM's Rp = 4 a sigma, Ru = a G - E,
// E = radFraction*Qdot of constRadFractionEmission::ECont): the two arrays the enthalpy assembly takes as su2 / sp.  One
// streaming pass, 4 (5 with a Cp field) doubles read and 2 written per cell; the operation order is that of oracle/plume.py:464-468.
__global__ void k_radiation_sh(long n, double KA, double Rp, double frac, const double *__restrict__ G, const double *__restrict__ T,
                               const double *__restrict__ he, const double *__restrict__ Qdot, const double *__restrict__ Cp, double CpConst,
                               double *__restrict__ su, double *__restrict__ sp)
{
    GRID_STRIDE(c, n) {
        const double t = T[c], T3 = t * t * t, cp = Cp ? Cp[c] : CpConst;
        const double Ru = KA * G[c] - frac * Qdot[c];
        sp[c] = 4.0 * Rp * T3 / cp;
        su[c] = Ru - Rp * T3 * (t - 4.0 * he[c] / cp);
    }
}
extern "C" int ffm_radiation_sh_d(ffm_ctx *ctx, long n, double absorption, double sigma, double radFraction, const double *G_d, const double *T_d,
                                  const double *he_d, const double *Qdot_d, const double *Cp_d, double CpConst, double *su_d, double *sp_d)
{
    if (!ctx || n < 0 || !G_d || !T_d || !he_d || !Qdot_d || !su_d || !sp_d) return FFM_ERR_ARG;
    if (n == 0) return FFM_OK;
    FFM_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_radiation_sh, dim3(sgrid(n)), dim3(256), 0, ctx->stream, n, absorption, 4.0 * absorption * sigma, radFraction, G_d, T_d, he_d,
                       Qdot_d, Cp_d, CpConst, su_d, sp_d);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

// The same with an absorptionEmissionModel's fields (fvDOM.C:588 Rp = 4 e sigma, :612 Ru = a G - E): sp and su in the order of
// k_radiation_sh.  a and e may be one array (no __restrict__ on them).
__device__ __forceinline__ void radiation_sh_cell(double a, double e, double sigma, double E, double G, double t, double he, double cp,
                                                  double &su, double &sp)
{
    const double T3 = t * t * t, Rp = 4.0 * e * sigma;
    const double Ru = a * G - E;
    sp = 4.0 * Rp * T3 / cp;
    su = Ru - Rp * T3 * (t - 4.0 * he / cp);
}
__global__ void k_radiation_sh_v(long n, const double *a, const double *e, double sigma, const double *__restrict__ E,
                                 const double *__restrict__ G, const double *__restrict__ T, const double *__restrict__ he,
                                 const double *__restrict__ Cp, double CpConst, double *__restrict__ su, double *__restrict__ sp)
{
    GRID_STRIDE(c, n) {
        double u, p;
        radiation_sh_cell(a[c], e[c], sigma, E[c], G[c], T[c], he[c], Cp ? Cp[c] : CpConst, u, p);
        su[c] = u; sp[c] = p;
    }
}
extern "C" int ffm_radiation_sh_v_d(ffm_ctx *ctx, long n, const double *a_d, const double *e_d, double sigma, const double *E_d, const double *G_d,
                                    const double *T_d, const double *he_d, const double *Cp_d, double CpConst, double *su_d, double *sp_d)
{
    if (!ctx || n < 0 || !a_d || !e_d || !E_d || !G_d || !T_d || !he_d || !su_d || !sp_d) return FFM_ERR_ARG;
    if (n == 0) return FFM_OK;
    FFM_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_radiation_sh_v, dim3(sgrid(n)), dim3(256), 0, ctx->stream, n, a_d, e_d, sigma, E_d, G_d, T_d, he_d, Cp_d, CpConst, su_d, sp_d);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}
// The per-step form with greyMeanAbsorptionEmission: a = e of the cell evaluated in registers (greymean_a: ffm_greymean_a_d's
// expression), E = EhrrCoeff*Qdot, then su and sp as above -- bit for bit ffm_greymean_a_d, ffm_greymean_E_d, ffm_radiation_sh_v_d,
// without the write and re-read of a and E and in one launch.  a is written once where asked for.
__global__ __launch_bounds__(256) void k_radiation_sh_greymean(long n, GreyMeanTable t, GreyMeanPtrs y, double sigma, const double *__restrict__ p,
                                                               const double *__restrict__ T, const double *__restrict__ G,
                                                               const double *__restrict__ he, const double *__restrict__ Qdot,
                                                               const double *__restrict__ Cp, double CpConst, double *__restrict__ aOut,
                                                               double *__restrict__ su, double *__restrict__ sp, int *flag)
{
    bool outside = false;
    GRID_STRIDE(c, n) {
        const double tc = T[c];
        const double a = greymean_a(t, y, c, p[c], tc, outside);
        const double E = t.EhrrCoeff * Qdot[c];
        double u, s;
        radiation_sh_cell(a, a, sigma, E, G[c], tc, he[c], Cp ? Cp[c] : CpConst, u, s);
        if (aOut) aOut[c] = a;
        su[c] = u; sp[c] = s;
    }
    if (flag && outside) *flag = 1;
}
extern "C" int ffm_radiation_sh_greymean_d(ffm_greymean *gm, long n, const double *const *Y_d, const double *p_d, const double *T_d, double sigma,
                                           const double *G_d, const double *he_d, const double *Qdot_d, const double *Cp_d, double CpConst,
                                           double *a_out_d, double *su_d, double *sp_d, int *flag_d)
{
    if (!gm || n < 0 || !Y_d || !p_d || !T_d || !G_d || !he_d || !Qdot_d || !su_d || !sp_d) return FFM_ERR_ARG;
    GreyMeanPtrs y; FFM_TRY(greymean_ptrs(gm, Y_d, y));
    if (n == 0) return FFM_OK;
    FFM_HIP(hipSetDevice(gm->ctx->device));
    hipLaunchKernelGGL(k_radiation_sh_greymean, dim3(sgrid(n)), dim3(256), 0, gm->ctx->stream, n, gm->t, y, sigma, p_d, T_d, G_d, he_d, Qdot_d, Cp_d,
                       CpConst, a_out_d, su_d, sp_d, flag_d);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

// fvDOM::updateG, cell part (fvDOM.C:697-718): G = sum Ii omega_i.  The sum of a cell is kept in a register and formed in ray-index
// order from zero, ((0 + I_0 w_0) + I_1 w_1) + ..., which is what nRay passes G = G + I_i*omega_i over a zeroed G leave: every ray is
// read once, G written once.  The ray pointers and omega are the same for all lanes (scalar loads); a lane's loads of a ray are
// adjacent to its neighbours'.  The unroll keeps four rays' loads in flight, the additions stay in order.
__global__ void k_fvdom_G(long n, int nRay, const double *const *__restrict__ I, const double *__restrict__ omega, double *__restrict__ G)
{
    GRID_STRIDE(c, n) {
        double g = 0.0;
#pragma unroll 4
        for (int i = 0; i < nRay; i++) g = g + I[i][c] * omega[i];
        G[c] = g;
    }
}
extern "C" int ffm_fvdom_G_d(ffm_ctx *ctx, long n, int nRay, const double *const *I_dd, const double *omega_d, double *G_d)
{
    if (!ctx || n < 0 || nRay < 1 || !I_dd || !omega_d || !G_d) return FFM_ERR_ARG;
    if (n == 0) return FFM_OK;
    FFM_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_fvdom_G, dim3(sgrid(n)), dim3(256), 0, ctx->stream, n, nRay, I_dd, omega_d, G_d);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}
