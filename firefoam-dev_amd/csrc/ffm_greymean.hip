// ffm_greymean.hip -- greyMeanAbsorptionEmission of the gas phase (reference packages/thermophysicalModels/radiation/submodels/
// absorptionEmissionModel/greyMeanAbsorptionEmission/greyMeanAbsorptionEmission.C:177-314): per cell
//   a = sum over the participating species of Xipi*(((((b5*Ti + b4)*Ti + b3)*Ti + b2)*Ti + b1)*Ti + b0),
//   Xipi = Y_s/(W_s*invWt)*paToAtm(p), invWt = sum Y/W over ALL species, b = T < Tcommon ? loTcoeffs : hiTcoeffs, Ti = invTemp ? 1/T : T,
// e = a, E = EhrrCoeff*Qdot (Qdot per volume).  One streaming pass: (nSpecies + 2) doubles read, one written per cell; no neighbour access.
// Summation order over the participating species: the CALLER'S LIST ORDER.  The reference walks a HashTable<label>, whose order follows
// upstream's string hash; that hash is not in the reference tree, so its order cannot be reproduced here -- unpinned by reference data.
// The lookUpTableFileName branch (species from a mixture-fraction table) is not built.
#include "ffm_greymean.hpp"
#include "ffm_mesh.hpp"

namespace {
__global__ __launch_bounds__(256) void k_greymean_a(long n, GreyMeanTable t, GreyMeanPtrs y, const double *__restrict__ p,
                                                    const double *__restrict__ T, double *__restrict__ a, int *flag)
{
    bool outside = false;
    GRID_STRIDE(i, n) a[i] = greymean_a(t, y, i, p[i], T[i], outside);
    if (flag && outside) *flag = 1;                       // only ever raised: the caller reads it when it next synchronises
}
__global__ void k_greymean_E(long n, double EhrrCoeff, const double *__restrict__ Qdot, double *__restrict__ E)
{
    GRID_STRIDE(i, n) E[i] = EhrrCoeff * Qdot[i];
}
}  // namespace

// W[nSpecies]: the molecular weights of ALL species of the mixture, in the order of Y_d.  The nPart participating species in the
// order their terms are summed: specie[j] (index into the species list, distinct), invTemp[j], Tcommon / Tlow / Thigh[j], the two
// coefficient sets lo / hi [nPart][6] (b0 .. b5).
extern "C" int ffm_greymean_create(ffm_ctx *ctx, int nSpecies, const double *W, int nPart, const int *specie, const int *invTemp,
                                   const double *Tcommon, const double *Tlow, const double *Thigh, const double *lo, const double *hi,
                                   double EhrrCoeff, ffm_greymean **out)
{
    if (!ctx || !out || nSpecies < 1 || nSpecies > GM_MAXSP || nPart < 1 || nPart > GM_MAXPART || !W || !specie || !invTemp || !Tcommon || !Tlow ||
        !Thigh || !lo || !hi) {
        ffm_set_error("ffm_greymean_create: bad argument (at most %d species, 1 to %d participating)", GM_MAXSP, GM_MAXPART); return FFM_ERR_ARG;
    }
    for (int i = 0; i < nSpecies; i++) if (!(W[i] > 0)) { ffm_set_error("ffm_greymean_create: W[%d] is not positive", i); return FFM_ERR_ARG; }
    for (int j = 0; j < nPart; j++) {
        if (specie[j] < 0 || specie[j] >= nSpecies) { ffm_set_error("ffm_greymean_create: specie[%d] = %d is out of range", j, specie[j]); return FFM_ERR_ARG; }
        for (int k = 0; k < j; k++) if (specie[k] == specie[j]) { ffm_set_error("ffm_greymean_create: specie %d is listed twice", specie[j]); return FFM_ERR_ARG; }
    }
    ffm_greymean *gm = new ffm_greymean(); gm->ctx = ctx;
    GreyMeanTable &t = gm->t;
    t.n = nSpecies; t.nPart = nPart; t.EhrrCoeff = EhrrCoeff;
    for (int i = 0; i < nSpecies; i++) t.W[i] = W[i];
    for (int j = 0; j < nPart; j++) {
        t.specie[j] = specie[j]; t.invTemp[j] = invTemp[j] ? 1 : 0; t.Wp[j] = W[specie[j]];
        t.Tcommon[j] = Tcommon[j]; t.Tlow[j] = Tlow[j]; t.Thigh[j] = Thigh[j];
        for (int c = 0; c < 6; c++) { t.lo[j][c] = lo[6 * j + c]; t.hi[j][c] = hi[6 * j + c]; }
    }
    *out = gm;
    return FFM_OK;
}
extern "C" int ffm_greymean_destroy(ffm_greymean *gm) { delete gm; return FFM_OK; }

extern "C" int ffm_greymean_a_d(ffm_greymean *gm, long n, const double *const *Y_d, const double *p_d, const double *T_d, double *a_d, int *flag_d)
{
    if (!gm || n < 0 || !Y_d || !p_d || !T_d || !a_d) return FFM_ERR_ARG;
    GreyMeanPtrs y; FFM_TRY(greymean_ptrs(gm, Y_d, y));
    if (n == 0) return FFM_OK;
    FFM_HIP(hipSetDevice(gm->ctx->device));
    hipLaunchKernelGGL(k_greymean_a, dim3(sgrid(n)), dim3(256), 0, gm->ctx->stream, n, gm->t, y, p_d, T_d, a_d, flag_d);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}

extern "C" int ffm_greymean_E_d(ffm_greymean *gm, long n, const double *Qdot_d, double *E_d)
{
    if (!gm || n < 0 || !Qdot_d || !E_d) return FFM_ERR_ARG;
    if (n == 0) return FFM_OK;
    FFM_HIP(hipSetDevice(gm->ctx->device));
    hipLaunchKernelGGL(k_greymean_E, dim3(sgrid(n)), dim3(256), 0, gm->ctx->stream, n, gm->t.EhrrCoeff, Qdot_d, E_d);
    FFM_HIP(hipGetLastError());
    return FFM_OK;
}
