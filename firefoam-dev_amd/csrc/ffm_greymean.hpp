// ffm_greymean.hpp -- the table and the per-cell evaluation of greyMeanAbsorptionEmission::aCont, shared by the model's own passes
// (ffm_greymean.hip) and the fused enthalpy-source pass (ffm_rad.hip: ffm_radiation_sh_greymean_d), so that both form `a` with the
// same expression and hence the same bits.
#pragma once
#include "ffm_internal.hpp"

constexpr int GM_MAXSP = 8;                 // TH_MAXSP of ffm_thermo.hip: the species a thermo table holds
constexpr int GM_MAXPART = 8;

// Travels by value in the kernel arguments (as ThermoTable does): uniform over the wave, so its loads are scalar.  Per participating
// species j, in the caller's list order: its index in the species list, W of that species (a copy: no runtime index into W), the
// polynomial's temperature range and switch, the two coefficient sets.
struct GreyMeanTable {
    int n, nPart;
    int specie[GM_MAXPART], invTemp[GM_MAXPART];
    double W[GM_MAXSP];
    double Wp[GM_MAXPART], Tcommon[GM_MAXPART], Tlow[GM_MAXPART], Thigh[GM_MAXPART];
    double lo[GM_MAXPART][6], hi[GM_MAXPART][6];
    double EhrrCoeff;
};
struct GreyMeanPtrs { const double *Y[GM_MAXSP]; };

struct ffm_greymean { ffm_ctx *ctx; GreyMeanTable t; };

// upstream OpenFOAM's paToAtm(p) = p/101325.0 (restated from knowledge: the function is not in the reference tree)
#define GM_PA_TO_ATM(p) ((p) / 101325.0)

#ifdef __HIPCC__
// aCont of one cell.  invWt is formed once (the reference recomputes it per species with the same operations: the same bits).  The
// species loops have fixed bounds and are guarded by the uniform counts; the mass fraction of a participating species is picked from
// the registers by uniform selects and the coefficient set by per-coefficient selects, so nothing is indexed at run time and nothing
// goes to scratch.  outside: raised where T leaves [Tlow, Thigh] of a participating species (absorptionCoeffs::checkT only warns).
__device__ __forceinline__ double greymean_a(const GreyMeanTable &t, const GreyMeanPtrs &y, long i, double p, double T, bool &outside)
{
    double Yv[GM_MAXSP];
    double invWt = 0.0;
#pragma unroll
    for (int s = 0; s < GM_MAXSP; s++) {
        Yv[s] = 0.0;
        if (s < t.n) { Yv[s] = y.Y[s][i]; invWt = invWt + Yv[s] / t.W[s]; }
    }
    const double patm = GM_PA_TO_ATM(p), Tinv = 1.0 / T;
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < GM_MAXPART; j++) if (j < t.nPart) {
        const int sp = t.specie[j];
        double Ys = Yv[0];
#pragma unroll
        for (int s = 1; s < GM_MAXSP; s++) Ys = sp == s ? Yv[s] : Ys;
        const double Xk = Ys / (t.Wp[j] * invWt);
        const double Xipi = Xk * patm;
        const bool low = T < t.Tcommon[j];
        const double b0 = low ? t.lo[j][0] : t.hi[j][0], b1 = low ? t.lo[j][1] : t.hi[j][1], b2 = low ? t.lo[j][2] : t.hi[j][2];
        const double b3 = low ? t.lo[j][3] : t.hi[j][3], b4 = low ? t.lo[j][4] : t.hi[j][4], b5 = low ? t.lo[j][5] : t.hi[j][5];
        const double Ti = t.invTemp[j] ? Tinv : T;
        a = a + Xipi * (((((b5 * Ti + b4) * Ti + b3) * Ti + b2) * Ti + b1) * Ti + b0);
        outside = outside || T < t.Tlow[j] || T > t.Thigh[j];
    }
    return a;
}
#endif

// Y_d (a host array of nSpecies device pointers) into the kernel-argument form; FFM_ERR_ARG on a NULL entry
static inline int greymean_ptrs(const ffm_greymean *gm, const double *const *Y, GreyMeanPtrs &y)
{
    for (int i = 0; i < GM_MAXSP; i++) y.Y[i] = nullptr;
    for (int i = 0; i < gm->t.n; i++) { if (!Y[i]) return FFM_ERR_ARG; y.Y[i] = Y[i]; }
    return FFM_OK;
}
