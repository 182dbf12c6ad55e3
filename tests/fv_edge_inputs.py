"""Designed inputs (test infrastructure) of the edge tests of the limited convection schemes -- limitedLinear k / limitedLinear01 k in
their five device copies (k_limited_weights and k_weights_from_limiter of csrc/ffm_fv.hip; limited_weight() in k_scalar_eqns and
k_div_phiK, mv_limiter() in k_mv_weights and k_mv_tile of csrc/ffm_fused.hip) and filteredLinear2V -- shared by
tests/test_fv_edge_inputs_cpu.py, which checks on the oracle alone that the design is exact and that every class of face is reached,
and by tests/test_fv_limiter_edges_gpu.py, which runs the same inputs through the kernels and compares the bits.  Only tests/ may
import this module.

Everything is dyadic, so that every operation before the division of NVDTVD::r is exact: meshes of spacing h = 1/8 (cell centres
are multiples of 1/16, also the bars' of tests/merged_mesh.py), cell values from a palette of multiples of 2^-6 that holds lo, hi, values
below lo and values above hi of both bound sets, gradient components from a palette of small dyadic numbers and of +-1998, +-2000
(with |d| = 1/8 and gradf = +-1/4: gradcf/gradf of 1/2, 9/16, 5/8, 3/4, 1, 3/2 -- the limiter's 0, blend and 1 at k = 1/2, 1, 2 -- the
exact tie |gradcf| = 1000 |gradf| and 999 |gradf| just below it), fluxes from {+0, -0, +-1/4, +-2^-1074}.  A value depends on the cell's
centre (a face's on its two cells'), not on its number: the classes reached do not change when the library renumbers the mesh.

restate() is the reference's C++ with one numpy ufunc per IEEE operation (limitedSurfaceInterpolationScheme::limiter / weights, NVDTVD::r,
limitedLinearLimiter, LimitedLimiter: oracle/fv.py limited_limiter cites them); exact() is the same in fractions.Fraction from the same
doubles.  Both label every face with the classes of CLASSES below."""
from fractions import Fraction

import numpy as np

import merged_mesh as MM

H = 0.125
MESHES = ["hex", "w8", "w16u14", "w32l30", "w32multi", "w32u18"]
BUCKET = {"hex": 3, "w8": 8, "w16u14": 16, "w32l30": 32, "w32multi": 32, "w32u18": 32}
HEX_N = (7, 6, 5)
# (k, lo, hi); k = 0: twoByk = 2/1e-15, every non-negative r gives the linear weights
PARAMS = [(1.0, 0.0, 1.0), (0.5, 0.0, 1.0), (2.0, 0.25, 0.75), (0.0, 0.0, 1.0)]
NF = 6
MV_SCHEMES = [2, 3, 3, 3, 2, 3]                        # mixed member schemes of the common limiter; the first nf of them
SCHEME_NAME = {2: "limitedLinear", 3: "limitedLinear01"}

VALUES = np.array([-16, 0, 16, 32, 48, 64, 80]) / 64.0                          # multiples of 2^-6: -1/4 .. 5/4
_G = [0.5, 1.0, 1.125, 1.25, 1.5, 2.0, 3.0, 1998.0, 2000.0, 2000.0]
GRADS = np.array([0.0, 0.0] + _G + [-g for g in _G])
DENORM = float(np.nextafter(0.0, 1.0))                                           # 2^-1074
FLUXES = np.array([0.0, -0.0, 0.25, -0.25, DENORM, -DENORM])
# fields 1 .. 5 are flat (one value, zero gradient) outside a part of the mesh: uniform regions next to steep ones, and a common limiter
# that is not 0 nearly everywhere; the flat values lie inside every [lo, hi] of PARAMS
ACTIVE = [1.0, 0.5, 0.35, 0.25, 0.2, 0.15]
FLAT = [0.5, 0.25, 0.75, 0.5, 0.25, 0.5]
# one seed per mesh, found by a search over 0, 1, 2 ... for the first at which every class of CLASSES is reached for every PARAMS
SEEDS = {"hex": 21, "w8": 4, "w16u14": 4, "w32l30": 3, "w32multi": 3, "w32u18": 0}

FLUX_CLASSES = ["+0", "-0", ">0", "<0", "+denormal", "-denormal"]
RATIO_CLASSES = ["uniform", "gradf0 gradcf>0", "gradf0 gradcf<0", "tie++", "tie+-", "tie-+", "tie--", "below tie"]
LIMITER_CLASSES = ["t<0", "t==0", "0<t<1", "t==1", "t>1"]
BOUND_CLASSES = ["flux>0 P==lo", "flux>0 P<lo", "flux>0 N==hi", "flux>0 N>hi", "flux<0 N==lo", "flux<0 N<lo", "flux<0 P==hi", "flux<0 P>hi",
                 "flux0 out of bounds"]
MV_CLASSES = ["mv 1", "mv blend", "mv 0 by one field"]
CLASSES = FLUX_CLASSES + RATIO_CLASSES + LIMITER_CLASSES + BOUND_CLASSES + MV_CLASSES


def host_mesh(name):
    from oracle import plume
    return plume.make_mesh(HEX_N, h=H) if name == "hex" else MM.case(name, h=H)


def required(k):
    """the classes every mesh must reach at this k.  At k = 0 twoByk is 2e15 and r = 2 gradcf/gradf - 1 a ratio of integers below
    2^20: t = twoByk r is 0 or beyond 1e9 in magnitude -- no face can have t in (0, 1] there, whatever the inputs"""
    out = [c for c in CLASSES if not (k == 0.0 and c in ("0<t<1", "t==1", "mv blend"))]
    return out


# ------------------------------------------------------------------------------------------------------------------ the inputs
def _mix(x):
    """splitmix64's finaliser on uint64 arrays"""
    x = np.asarray(x, np.uint64)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _pick(key, stream, n):
    return (_mix(key + np.uint64(0x9E3779B97F4A7C15 * (stream + 1) % 2 ** 64)) % np.uint64(n)).astype(np.int64)


def cell_keys(mesh, seed):
    """one 64-bit key per cell from its centre (multiples of 1/32 on these meshes): the same cell has the same key in every numbering"""
    q = np.rint(mesh.C * 32.0).astype(np.int64)
    assert np.array_equal(q / 32.0, mesh.C), "cell centres are no multiples of 1/32"
    k = (q[:, 0] + 4096 * (q[:, 1] + 4096 * q[:, 2])).astype(np.uint64)
    k = _mix(k + np.uint64(0xD1B54A32D192ED03 * (seed + 1) % 2 ** 64))
    assert len(np.unique(k)) == mesh.nCells
    return k


def face_keys(mesh, ck):
    return _mix(_mix(ck[mesh.l]) + ck[mesh.u])


def fields(mesh, name, nf=NF):
    """phi[F], vf[nf][N], grad[nf][N][3] of the mesh `name` (in any numbering)"""
    seed = SEEDS[name]
    ck = cell_keys(mesh, seed)
    phi = FLUXES[_pick(face_keys(mesh, ck), 0, len(FLUXES))]
    vf = np.empty((nf, mesh.nCells)); grad = np.empty((nf, mesh.nCells, 3))
    for i in range(nf):
        s = 10 * (i + 1)
        active = _pick(ck, s, 1000) < int(1000 * ACTIVE[i])
        vf[i] = np.where(active, VALUES[_pick(ck, s + 1, len(VALUES))], FLAT[i])
        for d in range(3):
            grad[i, :, d] = np.where(active, GRADS[_pick(ck, s + 2 + d, len(GRADS))], 0.0)
    return dict(phi=phi, vf=vf, grad=grad)


def dyadic_face_field(mesh, name, stream, palette):
    """a face field from a palette, by the faces' keys"""
    ck = cell_keys(mesh, SEEDS[name])
    palette = np.asarray(palette, float)
    return palette[_pick(face_keys(mesh, ck), stream, len(palette))]


# --------------------------------------------------------------------------------------------- the restatement and its exact twin
def _classes(phi, gradf, gradcf, t, P, Nn, lo, hi):
    """the class masks of every face; abs and the comparisons work on float64 arrays and on object arrays of Fractions alike"""
    b = lambda a: np.asarray(a).astype(bool)
    ag, ac = np.abs(gradf), np.abs(gradcf)
    c = {}
    c["uniform"] = b(gradf == 0) & b(gradcf == 0)
    c["gradf0 gradcf>0"] = b(gradf == 0) & b(gradcf > 0)
    c["gradf0 gradcf<0"] = b(gradf == 0) & b(gradcf < 0)
    tie = b(ac == 1000 * ag) & b(gradf != 0)
    for sc, mc in (("+", b(gradcf > 0)), ("-", b(gradcf < 0))):
        for sf, mf in (("+", b(gradf > 0)), ("-", b(gradf < 0))):
            c["tie" + sc + sf] = tie & mc & mf
    c["below tie"] = b(ac >= 999 * ag) & b(ac < 1000 * ag)
    c["t<0"], c["t==0"], c["0<t<1"], c["t==1"], c["t>1"] = b(t < 0), b(t == 0), b(t > 0) & b(t < 1), b(t == 1), b(t > 1)
    # the bound test of limitedLinear01 decides the face: the limiter without it is positive, and only the named comparison can fire
    pos, fp, fn = b(t > 0), phi > 0, phi < 0
    c["flux>0 P==lo"] = pos & fp & b(P == lo) & b(Nn <= hi)
    c["flux>0 P<lo"] = pos & fp & b(P < lo) & b(Nn <= hi)
    c["flux>0 N==hi"] = pos & fp & b(Nn == hi) & b(P >= lo)
    c["flux>0 N>hi"] = pos & fp & b(Nn > hi) & b(P >= lo)
    c["flux<0 N==lo"] = pos & fn & b(Nn == lo) & b(P <= hi)
    c["flux<0 N<lo"] = pos & fn & b(Nn < lo) & b(P <= hi)
    c["flux<0 P==hi"] = pos & fn & b(P == hi) & b(Nn >= lo)
    c["flux<0 P>hi"] = pos & fn & b(P > hi) & b(Nn >= lo)
    c["flux0 out of bounds"] = pos & (phi == 0) & (b(P < lo) | b(P > hi) | b(Nn < lo) | b(Nn > hi))
    return c


def flux_classes(phi):
    sb, den = np.signbit(phi), np.abs(phi) == DENORM
    return {"+0": (phi == 0) & ~sb, "-0": (phi == 0) & sb, ">0": (phi > 0) & ~den, "<0": (phi < 0) & ~den,
            "+denormal": den & ~sb, "-denormal": den & sb}


def two_by_k(k):
    return 2.0 / max(k, 1e-15)


def restate_parts(mesh, scheme, phi, vf, grad, k, bounds):
    """limitedSurfaceInterpolationScheme::limiter and ::weights for limitedLinear k (scheme 2 / "limitedLinear") and limitedLinear01 k
    (3 / "limitedLinear01"), one ufunc per operation of the C++:
        gradf = phiN - phiP;  gradcf = d & (faceFlux > 0 ? gradcP : gradcN)                        NVDTVD::r
        r = |gradcf| >= 1000 |gradf| ? 2*1000*sign(gradcf)*sign(gradf) - 1 : 2*(gradcf/gradf) - 1      sign(s) = s >= 0 ? 1 : -1
        limiter = max(min(twoByk*r, 1), 0)                                                             limitedLinearLimiter
        limiter = 0 where (faceFlux > 0 and (phiP < lo or phiN > hi)) or (faceFlux < 0 and (phiN < lo or phiP > hi))    LimitedLimiter
        weight = limiter*w_linear + (1 - limiter)*pos0(faceFlux)
    Returns a dict with every intermediate and the class masks."""
    scheme = SCHEME_NAME.get(scheme, scheme)
    l, u = mesh.l, mesh.u
    lo, hi = bounds
    P, Nn = vf[l], vf[u]
    d = [np.subtract(mesh.C[u, j], mesh.C[l, j]) for j in range(3)]
    gradf = np.subtract(Nn, P)
    up = np.where(np.greater(phi, 0.0), l, u)
    g = [grad[up, j] for j in range(3)]
    gradcf = np.add(np.add(np.multiply(d[0], g[0]), np.multiply(d[1], g[1])), np.multiply(d[2], g[2]))
    big = np.greater_equal(np.abs(gradcf), np.multiply(1000.0, np.abs(gradf)))
    sa = np.where(np.greater_equal(gradcf, 0.0), 1.0, -1.0)
    sb = np.where(np.greater_equal(gradf, 0.0), 1.0, -1.0)
    rbig = np.subtract(np.multiply(np.multiply(2.0 * 1000.0, sa), sb), 1.0)
    rsmall = np.subtract(np.multiply(2.0, np.divide(gradcf, np.where(big, 1.0, gradf))), 1.0)
    r = np.where(big, rbig, rsmall)
    twoByk = two_by_k(k)
    t = np.multiply(twoByk, r)
    lim = np.maximum(np.minimum(t, 1.0), 0.0)
    if scheme == "limitedLinear01":
        off = (np.greater(phi, 0.0) & (np.less(P, lo) | np.greater(Nn, hi))) | (np.less(phi, 0.0) & (np.less(Nn, lo) | np.greater(P, hi)))
        lim = np.where(off, 0.0, lim)
    elif scheme != "limitedLinear":
        raise ValueError(scheme)
    p0 = np.where(np.greater_equal(phi, 0.0), 1.0, 0.0)
    w = np.add(np.multiply(lim, mesh.weights), np.multiply(np.subtract(1.0, lim), p0))
    return dict(lim=lim, w=w, gradf=gradf, gradcf=gradcf, big=big, r=r, t=t, q=np.divide(gradcf, np.where(big, 1.0, gradf)),
                classes=_classes(phi, gradf, gradcf, t, P, Nn, lo, hi))


def restate(mesh, scheme, phi, vf, grad, k, bounds):
    """(limiter, weights) of restate_parts"""
    p = restate_parts(mesh, scheme, phi, vf, grad, k, bounds)
    return p["lim"], p["w"]


def weights_from_limiter(mesh, phi, lim):
    p0 = np.where(np.greater_equal(phi, 0.0), 1.0, 0.0)
    return np.add(np.multiply(lim, mesh.weights), np.multiply(np.subtract(1.0, lim), p0))


def common_limiter(mesh, schemes, phi, vf, grad, k, bounds):
    """multivariateSelectionScheme: the face-wise minimum of the member schemes' limiters, and every member's own"""
    lims = np.array([restate(mesh, s, phi, vf[i], grad[i], k, bounds)[0] for i, s in enumerate(schemes)])
    return lims.min(axis=0), lims


def mv_classes(lims):
    common = lims.min(axis=0)
    return {"mv 1": common == 1.0, "mv blend": (common > 0.0) & (common < 1.0),
            "mv 0 by one field": (common == 0.0) & ((lims == 0.0).sum(axis=0) == 1)}


def frac(a):
    out = np.empty(np.shape(a), object)
    out.ravel()[:] = [Fraction(float(x)) for x in np.ravel(a)]
    return out


def exact(mesh, scheme, phi, vf, grad, k, bounds):
    """restate_parts in fractions.Fraction from the doubles as given (the mesh's centres and weights, the fields, lo, hi; twoByk is the
    double 2.0/max(k, 1e-15)): the exact limiter and weight of every face, gradf, gradcf, and the class masks"""
    scheme = SCHEME_NAME.get(scheme, scheme)
    l, u = mesh.l, mesh.u
    lo, hi = Fraction(float(bounds[0])), Fraction(float(bounds[1]))
    V, G, C = frac(vf), frac(grad), frac(mesh.C)
    P, Nn = V[l], V[u]
    d = C[u] - C[l]
    gradf = Nn - P
    up = np.where(phi > 0, l, u)
    gradcf = (d[:, 0] * G[up, 0] + d[:, 1] * G[up, 1]) + d[:, 2] * G[up, 2]
    b = lambda a: np.asarray(a).astype(bool)
    big = b(np.abs(gradcf) >= 1000 * np.abs(gradf))
    sa = np.where(b(gradcf >= 0), Fraction(1), Fraction(-1)); sb = np.where(b(gradf >= 0), Fraction(1), Fraction(-1))
    q = gradcf / np.where(big, Fraction(1), gradf)
    r = np.where(big, 2000 * sa * sb - 1, 2 * q - 1)
    t = Fraction(two_by_k(k)) * r
    one, zero = Fraction(1), Fraction(0)
    lim = np.where(b(t > one), one, np.where(b(t < zero), zero, t))
    if scheme == "limitedLinear01":
        off = ((phi > 0) & (b(P < lo) | b(Nn > hi))) | ((phi < 0) & (b(Nn < lo) | b(P > hi)))
        lim = np.where(off, zero, lim)
    elif scheme != "limitedLinear":
        raise ValueError(scheme)
    p0 = np.where(phi >= 0, one, zero)
    w = lim * frac(mesh.weights) + (1 - lim) * p0
    return dict(lim=lim, w=w, gradf=gradf, gradcf=gradcf, big=big, r=r, t=t, q=q,
                classes=_classes(phi, gradf, gradcf, t, P, Nn, lo, hi))


def class_counts(mesh, name, k, lo, hi, parts=restate_parts):
    """how many (face, field) pairs of fields(mesh, name) fall in every class of CLASSES for one parameter set: the flux classes over
    the faces, the ratio and limiter classes over the six fields, the bound classes over the six fields under limitedLinear01, the
    multivariate classes over the faces for the first two and all six of MV_SCHEMES (the smaller count)"""
    f = fields(mesh, name)
    cnt = {c: int(m.sum()) for c, m in flux_classes(f["phi"]).items()}
    lims = []
    for i in range(NF):
        p = parts(mesh, 3, f["phi"], f["vf"][i], f["grad"][i], k, (lo, hi))
        for c in RATIO_CLASSES + LIMITER_CLASSES + BOUND_CLASSES:
            cnt[c] = cnt.get(c, 0) + int(p["classes"][c].sum())
        lims.append(p["lim"] if MV_SCHEMES[i] == 3 else parts(mesh, 2, f["phi"], f["vf"][i], f["grad"][i], k, (lo, hi))["lim"])
    lims = np.array(lims, dtype=float)
    two, six = mv_classes(lims[:2]), mv_classes(lims)
    for c in MV_CLASSES:
        cnt[c] = min(int(two[c].sum()), int(six[c].sum()))
    return cnt


# ------------------------------------------------------------------------------------------------------- filteredLinear2V k l
# (k, l): dyadic, so that l + 1 - k*x/den can land on 0 and on 1 exactly, and the case's own (cases/wallFireSpread2D/system/fvSchemes:41)
FL2V_PARAMS = [(0.25, 0.0625), (0.2, 0.05)]
FL2V_U = np.array([0.0, 0.0, 0.25, 0.5, -0.25, 1.0])
FL2V_G = np.array([0.0, 0.0, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0, 0.5, 8.0])
FL2V_CLASSES = ["df==0", "df==tcP", "df==tcN", "tcP>0", "tcP<0", "tcN>0", "tcN<0", "limiter==1 unclamped", "limiter==0 unclamped",
                "limiter blend", "phi +0", "phi -0"]


def fl2v_fields(mesh, name):
    """phi[F], U[N][3], gradU[N][3][3] (gradU[c][i][j] = d_i U_j): palettes by the cells' keys, a third of the cells uniform (U = 0,
    gradU = 0), and two planted x-faces between unit cells where, at (k, l) = (1/4, 1/16), the unclamped limiter is exactly 1 and exactly 0:
        U_N - U_P = (2, 0, 0), d & gradU_P = (-4, 0, 0), gradU_N = 0:  df = 4,  tcP = -16, tcN = 0:  17/16 - (1/4) 4/16 = 1
        U_N - U_P = (8, 2, 0), d & gradU_P = (-1, 0, 0), gradU_N = 0:  df = 68, tcP = -16, tcN = 0:  17/16 - (1/4) 68/16 = 0
    (|tc| = 16: the SMALL = 1e-15 of the denominator is below half a unit in the last place of 16 and vanishes in the sum)"""
    ck = cell_keys(mesh, SEEDS[name])
    fk = face_keys(mesh, ck)
    phi = FLUXES[_pick(fk, 0, len(FLUXES))]
    N = mesh.nCells
    live = _pick(ck, 100, 3) > 0
    U = np.zeros((N, 3)); g = np.zeros((N, 3, 3))
    for j in range(3):
        U[:, j] = np.where(live, FL2V_U[_pick(ck, 101 + j, len(FL2V_U))], 0.0)
        for i in range(3):
            g[:, i, j] = np.where(live, FL2V_G[_pick(ck, 110 + 3 * i + j, len(FL2V_G))], 0.0)
    d = mesh.C[mesh.u] - mesh.C[mesh.l]
    xf = np.nonzero((d[:, 0] == H) & (d[:, 1] == 0.0) & (d[:, 2] == 0.0))[0]
    xf = xf[np.argsort(fk[xf])]
    used, planted = set(), []
    for dU, gx in (((2.0, 0.0, 0.0), -32.0), ((8.0, 2.0, 0.0), -8.0)):
        f = next(int(f) for f in xf if mesh.l[f] not in used and mesh.u[f] not in used)
        P, Nn = mesh.l[f], mesh.u[f]
        used |= {P, Nn}
        U[P] = 0.0; U[Nn] = dU
        g[P] = 0.0; g[Nn] = 0.0; g[P, 0, 0] = gx
        planted.append(f)
    return dict(phi=phi, U=U, gradU=g, planted=planted)


def fl2v_parts(mesh, phi, U, gradU, k, l):
    """oracle.fv.filtered_linear2V_weights with its intermediates (the same expressions in the same order) and the class masks"""
    SMALL = 1.0e-15
    l1 = l + 1.0
    gV = U[mesh.u] - U[mesh.l]
    df = (gV[:, 0] * gV[:, 0] + gV[:, 1] * gV[:, 1]) + gV[:, 2] * gV[:, 2]
    d = mesh.C[mesh.u] - mesh.C[mesh.l]

    def tc(g):
        dg = [(d[:, 0] * g[:, 0, j] + d[:, 1] * g[:, 1, j]) + d[:, 2] * g[:, 2, j] for j in range(3)]
        return 2.0 * ((gV[:, 0] * dg[0] + gV[:, 1] * dg[1]) + gV[:, 2] * dg[2])
    tcP, tcN = tc(gradU[mesh.l]), tc(gradU[mesh.u])
    den = np.maximum(np.abs(tcP), np.abs(tcN)) + SMALL
    x = np.where(df > 0, np.minimum(np.maximum(df - tcP, 0.0), np.maximum(df - tcN, 0.0)),
                 np.minimum(np.maximum(tcP - df, 0.0), np.maximum(tcN - df, 0.0)))
    raw = l1 - k * x / den
    lim = np.maximum(np.minimum(raw, 1.0), 0.0)
    w = lim * mesh.weights + (1.0 - lim) * np.where(phi >= 0, 1.0, 0.0)
    sb = np.signbit(phi)
    c = {"df==0": df == 0, "df==tcP": (df > 0) & (df == tcP), "df==tcN": (df > 0) & (df == tcN), "tcP>0": tcP > 0, "tcP<0": tcP < 0,
         "tcN>0": tcN > 0, "tcN<0": tcN < 0, "limiter==1 unclamped": (x > 0) & (raw == 1.0), "limiter==0 unclamped": (x > 0) & (raw == 0.0),
         "limiter blend": (raw > 0.0) & (raw < 1.0), "phi +0": (phi == 0) & ~sb, "phi -0": (phi == 0) & sb}
    return dict(w=w, lim=lim, raw=raw, df=df, tcP=tcP, tcN=tcN, classes=c)


# ----------------------------------------------------------------------------------------- the tiled multivariate weights' fields
# boxes of tests/test_fused_gpu.py::test_tiled_multivariate_weights_equal_the_two_pass_form with the number of fields of each
TILED_BOXES = [((40, 36, 33), 6), ((24, 40, 20), 3), ((50, 34, 34), 6)]
# cell values in units of delta = 2^-6.  The tiled kernel forms its own Gauss gradients: on a box of spacing 1/8 the upwind cell's
# d & grad is (v[i+1] - v[i-1])/2 along the face's axis, so 1-D stencils (a, b, c) of three consecutive cells make the classes:
# (-1999, 0, 1), (1999, 0, -1), (-1999, 2, 1), (2001, 0, 1): the exact tie with the four sign pairs; (-1997, 0, 1): 999 |gradf|, just below;
# (0, 1, 9), (0, 1, 5), (0, 1, 3), (0, 1, 2): gradcf/gradf = 9/16, 5/8, 3/4, 1; (b, b, c): 1/2, r = 0
TILED_UNITS = np.array([-1999, 1999, 2001, -1997, 0, 0, 1, 1, 2, 3, 5, 9, -16, 16, 32, 48, 64, 80])
TILED_SEED = 7


def tiled_fields(mesh, nf):
    """phi[F], vf[nf][N], vb[nf][patch][faces]: vf from TILED_UNITS*2^-6 by the cells' keys on a part of the box (all of it for field 0),
    flat elsewhere; zero and signed-zero flux planes (the faces of two x-planes and one z-plane) among fluxes of FLUXES"""
    ck = cell_keys(mesh, TILED_SEED)
    phi = FLUXES[_pick(face_keys(mesh, ck), 0, len(FLUXES))]
    i, j, k = mesh.ijk
    phi = np.where((mesh.fdir == 0) & (i[mesh.l] == 3), 0.0, phi)
    phi = np.where((mesh.fdir == 0) & (i[mesh.l] == 11), -0.0, phi)
    phi = np.where((mesh.fdir == 2) & (k[mesh.l] == 5), np.where(j[mesh.l] % 2 == 0, 0.0, -0.0), phi)
    vf = np.empty((nf, mesh.nCells)); vb = []
    for f in range(nf):
        s = 10 * (f + 1)
        active = _pick(ck, s, 1000) < int(1000 * ACTIVE[f])
        vf[f] = np.where(active, TILED_UNITS[_pick(ck, s + 1, len(TILED_UNITS))] / 64.0, FLAT[f])
        vb.append([np.where(active[p.faceCells], VALUES[_pick(ck[p.faceCells], s + 2 + q, len(VALUES))], FLAT[f]) for q, p in enumerate(mesh.patches)])
    return dict(phi=phi, vf=vf, vb=vb)


def grad_exact_int(mesh, vf, vb):
    """64 * V * fvc::grad in exact integer arithmetic on a hex box of spacing 1/8 with values that are multiples of 2^-6:
    V grad = sum Sf (P + N)/2, Sf = +-2^-6 along the face's axis; in units: 2^13 V grad_d = sum +-(P + N)*64 (boundary: 2 * value * 64)"""
    q = lambda a: np.rint(np.asarray(a) * 64.0).astype(np.int64)
    v = q(vf)
    out = np.zeros((mesh.nCells, 3), np.int64)
    for d in range(3):
        sel = mesh.fdir == d
        s = v[mesh.l[sel]] + v[mesh.u[sel]]
        np.add.at(out[:, d], mesh.l[sel], s)
        np.subtract.at(out[:, d], mesh.u[sel], s)
    for p, b in zip(mesh.patches, vb):
        for d in range(3):
            np.add.at(out[:, d], p.faceCells, np.rint(np.sign(p.Sf[:, d])).astype(np.int64) * 2 * q(b))
    return out                                              # grad = out / (2 * 64 * h)  = out / 16


def boundary_field(mesh, name, stream, palette):
    """one array per patch from a palette, by the key of the face's cell"""
    ck = cell_keys(mesh, SEEDS[name])
    palette = np.asarray(palette, float)
    return [palette[_pick(ck[p.faceCells], stream + q, len(palette))] for q, p in enumerate(mesh.patches)]


# ------------------------------------------------------------------------------------------ one block with ghost cells
def ghost_block(m):
    """the last z-plane of the hex box as the ghost cells of the rest: (nOwn, nGhost, keep) with keep the faces of the block (owner
    owned; the faces among ghost cells are none of its faces) and cut the faces between an owned cell and a ghost cell"""
    nx, ny, nz = m.n
    nOwn = nx * ny * (nz - 1)
    keep = m.l < nOwn
    return nOwn, m.nCells - nOwn, keep, keep & (m.u >= nOwn)
