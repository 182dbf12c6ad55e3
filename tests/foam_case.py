"""The inputs of examples/b1_demo.C's b1_demo (one rhoEqn / YiEqn / UEqn / pEqn pass written against include/ffmFoam.H) on a
plume mesh, and a runner that executes it on the whole mesh or on ONE RANK's sub-domain of a decomposition (ghost-cell form:
firefoam-dev_amd/decompose.py SubDomain) -- shared by tests/test_foam_layer_decomposed_gpu.py and its worker.  The same for
b1_fvdom (the fvDOM handle) and for b1_physics (the thermo, LES, EDC and P1 handles, the burner's patch conditions and the
reductions: tests/test_foam_handles_decomposed_gpu.py)."""
import ctypes as C
import os

import numpy as np


def inputs(O, m):
    from oracle import fv
    N, F = m.nCells, m.nFaces
    hu = lambda seed, n: O.hash_u(seed, np.arange(n))
    pl = lambda seed, scale=1.0, shift=0.0: [shift + scale * hu(seed + q, p.size) for q, p in enumerate(m.patches)]
    I = dict(dt=2e-3, alphaY=0.8, mu=1.8e-5, pRef=101325.0)
    I["rho_old"] = 1.0 + 0.2 * hu(1, N); I["rho_now"] = I["rho_old"] * (1 + 0.01 * (hu(2, N) - 0.5))
    I["phi"] = 0.02 * (hu(3, F) - 0.5); I["phib"] = pl(10, 0.02, -0.01)
    I["Yi0"] = 0.1 + 0.8 * hu(4, N); I["dEff"] = 2e-5 * (1 + hu(5, N)); I["R"] = 0.5 * (hu(6, N) - 0.5)
    I["U0"] = np.stack([hu(20 + d, N) - 0.5 for d in range(3)])
    I["p_rgh"] = 10.0 * (hu(7, N) - 0.5); I["ghf"] = -9.81 * m.Cf[:, 1]; I["ghfb"] = [-9.81 * p.Cf[:, 1] for p in m.patches]
    bcY = fv.MixedBC(m, f=pl(30), ref=pl(40, 0.5), refGrad=pl(50, 0.1, -0.05))
    bcU = [fv.MixedBC(m, f=pl(60 + 10 * d), ref=pl(90 + 10 * d, 1.0, -0.5)) for d in range(3)]
    I["p_b"] = pl(120, 10.0, -5.0)
    I["psi_now"] = 1.17e-5 * (0.9 + 0.2 * hu(130, N)); I["psi_old"] = I["psi_now"] * (1 + 1e-3 * (hu(131, N) - 0.5))
    I["gh"] = -9.81 * m.C[:, 1]
    I["fluxMask"] = [np.full(p.size, 0.0 if p.name == "top" else 1.0) for p in m.patches]
    I["UfixMask"] = [np.full(p.size, 1.0 if p.name in ("inlet", "floor") else 0.0) for p in m.patches]
    for d in range(3):
        for q, p in enumerate(m.patches):
            if p.name in ("inlet", "floor"):
                bcU[d].f[q] = np.ones(p.size)
    bcP = fv.MixedBC(m, f=[np.full(p.size, 1.0 if p.name == "top" else 0.0) for p in m.patches], ref=pl(140, 2.0, -1.0))
    I["bcY"] = [bcY.f, bcY.ref, bcY.refGrad]
    I["bcU"] = [x for d in range(3) for x in (bcU[d].f, bcU[d].ref, bcU[d].refGrad)]
    I["bcP"] = [bcP.f, bcP.ref, bcP.refGrad]
    return I


class _Domain:
    """the whole mesh (sub None) or one rank's sub-domain `sub` of the decomposition `part` (cell -> rank) on the device:
    renumbering, flipped faces, the owned share of every patch, the ghost exchange with the global cell count; and the maps from
    the caller's cell, face and boundary orders to the device's"""

    def __init__(self, ffm, ctx, m, sub=None, part=None):
        N, F = m.nCells, m.nFaces
        if sub is None:
            gcell = np.arange(N); nOwn, nGhost = N, 0
            l, u, gface, sign = m.l, m.u, np.arange(F), np.ones(F)
            pmask = [np.ones(p.size, bool) for p in m.patches]
            g2l = np.arange(N)
        else:
            gcell, nOwn, nGhost = sub.gcell, sub.nOwned, sub.nGhost
            l, u, gface = sub.l, sub.u, sub.gface
            sign = np.where(sub.flip.astype(bool), -1.0, 1.0)
            pmask = [part[p.faceCells] == sub.rank for p in m.patches]
            g2l = np.full(N, -1, np.int64); g2l[gcell[:nOwn]] = np.arange(nOwn)
        nLoc = nOwn + nGhost
        cOrd, fOrd = ffm.renumber_levels(nOwn, l, u, nGhost=nGhost)
        l2, u2, oldToNew = ffm.hexmesh.apply_renumbering(nLoc, l, u, cOrd, fOrd)
        self.A = ffm.lduMatrix(ctx, nOwn, l2, u2, nGhost=nGhost)
        if sub is not None:
            self.A.set_ghost_exchange(sub.nbrRank, sub.sendCount, oldToNew[sub.sendCells], sub.recvCount, tags=sub.tags, globalCells=N)
        wgt = np.where(sign < 0, 1.0 - m.weights[gface], m.weights[gface])
        patches = [(oldToNew[g2l[p.faceCells[k]]].astype(np.int32), p.Sf[k].T.copy(), p.deltaCoeffs[k]) for p, k in zip(m.patches, pmask)]
        self.mesh = ffm.fvMesh(self.A, m.V[gcell][cOrd], m.C[gcell][cOrd].T.copy(), (m.Sf[gface] * sign[:, None])[fOrd].T.copy(), m.magSf[gface][fOrd],
                               wgt[fOrd], m.deltaCoeffs[gface][fOrd], patches)
        self.mesh.set_face_centres(m.Cf[gface][fOrd].T.copy())
        self.nOwn, self.nLoc, self.B, self.cOrd = nOwn, nLoc, sum(int(k.sum()) for k in pmask), cOrd
        self.nFaces, self.pmask = len(l), pmask
        self.owned = gcell[:nOwn].copy()
        off = np.cumsum([0] + [p.size for p in m.patches])
        self.bpos = np.concatenate([off[q] + np.nonzero(k)[0] for q, k in enumerate(pmask)])        # positions in the patches-concatenated global list
        h = lambda a: np.ascontiguousarray(a, np.float64)
        self.cell = lambda a: h(np.asarray(a)[..., gcell][..., cOrd])
        self.face = lambda a, s=None: h((np.asarray(a)[gface] * (sign if s else 1.0))[fOrd])
        self.bnd = lambda a: h(np.asarray(a)[..., self.bpos]) if self.B else np.zeros(np.asarray(a).shape[:-1] + (1,))

    def owned_cells(self, a):
        """a device-ordered cell array [..., nLoc] -> the owned cells in the sub-domain's order (self.owned: their global labels)"""
        o = np.empty_like(a); o[..., self.cOrd] = a
        return o[..., :self.nOwn].copy()

    def close(self):
        self.mesh.close(); self.A.close()


def run_b1_demo(ffm, ctx, m, I, sub=None, part=None):
    """sub None: the whole mesh on this context.  Otherwise: the sub-domain `sub` of the decomposition `part` (cell -> rank).
    Returns {field: values on the OWNED cells}, the owned cells' global labels and the iteration counts."""
    D = _Domain(ffm, ctx, m, sub, part)
    A, mesh, nLoc, nOwn, B, cOrd, cell, face = D.A, D.mesh, D.nLoc, D.nOwn, D.B, D.cOrd, D.cell, D.face
    bnd = lambda lst: D.bnd(np.concatenate(lst))
    lib = C.CDLL(os.path.join(os.path.dirname(ffm.libpath()), "libffm_b1demo.so"))
    dp = C.POINTER(C.c_double)
    h = lambda a: np.ascontiguousarray(a, np.float64)
    keep = []

    def P(a):
        keep.append(a)
        return a.ctypes.data_as(dp)

    def PP(arrs):
        arrs = [h(a) for a in arrs]; keep.append(arrs)
        arr = (dp * len(arrs))(*[a.ctypes.data_as(dp) for a in arrs]); keep.append(arr)
        return arr
    Fl = D.nFaces
    out = dict(rho=np.empty(nLoc), Yi=np.empty(nLoc), U=np.empty((3, nLoc)), K=np.empty(nLoc), rAU=np.empty(nLoc), HbyA=np.empty((3, nLoc)),
               p=np.empty(nLoc), phi=np.empty(max(Fl, 1)), phib=np.empty(max(B, 1)), Uc=np.empty((3, nLoc)))
    nit = (C.c_int * 16)()
    lib.b1_demo.restype = C.c_int
    lib.b1_demo.argtypes = ([C.c_void_p] * 3 + [C.c_double] * 2 + [dp] * 5 + [C.POINTER(dp)] + [dp] * 3 + [C.POINTER(dp)] + [C.c_double] + [dp] * 4
                            + [dp] * 3 + [C.c_double] + [C.POINTER(dp)] + [dp] * 2 + [dp] * 10 + [C.POINTER(C.c_int)])
    bcPp = PP([bnd(x) for x in I["bcP"]]); bcYp = PP([bnd(x) for x in I["bcY"]]); bcUp = PP([bnd(x) for x in I["bcU"]])
    ctx._ready()
    ns = lib.b1_demo(ctx.h, A.h, mesh.h, I["dt"], I["alphaY"], P(cell(I["rho_old"])), P(cell(I["rho_now"])), P(face(I["phi"], True)), P(bnd(I["phib"])),
                     P(cell(I["Yi0"])), bcYp, P(cell(I["dEff"])), P(cell(I["R"])), P(cell(I["U0"])), bcUp, I["mu"], P(face(I["ghf"])), P(bnd(I["ghfb"])),
                     P(cell(I["p_rgh"])), P(bnd(I["p_b"])), P(cell(I["psi_now"])), P(cell(I["psi_old"])), P(cell(I["gh"])), I["pRef"], bcPp,
                     P(bnd(I["fluxMask"])), P(bnd(I["UfixMask"])),
                     P(out["rho"]), P(out["Yi"]), P(out["U"]), P(out["K"]), P(out["rAU"]), P(out["HbyA"]),
                     P(out["p"]), P(out["phi"]), P(out["phib"]), P(out["Uc"]), nit)
    assert ns == 6
    res = {k: D.owned_cells(out[k]) for k in ("rho", "Yi", "U", "K", "rAU", "HbyA", "p", "Uc")}
    D.close()
    return res, D.owned, list(nit[:6])


def run_b1_fvdom(ffm, ctx, m, T, Tb, E, emis, sub=None, part=None, nPhi=2, nTheta=2, maxIter=3, tolerance=0.0, scheme=0, a=0.3, IiTol=1e-12, nCalls=2):
    """b1_fvdom of examples/b1_demo.C (the fvDOM handle with its iteration and grey-diffusive walls) on the whole mesh or on one rank's
    sub-domain.  T, E: global cell fields; Tb, emis: per patch.  Returns (I [nRay][owned], G [owned], qin per owned boundary face as a
    dict patch -> (global face positions, values)), the owned cells' global labels and the iterations of every call."""
    D = _Domain(ffm, ctx, m, sub, part)
    A, mesh, nLoc, B, cell = D.A, D.mesh, D.nLoc, D.B, D.cell
    bnd = lambda lst: D.bnd(np.concatenate(lst))
    lib = C.CDLL(os.path.join(os.path.dirname(ffm.libpath()), "libffm_b1demo.so"))
    dp = C.POINTER(C.c_double)
    solD = getattr(m, "solutionD", (1, 1, 1))
    nRay = 4 * nPhi * nTheta if min(solD) > 0 else 4 * nPhi
    Tc, Tbb, Ec, emb = cell(T), bnd(Tb), cell(E), bnd(emis)
    IOut, GOut = np.empty((nRay, nLoc)), np.empty(nLoc)
    qin, qem, qr = np.empty(max(B, 1)), np.empty(max(B, 1)), np.empty(max(B, 1))
    iters, nSolves = (C.c_int * nCalls)(), C.c_int()
    lib.b1_fvdom.restype = C.c_int
    lib.b1_fvdom.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_double, C.c_int, C.c_double, C.c_double] + [dp] * 4 + [C.c_int] + [dp] * 5 + [C.POINTER(C.c_int)] * 2
    os.environ["FFM_FOAM_QUIET"] = "1"
    ctx._ready()
    P = lambda x: x.ctypes.data_as(dp)
    n = lib.b1_fvdom(ctx.h, A.h, mesh.h, sum(1 << d for d in range(3) if solD[d] < 0), nPhi, nTheta, maxIter, tolerance, scheme, a, IiTol,
                     P(Tc), P(Tbb), P(Ec), P(emb), nCalls, P(IOut), P(GOut), P(qin), P(qem), P(qr), iters, C.byref(nSolves))
    assert n == nRay
    I, G = D.owned_cells(IOut), D.owned_cells(GOut)
    # qin per patch on this rank's faces: (positions inside the global patch, values)
    qp, off = {}, 0
    for p, k in zip(m.patches, D.pmask):
        cnt = int(k.sum())
        qp[p.name] = (np.nonzero(k)[0], qin[off:off + cnt].copy()); off += cnt
    D.close()
    return (I, G, qp), D.owned, list(iters)


PHYSICS = dict(dt=2e-3, t=4.0, table=(0.0, 0.01, 10.0, 0.03), mff=0.7, alphaK=0.9, a=0.3, e=0.45, sigmaS=0.2, Cs=0.5,
               Ck=0.094, Ce=1.048, Prt=1.0, PrtWall=0.85, C_EDC=4.0, fuel=2, o2=0)


def physics_inputs(O, m):
    """the inputs of examples/b1_demo.C's b1_physics on the GLOBAL mesh: cell arrays [N], face arrays [F], boundary arrays [B] with the
    patches concatenated; every field hashed and non-uniform.  |phi_b| >= 0.002 (no pos0 decision on rounding noise) except on every
    fourth inlet face, where it is exactly 0: the max(|phi|, SMALL) branch of totalFlowRateAdvectiveDiffusive."""
    N, F = m.nCells, m.nFaces
    B = sum(p.size for p in m.patches)
    hu = lambda seed, n: O.hash_u(seed, np.arange(n))
    on = lambda *names: np.concatenate([np.full(p.size, 1.0 if p.name in names else 0.0) for p in m.patches])
    inlet, fixed, open_ = on("inlet"), on("inlet", "floor"), on("top", "sides")
    I = dict(PHYSICS)
    for tag, n, s in (("", N, 200), ("b", B, 300)):
        Y = np.empty((5, n))
        Y[0] = 0.15 + 0.08 * hu(s, n); Y[1] = 0.02 + 0.03 * hu(s + 1, n); Y[2] = 0.05 + 0.2 * hu(s + 2, n); Y[3] = 0.02 + 0.03 * hu(s + 3, n)
        Y[4] = 1.0 - Y[:4].sum(axis=0)
        I["Y" + tag] = Y
        I["T" + tag] = 400.0 + 1200.0 * hu(s + 5, n)                                   # both janaf ranges (Tcommon = 1000 K)
        I["p" + tag] = 101325.0 * (1.0 + 0.01 * (hu(s + 6, n) - 0.5))
        I["rhoFac" + tag] = 1.0 + 0.01 * (hu(s + 7, n) - 0.3)
        I["fa" + tag] = hu(s + 8, n); I["fc" + tag] = hu(s + 9, n)
    I["Tstart"] = I["T"] * (1.0 + 0.05 * (hu(210, N) - 0.5))
    I["fixesT"] = fixed
    I["phi"] = 0.02 * (hu(220, F) - 0.5)
    sgn = np.where(inlet > 0.5, -1.0, np.where(hu(221, B) > 0.5, 1.0, -1.0))          # the inlet flows in; the other faces either way
    I["phib"] = sgn * (0.002 + 0.008 * hu(222, B))
    ii = np.nonzero(inlet > 0.5)[0]
    I["phib"][ii[::4]] = 0.0
    I["U0"] = np.stack([hu(230 + d, N) - 0.5 for d in range(3)])
    I["bcU"] = [x for d in range(3) for x in (np.where(fixed > 0.5, 1.0, hu(240 + d, B)), hu(250 + d, B) - 0.5, np.zeros(B))]
    Sf = np.concatenate([p.Sf for p in m.patches]); magSf = np.concatenate([p.magSf for p in m.patches])
    I["inletMask"] = inlet; I["inletNf"] = (Sf / magSf[:, None]).T.copy()
    I["k0"] = 2e-3 * (1.0 + hu(260, N)); I["delta"] = 0.1 * (0.9 + 0.2 * hu(261, N))
    I["bcK"] = [np.where(fixed > 0.5, 1.0, -1.0), 1e-3 * (1.0 + hu(262, B)), np.zeros(B)]               # fixedValue / inletOutlet
    I["nutZeroGrad"] = 1.0 - on("floor"); I["alphatZeroGrad"] = 1.0 - on("floor")
    I["bcY"] = [np.where(open_ > 0.5, -1.0, 0.0), np.where(inlet > 0.5, I["mff"], 0.05 + 0.1 * hu(270, B)), np.zeros(B)]
    I["E"] = 2.0e4 * hu(280, N); I["emissivity"] = 0.3 + 0.5 * hu(281, B)
    # the extremes of the two reduction fields: `fa` on two boundary faces at the far end of the last patch, `fc` in the last two cells
    I["fab"][B - 1] = 2.5; I["fab"][B - 2] = -1.5
    I["fc"][N - 1] = 3.0; I["fc"][N - 2] = -2.0
    return I


def run_b1_physics(ffm, ctx, m, I, sub=None, part=None):
    """b1_physics of examples/b1_demo.C on the whole mesh or on the sub-domain `sub` of the decomposition `part`.  Returns
    {name: values}: cell fields on the OWNED cells, boundary fields on this rank's boundary faces, `cells` / `bpos` their global
    labels (bpos: positions in the patches-concatenated list), `scalars` [18], `nit` the iteration counts of the six solves."""
    import json
    from oracle import thermo as TH
    D = _Domain(ffm, ctx, m, sub, part)
    here = os.path.dirname(os.path.abspath(__file__))
    data = json.load(open(os.path.join(here, "golden", "steckler_case_data.json")))
    table = {n: {k: (np.array(v) if isinstance(v, list) else v) for k, v in d.items()} for n, d in data["table"].items()}
    th = ffm.Thermo(ctx, data["species"], table, TH.RR)
    sp = TH.Species(data["species"], table)
    rx = data["reaction"]
    ss = TH.SingleStep(sp, [tuple(t) for t in rx["lhs"]], [tuple(t) for t in rx["rhs"]], fuel=data["fuel"], inert=data["inertSpecie"])
    from oracle import plume
    lib = C.CDLL(os.path.join(os.path.dirname(ffm.libpath()), "libffm_b1demo.so"))
    dp = C.POINTER(C.c_double); dpp = C.POINTER(dp)
    keep = []

    def P(a):
        a = np.ascontiguousarray(a, np.float64); keep.append(a)
        return a.ctypes.data_as(dp)

    def PP(arrs):
        ptrs = [P(a) for a in arrs]
        arr = (dp * len(ptrs))(*ptrs); keep.append(arr)
        return C.cast(arr, dpp)
    nLoc, B = D.nLoc, max(D.B, 1)
    out = dict(thermo=np.empty((4, nLoc)), thermob=np.empty((4, B)), nut0=np.empty((2, nLoc)), nut0b=np.empty((2, B)), wFuel=np.empty(nLoc), G=np.empty(nLoc), k=np.empty(nLoc),
               nut=np.empty((2, nLoc)), nutb=np.empty((2, B)), src=np.empty((3, nLoc)), U=np.empty((3, nLoc)), Ub=np.empty((3, B)),
               Yi=np.empty(nLoc), Yb=np.empty(B), f=np.empty(B), p1=np.empty((2, nLoc)), scalars=np.full(20, np.nan))
    nit = (C.c_int * 6)()
    names = (C.c_char_p * 5)(*[s.encode() for s in data["species"]]); keep.append(names)
    tab = np.array(I["table"], np.float64)
    fields = [("deltaT", C.c_double, I["dt"]), ("t", C.c_double, I["t"]), ("nTable", C.c_int, len(tab) // 2), ("table", dp, P(tab)),
              ("massFluxFraction", C.c_double, I["mff"]), ("th", C.c_void_p, th.h), ("nSpecies", C.c_int, 5),
              ("specieNames", C.POINTER(C.c_char_p), C.cast(names, C.POINTER(C.c_char_p))),
              ("Y", dpp, PP([D.cell(y) for y in I["Y"]])), ("Yb", dpp, PP([D.bnd(y) for y in I["Yb"]]))]
    fields += [(k, dp, P(D.cell(I[k]))) if not b else (k, dp, P(D.bnd(I[k])))
               for k, b in (("T", 0), ("Tb", 1), ("Tstart", 0), ("p", 0), ("pb", 1), ("fixesT", 1), ("rhoFac", 0), ("rhoFacb", 1))]
    fields += [("phiF", dp, P(D.face(I["phi"], True))), ("phiB", dp, P(D.bnd(I["phib"]))), ("U0", dp, P(D.cell(I["U0"]))),
               ("bcU", dpp, PP([D.bnd(x) for x in I["bcU"]])), ("inletMask", dp, P(D.bnd(I["inletMask"]))), ("inletNf", dp, P(D.bnd(I["inletNf"]))),
               ("k0", dp, P(D.cell(I["k0"]))), ("delta", dp, P(D.cell(I["delta"]))), ("bcK", dpp, PP([D.bnd(x) for x in I["bcK"]])),
               ("nutZeroGrad", dp, P(D.bnd(I["nutZeroGrad"]))), ("alphatZeroGrad", dp, P(D.bnd(I["alphatZeroGrad"]))), ("alphaK", C.c_double, I["alphaK"]),
               ("fuel", C.c_int, I["fuel"]), ("o2", C.c_int, I["o2"]), ("s", C.c_double, float(ss.s)), ("qFuel", C.c_double, float(ss.qFuel)),
               ("massCoeffs", dp, P(plume.NU)), ("bcY", dpp, PP([D.bnd(x) for x in I["bcY"]])),
               ("a", C.c_double, I["a"]), ("e", C.c_double, I["e"]), ("sigmaS", C.c_double, I["sigmaS"]), ("Cscatter", C.c_double, I["Cs"]),
               ("E", dp, P(D.cell(I["E"]))), ("emissivity", dp, P(D.bnd(I["emissivity"]))),
               ("fa", dp, P(D.cell(I["fa"]))), ("fab", dp, P(D.bnd(I["fab"]))), ("fc", dp, P(D.cell(I["fc"]))), ("fcb", dp, P(D.bnd(I["fcb"])))]
    fields += [(k + "Out", dp, out[k].ctypes.data_as(dp)) for k in ("thermo", "thermob", "nut0", "nut0b", "wFuel", "G", "k", "nut", "nutb", "src", "U", "Ub", "Yi", "Yb", "f", "p1")]
    fields += [("scalars", dp, out["scalars"].ctypes.data_as(dp)), ("nIter", C.POINTER(C.c_int), C.cast(nit, C.POINTER(C.c_int)))]

    class Data(C.Structure):                       # struct b1PhysicsData, field for field
        _fields_ = [(n, t) for n, t, _ in fields]
    io = Data(*[v for _, _, v in fields])
    lib.b1_physics.restype = C.c_int
    lib.b1_physics.argtypes = [C.c_void_p] * 3 + [C.POINTER(Data)]
    os.environ["FFM_FOAM_QUIET"] = "1"
    ctx._ready()
    ns = lib.b1_physics(ctx.h, D.A.h, D.mesh.h, C.byref(io))
    assert ns == 6, ns
    res = dict(cells=D.owned, bpos=D.bpos, nit=np.array(list(nit)), scalars=out["scalars"][:18].copy(), s=float(ss.s), qFuel=float(ss.qFuel))
    for k in ("thermo", "nut0", "wFuel", "G", "k", "nut", "src", "U", "Yi", "p1"):
        res[k] = D.owned_cells(out[k])
    for k in ("thermob", "nut0b", "nutb", "Ub", "Yb", "f"):
        res[k] = out[k][..., :D.B].copy()
    D.close(); th.close()
    return res


def fvdom_inputs(m):
    """a flame-like temperature / emission field and wall emissivities for run_b1_fvdom"""
    x, y = m.C[:, 0], m.C[:, 1]
    T = 500.0 + 600.0 * np.exp(-((x - x.mean()) ** 2 + (y - 0.3 * y.max()) ** 2) / 0.05)
    E = 2.0e5 * np.exp(-((x - x.mean()) ** 2 + (y - 0.3 * y.max()) ** 2) / 0.03)
    Tb = [np.full(p.size, 900.0 if p.name == "inlet" else 320.0) for p in m.patches]
    emis = [np.full(p.size, e) for p, e in zip(m.patches, (0.3, 0.85, 1.0, 0.55))]
    return T, Tb, E, emis
