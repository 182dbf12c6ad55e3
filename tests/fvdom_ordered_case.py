"""b1_fvdom_ordered of examples/b1_demo.C (the fvDOM handle with setOrderedSolves(true)) on the whole mesh or on ONE RANK's sub-domain
of a decomposition -- the set-up of foam_case.run_b1_fvdom with the ordered entry point, the Foam layer's log lines left on (a
helper, not a test): shared by tests/test_fvdom_ordered_decomposed_gpu.py and its worker."""
import ctypes as C
import os

import numpy as np


def run(ffm, ctx, m, T, Tb, E, emis, sub=None, part=None, nPhi=2, nTheta=2, maxIter=3, tolerance=0.0, scheme=0, a=0.3, nCalls=2, quiet=False):
    """Returns (I [nRay][owned], G [owned], qin per patch -> (positions inside the global patch, values)), the owned cells' global
    labels, the iterations of every call, the number of ray solves of the last call and the largest iteration count of any solve."""
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
    A = ffm.lduMatrix(ctx, nOwn, l2, u2, nGhost=nGhost)
    if sub is not None:
        A.set_ghost_exchange(sub.nbrRank, sub.sendCount, oldToNew[sub.sendCells], sub.recvCount, tags=sub.tags, globalCells=N)
    wgt = np.where(sign < 0, 1.0 - m.weights[gface], m.weights[gface])
    patches = [(oldToNew[g2l[p.faceCells[k]]].astype(np.int32), p.Sf[k].T.copy(), p.deltaCoeffs[k]) for p, k in zip(m.patches, pmask)]
    mesh = ffm.fvMesh(A, m.V[gcell][cOrd], m.C[gcell][cOrd].T.copy(), (m.Sf[gface] * sign[:, None])[fOrd].T.copy(), m.magSf[gface][fOrd],
                      wgt[fOrd], m.deltaCoeffs[gface][fOrd], patches)
    mesh.set_face_centres(m.Cf[gface][fOrd].T.copy())
    B = sum(int(k.sum()) for k in pmask)
    lib = C.CDLL(os.path.join(os.path.dirname(ffm.libpath()), "libffm_b1demo.so"))
    dp = C.POINTER(C.c_double)
    h = lambda x: np.ascontiguousarray(x, np.float64)
    cell = lambda x: h(np.asarray(x)[gcell][cOrd])
    bnd = lambda lst: h(np.concatenate([np.asarray(x)[k] for x, k in zip(lst, pmask)])) if B else np.zeros(1)
    solD = getattr(m, "solutionD", (1, 1, 1))
    nRay = 4 * nPhi * nTheta if min(solD) > 0 else 4 * nPhi
    Tc, Tbb, Ec, emb = cell(T), bnd(Tb), cell(E), bnd(emis)
    IOut, GOut = np.empty((nRay, nLoc)), np.empty(nLoc)
    qin, qem, qr = np.empty(max(B, 1)), np.empty(max(B, 1)), np.empty(max(B, 1))
    iters, nSolves, maxIts = (C.c_int * nCalls)(), C.c_int(), C.c_int(-1)
    lib.b1_fvdom_ordered.restype = C.c_int
    lib.b1_fvdom_ordered.argtypes = ([C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_double, C.c_int, C.c_double, C.c_double] + [dp] * 4 + [C.c_int] + [dp] * 5
                                     + [C.POINTER(C.c_int)] * 3)
    if quiet:
        os.environ["FFM_FOAM_QUIET"] = "1"
    else:
        os.environ.pop("FFM_FOAM_QUIET", None)
    ctx._ready()
    P = lambda x: x.ctypes.data_as(dp)
    n = lib.b1_fvdom_ordered(ctx.h, A.h, mesh.h, sum(1 << d for d in range(3) if solD[d] < 0), nPhi, nTheta, maxIter, tolerance, scheme, a, 1e-12,
                             P(Tc), P(Tbb), P(Ec), P(emb), nCalls, P(IOut), P(GOut), P(qin), P(qem), P(qr), iters, C.byref(nSolves), C.byref(maxIts))
    assert n == nRay
    inv = np.empty(nLoc, np.int64); inv[cOrd] = np.arange(nLoc)
    I = IOut[:, inv][:, :nOwn]; G = GOut[inv][:nOwn]
    qp, off = {}, 0
    for p, k in zip(m.patches, pmask):
        cnt = int(k.sum())
        qp[p.name] = (np.nonzero(k)[0], qin[off:off + cnt].copy()); off += cnt
    mesh.close(); A.close()
    return (I, G, qp), gcell[:nOwn].copy(), list(iters), nSolves.value, maxIts.value
