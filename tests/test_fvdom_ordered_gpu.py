"""The fvDOM handle with setOrderedSolves(true) (include/fireFoamHandles.H; every ray by fvScalarMatrix::solveOrdered, one exact forward
substitution in the order of its own matrix) through b1_fvdom_ordered of examples/b1_demo.C, against oracle/fvdom.py given the exact
solve as its linear solver: the serial forward substitution of tests/ray_matrix.py with OpenFOAM's normalised residuals.  The four
cases of tests/test_fvdom_gpu.py: iteration counts of fvDOM::calculate per call, the number of ray solves, every solve one iteration,
every Ii, G, qin, qem, qr.  With exact solves on both sides only the assembly's rounding (numpy against the device) separates the
two: the measured maxima over the four cases are 2.6e-16 (the intensities, relative L2), 1.1e-16 (G) and 4.4e-16 (the wall fluxes,
relative to the largest), so the comparison is asserted at 100 times the largest, 4.5e-14, not at the 1e-8 of the iterative comparison.  Control: on the first case today's iterative solves
(b1_fvdom, PBiCGStab + DILU to 1e-9) agree with the ordered ones to that 1e-8."""
import ctypes as C
import os

import numpy as np
import pytest

import ray_matrix as R
from common import rel_l2

pytestmark = pytest.mark.gpu

BOUND = 4.5e-14            # 100 x the measured maximum (docstring); the issue's ceiling for this comparison is 1e-8
CONTROL = 1e-8

PARAMS = [
    ((7, 8, 6), (), 2, 2, 4, 1e-6, "upwind", 2, (0.3, 0.85, 1.0, 0.55)),
    ((14, 18, 1), ("zmin", "zmax"), 2, 2, 5, 1e-3, "linearUpwind", 3, (0.17, 1.0, 1.0, 1.0)),
    ((14, 18, 1), ("zmin", "zmax"), 2, 2, 5, 1e-3, "linearUpwind", 3, (0.85, 1.0, 1.0, 1.0)),
    ((6, 7, 5), (), 2, 4, 1, 0.0, "upwind", 1, (1.0, 1.0, 1.0, 1.0))]


@pytest.mark.parametrize("case", range(len(PARAMS)))
def test_ordered_ray_solves_against_the_exactly_solved_oracle(O, ffm, ctx, case):
    shape, empty, nPhi, nTheta, maxIter, tol, scheme, nCalls, emis = PARAMS[case]
    from oracle import plume, fvdom
    lib = C.CDLL(os.path.join(os.path.dirname(ffm.libpath()), "libffm_b1demo.so"))
    m = plume.make_mesh(shape, empty=empty)
    N = m.nCells
    B = sum(p.size for p in m.patches)
    cOrd, fOrd = ffm.renumber_levels(N, m.l, m.u)
    l2, u2, oldToNew = ffm.hexmesh.apply_renumbering(N, m.l, m.u, cOrd, fOrd)
    A = ffm.lduMatrix(ctx, N, l2, u2)
    patches = [(oldToNew[p.faceCells].astype(np.int32), p.Sf.T.copy(), p.deltaCoeffs) for p in m.patches]
    mesh = ffm.fvMesh(A, m.V[cOrd], m.C[cOrd].T.copy(), m.Sf[fOrd].T.copy(), m.magSf[fOrd], m.weights[fOrd], m.deltaCoeffs[fOrd], patches)
    mesh.set_face_centres(m.Cf[fOrd].T.copy())
    solD = m.solutionD
    x, y = m.C[:, 0], m.C[:, 1]
    T = 500.0 + 600.0 * np.exp(-((x - x.mean()) ** 2 + (y - 0.3 * y.max()) ** 2) / 0.02)         # a flame-like hot spot
    Tb = [np.full(p.size, 900.0 if p.name == "inlet" else 320.0) for p in m.patches]
    E = 2.0e5 * np.exp(-((x - x.mean()) ** 2 + (y - 0.3 * y.max()) ** 2) / 0.01)
    a = 0.3
    emissivity = [np.full(p.size, e) for p, e in zip(m.patches, emis)]
    ml, mu = np.asarray(m.l, np.int64), np.asarray(m.u, np.int64)

    def solve(name, d, upper, lower, s, psi0):
        """the exact solve: forward substitution in the matrix's own Kahn order, OpenFOAM's residuals as Ldu.solve returns them"""
        lev, _, acyclic = R.kahn_levels(N, *R.edges(ml, mu, upper, lower))
        assert acyclic
        Ao = O.Ldu(N, m.l, m.u).set_coeffs(d, upper, lower)
        normFactor = Ao.norm_factor(psi0, s)
        psi = R.forward_substitution(N, ml, mu, d, upper, lower, s, np.argsort(lev, kind="stable"))
        return psi, dict(initialResidual=float(np.abs(Ao.residual(psi0, s)).sum() / normFactor),
                         finalResidual=float(np.abs(Ao.residual(psi, s)).sum() / normFactor), nIterations=1, converged=1, singular=0)
    ref = fvdom.FvDOM(m, nPhi, nTheta, solve, maxIter=maxIter, tolerance=tol, divScheme=scheme, solutionD=solD, emissivity=emissivity)
    its_ref = []
    for _ in range(nCalls):
        ref.calculate(T, Tb, a, E); its_ref.append(ref.nIterations)
    nRay = len(ref.rays)
    dp = C.POINTER(C.c_double)
    P = lambda v: np.ascontiguousarray(v, np.float64)
    Tc, Tbb, Ec, emb = P(T[cOrd]), P(np.concatenate(Tb)), P(E[cOrd]), P(np.concatenate(emissivity))
    base = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_double, C.c_int, C.c_double, C.c_double] + [dp] * 4 + [C.c_int] + [dp] * 5 + [C.POINTER(C.c_int)] * 2
    lib.b1_fvdom.restype = lib.b1_fvdom_ordered.restype = C.c_int
    lib.b1_fvdom.argtypes = base
    lib.b1_fvdom_ordered.argtypes = base + [C.POINTER(C.c_int)]
    os.environ["FFM_FOAM_QUIET"] = "1"
    ed = sum(1 << d for d in range(3) if solD[d] < 0)

    def run(fn, *extra):
        out = dict(I=np.empty((nRay, N)), G=np.empty(N), qin=np.empty(B), qem=np.empty(B), qr=np.empty(B))
        iters, nSolves = (C.c_int * nCalls)(), C.c_int()
        n = fn(ctx.h, A.h, mesh.h, ed, nPhi, nTheta, maxIter, tol, 5 if scheme == "linearUpwind" else 0, a, 1e-9,
               Tc.ctypes.data_as(dp), Tbb.ctypes.data_as(dp), Ec.ctypes.data_as(dp), emb.ctypes.data_as(dp), nCalls,
               *(out[k].ctypes.data_as(dp) for k in ("I", "G", "qin", "qem", "qr")), iters, C.byref(nSolves), *extra)
        assert n == nRay == (4 * nPhi if empty else 4 * nPhi * nTheta)
        return out, list(iters), nSolves.value
    maxIts = C.c_int(-1)
    got, iters, nSolves = run(lib.b1_fvdom_ordered, C.byref(maxIts))
    assert iters == its_ref, (iters, its_ref)
    assert nSolves == len(ref.log)
    assert maxIts.value == 1
    inv = np.empty(N, np.int64); inv[cOrd] = np.arange(N)
    errI = max(rel_l2(got["I"][i][inv], ref.I[i]) for i in range(nRay))
    errG = rel_l2(got["G"][inv], ref.G)
    errQ = {}
    for name, want in (("qin", ref.qin), ("qem", ref.qem), ("qr", ref.qr)):
        w = np.concatenate(want)
        errQ[name] = np.abs(got[name] - w).max() / max(np.abs(w).max(), 1e-300)
    print("ordered fvDOM against the exactly solved oracle, case %d: I %.3e  G %.3e  qin %.3e  qem %.3e  qr %.3e"
          % (case, errI, errG, errQ["qin"], errQ["qem"], errQ["qr"]))
    assert errI < BOUND and errG < BOUND, (errI, errG)
    for name, e in errQ.items():
        assert e <= BOUND, (name, e)
    if min(emis) < 1.0:
        assert max(its_ref) > 1                                                    # the walls' reflection needed the iteration
    if case == 0:
        # control: today's iterative ray solves on the same case
        it, iters_it, nSolves_it = run(lib.b1_fvdom)
        assert iters_it == iters and nSolves_it == nSolves
        for i in range(nRay):
            assert rel_l2(it["I"][i], got["I"][i]) < CONTROL, i
        assert rel_l2(it["G"], got["G"]) < CONTROL
        for name in ("qin", "qem", "qr"):
            assert np.abs(it[name] - got[name]).max() <= CONTROL * max(np.abs(got[name]).max(), 1e-300), name
    A.close()
