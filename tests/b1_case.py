"""The inputs of examples/b1_demo.C's b1_demo (a plume box in the library's cell order, seeded fields, mixed boundary conditions) and
the call itself, shared by tests/test_foam_layer_gpu.py (against the oracle) and tests/test_pool_poison_gpu.py (against itself with
the allocator handing out NaN-filled blocks)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np


def b1_inputs(O, ffm, ctx, n=(9, 8, 7)):
    """everything test_b1_demo_matches_oracle defines before the oracle's evaluation, as a namespace"""
    from oracle import fv, plume
    m = plume.make_mesh(n, h=0.1)
    N, F = m.nCells, m.nFaces
    B = sum(p.size for p in m.patches)
    cOrd, fOrd = ffm.renumber_levels(N, m.l, m.u)
    l2, u2, oldToNew = ffm.hexmesh.apply_renumbering(N, m.l, m.u, cOrd, fOrd)
    A = ffm.lduMatrix(ctx, N, l2, u2)
    patches = [(oldToNew[p.faceCells].astype(np.int32), p.Sf.T.copy(), p.deltaCoeffs) for p in m.patches]
    mesh = ffm.fvMesh(A, m.V[cOrd], m.C[cOrd].T.copy(), m.Sf[fOrd].T.copy(), m.magSf[fOrd], m.weights[fOrd], m.deltaCoeffs[fOrd], patches)
    mesh.set_face_centres(m.Cf[fOrd].T.copy())
    hu = lambda seed, n: O.hash_u(seed, np.arange(n))
    pl = lambda seed, scale=1.0, shift=0.0: [shift + scale * hu(seed + q, p.size) for q, p in enumerate(m.patches)]
    dt, alphaY, mu = 2e-3, 0.8, 1.8e-5
    rho_old = 1.0 + 0.2 * hu(1, N); rho_now = rho_old * (1 + 0.01 * (hu(2, N) - 0.5))
    phi = 0.02 * (hu(3, F) - 0.5); phib = pl(10, 0.02, -0.01)
    Yi0 = 0.1 + 0.8 * hu(4, N); dEff = 2e-5 * (1 + hu(5, N)); R = 0.5 * (hu(6, N) - 0.5)
    U0 = np.stack([hu(20 + d, N) - 0.5 for d in range(3)])
    p_rgh = 10.0 * (hu(7, N) - 0.5); ghf = -9.81 * m.Cf[:, 1]; ghfb = [-9.81 * p.Cf[:, 1] for p in m.patches]
    bcY = fv.MixedBC(m, f=pl(30), ref=pl(40, 0.5), refGrad=pl(50, 0.1, -0.05))
    bcU = [fv.MixedBC(m, f=pl(60 + 10 * d), ref=pl(90 + 10 * d, 1.0, -0.5)) for d in range(3)]
    p_b = pl(120, 10.0, -5.0)
    # pEqn inputs: compressibility now / old, gh, pRef; p_rgh: fixedFluxPressure on inlet, floor and sides (gradient set by
    # constrainPressure), fixedValue on the top; U fixes its value on inlet and floor
    psi_now = 1.17e-5 * (0.9 + 0.2 * hu(130, N)); psi_old = psi_now * (1 + 1e-3 * (hu(131, N) - 0.5))
    gh = -9.81 * m.C[:, 1]; pRef = 101325.0
    names = [p.name for p in m.patches]
    fluxMask = [np.full(p.size, 0.0 if p.name == "top" else 1.0) for p in m.patches]
    UfixMask = [np.full(p.size, 1.0 if p.name in ("inlet", "floor") else 0.0) for p in m.patches]
    for d in range(3):                                    # consistent with the mask: fixedValue there
        for q, p in enumerate(m.patches):
            if p.name in ("inlet", "floor"):
                bcU[d].f[q] = np.ones(p.size)
    bcP = fv.MixedBC(m, f=[np.full(p.size, 1.0 if p.name == "top" else 0.0) for p in m.patches], ref=pl(140, 2.0, -1.0))
    rdt = 1.0 / dt
    zb = [np.zeros(p.size) for p in m.patches]
    ctl = dict(tolerance=1e-10, relTol=0.0)
    return SimpleNamespace(**{k: v for k, v in locals().items() if k not in ("O", "ffm", "ctx", "fv", "plume")})


def run_b1_demo(ffm, ctx, I):
    """b1_demo on the device: (number of solves, the ten output arrays, the iteration counts)"""
    A, mesh, m, N, F, B, cOrd, fOrd = I.A, I.mesh, I.m, I.N, I.F, I.B, I.cOrd, I.fOrd
    dt, alphaY, mu, pRef = I.dt, I.alphaY, I.mu, I.pRef
    rho_old, rho_now, phi, phib, Yi0, dEff, R, U0 = I.rho_old, I.rho_now, I.phi, I.phib, I.Yi0, I.dEff, I.R, I.U0
    p_rgh, ghf, ghfb, p_b, psi_now, psi_old, gh = I.p_rgh, I.ghf, I.ghfb, I.p_b, I.psi_now, I.psi_old, I.gh
    bcY, bcU, bcP, fluxMask, UfixMask = I.bcY, I.bcU, I.bcP, I.fluxMask, I.UfixMask
    lib = C.CDLL(os.path.join(os.path.dirname(ffm.libpath()), "libffm_b1demo.so"))
    dp = C.POINTER(C.c_double)
    h = lambda a: np.ascontiguousarray(a, np.float64)
    cell = lambda a: h(np.asarray(a)[..., cOrd])
    face = lambda a: h(np.asarray(a)[fOrd])
    bnd = lambda lst: h(np.concatenate(lst))
    keep = []
    def P(a):
        keep.append(a)
        return a.ctypes.data_as(dp)
    def PP(arrs):
        arrs = [h(a) for a in arrs]; keep.append(arrs)
        arr = (dp * len(arrs))(*[a.ctypes.data_as(dp) for a in arrs]); keep.append(arr)
        return arr
    out = dict(rho=np.empty(N), Yi=np.empty(N), U=np.empty((3, N)), K=np.empty(N), rAU=np.empty(N), HbyA=np.empty((3, N)),
               p=np.empty(N), phi=np.empty(F), phib=np.empty(B), Uc=np.empty((3, N)))
    nit = (C.c_int * 16)()
    lib.b1_demo.restype = C.c_int
    lib.b1_demo.argtypes = ([C.c_void_p] * 3 + [C.c_double] * 2 + [dp] * 5 + [C.POINTER(dp)] + [dp] * 3 + [C.POINTER(dp)] + [C.c_double] + [dp] * 4
                            + [dp] * 3 + [C.c_double] + [C.POINTER(dp)] + [dp] * 2 + [dp] * 10 + [C.POINTER(C.c_int)])
    bcPp = PP([bnd(bcP.f), bnd(bcP.ref), bnd(bcP.refGrad)])
    bcYp = PP([bnd(bcY.f), bnd(bcY.ref), bnd(bcY.refGrad)])
    bcUp = PP([x for d in range(3) for x in (bnd(bcU[d].f), bnd(bcU[d].ref), bnd(bcU[d].refGrad))])
    ctx._ready()
    ns = lib.b1_demo(ctx.h, A.h, mesh.h, dt, alphaY, P(cell(rho_old)), P(cell(rho_now)), P(face(phi)), P(bnd(phib)),
                     P(cell(Yi0)), bcYp, P(cell(dEff)), P(cell(R)), P(cell(U0)), bcUp, mu, P(face(ghf)), P(bnd(ghfb)),
                     P(cell(p_rgh)), P(bnd(p_b)), P(cell(psi_now)), P(cell(psi_old)), P(cell(gh)), pRef, bcPp, P(bnd(fluxMask)), P(bnd(UfixMask)),
                     P(out["rho"]), P(out["Yi"]), P(out["U"]), P(out["K"]), P(out["rAU"]), P(out["HbyA"]),
                     P(out["p"]), P(out["phi"]), P(out["phib"]), P(out["Uc"]), nit)
    return ns, out, list(nit)


def sequence_inputs(O, ffm, ctx, n=(24, 20, 18)):
    """the inputs of examples/b1_demo.C's b1_solve_sequence in the style of b1_demo's, on a box whose sweeps are tiled, with a GAMG
    agglomeration on the same matrix handle"""
    from oracle import fv, plume
    m = plume.make_mesh(n, h=0.1)
    N, F = m.nCells, m.nFaces
    cOrd, fOrd = ffm.renumber_levels(N, m.l, m.u)
    l2, u2, oldToNew = ffm.hexmesh.apply_renumbering(N, m.l, m.u, cOrd, fOrd)
    A = ffm.lduMatrix(ctx, N, l2, u2)
    assert A.sweep_mode == 2 and A.native_order
    patches = [(oldToNew[p.faceCells].astype(np.int32), p.Sf.T.copy(), p.deltaCoeffs) for p in m.patches]
    mesh = ffm.fvMesh(A, m.V[cOrd], m.C[cOrd].T.copy(), m.Sf[fOrd].T.copy(), m.magSf[fOrd], m.weights[fOrd], m.deltaCoeffs[fOrd], patches)
    mesh.set_face_centres(m.Cf[fOrd].T.copy())
    G = ffm.GAMG(ctx, A, l2, u2, Sf=m.Sf[fOrd])
    hu = lambda seed, n: O.hash_u(seed, np.arange(n))
    pl = lambda seed, scale=1.0, shift=0.0: [shift + scale * hu(seed + q, p.size) for q, p in enumerate(m.patches)]
    dt, alphaY, mu = 0.05, 0.8, 1.8e-5             # (a time step and a diffusivity at which the specie solves take several iterations)
    rho_old = 1.0 + 0.2 * hu(1, N); rho_now = rho_old * (1 + 0.01 * (hu(2, N) - 0.5))
    phi = 0.02 * (hu(3, F) - 0.5); phib = pl(10, 0.02, -0.01)
    Yi0 = 0.1 + 0.8 * hu(4, N); Yj0 = 0.05 + 0.9 * hu(8, N); dEff = 0.5 * (1 + hu(5, N))
    Ri = 0.5 * (hu(6, N) - 0.5); Rj = 0.5 * (hu(9, N) - 0.5)
    U0 = np.stack([hu(20 + d, N) - 0.5 for d in range(3)])
    bcY = fv.MixedBC(m, f=pl(30), ref=pl(40, 0.5), refGrad=pl(50, 0.1, -0.05))
    bcU = [fv.MixedBC(m, f=pl(60 + 10 * d), ref=pl(90 + 10 * d, 1.0, -0.5)) for d in range(3)]
    psi = 1.17e-5 * (0.9 + 0.2 * hu(130, N)); gam = 1e-3 * (0.5 + hu(132, N)); p0 = 10.0 * (hu(7, N) - 0.5); S = 2.0 * hu(133, N) - 1.0
    bcP = fv.MixedBC(m, f=[np.full(p.size, 1.0 if p.name == "top" else 0.0) for p in m.patches], ref=pl(140, 2.0, -1.0))
    # the other user's system: symmetric, diagonally dominant, unrelated to anything above (LDU face order of the renumbered mesh)
    oUp = -(0.5 + hu(0xA0, F))
    oDiag = np.zeros(N); np.add.at(oDiag, l2, -oUp); np.add.at(oDiag, u2, -oUp); oDiag += 0.05 * (1.0 + hu(0xA1, N))
    oSrc = 2.0 * hu(0xA2, N) - 1.0
    rdt = 1.0 / dt
    ctl = dict(tolerance=1e-10, relTol=0.0)

    return SimpleNamespace(**{k: v for k, v in locals().items() if k not in ("O", "ffm", "ctx", "fv", "plume")})


def run_solve_sequence(ffm, ctx, I):
    """b1_solve_sequence on the device: (solves logged, fields [7][N], GAMG's field, iteration counts, residuals [14][2], epochs [9])"""
    A, mesh, G, N, cOrd, fOrd = I.A, I.mesh, I.G, I.N, I.cOrd, I.fOrd
    dt, alphaY, mu = I.dt, I.alphaY, I.mu
    rho_old, rho_now, phi, phib, Yi0, Yj0, dEff, Ri, Rj, U0 = I.rho_old, I.rho_now, I.phi, I.phib, I.Yi0, I.Yj0, I.dEff, I.Ri, I.Rj, I.U0
    bcY, bcU, bcP, psi, gam, p0, S, oDiag, oUp, oSrc = I.bcY, I.bcU, I.bcP, I.psi, I.gam, I.p0, I.S, I.oDiag, I.oUp, I.oSrc
    lib = C.CDLL(os.path.join(os.path.dirname(ffm.libpath()), "libffm_b1demo.so"))
    dp = C.POINTER(C.c_double)
    h = lambda a: np.ascontiguousarray(a, np.float64)
    cell = lambda a: h(np.asarray(a)[..., cOrd])
    face = lambda a: h(np.asarray(a)[fOrd])
    bnd = lambda lst: h(np.concatenate(lst))
    keep = []
    def P(a):
        keep.append(a)
        return a.ctypes.data_as(dp)
    def PP(arrs):
        arrs = [h(a) for a in arrs]; keep.append(arrs)
        arr = (dp * len(arrs))(*[a.ctypes.data_as(dp) for a in arrs]); keep.append(arr)
        return arr
    fields, gamgOut = np.empty((7, N)), np.empty(N)
    nit = (C.c_int * 16)(); res = np.empty((16, 2)); epochs = (C.c_ulong * 16)()
    lib.b1_solve_sequence.restype = C.c_int
    lib.b1_solve_sequence.argtypes = ([C.c_void_p] * 4 + [C.c_double] * 2 + [dp] * 6 + [C.POINTER(dp)] + [dp] * 4 + [C.POINTER(dp), C.c_double]
                                      + [dp] * 3 + [C.POINTER(dp)] + [dp] * 4 + [dp] * 2 + [C.POINTER(C.c_int), dp, C.POINTER(C.c_ulong)])
    bcYp = PP([bnd(bcY.f), bnd(bcY.ref), bnd(bcY.refGrad)])
    bcUp = PP([x for d_ in range(3) for x in (bnd(bcU[d_].f), bnd(bcU[d_].ref), bnd(bcU[d_].refGrad))])
    bcPp = PP([bnd(bcP.f), bnd(bcP.ref), bnd(bcP.refGrad)])
    ctx._ready()
    os.environ["FFM_FOAM_QUIET"] = "1"
    ns = lib.b1_solve_sequence(ctx.h, A.h, mesh.h, G.h, dt, alphaY, P(cell(rho_old)), P(cell(rho_now)), P(face(phi)), P(bnd(phib)),
                               P(cell(Yi0)), P(cell(Yj0)), bcYp, P(cell(dEff)), P(cell(Ri)), P(cell(Rj)), P(cell(U0)), bcUp, mu,
                               P(cell(psi)), P(cell(gam)), P(cell(p0)), bcPp, P(cell(S)),
                               P(h(oDiag)), P(h(oUp)), P(h(oSrc)),
                               P(fields), P(gamgOut), nit, P(res), epochs)
    return ns, fields, gamgOut, list(nit[:14]), res[:14].copy(), list(epochs[:9])


def gamg_layer_inputs(O, ffm, ctx, n=(16, 14, 12)):
    """the set-up of tests/test_gamg_gpu.py::test_solver_GAMG_through_the_foam_layer (examples/b1_demo.C: b1_gamg_solve), single rank"""
    from oracle import fv, plume
    m = plume.make_mesh(n, h=0.1)
    N = m.nCells
    cOrd, fOrd = ffm.renumber_levels(N, m.l, m.u)
    l2, u2, oldToNew = ffm.hexmesh.apply_renumbering(N, m.l, m.u, cOrd, fOrd)
    A = ffm.lduMatrix(ctx, N, l2, u2)
    patches = [(oldToNew[p.faceCells].astype(np.int32), p.Sf.T.copy(), p.deltaCoeffs) for p in m.patches]
    mesh = ffm.fvMesh(A, m.V[cOrd], m.C[cOrd].T.copy(), m.Sf[fOrd].T.copy(), m.magSf[fOrd], m.weights[fOrd], m.deltaCoeffs[fOrd], patches)
    G = ffm.GAMG(ctx, A, l2, u2, Sf=m.Sf[fOrd])
    hu = lambda seed, k: O.hash_u(seed, np.arange(k))
    dt = 1e-3
    psi = 1.17e-5 * (0.9 + 0.2 * hu(1, N)); gam = 1e-3 * (0.5 + hu(2, N)); p0 = 10.0 * (hu(3, N) - 0.5); S = 2.0 * hu(4, N) - 1.0
    bc = fv.MixedBC(m, f=[np.full(p.size, 1.0 if p.name == "top" else 0.0) for p in m.patches],
                    ref=[2.0 * hu(40 + q, p.size) - 1.0 for q, p in enumerate(m.patches)])
    return SimpleNamespace(m=m, N=N, cOrd=cOrd, A=A, mesh=mesh, G=G, dt=dt, psi=psi, gam=gam, p0=p0, S=S, bc=bc)


def run_gamg_layer(ffm, ctx, I, smoother, tolerance=1e-8):
    """b1_gamg_solve on the device: (iterations, the field, [initial, final] residual)"""
    lib = C.CDLL(os.path.join(os.path.dirname(ffm.libpath()), "libffm_b1demo.so"))
    dp = C.POINTER(C.c_double)
    h = lambda a: np.ascontiguousarray(a, np.float64)
    keep = [h(I.psi[I.cOrd]), h(I.gam[I.cOrd]), h(I.p0[I.cOrd]), h(I.S[I.cOrd])] + [h(np.concatenate(x)) for x in (I.bc.f, I.bc.ref, I.bc.refGrad)]
    P = lambda a: a.ctypes.data_as(dp)
    bcp = (dp * 3)(P(keep[4]), P(keep[5]), P(keep[6]))
    out = np.empty(I.N); res = np.empty(2)
    lib.b1_gamg_solve.restype = C.c_int
    lib.b1_gamg_solve.argtypes = [C.c_void_p] * 4 + [C.c_double, C.c_int, C.c_double, C.c_double] + [dp] * 3 + [C.POINTER(dp)] + [dp] * 3
    ctx._ready()
    os.environ["FFM_FOAM_QUIET"] = "1"
    nit = lib.b1_gamg_solve(ctx.h, I.A.h, I.mesh.h, I.G.h, I.dt, {"GaussSeidel": 3, "DIC": 1}[smoother], tolerance, 0.0,
                            P(keep[0]), P(keep[1]), P(keep[2]), bcp, P(keep[3]), P(out), P(res))
    return nit, out, res
