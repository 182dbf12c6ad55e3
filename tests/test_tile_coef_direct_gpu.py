"""The tiled sweeps' coefficient layout written by the kernel that assembles the matrix (csrc/ffm_fused.hip: ffm_fvm_pressure_eqn_direct,
ffm_fvm_scalar_transport_multi_ws_direct; csrc/ffm_fv.hip: ffm_fvm_transport_scheme_direct; csrc/ffm_tile.hip: ffm_tile_coef_direct)
instead of gathered from the native coefficients by a pass of its own (k_tile_gather).

Every comparison is of bytes: the three arrays -- forward upper, forward lower, backward upper; three doubles per cell -- against the
gather from the same native coefficients on a fresh handle, and solves that read them (PCG + DIC, PBiCGStab + DILU with 1, 3 and 5
lanes, symGaussSeidel) against the plain entry point + bind.  ffm_ldu_tile_gathers counts the gather passes of a handle, so that
"direct" is seen to have gathered nothing and "stale" to have gathered again.  Inputs are hexmesh.hash_u fields.

Boxes: 20 x 18 x 12 (tiles cut, rows with 0 - 3 lower and upper neighbours), 16 x 16 x 5 (one tile), 33 x 17 x 3 (ragged tiles).
Refused, the plain path giving the answer of a handle that never asked: rows wider than three entries (merged mesh `w4`), a matrix
without a tile plan (FFM_SWEEP=levels), a block with ghost cells."""
import ctypes as C
import os

import numpy as np
import pytest

import merged_mesh as MM

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
UNSUPPORTED = r"failed \(-5\)"                 # FFM_ERR_UNSUPPORTED through binding._check
BOXES = [(20, 18, 12), (16, 16, 5), (33, 17, 3)]
RDT = 1000.0


def _h(ffm, seed, n, lo=0.0, hi=1.0):
    return lo + (hi - lo) * ffm.hexmesh.hash_u(seed, np.arange(n))


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _box(ffm, ctx, n):
    from oracle import plume
    m = plume.make_mesh(n, h=0.1)
    N, F = m.nCells, m.nFaces
    cOrd, fOrd = ffm.renumber_levels(N, m.l, m.u)
    l2, u2, oldToNew = ffm.hexmesh.apply_renumbering(N, m.l, m.u, cOrd, fOrd)
    s = dict(N=N, F=F, B=sum(p.size for p in m.patches), l=l2, u=u2, handles=[])

    def handle():
        A = ffm.lduMatrix(ctx, N, l2, u2)
        s["handles"].append(A)
        return A
    s["handle"] = handle
    A = handle()
    assert A.native_order and A.sweep_mode == 2
    patches = [(oldToNew[p.faceCells].astype(np.int32), p.Sf.T.copy(), p.deltaCoeffs) for p in m.patches]
    s["A"] = A
    s["mesh"] = ffm.fvMesh(A, m.V[cOrd], m.C[cOrd].T.copy(), m.Sf[fOrd].T.copy(), m.magSf[fOrd], m.weights[fOrd], m.deltaCoeffs[fOrd], patches)
    # rows with 0 .. 3 lower and upper neighbours: the triples have 0 .. 3 absent slots
    nl, nu = np.bincount(u2, minlength=N), np.bincount(l2, minlength=N)
    s["nl"], s["nu"] = nl, nu
    return s


@pytest.fixture(scope="module", params=BOXES, ids=lambda n: "x".join(map(str, n)))
def box(request, ffm, ctx):
    s = _box(ffm, ctx, request.param)
    yield s
    s["mesh"].close()
    for A in s["handles"]:
        A.close()


# ---- the three assemblies: (entry point, arguments, outputs) with fresh outputs per call -------------------------------------------
def _pressure(s, ffm, ctx, direct, seed=0):
    mesh, N, F, B = s["mesh"], s["N"], s["F"], s["B"]
    dev, nat = ctx.to_device, lambda sd, lo, hi: mesh.to_native(_h(ffm, sd + seed, F, lo, hi))
    psi, psi0 = dev(_h(ffm, 60 + seed, N, 1e-5, 2e-5)), dev(_h(ffm, 61, N, 1e-5, 2e-5))
    p0, rho, rho0, gh = dev(_h(ffm, 62, N, -50.0, 50.0)), dev(_h(ffm, 63, N, 1.0, 1.3)), dev(_h(ffm, 64, N, 1.0, 1.3)), dev(_h(ffm, 65, N, -9.0, 0.0))
    gam, gamb = nat(66, 1e-3, 2e-3), dev(_h(ffm, 67, B, 1e-3, 2e-3))
    phiH, phiHb = nat(32, -0.15, 0.15), dev(_h(ffm, 70, B, -0.1, 0.1))
    f, ref, rg = dev(np.round(_h(ffm, 80, B) * 2) / 2), dev(_h(ffm, 84, B)), dev(_h(ffm, 88, B, -0.5, 0.5))
    ic, bc = ctx.zeros(B), ctx.zeros(B)
    mesh.call("fvm_boundary_coeffs", None, gamb, -1, f, ref, rg, ic, bc)
    up, dO, sO = ctx.zeros(mesh.nNative) + SENTINEL, ctx.zeros(N) + SENTINEL, ctx.zeros(N) + SENTINEL
    mesh.call("fvm_pressure_eqn" + ("_direct" if direct else ""), RDT, psi, psi0, p0, rho, rho0, gh, 1.0e5, gam, phiH, phiHb, ic, bc, up, None, dO, sO)
    return dict(diag=dO, upper=up, lower=None, src=sO, outs=[up, dO, sO])


def _transport(s, ffm, ctx, direct, seed=0, scheme=4, out=None):
    """out: an earlier result whose diag / upper / lower arrays are written again"""
    mesh, N, F = s["mesh"], s["N"], s["F"]
    ph = _h(ffm, 32 + seed, F, -0.15, 0.15)
    ph[::7] = 0.0
    phi, gam, rho = mesh.to_native(ph), mesh.to_native(_h(ffm, 63, F, 0.01, 0.02)), ctx.to_device(_h(ffm, 60, N, 1.0, 2.0))
    d, up, lo = ctx.zeros(N) + SENTINEL, ctx.zeros(mesh.nNative) + SENTINEL, ctx.zeros(mesh.nNative) + SENTINEL
    if out is not None:
        d, up, lo = out["diag"], out["upper"], out["lower"]
    mesh.call("fvm_transport_scheme" + ("_direct" if direct else ""), RDT, rho, phi, scheme, gam, -1, d, up, lo)
    return dict(diag=d, upper=up, lower=lo, src=ctx.to_device(_h(ffm, 44, N, -0.5, 0.5)), outs=[d, up, lo])


def _multi(s, ffm, ctx, direct, seed=0, nf=5):
    """the species' (and h's) assembly under common weights: field 0 alone writes the off-diagonals (nOffDiag = 1)"""
    mesh, N, F, B = s["mesh"], s["N"], s["F"], s["B"]
    dev = ctx.to_device
    ph = _h(ffm, 32 + seed, F, -0.15, 0.15)
    ph[::5] = 0.0
    phi, w = mesh.to_native(ph), mesh.to_native(_h(ffm, 41, F))
    rho, rho0 = dev(1.0 + _h(ffm, 60, N)), dev(1.0 + _h(ffm, 61, N))
    vf0 = [dev(_h(ffm, 62 + i, N)) for i in range(nf)]
    gam, gamb = mesh.to_native(0.01 * (1 + _h(ffm, 63, F))), dev(0.01 * (1 + _h(ffm, 64, B)))
    phib = dev(0.2 * (_h(ffm, 70, B) - 0.5))
    f = [dev(np.round(_h(ffm, 80 + i, B) * 2) / 2) for i in range(nf)]
    ref, rg = [dev(_h(ffm, 84 + i, B)) for i in range(nf)], [dev(_h(ffm, 88 + i, B) - 0.5) for i in range(nf)]
    su = [dev(_h(ffm, 90, N) - 0.3)] * nf
    fac = (C.c_double * nf)(*[0.5 + 0.25 * i for i in range(nf)])
    D, S = [ctx.zeros(N) + SENTINEL for _ in range(nf)], [ctx.zeros(N) + SENTINEL for _ in range(nf)]
    up, lo = ctx.zeros(mesh.nNative) + SENTINEL, ctx.zeros(mesh.nNative) + SENTINEL
    mesh.call("fvm_scalar_transport_multi_ws" + ("_direct" if direct else ""), nf, w, RDT, rho, rho0, phi, phib, gam, gamb, vf0, f, ref, rg, su, fac,
              None, None, None, D, [up] + [None] * (nf - 1), [lo] + [None] * (nf - 1), S)
    return dict(diag=D[0], upper=up, lower=lo, src=S[0], diags=D, srcs=S, outs=[up, lo] + D + S)


ASSEMBLIES = {"pressure": _pressure, "transport": _transport, "multi5": _multi, "multi4": lambda *a, **k: _multi(*a, nf=4, **k)}


def _arrays(A, asym):
    return [A.tile_coef(w) for w in ((0, 1, 2) if asym else (0, 2))]


@pytest.mark.parametrize("kind", list(ASSEMBLIES))
def test_direct_arrays_equal_the_gather_as_bytes(box, ffm, ctx, kind):
    s, A = box, box["A"]
    asym = kind != "pressure"
    plain = ASSEMBLIES[kind](s, ffm, ctx, False)
    g0 = A.tile_gathers()
    d = ASSEMBLIES[kind](s, ffm, ctx, True)
    for a, b in zip(d["outs"], plain["outs"]):                 # the native outputs are those of the plain entry point
        assert _same(a, b)
    A.bind_coeffs_native(d["diag"], d["upper"], d["lower"])
    got = _arrays(A, asym)
    assert A.tile_gathers() == g0                               # nothing gathered: these are the kernel's own stores
    B = s["handle"]()
    B.bind_coeffs_native(plain["diag"], plain["upper"], plain["lower"])
    want = _arrays(B, asym)
    assert B.tile_gathers() == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert _same(a, b), (kind, i, int((_bits(a) != _bits(b)).sum()))
    # the layout itself: the present entries first, then zeros; every count of neighbours from 0 to 3 occurs
    fU, bU = got[0].reshape(-1, 3), got[-1].reshape(-1, 3)
    for t, cnt in ((fU, s["nl"]), (bU, s["nu"])):
        assert set(np.unique(cnt)) == {0, 1, 2, 3}
        assert np.array_equal((t != 0.0).sum(axis=1) <= cnt, np.ones(len(cnt), bool))
        assert all(np.array_equal(_bits(t[cnt <= k, k]), np.zeros(int((cnt <= k).sum()), np.uint64)) for k in range(3))
    # the backward lower array is never written directly: it gathers, and from the same coefficients
    if asym:
        assert _same(A.tile_coef(3), B.tile_coef(3)) and A.tile_gathers() == g0 + 1


def _solve(ctx, A, c, solver, precond, diag=None, **kw):
    psi = ctx.zeros(A.nCells)
    A.bind_coeffs_native(c["diag"] if diag is None else diag, c["upper"], c["lower"])
    perf = A.solve(psi, c["src"], solver=solver, preconditioner=precond, tolerance=1e-9, relTol=0.0, **kw)
    ctx.sync()
    return psi.cpu().numpy(), perf


def _same_solve(a, b):
    return _same(a[0], b[0]) and a[1] == b[1]


SOLVES = [("pressure", "PCG", "DIC", {}), ("transport", "PBiCGStab", "DILU", {}), ("multi5", "PBiCGStab", "DILU", {}),
          ("transport", "smoothSolver", "symGaussSeidel", dict(maxIter=20)), ("pressure", "smoothSolver", "symGaussSeidel", dict(maxIter=20))]


@pytest.mark.parametrize("kind,solver,precond,kw", SOLVES)
def test_solves_on_direct_arrays_equal_the_gather_path(box, ffm, ctx, kind, solver, precond, kw):
    s, A = box, box["A"]
    g0 = A.tile_gathers()
    got = _solve(ctx, A, ASSEMBLIES[kind](s, ffm, ctx, True), solver, precond, **kw)
    assert A.tile_gathers() == g0 and got[1]["nIterations"] >= 2
    B = s["handle"]()
    want = _solve(ctx, B, ASSEMBLIES[kind](s, ffm, ctx, False), solver, precond, **kw)
    assert B.tile_gathers() >= 2
    assert _same_solve(got, want), (got[1], want[1])


@pytest.mark.parametrize("nLanes", [1, 3, 5])
def test_lock_step_lanes_on_direct_arrays(box, ffm, ctx, nLanes):
    s, A = box, box["A"]
    kw = dict(solver="PBiCGStab", preconditioner="DILU", tolerance=1e-9, relTol=0.0)
    res = []
    for direct, M in ((True, A), (False, s["handle"]())):
        c = _multi(s, ffm, ctx, direct)
        g0 = M.tile_gathers()
        psis = [ctx.zeros(s["N"]) for _ in range(nLanes)]
        perf = M.solve_multi(c["diags"][:nLanes], c["upper"], c["lower"], psis, c["srcs"][:nLanes], **kw)
        ctx.sync()
        assert (M.tile_gathers() == g0) if direct else (M.tile_gathers() > g0)
        res.append(([p.cpu().numpy() for p in psis], perf))
    assert res[0][1] == res[1][1] and all(p["nIterations"] >= 1 for p in res[0][1])
    for a, b in zip(res[0][0], res[1][0]):
        assert _same(a, b)


def test_stale_arrays_are_gathered_again(box, ffm, ctx):
    s, A = box, box["A"]
    S, P = ("PBiCGStab", "DILU"), ("PCG", "DIC")
    fresh = lambda c, sp, diag=None: _solve(ctx, s["handle"](), c, *sp, diag=diag)
    t1 = _transport(s, ffm, ctx, True)
    first = _solve(ctx, A, t1, *S)
    # other native coefficients bound without a direct write: gathered
    g = A.tile_gathers()
    x = _transport(s, ffm, ctx, False, seed=5)
    assert not _same(x["upper"], t1["upper"])
    assert _same_solve(_solve(ctx, A, x, *S), fresh(x, S)) and A.tile_gathers() > g
    # and the other way round: direct again, symmetric this time, then asymmetric
    g = A.tile_gathers()
    p1 = _pressure(s, ffm, ctx, True)
    assert _same_solve(_solve(ctx, A, p1, *P), fresh(_pressure(s, ffm, ctx, False), P)) and A.tile_gathers() == g
    assert _same_solve(_solve(ctx, A, _transport(s, ffm, ctx, True), *S), first) and A.tile_gathers() == g
    # offDiagUnchanged after a direct write keeps the arrays: another diagonal on the same off-diagonals
    t2 = _transport(s, ffm, ctx, True)
    _solve(ctx, A, t2, *S)
    d2 = t2["diag"] * 1.25
    psi = ctx.zeros(s["N"])
    A.bind_coeffs_native(d2, t2["upper"], t2["lower"], offDiagUnchanged=True)
    perf = A.solve(psi, t2["src"], solver=S[0], preconditioner=S[1], tolerance=1e-9, relTol=0.0)
    ctx.sync()
    assert A.tile_gathers() == g and _same_solve((psi.cpu().numpy(), perf), fresh(t2, S, diag=d2))
    # a direct write whose arrays are NOT the ones bound next: the declaration is dropped, the arrays are gathered
    _transport(s, ffm, ctx, True, seed=9)
    assert _same_solve(_solve(ctx, A, x, *S), fresh(x, S)) and A.tile_gathers() > g
    # a direct write, then a plain assembly that refills the SAME arrays with other coefficients: the triples are not theirs
    g = A.tile_gathers()
    t3 = _transport(s, ffm, ctx, True)
    t3 = _transport(s, ffm, ctx, False, seed=5, out=t3)
    assert _same(t3["upper"], x["upper"]) and _same_solve(_solve(ctx, A, t3, *S), fresh(x, S)) and A.tile_gathers() > g
    # ... also where the bind says offDiagUnchanged (the caller's claim is about the native arrays; the plan's were overwritten)
    g = A.tile_gathers()
    _transport(s, ffm, ctx, True, seed=9)
    psi = ctx.zeros(s["N"])
    A.bind_coeffs_native(x["diag"], x["upper"], x["lower"], offDiagUnchanged=True)
    perf = A.solve(psi, x["src"], solver=S[0], preconditioner=S[1], tolerance=1e-9, relTol=0.0)
    ctx.sync()
    assert _same_solve((psi.cpu().numpy(), perf), fresh(x, S)) and A.tile_gathers() > g


def _refused(s, ffm, ctx):
    """all three direct forms refuse, nothing written; the plain forms then give what a handle that never asked gives"""
    A = s["A"]
    for kind, fn in ASSEMBLIES.items():
        with pytest.raises(ffm.FfmError, match=UNSUPPORTED):
            fn(s, ffm, ctx, True)
    mesh, N = s["mesh"], s["N"]
    d, up, lo = ctx.zeros(N) + SENTINEL, ctx.zeros(mesh.nNative) + SENTINEL, ctx.zeros(mesh.nNative) + SENTINEL
    one = ctx.zeros(mesh.nNative) + 0.01
    with pytest.raises(ffm.FfmError, match=UNSUPPORTED):
        mesh.call("fvm_transport_scheme_direct", RDT, ctx.zeros(N) + 1.0, one, 4, one, -1, d, up, lo)
    for o in (d, up, lo):
        assert np.array_equal(_bits(o), np.full(o.numel(), SENTINEL).view(np.uint64))
    return A


def test_rows_wider_than_the_plan_are_refused(ffm, ctx):
    s = MM.device_mesh(ffm, ctx, MM.case("w4"))
    s["handles"] = []
    try:
        assert s["W"] == 4
        A = _refused(s, ffm, ctx)
        c = _transport(s, ffm, ctx, False)
        got = _solve(ctx, A, c, "PBiCGStab", "DILU")
        B = ffm.lduMatrix(ctx, s["N"], s["l"], s["u"]); s["handles"].append(B)
        assert _same_solve(got, _solve(ctx, B, c, "PBiCGStab", "DILU")) and got[1]["nIterations"] >= 2
    finally:
        s["mesh"].close(); s["A"].close()
        for B in s["handles"]:
            B.close()


def test_a_matrix_without_a_tile_plan_is_refused(ffm, ctx):
    os.environ["FFM_SWEEP"] = "levels"
    try:
        s = _box_levels(ffm, ctx)
    finally:
        os.environ.pop("FFM_SWEEP", None)
    try:
        A = _refused(s, ffm, ctx)
        with pytest.raises(ffm.FfmError, match=UNSUPPORTED):
            A.tile_coef(0)
        c = _transport(s, ffm, ctx, False)
        got = _solve(ctx, A, c, "PBiCGStab", "DILU")
        assert got[1]["nIterations"] >= 2 and got[1]["converged"] == 1 and A.tile_gathers() == 0
    finally:
        s["mesh"].close(); s["A"].close()


def _box_levels(ffm, ctx):
    from oracle import plume
    m = plume.make_mesh((9, 8, 7), h=0.1)
    s = MM.device_mesh(ffm, ctx, m)
    assert s["A"].sweep_mode != 2
    return s


def test_a_block_with_ghost_cells_is_refused(ffm, ctx):
    """the cells of the last z-plane of a box as the ghost cells of the rest (the faces among them are no faces of the block)"""
    from oracle import plume
    n = (16, 16, 6)
    m = plume.make_mesh(n, h=0.1)
    nOwn = n[0] * n[1] * (n[2] - 1); nGhost = m.nCells - nOwn
    keep = m.l < nOwn
    l, u = m.l[keep], m.u[keep]
    hint = np.zeros(nOwn, np.int32)                 # one tile: with a group hint a block with ghost cells gets a tile plan
    cOrd, fOrd = ffm.renumber_levels(nOwn, l, u, groupHint=hint, nGhost=nGhost)
    l2, u2, oldToNew = ffm.hexmesh.apply_renumbering(m.nCells, l, u, cOrd, fOrd)
    A = ffm.lduMatrix(ctx, nOwn, l2, u2, groupHint=hint[cOrd[:nOwn]], nGhost=nGhost)
    gface = np.nonzero(keep)[0][fOrd]
    pk = [p.faceCells < nOwn for p in m.patches]
    patches = [(oldToNew[p.faceCells[k]].astype(np.int32), p.Sf[k].T.copy(), p.deltaCoeffs[k]) for p, k in zip(m.patches, pk)]
    mesh = ffm.fvMesh(A, m.V[cOrd], m.C[cOrd].T.copy(), m.Sf[gface].T.copy(), m.magSf[gface], m.weights[gface], m.deltaCoeffs[gface], patches)
    try:
        assert A.sweep_mode == 2                    # the plan is there; the ghost cells are the reason
        s = dict(A=A, mesh=mesh, N=m.nCells, F=int(keep.sum()), B=sum(int(k.sum()) for k in pk))
        _refused(s, ffm, ctx)
    finally:
        mesh.close(); A.close()
