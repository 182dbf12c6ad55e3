"""The set-up of a solve without its separate vector passes (csrc/ffm_solve.hip: k_prologue; csrc/ffm_tile.hip: the tiled
calcReciprocalD stores 1/D itself).

(a) calcReciprocalD through the tiled sweeps -- one system (k_tile<TM_RD, 1>) and several systems in one sweep (k_tile<TM_RD, NF>) --
    gives rD BITWISE equal to the reciprocal of the oracle's face loop (oracle/ffo_precond.c): one system on the meshes of
    test_ldu_gpu.py; several systems on boxes in the library's own cell order, which the lock-step form requires (its `hex_big` box
    among them).
(b) PCG + DIC and PBiCGStab + DILU / DIC, one solve at a time and through ffm_solve_multi_d (PBiCGStab: lock step), against the oracle
    with the bars of test_ldu_gpu.py::test_solver_parity: equal iteration counts, initial residual to 1e-12 relative, final residual
    to 5 % + 2e-12 (tree sums against serial sums), fields to 1e-8 rel-L2.  The merged meshes `w4`, `w16u14`, `w32l30`, `w32multi`
    (tests/merged_mesh.py) bring the W = 4, 16 and 32 instantiations of k_flow_sweep and of the prologue's row kernels.  One system starts from its solution: no iteration, the
    field untouched (its residual is rounding noise of the Amul, so only `below the tolerance` is asked of it); the lock-step lanes
    stop at different iterations."""
import os

import numpy as np
import pytest

from common import laplacian_like, rel_l2
from test_ldu_gpu import _make_case

pytestmark = pytest.mark.gpu

CASES = ["hex_natural", "hex_levelmajor", "dag_random", "chain", "plane", "hex_levelmajor_t41", "hex_natural_t29", "plane_t17",
         "hex_natural_t37", "dag_random_t23", "chain_t64", "plane_t50", "hex_natural_t500", "hex_tiles_t0", "hex_big", "hex_baffled_t0",
         "w4", "w16u14", "w32l30", "w32multi"]


@pytest.fixture(scope="module", params=CASES)
def case(request, O, ffm, ctx):
    name, grp = request.param, None
    if "_t" in name:
        name, grp = name.rsplit("_t", 1)
        if grp != "0":
            os.environ["FFM_PIPE_GROUP_CELLS"] = grp
        os.environ["FFM_SWEEP"] = "tile"
    try:
        yield from _make_case(name, grp, O, ffm, ctx)
    finally:
        os.environ.pop("FFM_PIPE_GROUP_CELLS", None)
        os.environ.pop("FFM_SWEEP", None)


@pytest.mark.parametrize("precond,asym", [("DIC", 0.0), ("DILU", 0.35), ("DILU", 0.0)])
def test_reciprocalD_single_bit_exact(O, ctx, case, precond, asym):
    name, N, l, u, A = case
    diag, up, lo = laplacian_like(O, N, l, u, seed=7, asym=asym, shift=0.05)
    A.set_coeffs(diag, up, lo)
    Ao = O.Ldu(N, l, u).set_coeffs(diag, up, lo)
    rD = Ao.dic_rD() if precond == "DIC" else Ao.dilu_rD()
    got = A.reciprocalD(precond).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), rD.view(np.uint64)), np.abs(got - rD).max()


def _native_box(ffm, ctx, n, asym, seed):
    """a box in the library's cell order with a tile plan (as tests/test_solve_multi_gpu.py builds it)"""
    rng = np.random.default_rng(seed)
    N, l, u = ffm.hexmesh.hex_ldu(*n)
    cOrd, fOrd = ffm.renumber_levels(N, l, u)
    l2, u2, _ = ffm.hexmesh.apply_renumbering(N, l, u, cOrd, fOrd)
    A = ffm.lduMatrix(ctx, N, l2, u2)
    assert A.sweep_mode == 2 and A.native_order
    F = l2.size
    g = rng.uniform(0.5, 1.5, F)
    phi = rng.normal(0.0, 0.6, F) if asym else np.zeros(F)
    upper, lower = -g + 0.5 * phi, -g - 0.5 * phi
    base = np.zeros(N)
    np.add.at(base, l2, -lower); np.add.at(base, u2, -upper)
    fmap = A.face_map()
    nat = lambda f: (lambda out: (out.__setitem__(fmap, f), out)[1])(np.zeros(A.nNative))
    up_d = ctx.to_device(nat(upper))
    lo_d = ctx.to_device(nat(lower)) if asym else None
    return A, N, l2, u2, upper, lower, base, rng, up_d, lo_d


def _diags(base, rng, N, nSys):
    return [base * (1.0 + 0.02 * 4.0 ** i * rng.uniform(0.5, 1.5, N)) + (10.0 if i == 2 else 0.02) * rng.uniform(0.0, 1.0, N) for i in range(nSys)]


@pytest.mark.parametrize("n,nSys,asym", [((23, 37, 41), 4, True), ((23, 37, 41), 3, False), ((33, 17, 29), 2, True), ((24, 20, 18), 2, False)])
def test_reciprocalD_multi_lane_bit_exact(O, ffm, ctx, n, nSys, asym):
    A, N, l, u, upper, lower, base, rng, up_d, lo_d = _native_box(ffm, ctx, n, asym, seed=sum(n) + nSys)
    diags = _diags(base, rng, N, nSys)
    dd = [ctx.to_device(d) for d in diags]
    A.bind_coeffs_native(dd[0], up_d, lo_d)
    precond = "DILU" if asym else "DIC"
    got = A.reciprocalD_multi(precond, dd)
    for i in range(nSys):
        Ao = O.Ldu(N, l, u).set_coeffs(diags[i], upper, lower if asym else None)
        rD = Ao.dilu_rD() if asym else Ao.dic_rD()
        g = got[i].cpu().numpy()
        assert np.array_equal(g.view(np.uint64), rD.view(np.uint64)), (i, np.abs(g - rD).max())
        # the same lane alone (k_tile<TM_RD>)
        A.bind_coeffs_native(dd[i], up_d, lo_d)
        assert np.array_equal(A.reciprocalD(precond).cpu().numpy().view(np.uint64), rD.view(np.uint64)), i
    A.close()


def _parity(pg, pr, got, ref, entry_converged, tol):
    assert pg["nIterations"] == pr["nIterations"], (pg, pr)
    assert pg["converged"] == 1 and pr["converged"] == 1
    if entry_converged:
        assert pg["nIterations"] == 0 and pg["initialResidual"] < tol and pr["initialResidual"] < tol
        assert pg["finalResidual"] == pg["initialResidual"]
        return
    assert abs(pg["initialResidual"] - pr["initialResidual"]) <= 1e-12 * pr["initialResidual"], (pg, pr)
    assert abs(pg["finalResidual"] - pr["finalResidual"]) <= 0.05 * pr["finalResidual"] + 2e-12, (pg, pr)
    assert rel_l2(got, ref) < 1e-8


def _amul(l, u, d, upper, lower, x):
    y = d * x
    np.add.at(y, u, lower * x[l]); np.add.at(y, l, upper * x[u])
    return y


@pytest.mark.parametrize("solver,precond,asym", [("PCG", "DIC", 0.0), ("PBiCGStab", "DILU", 0.35), ("PBiCGStab", "DILU", 0.0)])
def test_single_solves_match_oracle(O, ctx, case, solver, precond, asym):
    name, N, l, u, A = case
    diag, up, lo = laplacian_like(O, N, l, u, seed=3, asym=asym, shift=0.05)
    A.set_coeffs(diag, up, lo)
    Ao = O.Ldu(N, l, u).set_coeffs(diag, up, lo)
    os_, op_ = getattr(O, {"PCG": "PCG", "PBiCGStab": "PBICGSTAB"}[solver]), getattr(O, precond)
    kw = dict(tolerance=1e-11, relTol=0.0, maxIter=3000)
    b = 2 * O.hash_u(0xF3, np.arange(N)) - 1
    ref, pr = Ao.solve(os_, op_, np.zeros(N), b, **kw)
    psi = ctx.zeros(N)
    pg = A.solve(psi, ctx.to_device(b), solver=solver, preconditioner=precond, **kw)
    _parity(pg, pr, psi.cpu().numpy(), ref, False, kw["tolerance"])
    # converged on entry: the right-hand side is A x for the start value x
    x = 2 * O.hash_u(0xA7, np.arange(N)) - 1
    bx = Ao.amul(x)
    kw0 = dict(tolerance=1e-9, relTol=0.0, maxIter=3000)
    ref0, pr0 = Ao.solve(os_, op_, x.copy(), bx, **kw0)
    psi0 = ctx.to_device(x)
    pg0 = A.solve(psi0, ctx.to_device(bx), solver=solver, preconditioner=precond, **kw0)
    _parity(pg0, pr0, None, None, True, kw0["tolerance"])
    assert np.array_equal(psi0.cpu().numpy().view(np.uint64), x.view(np.uint64)) and np.array_equal(ref0, x)


@pytest.mark.parametrize("n,nSys,solver,asym", [((24, 20, 18), 3, "PBiCGStab", True), ((33, 17, 29), 4, "PBiCGStab", True),
                                                ((20, 16, 24), 4, "PBiCGStab", False), ((20, 20, 20), 2, "PBiCGStab", True),
                                                ((20, 16, 24), 3, "PCG", False)])
def test_multi_solves_match_oracle(O, ffm, ctx, n, nSys, solver, asym):
    A, N, l, u, upper, lower, base, rng, up_d, lo_d = _native_box(ffm, ctx, n, asym, seed=sum(n) + nSys)
    diags = _diags(base, rng, N, nSys)
    srcs, psi0 = [], []
    for i in range(nSys):
        x = rng.standard_normal(N)
        srcs.append(_amul(l, u, diags[i], upper, lower, x) if i == 1 else rng.standard_normal(N))
        psi0.append(x if i == 1 else np.zeros(N))
    precond = "DILU" if asym else "DIC"
    tol = 1e-9
    dev = lambda a: ctx.to_device(a)
    dd, pp, ss = [dev(a) for a in diags], [dev(a) for a in psi0], [dev(a) for a in srcs]
    perf = A.solve_multi(dd, up_d, lo_d, pp, ss, solver=solver, preconditioner=precond, tolerance=tol, relTol=0.0)
    ctx.sync()
    counts = [p["nIterations"] for p in perf]
    assert counts[1] == 0 and len(set(counts)) >= 2, counts            # lanes stop at different iterations, one never starts
    os_ = getattr(O, {"PCG": "PCG", "PBiCGStab": "PBICGSTAB"}[solver])
    for i in range(nSys):
        Ao = O.Ldu(N, l, u).set_coeffs(diags[i], upper, lower if asym else None)
        ref, pr = Ao.solve(os_, getattr(O, precond), psi0[i].copy(), srcs[i], tolerance=tol, relTol=0.0)
        got = pp[i].cpu().numpy()
        _parity(perf[i], pr, got, ref, i == 1, tol)
        if i == 1:
            assert np.array_equal(got.view(np.uint64), psi0[i].view(np.uint64))
    A.close()
