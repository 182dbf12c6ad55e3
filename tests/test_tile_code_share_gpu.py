"""Tile plans whose entries share their neighbour-code blocks (csrc/ffm_tile.hip, csrc/ffm_tile_share.cpp) against plans that give every entry
a block of its own (FFM_TILE_CODE_SHARE=0, read when the plan is built: the per-cell layout byte for byte).  The kernels are the same ones, so
every result must be equal as uint64 -- and equal to the serial face loops of the oracle where tests/test_ldu_gpu.py holds the library to them:

* DIC and DILU application (DILU also transposed), calcReciprocalD, the Gauss-Seidel and symmetric Gauss-Seidel sweeps;
* the lock-step sweeps of 2, 3 and 5 systems (5: the 2048 ring), as calcReciprocalD of several diagonals and as PBiCGStab + DILU solves;
* the tiled Amul, symmetric and asymmetric;
* PCG + DIC with the fused iteration: same iterates, same iteration count.

Shapes: an 80 x 32 x 32 box = four 16 x 16 column tiles of 110 levels (the 4096 ring wraps five times, entry parity alternates, full levels
repeat: the pools must come out smaller than the arrays); 40 x 20 x 18 and 5 x 33 x 17 (tiles that are not 16 wide, levels that are never full);
chunk groups (FFM_PIPE_GROUP_CELLS); a hinted box with a fifth of its faces removed and a polyhedral mesh with a wide row (nothing repeats, or no
tile plan at all); one rank's block of a decomposed box, with ghost cells."""
import os

import numpy as np
import pytest

import merged_mesh as MM
from common import laplacian_like, rel_l2

pytestmark = pytest.mark.gpu

CASES = {
    # name: (mesh, environment while renumbering and creating, expects a tile plan)
    "box_80x32x32": (("hex", (80, 32, 32)), {}, True),
    "box_40x20x18": (("hex", (40, 20, 18)), {}, True),
    "box_5x33x17": (("hex", (5, 33, 17)), {}, True),
    "chunks37": (("hex", (9, 7, 8)), {"FFM_SWEEP": "tile", "FFM_PIPE_GROUP_CELLS": "37"}, True),
    "chunks500": (("hex", (23, 37, 41)), {"FFM_SWEEP": "tile", "FFM_PIPE_GROUP_CELLS": "500"}, True),
    "baffled_hint": (("baffled", (11, 13, 12)), {}, True),
    "poly_w4": (("merged", "w4"), {"FFM_SWEEP": "tile", "FFM_PIPE_GROUP_CELLS": "29"}, False),
    "ghost_block": (("ghost", (12, 10, 8)), {"FFM_SWEEP": "tile", "FFM_PIPE_GROUP_CELLS": "41"}, True),
}


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in ("FFM_SWEEP", "FFM_PIPE_GROUP_CELLS", "FFM_TILE_CODE_SHARE")}
        for k in self.old:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _mesh(O, ffm, kind, arg, env):
    """(nOwned, nGhost, l, u, hint) in the library's own cell order where it offers one"""
    hint, nGhost = None, 0
    if kind == "merged":
        m = MM.case(arg)
        return m.nCells, 0, m.l.astype(np.int32), m.u.astype(np.int32), None
    N, l, u = O.hex_ldu(*arg)
    if kind == "ghost":
        S = ffm.decompose.SubDomain(N, l, u, ffm.decompose.partition_graph(N, l, u, 2), 2, 0)
        assert S.nGhost > 0
        return S.nOwned, S.nGhost, S.l, S.u, None
    if kind == "baffled":
        nx, ny, nz = arg
        keep = O.hash_u(0xBAF, np.arange(len(l))) > 0.2
        l, u = l[keep], u[keep]
        c = np.arange(N)
        hint = (((c // nx) % ny) // 3 + 10 * ((c // (nx * ny)) // 3)).astype(np.int32)
    with _Env(env):
        cOrd, fOrd = ffm.renumber_levels(N, l, u, groupHint=hint)
    l2, u2, _ = ffm.hexmesh.apply_renumbering(N, l, u, cOrd, fOrd)
    return N, 0, l2.astype(np.int32), u2.astype(np.int32), (None if hint is None else hint[cOrd])


def _results(O, ffm, ctx, name, share):
    """every operation on a handle of its own, made with or without sharing: {label: float64 array}, the figures, the sweep mode"""
    (kind, arg), env, _ = CASES[name]
    N, nGhost, l, u, hint = _mesh(O, ffm, kind, arg, env)
    nAll = N + nGhost
    with _Env(dict(env, **({} if share else {"FFM_TILE_CODE_SHARE": "0"}))):
        A = ffm.lduMatrix(ctx, N, l, u, groupHint=hint, nGhost=nGhost)
    out, host = {}, lambda t: (ctx.sync(), t.cpu().numpy().copy())[1]
    tiled = A.sweep_mode == 2
    figures = [A.tile_code_bytes(w) for w in range(3)] if tiled else None
    cells = np.arange(nAll)
    r = 2 * O.hash_u(11, cells) - 1
    x = 2 * O.hash_u(0xF4, cells) - 0.7
    psi0, b = O.hash_u(13, cells), O.hash_u(14, cells)
    own = lambda a: np.concatenate([a[:N], np.zeros(nGhost)])       # coefficients: nothing on the ghost cells' diagonal
    # ---- symmetric coefficients
    diag, up, _ = laplacian_like(O, nAll, l, u, seed=3, asym=0.0, shift=0.05)
    A.set_coeffs(own(diag), up, None)
    out["dic_rD"] = host(A.reciprocalD("DIC"))
    out["dic"] = host(A.precondition("DIC", ctx.to_device(r)))
    out["amul_sym"] = host(A.Amul(ctx.to_device(x)))
    if not nGhost:
        out["symgs"] = host(A.smooth(ctx.to_device(psi0), ctx.to_device(b), nSweeps=2, smoother="symGaussSeidel"))
        psi = ctx.zeros(N)
        p = A.solve(psi, ctx.to_device(2 * b - 1), tolerance=0.0, minIter=5, maxIter=5)
        out["pcg5"] = host(psi); out["pcg5_perf"] = np.array([p["nIterations"], p["initialResidual"], p["finalResidual"]])
        psi = ctx.zeros(N)
        p = A.solve(psi, ctx.to_device(2 * b - 1), tolerance=1e-10, maxIter=500)
        assert p["converged"] == 1
        out["pcg"] = host(psi); out["pcg_perf"] = np.array([p["nIterations"], p["initialResidual"], p["finalResidual"]])
    # ---- asymmetric coefficients
    diagA, upA, loA = laplacian_like(O, nAll, l, u, seed=3, asym=0.35, shift=0.05)
    A.set_coeffs(own(diagA), upA, loA)
    out["dilu_rD"] = host(A.reciprocalD("DILU"))
    out["dilu"] = host(A.precondition("DILU", ctx.to_device(r)))
    out["diluT"] = host(A.precondition("DILU", ctx.to_device(r), transpose=True))
    out["amul_asym"] = host(A.Amul(ctx.to_device(x)))
    if not nGhost:
        out["gs"] = host(A.smooth(ctx.to_device(psi0), ctx.to_device(b), nSweeps=2, smoother="GaussSeidel"))
        out["symgs_asym"] = host(A.smooth(ctx.to_device(psi0), ctx.to_device(b), nSweeps=2, smoother="symGaussSeidel"))
    # ---- lock-step systems (tiled matrices in the library's order): common off-diagonals, five diagonals
    if tiled and not nGhost and A.native_order:
        fmap = A.face_map()
        nat = lambda f: (lambda o: (o.__setitem__(fmap, f), o)[1])(np.zeros(A.nNative))
        up_d, lo_d = ctx.to_device(nat(upA)), ctx.to_device(nat(loA))
        diags = [diagA * (1.0 + 0.02 * 4.0 ** i * (0.5 + O.hash_u(40 + i, cells))) for i in range(5)]
        for n in (2, 3, 5):
            dd = [ctx.to_device(d) for d in diags[:n]]
            A.bind_coeffs_native(dd[0], up_d, lo_d)
            for i, t in enumerate(A.reciprocalD_multi("DILU", dd)):
                out["rD_multi%d_%d" % (n, i)] = host(t)
            pp = [ctx.zeros(N) for _ in range(n)]
            ss = [ctx.to_device(2 * O.hash_u(60 + i, cells) - 1) for i in range(n)]
            perf = A.solve_multi(dd, up_d, lo_d, pp, ss, solver="PBiCGStab", preconditioner="DILU", tolerance=1e-9, maxIter=40)
            for i in range(n):
                out["multi%d_%d" % (n, i)] = host(pp[i])
                out["multi%d_%d_perf" % (n, i)] = np.array([perf[i]["nIterations"], perf[i]["initialResidual"], perf[i]["finalResidual"]])
            A.unbind_coeffs()
    A.close()
    if nGhost:          # the operators write the owned rows; the ghost entries of their outputs are whatever the allocation held
        out = {k: v[:N] for k, v in out.items()}
    return out, figures, tiled, (N, nGhost, l, u, (diag, up), (diagA, upA, loA), (r, x, psi0, b))


@pytest.fixture(scope="module")
def runs(O, ffm, ctx):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = (_results(O, ffm, ctx, name, True), _results(O, ffm, ctx, name, False))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_shared_and_unshared_plans_give_the_same_bytes(runs, name):
    (on, figOn, tiledOn, _), (off, figOff, tiledOff, _) = runs(name)
    assert tiledOn == tiledOff == CASES[name][2]
    assert sorted(on) == sorted(off) and len(on) >= 7
    if tiledOn and name not in ("ghost_block",):
        assert any(k.startswith("multi5_") for k in on), sorted(on)          # the lock-step sweeps ran
    for k in sorted(on):
        assert on[k].shape == off[k].shape, (name, k)
        bad = np.nonzero(on[k].view(np.uint64) != off[k].view(np.uint64))[0]
        assert bad.size == 0, (name, k, "%d of %d differ, first at %d" % (bad.size, on[k].size, bad[0]))


@pytest.mark.parametrize("name", [n for n in CASES if n != "ghost_block"])
def test_shared_plans_against_the_serial_face_loops(O, runs, name):
    (on, _, _, (N, nGhost, l, u, (diag, up), (diagA, upA, loA), (r, x, psi0, b))), _ = runs(name)
    Ao = O.Ldu(N, l, u).set_coeffs(diag, up, None)
    rD = Ao.dic_rD()
    assert np.array_equal(on["dic_rD"], rD)
    assert np.array_equal(on["dic"], Ao.dic_precondition(rD, r))
    assert np.array_equal(on["amul_sym"], Ao.amul(x))
    assert np.array_equal(on["symgs"], Ao.gs_smooth(psi0, b, nSweeps=2, sym=True))
    ref, pr = Ao.solve(O.PCG, O.DIC, np.zeros(N), 2 * b - 1, tolerance=0.0, minIter=5, maxIter=5)
    assert on["pcg5_perf"][0] == pr["nIterations"] == 5 and rel_l2(on["pcg5"], ref) < 1e-12
    ref, pr = Ao.solve(O.PCG, O.DIC, np.zeros(N), 2 * b - 1, tolerance=1e-10, maxIter=500)
    assert on["pcg_perf"][0] == pr["nIterations"] and rel_l2(on["pcg"], ref) < 1e-8
    Ao = O.Ldu(N, l, u).set_coeffs(diagA, upA, loA)
    rD = Ao.dilu_rD()
    assert np.array_equal(on["dilu_rD"], rD)
    assert np.array_equal(on["dilu"], Ao.dilu_precondition(rD, r))
    assert np.array_equal(on["diluT"], Ao.dilu_precondition(rD, r, transpose=True))
    assert np.array_equal(on["amul_asym"], Ao.amul(x))
    assert np.array_equal(on["gs"], Ao.gs_smooth(psi0, b, nSweeps=2, sym=False))
    assert np.array_equal(on["symgs_asym"], Ao.gs_smooth(psi0, b, nSweeps=2, sym=True))


def test_the_figures(runs):
    """On the box of full 16 x 16 tiles the three pools are smaller than the arrays they replace; switched off, unique == total; the total is
    what one array per cell held (8 B per cell and direction, 16 B per cell for the Amul) whichever way the plan was built."""
    (_, figOn, _, (N, *_)), (_, figOff, _, _) = runs("box_80x32x32")
    print("code bytes (unique, total) forward / backward / Amul:", figOn, "switched off:", figOff)
    for w in range(3):
        assert 0 < figOn[w][0] < figOn[w][1] == figOff[w][1] == figOff[w][0] == (16 if w == 2 else 8) * N, (w, figOn, figOff)
    for name in CASES:
        (_, figOn, tiled, (N, *_)), (_, figOff, _, _) = runs(name)
        if not tiled:
            continue
        for w in range(3):
            assert figOff[w][0] == figOff[w][1] == figOn[w][1] and 0 <= figOn[w][0] <= figOn[w][1], (name, w, figOn, figOff)
            assert figOn[w][1] in ((16 if w == 2 else 8) * N, 0), (name, w, figOn)          # (0: no ring plan for the tiled Amul)
