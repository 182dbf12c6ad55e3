"""The processor-interface form of the device lduMatrix (ffm_ldu_set_interfaces: OpenFOAM's faceCells / interfaceBouCoeffs /
interfaceIntCoeffs / neighbProcNo per processor patch, applied in (patch, face) order after the exchange) against the oracle's
ranks in the same form (oracle/ffo_ldu.c update_interfaces, oracle/ffo_precond.c ffo_gs_smooth).

In-process part: one process, a fresh Context per emulated rank with comm_init_host(rank, world, ...) and the exchange of
tests/iface_cases.py, which hands both sides the same neighbour values.  Every comparison is BITWISE: the rows are bit-exact
already (tests/test_ldu_gpu.py) and the interface part is acc -/+ coeff*val per cell in (patch, face) order on both sides, FMA
contraction off.  That the oracle's ranks are right is shown by tests/test_ldu_interfaces_cpu.py and
tests/test_decomposed_gloo_cpu.py.

Multi-process part: tests/workers/part_rank.py mode "gpu_if" (ranks sharing cuda:0 over gloo) against mode "oracle" on the same
decomposition -- the same form on both sides, so a smoother call is bitwise and the solvers differ by the order of their dot
products only (bars of tests/test_ldu_gpu.py::test_solver_parity and tests/test_partition_gpu.py)."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import iface_cases as IC
import part_cases
from common import rel_l2, free_port
from test_partition_gpu import _run_ranks

pytestmark = pytest.mark.gpu

FFM_ERR_ARG, FFM_ERR_UNSUPPORTED = -1, -5


class Env:
    """environment variables around the creation of a handle (FFM_SWEEP, FFM_PIPE_GROUP_CELLS are read there)"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class DeviceRank:
    """one emulated rank on the device: its own Context on the host transport, the in-process exchange, the oracle's twin"""

    def __init__(self, O, ffm, case, rk, env=None, interfaces=True):
        self.O, self.rk, self.N = O, rk, case.N
        self.ex, self.exo = IC.Exchange(rk), IC.Exchange(rk)
        self.ctx = ffm.Context(0)
        self.ctx.comm_init_host(rk.rank, rk.world, IC.Exchange.allreduce, self.ex.device_fn())
        with Env(**(env or {})):
            self.A = ffm.lduMatrix(self.ctx, rk.nOwned, rk.l, rk.u)
        self.A.set_coeffs(rk.diag, rk.upper, rk.lower)
        if interfaces:
            self.A.set_interfaces(rk.faceCells, rk.bou, rk.nbrRank, intCoeffs=rk.int_, globalCells=case.N)
        self.Ao = rk.oracle(O, case.N)
        self.Ao.comm, self._keep = self.exo.oracle_comm(O)

    def both(self, x):
        """the global vector whose neighbour values the two exchanges hand out"""
        self.ex.x = self.exo.x = x

    def plain(self):
        """the oracle's matrix without the interfaces"""
        rk = self.rk
        return self.O.Ldu(rk.nOwned, rk.l, rk.u).set_coeffs(rk.diag, rk.upper, rk.lower)

    def close(self):
        self.A.close(); self.ctx.close()


def _ranks(case):
    return [rk for rk in case.ranks if rk is not None]


def _row_operations(O, ffm, case, env=None, mode=None, native=None):
    x, b = IC.vectors(O, case.N)
    gathered = np.full(case.N, np.nan)
    for rk in _ranks(case):
        D = DeviceRank(O, ffm, case, rk, env)
        try:
            A, Ao, ctx = D.A, D.Ao, D.ctx
            if mode is not None:
                assert A.sweep_mode == mode, (rk.rank, A.sweep_mode)
            if native is not None:
                assert A.native_order == native, rk.rank
            D.both(x)
            xl, bl = x[rk.gcell], b[rk.gcell]
            xd, bd = ctx.to_device(xl), ctx.to_device(bl)
            packed = np.concatenate([xl[fc] for fc in rk.faceCells])          # x[faceCells] in the caller's numbering, patch after patch
            y = A.Amul(xd).cpu().numpy()
            assert D.ex.calls == 1 and D.ex.ranks == rk.nbrRank
            assert D.ex.sent.tobytes() == packed.tobytes()                      # k_halo_pack through the old -> new cell map
            assert np.array_equal(y, Ao.amul(xl))
            gathered[rk.gcell] = y
            D.ex.sent = None
            assert np.array_equal(A.Tmul(xd).cpu().numpy(), Ao.tmul(xl))        # interfaceIntCoeffs
            assert D.ex.calls == 2 and D.ex.sent.tobytes() == packed.tobytes()
            assert np.array_equal(A.residual(xd, bd).cpu().numpy(), Ao.residual(xl, bl))
            assert D.ex.calls == 3
            assert np.array_equal(A.sumA().cpu().numpy(), Ao.sumA())
            assert D.ex.calls == 3                                              # sumA exchanges nothing
            if rk.int_ is not None:                                             # interfaceIntCoeffs are other numbers: a mixed-up array shows
                assert all(len(i) == 0 or not np.array_equal(i, c) for i, c in zip(rk.int_, rk.bou))
        finally:
            D.close()
    if case.glob is not None:
        assert rel_l2(gathered, case.global_oracle(O).amul(x)) < 1e-14


@pytest.mark.parametrize("name", IC.CASES)
def test_row_operations_bitwise_on_every_rank(O, ffm, ctx, name):
    """Amul, Tmul, residual and sumA of every rank of every case (slab: the middle block, whose 266 240 boundary cells and 532 480 packed
    items run the grid-stride loops of k_halo_pack / k_halo_apply past their 1024 x 256 threads)"""
    case = IC.build(O, ffm, name)
    _row_operations(O, ffm, case, native=False if name.startswith("dag") else None)


# FFM_SWEEP=tile with small groups: the relabelled box has cells with more than 3 upper neighbours, which the tile planner does not take
# (the handle falls back to the level-scheduled sweeps, as `dag_random_t23` of tests/test_ldu_gpu.py does); the blocks in chunks of 5
# cells are tiled, 3 or 4 groups each
SWEEPS = [("blocks222", {"FFM_SWEEP": "levels"}, 0), ("dag2r", {"FFM_SWEEP": "tile", "FFM_PIPE_GROUP_CELLS": "23"}, 0),
          ("blocks222", {"FFM_SWEEP": "tile", "FFM_PIPE_GROUP_CELLS": "5"}, 2)]


@pytest.mark.parametrize("name,env,mode", SWEEPS)
def test_row_operations_in_both_sweep_modes(O, ffm, ctx, name, env, mode):
    _row_operations(O, ffm, IC.build(O, ffm, name), env=env, mode=mode)


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("name,env,mode", [("blocks222", {}, 2), ("dag4g", {}, 0)] + SWEEPS)
def test_one_smoother_sweep_bitwise(O, ffm, ctx, name, env, mode, sym):
    """bPrime = source + interfaceBouCoeffs * neighbour values before the sweep (ffm_gs_smooth_i), tiled and level-scheduled"""
    case = IC.build(O, ffm, name)
    psi0, b = O.hash_u(0xF5, np.arange(case.N)) + 0.25, O.hash_u(0xF3, np.arange(case.N)) - 0.4
    for rk in case.ranks:
        D = DeviceRank(O, ffm, case, rk, env)
        try:
            assert D.A.sweep_mode == mode, (rk.rank, D.A.sweep_mode)
            D.both(psi0)
            pl, bl = psi0[rk.gcell], b[rk.gcell]
            got = D.A.smooth(D.ctx.to_device(pl), D.ctx.to_device(bl), nSweeps=1, smoother="symGaussSeidel" if sym else "GaussSeidel").cpu().numpy()
            ref = D.Ao.gs_smooth(pl, bl, nSweeps=1, sym=sym)
            assert D.ex.calls == 1 and D.exo.calls == 1
            assert np.array_equal(got, ref)
            assert not np.array_equal(ref, D.plain().gs_smooth(pl, bl, nSweeps=1, sym=sym))      # the interface term is part of the sweep
        finally:
            D.close()


# ----------------------------------------------------------------------------------------------------------- handle history ---
def _amul(D, x):
    xl = x[D.rk.gcell]
    return D.A.Amul(D.ctx.to_device(xl)).cpu().numpy(), xl


@pytest.mark.parametrize("name,r", [("blocks222", 2), ("dag4g", 0)])
def test_handle_history(O, ffm, ctx, name, r):
    case = IC.build(O, ffm, name)
    rk = case.ranks[r]
    x, _ = IC.vectors(O, case.N)
    D = DeviceRank(O, ffm, case, rk)                     # set_coeffs, then set_interfaces
    try:
        D.both(x)
        y0, xl = _amul(D, x)
        assert np.array_equal(y0, D.Ao.amul(xl))
        # the opposite order on a second handle of the context: the same bytes
        B = ffm.lduMatrix(D.ctx, rk.nOwned, rk.l, rk.u)
        B.set_interfaces(rk.faceCells, rk.bou, rk.nbrRank, intCoeffs=rk.int_, globalCells=case.N)
        B.set_coeffs(rk.diag, rk.upper, rk.lower)
        assert np.array_equal(B.Amul(D.ctx.to_device(xl)).cpu().numpy(), y0)
        B.close()
        # a second set_interfaces with other coefficients replaces the first
        bou2 = [1.5 * c + 0.01 for c in rk.bou]
        D.A.set_interfaces(rk.faceCells, bou2, rk.nbrRank, globalCells=case.N)
        D.Ao.set_interfaces(rk.faceCells, bou2)
        y2, _ = _amul(D, x)
        assert np.array_equal(y2, D.Ao.amul(xl)) and not np.array_equal(y2, y0)
        assert np.array_equal(D.A.Tmul(D.ctx.to_device(xl)).cpu().numpy(), D.Ao.tmul(xl))        # no intCoeffs given: bouCoeffs
        # an empty patch in the middle of the list changes nothing
        k, none = 1, np.zeros(0, np.int32)
        rk3 = IC.Rank(rk.rank, rk.world, rk.gcell, rk.l, rk.u, rk.diag, rk.upper, rk.lower, rk.faceCells[:k] + [none] + rk.faceCells[k:],
                      bou2[:k] + [np.zeros(0)] + bou2[k:], None, rk.nbrRank[:k] + [rk.nbrRank[0]] + rk.nbrRank[k:], rk.nbrCells[:k] + [none] + rk.nbrCells[k:])
        D.A.set_interfaces(rk3.faceCells, rk3.bou, rk3.nbrRank, globalCells=case.N)
        calls, D.ex.rank = D.ex.calls, rk3                    # (the exchange now expects the patch of size 0 too)
        y3, _ = _amul(D, x)
        D.ex.rank = rk
        assert D.ex.calls == calls + 1 and D.ex.sizes[k] == 0 and np.array_equal(y3, y2)
        # no patches: the plain matrix, and the exchange is not called
        D.A.set_interfaces([], [], [])
        calls = D.ex.calls
        yp, _ = _amul(D, x)
        assert np.array_equal(yp, D.plain().amul(xl)) and D.ex.calls == calls
        assert np.array_equal(D.A.sumA().cpu().numpy(), D.plain().sumA())
    finally:
        D.close()


def test_a_rank_of_several_without_patches(O, ffm, ctx):
    """a rank of a multi-rank context that touches no other rank: never given interfaces, or given none"""
    case = IC.build(O, ffm, "blocks222")
    rk = case.ranks[5]
    x, b = IC.vectors(O, case.N)
    for give_none in (False, True):
        D = DeviceRank(O, ffm, case, rk, interfaces=False)
        try:
            if give_none:
                D.A.set_interfaces([], [], [], globalCells=case.N)
            D.both(x)
            y, xl = _amul(D, x)
            assert np.array_equal(y, D.plain().amul(xl))
            got = D.A.smooth(D.ctx.to_device(xl), D.ctx.to_device(b[rk.gcell]), nSweeps=1).cpu().numpy()
            assert np.array_equal(got, D.plain().gs_smooth(xl, b[rk.gcell], nSweeps=1, sym=True))
            assert D.ex.calls == 0
        finally:
            D.close()


def _native_rank(O, ffm, asym=0.3, n=(5, 4, 3)):
    """a rank in the library's own cell order (what the native coefficient layout and ffm_solve_triangular_rows_d need): a level-major
    box with two invented patches, the second one with two faces on one cell"""
    N, l, u = ffm.hexmesh.hex_ldu(*n)
    cOrd, fOrd = ffm.renumber_levels(N, l, u)
    l, u, _ = ffm.hexmesh.apply_renumbering(N, l, u, cOrd, fOrd)
    F = len(l)
    up = -(0.5 + O.hash_u(31, np.arange(F)))
    lo = up * (1.0 + asym * (O.hash_u(32, np.arange(F)) - 0.3))
    fcs = [np.array([0, 7, N - 1, 13], np.int32), np.array([13, 13, 30, 2, N - 2], np.int32)]
    bou = [0.3 + O.hash_u(33 + p, np.arange(len(fc))) for p, fc in enumerate(fcs)]
    int_ = [0.2 + O.hash_u(43 + p, np.arange(len(fc))) for p, fc in enumerate(fcs)]
    diag = np.full(N, 0.4)
    np.add.at(diag, l, -up); np.add.at(diag, u, -lo)
    for fc, c in zip(fcs, bou):
        np.add.at(diag, fc, c)
    nbrCells = [N + np.arange(4), N + 4 + np.arange(5)]            # the far cells: entries behind the rank's own in the "global" vector
    rk = IC.Rank(1, 3, np.arange(N), l, u, diag, up, lo, fcs, bou, int_, [0, 2], nbrCells)
    return IC.Case("native", N + 9, [None, rk, None], None), rk


def test_native_coefficient_bind_keeps_the_interfaces(O, ffm, ctx):
    case, rk = _native_rank(O, ffm)
    D = DeviceRank(O, ffm, case, rk)
    try:
        A, c = D.A, D.ctx
        assert A.native_order
        x = 2 * O.hash_u(0xF4, np.arange(case.N)) - 0.7
        D.both(x)
        fmap = A.face_map()
        nat = lambda f: (lambda out: (out.__setitem__(fmap, f), out)[1])(np.zeros(A.nNative))
        d2 = rk.diag * 1.25
        A.bind_coeffs_native(c.to_device(d2), c.to_device(nat(rk.upper)), c.to_device(nat(rk.lower)))
        D.Ao.set_coeffs(d2, rk.upper, rk.lower)
        y, xl = _amul(D, x)
        assert np.array_equal(y, D.Ao.amul(xl))
        assert np.array_equal(A.Tmul(c.to_device(xl)).cpu().numpy(), D.Ao.tmul(xl))
        assert D.ex.calls == 2
        A.unbind_coeffs()
    finally:
        D.close()


def _echo_comm(O, rank=0, world=1):
    """the oracle's communicator of a rank whose every patch receives what it sent (keep the tuple alive with the matrix)"""
    def echo(user, nIf, size, send, recv):
        for p in range(nIf):
            np.ctypeslib.as_array(recv[p], shape=(size[p],))[:] = np.ctypeslib.as_array(send[p], shape=(size[p],))
    cb = (O.ALLREDUCE_FN(lambda user, vals, n: None), O.EXCHANGE_FN(echo))
    return O.Comm(None, rank, world, cb[0], cb[1]), cb


def test_solve_multi_takes_a_tiled_matrix_with_interfaces_one_system_at_a_time(O, ffm, ctx):
    """ffm_solve_multi_d runs three PBiCGStab + DILU systems of a tiled matrix in the library's cell order as lock-step lanes; its
    multi-system row kernel has no interface term, so with interfaces set the same call must go one system after the other.  On a
    12 x 10 x 8 box (tiled, native order) with two patches whose exchange echoes (a linear operator: the neighbour value of a patch face
    is the face cell's own).  Which way a call went shows in the diagonal the handle is left bound to: the first system's after the
    lanes, the last one's after one ffm_solve_d per system.  The results are bitwise those of single solves and meet the oracle's
    rank at the bars of tests/test_ldu_gpu.py::test_solver_parity."""
    case, rk = _native_rank(O, ffm, n=(12, 10, 8))
    N = rk.nOwned
    calls = [0]

    def echo(sizes, ranks, offs, send, recv):
        calls[0] += 1
        recv[:] = send
    c = ffm.Context(0)
    c.comm_init_host(0, 1, IC.Exchange.allreduce, echo)                    # one rank that is its own neighbour: the sums are its own
    A = ffm.lduMatrix(c, N, rk.l, rk.u)
    try:
        assert A.sweep_mode == 2 and A.native_order
        reach, _, limit5 = A.tile_reach()                                   # a tile plan that holds three systems (any plan holds up to four)
        fmap = A.face_map()
        nat = lambda f: (lambda out: (out.__setitem__(fmap, f), out)[1])(np.zeros(A.nNative))
        up_d, lo_d = c.to_device(nat(rk.upper)), c.to_device(nat(rk.lower))
        ds = [rk.diag * (1.0 + 0.3 * k) + 0.02 * k for k in range(3)]
        bs = [O.hash_u(0x71 + k, np.arange(N)) - 0.4 for k in range(3)]
        x = 2 * O.hash_u(0xF4, np.arange(N)) - 0.7
        dev = c.to_device
        kw = dict(solver="PBiCGStab", preconditioner="DILU", tolerance=1e-11, relTol=0.0, maxIter=1000)

        def multi():
            psis = [c.zeros(N) for _ in range(3)]
            perfs = A.solve_multi([dev(d) for d in ds], up_d, lo_d, psis, [dev(b) for b in bs], **kw)
            c.sync()
            return [p.cpu().numpy() for p in psis], perfs, A.Amul(dev(x)).cpu().numpy()
        plain = lambda d: O.Ldu(N, rk.l, rk.u).set_coeffs(d, rk.upper, rk.lower)
        # no interfaces: the lanes; the handle stays bound to the first system
        p0, f0, y0 = multi()
        assert calls[0] == 0 and all(f["converged"] == 1 and f["nIterations"] >= 2 for f in f0)
        assert np.array_equal(y0, plain(ds[0]).amul(x)) and not np.array_equal(y0, plain(ds[2]).amul(x))
        # interfaces: one system after the other; the handle stays bound to the last one
        A.set_interfaces(rk.faceCells, rk.bou, [0, 0], intCoeffs=rk.int_, globalCells=N)
        p1, f1, y1 = multi()
        oracles = []
        for d in ds:
            Ao = plain(d)
            Ao.set_interfaces(rk.faceCells, rk.bou, rk.int_).set_global_cells(N)
            Ao.comm, keep = _echo_comm(O)
            oracles.append((Ao, keep))
        assert calls[0] > 0
        assert np.array_equal(y1, oracles[2][0].amul(x)) and not np.array_equal(y1, oracles[0][0].amul(x))
        for k in range(3):
            A.bind_coeffs_native(dev(ds[k]), up_d, lo_d)
            psi = c.zeros(N)
            perf = A.solve(psi, dev(bs[k]), **kw)
            assert np.array_equal(p1[k], psi.cpu().numpy()) and perf == f1[k], (k, perf, f1[k])
            assert not np.array_equal(p1[k], p0[k])                         # the interfaces are part of the system
            ref, pr = oracles[k][0].solve(O.PBICGSTAB, O.DILU, np.zeros(N), bs[k], tolerance=1e-11, relTol=0.0, maxIter=1000)
            assert perf["converged"] == 1 and pr["converged"] == 1 and perf["nIterations"] == pr["nIterations"] >= 2
            assert abs(perf["initialResidual"] - pr["initialResidual"]) <= 1e-12 * pr["initialResidual"]
            assert abs(perf["finalResidual"] - pr["finalResidual"]) <= 0.05 * pr["finalResidual"] + 2e-12
            assert rel_l2(p1[k], ref) < 1e-8
        A.unbind_coeffs()
    finally:
        A.close(); c.close()


# ---------------------------------------------------------------------------------------------------------------- refusals ---
def _raw_set_interfaces(ffm, A, sizes, faceCells, bou, ranks, nPatches=None):
    """ffm_ldu_set_interfaces as the C ABI takes it; an entry None of faceCells / bou is passed as a null pointer"""
    n = len(sizes)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    fc = [None if a is None else np.ascontiguousarray(a, np.int32) for a in faceCells]
    bc = [None if a is None else np.ascontiguousarray(a, np.float64) for a in bou]
    fcp = (ip * n)(*[ip() if a is None else a.ctypes.data_as(ip) for a in fc])
    bcp = (dp * n)(*[dp() if a is None else a.ctypes.data_as(dp) for a in bc])
    return ffm.lib().ffm_ldu_set_interfaces(A.h, n if nPatches is None else nPatches, (C.c_int * n)(*sizes), fcp, bcp, bcp, (C.c_int * n)(*ranks))


@pytest.mark.parametrize("what,patch", [("size", 0), ("size", 1), ("rank", 0), ("rank", 1), ("rank_low", 2), ("faceCell", 1), ("faceCell_low", 0),
                                        ("null_faceCells", 1), ("null_bou", 2), ("nPatches", 0)])
def test_a_refused_set_interfaces_leaves_no_interfaces(O, ffm, ctx, what, patch):
    """A bad size, neighbour rank or faceCell at any patch: FFM_ERR_ARG, and the handle -- which held interfaces before the call -- has
    none afterwards: Amul is the plain matrix's and exchanges nothing.  (Before the checks were moved in front of everything that is
    stored, a bad size or rank at patch >= 1 left the earlier patches in the handle with their buffers freed.)"""
    case = IC.build(O, ffm, "blocks222")
    rk = case.ranks[2]
    x, _ = IC.vectors(O, case.N)
    D = DeviceRank(O, ffm, case, rk)
    try:
        D.both(x)
        y0, xl = _amul(D, x)
        assert np.array_equal(y0, D.Ao.amul(xl)) and D.ex.calls == 1
        sizes, fcs, ranks, bou, nP = [len(a) for a in rk.faceCells], [a.copy() for a in rk.faceCells], list(rk.nbrRank), list(rk.bou), None
        if what == "size":
            sizes[patch] = -1
        elif what == "rank":
            ranks[patch] = rk.world
        elif what == "rank_low":
            ranks[patch] = -1
        elif what == "faceCell":
            fcs[patch][-1] = rk.nOwned
        elif what == "faceCell_low":
            fcs[patch][0] = -1
        elif what == "null_faceCells":
            fcs[patch] = None
        elif what == "null_bou":
            bou[patch] = None
        else:
            nP = -1
        assert _raw_set_interfaces(ffm, D.A, sizes, fcs, bou, ranks, nP) == FFM_ERR_ARG
        message = ffm.lib().ffm_last_error().decode()
        assert ("null" in message) if what.startswith("n") else ("interface %d" % patch in message), message
        y, _ = _amul(D, x)
        assert np.array_equal(y, D.plain().amul(xl))
        assert np.array_equal(D.A.residual(D.ctx.to_device(xl), D.ctx.to_device(xl)).cpu().numpy(), D.plain().residual(xl, xl))
        assert np.array_equal(D.A.sumA().cpu().numpy(), D.plain().sumA())
        assert D.ex.calls == 1
        # and the handle takes its interfaces again
        D.A.set_interfaces(rk.faceCells, rk.bou, rk.nbrRank, globalCells=case.N)
        y, _ = _amul(D, x)
        assert np.array_equal(y, y0) and D.ex.calls == 2
    finally:
        D.close()


def test_exchange_tags_of_the_patches(O, ffm, ctx):
    """ffm_ldu_set_exchange_tags kind 0: one tag per patch or FFM_ERR_ARG; the tags order RCCL's messages, the host transport's result
    does not depend on them"""
    case = IC.build(O, ffm, "blocks222")
    rk = case.ranks[2]
    x, _ = IC.vectors(O, case.N)
    D = DeviceRank(O, ffm, case, rk)
    try:
        D.both(x)
        L, ip = ffm.lib(), C.POINTER(C.c_int)
        n = len(rk.faceCells)
        tags = np.arange(n + 1, dtype=np.int32)[::-1].copy()
        assert L.ffm_ldu_set_exchange_tags(D.A.h, 0, n + 1, tags.ctypes.data_as(ip)) == FFM_ERR_ARG
        assert L.ffm_ldu_set_exchange_tags(D.A.h, 0, n - 1, tags.ctypes.data_as(ip)) == FFM_ERR_ARG
        assert L.ffm_ldu_set_exchange_tags(D.A.h, 2, n, tags.ctypes.data_as(ip)) == FFM_ERR_ARG
        assert L.ffm_ldu_set_exchange_tags(D.A.h, 0, n, tags.ctypes.data_as(ip)) == 0
        y, xl = _amul(D, x)
        assert np.array_equal(y, D.Ao.amul(xl))
    finally:
        D.close()


def test_ordered_solves_refuse_a_matrix_with_interfaces(O, ffm, ctx):
    """ffm_flow_order_create, ffm_solve_ordered_d, ffm_flow_order_create_staged and ffm_solve_triangular_rows_d: FFM_ERR_UNSUPPORTED,
    psi untouched"""
    case, rk = _native_rank(O, ffm)
    D = DeviceRank(O, ffm, case, rk, interfaces=False)
    try:
        A, c = D.A, D.ctx
        A.set_coeffs(rk.diag, rk.upper, np.zeros_like(rk.upper))                    # upper triangular: acyclic, an order exists
        order = A.flow_order()
        A.set_interfaces(rk.faceCells, rk.bou, rk.nbrRank, globalCells=case.N)
        start = O.hash_u(0x77, np.arange(rk.nOwned))
        psi, src = c.to_device(start), c.to_device(start[::-1].copy())
        with pytest.raises(ffm.FfmError, match=r"\(-5\).*processor interfaces"):
            A.flow_order()
        with pytest.raises(ffm.FfmError, match=r"\(-5\).*processor interfaces"):
            A.solve_ordered(order, psi, src)
        with pytest.raises(ffm.FfmError, match=r"\(-5\).*processor interfaces"):
            A.flow_order_staged()
        perf = ffm.binding.Perf()
        c._ready()
        rc = ffm.lib().ffm_solve_triangular_rows_d(A.h, C.c_void_p(psi.data_ptr()), C.c_void_p(src.data_ptr()), C.byref(perf))
        assert rc == FFM_ERR_UNSUPPORTED and b"coupled patches" in ffm.lib().ffm_last_error()
        c.sync()
        assert np.array_equal(psi.cpu().numpy(), start) and D.ex.calls == 0
        # without the interfaces the same calls go through
        A.set_interfaces([], [], [])
        A.solve_ordered(order, psi, src)
        assert not np.array_equal(psi.cpu().numpy(), start)
        order.close()
    finally:
        D.close()


def test_gamg_refuses_a_matrix_with_interfaces(O, ffm, ctx):
    """the coarse levels of ffm_gamg_* couple the ranks through ghost cells; a matrix with processor interfaces would get a single-rank
    hierarchy below its finest level, so it is refused and the message names the form to use"""
    case = IC.build(O, ffm, "dag4g")
    rk = case.ranks[0]
    D = DeviceRank(O, ffm, case, rk)
    try:
        w = 0.5 + O.hash_u(0xC7, np.arange(len(rk.l)))
        with pytest.raises(ffm.FfmError, match=r"\(-5\).*ffm_ldu_set_interfaces.*ffm_ldu_set_ghost_exchange"):
            ffm.GAMG(D.ctx, D.A, rk.l, rk.u, weights=w)
        D.A.set_interfaces([], [], [])
        G = ffm.GAMG(D.ctx, D.A, rk.l, rk.u, weights=w)                             # the plain matrix is taken
        # interfaces set on the finest matrix after the hierarchy was made: refused where the matrix is used
        D.A.set_interfaces(rk.faceCells, rk.bou, rk.nbrRank, globalCells=case.N)
        dev = D.ctx.to_device
        with pytest.raises(ffm.FfmError, match=r"\(-5\).*ffm_ldu_set_interfaces"):
            G.set_matrix(dev(rk.diag), dev(rk.upper), dev(rk.lower))
        D.A.set_interfaces([], [], [])
        G.set_matrix(dev(rk.diag), dev(rk.upper), dev(rk.lower))
        D.A.set_interfaces(rk.faceCells, rk.bou, rk.nbrRank, globalCells=case.N)
        psi = D.ctx.zeros(rk.nOwned)
        with pytest.raises(ffm.FfmError, match=r"\(-5\).*ffm_ldu_set_interfaces"):
            G.solve(psi, dev(np.ones(rk.nOwned)), smoother="DILU")
        assert not psi.cpu().numpy().any()
        G.close()
    finally:
        D.close()


# ------------------------------------------------------------------------------------------------- one-rank RCCL communicator ---
def test_interfaces_through_a_one_rank_rccl_communicator(O, ffm):
    """ncclSend / ncclRecv of the patches (ffm_halo_exchange) on real hardware as far as one GPU allows: a 300-cell chain whose two
    patches, of 1 and 3 faces, both lead to rank 0 itself.  RCCL matches the messages of a pair of ranks in issue order, so each patch
    receives what it sent: the oracle's exchange echoes send to recv."""
    os.environ["FFM_FORCE_COMM"] = "1"
    try:
        ctx = ffm.Context(0)
        ctx.comm_init_rccl(0, 1, ffm.Context.comm_unique_id())
    finally:
        del os.environ["FFM_FORCE_COMM"]
    N = 300
    l, u = np.arange(N - 1, dtype=np.int32), np.arange(1, N, dtype=np.int32)
    fcs = [np.array([0], np.int32), np.array([N - 1, 120, 7], np.int32)]
    upper = -(0.5 + O.hash_u(1, np.arange(N - 1)))
    bou = [0.5 + O.hash_u(5 + p, np.arange(len(fc))) for p, fc in enumerate(fcs)]
    diag = np.full(N, 0.3)
    np.add.at(diag, l, -upper); np.add.at(diag, u, -upper)
    for fc, c in zip(fcs, bou):
        np.add.at(diag, fc, 2 * c)
    A = ffm.lduMatrix(ctx, N, l, u).set_coeffs(diag, upper)
    A.set_interfaces(fcs, bou, [0, 0], globalCells=N)
    Ao = O.Ldu(N, l, u).set_coeffs(diag, upper)
    Ao.set_interfaces(fcs, bou).set_global_cells(N)
    Ao.comm, keep = _echo_comm(O)
    x, b = 2 * O.hash_u(2, np.arange(N)) - 0.7, O.hash_u(3, np.arange(N)) - 0.5
    xd, bd = ctx.to_device(x), ctx.to_device(b)
    for _ in range(2):                                           # back to back: the send and receive buffers are reused
        assert np.array_equal(A.Amul(xd).cpu().numpy(), Ao.amul(x))
    assert np.array_equal(A.residual(xd, bd).cpu().numpy(), Ao.residual(x, b))
    for sym in (False, True):
        got = A.smooth(xd, bd, nSweeps=2, smoother="symGaussSeidel" if sym else "GaussSeidel").cpu().numpy()
        assert np.array_equal(got, Ao.gs_smooth(x, b, nSweeps=2, sym=sym))
    # the operator written out: the neighbour value of a patch face is the face cell's own
    M = np.zeros((N, N))
    M[np.arange(N), np.arange(N)] = diag
    M[l, u] += upper; M[u, l] += upper
    for fc, c in zip(fcs, bou):
        np.add.at(M, (fc, fc), -c)
    assert np.abs(Ao.amul(x) - M @ x).max() <= 1e-13 * np.abs(M @ x).max()
    psi = ctx.zeros(N)
    perf = A.solve(psi, bd, solver="PCG", preconditioner="DIC", tolerance=1e-12, relTol=0.0)
    assert perf["converged"]
    ref = np.linalg.solve(M, b)
    assert np.linalg.norm(psi.cpu().numpy() - ref) <= 1e-9 * np.linalg.norm(ref)
    A.close(); ctx.close()


# ------------------------------------------------------------------------------------------------------------ several processes ---
def _gather(parts, key="psi"):
    N = sum(len(p["gcell"]) for p in parts)
    a = np.empty(N)
    for p in parts:
        a[p["gcell"]] = p[key]
    return a


def _both_modes(world, args):
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        ref = _run_ranks("oracle", world, free_port(), args, t1, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
        got = _run_ranks("gpu_if", world, free_port(), args, t2)
    return ref, got


@pytest.mark.parametrize("precond", ["GS", "SYMGS"])
@pytest.mark.parametrize("meshName,partitioner,world", [("dag_random", "graph", 2), ("steckler", "rcb", 4)])
def test_two_smoother_sweeps_over_gloo_bitwise(O, ffm, ctx, meshName, partitioner, world, precond):
    """ONE smoother call of two sweeps on ranks in separate processes: sweep 2 takes the neighbour ranks' values after sweep 1.  The
    same arithmetic as the oracle's ranks and an exchange that moves bytes: psi is the oracle's bit for bit."""
    ref, got = _both_modes(world, [meshName, partitioner, "GS2", precond, "0.3"])
    a, b = _gather(ref), _gather(got)
    assert all(int(p["nPatches"]) > 0 for p in got)
    assert rel_l2(a, O.hash_u(0xF5, np.arange(len(a)))) > 1e-2
    assert np.array_equal(b, a), rel_l2(b, a)


@pytest.mark.parametrize("meshName,partitioner,world,solver,precond,asym", [
    ("steckler", "rcb", 4, "PCG", "DIC", 0.0), ("dag_random", "graph", 2, "PBICGSTAB", "DILU", 0.3),
    ("dag_random", "rcb", 2, "PBICG", "DILU", 0.3), ("dag_random", "graph", 4, "SMOOTH", "SYMGS", 0.3)])
def test_solves_over_gloo(O, ffm, ctx, meshName, partitioner, world, solver, precond, asym):
    """Solves at tolerance 1e-12 against the oracle's ranks (bars of tests/test_ldu_gpu.py::test_solver_parity: the two differ in the
    order of the dot products' sums) and against the serial oracle solve (bars of tests/test_partition_gpu.py)."""
    ref, got = _both_modes(world, [meshName, partitioner, solver, precond, str(asym)])
    assert len({int(p["nIter"]) for p in got}) == 1 and len({int(p["nIter"]) for p in ref}) == 1
    for r in range(world):
        g, o = got[r], ref[r]
        print(r, int(g["nIter"]), int(o["nIter"]), float(g["initialResidual"]), float(o["initialResidual"]), float(g["finalResidual"]), float(o["finalResidual"]))
        assert int(g["converged"]) == 1 and int(g["nIter"]) == int(o["nIter"])
        assert abs(float(g["initialResidual"]) - float(o["initialResidual"])) <= 1e-12 * float(o["initialResidual"])
        assert abs(float(g["finalResidual"]) - float(o["finalResidual"])) <= 0.05 * float(o["finalResidual"]) + 2e-12
    a, b = _gather(ref), _gather(got)
    print(rel_l2(b, a))
    assert rel_l2(b, a) < 1e-8
    N, l, u, centres, diag, up, lo, source = part_cases.build(O, meshName, asym)
    serial, _ = O.Ldu(N, l, u).set_coeffs(diag, up, lo).solve(getattr(O, solver), getattr(O, precond), np.zeros(N), source, tolerance=1e-12, maxIter=1000)
    print(rel_l2(b, serial))
    assert rel_l2(b, serial) < (1e-10 if solver != "SMOOTH" else 1e-9)
