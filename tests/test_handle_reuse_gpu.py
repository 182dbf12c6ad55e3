"""One lduMatrix handle through a history of coefficient sets, binds and solves: every result must be what a handle created fresh for
that one operation gives, BIT FOR BIT (fields, iteration counts, residuals), and must meet the oracle at the bars the single-operation
tests use (bitwise for Amul / Tmul / reciprocalD / precondition / Gauss-Seidel; test_ldu_gpu.py::test_solver_parity's bars for solves:
equal iteration counts, initial residual to 1e-12 relative, final residual to 5 % + 2e-12, fields to 1e-8 rel-L2).

The bitwise bar between the reused and the fresh handle is derived, not measured: both run the same kernels on the same inputs, the
reductions are two-stage sums in a fixed order, the sweeps are the serial face loops bit for bit.  What it guards is the state a handle
carries from one call to the next (csrc/ffm_internal.hpp: ffm_ldu): coeffEpoch / offDiagEpoch and the gathered tile coefficients that
follow offDiagEpoch (csrc/ffm_tile.hip: tile_coef), the rDKind / rDEpoch short cut of ffm_precond_setup_i, lowerBuf (allocated by the
first asymmetric set and kept), the work vectors (never cleared), LaneGuard putting diag / rD / the scalar block back after a lock-step
solve, and ffm_ldu_bind_coeffs_native_d(..., offDiagUnchanged) / ffm_ldu_unbind_coeffs.

Steps on ONE handle (coefficient sets: S1 symmetric, S2 asymmetric, S3 = S2's off-diagonals with another diagonal, S4 symmetric with
other values, S5 / S6 a second asymmetric pair of that kind):
 1  set S1: PCG + DIC, Amul, reciprocalD(DIC), precondition(DIC)
 2  set S2 (lowerBuf appears): PBiCGStab + DILU, PBiCG + DILU, Tmul, precondition(DILU, transposed)
 3  set S4 (symmetric again, lowerBuf stale): PCG + DIC, precondition(DILU), GaussSeidel, symGaussSeidel, reciprocalD DIC / DILU / DIC
 4  (boxes in the library's cell order) bind S2; bind S3's diagonal with offDiagUnchanged; lock-step solve_multi over four diagonals (one
    lane converged on entry, different iteration counts); a single solve right after it, without a new bind; the bound off-diagonal
    tensors overwritten in place with S5's and bound again (the library must gather again); the bound diagonal overwritten in place with
    S6's and bound with offDiagUnchanged (rD must be recomputed); unbind; set S1 again: step 1's operations give step 1's bits.
 5  GAMG: one ffm_gamg handle given S1, S4, S1 (smoothers GaussSeidel and DIC) on the 128^3 box of test_gamg_gpu.py, whose finest level is
    tiled: every solve bitwise that of a fresh GAMG handle, the third bitwise the first."""
import numpy as np
import pytest

from common import laplacian_like, rel_l2
from test_ldu_gpu import _make_case
from test_solve_prologue_gpu import _amul, _native_box, _parity

pytestmark = pytest.mark.gpu

KW = dict(tolerance=1e-11, relTol=0.0, maxIter=3000)
OR = {"PCG": "PCG", "PBiCGStab": "PBICGSTAB", "PBiCG": "PBICG"}
MESHES = ["box_24_20_18", "box_33_17_29", "hex_natural", "dag_random", "hex_levelmajor_t41"]
bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


class _Mesh:
    """the addressing of one case and a factory of fresh handles on it"""

    def __init__(self, name, O, ffm, ctx):
        self.name, self.ctx, self.ffm, self.O, self._gens = name, ctx, ffm, O, []
        self.native = name.startswith("box_")
        if self.native:
            n = tuple(int(v) for v in name.split("_")[1:])
            A, self.N, self.l, self.u = _native_box(ffm, ctx, n, True, seed=1)[:4]
            A.close()
        else:
            self.case, self.grp = name.rsplit("_t", 1) if "_t" in name else (name, None)
            _, self.N, self.l, self.u, A = self._from_case()
            A.close()

    def _from_case(self):
        g = _make_case(self.case, self.grp, self.O, self.ffm, self.ctx)
        self._gens.append(g)
        return next(g)

    def fresh(self):
        if self.native:
            A = self.ffm.lduMatrix(self.ctx, self.N, self.l, self.u)
            assert A.sweep_mode == 2 and A.native_order
            return A
        return self._from_case()[4]

    def native_face(self, A, f):
        out = np.zeros(A.nNative); out[A.face_map()] = f
        return self.ctx.to_device(out)


def _sets(O, N, l, u):
    h = lambda seed: O.hash_u(seed, np.arange(N))
    S1 = laplacian_like(O, N, l, u, seed=3, asym=0.0, shift=0.05)
    S2 = laplacian_like(O, N, l, u, seed=5, asym=0.35, shift=0.05)
    S3 = (S2[0] * (1.0 + 0.2 * h(0x31)) + 0.03 * h(0x32), S2[1], S2[2])
    S4 = laplacian_like(O, N, l, u, seed=11, asym=0.0, shift=0.08)
    S5 = laplacian_like(O, N, l, u, seed=17, asym=0.3, shift=0.05)
    S6 = (S5[0] * (1.0 + 0.3 * h(0x61)) + 0.02 * h(0x62), S5[1], S5[2])
    return dict(S1=S1, S2=S2, S3=S3, S4=S4, S5=S5, S6=S6)


def _run(A, ctx, O, N, op):
    """one operation on a handle: (arrays, perf or None)"""
    h = lambda seed: O.hash_u(seed, np.arange(N))
    dev = ctx.to_device
    if op[0] == "solve":
        psi = ctx.zeros(N)
        pf = A.solve(psi, dev(2 * h(0xF3) - 1), solver=op[1], preconditioner=op[2], **KW)
        ctx.sync()
        return [psi.cpu().numpy()], pf
    if op[0] == "Amul":
        return [A.Amul(dev(2 * h(0xF4) - 0.7)).cpu().numpy()], None
    if op[0] == "Tmul":
        return [A.Tmul(dev(2 * h(0xF4) - 0.7)).cpu().numpy()], None
    if op[0] == "rD":
        return [A.reciprocalD(k).cpu().numpy() for k in op[1:]], None
    if op[0] == "precondition":
        return [A.precondition(op[1], dev(2 * h(12) - 1), transpose=op[2]).cpu().numpy()], None
    if op[0] == "smooth":
        return [A.smooth(dev(h(13)), dev(h(14)), nSweeps=2, smoother=op[1]).cpu().numpy()], None
    raise ValueError(op)


def _oracle(Ao, O, N, op):
    h = lambda seed: O.hash_u(seed, np.arange(N))
    if op[0] == "solve":
        ref, pr = Ao.solve(getattr(O, OR[op[1]]), getattr(O, op[2]), np.zeros(N), 2 * h(0xF3) - 1, **KW)
        return [ref], pr
    if op[0] == "Amul":
        return [Ao.amul(2 * h(0xF4) - 0.7)], None
    if op[0] == "Tmul":
        return [Ao.tmul(2 * h(0xF4) - 0.7)], None
    if op[0] == "rD":
        return [Ao.dic_rD() if k == "DIC" else Ao.dilu_rD() for k in op[1:]], None
    if op[0] == "precondition":
        r = 2 * h(12) - 1
        return [Ao.dic_precondition(Ao.dic_rD(), r) if op[1] == "DIC" else Ao.dilu_precondition(Ao.dilu_rD(), r, transpose=op[2])], None
    if op[0] == "smooth":
        return [Ao.gs_smooth(h(13), h(14), nSweeps=2, sym=op[1] == "symGaussSeidel")], None
    raise ValueError(op)


def _same_bits(tag, got, ref):
    (ga, gp), (ra, rp) = got, ref
    assert len(ga) == len(ra)
    for k, (a, b) in enumerate(zip(ga, ra)):
        assert np.array_equal(bits(a), bits(b)), (tag, k, rel_l2(a, b))
    if gp is not None:
        assert gp["nIterations"] == rp["nIterations"] and gp["converged"] == rp["converged"], (tag, gp, rp)
        assert np.array_equal(bits([gp["initialResidual"], gp["finalResidual"]]), bits([rp["initialResidual"], rp["finalResidual"]])), (tag, gp, rp)


def _meets_oracle(tag, got, ref):
    (ga, gp), (ra, rp) = got, ref
    if gp is None:
        for k, (a, b) in enumerate(zip(ga, ra)):
            assert np.array_equal(bits(a), bits(b)), (tag, k, rel_l2(a, b))
        return
    assert gp["converged"] == 1 and rp["converged"] == 1, (tag, gp, rp)
    assert gp["nIterations"] == rp["nIterations"], (tag, gp, rp)
    assert abs(gp["initialResidual"] - rp["initialResidual"]) <= 1e-12 * rp["initialResidual"], (tag, gp, rp)
    assert abs(gp["finalResidual"] - rp["finalResidual"]) <= 0.05 * rp["finalResidual"] + 2e-12, (tag, gp, rp)
    assert rel_l2(ga[0], ra[0]) < 1e-8, (tag, rel_l2(ga[0], ra[0]))


STEP1 = [("solve", "PCG", "DIC"), ("Amul",), ("rD", "DIC"), ("precondition", "DIC", False)]
STEP2 = [("solve", "PBiCGStab", "DILU"), ("solve", "PBiCG", "DILU"), ("Tmul",), ("precondition", "DILU", True)]
STEP3 = [("solve", "PCG", "DIC"), ("precondition", "DILU", False), ("smooth", "GaussSeidel"), ("smooth", "symGaussSeidel"),
         ("rD", "DIC", "DILU", "DIC")]


@pytest.mark.parametrize("name", MESHES)
def test_one_handle_through_a_history(O, ffm, ctx, name, monkeypatch):
    if "_t" in name:
        monkeypatch.setenv("FFM_PIPE_GROUP_CELLS", name.rsplit("_t", 1)[1])
        monkeypatch.setenv("FFM_SWEEP", "tile")
    M = _Mesh(name, O, ffm, ctx)
    N, l, u = M.N, M.l, M.u
    S = _sets(O, N, l, u)
    H = M.fresh()
    done = []

    def step(tag, sname, ops, prepare=None, fresh_prepare=None, keep=None):
        """ops on the reused handle (after prepare(H); default: set_coeffs) against a fresh handle each and the oracle"""
        coeffs = S[sname] if isinstance(sname, str) else sname
        (prepare or (lambda A: A.set_coeffs(*coeffs)))(H)
        Ao = O.Ldu(N, l, u).set_coeffs(*coeffs)
        for op in ops:
            got = _run(H, ctx, O, N, op)
            F = M.fresh()
            (fresh_prepare or (lambda A: A.set_coeffs(*coeffs)))(F)
            _same_bits((name, tag, op, "fresh handle"), got, _run(F, ctx, O, N, op))
            F.close()
            _meets_oracle((name, tag, op, "oracle"), got, _oracle(Ao, O, N, op))
            if keep is not None:
                keep.append(got)
            done.append((tag, op))

    first = []
    step("1", "S1", STEP1, keep=first)
    step("2", "S2", STEP2)
    step("3", "S4", STEP3)
    expected = len(STEP1) + len(STEP2) + len(STEP3)
    if M.native:
        dev = ctx.to_device
        SOLVE = [("solve", "PBiCGStab", "DILU")]
        nat = lambda A, f: M.native_face(A, f)
        bound = lambda c: (lambda A: A.bind_coeffs_native(dev(c[0]), nat(A, c[1]), nat(A, c[2])))          # a fresh handle's plain bind
        d2, up, lo = dev(S["S2"][0]), nat(H, S["S2"][1]), nat(H, S["S2"][2])
        step("4a bind", "S2", SOLVE, prepare=lambda A: A.bind_coeffs_native(d2, up, lo), fresh_prepare=bound(S["S2"]))
        d3 = dev(S["S3"][0])
        step("4b diagonal, offDiagUnchanged", "S3", SOLVE, prepare=lambda A: A.bind_coeffs_native(d3, up, lo, offDiagUnchanged=True),
             fresh_prepare=bound(S["S3"]))
        # 4c the lock-step solve: four diagonals over S2's off-diagonals; lane 1 starts from its solution
        rng = np.random.default_rng(41)
        nSys, tol = 4, 1e-9
        base = S["S2"][0]
        diags = [base * (1.0 + 0.02 * 4.0 ** i * rng.uniform(0.5, 1.5, N)) + (10.0 if i == 2 else 0.02) * rng.uniform(0.0, 1.0, N) for i in range(nSys)]
        srcs, psi0 = [], []
        for i in range(nSys):
            x = rng.standard_normal(N)
            srcs.append(_amul(l, u, diags[i], S["S2"][1], S["S2"][2], x) if i == 1 else rng.standard_normal(N))
            psi0.append(x if i == 1 else np.zeros(N))

        def multi(A, up_, lo_):
            dd, pp, ss = [dev(a) for a in diags], [dev(a) for a in psi0], [dev(a) for a in srcs]
            perf = A.solve_multi(dd, up_, lo_, pp, ss, solver="PBiCGStab", preconditioner="DILU", tolerance=tol, relTol=0.0)
            ctx.sync()
            return [p.cpu().numpy() for p in pp], perf, dd
        gotF, perfH, ddH = multi(H, up, lo)
        counts = [p["nIterations"] for p in perfH]
        assert counts[1] == 0 and len(set(counts)) >= 2, counts
        F = M.fresh()
        refF, perfF, _ = multi(F, nat(F, S["S2"][1]), nat(F, S["S2"][2]))
        for i in range(nSys):
            _same_bits((name, "4c lock step", i, "fresh handle"), ([gotF[i]], perfH[i]), ([refF[i]], perfF[i]))
            ref, pr = O.Ldu(N, l, u).set_coeffs(diags[i], S["S2"][1], S["S2"][2]).solve(O.PBICGSTAB, O.DILU, psi0[i].copy(), srcs[i], tolerance=tol, relTol=0.0)
            _parity(perfH[i], pr, gotF[i], ref, i == 1, tol)
        F.close()
        done.append(("4c", "solve_multi"))
        # 4d a single solve right after it, no new bind: the matrix is lane 0's
        step("4d after lock step", (diags[0], S["S2"][1], S["S2"][2]), SOLVE, prepare=lambda A: None,
             fresh_prepare=bound((diags[0], S["S2"][1], S["S2"][2])))
        # 4e the bound off-diagonal tensors overwritten in place, bound again: gathered again
        d5 = dev(S["S5"][0])
        def overwrite_offdiag(A):
            up.copy_(nat(A, S["S5"][1])); lo.copy_(nat(A, S["S5"][2]))
            A.bind_coeffs_native(d5, up, lo, offDiagUnchanged=False)
        step("4e off-diagonals in place", "S5", SOLVE, prepare=overwrite_offdiag, fresh_prepare=bound(S["S5"]))
        def overwrite_diag(A):
            d5.copy_(dev(S["S6"][0]))
            A.bind_coeffs_native(d5, up, lo, offDiagUnchanged=True)
        step("4f diagonal in place", "S6", SOLVE, prepare=overwrite_diag, fresh_prepare=bound(S["S6"]))
        H.unbind_coeffs()
        again = []
        step("4h", "S1", STEP1, keep=again)
        for op, a, b in zip(STEP1, first, again):
            _same_bits((name, "4h against step 1", op), b, a)
        expected += 1 + 1 + 1 + 1 + 1 + 1 + len(STEP1)
    assert len(done) == expected, done           # every step ran
    H.close()
    for g in M._gens:
        next(g, None)                            # (the case generators close their handles)


@pytest.mark.parametrize("smoother", ["GaussSeidel", "DIC"])
def test_one_gamg_handle_through_three_matrices(O, ffm, ctx, smoother):
    from test_gamg_gpu import _box
    n = (128, 128, 128)
    blk, s, Sf = _box(ffm, n)
    N = blk.nCells
    hu = ffm.hexmesh.hash_u
    S1 = (s["diag"], s["upper"])
    up4 = s["upper"] * (0.6 + 0.8 * hu(0xC4, blk.gface))                   # symmetric, other values
    rest = s["diag"].copy(); np.add.at(rest, blk.l, s["upper"]); np.add.at(rest, blk.u, s["upper"])      # the compressibility and boundary part (> 0)
    d4 = 1.5 * rest; np.add.at(d4, blk.l, -up4); np.add.at(d4, blk.u, -up4)
    S4 = (d4, up4)
    src = ctx.to_device(s["source"])

    def handle():
        A = ffm.lduMatrix(ctx, N, blk.l, blk.u)
        assert A.sweep_mode == 2
        return A, ffm.GAMG(ctx, A, blk.l, blk.u, Sf=Sf)

    def solve(G, S):
        G.set_matrix(ctx.to_device(S[0]), ctx.to_device(S[1]))
        psi = ctx.to_device(np.zeros(N))
        pf = G.solve(psi, src, smoother=smoother, tolerance=1e-8, maxIter=50)
        ctx.sync()
        return [psi.cpu().numpy()], pf

    A, G = handle()
    assert G.nLevels >= 15
    got = [solve(G, S) for S in (S1, S4, S1)]
    G.close(); A.close()
    for k, S in ((0, S1), (1, S4)):
        Af, Gf = handle()
        ref = solve(Gf, S)
        Gf.close(); Af.close()
        assert ref[1]["converged"] and ref[1]["nIterations"] >= 2, ref[1]
        _same_bits((smoother, "solve %d" % (k + 1), "fresh GAMG handle"), got[k], ref)
        if k == 0:
            _same_bits((smoother, "solve 3", "fresh GAMG handle"), got[2], ref)
    _same_bits((smoother, "solve 3 against solve 1"), got[2], got[0])
