"""The ends of a solve's reductions and the start of PBiCGStab (csrc/ffm_solve.hip).

On one rank the scalar operation that follows a dot product or a norm (alpha, beta, omega, the residual) runs in the one-workgroup
launch that sums the partials, not in a launch of its own; and PBiCGStab's prologue writes ONE vector -- rA0 -- which iteration 0
reads wherever it reads rA or the search direction pA.  Neither changes a number, so on boxes of 12 x 10 x 8 and 20 x 18 x 12 cells:

(a) PCG + DIC and PBiCGStab + DILU against the oracle, with the bars of test_ldu_gpu.py::test_solver_parity (equal iteration
    counts, initial residual to 1e-12 relative, final residual to 5 % + 2e-12 -- tree sums against serial sums --, fields to 1e-8
    rel-L2) and the residual bar of test_solve_multi_gpu.py (|b - A psi| <= 1e-6 |b| + 1e-12, with the oracle's Amul);
(b) one system alone against the same system as a lane of a lock-step call: bit for bit, as test_solve_multi_gpu.py asks;
(c) the ways out of PBiCGStab that leave iteration 0 early or never enter it: a lane whose initial residual is below the tolerance
    (psi untouched, no iteration), a lane that stops after the first half iteration (shown to be that exit with the oracle's
    operators), maxIter = 1, and a zero right-hand side with minIter = 1 (the singular exit);
(d) two solves in a row on one handle -- the second finds the first's work vectors -- against a fresh handle."""
import numpy as np
import pytest

from common import rel_l2

pytestmark = pytest.mark.gpu

BOXES = [(12, 10, 8), (20, 18, 12)]
SELECT = [("PCG", "DIC", False), ("PBiCGStab", "DILU", True), ("PBiCGStab", "DIC", False)]


class Box:
    """a convection-diffusion-like matrix on a box in the library's cell order, coefficients bound in the native layout"""

    def __init__(self, ffm, ctx, n, asym, seed):
        self.ctx, self.asym = ctx, asym
        rng = self.rng = np.random.default_rng(seed)
        N, l, u = ffm.hexmesh.hex_ldu(*n)
        cOrd, fOrd = ffm.renumber_levels(N, l, u)
        self.l, self.u, _ = ffm.hexmesh.apply_renumbering(N, l, u, cOrd, fOrd)
        self.N, self.ffm = N, ffm
        F = self.l.size
        g = rng.uniform(0.5, 1.5, F)
        phi = rng.normal(0.0, 0.6, F) if asym else np.zeros(F)
        self.upper, self.lower = -g + 0.5 * phi, -g - 0.5 * phi
        self.base = np.zeros(N)
        np.add.at(self.base, self.l, -self.lower); np.add.at(self.base, self.u, -self.upper)
        self.handles = []
        self.A = self.handle()

    def handle(self):
        A = self.ffm.lduMatrix(self.ctx, self.N, self.l, self.u)
        assert A.native_order
        fmap = A.face_map()
        nat = lambda f: (lambda out: (out.__setitem__(fmap, f), out)[1])(np.zeros(A.nNative))
        A.up_d = self.ctx.to_device(nat(self.upper))
        A.lo_d = self.ctx.to_device(nat(self.lower)) if self.asym else None
        self.handles.append(A)
        return A

    def diag(self, dominance):
        return self.base * (1.0 + dominance * self.rng.uniform(0.5, 1.5, self.N)) + 0.02 * self.rng.uniform(0.0, 1.0, self.N)

    def oracle(self, O, d):
        return O.Ldu(self.N, self.l, self.u).set_coeffs(d, self.upper, self.lower if self.asym else None)

    def solve(self, d, psi0, b, A=None, **kw):
        A = A or self.A
        dd, pp, ss = self.ctx.to_device(d), self.ctx.to_device(psi0), self.ctx.to_device(b)
        A.bind_coeffs_native(dd, A.up_d, A.lo_d)
        perf = A.solve(pp, ss, **kw)
        self.ctx.sync()
        return pp.cpu().numpy(), perf

    def solve_multi(self, ds, psi0s, bs, **kw):
        dev = self.ctx.to_device
        dd, pp, ss = [dev(a) for a in ds], [dev(a) for a in psi0s], [dev(a) for a in bs]
        perf = self.A.solve_multi(dd, self.A.up_d, self.A.lo_d, pp, ss, **kw)
        self.ctx.sync()
        return [p.cpu().numpy() for p in pp], perf

    def close(self):
        for A in self.handles:
            A.close()


@pytest.fixture(scope="module", params=BOXES, ids=lambda n: "x".join(map(str, n)))
def boxes(request, ffm, ctx):
    n = request.param
    b = {False: Box(ffm, ctx, n, False, seed=sum(n)), True: Box(ffm, ctx, n, True, seed=sum(n) + 1)}
    yield b
    for x in b.values():
        x.close()


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def same_perf(p, q):
    return all(p[k] == q[k] for k in ("initialResidual", "finalResidual", "nIterations", "converged", "singular"))


def parity(pg, pr, got, ref):
    assert pg["nIterations"] == pr["nIterations"] and pg["converged"] == pr["converged"] and pg["singular"] == pr["singular"], (pg, pr)
    assert abs(pg["initialResidual"] - pr["initialResidual"]) <= 1e-12 * pr["initialResidual"], (pg, pr)
    assert abs(pg["finalResidual"] - pr["finalResidual"]) <= 0.05 * pr["finalResidual"] + 2e-12, (pg, pr)
    assert rel_l2(got, ref) < 1e-8


def oracle_ids(O, solver, precond):
    return getattr(O, {"PCG": "PCG", "PBiCGStab": "PBICGSTAB"}[solver]), getattr(O, precond)


@pytest.mark.parametrize("solver,precond,asym", SELECT)
def test_solves_match_the_oracle_and_their_lock_step_lanes(O, boxes, solver, precond, asym):
    B = boxes[asym]
    kw = dict(solver=solver, preconditioner=precond, tolerance=1e-9, relTol=0.0)
    os_, op_ = oracle_ids(O, solver, precond)
    ds = [B.diag(0.02 * 4.0 ** i) for i in range(3)]           # different dominance: different iteration counts
    bs = [B.rng.standard_normal(B.N) for _ in range(3)]
    zero = np.zeros(B.N)
    alone = [B.solve(ds[i], zero, bs[i], **kw) for i in range(3)]
    for i in range(3):
        Ao = B.oracle(O, ds[i])
        ref, pr = Ao.solve(os_, op_, zero, bs[i], tolerance=1e-9, relTol=0.0)
        parity(alone[i][1], pr, alone[i][0], ref)
        assert pr["nIterations"] >= 2                           # past iteration 1, where PBiCGStab first forms pA
        assert np.abs(bs[i] - Ao.amul(alone[i][0])).sum() <= 1e-6 * np.abs(bs[i]).sum() + 1e-12
    psis, perfs = B.solve_multi(ds, [zero] * 3, bs, **kw)
    assert len({p["nIterations"] for p in perfs}) >= 2, perfs
    for i in range(3):
        assert same_bits(psis[i], alone[i][0]) and same_perf(perfs[i], alone[i][1]), (i, perfs[i], alone[i][1])
    # the matrix's own lane through the lock-step entry point
    psi1, perf1 = B.solve_multi(ds[:1], [zero], bs[:1], **kw)
    assert same_bits(psi1[0], alone[0][0]) and same_perf(perf1[0], alone[0][1])


@pytest.mark.parametrize("solver,precond,asym", SELECT)
def test_a_start_value_that_solves_the_system_is_left_alone(O, boxes, solver, precond, asym):
    B = boxes[asym]
    kw = dict(solver=solver, preconditioner=precond, tolerance=1e-9, relTol=0.0)
    d = B.diag(0.1)
    x = B.rng.standard_normal(B.N)
    b = B.oracle(O, d).amul(x)
    psi, perf = B.solve(d, x, b, **kw)
    assert perf["nIterations"] == 0 and perf["converged"] == 1 and perf["singular"] == 0 and perf["initialResidual"] < 1e-9
    assert perf["finalResidual"] == perf["initialResidual"] and same_bits(psi, x)
    # as a lane between two that iterate
    d2 = [B.diag(0.05), d, B.diag(0.3)]
    b2 = [B.rng.standard_normal(B.N), b, B.rng.standard_normal(B.N)]
    p2 = [np.zeros(B.N), x, np.zeros(B.N)]
    psis, perfs = B.solve_multi(d2, p2, b2, **kw)
    assert same_bits(psis[1], x) and same_perf(perfs[1], perf)
    for i in (0, 2):
        pa, fa = B.solve(d2[i], p2[i], b2[i], **kw)
        assert fa["nIterations"] >= 1 and same_bits(psis[i], pa) and same_perf(perfs[i], fa)


@pytest.mark.parametrize("asym", [True, False])
def test_pbicgstab_stops_after_the_first_half_iteration(O, boxes, asym):
    """A diagonal 1e6 times the off-diagonals: DILU is the inverse to 1e-6, and sA = rA - alpha AyA is below a tolerance of 1e-4
    where rA is not.  That this is the exit taken is shown with the oracle's operators, not assumed."""
    B = boxes[asym]
    precond = "DILU" if asym else "DIC"
    tol = 1e-4
    d = 1e6 * B.base * B.rng.uniform(0.5, 1.5, B.N)
    b = B.rng.standard_normal(B.N)
    Ao = B.oracle(O, d)
    zero = np.zeros(B.N)
    nf = Ao.norm_factor(zero, b)
    rD = Ao.dilu_rD() if asym else Ao.dic_rD()
    yA = Ao.dilu_precondition(rD, b) if asym else Ao.dic_precondition(rD, b)
    AyA = Ao.amul(yA)
    alpha = (b @ b) / (b @ AyA)
    assert np.abs(b).sum() / nf > tol and np.abs(b - alpha * AyA).sum() / nf < 0.01 * tol       # not at entry; at the half iteration
    ref, pr = Ao.solve(O.PBICGSTAB, getattr(O, precond), zero, b, tolerance=tol, relTol=0.0)
    assert pr["nIterations"] == 1 and rel_l2(ref, alpha * yA) < 1e-12
    kw = dict(solver="PBiCGStab", preconditioner=precond, tolerance=tol, relTol=0.0)
    psi, perf = B.solve(d, zero, b, **kw)
    parity(perf, pr, psi, ref)
    assert rel_l2(psi, alpha * yA) < 1e-12
    # as a lane beside one that goes on: that one's first rA comes from k_bs_xr, this one's psi from the half step
    d2, b2 = [B.diag(0.05), d], [B.rng.standard_normal(B.N), b]
    psis, perfs = B.solve_multi(d2, [zero, zero], b2, **kw)
    assert same_bits(psis[1], psi) and same_perf(perfs[1], perf)
    pa, fa = B.solve(d2[0], zero, b2[0], **kw)
    assert fa["nIterations"] >= 2 and same_bits(psis[0], pa) and same_perf(perfs[0], fa)


@pytest.mark.parametrize("solver,precond,asym", SELECT)
def test_maxIter_one(O, boxes, solver, precond, asym):
    B = boxes[asym]
    kw = dict(solver=solver, preconditioner=precond, tolerance=1e-12, relTol=0.0, maxIter=1)
    os_, op_ = oracle_ids(O, solver, precond)
    d, b, zero = B.diag(0.02), B.rng.standard_normal(B.N), np.zeros(B.N)
    ref, pr = B.oracle(O, d).solve(os_, op_, zero, b, tolerance=1e-12, relTol=0.0, maxIter=1)
    psi, perf = B.solve(d, zero, b, **kw)
    assert pr["nIterations"] == 1 and pr["converged"] == 0
    parity(perf, pr, psi, ref)
    psis, perfs = B.solve_multi([d, B.diag(0.3)], [zero, zero], [b, B.rng.standard_normal(B.N)], **kw)
    assert same_bits(psis[0], psi) and same_perf(perfs[0], perf) and perfs[1]["nIterations"] == 1


@pytest.mark.parametrize("solver,precond,asym", SELECT)
def test_zero_right_hand_side_takes_the_singular_exit(O, boxes, solver, precond, asym):
    B = boxes[asym]
    os_, op_ = oracle_ids(O, solver, precond)
    d, zero = B.diag(0.1), np.zeros(B.N)
    # without minIter the solve is converged on entry
    psi, perf = B.solve(d, zero, zero, solver=solver, preconditioner=precond, tolerance=1e-9, relTol=0.0)
    assert perf["nIterations"] == 0 and perf["converged"] == 1 and perf["initialResidual"] == 0.0 and same_bits(psi, zero)
    # minIter = 1 enters the iteration: rA0.rA = 0 (PBiCGStab), wApA = 0 (PCG)
    kw = dict(tolerance=1e-9, relTol=0.0, minIter=1)
    ref, pr = B.oracle(O, d).solve(os_, op_, zero, zero, **kw)
    psi, perf = B.solve(d, zero, zero, solver=solver, preconditioner=precond, **kw)
    assert pr["singular"] == 1
    assert same_perf(perf, pr), (perf, pr)
    assert same_bits(psi, ref) and same_bits(psi, zero)
    psis, perfs = B.solve_multi([B.diag(0.3), d], [zero, zero], [B.rng.standard_normal(B.N), zero], solver=solver, preconditioner=precond, **kw)
    assert same_perf(perfs[1], perf) and same_bits(psis[1], zero) and perfs[0]["singular"] == 0 and perfs[0]["converged"] == 1


@pytest.mark.parametrize("solver,precond,asym", SELECT)
def test_a_second_solve_on_the_handle_equals_a_fresh_handle(boxes, solver, precond, asym):
    B = boxes[asym]
    kw = dict(solver=solver, preconditioner=precond, tolerance=1e-9, relTol=0.0)
    zero = np.zeros(B.N)
    d1, b1 = B.diag(0.02), B.rng.standard_normal(B.N)
    d2, b2 = B.diag(0.2), 1e3 * B.rng.standard_normal(B.N)
    first = B.solve(d1, zero, b1, **kw)
    second = B.solve(d2, zero, b2, **kw)               # finds pA, rA, rA0 of the first solve in the work vectors
    assert first[1]["nIterations"] >= 2 and second[1]["nIterations"] >= 1
    fresh = B.handle()
    ref = B.solve(d2, zero, b2, A=fresh, **kw)
    assert same_bits(second[0], ref[0]) and same_perf(second[1], ref[1])
    again = B.solve(d1, zero, b1, **kw)
    assert same_bits(again[0], first[0]) and same_perf(again[1], first[1])
