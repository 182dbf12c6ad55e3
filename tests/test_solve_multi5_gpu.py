"""Five lock-step systems (ffm_solve_multi_d with nSys = 5: the four species and h of the plume step) against five ffm_solve_d.

Five LDS rings of the plan's length do not fit a workgroup, so k_tile<MODE,5,2048> runs on a ring of 2048 doubles and derives its slots from
the plan's codes; it serves plans whose ring neighbours lie within 2048 - 512 cells (ffm_ldu_tile_reach).  Checked here, all bitwise:

* solutions, residuals and iteration counts of five lanes equal those of five single solves, on boxes whose sizes are and are not
  multiples of the tile, with lanes that stop at different times, so that the sweeps hand down from five systems to four, three, two, one;
* a plan whose reach lies between the two rings' limits (one group over a 64 x 64 x 32 box) solves five systems one after the other and
  still agrees, and refuses the five-system calcReciprocalD;
* ffm_precond_setup_multi with five diagonals against five ffm_precond_setup.
"""
import numpy as np
import pytest

from ffm_import import ffm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = ffm.Context(0)
    yield c
    c.close()


def Amul(l, u, d, upper, lower, x):
    y = d * x
    np.add.at(y, u, lower * x[l]); np.add.at(y, l, upper * x[u])
    return y


def build(ctx, n, seed, oneGroup=False):
    """an asymmetric convection-diffusion-like matrix on a box in the library's cell order (native coefficient layout)"""
    rng = np.random.default_rng(seed)
    N, l, u = ffm.hexmesh.hex_ldu(*n)
    F = l.size
    hint = np.zeros(N, np.int32) if oneGroup else None
    cOrd, fOrd = ffm.renumber_levels(N, l, u, groupHint=hint)
    l2, u2, _ = ffm.hexmesh.apply_renumbering(N, l, u, cOrd, fOrd)
    A = ffm.lduMatrix(ctx, N, l2, u2, groupHint=hint)
    assert A.sweep_mode == 2 and A.native_order
    g = rng.uniform(0.5, 1.5, F)
    phi = rng.normal(0.0, 0.6, F)
    upper, lower = -g + 0.5 * phi, -g - 0.5 * phi
    base = np.zeros(N)
    np.add.at(base, l2, -lower); np.add.at(base, u2, -upper)
    fmap = A.face_map()
    nat = lambda f: (lambda out: (out.__setitem__(fmap, f), out)[1])(np.zeros(A.nNative))
    return A, N, l2, u2, upper, lower, base, rng, ctx.to_device(nat(upper)), ctx.to_device(nat(lower))


def systems(N, l, u, upper, lower, base, rng):
    """five diagonals of different dominance: every system iterates, each for another number of iterations"""
    diags, srcs, psi0 = [], [], []
    for i in range(5):
        d = base * (1.0 + 0.02 * 4.0 ** i * rng.uniform(0.5, 1.5, N)) + 0.02 * rng.uniform(0.0, 1.0, N)
        diags.append(d); srcs.append(rng.standard_normal(N)); psi0.append(np.zeros(N))
    return diags, srcs, psi0


KW = dict(solver="PBiCGStab", preconditioner="DILU", tolerance=1e-9, relTol=0.0)


def compare(ctx, A, N, l, u, upper, lower, up_d, lo_d, diags, srcs, psi0):
    dev = lambda a: ctx.to_device(a)
    host = lambda t: (ctx.sync(), t.cpu().numpy())[1]
    ref, refPerf = [], []
    for i in range(5):
        dd, pp, ss = dev(diags[i]), dev(psi0[i]), dev(srcs[i])
        A.bind_coeffs_native(dd, up_d, lo_d)
        refPerf.append(A.solve(pp, ss, **KW)); ref.append(host(pp))
    dd, pp, ss = [dev(a) for a in diags], [dev(a) for a in psi0], [dev(a) for a in srcs]
    perf = A.solve_multi(dd, up_d, lo_d, pp, ss, **KW)
    counts = [p["nIterations"] for p in perf]
    print("iterations", counts)
    assert counts == [p["nIterations"] for p in refPerf], (counts, refPerf)
    for i in range(5):
        assert np.array_equal(host(pp[i]).view(np.uint64), ref[i].view(np.uint64)), (i, np.abs(host(pp[i]) - ref[i]).max())
        for key in ("initialResidual", "finalResidual", "converged"):
            assert perf[i][key] == refPerf[i][key], (i, key, perf[i], refPerf[i])
        r = srcs[i] - Amul(l, u, diags[i], upper, lower, host(pp[i]))
        assert np.abs(r).sum() <= 1e-6 * np.abs(srcs[i]).sum() + 1e-12
    return counts


@pytest.mark.parametrize("n", [(18, 18, 18), (33, 17, 29)])
def test_five_lock_step_solves_equal_five_solves(ctx, n):
    A, N, l, u, upper, lower, base, rng, up_d, lo_d = build(ctx, n, seed=sum(n))
    reach, limit, limit5 = A.tile_reach()
    assert reach <= limit5 < limit, (reach, limit5, limit)                   # the short ring serves this plan
    diags, srcs, psi0 = systems(N, l, u, upper, lower, base, rng)
    counts = compare(ctx, A, N, l, u, upper, lower, up_d, lo_d, diags, srcs, psi0)
    # all five iterate and leave at four different times or more: the sweeps run with five systems and hand down to four, three, ...
    assert min(counts) >= 1 and len(set(counts)) >= 4, counts
    A.close()


def test_a_plan_beyond_the_short_ring_solves_one_after_the_other(ctx):
    A, N, l, u, upper, lower, base, rng, up_d, lo_d = build(ctx, (64, 64, 32), seed=7, oneGroup=True)
    reach, limit, limit5 = A.tile_reach()
    print("reach", reach, "limits", limit5, limit)
    assert limit5 < reach <= limit, (reach, limit5, limit)
    diags, srcs, psi0 = systems(N, l, u, upper, lower, base, rng)
    A.bind_coeffs_native(ctx.to_device(diags[0]), up_d, lo_d)
    with pytest.raises(ffm.FfmError):                                          # the one-sweep form is not offered for five ...
        A.reciprocalD_multi("DILU", [ctx.to_device(d) for d in diags])
    four = A.reciprocalD_multi("DILU", [ctx.to_device(d) for d in diags[:4]])   # ... and is for four
    ctx.sync()
    assert len(four) == 4
    compare(ctx, A, N, l, u, upper, lower, up_d, lo_d, diags, srcs, psi0)
    A.close()


@pytest.mark.parametrize("n", [(18, 18, 18), (33, 17, 29)])
def test_reciprocalD_of_five_diagonals_in_one_sweep(ctx, n):
    A, N, l, u, upper, lower, base, rng, up_d, lo_d = build(ctx, n, seed=3 + sum(n))
    diags = [base * (1.05 + 0.1 * i) + 0.05 * rng.uniform(0.0, 1.0, N) for i in range(5)]
    dd = [ctx.to_device(d) for d in diags]
    ref = []
    for i in range(5):
        A.bind_coeffs_native(dd[i], up_d, lo_d)
        ref.append(A.reciprocalD("DILU").cpu().numpy())
    A.bind_coeffs_native(dd[0], up_d, lo_d)
    got = A.reciprocalD_multi("DILU", dd)
    ctx.sync()
    for i in range(5):
        assert np.array_equal(got[i].cpu().numpy().view(np.uint64), ref[i].view(np.uint64)), i
    A.close()
