"""GAMG on polyhedral and unstructured meshes whose coarse levels have rows of 17 to 22 owned upper faces (tests/gamg_wide_cases.py: the
merged meshes of tests/merged_mesh.py with their real face areas and with hashed weights, and two randomly relabelled boxes; two rows
that stay at 16 and below are the controls).  A lower entry of such a level packs owner << 5 | slot instead of owner << 4 | slot
(csrc/ffm_ldu_analysis.cpp: check_layout_limits), and every row kernel, sweep and restriction of the V-cycle decodes it.

Against the oracle (oracle/gamg.py), as tests/test_gamg_gpu.py on boxes: the same hierarchy level by level, the coarse coefficients bit
for bit (symmetric and asymmetric), and per smoother the same number of V-cycles, initialResidual to 1e-12 and finalResidual to 1e-6
relative (test_gamg_solve_equals_the_oracle), the field to 1e-9 rel-L2 (test_gamg_on_unstructured_addressing) and the iteration counts
of the coarsest-level solves."""
import numpy as np
import pytest

import gamg_wide_cases as GW
from common import laplacian_like, rel_l2

pytestmark = pytest.mark.gpu


def _context_works(O, ffm, ctx):
    """the closing check of test_ldu_gpu.py::test_too_wide_rows_are_refused"""
    N, l, u = O.hex_ldu(9, 7, 8)
    diag, up, lo = laplacian_like(O, N, l, u, seed=3, asym=0.35, shift=0.05)
    A = ffm.lduMatrix(ctx, N, l, u).set_coeffs(diag, up, lo)
    x = 2 * O.hash_u(0xF4, np.arange(N)) - 0.7
    assert np.array_equal(A.Amul(ctx.to_device(x)).cpu().numpy(), O.Ldu(N, l, u).set_coeffs(diag, up, lo).amul(x))
    A.close()


def _gamg(O, ffm, ctx, name):
    """the row's lduMatrix and GAMG; a GAMG that cannot be built leaves a working context behind"""
    N, l, u, w, agg = GW.build(O, name)
    GW.check_widths(name, agg)
    A = ffm.lduMatrix(ctx, N, l, u)
    try:
        G = ffm.GAMG(ctx, A, l, u, weights=w)
    except ffm.FfmError:
        A.close()
        _context_works(O, ffm, ctx)
        raise
    return N, l, u, agg, A, G


def _coeffs(O, N, l, u, asym):
    return laplacian_like(O, N, l, u, seed=3, asym=0.35 if asym else 0.0, shift=0.05)


@pytest.mark.parametrize("name", GW.SMALL)
def test_hierarchy_and_coarse_matrices_equal_the_oracle(O, ffm, ctx, name):
    from oracle import gamg
    N, l, u, agg, A, G = _gamg(O, ffm, ctx, name)
    assert G.nLevels == agg.nLevels and agg.nLevels >= 3
    for lev in range(agg.nLevels + 1):
        gl, gu = G.level_addressing(lev)
        assert np.array_equal(gl, agg.l[lev]) and np.array_equal(gu, agg.u[lev]), lev
        assert G.level_size(lev) == (agg.nCells[lev], len(agg.l[lev])), lev
    for asym in (False, True):
        diag, up, lo = _coeffs(O, N, l, u, asym)
        G.set_matrix(ctx.to_device(diag), ctx.to_device(up), None if lo is None else ctx.to_device(lo))
        ref = gamg.GAMGSolver(agg, diag, up, lo)
        for lev in range(agg.nLevels + 1):
            d, uu, ll = G.level_coeffs(lev)
            rd, ru, rl = ref.coef[lev]
            assert np.array_equal(d, rd) and np.array_equal(uu, ru), (asym, lev)
            assert np.array_equal(ll, ru if rl is None else rl), (asym, lev)
    G.close(); A.close()
    _context_works(O, ffm, ctx)


@pytest.mark.parametrize("smoother", ["GaussSeidel", "DIC", "DILU"])
@pytest.mark.parametrize("name", GW.SMALL)
def test_solve_equals_the_oracle(O, ffm, ctx, name, smoother):
    from oracle import gamg
    N, l, u, agg, A, G = _gamg(O, ffm, ctx, name)
    diag, up, lo = _coeffs(O, N, l, u, smoother == "DILU")
    G.set_matrix(ctx.to_device(diag), ctx.to_device(up), None if lo is None else ctx.to_device(lo))
    ref = gamg.GAMGSolver(agg, diag, up, lo, smoother=smoother)
    source = O.hash_u(0xF3, np.arange(N)) - 0.4
    xr, pr = ref.solve(np.zeros(N), source, tolerance=1e-8)
    assert pr["converged"] and 2 <= pr["nIterations"] < 60, pr
    psi = ctx.to_device(np.zeros(N))
    pf = G.solve(psi, ctx.to_device(source), smoother=smoother, tolerance=1e-8)
    cs = G.coarsest_solves()
    print("%s %s: V-cycles %d (oracle %d), initial %.3e rel %.1e, final %.3e rel %.1e, field rel-L2 %.1e" % (
        name, smoother, pf["nIterations"], pr["nIterations"], pf["initialResidual"],
        abs(pf["initialResidual"] - pr["initialResidual"]) / pr["initialResidual"], pf["finalResidual"],
        abs(pf["finalResidual"] - pr["finalResidual"]) / pr["finalResidual"], rel_l2(psi.cpu().numpy(), xr)))
    assert pf["nIterations"] == pr["nIterations"] and pf["converged"], (pf, pr)
    assert abs(pf["initialResidual"] - pr["initialResidual"]) <= 1e-12 * pr["initialResidual"], (pf, pr)
    assert abs(pf["finalResidual"] - pr["finalResidual"]) <= 1e-6 * pr["finalResidual"], (pf, pr)
    assert rel_l2(psi.cpu().numpy(), xr) < 1e-9
    assert [c["nIterations"] for c in cs] == [c["nIterations"] for c in ref.coarsest_log], (cs, ref.coarsest_log)
    G.close(); A.close()
    _context_works(O, ffm, ctx)
