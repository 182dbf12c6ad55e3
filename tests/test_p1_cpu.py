"""The P1 radiation model without a GPU: the restatement tests/p1_ref.py (which the GPU tests hold the kernels of csrc/ffm_p1.hip
against) checked on its own ground, and the C ABI of the model.

  equilibrium   uniform T, T_b = T, emissivity 1, E = 0, a = e: G = 4 sigma T^4 solves the assembled system to rounding, qr = 0,
                Ru - Rp T^4 = 0 -- on a hex box and on a polyhedral mesh with a 14-face row;
  1-D slab      n x 1 x 1 cells of length 1 between two Marshak walls, every other face reflecting (emissivity 0), against
                G(x) = 4 sigma T^4 + A cosh(k (x - L/2)),  A = -Ep 4 sigma (T^4 - T_w^4)/(gamma k sinh(k L/2) + Ep cosh(k L/2)),
                gamma = 1/(3 a), k = sqrt(a/gamma), Ep = eps/(2 (2 - eps)),  qr = -gamma A k sinh(k L/2):
                second order (error ratio n = 16 -> 32 in [3.5, 4.5]), error at n = 32 below 2e-4, qr at n = 64 within 1e-4 -- measured
                here (max over the cells of |G/G_analytic - 1|) 1.07e-4 / 3.95e-5 / 2.03e-6 and ratios 3.91 / 3.92 / 3.99 for eps 1.0 / 0.7 /
                0.2, qr within 2.0e-5 / 1.6e-5 / 5.7e-6;
  edge values   emissivity 0 gives valueFraction == 0.0 with everything finite; a = 0 in some cells without scattering gives a finite gamma;
  ABI           the entry points are declared in include/ffm.h and exported by the built library (fails on a library without them)."""
import numpy as np
import pytest

import merged_mesh as MM
import p1_ref as P1


def _mesh(which):
    from oracle import plume
    return plume.make_mesh((7, 8, 6)) if which == "hex" else MM.case(which)


@pytest.mark.parametrize("which", ["hex", "w16u14"])
def test_equilibrium_is_the_known_answer(O, which):
    m = _mesh(which)
    T, a = 1200.0, 0.5
    S = P1.system(m, a, a, 0.0, np.full(m.nCells, T), T, 1.0)
    Geq = 4.0 * P1.SIGMA * T ** 4
    G = np.full(m.nCells, Geq)
    r = P1.residual(m, S, G)
    print("%s: |b - A G|_inf %.3e, |b|_inf %.3e" % (which, np.abs(r).max(), np.abs(S.s).max()))
    assert np.abs(r).max() < 1e-12 * np.abs(S.s).max()
    _, qr = P1.wall(m, S, G)
    assert max(np.abs(q).max() for q in qr) < 1e-9 * P1.SIGMA * T ** 4
    assert np.abs(P1.Ru(a, G, 0.0) - P1.Rp(a) * T ** 4).max() <= 1e-14 * P1.Rp(a) * T ** 4
    # ... and the solver finds it from zero
    Gs, perf = P1.solve(O, m, S, np.zeros(m.nCells), tolerance=1e-12)
    assert perf["converged"] and np.abs(Gs / Geq - 1.0).max() < 1e-9


def _slab(O, n, eps, a=0.5, T=1200.0, Tw=400.0, L=1.0):
    from oracle import fv
    m = fv.HexMesh((n, 1, 1), (0, 0, 0), (L, 0.1, 0.1)).set_patches([("walls", ["xmin", "xmax"]), ("mirror", ["ymin", "ymax", "zmin", "zmax"])])
    S = P1.system(m, a, a, 0.0, np.full(m.nCells, T), [np.full(2, Tw), np.full(4 * n, T)], [np.full(2, eps), np.zeros(4 * n)])
    assert all(np.all(f == 0.0) for f in S.bc.f[1:])                 # reflecting: the problem is one-dimensional
    G, perf = P1.solve(O, m, S, np.zeros(m.nCells), tolerance=1e-13)
    assert perf["converged"]
    gam = 1.0 / (3.0 * a); k = np.sqrt(a / gam); Ep = eps / (2.0 * (2.0 - eps))
    A = -Ep * 4.0 * P1.SIGMA * (T ** 4 - Tw ** 4) / (gam * k * np.sinh(k * L / 2) + Ep * np.cosh(k * L / 2))
    Gan = 4.0 * P1.SIGMA * T ** 4 + A * np.cosh(k * (m.C[:, 0] - L / 2))
    _, qr = P1.wall(m, S, G)
    return np.abs(G / Gan - 1.0).max(), qr[0], -gam * A * k * np.sinh(k * L / 2)


@pytest.mark.parametrize("eps", [1.0, 0.7, 0.2])
def test_slab_between_marshak_walls_against_its_analytic_solution(O, eps):
    e16, _, _ = _slab(O, 16, eps)
    e32, _, _ = _slab(O, 32, eps)
    _, qr, qan = _slab(O, 64, eps)
    print("eps %.1f: error n=16 %.3e, n=32 %.3e, ratio %.3f; qr n=64 %.8e / %.8e analytic %.8e" % (eps, e16, e32, e16 / e32, qr[0], qr[1], qan))
    assert 3.5 <= e16 / e32 <= 4.5
    assert e32 < 2e-4
    assert np.abs(qr / qan - 1.0).max() < 1e-4
    assert qan > 0                                                  # the hot medium loses heat to the cold walls: qr, along the outward normal, is positive


def test_edge_values_stay_ieee():
    from oracle import plume
    m = plume.make_mesh((4, 5, 3))
    N = m.nCells
    T = 300.0 + 900.0 * (np.arange(N) % 7) / 6.0
    emis = [np.zeros(p.size) for p in m.patches]
    emis[2][:] = 1.0; emis[3][::2] = 0.4
    S = P1.system(m, 0.3, 0.2, 10.0, T, 350.0, emis)
    assert all(np.all(f == 0.0) for f in S.bc.f[:2]) and np.all(S.bc.f[3][1::2] == 0.0) and np.all(S.bc.f[2] > 0.0)
    for x in [S.d, S.s, S.upper] + S.bc.f + S.bc.ref:
        assert np.isfinite(x).all()
    a = np.full(N, 0.3); a[::5] = 0.0
    g = P1.gamma(a, 0.0)
    assert np.isfinite(g).all() and np.all(g[::5] == 1.0 / P1.A0)
    S = P1.system(m, a, 0.2, 0.0, T, 350.0, 1.0, a_b=[np.full(p.size, 0.3) for p in m.patches])
    assert all(np.isfinite(x).all() for x in (S.d, S.s, S.upper))


NEW_SYMBOLS = ["ffm_p1_gamma_d", "ffm_p1_marshak_coeffs_d", "ffm_p1_assemble_d", "ffm_p1_wall_flux_d", "ffm_plume_set_radiation_p1"]


def test_the_entry_points_are_declared_and_exported(ffm):
    declared = ffm.declared_symbols()
    ffm.build()
    exported = ffm.exported_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in exported, name
