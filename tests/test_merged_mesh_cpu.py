"""The wide-row mesh builder tests/merged_mesh.py, checked independently of the library (no GPU): every named case is a closed, planar-
faced polyhedral mesh in upper-triangular order with the widths -- and so the FFM_DISPATCH_W bucket -- its name claims, and
oracle/fv.py runs on it."""
import numpy as np
import pytest

import merged_mesh as MM

ALL = {**MM.CASES, **MM.REFUSED}


@pytest.fixture(scope="module", params=sorted(ALL))
def built(request):
    return request.param, MM.case(request.param)


def test_cells_are_closed_and_fill_the_box(built):
    from oracle import fv
    name, m = built
    n = ALL[name][0]
    closure = np.zeros((m.nCells, 3))
    np.add.at(closure, m.l, m.Sf); np.subtract.at(closure, m.u, m.Sf)
    for p in m.patches:
        np.add.at(closure, p.faceCells, p.Sf)
    big = max(m.magSf.max(), max(p.magSf.max() for p in m.patches))
    assert np.abs(closure).max() <= 1e-14 * big
    assert abs(m.V.sum() - n[0] * n[1] * n[2] * 0.1 ** 3) <= 1e-14 * m.V.sum()
    assert m.nCells == ALL[name][3]
    # the same statement through the oracle: the gradient of a constant is zero
    g = fv.grad(m, np.full(m.nCells, 3.0), [np.full(p.size, 3.0) for p in m.patches])
    assert np.abs(g).max() <= 1e-12 * 3.0 / 0.1
    # centres: volume-weighted means of the fine cells, inside the box
    assert np.allclose((m.V[:, None] * m.C).sum(axis=0), (m.fine.V[:, None] * m.fine.C).sum(axis=0), rtol=1e-13)


def test_faces_are_planar_and_upper_triangular(built):
    name, m = built
    assert np.all(np.abs(m.magSf - m.sumMagSf) <= 1e-14 * m.sumMagSf)             # |sum Sf| == sum |Sf|
    assert np.all(m.l < m.u)
    key = m.l.astype(np.int64) * m.nCells + m.u
    assert np.all(np.diff(key) > 0)                                               # (l, u) strictly increasing
    assert np.all(m.weights > 0) and np.all(m.weights < 1)
    assert np.all(m.deltaCoeffs > 0) and all(np.all(p.deltaCoeffs > 0) for p in m.patches)
    # the area vector points from the owner to the neighbour
    assert np.all(np.einsum("fd,fd->f", m.Sf, m.C[m.u] - m.C[m.l]) > 0)
    assert all(np.all(np.einsum("fd,fd->f", p.Sf, p.Cf - m.C[p.faceCells]) > 0) for p in m.patches)


def test_widths_and_buckets_are_the_named_ones(built):
    name, m = built
    _, bars, first, cells, wu, wl, W = ALL[name]
    assert MM.widths(m.l, m.u) == (wu, wl)
    if W is not None:
        assert MM.bucket(max(wu, wl)) == W
    # the wide row is one among narrow ones: every cell but the bars has at most 4 faces on a side
    nU, nL = np.bincount(m.l, minlength=m.nCells), np.bincount(m.u, minlength=m.nCells)
    isbar = np.zeros(m.nCells, bool)
    isbar[np.arange(len(bars)) + (0 if first else m.nCells - len(bars))] = True
    assert nU[~isbar].max() <= 4 and nL[~isbar].max() <= 4
    # a bar of L cells is a polyhedron of 4L+2 faces, less the fine faces it shares with another bar and merges into one
    nB = np.zeros(m.nCells, int)
    for p in m.patches:
        nB += np.bincount(p.faceCells, minlength=m.nCells)
    tot = (nU + nL + nB)[isbar]
    assert np.all(tot <= np.array([4 * b[3] + 2 for b in bars])) and (name == "w32multi" or np.all(tot == [4 * b[3] + 2 for b in bars]))
    assert (m.nCells + 63) // 64 in (1, 2, 3, 4)


def test_bucket_thresholds():
    assert [MM.bucket(w) for w in (1, 3, 4, 5, 8, 9, 16, 17, 32)] == [3, 3, 4, 8, 8, 16, 16, 32, 32]


def test_oracle_operators_run_and_are_finite(built):
    from oracle import fv
    name, m = built
    rng = np.random.default_rng(5)
    vf = rng.uniform(0.2, 1.2, m.nCells); vb = [rng.uniform(0.1, 1.1, p.size) for p in m.patches]
    phi = rng.uniform(-0.15, 0.15, m.nFaces); phib = [rng.uniform(-0.05, 0.05, p.size) for p in m.patches]
    g = fv.grad(m, vf, vb)
    r = fv.reconstruct(m, phi, phib)
    w = fv.limited_weights(m, "limitedLinear", phi, vf, g, 1.0)
    assert np.isfinite(g).all() and np.isfinite(r).all() and np.isfinite(w).all()
    assert w.min() >= 0 and w.max() <= 1
    assert np.linalg.cond(fv.reconstruct_tensor(m)).max() < 1e3
    # a linear field with its exact face values: the Gauss gradient of a closed polyhedron is exact only with exact FACE values; with
    # linear interpolation it is exact where weights*C_l + (1-weights)*C_u = Cf, i.e. away from the bars
    a = np.array([0.7, -1.3, 2.1])
    glin = fv.grad(m, m.C @ a + 0.4, [p.Cf @ a + 0.4 for p in m.patches])
    nbr = np.zeros(m.nCells, bool)
    skew = np.linalg.norm(m.weights[:, None] * m.C[m.l] + (1 - m.weights[:, None]) * m.C[m.u] - m.Cf, axis=1) > 1e-12
    nbr[m.l[skew]] = True; nbr[m.u[skew]] = True
    assert (~nbr).sum() > 0 and np.abs(glin[~nbr] - a).max() < 1e-12
