"""The wall kernel of csrc/ffm_rad.hip on its own: ffm_fvdom_wall_coeffs_d (greyDiffusiveRadiationMixedFvPatchScalarField::updateCoeffs for
all boundary faces) and ffm_fvdom_sum_rays_d, called directly on the fvMesh of a small box, against a numpy restatement in the kernel's
order of operations.  The kernel has no transcendental function: the comparison is bitwise.  tests/test_fvdom_gpu.py reaches the kernel
only through the whole fvDOM iteration (1e-8, 8 or more rays, emissivities always given); here one ray (no other ray to sum), the
`ray == 0` start of the Ir sum and its skipped own entry, a null emissivity, faces exactly tangent to the ray (d.n == 0 counts as
inflow), a boundary of one face and one of more than 256 faces, and the rows of the other rays left unwritten."""
import ctypes as C

import numpy as np
import pytest

import merged_mesh as MM

pytestmark = pytest.mark.gpu

SIGMA = 5.670367e-08


def _box(n, groups):
    from oracle import fv
    m = fv.HexMesh(n, (0.0, 0.0, 0.0), (0.13 * n[0], 0.11 * n[1], 0.07 * n[2]))
    m.set_patches([(g, [g]) for g in groups])
    return m


@pytest.fixture(scope="module")
def boxes(ffm, ctx):
    """a box whose six sides give 292 boundary faces (two blocks of 256 threads), and two cells with one boundary face"""
    out = {"box": MM.device_mesh(ffm, ctx, _box((8, 7, 6), ["ymin", "xmax", "zmin", "ymax", "xmin", "zmax"])),
           "one": MM.device_mesh(ffm, ctx, _box((2, 1, 1), ["xmin"]))}
    assert out["box"]["B"] == 292 and out["one"]["B"] == 1
    yield out
    for s in out.values():
        s["mesh"].close(); s["A"].close()


def _wall_reference(Sf, mag, nRay, ray, d, dAve, Iw, emis, Tb, qin, qem, qr):
    """k_grey_diffusive in numpy, term by term in the kernel's order; qin / qem / qr [nRay][B] are updated in place"""
    nx, ny, nz = Sf[:, 0] / mag, Sf[:, 1] / mag, Sf[:, 2] / mag
    nAve = (nx * dAve[0] + ny * dAve[1]) + nz * dAve[2]
    qr[ray] = 0.0 + Iw * nAve
    Ir = np.zeros(len(mag)) if ray == 0 else qin[0].copy()
    for j in range(1, nRay):
        Ir = Ir + (0.0 if j == ray else qin[j])
    out = -((nx * d[0] + ny * d[1]) + nz * d[2]) > 0.0
    e = np.ones(len(mag)) if emis is None else emis
    val = (Ir * (1.0 - e) + e * SIGMA * ((Tb * Tb) * (Tb * Tb))) / np.pi
    qem[ray] = np.where(out, val * nAve, 0.0)
    qin[ray] = np.where(out, 0.0, Iw * nAve)
    return np.where(out, 1.0, 0.0), np.where(out, val, 0.0), out


def _fields(B, nRay, seed):
    rng = np.random.default_rng(seed)
    Iw = 1.0e3 * (0.5 + rng.random(B)); emis = 0.1 + 0.85 * rng.random(B); Tb = 300.0 + 900.0 * rng.random(B)
    # the rows of every ray hold known values: what the other rays deposited (qin), and marks where nothing may be written
    qin = 1.0e3 * (1.0 + np.arange(nRay)[:, None]) + rng.random((nRay, B))
    qem = -1.0 - rng.random((nRay, B)); qr = -2.0 - rng.random((nRay, B))
    return Iw, emis, Tb, qin, qem, qr


OBLIQUE = (np.array([0.48, -0.6, 0.64]), np.array([0.31, -0.42, 0.37]))
ALONG_X = (np.array([-1.0, 0.0, 0.0]), np.array([-0.8, 0.05, -0.03]))     # d along -x: the y and z sides are exactly tangent


@pytest.mark.parametrize("mesh", ["box", "one"])
@pytest.mark.parametrize("given", [True, False])
@pytest.mark.parametrize("nRay,ray", [(1, 0), (8, 0), (8, 3), (8, 7)])
@pytest.mark.parametrize("dirs", [OBLIQUE, ALONG_X], ids=["oblique", "along_x"])
def test_wall_coeffs_bitwise(ffm, ctx, boxes, mesh, given, nRay, ray, dirs):
    s = boxes[mesh]
    m, B = s["m"], s["B"]
    d, dAve = dirs
    Sf = np.concatenate([p.Sf for p in m.patches]); mag = np.concatenate([p.magSf for p in m.patches])
    Iw, emis, Tb, qin, qem, qr = _fields(B, nRay, seed=7 + ray)
    D = lambda a: ctx.to_device(np.ascontiguousarray(a, np.float64).ravel())
    qd, ed, rd = D(qin), D(qem), D(qr)
    fd, refd = D(np.full(B, -3.0)), D(np.full(B, -3.0))
    hp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    s["mesh"].call("fvdom_wall_coeffs_d", nRay, ray, hp(d), hp(dAve), SIGMA, D(Iw), D(emis) if given else None, D(Tb), qd, ed, rd, fd, refd)
    before = [a.copy() for a in (qin, qem, qr)]
    f, ref, out = _wall_reference(Sf, mag, nRay, ray, d, dAve, Iw, emis if given else None, Tb, qin, qem, qr)
    got = [t.cpu().numpy().reshape(nRay, B) for t in (qd, ed, rd)]
    for name, g, r, b in zip(("qin", "qem", "qr"), got, (qin, qem, qr), before):
        assert np.array_equal(g, r), name
        others = np.arange(nRay) != ray
        assert np.array_equal(g[others], b[others]), name                     # rows of the other rays are not written
    assert np.array_equal(fd.cpu().numpy(), f) and np.array_equal(refd.cpu().numpy(), ref)
    if nRay > 1:                # the Ir sum is visible: it holds every other ray's thousands and not the ray's own
        e = emis if given else np.ones(B)
        Ir = sum(before[0][j] for j in range(nRay) if j != ray)
        if given and out.any():
            assert np.allclose((ref * np.pi - e * SIGMA * Tb ** 4)[out], (Ir * (1.0 - e))[out], rtol=1e-9)
            assert np.all(Ir >= 1.0e3 * (sum(range(1, nRay + 1)) - (ray + 1)))
    if dirs is ALONG_X:
        nx = Sf[:, 0] / mag
        tangent = nx == 0.0
        assert tangent.sum() == (B - 2 * 42 if mesh == "box" else 0)
        assert np.all(f[tangent] == 0.0) and np.all(ref[tangent] == 0.0) and np.all(got[1][ray][tangent] == 0.0)
        nAve = (Sf[:, 1] / mag) * dAve[1] + (Sf[:, 2] / mag) * dAve[2]
        assert np.array_equal(got[0][ray][tangent], (Iw * nAve)[tangent]) and (mesh == "one" or np.all(got[0][ray][tangent] != 0.0))
        assert np.array_equal(out, nx > 0.0)                                  # the wall value leaves only the side the ray comes from
    elif mesh == "box":
        assert 0 < out.sum() < B
    if mesh == "one":           # the single face (xmin) sends its wall value along the oblique ray and receives the ray along -x
        assert out[0] == (dirs is OBLIQUE)


@pytest.mark.parametrize("mesh", ["box", "one"])
@pytest.mark.parametrize("nRay", [1, 8])
def test_sum_rays_bitwise(ffm, ctx, boxes, mesh, nRay):
    s = boxes[mesh]
    B = s["B"]
    rng = np.random.default_rng(3)
    a = rng.random((nRay, B)) * 10.0 ** rng.integers(-6, 6, (nRay, B))        # magnitudes for which the order of the sum matters
    out = ctx.to_device(np.full(B, -1.0))
    s["mesh"].call("fvdom_sum_rays_d", nRay, ctx.to_device(a.ravel()), out)
    r = np.zeros(B)
    for j in range(nRay):
        r = r + a[j]
    assert np.array_equal(out.cpu().numpy(), r)
    if nRay > 1 and mesh == "box":
        back = np.zeros(B)
        for j in reversed(range(nRay)):
            back = back + a[j]
        assert not np.array_equal(back, r)                                    # another order would have shown


def test_wall_coeffs_refuse_a_ray_outside_the_set(ffm, boxes, ctx):
    s = boxes["one"]
    z = ctx.zeros(8)
    hp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    d = np.array([1.0, 0.0, 0.0])
    for nRay, ray in ((0, 0), (4, 4), (4, -1)):
        with pytest.raises(ffm.FfmError, match=r"\(-1\)"):
            s["mesh"].call("fvdom_wall_coeffs_d", nRay, ray, hp(d), hp(d), SIGMA, z, None, z, z, z, z, z, z)
    assert not z.cpu().numpy().any()
