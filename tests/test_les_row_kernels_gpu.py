"""The kEqn kernels of the compiled time step on their own (csrc/ffm_fused.hip: ffm_les_keqn_terms, ffm_les_face_diffusivity,
ffm_les_keqn_update) against numpy, on one mesh per row-width bucket of FFM_DISPATCH_W: the 7 x 8 x 6 hex box (W = 3) and the merged
meshes w4, w8, w16u14, w32l30, w32multi, w32u18 of tests/merged_mesh.py.  The inputs hold a patch with nut_b = 0 (the floor), a cell with
k = SMALL and cells below it; ffm_les_keqn_update is also launched on one cell.

Agreement.  The numpy side states each expression in the kernels' operation order on the mesh in the device's numbering, where the
serial face loop (oracle/fv.py: surface_integrate) is the row's summation order; +, -, *, / and sqrt are correctly rounded on both
sides and FMA contraction is off, so every output is compared BIT FOR BIT.  G is also held against the tensor form of
oracle/steckler_case.py (einsum, another summation order) to 16 ulp of the sum of the magnitudes of its nine products."""
import numpy as np
import pytest

import merged_mesh as MM

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
SMALL = 1.0e-15
MESHES = {"hex": 3, "w4": 4, "w8": 8, "w16u14": 16, "w32l30": 32, "w32multi": 32, "w32u18": 32}
MU, CE, CK, PRT = 1.8e-5, 1.048, 0.094, 0.85


@pytest.fixture(scope="module")
def meshes(ffm, ctx):
    made = {}

    def get(name):
        if name not in made:
            from oracle import plume
            s = MM.device_mesh(ffm, ctx, plume.make_mesh((7, 8, 6), h=0.1) if name == "hex" else MM.case(name))
            assert s["W"] == MESHES[name]
            s["pad"] = s["mesh"].to_native(np.ones(s["F"])).cpu().numpy() == 0.0
            made[name] = s
        return made[name]
    yield get
    for s in made.values():
        s["mesh"].close(); s["A"].close()


def _h(O, seed, n, lo=0.0, hi=1.0):
    return lo + (hi - lo) * O.hash_u(seed, np.arange(n))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _inputs(s, O):
    """fields on the oracle's mesh s["m"]: cells [N], faces [F], patch faces per patch"""
    m, N, F = s["m"], s["N"], s["F"]
    d = dict(rho=_h(O, 1, N, 1.0, 1.3), nut=_h(O, 2, N, 0.0, 4e-4), k=_h(O, 3, N, 1e-5, 5e-3), delta=np.cbrt(m.V),
             phi=_h(O, 4, F, -2e-3, 2e-3), alphat=_h(O, 5, N, 0.0, 5e-4), g=[_h(O, 10 + q, N, -3.0, 3.0) for q in range(9)])
    d["k"][N // 2] = SMALL; d["nut"][N // 3] = 0.0
    d["g"][4][::5] = 0.0
    d["rhob"] = [_h(O, 20 + q, p.size, 1.0, 1.3) for q, p in enumerate(m.patches)]
    d["phib"] = [_h(O, 30 + q, p.size, -2e-3, 2e-3) for q, p in enumerate(m.patches)]
    d["nutb"] = [np.zeros(p.size) if p.name == "floor" else _h(O, 40 + q, p.size, 0.0, 4e-4) for q, p in enumerate(m.patches)]
    d["alphatb"] = [np.zeros(p.size) if p.name == "floor" else _h(O, 50 + q, p.size, 0.0, 5e-4) for q, p in enumerate(m.patches)]
    assert any(p.name == "floor" and p.size for p in m.patches)
    return d


def _G_in_kernel_order(g, nut):
    """les_G_of: g[3*a + b] = d_a U_b"""
    G = lambda a, b: g[3 * a + b]
    ts = [[G(a, b) + G(b, a) for b in range(3)] for a in range(3)]
    tr = (ts[0][0] + ts[1][1]) + ts[2][2]
    for a in range(3):
        ts[a][a] = ts[a][a] - (1.0 / 3.0) * tr
    acc = np.zeros_like(nut)
    for a in range(3):
        for b in range(3):
            acc = acc + G(a, b) * ts[a][b]
    return nut * acc


@pytest.mark.parametrize("name", list(MESHES))
def test_keqn_terms_against_numpy(meshes, O, ctx, name):
    from oracle import fv
    s = meshes(name); m, mesh, N, c, f = s["m"], s["mesh"], s["N"], s["cOrd"], s["fOrd"]
    d = _inputs(s, O)
    dev = ctx.to_device
    cat = lambda bs: dev(np.concatenate(bs))
    out = [ctx.zeros(N) + SENTINEL for _ in range(3)]
    mesh.call("les_keqn_terms", [dev(g[c]) for g in d["g"]], dev(d["nut"][c]), dev(d["rho"][c]), cat(d["rhob"]), dev(d["k"][c]),
              dev(d["delta"][c]), mesh.to_native(d["phi"][f]), cat(d["phib"]), CE, *out)
    su, su2, sp = (o.cpu().numpy() for o in out)
    rhof, _ = fv.interpolate(m, d["rho"], d["rhob"])
    divU = fv.surface_integrate(m, d["phi"] / rhof, [a / b for a, b in zip(d["phib"], d["rhob"])])
    G = _G_in_kernel_order(d["g"], d["nut"])
    ss = (2.0 / 3.0) * d["rho"] * divU
    assert (ss > 0).any() and (ss < 0).any()
    want_su = d["rho"] * G
    want_su2 = -(np.minimum(ss, 0.0) * d["k"])
    want_sp = np.maximum(ss, 0.0) + CE * d["rho"] * np.sqrt(d["k"]) / d["delta"]
    for got, want, what in ((su, want_su, "su"), (su2, want_su2, "su2"), (sp, want_sp, "sp")):
        assert np.array_equal(_bits(got), _bits(want[c])), (what, np.abs(got - want[c]).max())
    # G against the tensor form: nut*(gradU && dev(twoSymm(gradU)))
    gU = np.stack(d["g"], axis=1).reshape(N, 3, 3)
    two = gU + np.swapaxes(gU, 1, 2)
    dev_ = two - (1.0 / 3.0) * np.trace(two, axis1=1, axis2=2)[:, None, None] * np.eye(3)
    scale = d["nut"] * np.abs(gU * dev_).sum(axis=(1, 2))
    assert (np.abs(G - d["nut"] * np.einsum("nij,nij->n", gU, dev_)) <= 16 * np.spacing(scale) + 1e-300).all()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(MESHES))
def test_face_diffusivity_against_numpy(meshes, O, ctx, name, mode):
    from oracle import fv
    s = meshes(name); m, mesh, N, c, f = s["m"], s["mesh"], s["N"], s["cOrd"], s["fOrd"]
    d = _inputs(s, O)
    dev = ctx.to_device
    cat = lambda bs: dev(np.concatenate(bs))
    outf, outb = ctx.zeros(mesh.nNative) + SENTINEL, ctx.zeros(s["B"]) + SENTINEL
    if mode == 0:
        mesh.call("les_face_diffusivity", 0, MU, dev(d["rho"][c]), cat(d["rhob"]), dev(d["nut"][c]), cat(d["nutb"]), outf, outb)
        cell = d["rho"] * (d["nut"] + MU / d["rho"])
        patch = [r * (n + MU / r) for r, n in zip(d["rhob"], d["nutb"])]
    else:
        mesh.call("les_face_diffusivity", 1, MU / 0.7, None, None, dev(d["alphat"][c]), cat(d["alphatb"]), outf, outb)
        cell = MU / 0.7 + d["alphat"]
        patch = [MU / 0.7 + b for b in d["alphatb"]]
    want, _ = fv.interpolate(m, cell, patch)
    assert np.array_equal(_bits(mesh.from_native(outf)), _bits(want[f]))
    assert np.array_equal(_bits(outb.cpu().numpy()), _bits(np.concatenate(patch)))
    if mode == 0:                                               # the floor: nut_b = 0 leaves the molecular part, rho_b*(mu/rho_b)
        q = [p.name for p in m.patches].index("floor")
        assert np.array_equal(_bits(patch[q]), _bits(d["rhob"][q] * (0.0 + MU / d["rhob"][q])))
    # only real faces are written (as ffm_fvc_interpolate)
    assert np.array_equal(_bits(outf.cpu().numpy()[s["pad"]]), _bits(np.full(int(s["pad"].sum()), SENTINEL)))


@pytest.mark.parametrize("name", ["hex", "w32multi"])
def test_keqn_update_against_numpy_and_on_one_cell(meshes, O, ctx, name):
    s = meshes(name); mesh, N = s["mesh"], s["N"]
    d = _inputs(s, O)
    k0 = d["k"].copy(); k0[1] = 1e-17; k0[2] = 0.0; k0[3] = -1e-6            # below SMALL, zero, negative (an unbounded solve): bounded
    dev = ctx.to_device
    for n in (N, 1):
        k, nut, alphat = dev(k0), ctx.zeros(N) + SENTINEL, ctx.zeros(N) + SENTINEL
        mesh.call("les_keqn_update", n, SMALL, CK, PRT, k, dev(d["delta"]), dev(d["rho"]), nut, alphat)
        kb = np.maximum(k0, SMALL)
        want_nut = CK * np.sqrt(kb) * d["delta"]
        want_alphat = d["rho"] * want_nut / PRT
        assert kb[N // 2] == SMALL and kb[1] == SMALL and kb[2] == SMALL and kb[3] == SMALL
        for got, want, before, what in ((k, kb, k0, "k"), (nut, want_nut, None, "nut"), (alphat, want_alphat, None, "alphat")):
            got = got.cpu().numpy()
            assert np.array_equal(_bits(got[:n]), _bits(want[:n])), (what, n)
            rest = np.full(N - n, SENTINEL) if before is None else before[n:]
            assert np.array_equal(_bits(got[n:]), _bits(rest)), (what, n, "cells beyond n touched")
    with pytest.raises(Exception, match=r"failed \(-1\)"):
        mesh.call("les_keqn_update", N + 1, SMALL, CK, PRT, dev(k0), dev(d["delta"]), dev(d["rho"]), ctx.zeros(N), ctx.zeros(N))
