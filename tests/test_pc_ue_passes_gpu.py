"""The passes of the pressure corrector and UEqn that form a face field where it is used (csrc/ffm_fused.hip: ffm_pc_face_fluxes,
ffm_pc_finish, ffm_ue_buoyancy_source3; csrc/ffm_fv.hip: ffm_fvm_transport_scheme; ffm_fvm_pressure_eqn with lower = NULL) against the
chain of entry points each replaces.  Every assertion is a byte comparison: the new kernels copy the expressions and the summation
order of the kernels they replace, FMA contraction off, and a face value that both cells of a face need is formed by both from the
same operands in the same roles.

Meshes: a 5 x 6 x 7 hex box (210 cells: three full 64-cell slices and a partial one) in the level numbering and in tile numbering,
the sheared box of tests/test_fv_operators_gpu.py, and the merged meshes `w4` and `w8` of tests/merged_mesh.py (W = 4, 8).  The two
cell passes refuse `w16u14` (W = 16) with every output untouched; the owner-row pass also runs on `w32multi`.  Face outputs are
pre-filled with a pattern: the padding slots of the cells' slice rows must have been written with 0, and the entries of the last
slice that belong to no cell must still hold the pattern."""
import numpy as np
import pytest

import merged_mesh as MM

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
UNSUPPORTED = r"failed \(-5\)"                 # FFM_ERR_UNSUPPORTED through binding._check
BAD_ARG = r"failed \(-1\)"                     # FFM_ERR_ARG
MESHES = ["hex", "hex_tile", "sheared", "w4", "w8"]
BUCKET = {"hex": 3, "hex_tile": 3, "sheared": 3, "w4": 4, "w8": 8, "w16u14": 16, "w32multi": 32}


def _box_mesh(ffm, ctx, m, tiled):
    """MM.device_mesh for a hex box, optionally in tile numbering (tiles of 3 x 3 cell columns)"""
    N, F = m.nCells, m.nFaces
    hint = ffm.tile_hint_from_centres(m.C.T.copy(), tileCells=3) if tiled else None
    cOrd, fOrd = ffm.renumber_levels(N, m.l, m.u, groupHint=hint)
    l2, u2, oldToNew = ffm.hexmesh.apply_renumbering(N, m.l, m.u, cOrd, fOrd)
    A = ffm.lduMatrix(ctx, N, l2, u2, groupHint=None if hint is None else hint[cOrd])
    patches = [(oldToNew[p.faceCells].astype(np.int32), p.Sf.T.copy(), p.deltaCoeffs) for p in m.patches]
    mesh = ffm.fvMesh(A, m.V[cOrd], m.C[cOrd].T.copy(), m.Sf[fOrd].T.copy(), m.magSf[fOrd], m.weights[fOrd], m.deltaCoeffs[fOrd], patches)
    wu, wl = MM.widths(l2, u2)
    return dict(m=m, A=A, mesh=mesh, N=N, F=F, B=sum(p.size for p in m.patches), W=MM.bucket(max(wu, wl)))


def _make(name, ffm, ctx):
    from oracle import fv, plume
    if name in ("hex", "hex_tile"):
        s = _box_mesh(ffm, ctx, plume.make_mesh((5, 6, 7), h=0.1), name == "hex_tile")
    elif name == "sheared":
        m = plume.make_mesh((7, 6, 5), h=0.1)
        fv.shear(m, [[1.0, 0.35, 0.1], [0.0, 1.0, 0.25], [0.0, 0.0, 1.0]])
        s = _box_mesh(ffm, ctx, m, False)
    else:
        s = MM.device_mesh(ffm, ctx, MM.case(name))
    assert s["W"] == BUCKET[name]
    s["name"] = name
    # the padding entries of the native face layout: where a field of ones comes back 0
    mesh = s["mesh"]
    s["pad"] = mesh.to_native(np.ones(s["F"])).cpu().numpy() == 0.0
    assert int(s["pad"].sum()) == mesh.nNative - s["F"]
    # of these, the slots of a cell's slice row (ffm_pc_phig writes 0 there); the rest are lanes of the last slice without a cell
    one, out = ctx.zeros(mesh.nNative) + 1.0, ctx.zeros(mesh.nNative) + SENTINEL
    mesh.call("pc_phig", one, one, ctx.zeros(s["N"]) + 1.0, out)
    s["rowpad"] = s["pad"] & (out.cpu().numpy() == 0.0)
    assert s["rowpad"].any()
    return s


@pytest.fixture(scope="module")
def meshes(ffm, ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _make(name, ffm, ctx)
        return made[name]
    yield get
    for s in made.values():
        s["mesh"].close(); s["A"].close()


def _h(O, seed, n, lo=0.0, hi=1.0):
    return lo + (hi - lo) * O.hash_u(seed, np.arange(n))


def _bits(t):
    return t.cpu().numpy().view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _untouched(outs):
    return all(np.array_equal(_bits(o), np.full(o.numel(), SENTINEL).view(np.uint64)) for o in outs)


def _pad_zero(s, t):
    """0 in the padding slots of the rows, the pattern where no row is"""
    b, nowhere = _bits(t), s["pad"] & ~s["rowpad"]
    return (np.array_equal(b[s["rowpad"]], np.zeros(int(s["rowpad"].sum()), np.uint64))
            and np.array_equal(b[nowhere], np.full(int(nowhere.sum()), SENTINEL).view(np.uint64)))


def _corrector_inputs(s, O, ctx):
    """the random fields of tests/test_fused_gpu.py's pressure-corrector tests"""
    mesh, N, F, B = s["mesh"], s["N"], s["F"], s["B"]
    dev = ctx.to_device
    nat = lambda seed, lo, hi: mesh.to_native(_h(O, seed, F, lo, hi))
    d = dict(rho=dev(_h(O, 60, N, 1.0, 1.3)), prgh=dev(_h(O, 61, N, -5.0, 5.0)), rhorAU=dev(_h(O, 74, N, 1e-3, 2e-3)),
             ghf=nat(72, -9.0, 0.0), dcorr=nat(73, -0.5, 0.5), H=[dev(_h(O, 50 + c, N, -0.5, 0.5)) for c in range(3)],
             up=nat(41, -1.0, -0.2), lo=nat(42, -2.0, -1.1), rAU=dev(_h(O, 55, N, 0.5, 1.5)), gh=dev(_h(O, 65, N, -9.0, 0.0)),
             p0=dev(_h(O, 62, N, 1.0e5 - 50.0, 1.0e5 + 50.0)), rho0=dev(_h(O, 64, N, 1.0, 1.3)),
             phib=dev(_h(O, 70, B, -0.1, 0.1)), tb=dev(_h(O, 75, B, -3.0, 3.0)))
    return d


@pytest.mark.parametrize("name", MESHES + ["w32multi"])
def test_pc_face_fluxes_equal_interpolate_phig_phiHbyA(meshes, O, ctx, name):
    """ffm_pc_face_fluxes == ffm_fvc_interpolate(NULL, rhorAU) -> ffm_pc_phig -> ffm_pc_phiHbyA: rhorAUf, phig and phiHbyA on every face
    (ffm_fvc_interpolate writes the real faces only), the padding slots of the rows 0, nothing written elsewhere"""
    s = meshes(name); mesh = s["mesh"]
    d = _corrector_inputs(s, O, ctx)
    new = [ctx.zeros(mesh.nNative) + SENTINEL for _ in range(3)]
    mesh.call("pc_face_fluxes", d["rhorAU"], d["ghf"], d["rho"], *d["H"], d["dcorr"], *new)
    raf, phig, phiH = ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative) + SENTINEL, ctx.zeros(mesh.nNative) + SENTINEL
    mesh.call("fvc_interpolate", None, d["rhorAU"], raf)
    mesh.call("pc_phig", raf, d["ghf"], d["rho"], phig)
    mesh.call("pc_phiHbyA", d["rho"], *d["H"], raf, d["dcorr"], phig, phiH)
    for got, want, what in zip(new, (raf, phig, phiH), ("rhorAUf", "phig", "phiHbyA")):
        assert np.array_equal(_bits(got)[~s["pad"]], _bits(want)[~s["pad"]]), what
        assert _pad_zero(s, got), what
    assert _same(new[1], phig) and _same(new[2], phiH)


def _finish_args(s, ctx, d, up, lo, raf, phig, phiH, outs):
    phi, U, K, p, dpdt, rho = outs
    return (1000.0, 1.0e5, up, lo, d["prgh"], phiH, phig, raf, d["phib"], d["tb"], d["rAU"], d["H"], d["gh"], d["p0"], d["rho0"],
            phi, U, K, p, dpdt, rho)


def _finish_outputs(s, ctx, d):
    mesh, N = s["mesh"], s["N"]
    return [ctx.zeros(mesh.nNative) + SENTINEL, [ctx.zeros(N) + SENTINEL for _ in range(3)], ctx.zeros(N) + SENTINEL,
            ctx.zeros(N) + SENTINEL, ctx.zeros(N) + SENTINEL, d["rho"].clone()]


def _faces_for_finish(s, O, ctx, d):
    mesh = s["mesh"]
    raf_h = _h(O, 71, s["F"], 1e-3, 2e-3); raf_h[::11] = 0.0            # rhorAUf == 0: t = 0 on those faces
    raf = mesh.to_native(raf_h)
    phig, phiH = mesh.to_native(_h(O, 76, s["F"], -0.2, 0.2)), mesh.to_native(_h(O, 32, s["F"], -0.15, 0.15))
    return raf, phig, phiH


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("name", MESHES)
def test_pc_finish_equals_the_chain_after_the_solve(meshes, O, ctx, name, symmetric):
    """ffm_pc_finish == ffm_pc_flux -> ffm_fvc_reconstruct -> U = HbyA + rAU*rec, K, p, dpdt (pc_flux_U's lambda, the density that comes
    in) -> ffm_fvc_rho_eqn: phi (padding 0), U[3], K, p, dpdt and rho, rho being the same buffer for input and output.  upper != lower
    shows the roles of the pair; symmetric: one array in both roles, as the driver passes it."""
    s = meshes(name); mesh, N = s["mesh"], s["N"]
    d = _corrector_inputs(s, O, ctx)
    raf, phig, phiH = _faces_for_finish(s, O, ctx, d)
    up, lo = d["up"], (d["up"] if symmetric else d["lo"])
    outs = _finish_outputs(s, ctx, d)
    mesh.call("pc_finish", *_finish_args(s, ctx, d, up, lo, raf, phig, phiH, outs))
    phi, U, K, p, dpdt, rho = outs
    fl, phi2, t = (ctx.zeros(mesh.nNative) + SENTINEL for _ in range(3))
    mesh.call("pc_flux", up, lo, d["prgh"], phiH, phig, raf, fl, phi2, t)
    rec = [ctx.zeros(N) for _ in range(3)]
    mesh.call("fvc_reconstruct", t, d["tb"], *rec)
    a, b, c = (d["H"][i] + d["rAU"] * rec[i] for i in range(3))
    pp = d["prgh"] + d["rho"] * d["gh"] + 1.0e5
    rho2 = ctx.zeros(N)
    mesh.call("fvc_rho_eqn", 1000.0, phi2, d["phib"], d["rho0"], rho2)
    assert _same(phi, phi2) and _pad_zero(s, phi)
    for i, (got, want) in enumerate(zip(U, (a, b, c))):
        assert _same(got, want), i
    assert _same(K, 0.5 * ((a * a + b * b) + c * c))
    assert _same(p, pp) and _same(dpdt, 1000.0 * (pp - d["p0"]))
    assert _same(rho, rho2)
    assert (t.cpu().numpy()[~s["pad"]] == 0.0).any() and (t.cpu().numpy()[~s["pad"]] != 0.0).any()


def test_pc_finish_refuses_rows_wider_than_8(meshes, O, ffm, ctx):
    s = meshes("w16u14"); mesh = s["mesh"]
    d = _corrector_inputs(s, O, ctx)
    raf, phig, phiH = _faces_for_finish(s, O, ctx, d)
    outs = _finish_outputs(s, ctx, d)
    outs[5] = ctx.zeros(s["N"]) + SENTINEL
    with pytest.raises(ffm.FfmError, match=UNSUPPORTED):
        mesh.call("pc_finish", *_finish_args(s, ctx, d, d["up"], d["lo"], raf, phig, phiH, outs))
    assert _untouched([outs[0], *outs[1], *outs[2:]])


@pytest.mark.parametrize("name", MESHES)
def test_pressure_eqn_without_lower(meshes, O, ctx, name):
    """ffm_fvm_pressure_eqn with lower = NULL: upper, diag and source equal to the call with lower given (whose lower == upper)"""
    s = meshes(name); mesh, N, F, B = s["mesh"], s["N"], s["F"], s["B"]
    dev = ctx.to_device
    psi, psi0 = dev(_h(O, 60, N, 1e-5, 2e-5)), dev(_h(O, 61, N, 1e-5, 2e-5))
    p0, rho, rho0, gh = dev(_h(O, 62, N, -50.0, 50.0)), dev(_h(O, 63, N, 1.0, 1.3)), dev(_h(O, 64, N, 1.0, 1.3)), dev(_h(O, 65, N, -9.0, 0.0))
    gam, gamb = mesh.to_native(_h(O, 66, F, 1e-3, 2e-3)), dev(_h(O, 67, B, 1e-3, 2e-3))
    phiH, phiHb = mesh.to_native(_h(O, 32, F, -0.15, 0.15)), dev(_h(O, 70, B, -0.1, 0.1))
    f, ref, rg = dev(np.round(_h(O, 80, B) * 2) / 2), dev(_h(O, 84, B)), dev(_h(O, 88, B, -0.5, 0.5))
    ic, bc = ctx.zeros(B), ctx.zeros(B)
    mesh.call("fvm_boundary_coeffs", None, gamb, -1, f, ref, rg, ic, bc)
    res = []
    for with_lower in (True, False):
        up, lo = ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative) + SENTINEL
        dO, sO = ctx.zeros(N), ctx.zeros(N)
        mesh.call("fvm_pressure_eqn", 1000.0, psi, psi0, p0, rho, rho0, gh, 1.0e5, gam, phiH, phiHb, ic, bc, up, lo if with_lower else None, dO, sO)
        res.append((up, dO, sO, lo))
    for a, b in zip(res[0][:3], res[1][:3]):
        assert _same(a, b)
    assert np.array_equal(_bits(res[0][3])[~s["pad"]], _bits(res[0][0])[~s["pad"]])
    assert _untouched([res[1][3]])


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("scheme", [0, 1, 4])
@pytest.mark.parametrize("name", MESHES)
def test_transport_scheme_equals_weights_then_transport(meshes, O, ctx, name, scheme, mixed):
    """ffm_fvm_transport_scheme(upwind 0 | linear 1 | LUST 4) == ffm_fv_limited_weights(scheme) + ffm_fvm_transport: diag, upper and lower,
    with positive and with mixed-sign fluxes that include exact zeros"""
    s = meshes(name); mesh, N, F = s["mesh"], s["N"], s["F"]
    ph = _h(O, 32, F, -0.15, 0.15) if mixed else _h(O, 32, F, 0.01, 0.3)
    ph[::7] = 0.0
    phi, gam, rho = mesh.to_native(ph), mesh.to_native(_h(O, 63, F, 0.01, 0.02)), ctx.to_device(_h(O, 60, N, 1.0, 2.0))
    new = [ctx.zeros(N) + SENTINEL, ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative)]
    mesh.call("fvm_transport_scheme", 1000.0, rho, phi, scheme, gam, -1, *new)
    w = ctx.zeros(mesh.nNative)
    mesh.call("fv_limited_weights", scheme, 1.0, 0.0, 1.0, phi, None, None, None, None, w)
    old = [ctx.zeros(N), ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative)]
    mesh.call("fvm_transport", 1000.0, rho, phi, w, gam, -1, *old)
    for got, want, what in zip(new, old, ("diag", "upper", "lower")):
        assert _same(got, want), what
    assert not _same(old[1], old[2])


def test_transport_scheme_refuses_a_limited_scheme(meshes, O, ffm, ctx):
    s = meshes("hex"); mesh, N, F = s["mesh"], s["N"], s["F"]
    phi, gam, rho = mesh.to_native(_h(O, 32, F, -0.15, 0.15)), mesh.to_native(_h(O, 63, F, 0.01, 0.02)), ctx.to_device(_h(O, 60, N, 1.0, 2.0))
    out = [ctx.zeros(N) + SENTINEL, ctx.zeros(mesh.nNative) + SENTINEL, ctx.zeros(mesh.nNative) + SENTINEL]
    with pytest.raises(ffm.FfmError, match=BAD_ARG):
        mesh.call("fvm_transport_scheme", 1000.0, rho, phi, 2, gam, -1, *out)
    assert _untouched(out)


def _buoyancy(s, O, ctx):
    N, B = s["N"], s["B"]
    dev = ctx.to_device
    d = _corrector_inputs(s, O, ctx)
    d.update(ic=[dev(_h(O, 46 + c, B, 0.0, 0.4)) for c in range(3)], bc=[dev(_h(O, 49 + c, B, -0.3, 0.3)) for c in range(3)],
             diag=dev(_h(O, 56, N, 1.0, 2.0)), src=[dev(_h(O, 43 + c, N, -0.5, 0.5)) for c in range(3)])
    outs = [[ctx.zeros(N) + SENTINEL for _ in range(3)], [ctx.zeros(N) + SENTINEL for _ in range(3)]]
    return d, outs


@pytest.mark.parametrize("name", MESHES)
def test_ue_buoyancy_source3_equals_flux_reconstruct_add_boundary(meshes, O, ctx, name):
    """ffm_ue_buoyancy_source3 == ffm_ue_buoyancy_flux -> ffm_fvc_reconstruct -> ffm_fvm_add_boundary per component (su = rec_c): the
    diagonals and sources of the three components; source, internalCoeffs and boundaryCoeffs stay as they were"""
    s = meshes(name); mesh, N = s["mesh"], s["N"]
    d, (dO, sO) = _buoyancy(s, O, ctx)
    keep = [x.clone() for x in d["src"] + d["ic"] + d["bc"]]
    mesh.call("ue_buoyancy_source3", d["ghf"], d["rho"], d["prgh"], d["tb"], d["ic"], d["bc"], d["diag"], d["src"], dO, sO)
    t = ctx.zeros(mesh.nNative)
    mesh.call("ue_buoyancy_flux", d["ghf"], d["rho"], d["prgh"], t)
    rec = [ctx.zeros(N) for _ in range(3)]
    mesh.call("fvc_reconstruct", t, d["tb"], *rec)
    for c in range(3):
        d2, s2 = ctx.zeros(N), ctx.zeros(N)
        mesh.call("fvm_add_boundary", d["ic"][c], d["bc"][c], d["diag"], d["src"][c], rec[c], d2, s2)
        assert _same(dO[c], d2) and _same(sO[c], s2), c
    assert all(_same(a, b) for a, b in zip(keep, d["src"] + d["ic"] + d["bc"]))
    assert not _same(dO[0], dO[1])


def test_ue_buoyancy_source3_refuses_rows_wider_than_8(meshes, O, ffm, ctx):
    s = meshes("w16u14"); mesh = s["mesh"]
    d, (dO, sO) = _buoyancy(s, O, ctx)
    with pytest.raises(ffm.FfmError, match=UNSUPPORTED):
        mesh.call("ue_buoyancy_source3", d["ghf"], d["rho"], d["prgh"], d["tb"], d["ic"], d["bc"], d["diag"], d["src"], dO, sO)
    assert _untouched(dO + sO)
