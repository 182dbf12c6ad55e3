"""The fused assembly passes (csrc/ffm_fused.hip: ffm_fvc_grad_multi, ffm_fvm_scalar_transport_multi, ffm_fvm_lust_source3) must
give, bit for bit, what the chain of per-operator entry points gives (each of which is compared with the oracle in
tests/test_fv_operators_gpu.py): same expressions, same order, FMA contraction off.  And the compiled time step built on them
must equal the one built on the per-operator kernels (FFM_PLUME_UNFUSED) in every field, bitwise.

The same for the other entry points of the compiled time step (ffm_fvc_div_phiK_terms, ffm_fvc_rho_eqn, ffm_fvc_ddt_corr,
ffm_fvc_flux_rho, ffm_fvm_HbyA3, ffm_fvm_pressure_eqn, ffm_pc_phig / _phiHbyA / _flux, ffm_ue_buoyancy_flux, ffm_fvdom_ray_assemble_d):
each against the `_ops` chain of csrc/ffm_plume_step.hip it replaced, bitwise, and against oracle/fv.py.

Row-width buckets (FFM_DISPATCH_W of csrc/ffm_device.hpp): the tests that take `setup` run on the hex box (W = 3) and, through
TestMergedMeshes, on the merged meshes `w4`, `w8`, `w16u14`, `w32l30`, `w32multi`, `w32u18` of tests/merged_mesh.py (W = 4, 8, 16, 32, 32, 32); the ray
assembly on hex, `w8`, `w16u14`, `w32l30`, `w32u18`.  The entry points that pick their bucket by hand must refuse the rows they were not built for
(div_phiK: W > 8; rho_eqn: W > 16; the tiled multivariate weights: W > 3) with FFM_ERR_UNSUPPORTED and leave their outputs untouched.
The time-step and tiled-weights tests build their own box meshes (W = 3; the decomposed plume elsewhere reaches W = 8)."""
import os
from ctypes import c_int as C_int

import numpy as np
import pytest

import merged_mesh as MM
from common import rel_l2

pytestmark = pytest.mark.gpu


MESHES = ["hex", "w4", "w8", "w16u14", "w32l30", "w32multi", "w32u18"]
BUCKET = {"hex": 3, "w4": 4, "w8": 8, "w16u14": 16, "w32l30": 32, "w32multi": 32, "w32u18": 32}


def _bucket(s):
    """the row width FFM_DISPATCH_W picks, from the addressing the library was given"""
    return MM.bucket(max(np.bincount(s["l"]).max(), np.bincount(s["u"]).max()))


def _setup(name, ffm, ctx):
    from oracle import fv, plume
    m = plume.make_mesh((9, 8, 7), h=0.1) if name == "hex" else MM.case(name)
    s = MM.device_mesh(ffm, ctx, m, face_centres=True)
    assert _bucket(s) == BUCKET[name]
    if name != "hex":
        assert (s["wu"], s["wl"]) == MM.CASES[name][4:6]
    s.update(fv=fv, name=name)
    yield s
    s["mesh"].close(); s["A"].close()


@pytest.fixture(scope="module")
def setup(O, ffm, ctx):
    yield from _setup("hex", ffm, ctx)


def _fields(s, O, ctx, nf):
    N, F, B, mesh = s["N"], s["F"], s["B"], s["mesh"]
    dev = ctx.to_device
    vf = [dev(0.2 + O.hash_u(31 + 7 * i, np.arange(N))) for i in range(nf)]
    # one field that is constant over most of the mesh (exercises the large-ratio branch of NVDTVD::r)
    a = 0.2 + O.hash_u(31, np.arange(N)); vf[0] = dev(np.where(a > 0.9, a, 0.25))
    vb = [dev(0.1 + O.hash_u(133 + i, np.arange(B))) for i in range(nf)]
    phi = mesh.to_native(0.3 * (O.hash_u(32, np.arange(F)) - 0.5))
    return vf, vb, phi


@pytest.mark.parametrize("nf", [1, 3, 4])
def test_grad_multi_equals_grad(setup, O, ctx, nf):
    s, mesh = setup, setup["mesh"]
    vf, vb, _ = _fields(s, O, ctx, nf)
    g = [[ctx.zeros(s["N"]) for _ in range(3)] for _ in range(nf)]
    mesh.call("fvc_grad_multi", nf, vf, vb, [x[0] for x in g], [x[1] for x in g], [x[2] for x in g])
    for i in range(nf):
        r = [ctx.zeros(s["N"]) for _ in range(3)]
        mesh.call("fvc_grad", vf[i], vb[i], *r)
        for d in range(3):
            assert np.array_equal(g[i][d].cpu().numpy(), r[d].cpu().numpy()), (i, d)


@pytest.mark.parametrize("nf,scheme,with_expl", [(4, 3, False), (1, 2, True), (2, 2, False)])
def test_scalar_transport_multi_equals_the_operator_chain(setup, O, ctx, nf, scheme, with_expl):
    s, mesh = setup, setup["mesh"]
    N, F, B = s["N"], s["F"], s["B"]
    dev = ctx.to_device
    vf, vb, phi = _fields(s, O, ctx, nf)
    if scheme == 3:
        vf = [v * 1.1 - 0.2 for v in vf]                          # some values outside [0, 1]
    rho, rho0 = dev(1.0 + O.hash_u(60, np.arange(N))), dev(1.0 + O.hash_u(61, np.arange(N)))
    vf0 = [dev(O.hash_u(62 + i, np.arange(N))) for i in range(nf)]
    gam = mesh.to_native(0.01 * (1 + O.hash_u(63, np.arange(F)))); gamb = dev(0.01 * (1 + O.hash_u(64, np.arange(B))))
    phib = dev(0.2 * (O.hash_u(70, np.arange(B)) - 0.5))
    f = [dev(np.round(O.hash_u(80 + i, np.arange(B)) * 2) / 2) for i in range(nf)]
    ref = [dev(O.hash_u(84 + i, np.arange(B))) for i in range(nf)]
    rg = [dev(O.hash_u(88 + i, np.arange(B)) - 0.5) for i in range(nf)]
    su = [dev(O.hash_u(90 + i, np.arange(N)) - 0.3) if i % 2 == 0 else None for i in range(nf)]
    expl = [dev(O.hash_u(95 + e, np.arange(N)) - 0.5) for e in range(3)] if with_expl else None
    # a second explicit source and an implicit one (radiation->Sh in the enthalpy equation): on the first field when expl is on
    su2 = [dev(O.hash_u(98, np.arange(N)) - 0.2) if (with_expl and i == 0) else None for i in range(nf)]
    sp = [dev(O.hash_u(99, np.arange(N))) if (with_expl and i == 0) else None for i in range(nf)]
    rdt = 1000.0
    # gradients of the fields (the limiter's input)
    g = [[ctx.zeros(N) for _ in range(3)] for _ in range(nf)]
    for i in range(nf):
        mesh.call("fvc_grad", vf[i], vb[i], *g[i])
    D = [ctx.zeros(N) for _ in range(nf)]; S = [ctx.zeros(N) for _ in range(nf)]
    Up = [ctx.zeros(mesh.nNative) for _ in range(nf)]; Lo = [ctx.zeros(mesh.nNative) for _ in range(nf)]
    mesh.call("fvm_scalar_transport_multi", nf, scheme, 1.0, 0.0, 1.0, rdt, rho, rho0, phi, phib, gam, gamb,
              vf, [x[0] for x in g], [x[1] for x in g], [x[2] for x in g], vf0, f, ref, rg, su, su2, sp,
              (expl + [None] * (3 * (nf - 1))) if with_expl else None, D, Up, Lo, S)
    V = dev(s["m"].V[s["cOrd"]])
    for i in range(nf):
        w = ctx.zeros(mesh.nNative)
        mesh.call("fv_limited_weights", scheme, 1.0, 0.0, 1.0, phi, vf[i], *g[i], w)
        d, up, lo = ctx.zeros(N), ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative)
        mesh.call("fvm_transport", rdt, rho, phi, w, gam, -1, d, up, lo)
        ic, bc = ctx.zeros(B), ctx.zeros(B)
        mesh.call("fvm_boundary_coeffs", phib, gamb, -1, f[i], ref[i], rg[i], ic, bc)
        src = rdt * rho0 * vf0[i] * V
        if with_expl and i == 0:
            src = ((src - V * expl[0]) - V * expl[1]) - V * expl[2]
        if su[i] is not None:
            src = src + V * su[i]
        if sp[i] is not None:
            d = d + V * sp[i]
        if su2[i] is not None:
            src = src + V * su2[i]
        dO, sO = ctx.zeros(N), ctx.zeros(N)
        mesh.call("fvm_add_boundary", ic, bc, d, src, None, dO, sO)
        assert np.array_equal(Up[i].cpu().numpy(), up.cpu().numpy()), i
        assert np.array_equal(Lo[i].cpu().numpy(), lo.cpu().numpy()), i
        assert np.array_equal(D[i].cpu().numpy(), dO.cpu().numpy()), i
        assert np.array_equal(S[i].cpu().numpy(), sO.cpu().numpy()), i


@pytest.mark.parametrize("nf", [2, 6])
def test_multivariate_weights_equal_the_running_minimum_chain(setup, O, ctx, nf):
    """multivariateSelectionScheme: the weights of ONE limiter, the minimum over the fields' own limitedLinear / limitedLinear01
    limiters.  The one-pass kernel (ffm_fv_multivariate_weights, the compiled time step) = ffm_fv_limited_limiter over the fields
    (running minimum) + ffm_fv_weights_from_limiter (what the Foam layer's convectionScheme calls), bit for bit; and the minimum of the
    fields' own weights can be recovered from it where the limiter is 0 or 1."""
    import ctypes as C
    s, mesh = setup, setup["mesh"]
    N = s["N"]
    vf, vb, phi = _fields(s, O, ctx, nf)
    vf = [v * 1.1 - 0.2 if i % 2 else v for i, v in enumerate(vf)]           # limitedLinear01 fields with values outside [0, 1]
    sch = [2 if i == 0 else 3 for i in range(nf)]
    g = [[ctx.zeros(N) for _ in range(3)] for _ in range(nf)]
    for i in range(nf):
        mesh.call("fvc_grad", vf[i], vb[i], *g[i])
    w1 = ctx.zeros(mesh.nNative)
    mesh.call("fv_multivariate_weights", nf, (C.c_int * nf)(*sch), 1.0, 0.0, 1.0, phi, vf, [x[0] for x in g], [x[1] for x in g], [x[2] for x in g], w1)
    lim, w2 = ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative)
    for i in range(nf):
        mesh.call("fv_limited_limiter", sch[i], 1.0, 0.0, 1.0, phi, vf[i], *g[i], lim, 0 if i == 0 else 1)
    mesh.call("fv_weights_from_limiter", phi, lim, w2)
    assert np.array_equal(w1.cpu().numpy(), w2.cpu().numpy())
    # against the per-field weights: limiter_i = (w_i - upwind)/(linear - upwind); the common limiter is their minimum (real faces only:
    # the native layout has padding entries)
    fn = mesh.from_native
    up = (fn(phi) >= 0).astype(float)
    wl = ctx.zeros(mesh.nNative); mesh.call("fv_limited_weights", 1, 1.0, 0.0, 1.0, phi, None, None, None, None, wl)
    lims = []
    for i in range(nf):
        wi = ctx.zeros(mesh.nNative)
        mesh.call("fv_limited_weights", sch[i], 1.0, 0.0, 1.0, phi, vf[i], *g[i], wi)
        lims.append((fn(wi) - up) / (fn(wl) - up))
    assert np.allclose(np.min(lims, axis=0), fn(lim), rtol=0, atol=1e-12)
    assert float(np.mean(fn(lim) > 0)) < 0.999 and (nf > 2 or float(np.mean(fn(lim) > 0)) > 0.02)      # (six random fields: the minimum is 0 nearly everywhere)


@pytest.mark.parametrize("nf,with_expl", [(4, False), (1, True)])
def test_scalar_transport_multi_with_given_weights_equals_the_operator_chain(setup, O, ctx, nf, with_expl):
    """ffm_fvm_scalar_transport_multi_w (mvConvection->fvmDiv with the common weights + ddt + laplacian + sources + boundary terms of nf
    equations in one pass) against fvm_transport(w) / fvm_boundary_coeffs / fvm_add_boundary per field, bitwise."""
    s, mesh = setup, setup["mesh"]
    N, F, B = s["N"], s["F"], s["B"]
    dev = ctx.to_device
    _, _, phi = _fields(s, O, ctx, nf)
    w = mesh.to_native(O.hash_u(41, np.arange(F)))                             # any weights in [0, 1]
    rho, rho0 = dev(1.0 + O.hash_u(60, np.arange(N))), dev(1.0 + O.hash_u(61, np.arange(N)))
    vf0 = [dev(O.hash_u(62 + i, np.arange(N))) for i in range(nf)]
    gam = mesh.to_native(0.01 * (1 + O.hash_u(63, np.arange(F)))); gamb = dev(0.01 * (1 + O.hash_u(64, np.arange(B))))
    phib = dev(0.2 * (O.hash_u(70, np.arange(B)) - 0.5))
    f = [dev(np.round(O.hash_u(80 + i, np.arange(B)) * 2) / 2) for i in range(nf)]
    ref = [dev(O.hash_u(84 + i, np.arange(B))) for i in range(nf)]
    rg = [dev(O.hash_u(88 + i, np.arange(B)) - 0.5) for i in range(nf)]
    su = [dev(O.hash_u(90 + i, np.arange(N)) - 0.3) if i % 2 == 0 else None for i in range(nf)]
    expl = [dev(O.hash_u(95 + e, np.arange(N)) - 0.5) for e in range(3)] if with_expl else None
    su2 = [dev(O.hash_u(98, np.arange(N)) - 0.2) if (with_expl and i == 0) else None for i in range(nf)]
    sp = [dev(O.hash_u(99, np.arange(N))) if (with_expl and i == 0) else None for i in range(nf)]
    rdt = 1000.0
    D = [ctx.zeros(N) for _ in range(nf)]; S = [ctx.zeros(N) for _ in range(nf)]
    Up = [ctx.zeros(mesh.nNative) for _ in range(nf)]; Lo = [ctx.zeros(mesh.nNative) for _ in range(nf)]
    mesh.call("fvm_scalar_transport_multi_w", nf, w, rdt, rho, rho0, phi, phib, gam, gamb, vf0, f, ref, rg, su, su2, sp,
              (expl + [None] * (3 * (nf - 1))) if with_expl else None, D, Up, Lo, S)
    V = dev(s["m"].V[s["cOrd"]])
    for i in range(nf):
        d, up, lo = ctx.zeros(N), ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative)
        mesh.call("fvm_transport", rdt, rho, phi, w, gam, -1, d, up, lo)
        ic, bc = ctx.zeros(B), ctx.zeros(B)
        mesh.call("fvm_boundary_coeffs", phib, gamb, -1, f[i], ref[i], rg[i], ic, bc)
        src = rdt * rho0 * vf0[i] * V
        if with_expl and i == 0:
            src = ((src - V * expl[0]) - V * expl[1]) - V * expl[2]
        if su[i] is not None:
            src = src + V * su[i]
        if sp[i] is not None:
            d = d + V * sp[i]
        if su2[i] is not None:
            src = src + V * su2[i]
        dO, sO = ctx.zeros(N), ctx.zeros(N)
        mesh.call("fvm_add_boundary", ic, bc, d, src, None, dO, sO)
        assert np.array_equal(Up[i].cpu().numpy(), up.cpu().numpy()), i
        assert np.array_equal(Lo[i].cpu().numpy(), lo.cpu().numpy()), i
        assert np.array_equal(D[i].cpu().numpy(), dO.cpu().numpy()), i
        assert np.array_equal(S[i].cpu().numpy(), sO.cpu().numpy()), i


def test_lust_source3_equals_the_operator_chain(setup, O, ctx):
    s, mesh = setup, setup["mesh"]
    N, B = s["N"], s["B"]
    dev = ctx.to_device
    vf, vb, phi = _fields(s, O, ctx, 3)
    rho0 = dev(1.0 + O.hash_u(61, np.arange(N)))
    U0 = [dev(O.hash_u(62 + i, np.arange(N)) - 0.5) for i in range(3)]
    g = [[ctx.zeros(N) for _ in range(3)] for _ in range(3)]
    for i in range(3):
        mesh.call("fvc_grad", vf[i], vb[i], *g[i])
    out = [ctx.zeros(N) for _ in range(3)]
    rdt = 250.0
    mesh.call("fvm_lust_source3", rdt, phi, rho0, U0, [x[0] for x in g], [x[1] for x in g], [x[2] for x in g], out)
    V = dev(s["m"].V[s["cOrd"]])
    zb = ctx.zeros(B)
    for i in range(3):
        corr = ctx.zeros(mesh.nNative)
        mesh.call("fv_lust_correction", phi, *g[i], corr)
        corr = phi * corr
        divc = ctx.zeros(N)
        mesh.call("fvc_surface_integrate", corr, zb, divc)
        ref = rdt * rho0 * U0[i] * V - V * divc
        assert np.array_equal(out[i].cpu().numpy(), ref.cpu().numpy()), i


# ---- entry points of the compiled time step that no test named before: each against the per-operator chain the unfused driver runs
# (the `_ops` forms of csrc/ffm_plume_step.hip) bit for bit, and against oracle/fv.py (the expressions of oracle/plume.py).  Cell and
# boundary fields are hashed in the device's order; `_o` brings them into the oracle's.  Element-wise steps of a chain are done by
# torch on the device or by numpy on the host: single IEEE operations in the order of the driver's lambdas, no contraction.
SENTINEL = -7.25
UNSUPPORTED = r"failed \(-5\)"                 # FFM_ERR_UNSUPPORTED through binding._check


def _h(O, seed, n, lo=0.0, hi=1.0):
    return lo + (hi - lo) * O.hash_u(seed, np.arange(n))


def _cells_o(s, a):
    out = np.empty(s["N"]); out[s["cOrd"]] = a.cpu().numpy() if hasattr(a, "cpu") else a
    return out


def _faces_o(s, t):
    out = np.empty(s["F"]); out[s["fOrd"]] = s["mesh"].from_native(t)
    return out


def _patches_o(s, a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return np.split(a, np.cumsum([p.size for p in s["m"].patches])[:-1])


def _untouched(outs):
    return all(np.array_equal(o.cpu().numpy().view(np.uint64), np.full(o.numel(), SENTINEL).view(np.uint64)) for o in outs)


def _nat(s, a):
    """a face field of the oracle's mesh in the device's native layout"""
    return s["mesh"].to_native(np.asarray(a)[s["fOrd"]])


@pytest.mark.parametrize("scheme,name", [(2, "limitedLinear"), (3, "limitedLinear01")])
def test_div_phiK_terms_equal_the_operator_chain(setup, O, ffm, ctx, scheme, name):
    """ffm_fvc_div_phiK_terms (k_div_phiK<3|4|8>) == div_phiK_ops: ffm_fv_limited_weights, ffm_fvc_interpolate, the product with phi,
    ffm_fvc_surface_integrate and the two cell expressions, bitwise; divK against oracle/fv.py per cell within the bars of
    tests/test_fv_operators_gpu.py carried through the sum (weights to 1e-13, a row sum to 1e-14 of its terms' magnitudes).  Rows wider
    than 8 are refused (the caller's only protection since the driver dropped its own fall-back) and nothing is written."""
    s, mesh, fv, m = setup, setup["mesh"], setup["fv"], setup["m"]
    N, F, B = s["N"], s["F"], s["B"]
    dev = ctx.to_device
    K = dev(_h(O, 31, N, 0.2, 1.2) * (1.1 if scheme == 3 else 1.0) - (0.2 if scheme == 3 else 0.0))     # scheme 3: values outside [0, 1]
    Kb, phib = dev(_h(O, 133, B, 0.1, 1.1)), dev(_h(O, 70, B, -0.1, 0.1))
    phi = mesh.to_native(_h(O, 32, F, -0.15, 0.15))
    rho, rho0, K0, dpdt = dev(_h(O, 60, N, 1.0, 2.0)), dev(_h(O, 61, N, 1.0, 2.0)), dev(_h(O, 62, N)), dev(_h(O, 63, N, -50.0, 50.0))
    g = [ctx.zeros(N) for _ in range(3)]
    mesh.call("fvc_grad", K, Kb, *g)
    rdt = 1000.0
    out = [ctx.zeros(N) + SENTINEL for _ in range(3)]
    args = (scheme, 1.0, 0.0, 1.0, rdt, phi, phib, K, Kb, *g, rho, rho0, K0, dpdt, *out)
    if _bucket(s) > 8:
        with pytest.raises(ffm.FfmError, match=UNSUPPORTED):
            mesh.call("fvc_div_phiK_terms", *args)
        assert _untouched(out)
        return
    mesh.call("fvc_div_phiK_terms", *args)
    divK, ddtK, ndpdt = out
    wK, Kf, div = ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative), ctx.zeros(N)
    mesh.call("fv_limited_weights", scheme, 1.0, 0.0, 1.0, phi, K, *g, wK)
    mesh.call("fvc_interpolate", wK, K, Kf)
    mesh.call("fvc_surface_integrate", phi * Kf, phib * Kb, div)
    assert np.array_equal(divK.cpu().numpy(), div.cpu().numpy())
    assert np.array_equal(ddtK.cpu().numpy(), (rdt * (rho * K - rho0 * K0)).cpu().numpy())
    assert np.array_equal(ndpdt.cpu().numpy(), (-dpdt).cpu().numpy())
    # the oracle on the same inputs (the gradient is the device's: compared in tests/test_fv_operators_gpu.py)
    Ko, phio = _cells_o(s, K), _faces_o(s, phi)
    go = np.stack([_cells_o(s, x) for x in g], axis=1)
    w = fv.limited_weights(m, name, phio, Ko, go, 1.0)
    tf = phio * (w * Ko[m.l] + (1.0 - w) * Ko[m.u])
    tb = [a * b for a, b in zip(_patches_o(s, phib), _patches_o(s, Kb))]
    ref = fv.surface_integrate(m, tf, tb)
    mag = fv.surface_sum(m, np.abs(tf), [np.abs(b) for b in tb]) / m.V
    dw = fv.surface_sum(m, np.abs(phio * (Ko[m.l] - Ko[m.u])), [np.zeros(p.size) for p in m.patches]) / m.V
    err = np.abs(_cells_o(s, divK) - ref)
    assert np.all(err <= 1e-13 * dw + 1e-14 * mag), float((err / (1e-13 * dw + 1e-14 * mag)).max())
    assert np.array_equal(_cells_o(s, ddtK), rdt * (_cells_o(s, rho) * Ko - _cells_o(s, rho0) * _cells_o(s, K0)))


def test_rho_eqn_equals_surface_integrate_and_the_cell_expression(setup, O, ffm, ctx):
    """ffm_fvc_rho_eqn (k_rho_eqn<3|4|8|16>) == rho_eqn_ops: ffm_fvc_surface_integrate + rho = (rdt rho0 V - V div)/(rdt V), bitwise, and
    the oracle's to 1e-15 rel-L2; rows wider than 16 are refused with rho untouched."""
    s, mesh, fv, m = setup, setup["mesh"], setup["fv"], setup["m"]
    N, F, B = s["N"], s["F"], s["B"]
    dev = ctx.to_device
    phi, phib, rho0 = mesh.to_native(_h(O, 32, F, -0.15, 0.15)), dev(_h(O, 70, B, -0.1, 0.1)), dev(_h(O, 61, N, 1.0, 2.0))
    rdt = 1000.0
    rho = ctx.zeros(N) + SENTINEL
    if _bucket(s) > 16:
        with pytest.raises(ffm.FfmError, match=UNSUPPORTED):
            mesh.call("fvc_rho_eqn", rdt, phi, phib, rho0, rho)
        assert _untouched([rho])
        return
    mesh.call("fvc_rho_eqn", rdt, phi, phib, rho0, rho)
    div = ctx.zeros(N)
    mesh.call("fvc_surface_integrate", phi, phib, div)
    V = dev(m.V[s["cOrd"]])
    assert np.array_equal(rho.cpu().numpy(), ((rdt * rho0 * V - V * div) / (rdt * V)).cpu().numpy())
    r0 = _cells_o(s, rho0)
    ref = (rdt * r0 * m.V - m.V * fv.surface_integrate(m, _faces_o(s, phi), _patches_o(s, phib))) / (rdt * m.V)
    assert rel_l2(_cells_o(s, rho), ref) < 1e-15


def test_flux_rho_and_ddt_corr_equal_the_operator_chain(setup, O, ctx):
    """ffm_fvc_flux_rho == ffm_fvc_flux of the product fields; ffm_fvc_ddt_corr == that flux of the old-time fields + ddtCouplingCoeff's
    face algebra (pc_ddtCorr_ops); both bitwise, and against oracle/plume.py's expressions"""
    s, mesh, fv, m = setup, setup["mesh"], setup["fv"], setup["m"]
    N, F = s["N"], s["F"]
    dev = ctx.to_device
    rho = dev(_h(O, 60, N, 1.0, 2.0)); U = [dev(_h(O, 50 + d, N, -0.5, 0.5)) for d in range(3)]
    fl, ref = ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative)
    mesh.call("fvc_flux_rho", rho, *U, fl)
    mesh.call("fvc_flux", *[rho * u for u in U], ref)
    assert np.array_equal(mesh.from_native(fl), mesh.from_native(ref))
    ro, Uo = _cells_o(s, rho), [_cells_o(s, u) for u in U]
    flo = sum((m.weights * (ro * Uo[d])[m.l] + (1 - m.weights) * (ro * Uo[d])[m.u]) * m.Sf[:, d] for d in range(3))
    assert rel_l2(_faces_o(s, fl), flo) < 1e-15
    # ddtCorr: the old-time flux near the interpolated one on some faces (coefficient close to 1) and far from it on others (0)
    phi0_o = flo * _h(O, 34, F, 0.2, 1.8)
    phi0_o[::5] = -phi0_o[::5]
    phi0 = _nat(s, phi0_o)
    rdt = 1000.0
    dc = ctx.zeros(mesh.nNative)
    mesh.call("fvc_ddt_corr", rdt, rho, *U, phi0, dc)
    p0, f0 = mesh.from_native(phi0), mesh.from_native(fl)
    phiCorr = p0 - f0
    coeff = 1.0 - np.minimum(np.abs(phiCorr) / (np.abs(p0) + 1e-15), 1.0)
    assert np.array_equal(mesh.from_native(dc), coeff * rdt * phiCorr)
    phiCorr = phi0_o - flo
    coeff = 1.0 - np.minimum(np.abs(phiCorr) / (np.abs(phi0_o) + 1e-15), 1.0)
    assert (coeff > 0.5).any() and (coeff == 0.0).any()
    assert rel_l2(_faces_o(s, dc), coeff * rdt * phiCorr) < 1e-14


def _momentum_matrix(s, O, ctx):
    """an asymmetric vector matrix (upper != lower on every face) with per-component patch coefficients, sources and fields"""
    mesh, N, F, B = s["mesh"], s["N"], s["F"], s["B"]
    dev = ctx.to_device
    up, lo = mesh.to_native(_h(O, 41, F, -1.0, -0.2)), mesh.to_native(_h(O, 42, F, -2.0, -1.1))
    src = [dev(_h(O, 43 + d, N, -0.5, 0.5)) for d in range(3)]
    ic = [dev(_h(O, 46 + d, B, 0.0, 0.4)) for d in range(3)]
    bc = [dev(_h(O, 49 + d, B, -0.3, 0.3)) for d in range(3)]
    psi = [dev(_h(O, 52 + d, N, -1.0, 1.0)) for d in range(3)]
    rAU = dev(_h(O, 55, N, 0.5, 1.5))
    return up, lo, src, ic, bc, psi, rAU


def test_HbyA3_equals_three_H_passes(setup, O, ctx):
    """ffm_fvm_HbyA3 (k_matrix_HbyA3<W>) == ffm_fvm_H per component followed by the product with rAU (pc_HbyA_ops), bitwise, and
    fvMatrix<vector>::H() of oracle/fv.py times rAU at 1e-14; upper and lower differ on every face, so transposing a pair shows"""
    s, mesh, fv, m = setup, setup["mesh"], setup["fv"], setup["m"]
    N = s["N"]
    up, lo, src, ic, bc, psi, rAU = _momentum_matrix(s, O, ctx)
    out = [ctx.zeros(N) for _ in range(3)]
    mesh.call("fvm_HbyA3", up, lo, src, ic, bc, psi, rAU, out)
    M = fv.Matrix(m, 3)
    M.upper, M.lower = _faces_o(s, up), _faces_o(s, lo)
    M.source = np.stack([_cells_o(s, x) for x in src])
    for q in range(len(m.patches)):
        M.internalCoeffs[q] = np.stack([_patches_o(s, ic[d])[q] for d in range(3)])
        M.boundaryCoeffs[q] = np.stack([_patches_o(s, bc[d])[q] for d in range(3)])
    Ho = M.H(np.stack([_cells_o(s, x) for x in psi]))
    for d in range(3):
        h = ctx.zeros(N)
        mesh.call("fvm_H", 3, d, up, lo, src[d], ic[0], ic[1], ic[2], bc[d], psi[d], h)
        assert np.array_equal(out[d].cpu().numpy(), (rAU * h).cpu().numpy()), d
        assert rel_l2(_cells_o(s, out[d]), _cells_o(s, rAU) * Ho[d]) < 1e-14, d
    mesh.call("fvm_HbyA3", up, lo, src, ic, bc, psi, None, out)           # rAU null: H itself
    for d in range(3):
        h = ctx.zeros(N)
        mesh.call("fvm_H", 3, d, up, lo, src[d], ic[0], ic[1], ic[2], bc[d], psi[d], h)
        assert np.array_equal(out[d].cpu().numpy(), h.cpu().numpy()), d


def test_pressure_eqn_equals_the_operator_chain(setup, O, ctx):
    """ffm_fvm_pressure_eqn (k_p_rgh_eqn<W>) == pc_p_rgh_eqn_ops: ffm_fvm_transport (laplacian only), ffm_fvc_surface_integrate, the source
    expression and ffm_fvm_add_boundary, bitwise; and the matrix oracle/plume.py's p_corrector builds from the same inputs"""
    s, mesh, fv, m = setup, setup["mesh"], setup["fv"], setup["m"]
    N, F, B = s["N"], s["F"], s["B"]
    dev = ctx.to_device
    psi, psi0 = dev(_h(O, 60, N, 1e-5, 2e-5)), dev(_h(O, 61, N, 1e-5, 2e-5))
    p0, rho, rho0, gh = dev(_h(O, 62, N, -50.0, 50.0)), dev(_h(O, 63, N, 1.0, 1.3)), dev(_h(O, 64, N, 1.0, 1.3)), dev(_h(O, 65, N, -9.0, 0.0))
    gam, gamb = mesh.to_native(_h(O, 66, F, 1e-3, 2e-3)), dev(_h(O, 67, B, 1e-3, 2e-3))
    phiH, phiHb = mesh.to_native(_h(O, 32, F, -0.15, 0.15)), dev(_h(O, 70, B, -0.1, 0.1))
    f, ref, rg = dev(np.round(_h(O, 80, B) * 2) / 2), dev(_h(O, 84, B)), dev(_h(O, 88, B, -0.5, 0.5))
    rdt, pRef = 1000.0, 1.0e5
    ic, bc = ctx.zeros(B), ctx.zeros(B)
    mesh.call("fvm_boundary_coeffs", None, gamb, -1, f, ref, rg, ic, bc)
    up, lo = ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative)
    dO, sO = ctx.zeros(N), ctx.zeros(N)
    mesh.call("fvm_pressure_eqn", rdt, psi, psi0, p0, rho, rho0, gh, pRef, gam, phiH, phiHb, ic, bc, up, lo, dO, sO)
    d1, u1, l1 = ctx.zeros(N), ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative)
    mesh.call("fvm_transport", rdt, psi, None, None, gam, -1, d1, u1, l1)
    div = ctx.zeros(N)
    mesh.call("fvc_surface_integrate", phiH, phiHb, div)
    V = dev(m.V[s["cOrd"]])
    src = ((rdt * psi0 * p0 * V - V * (rdt * (psi * rho - psi0 * rho0) * gh)) - V * (rdt * (psi - psi0) * pRef)) - V * div
    d2, s2 = ctx.zeros(N), ctx.zeros(N)
    mesh.call("fvm_add_boundary", ic, bc, d1, src, None, d2, s2)
    fn = mesh.from_native
    assert np.array_equal(fn(up), fn(u1)) and np.array_equal(fn(lo), fn(l1))
    assert np.array_equal(dO.cpu().numpy(), d2.cpu().numpy())
    assert np.array_equal(sO.cpu().numpy(), s2.cpu().numpy())
    # the oracle's p_rghEqn
    c = lambda t: _cells_o(s, t)
    bcp = fv.MixedBC(m, f=_patches_o(s, f), ref=_patches_o(s, ref), refGrad=_patches_o(s, rg))
    E = fv.fvm_ddt(m, rdt, c(psi), c(psi0), c(p0))
    E.add_vol(rdt * (c(psi) * c(rho) - c(psi0) * c(rho0)) * c(gh))
    E.add_vol(rdt * (c(psi) - c(psi0)) * pRef)
    E.add_vol(fv.surface_integrate(m, _faces_o(s, phiH), _patches_o(s, phiHb)))
    E -= fv.fvm_laplacian(m, _faces_o(s, gam), _patches_o(s, gamb), [bcp])
    dref, sref = E.solve_system()
    assert np.array_equal(_faces_o(s, up), E.upper) and np.array_equal(_faces_o(s, lo), E.lower)
    assert rel_l2(c(dO), dref) < 1e-15 and rel_l2(c(sO), sref) < 1e-14


def test_pressure_corrector_face_passes_equal_the_operator_chain(setup, O, ctx):
    """ffm_pc_phig, ffm_pc_phiHbyA, ffm_pc_flux and ffm_ue_buoyancy_flux == the two per-operator passes each replaced with their face
    algebra (pc_phig_flux_ops, pc_ddtCorr_ops, pc_flux_U, u_buoyancy), bitwise on the real faces, and oracle/plume.py's expressions"""
    s, mesh, fv, m = setup, setup["mesh"], setup["fv"], setup["m"]
    N, F = s["N"], s["F"]
    dev, fn = ctx.to_device, mesh.from_native
    nat = lambda seed, lo, hi: mesh.to_native(_h(O, seed, F, lo, hi))
    rho, prgh = dev(_h(O, 60, N, 1.0, 1.3)), dev(_h(O, 61, N, -5.0, 5.0))
    rhorAUf, ghf, dcorr = nat(71, 1e-3, 2e-3), nat(72, -9.0, 0.0), nat(73, -0.5, 0.5)
    magSf = _nat(s, m.magSf)
    ro, po = _cells_o(s, rho), _cells_o(s, prgh)
    sg_o, sp_o = m.deltaCoeffs * (ro[m.u] - ro[m.l]), m.deltaCoeffs * (po[m.u] - po[m.l])
    # phig
    phig, sg = ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative)
    mesh.call("pc_phig", rhorAUf, ghf, rho, phig)
    mesh.call("fvc_snGrad", rho, sg)
    assert np.array_equal(fn(phig), fn(-rhorAUf * ghf * sg * magSf))
    assert rel_l2(_faces_o(s, phig), -_faces_o(s, rhorAUf) * _faces_o(s, ghf) * sg_o * m.magSf) < 1e-15
    # the buoyancy flux of UEqn
    t, sgp = ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative)
    mesh.call("ue_buoyancy_flux", ghf, rho, prgh, t)
    mesh.call("fvc_snGrad", prgh, sgp)
    assert np.array_equal(fn(t), fn((-ghf * sg - sgp) * magSf))
    assert rel_l2(_faces_o(s, t), (-_faces_o(s, ghf) * sg_o - sp_o) * m.magSf) < 1e-15
    # phiHbyA
    H = [dev(_h(O, 50 + d, N, -0.5, 0.5)) for d in range(3)]
    phiH, fl = ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative)
    mesh.call("pc_phiHbyA", rho, *H, rhorAUf, dcorr, phig, phiH)
    mesh.call("fvc_flux", *[rho * h for h in H], fl)
    assert np.array_equal(fn(phiH), fn((fl + rhorAUf * dcorr) + phig))
    Ho = [_cells_o(s, h) for h in H]
    flo = sum((m.weights * (ro * Ho[d])[m.l] + (1 - m.weights) * (ro * Ho[d])[m.u]) * m.Sf[:, d] for d in range(3))
    assert rel_l2(_faces_o(s, phiH), flo + _faces_o(s, rhorAUf) * _faces_o(s, dcorr) + _faces_o(s, phig)) < 1e-14
    # p_rghEqn.flux(), phi and the argument of fvc::reconstruct; upper != lower, so the pair's roles show
    up, lo = nat(41, -1.0, -0.2), nat(42, -2.0, -1.1)
    B = s["B"]
    zb = ctx.zeros(B)
    f1, phi, tt, f2 = (ctx.zeros(mesh.nNative) for _ in range(4))
    fb = ctx.zeros(B)
    mesh.call("pc_flux", up, lo, prgh, phiH, phig, rhorAUf, f1, phi, tt)
    mesh.call("fvm_flux", up, lo, zb, zb, prgh, f2, fb)
    assert np.array_equal(fn(f1), fn(f2))
    assert np.array_equal(fn(phi), fn(phiH + f2))
    assert np.array_equal(fn(tt), fn(f2 + phig) / fn(rhorAUf))
    flx = _faces_o(s, up) * po[m.u] - _faces_o(s, lo) * po[m.l]
    assert rel_l2(_faces_o(s, f1), flx) < 1e-15
    assert rel_l2(_faces_o(s, tt), (flx + _faces_o(s, phig)) / _faces_o(s, rhorAUf)) < 1e-14


RAY_MESHES = ["hex", "w8", "w16u14", "w32l30", "w32u18"]


@pytest.mark.parametrize("which", RAY_MESHES)
def test_ray_assembly_equals_the_operator_chain(O, ffm, ctx, which):
    """ffm_fvdom_ray_assemble_d (k_ray_assemble<W>) at mesh level == ray_assemble_ops of csrc/ffm_plume_rad.hip: Ji and the upwind weights,
    Jb and the inflow fraction, ffm_fvm_transport, ffm_fvm_boundary_coeffs, the absorption and source terms, ffm_fvm_add_boundary;
    bitwise, for a ray with all-positive direction components and one with mixed signs, with the emission term"""
    import ctypes as C
    from oracle import plume
    m = plume.make_mesh((9, 8, 7), h=0.1) if which == "hex" else MM.case(which)
    s = MM.device_mesh(ffm, ctx, m)
    assert _bucket(s) == BUCKET[which]
    m, mesh, N, F, B = s["m"], s["mesh"], s["N"], s["F"], s["B"]
    dev, fn = ctx.to_device, mesh.from_native
    T, E, refb = dev(_h(O, 21, N, 300.0, 1500.0)), dev(_h(O, 22, N, 0.0, 5e4)), dev(_h(O, 23, B, 100.0, 200.0))
    V = dev(m.V[s["cOrd"]])
    omega, KA, SIG = 0.39, 0.08, 5.670374e-8
    Sf, bSf = m.Sf[s["fOrd"]], np.concatenate([p.Sf for p in m.patches])
    for d in ([0.31, 0.18, 0.12], [0.31, -0.18, 0.12]):
        dA = np.ascontiguousarray(d, np.float64)
        J, w, up, lo = (ctx.zeros(mesh.nNative) for _ in range(4))
        dg, sr = ctx.zeros(N), ctx.zeros(N)
        mesh.call("fvdom_ray_assemble_d", dA.ctypes.data_as(C.POINTER(C.c_double)), omega, KA, SIG, T, E, refb, J, w, up, lo, dg, sr)
        j = (d[0] * Sf[:, 0] + d[1] * Sf[:, 1]) + d[2] * Sf[:, 2]
        jb = (d[0] * bSf[:, 0] + d[1] * bSf[:, 1]) + d[2] * bSf[:, 2]
        assert (j > 0).any() and (jb > 0).any() and (jb < 0).any() and ((j < 0).any() or min(d) > 0)
        Jn, wn = mesh.to_native(j), mesh.to_native((j >= 0).astype(float))
        assert np.array_equal(fn(J), j) and np.array_equal(fn(w), (j >= 0).astype(float))
        d1, u1, l1 = ctx.zeros(N), ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative)
        mesh.call("fvm_transport", 0.0, None, Jn, wn, None, -1, d1, u1, l1)
        ic, bc = ctx.zeros(B), ctx.zeros(B)
        mesh.call("fvm_boundary_coeffs", dev(jb), None, -1, dev(1.0 - (jb >= 0).astype(float)), refb, ctx.zeros(B), ic, bc)
        kO, cS, kS = KA * omega, 1.0 / np.pi * omega, KA * SIG
        d1 = d1 + V * kO
        su = V * (cS * (kS * ((T * T) * (T * T)) + E / 4.0))
        d2, s2 = ctx.zeros(N), ctx.zeros(N)
        mesh.call("fvm_add_boundary", ic, bc, d1, su, None, d2, s2)
        assert np.array_equal(fn(up), fn(u1)) and np.array_equal(fn(lo), fn(l1)), d
        assert np.array_equal(dg.cpu().numpy(), d2.cpu().numpy()), d
        assert np.array_equal(sr.cpu().numpy(), s2.cpu().numpy()), d
        assert np.isfinite(d2.cpu().numpy()).all() and np.isfinite(s2.cpu().numpy()).all() and np.abs(fn(l1)).max() > 0
    mesh.close(); s["A"].close()


FIELDS = ["rho", "p", "p_rgh", "T", "h", "Ux", "Uy", "Uz", "O2", "H2O", "C3H8", "CO2", "N2", "K"]


@pytest.mark.parametrize("n", [(12, 16, 12), (40, 36, 33)])
def test_time_step_fused_equals_per_operator(ffm, ctx, n):
    """the compiled time step on the fused passes == the same step on one kernel per operator: every field and every
    iteration count identical after three steps (the second size has several tiles and levels wider than one entry)"""
    fused = ffm.Plume(ctx, n)
    os.environ["FFM_PLUME_UNFUSED"] = "1"
    try:
        plain = ffm.Plume(ctx, n)
    finally:
        os.environ.pop("FFM_PLUME_UNFUSED", None)
    for step in range(3):
        fused.step(); plain.step()
        assert [(a, p["nIterations"]) for a, p in fused.solves()] == [(a, p["nIterations"]) for a, p in plain.solves()]
        for name in FIELDS:
            assert np.array_equal(fused.field(name), plain.field(name)), (step, name)
    fused.close(); plain.close()


@pytest.mark.parametrize("n,nf", [((40, 36, 33), 6), ((24, 40, 20), 3), ((50, 34, 34), 6)])
def test_tiled_multivariate_weights_equal_the_two_pass_form(O, ffm, ctx, n, nf):
    """ffm_fv_multivariate_weights_tiled (k_mv_tile: gradients + common limiter in one pass, cell values staged through LDS on the tile
    numbering) == ffm_fvc_grad_multi + ffm_fv_multivariate_weights, bit for bit, on the tile-numbered mesh of the plume case with hashed
    fields (values outside [0, 1], a field that is constant over most of the mesh, fluxes of both signs and exact zeros)."""
    case = ffm.Plume(ctx, n)
    mesh = case.mesh()
    N, B, nNat = case.nCells, mesh.nBoundary, mesh.nNative
    dev = ctx.to_device
    vf = [dev(1.1 * (0.2 + O.hash_u(31 + 7 * i, np.arange(N))) - 0.2) for i in range(nf)]
    a = 0.2 + O.hash_u(31, np.arange(N)); vf[0] = dev(np.where(a > 0.9, a, 0.25))
    vb = [dev(0.1 + O.hash_u(133 + i, np.arange(B))) for i in range(nf)]
    ph = 0.3 * (O.hash_u(32, np.arange(nNat)) - 0.5); ph[::7] = 0.0
    phi = dev(ph)
    sch = (C_int * nf)(*([2] + [3] * (nf - 1)))
    g = [[ctx.zeros(N) for _ in range(3)] for _ in range(nf)]
    mesh.call("fvc_grad_multi", nf if nf <= 4 else 4, vf[:4], vb[:4], [x[0] for x in g[:4]], [x[1] for x in g[:4]], [x[2] for x in g[:4]])
    if nf > 4:
        mesh.call("fvc_grad_multi", nf - 4, vf[4:], vb[4:], [x[0] for x in g[4:]], [x[1] for x in g[4:]], [x[2] for x in g[4:]])
    two = ctx.zeros(nNat) + 7.0
    mesh.call("fv_multivariate_weights", nf, sch, 1.0, 0.0, 1.0, phi, vf, [x[0] for x in g], [x[1] for x in g], [x[2] for x in g], two)
    one = ctx.zeros(nNat) + 7.0
    mesh.call("fv_multivariate_weights_tiled", nf, sch, 1.0, 0.0, 1.0, phi, vf, vb, one)
    a, b = one.cpu().numpy(), two.cpu().numpy()
    assert np.array_equal(a, b), (np.abs(a - b).max(), int((a != b).sum()))
    real = b[b != 7.0]                                                                  # (padding entries of the native layout keep the fill value)
    assert ((real > 1e-6) & (real < 1 - 1e-6) & (np.abs(real - 0.5) > 1e-6)).any() and (real == 1.0).any() and (real == 0.0).any()
    case.close()


class TestMergedMeshes:
    """every test above that takes `setup` once more per merged mesh (tests/merged_mesh.py): the same functions and bars on the
    W = 4, 8, 16 and 32 instantiations, one wide row among narrow ones"""

    @pytest.fixture(scope="class", params=MESHES[1:])
    def setup(self, request, O, ffm, ctx):
        yield from _setup(request.param, ffm, ctx)

    test_grad_multi_equals_grad = staticmethod(test_grad_multi_equals_grad)
    test_scalar_transport_multi_equals_the_operator_chain = staticmethod(test_scalar_transport_multi_equals_the_operator_chain)
    test_multivariate_weights_equal_the_running_minimum_chain = staticmethod(test_multivariate_weights_equal_the_running_minimum_chain)
    test_scalar_transport_multi_with_given_weights_equals_the_operator_chain = staticmethod(
        test_scalar_transport_multi_with_given_weights_equals_the_operator_chain)
    test_lust_source3_equals_the_operator_chain = staticmethod(test_lust_source3_equals_the_operator_chain)
    test_div_phiK_terms_equal_the_operator_chain = staticmethod(test_div_phiK_terms_equal_the_operator_chain)
    test_rho_eqn_equals_surface_integrate_and_the_cell_expression = staticmethod(test_rho_eqn_equals_surface_integrate_and_the_cell_expression)
    test_flux_rho_and_ddt_corr_equal_the_operator_chain = staticmethod(test_flux_rho_and_ddt_corr_equal_the_operator_chain)
    test_HbyA3_equals_three_H_passes = staticmethod(test_HbyA3_equals_three_H_passes)
    test_pressure_eqn_equals_the_operator_chain = staticmethod(test_pressure_eqn_equals_the_operator_chain)
    test_pressure_corrector_face_passes_equal_the_operator_chain = staticmethod(test_pressure_corrector_face_passes_equal_the_operator_chain)

    def test_tiled_multivariate_weights_are_refused(self, setup, O, ffm, ctx):
        """ffm_fv_multivariate_weights_tiled refuses every mesh with rows wider than a hex cell's and writes nothing: the plume
        driver's fall-back (mv_weights_grad_multi) relies on the return code"""
        s, mesh = setup, setup["mesh"]
        assert _bucket(s) > 3
        nf = 3
        vf, vb, phi = _fields(s, O, ctx, nf)
        out = ctx.zeros(mesh.nNative) + SENTINEL
        with pytest.raises(ffm.FfmError, match=UNSUPPORTED):
            mesh.call("fv_multivariate_weights_tiled", nf, (C_int * nf)(2, 3, 3), 1.0, 0.0, 1.0, phi, vf, vb, out)
        assert _untouched([out])
