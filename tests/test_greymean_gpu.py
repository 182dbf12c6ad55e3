"""The kernels of greyMeanAbsorptionEmission (csrc/ffm_greymean.hip) and the field forms of its two consumers (csrc/ffm_rad.hip) on the
device.  Every comparison is BITWISE: only + - * / occur, correctly rounded on both sides in a stated order, contraction off.

  (a) ffm_greymean_a_d == tests/greymean_ref.py on the designed inputs (tests/test_greymean_cpu.py shows which edges they reach), 5 species,
      n = 1 and n = 1027 (a partial last wave, several workgroups); nPart 1, 3 (the fixture's order and its reverse) and 5 = nSpecies; the
      flag raised exactly when a T leaves a participating species' [Tlow, Thigh] and untouched otherwise; ffm_greymean_E_d; the guards
      around the outputs intact; argument errors and refused tables leave NaN-prefilled outputs alone.
  (b) uniform a: ffm_fvdom_ray_assemble_v_d == ffm_fvdom_ray_assemble_d and ffm_radiation_sh_v_d == ffm_radiation_sh_d, on the five meshes
      of tests/test_p1_gpu.py (every row-width bucket) and for the five rays of tests/ray_matrix.py:five_directions().
  (c) non-uniform a: ffm_fvdom_ray_assemble_v_d == the operator chain (ffm_fvm_transport, ffm_fvm_boundary_coeffs, diag += V*(a*omega),
      source = V*(cS*((a*sigma)*T^4 [+ E/4])), ffm_fvm_add_boundary) on the same meshes, with and without E.
  (d) ffm_radiation_sh_greymean_d == ffm_greymean_a_d, ffm_greymean_E_d, ffm_radiation_sh_v_d: su, sp, a_out and the flag, with a Cp field
      and with the constant, with and without a_out, at n = 1027."""
import ctypes as C

import numpy as np
import pytest

import greymean_ref as GM
import merged_mesh as MM
import ray_matrix as R
from test_thermo_edges_gpu import GUARD, _P, _guarded, _guards_intact

pytestmark = pytest.mark.gpu

MESHES = ["hex", "w8", "w16u14", "w32l30", "w32u18"]
BUCKET = {"hex": 3, "w8": 8, "w16u14": 16, "w32l30": 32, "w32u18": 32}
SIGMA = 5.670367e-8
ERR_ARG = -1
FILL = -12345.0
ORDERS = [["CH4"], ["CO2", "H2O", "CH4"], ["CH4", "H2O", "CO2"], ["CO2", "H2O", "CH4", "O2", "N2"]]


def _coeffs():
    co = GM.edge_coeffs()
    # O2 and N2 do not absorb in the infrared; here they carry small polynomials so that nPart == nSpecies has five live terms
    co["O2"] = dict(Tcommon=500.0, invTemp=False, Tlow=200.0, Thigh=2500.0, loTcoeffs=[0.02, 1e-5, 0, 0, 0, 0], hiTcoeffs=[0.03, -2e-6, 1e-9, 0, 0, 0])
    co["N2"] = dict(Tcommon=400.0, invTemp=True, Tlow=200.0, Thigh=2500.0, loTcoeffs=[0.01, 2.0, 0, 0, 0, 0], hiTcoeffs=[0.015, -1.5, 30.0, 0, 0, 0])
    return co


def _model(ffm, ctx, order, Ehrr=0.27):
    return ffm.GreyMean(ctx, GM.SPECIES5, GM.W, _coeffs(), Ehrr, order=order)


def _flag(ctx, v=0):
    return ctx.torch.full((1,), v, dtype=ctx.torch.int32, device=ctx.device)


def _inner(buf, n):
    return buf.cpu().numpy()[GUARD:GUARD + n]


@pytest.mark.parametrize("n", [1, 1027])
@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "-".join(o))
def test_a_against_the_restatement_bitwise(ffm, ctx, n, order):
    L = ffm.lib()
    gm = _model(ffm, ctx, order)
    co = _coeffs()
    for in_range in (False, True):
        Y, p, T, _ = GM.edge_inputs(n, seed=5 + n, in_range=in_range)
        want = GM.aCont(GM.SPECIES5, GM.W, co, order, Y, p, T)
        Yd, pd, Td = [ctx.to_device(y) for y in Y], ctx.to_device(p), ctx.to_device(T)
        Yp = (C.c_void_p * 5)(*[y.data_ptr() for y in Yd])
        for start in (0, 7):                                            # the flag is only ever raised: a value it holds stays
            buf, ap = _guarded(ctx, n, FILL)
            flag = _flag(ctx, start)
            ctx._ready()
            assert L.ffm_greymean_a_d(gm.h, n, Yp, _P(pd), _P(Td), ap, _P(flag)) == 0
            ctx.sync()
            assert _guards_intact(buf, n, FILL)
            got = _inner(buf, n)
            assert np.isfinite(got).all() and got.tobytes() == want.tobytes(), (n, order, np.abs(got - want).max())
            raised = GM.outside(co, order, T)
            assert int(flag.cpu()[0]) == (1 if raised else start), (n, order, in_range, start)
        if n > 1:
            assert GM.outside(co, order, T) == (not in_range)
        buf, ap = _guarded(ctx, n, FILL)                                # no flag asked for
        ctx._ready()
        assert L.ffm_greymean_a_d(gm.h, n, Yp, _P(pd), _P(Td), ap, None) == 0
        ctx.sync()
        assert _inner(buf, n).tobytes() == want.tobytes() and _guards_intact(buf, n, FILL)
    # E = EhrrCoeff*Qdot
    Q = np.random.RandomState(n).uniform(0.0, 5e6, n); Q[::3] = 0.0
    buf, ep = _guarded(ctx, n, FILL)
    Qd = ctx.to_device(Q)
    ctx._ready()
    assert L.ffm_greymean_E_d(gm.h, n, _P(Qd), ep) == 0
    ctx.sync()
    assert _inner(buf, n).tobytes() == (0.27 * Q).tobytes() and _guards_intact(buf, n, FILL)
    gm.close()


def test_argument_errors_and_refused_tables_write_nothing(ffm, ctx):
    L = ffm.lib()
    gm = _model(ffm, ctx, ORDERS[1])
    n = 65
    Y, p, T, _ = GM.edge_inputs(n)
    Yd, pd, Td = [ctx.to_device(y) for y in Y], ctx.to_device(p), ctx.to_device(T)
    Yp = (C.c_void_p * 5)(*[y.data_ptr() for y in Yd])
    Ynull = (C.c_void_p * 5)(*[None if i == 2 else y.data_ptr() for i, y in enumerate(Yd)])
    outs = [ctx.to_device(np.full(n, np.nan)) for _ in range(4)]
    a, E, su, sp = [_P(o) for o in outs]
    flag = _flag(ctx)
    ctx._ready()
    ok = (gm.h, n, Yp, _P(pd), _P(Td), a, _P(flag))
    assert L.ffm_greymean_a_d(gm.h, 0, *ok[2:]) == 0                                    # n == 0: a no-op
    for k in (0, 2, 3, 4, 5):
        assert L.ffm_greymean_a_d(*[None if j == k else v for j, v in enumerate(ok)]) == ERR_ARG, k
    assert L.ffm_greymean_a_d(gm.h, -1, *ok[2:]) == ERR_ARG
    assert L.ffm_greymean_a_d(gm.h, n, Ynull, *ok[3:]) == ERR_ARG                       # a NULL species pointer
    assert L.ffm_greymean_E_d(gm.h, 0, _P(pd), E) == 0
    assert L.ffm_greymean_E_d(None, n, _P(pd), E) == ERR_ARG and L.ffm_greymean_E_d(gm.h, n, None, E) == ERR_ARG
    assert L.ffm_greymean_E_d(gm.h, n, _P(pd), None) == ERR_ARG and L.ffm_greymean_E_d(gm.h, -1, _P(pd), E) == ERR_ARG
    x = _P(pd)
    shv = (ctx.h, n, x, x, SIGMA, x, x, _P(Td), x, None, 1005.0, su, sp)
    assert L.ffm_radiation_sh_v_d(ctx.h, 0, *shv[2:]) == 0
    for k in (0, 2, 3, 5, 6, 7, 8, 11, 12):
        assert L.ffm_radiation_sh_v_d(*[None if j == k else v for j, v in enumerate(shv)]) == ERR_ARG, k
    assert L.ffm_radiation_sh_v_d(ctx.h, -1, *shv[2:]) == ERR_ARG
    shg = (gm.h, n, Yp, x, _P(Td), SIGMA, x, x, x, None, 1005.0, a, su, sp, _P(flag))
    assert L.ffm_radiation_sh_greymean_d(gm.h, 0, *shg[2:]) == 0
    for k in (0, 2, 3, 4, 6, 7, 8, 12, 13):
        assert L.ffm_radiation_sh_greymean_d(*[None if j == k else v for j, v in enumerate(shg)]) == ERR_ARG, k
    assert L.ffm_radiation_sh_greymean_d(gm.h, -1, *shg[2:]) == ERR_ARG
    assert L.ffm_radiation_sh_greymean_d(gm.h, n, Ynull, *shg[3:]) == ERR_ARG
    ctx.sync()
    for o in outs:
        assert np.isnan(o.cpu().numpy()).all()
    assert int(flag.cpu()[0]) == 0
    gm.close()
    # tables the library refuses: nothing is created
    hp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    W = np.array([16.0, 32.0, 28.0, 18.0, 44.0, 2.0, 4.0, 40.0, 30.0])
    one = np.ones(9); six = np.ones(54)
    H = lambda v: v.ctypes.data_as(hp)

    def create(nSpecies=5, nPart=3, specie=(0, 3, 4), Wv=W):
        sp_ = np.array(specie + (0,) * 9, np.int32)[:9]
        inv = np.zeros(9, np.int32)
        h = C.c_void_p()
        rc = L.ffm_greymean_create(ctx.h, nSpecies, H(Wv), nPart, sp_.ctypes.data_as(ip), inv.ctypes.data_as(ip), H(one), H(one), H(one), H(six), H(six), 0.0, C.byref(h))
        return rc, h
    for kw in (dict(nSpecies=9), dict(nSpecies=0), dict(nPart=0), dict(nPart=9, nSpecies=8, specie=tuple(range(8)) + (0,)), dict(specie=(0, 5, 4)),
               dict(specie=(0, -1, 4)), dict(specie=(0, 3, 3)), dict(Wv=np.where(np.arange(9) == 1, 0.0, W))):
        rc, h = create(**kw)
        assert rc == ERR_ARG and not h.value, kw
    rc, h = create(nSpecies=8, nPart=8, specie=tuple(range(8)))             # the limits themselves are accepted
    assert rc == 0 and h.value
    L.ffm_greymean_destroy(h)


def _device(ffm, ctx, which):
    from oracle import plume
    m = plume.make_mesh((9, 8, 7), h=0.1) if which == "hex" else MM.case(which)
    s = MM.device_mesh(ffm, ctx, m)
    assert MM.bucket(max(np.bincount(s["l"]).max(), np.bincount(s["u"]).max())) == BUCKET[which]
    return s


def _h(O, seed, n, lo, hi):
    return lo + (hi - lo) * O.hash_u(seed, np.arange(n))


def _assemble(ctx, mesh, N, name, dA, omega, a, T, E, refb):
    J, w, up, lo = (ctx.zeros(mesh.nNative) for _ in range(4))
    dg, sr = ctx.zeros(N), ctx.zeros(N)
    mesh.call(name, dA.ctypes.data_as(C.POINTER(C.c_double)), omega, a, SIGMA, T, E, refb, J, w, up, lo, dg, sr)
    fn = mesh.from_native
    return dict(J=fn(J), w=fn(w), upper=fn(up), lower=fn(lo), diag=dg.cpu().numpy(), source=sr.cpu().numpy())


@pytest.mark.parametrize("which", MESHES)
def test_ray_assembly_field_form(O, ffm, ctx, which):
    s = _device(ffm, ctx, which)
    m, mesh, N, B = s["m"], s["mesh"], s["N"], s["B"]
    dev = ctx.to_device
    Tn, En, an = _h(O, 21, N, 300.0, 1500.0), _h(O, 22, N, 0.0, 5e4), _h(O, 24, N, 0.0, 3.0)
    an[::9] = 0.0                                                          # transparent cells
    T, E, refb = dev(Tn), dev(En), dev(_h(O, 23, B, 100.0, 200.0))
    V = m.V[s["cOrd"]]
    Sf, bSf = m.Sf[s["fOrd"]], np.concatenate([p.Sf for p in m.patches])
    octants = set()
    for name, d, omega in R.five_directions():
        dA = np.ascontiguousarray(d, np.float64)
        octants.add(R.octant(dA))
        # (b) uniform a == the scalar form
        x = 0.08
        for Ef in (E, None):
            want = _assemble(ctx, mesh, N, "fvdom_ray_assemble_d", dA, omega, x, T, Ef, refb)
            got = _assemble(ctx, mesh, N, "fvdom_ray_assemble_v_d", dA, omega, dev(np.full(N, x)), T, Ef, refb)
            for k in want:
                assert np.isfinite(got[k]).all() and np.array_equal(got[k], want[k]), (which, name, k, Ef is None)
        # (c) non-uniform a == the operator chain
        j = (dA[0] * Sf[:, 0] + dA[1] * Sf[:, 1]) + dA[2] * Sf[:, 2]
        jb = (dA[0] * bSf[:, 0] + dA[1] * bSf[:, 1]) + dA[2] * bSf[:, 2]
        d1, u1, l1 = ctx.zeros(N), ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative)
        mesh.call("fvm_transport", 0.0, None, mesh.to_native(j), mesh.to_native((j >= 0).astype(float)), None, -1, d1, u1, l1)
        ic, bc = ctx.zeros(B), ctx.zeros(B)
        mesh.call("fvm_boundary_coeffs", dev(jb), None, -1, dev(1.0 - (jb >= 0).astype(float)), refb, ctx.zeros(B), ic, bc)
        cS = 1.0 / np.pi * omega
        T4 = (Tn * Tn) * (Tn * Tn)
        dn = d1.cpu().numpy() + V * (an * omega)
        for Ef, su in ((E, V * (cS * ((an * SIGMA) * T4 + En / 4.0))), (None, V * (cS * ((an * SIGMA) * T4)))):
            d2, s2 = ctx.zeros(N), ctx.zeros(N)
            mesh.call("fvm_add_boundary", ic, bc, dev(dn), dev(su), None, d2, s2)
            got = _assemble(ctx, mesh, N, "fvdom_ray_assemble_v_d", dA, omega, dev(an), T, Ef, refb)
            assert np.array_equal(got["upper"], mesh.from_native(u1)) and np.array_equal(got["lower"], mesh.from_native(l1)), (which, name)
            assert np.array_equal(got["diag"], d2.cpu().numpy()), (which, name, Ef is None)
            assert np.array_equal(got["source"], s2.cpu().numpy()), (which, name, Ef is None)
            assert np.array_equal(got["J"], j)
    assert len(octants) >= 4
    # refused arguments
    L = ffm.lib()
    dp = dA.ctypes.data_as(C.POINTER(C.c_double))
    z = [ctx.to_device(np.full(k, np.nan)) for k in (mesh.nNative, mesh.nNative, N, N)]
    ctx._ready()
    ok = [mesh.h, dp, 0.3, _P(dev(an)), SIGMA, _P(T), None, _P(refb), None, None] + [_P(t) for t in z]
    for k in (0, 1, 3, 5, 7, 10, 11, 12, 13):
        assert L.ffm_fvdom_ray_assemble_v_d(*[None if jx == k else v for jx, v in enumerate(ok)]) == ERR_ARG, k
    ctx.sync()
    assert all(np.isnan(t.cpu().numpy()).all() for t in z)
    mesh.close(); s["A"].close()


@pytest.mark.parametrize("which", MESHES)
def test_radiation_sh_field_form_with_uniform_fields(O, ffm, ctx, which):
    """uniform a = e = x and E = frac*Qdot give the scalar form's bits, on the cell counts of the five meshes; a_d and e_d the same array"""
    s = _device(ffm, ctx, which)
    N = s["N"]
    L = ffm.lib()
    G, T, he, Q, Cp = _h(O, 31, N, 0.0, 4e5), _h(O, 32, N, 250.0, 2500.0), _h(O, 33, N, -6e4, 3.5e6), _h(O, 34, N, 0.0, 5e6), _h(O, 35, N, 900.0, 2500.0)
    G[::3] = 0.0; Q[1::4] = 0.0
    dev = [ctx.to_device(v) for v in (G, T, he, Q, Cp)]
    for x, frac, field in ((0.1, 0.36, True), (0.1, 0.36, False), (0.0, 0.22, False), (0.08, 0.0, True)):
        (b0, su0), (b1, sp0), (b2, su1), (b3, sp1) = (_guarded(ctx, N, FILL) for _ in range(4))
        ad, Ed = ctx.to_device(np.full(N, x)), ctx.to_device(frac * Q)
        cp = _P(dev[4]) if field else None
        ctx._ready()
        assert L.ffm_radiation_sh_d(ctx.h, N, x, SIGMA, frac, *[_P(d) for d in dev[:4]], cp, 1005.0, su0, sp0) == 0
        assert L.ffm_radiation_sh_v_d(ctx.h, N, _P(ad), _P(ad), SIGMA, _P(Ed), _P(dev[0]), _P(dev[1]), _P(dev[2]), cp, 1005.0, su1, sp1) == 0
        ctx.sync()
        assert all(_guards_intact(b, N, FILL) for b in (b0, b1, b2, b3))
        assert _inner(b2, N).tobytes() == _inner(b0, N).tobytes() and _inner(b3, N).tobytes() == _inner(b1, N).tobytes(), (which, x, frac, field)
        su, sp = GM.radiation_sh(np.full(N, x), np.full(N, x), SIGMA, frac * Q, G, T, he, Cp if field else 1005.0)
        assert _inner(b2, N).tobytes() == su.tobytes() and _inner(b3, N).tobytes() == sp.tobytes()
    s["mesh"].close(); s["A"].close()


@pytest.mark.parametrize("order", [ORDERS[1], ORDERS[3]], ids=lambda o: "-".join(o))
def test_fused_source_pass_equals_the_three_call_chain(ffm, ctx, order):
    L = ffm.lib()
    n = 1027
    gm = _model(ffm, ctx, order)
    r = np.random.RandomState(3)
    G, he, Q, Cp = r.uniform(0.0, 4e5, n), r.uniform(-6e4, 3.5e6, n), r.uniform(0.0, 5e6, n), r.uniform(900.0, 2500.0, n)
    G[::3] = 0.0; Q[1::4] = 0.0
    Gd, hd, Qd, Cd = (ctx.to_device(v) for v in (G, he, Q, Cp))
    for in_range in (True, False):
        Y, p, T, _ = GM.edge_inputs(n, in_range=in_range)
        Yd, pd, Td = [ctx.to_device(y) for y in Y], ctx.to_device(p), ctx.to_device(T)
        Yp = (C.c_void_p * 5)(*[y.data_ptr() for y in Yd])
        # the chain
        a, E = ctx.zeros(n), ctx.zeros(n)
        f0 = _flag(ctx)
        ctx._ready()
        assert L.ffm_greymean_a_d(gm.h, n, Yp, _P(pd), _P(Td), _P(a), _P(f0)) == 0
        assert L.ffm_greymean_E_d(gm.h, n, _P(Qd), _P(E)) == 0
        for field in (True, False):
            cp = _P(Cd) if field else None
            su0, sp0 = ctx.zeros(n), ctx.zeros(n)
            assert L.ffm_radiation_sh_v_d(ctx.h, n, _P(a), _P(a), SIGMA, _P(E), _P(Gd), _P(Td), _P(hd), cp, 1005.0, _P(su0), _P(sp0)) == 0
            for with_a in (True, False):
                (ba, ap), (bu, sup), (bp, spp) = (_guarded(ctx, n, FILL) for _ in range(3))
                f1 = _flag(ctx)
                assert L.ffm_radiation_sh_greymean_d(gm.h, n, Yp, _P(pd), _P(Td), SIGMA, _P(Gd), _P(hd), _P(Qd), cp, 1005.0, ap if with_a else None,
                                                     sup, spp, _P(f1)) == 0
                ctx.sync()
                assert all(_guards_intact(b, n, FILL) for b in (ba, bu, bp))
                assert _inner(bu, n).tobytes() == su0.cpu().numpy().tobytes(), (order, in_range, field, with_a, "su")
                assert _inner(bp, n).tobytes() == sp0.cpu().numpy().tobytes(), (order, in_range, field, with_a, "sp")
                assert (_inner(ba, n).tobytes() == a.cpu().numpy().tobytes()) if with_a else np.all(ba.cpu().numpy() == FILL)
                assert int(f1.cpu()[0]) == int(f0.cpu()[0]) == (0 if in_range else 1)
        # and the chain itself is the restatement
        an = GM.aCont(GM.SPECIES5, GM.W, _coeffs(), order, Y, p, T)
        su, sp = GM.radiation_sh(an, an, SIGMA, 0.27 * Q, G, T, he, 1005.0)
        assert su0.cpu().numpy().tobytes() == su.tobytes() and sp0.cpu().numpy().tobytes() == sp.tobytes()
        assert np.isfinite(su).all() and np.abs(sp).max() > 0
    gm.close()
