"""The class layer's greyMeanAbsorptionEmission (include/fireFoamHandles.H) and the absorption / emission hooks of fvDOM and P1, driven
through b1_greymean of examples/b1_demo.C on the (7, 8, 6) box: a five-species mixture with hot CO2 / H2O around a flame-like hot spot, the
model built from a dictionary file written here from tests/golden/greymean_case_data.json (with a comment inside the coefficient lists, as
the case file has them, `lookUpTableFileName none` and EhrrCoeff 0.3 so that the emission term is live).

  (a) aCont(): the cells bitwise the restatement (tests/greymean_ref.py), the patch values the adjacent cells'; ECont() = EhrrCoeff*Qdot;
      any lookUpTableFileName other than none is refused with a message naming it (the fixture's own "SpeciesTable" included).
  (b) fvDOM with the hooks set and ordered (exact) ray solves against oracle/fvdom.py fed with the restatement's field and the same exact
      solve: every Ii, G, and the diagonal and source of Sh(thermo, he) within the project's 1e-8.
  (c) P1 with the hooks set against tests/p1_ref.py fed with the same field and its patch values: the same PCG iteration counts, G, G_b, qr
      within 1e-8, and Sh.
  (d) hooks unset, bit for bit against the scalar ABI called from here: fvDOM's every ray, G and summed wall fluxes equal the chain of
      scalar entry points (wall coefficients, upwind weights, transport, boundary coefficients, ordered solve, patch evaluation) with the
      class layer's rounding of the cell terms; P1's G, G_b, qr and iteration counts equal those of b1_p1 (the driver that never touches
      the hooks) and its system equals ffm_p1_assemble_d's; Sh's diagonal equals -(V*sp) of ffm_radiation_sh_d and its source the ABI's
      two pieces rounded as the class layer's two fvm::Su terms round them.  And the providers set to the uniform constants give the same
      bits once more (the field statements with a uniform field are the constant's statements).
Unpinned by reference data: the reference ships no output of a run with this model."""
import ctypes as C
import os

import numpy as np
import pytest

import foam_case
import greymean_ref as GM
import merged_mesh as MM
import p1_ref as P1
import ray_matrix as R
from common import rel_l2

pytestmark = pytest.mark.gpu

SPECIES = GM.SPECIES5
EHRR = 0.3
SIGMA = 5.670367e-8
dp = C.POINTER(C.c_double)


def _dict_text(table="none"):
    fx = GM.fixture()
    out = ["FoamFile { version 2.0; format ascii; class dictionary; object radiationProperties; }", "absorptionEmissionModel greyMeanAbsorptionEmission;",
           "greyMeanAbsorptionEmissionCoeffs", "{", "    lookUpTableFileName     %s;" % table, "    EhrrCoeff                %r;" % EHRR]
    for s in fx["species"]:
        c = fx["coeffs"][s]
        out += ["    %s" % s, "    {", "        Tcommon %r; //Common Temp" % c["Tcommon"], "        invTemp %s;" % ("true" if c["invTemp"] else "false"),
                "        Tlow %r;" % c["Tlow"], "        Thigh %r;" % c["Thigh"], "        loTcoeffs //coefss for T < Tcommon", "        ("]
        out += ["            %r // a%d*T^(+/-)%d +" % (v, k, k) for k, v in enumerate(c["loTcoeffs"])]
        out += ["        );", "        hiTcoeffs", "        ("] + ["            %r /* a%d */" % (v, k) for k, v in enumerate(c["hiTcoeffs"])] + ["        );", "    }"]
    return "\n".join(out + ["}", ""])


@pytest.fixture(scope="module")
def case(O, ffm, ctx, tmp_path_factory):
    from oracle import plume
    s = MM.device_mesh(ffm, ctx, plume.make_mesh((7, 8, 6)))
    m, N = s["m"], s["N"]
    T, Tb, Q, emis = foam_case.fvdom_inputs(m)
    T = T + 900.0 * (T - 500.0) / 600.0                                  # 500 K to 2000 K in the hot spot
    burnt = (T - 500.0) / 1500.0
    Y = np.array([0.02 * (1.0 - burnt), 0.23 * (1.0 - burnt) + 0.01, 0.72 - 0.05 * burnt, 0.01 + 0.09 * burnt, 0.01 + 0.15 * burnt])
    Y = [np.ascontiguousarray(y) for y in Y / Y.sum(axis=0)]
    p = 101325.0 + 40.0 * (m.C[:, 1] - m.C[:, 1].mean())
    he = 1005.0 * (T - 298.15)
    Cp = 1005.0 + 0.2 * (T - 298.15)
    fx = GM.fixture()
    a = GM.aCont(SPECIES, GM.W, fx["coeffs"], fx["species"], Y, p, T)
    path = tmp_path_factory.mktemp("greymean") / "radiationProperties"
    path.write_text(_dict_text())
    s.update(T=T, Tb=Tb, Q=Q, emis=emis, Y=Y, p=p, he=he, Cp=Cp, a=a, path=str(path),
             lib=C.CDLL(os.path.join(os.path.dirname(ffm.libpath()), "libffm_b1demo.so")))
    yield s
    s["mesh"].close(); s["A"].close()


def _run(ctx, s, model, hooks, aConst=0.3, eConst=0.3, nPhi=2, nTheta=2, nCalls=2, tol=1e-6, path=None, table=b""):
    lib, cOrd, N, B, mesh = s["lib"], s["cOrd"], s["N"], s["B"], s["mesh"]
    lib.b1_greymean.restype = C.c_int
    lib.b1_greymean.argtypes = ([C.c_void_p] * 3 + [C.c_char_p] * 3 + [dp, C.POINTER(dp)] + [dp] * 7 + [C.c_int, C.c_int, C.c_double, C.c_double] + [C.c_int] * 3
                                + [C.c_double, dp, dp, C.POINTER(C.c_int)] + [dp] * 4 + [C.POINTER(C.c_int), dp])
    h = lambda v: np.ascontiguousarray(v, np.float64)
    P = lambda v: v.ctypes.data_as(dp)
    Yc = [h(y[cOrd]) for y in s["Y"]]
    Yp = (dp * len(Yc))(*[P(y) for y in Yc])
    W = h([GM.W[k] for k in SPECIES])
    ins = [h(s[k][cOrd]) for k in ("p", "T")] + [h(np.concatenate(s["Tb"]))] + [h(s[k][cOrd]) for k in ("Q", "he", "Cp")] + [h(np.concatenate(s["emis"]))]
    nRay = 4 * nPhi * nTheta
    out = dict(a=np.empty(N + B), E=np.empty(N), I=np.empty((nRay, N)), G=np.empty(N), Gb=np.empty(B), qr=np.empty(B), sh=np.empty(2 * N))
    iters, flag = (C.c_int * nCalls)(), C.c_int(-1)
    os.environ["FFM_FOAM_QUIET"] = "1"
    ctx._ready()
    rc = lib.b1_greymean(ctx.h, s["A"].h, mesh.h, (path or s["path"]).encode(), table, " ".join(SPECIES).encode(), P(W), Yp, *[P(v) for v in ins], model, hooks,
                         aConst, eConst, nPhi, nTheta, nCalls, tol, P(out["a"]), P(out["E"]), C.byref(flag), P(out["I"]), P(out["G"]), P(out["Gb"]),
                         P(out["qr"]), iters, P(out["sh"]))
    out.update(rc=rc, iters=list(iters), flag=flag.value)
    return out


def _cells_o(s, v):
    o = np.empty(s["N"]); o[s["cOrd"]] = v
    return o


def _sh_ref(m, a, e, E, G, T, he, Cp):
    """diag and source of Sh = Su(Ru) - Sp(4 Rp T^3/Cpv) - Su(Rp T^3 (T - 4 he/Cpv)): fvm::Su is source -= V*su, fvm::Sp is diag += V*sp"""
    su, sp = GM.radiation_sh(a, e, SIGMA, E, G, T, he, Cp)
    return -(m.V * sp), -(m.V * su)


def test_aCont_cells_patches_and_the_refused_table(O, ffm, ctx, case, tmp_path):
    s = case
    m, N = s["m"], s["N"]
    got = _run(ctx, s, 0, 1)
    assert got["rc"] == 0 and got["flag"] == 0
    a = _cells_o(s, got["a"][:N])
    assert a.tobytes() == s["a"].tobytes(), np.abs(a - s["a"]).max()
    assert s["a"].min() > 0.5 and np.ptp(s["a"]) > 0.5                  # (the restatement's field: about 0.8 to 1.5 per metre here)
    assert np.array_equal(got["a"][N:], np.concatenate([a[p.faceCells] for p in m.patches]))
    assert _cells_o(s, got["E"]).tobytes() == (EHRR * s["Q"]).tobytes()
    # the look-up table branch is not built: a file that names a table, as the reference's do, is refused (a FatalError ends the process,
    # so the message is asked for, not provoked) and the override makes the same file readable
    bad = tmp_path / "radiationProperties"
    bad.write_text(_dict_text('"SpeciesTable"'))
    lib = s["lib"]
    lib.b1_greymean_table_refusal.restype = C.c_int
    lib.b1_greymean_table_refusal.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    msg = C.create_string_buffer(512)
    assert lib.b1_greymean_table_refusal(str(bad).encode(), b"", msg, 512) > 0 and b"SpeciesTable" in msg.value
    assert lib.b1_greymean_table_refusal(str(bad).encode(), b"none", msg, 512) == 0
    assert lib.b1_greymean_table_refusal(s["path"].encode(), b"", msg, 512) == 0
    got2 = _run(ctx, s, 0, 1, path=str(bad), table=b"none")
    assert np.array_equal(got2["a"], got["a"])


def test_fvDOM_with_the_hooks_against_the_oracle(O, ffm, ctx, case):
    from oracle import fvdom
    s = case
    m, N = s["m"], s["N"]
    ml, mu = np.asarray(m.l, np.int64), np.asarray(m.u, np.int64)

    def solve(name, d, upper, lower, src, psi0):
        lev, _, acyclic = R.kahn_levels(N, *R.edges(ml, mu, upper, lower))
        assert acyclic
        Ao = O.Ldu(N, m.l, m.u).set_coeffs(d, upper, lower)
        nf = Ao.norm_factor(psi0, src)
        psi = R.forward_substitution(N, ml, mu, d, upper, lower, src, np.argsort(lev, kind="stable"))
        return psi, dict(initialResidual=float(np.abs(Ao.residual(psi0, src)).sum() / nf), finalResidual=float(np.abs(Ao.residual(psi, src)).sum() / nf),
                         nIterations=1, converged=1, singular=0)
    ref = fvdom.FvDOM(m, 2, 2, solve, maxIter=1, tolerance=0.0, emissivity=s["emis"])
    E = EHRR * s["Q"]
    for _ in range(2):
        ref.calculate(s["T"], s["Tb"], s["a"], E)
    got = _run(ctx, s, 1, 1)
    assert got["rc"] == len(ref.rays) == 16 and got["iters"] == [1, 1]
    errI = max(rel_l2(_cells_o(s, got["I"][i]), ref.I[i]) for i in range(16))
    errG = rel_l2(_cells_o(s, got["G"]), ref.G)
    dg, sr = _sh_ref(m, s["a"], s["a"], E, ref.G, s["T"], s["he"], s["Cp"])
    errD, errS = rel_l2(_cells_o(s, got["sh"][:N]), dg), rel_l2(_cells_o(s, got["sh"][N:]), sr)
    print("fvDOM + greyMean: I %.3e  G %.3e  Sh diag %.3e  Sh source %.3e" % (errI, errG, errD, errS))
    assert errI < 1e-8 and errG < 1e-8 and errD < 1e-8 and errS < 1e-8
    # the model matters: the constant the case would otherwise use gives another G
    const = _run(ctx, s, 1, 0)
    assert rel_l2(const["G"], got["G"]) > 1e-3


def test_P1_with_the_hooks_against_the_restatement(O, ffm, ctx, case):
    s = case
    m, N = s["m"], s["N"]
    E = EHRR * s["Q"]
    a_b = [s["a"][p.faceCells] for p in m.patches]
    G, its = np.zeros(N), []
    for _ in range(3):
        S = P1.system(m, s["a"], s["a"], E, s["T"], s["Tb"], s["emis"], 0.0, 0.0, a_b=a_b)
        G, perf = P1.solve(O, m, S, G, 1e-6)
        its.append(perf["nIterations"])
    Gb, qr = P1.wall(m, S, G)
    got = _run(ctx, s, 2, 1, nCalls=3)
    print("P1 + greyMean: iterations %s (restatement %s)" % (got["iters"], its))
    assert got["rc"] == 3 and got["iters"] == its and its[0] > 3
    dg, sr = _sh_ref(m, s["a"], s["a"], E, G, s["T"], s["he"], s["Cp"])
    errs = dict(G=rel_l2(_cells_o(s, got["G"]), G), G_b=rel_l2(got["Gb"], np.concatenate(Gb)), qr=rel_l2(got["qr"], np.concatenate(qr)),
                shDiag=rel_l2(_cells_o(s, got["sh"][:N]), dg), shSource=rel_l2(_cells_o(s, got["sh"][N:]), sr))
    print(", ".join("%s %.2e" % kv for kv in errs.items()))
    assert all(v < 1e-8 for v in errs.values()), errs
    assert np.abs(got["qr"]).max() > 0


def _ray_set(nPhi, nTheta):
    """fvDOM::initialise for a 3-D mesh in the operation order of include/fireFoamHandles.H (libm's sin and cos, as there): (d, dAve, omega)"""
    from math import cos, sin
    pi = 3.14159265358979323846
    dPhi, dTheta = pi / (2.0 * nPhi), pi / nTheta
    rays = []
    for n in range(1, nTheta + 1):
        for k in range(1, 4 * nPhi + 1):
            phi, theta = (2.0 * k - 1.0) * dPhi / 2.0, (2.0 * n - 1.0) * dTheta / 2.0
            c = sin(0.5 * dPhi) * (dTheta - cos(2.0 * theta) * sin(dTheta))
            rays.append((np.array([sin(theta) * sin(phi), sin(theta) * cos(phi), cos(theta)]),
                         np.array([sin(phi) * c, cos(phi) * c, 0.5 * dPhi * sin(2.0 * theta) * sin(dTheta)]),
                         2.0 * sin(theta) * sin(dTheta / 2.0) * dPhi))
    return rays


def _fvdom_scalar_abi_chain(ctx, s, a, nPhi, nTheta, nCalls):
    """fvDOM::correct() with a constant a, maxIter 1, ordered ray solves, E = Qdot, through the library's scalar entry points alone:
    ffm_fvdom_wall_coeffs_d | ffm_fv_limited_weights (upwind) | ffm_fvm_transport | ffm_fvm_boundary_coeffs | diag + V*(a*omega), source
    0 + V*((1/pi*omega)*(a*(sigma*T^4) + E/4)) on the host in IEEE double | ffm_fvm_add_boundary | ffm_solve_ordered_d | ffm_bc_values, ray
    after ray, then G = ((0 + I_0 w_0) + I_1 w_1) + ...  The rounding is the class layer's statement `k*sigmaT4` (the one-pass
    ffm_fvdom_ray_assemble_d associates (a*sigma)*T^4, as the plume's operator chain does, so it is no bitwise yardstick for the class)."""
    m, mesh, A, N, B, cOrd, fOrd = s["m"], s["mesh"], s["A"], s["N"], s["B"], s["cOrd"], s["fOrd"]
    dev = lambda v: ctx.to_device(np.ascontiguousarray(v, np.float64))
    H = lambda v: np.ascontiguousarray(v, np.float64).ctypes.data_as(dp)
    pi = 3.14159265358979323846
    rays = _ray_set(nPhi, nTheta)
    nRay = len(rays)
    Sf, bSf = m.Sf[fOrd], np.concatenate([p.Sf for p in m.patches])
    V, T, E = m.V[cOrd], s["T"][cOrd], s["Q"][cOrd]
    T2 = T * T
    sigmaT4 = SIGMA * (T2 * T2)
    Tb, em, zeroB = dev(np.concatenate(s["Tb"])), dev(np.concatenate(s["emis"])), ctx.zeros(B)
    qin, qem, qr = ctx.zeros(nRay * B), ctx.zeros(nRay * B), ctx.zeros(nRay * B)
    I, Ib, orders = [ctx.zeros(N) for _ in rays], [ctx.zeros(B) for _ in rays], [None] * nRay
    for _ in range(nCalls):
        for i, (d, dAve, omega) in enumerate(rays):
            j = (dAve[0] * Sf[:, 0] + dAve[1] * Sf[:, 1]) + dAve[2] * Sf[:, 2]
            jb = (dAve[0] * bSf[:, 0] + dAve[1] * bSf[:, 1]) + dAve[2] * bSf[:, 2]
            f, ref = ctx.zeros(B), ctx.zeros(B)
            d3, a3 = np.ascontiguousarray(d), np.ascontiguousarray(dAve)
            mesh.call("fvdom_wall_coeffs_d", nRay, i, H(d3), H(a3), SIGMA, Ib[i], em, Tb, qin, qem, qr, f, ref)
            Jn, w = mesh.to_native(j), ctx.zeros(mesh.nNative)
            mesh.call("fv_limited_weights", 0, 1.0, 0.0, 1.0, Jn, None, None, None, None, w)
            d1, u1, l1 = ctx.zeros(N), ctx.zeros(mesh.nNative), ctx.zeros(mesh.nNative)
            mesh.call("fvm_transport", 0.0, None, Jn, w, None, 0, d1, u1, l1)
            ic, bc = ctx.zeros(B), ctx.zeros(B)
            mesh.call("fvm_boundary_coeffs", dev(jb), None, 0, f, ref, zeroB, ic, bc)
            dn = d1.cpu().numpy() + V * (a * omega)
            sn = 0.0 + V * ((1.0 / pi * omega) * (a * sigmaT4 + E / 4.0))
            d2, s2 = ctx.zeros(N), ctx.zeros(N)
            mesh.call("fvm_add_boundary", ic, bc, dev(dn), dev(sn), None, d2, s2)
            A.bind_coeffs_native(d2, u1, l1)
            if orders[i] is None:
                orders[i] = A.flow_order()
            perf = A.solve_ordered(orders[i], I[i], s2)
            A.unbind_coeffs()
            assert perf["nIterations"] == 1
            mesh.call("bc_values", f, ref, zeroB, I[i], Ib[i])
    G = np.zeros(N)
    Ih = [t.cpu().numpy() for t in I]
    for Ii, (_, _, omega) in zip(Ih, rays):
        G = G + Ii * omega
    qinS, qrS = ctx.zeros(B), ctx.zeros(B)
    mesh.call("fvdom_sum_rays_d", nRay, qin, qinS)
    mesh.call("fvdom_sum_rays_d", nRay, qr, qrS)
    for o in orders:
        o.close()
    return dict(I=np.array(Ih), G=G, Gb=qinS.cpu().numpy(), qr=qrS.cpu().numpy())


def _p1_scalar_driver(ctx, s, a, e, nCalls, tol=1e-6):
    """b1_p1, the driver of tests/test_p1_foam_gpu.py (constants, hooks never touched): G, G_b, qr, the iteration counts and the system of
    the class layer beside ffm_p1_assemble_d's"""
    lib, mesh, A, N, B, cOrd = s["lib"], s["mesh"], s["A"], s["N"], s["B"], s["cOrd"]
    h = lambda v: np.ascontiguousarray(v, np.float64)
    P = lambda v: v.ctypes.data_as(dp)
    Tc, Tbb, Ec, emb = h(s["T"][cOrd]), h(np.concatenate(s["Tb"])), h(s["Q"][cOrd]), h(np.concatenate(s["emis"]))
    out = dict(G=np.empty(N), Gb=np.empty(B), qr=np.empty(B), sysC=np.empty(mesh.nNative + 2 * N), sysF=np.empty(mesh.nNative + 2 * N))
    iters = (C.c_int * nCalls)()
    lib.b1_p1.restype = C.c_int
    lib.b1_p1.argtypes = [C.c_void_p] * 3 + [C.c_double] * 4 + [dp] * 4 + [C.c_double, C.c_int] + [dp] * 3 + [C.POINTER(C.c_int)] + [dp] * 2
    ctx._ready()
    n = lib.b1_p1(ctx.h, A.h, mesh.h, a, e, 0.0, 0.0, P(Tc), P(Tbb), P(Ec), P(emb), tol, nCalls, P(out["G"]), P(out["Gb"]), P(out["qr"]), iters,
                  P(out["sysC"]), P(out["sysF"]))
    assert n == nCalls
    out["iters"] = list(iters)
    return out


@pytest.mark.parametrize("model", [1, 2], ids=["fvDOM", "P1"])
def test_hooks_unset_give_the_scalar_abi_chains_bits(O, ffm, ctx, case, model):
    s = case
    m, N, cOrd = s["m"], s["N"], s["cOrd"]
    a, e = 0.3, (0.3 if model == 1 else 0.45)
    unset = _run(ctx, s, model, 0, aConst=a, eConst=e)
    # the providers set to the uniform constants: the field statements with a uniform field give the constant's bits
    uniform = _run(ctx, s, model, 2, aConst=a, eConst=e)
    assert unset["iters"] == uniform["iters"] and unset["rc"] == uniform["rc"]
    for k in ("G", "Gb", "qr", "sh") + (("I",) if model == 1 else ()):
        assert np.isfinite(unset[k]).all() and unset[k].tobytes() == uniform[k].tobytes(), k
    assert np.ptp(unset["G"]) > 0
    if model == 1:
        # every ray, G and the summed wall fluxes: the scalar entry points, called from here
        chain = _fvdom_scalar_abi_chain(ctx, s, a, 2, 2, 2)
        for k in ("I", "G", "Gb", "qr"):
            assert unset[k].tobytes() == chain[k].tobytes(), (k, np.abs(unset[k] - chain[k]).max())
    else:
        # the driver that never touches the hooks, and its system beside ffm_p1_assemble_d's (scalar a, e)
        old = _p1_scalar_driver(ctx, s, a, e, 2)
        assert old["iters"] == unset["iters"]
        for k in ("G", "Gb", "qr"):
            assert unset[k].tobytes() == old[k].tobytes(), k
        nNat, fm = s["mesh"].nNative, s["A"].face_map()
        for name, c, f in (("upper", old["sysC"][:nNat][fm], old["sysF"][:nNat][fm]), ("diag", old["sysC"][nNat:nNat + N], old["sysF"][nNat:nNat + N]),
                           ("source", old["sysC"][nNat + N:], old["sysF"][nNat + N:])):
            assert np.isfinite(c).all() and np.array_equal(c, f), name
    # Sh against the scalar ABI fed with the handle's own G
    L = ffm.lib()
    dev = lambda v: ctx.to_device(np.ascontiguousarray(v))
    G, T, he, Q, Cp, V = unset["G"], s["T"][cOrd], s["he"][cOrd], s["Q"][cOrd], s["Cp"][cOrd], m.V[cOrd]
    Gd, Td, hd, Qd, Cd = dev(G), dev(T), dev(he), dev(Q), dev(Cp)
    su, sp = ctx.zeros(N), ctx.zeros(N)
    P = lambda t: C.c_void_p(t.data_ptr())
    ctx._ready()
    if model == 1:                      # a = e: the scalar entry point as it stands
        assert L.ffm_radiation_sh_d(ctx.h, N, a, SIGMA, 1.0, P(Gd), P(Td), P(hd), P(Qd), P(Cd), 1005.0, P(su), P(sp)) == 0
    else:                               # a != e: the scalar entry point has one coefficient, so the field form carries the two constants
        ad, ed = dev(np.full(N, a)), dev(np.full(N, e))
        assert L.ffm_radiation_sh_v_d(ctx.h, N, P(ad), P(ed), SIGMA, P(Qd), P(Gd), P(Td), P(hd), P(Cd), 1005.0, P(su), P(sp)) == 0
    ctx.sync()
    su, sp = su.cpu().numpy(), sp.cpu().numpy()
    assert np.array_equal(unset["sh"][:N], -(V * sp))
    # the source: the ABI forms su = Ru - X in one expression, the class layer two fvm::Su terms, (0 - V*Ru) - (0 - V*X): the ABI's pieces,
    # rounded as the class layer rounds them
    Ru = a * G - Q
    RpT3 = (4.0 * e * SIGMA) * (T * (T * T))
    X = RpT3 * (T - 4.0 * he / Cp)
    assert np.array_equal(su, Ru - X) and np.array_equal(sp, 4.0 * RpT3 / Cp)            # (the pieces are the ABI's)
    assert unset["sh"][N:].tobytes() == ((0.0 - V * Ru) - (0.0 - V * X)).tobytes()
