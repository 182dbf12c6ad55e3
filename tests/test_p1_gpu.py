"""The kernels of the P1 radiation model (csrc/ffm_p1.hip) on the device.

  (a) ffm_p1_assemble_d == the chain of entry points it restates, bit for bit -- ffm_p1_gamma_d (cells, patches), ffm_fvc_interpolate,
      ffm_fvm_transport (laplacian alone, sign +1), ffm_p1_marshak_coeffs_d, ffm_fvm_boundary_coeffs, diag -= V a, source = 0 + V su,
      ffm_fvm_add_boundary -- in every row-width bucket of FFM_DISPATCH_W (the meshes of tests/test_fused_gpu.py's ray assembly), with
      hashed cell fields and emissivities that are exactly 1 on some faces and exactly 0 on others, and once more in the constant
      (NULL-array) forms; the argument checks leave poisoned outputs alone;
  (b) matrix and source against tests/p1_ref.py at the bound tests/test_fused_gpu.py holds operator outputs to (rel-L2 < 1e-14), then
      lduMatrix.solve (PCG + DIC, 1e-6, relTol 0) against the oracle's solve of the restated system: the same iteration count and G
      within 1e-8; ffm_p1_wall_flux_d == ffm_bc_values + ffm_fvc_snGrad_b + one multiply bit for bit, and within 1e-8 of the restatement;
  (c) equilibrium: uniform T, T_b = T, emissivity 1, a = e, solved to 1e-12 from G = 0: max |G/(4 sigma T^4) - 1| < 1e-9 (a normalised
      residual of 1e-12 times a condition number of at most about 1e3 at this size)."""
import ctypes as C

import numpy as np
import pytest

import merged_mesh as MM
import p1_ref as P1
from common import rel_l2

pytestmark = pytest.mark.gpu

MESHES = ["hex", "w8", "w16u14", "w32l30", "w32u18"]
BUCKET = {"hex": 3, "w8": 8, "w16u14": 16, "w32l30": 32, "w32u18": 32, "w32multi": 32}
ERR_ARG = -1
SIG = P1.SIGMA


def _bucket(s):
    return MM.bucket(max(np.bincount(s["l"]).max(), np.bincount(s["u"]).max()))


def _device(ffm, ctx, which, n=(9, 8, 7)):
    from oracle import plume
    m = plume.make_mesh(n, h=0.1) if which == "hex" else MM.case(which)
    s = MM.device_mesh(ffm, ctx, m)
    assert _bucket(s) == BUCKET[which]
    return s


def _ptr(a):
    return None if a is None else C.c_void_p(a.data_ptr())


def _gamma(ffm, ctx, n, a, aConst, sigmaEff, out):
    ctx._ready()
    rc = ffm.lib().ffm_p1_gamma_d(ctx.h, n, _ptr(a), aConst, sigmaEff, _ptr(out))
    ctx.sync()
    return rc


def _h(O, seed, n, lo, hi):
    return lo + (hi - lo) * O.hash_u(seed, np.arange(n))


def _emissivity(O, B):
    em = 1.0 - O.hash_u(47, np.arange(B))                        # (0, 1]
    em[::7] = 1.0; em[3::11] = 0.0
    assert (em == 1.0).any() and (em == 0.0).any() and ((em > 0) & (em < 1)).any()
    return em


def _chain(ffm, ctx, s, sigmaEff, a, aConst, a_b, e, eConst, E, T, Tb, em):
    """the per-operator chain; a, a_b, e, E: numpy arrays or None (the constants); returns numpy arrays in the device's orders"""
    mesh, N, B = s["mesh"], s["N"], s["B"]
    dev = ctx.to_device
    V = s["m"].V[s["cOrd"]]
    ad, abd = (None if a is None else dev(a)), (None if a_b is None else dev(a_b))
    gam, gb = ctx.zeros(N), ctx.zeros(B)
    assert _gamma(ffm, ctx, N, ad, aConst, sigmaEff, gam) == 0 and _gamma(ffm, ctx, B, abd, aConst, sigmaEff, gb) == 0
    gf = ctx.zeros(mesh.nNative)
    mesh.call("fvc_interpolate", None, gam, gf)
    d1, u1 = ctx.zeros(N), ctx.zeros(mesh.nNative)
    mesh.call("fvm_transport", 0.0, None, None, None, gf, 1, d1, u1, None)
    f, ref = ctx.zeros(B), ctx.zeros(B)
    mesh.call("p1_marshak_coeffs_d", SIG, gb, dev(Tb), dev(em), f, ref)
    ic, bc = ctx.zeros(B), ctx.zeros(B)
    mesh.call("fvm_boundary_coeffs", None, gb, 1, f, ref, ctx.zeros(B), ic, bc)
    # the cell algebra on the host, in IEEE double without contraction: diag -= V*a; source = 0 + V*su (fvMatrix == volField)
    an = np.full(N, aConst) if a is None else a
    en = np.full(N, eConst) if e is None else e
    su = -(4.0 * ((en * SIG) * ((T * T) * (T * T))))
    if E is not None:
        su = su - E
    d1n = d1.cpu().numpy() - V * an
    srn = 0.0 + V * su
    d2, s2 = ctx.zeros(N), ctx.zeros(N)
    mesh.call("fvm_add_boundary", ic, bc, dev(d1n), dev(srn), None, d2, s2)
    cpu = lambda t: t.cpu().numpy()
    return dict(upper=mesh.from_native(u1), diag=cpu(d2), source=cpu(s2), gamma_b=cpu(gb), f=cpu(f), ref=cpu(ref))


def _assemble(ctx, s, sigmaEff, a, aConst, a_b, e, eConst, E, T, Tb, em):
    mesh, N, B = s["mesh"], s["N"], s["B"]
    dev = lambda x: None if x is None else ctx.to_device(x)
    up, dg, sr = ctx.zeros(mesh.nNative), ctx.zeros(N), ctx.zeros(N)
    gb, fb, rb = ctx.zeros(B), ctx.zeros(B), ctx.zeros(B)
    mesh.call("p1_assemble_d", sigmaEff, SIG, dev(a), aConst, dev(a_b), dev(e), eConst, dev(E), dev(T), dev(Tb), dev(em), up, dg, sr, gb, fb, rb)
    cpu = lambda t: t.cpu().numpy()
    return dict(upper=mesh.from_native(up), diag=cpu(dg), source=cpu(sr), gamma_b=cpu(gb), f=cpu(fb), ref=cpu(rb)), (up, dg, sr, gb, fb, rb)


@pytest.mark.parametrize("which", MESHES)
def test_assembly_equals_the_operator_chain(O, ffm, ctx, which):
    s = _device(ffm, ctx, which)
    N, B = s["N"], s["B"]
    a, e, E = _h(O, 41, N, 0.05, 3.0), _h(O, 42, N, 0.05, 3.0), _h(O, 43, N, 0.0, 5e4)
    T, Tb, a_b = _h(O, 44, N, 300.0, 1500.0), _h(O, 45, B, 300.0, 900.0), _h(O, 46, B, 0.05, 3.0)
    em = _emissivity(O, B)
    for form, (sigmaEff, av, abv, ev, Ev) in (("fields", (0.35 * (3.0 - 0.2), a, a_b, e, E)), ("constants", (0.0, None, None, None, None))):
        aConst, eConst = 0.7, 0.4
        want = _chain(ffm, ctx, s, sigmaEff, av, aConst, abv, ev, eConst, Ev, T, Tb, em)
        got, _ = _assemble(ctx, s, sigmaEff, av, aConst, abv, ev, eConst, Ev, T, Tb, em)
        for k in ("upper", "diag", "source", "gamma_b", "f", "ref"):
            assert np.isfinite(got[k]).all(), (form, k)
            assert np.array_equal(got[k], want[k]), (which, form, k, np.abs(got[k] - want[k]).max())
        assert np.abs(got["upper"]).min() > 0
        assert np.all(got["f"][em == 0.0] == 0.0) and np.all(got["f"][em > 0.0] > 0.0)
    s["mesh"].close(); s["A"].close()


def test_argument_checks_leave_the_outputs_alone(O, ffm, ctx):
    s = _device(ffm, ctx, "hex", n=(4, 5, 3))
    mesh, N, B = s["mesh"], s["N"], s["B"]
    L = ffm.lib()
    dev = ctx.to_device
    T, Tb, em, gbin = dev(np.full(N, 500.0)), dev(np.full(B, 400.0)), dev(np.full(B, 0.5)), dev(np.full(B, 0.6))
    POISON = 7.25
    outs = dict(up=dev(np.full(mesh.nNative, POISON)), dg=dev(np.full(N, POISON)), sr=dev(np.full(N, POISON)), gb=dev(np.full(B, POISON)),
                fb=dev(np.full(B, POISON)), rb=dev(np.full(B, POISON)), Gb=dev(np.full(B, POISON)), qr=dev(np.full(B, POISON)), gam=dev(np.full(N, POISON)))
    ctx._ready()

    def assemble(msh=mesh.h, T_=T, Tb_=Tb, up="up", dg="dg", sr="sr", gb="gb", fb="fb", rb="rb"):
        o = lambda k: None if k is None else _ptr(outs[k])
        return L.ffm_p1_assemble_d(msh, 0.0, SIG, None, 0.5, None, None, 0.5, None, _ptr(T_), _ptr(Tb_), _ptr(em), o(up), o(dg), o(sr), o(gb), o(fb), o(rb))
    assert assemble(msh=None) == ERR_ARG and assemble(T_=None) == ERR_ARG and assemble(Tb_=None) == ERR_ARG
    for k in ("up", "dg", "sr", "gb", "fb", "rb"):
        assert assemble(**{k: None}) == ERR_ARG, k
    g, f, r, G = _ptr(gbin), _ptr(em), _ptr(Tb), _ptr(T)
    assert L.ffm_p1_marshak_coeffs_d(None, SIG, g, r, f, _ptr(outs["fb"]), _ptr(outs["rb"])) == ERR_ARG
    assert L.ffm_p1_marshak_coeffs_d(mesh.h, SIG, None, r, f, _ptr(outs["fb"]), _ptr(outs["rb"])) == ERR_ARG
    assert L.ffm_p1_marshak_coeffs_d(mesh.h, SIG, g, None, f, _ptr(outs["fb"]), _ptr(outs["rb"])) == ERR_ARG
    assert L.ffm_p1_marshak_coeffs_d(mesh.h, SIG, g, r, f, None, _ptr(outs["rb"])) == ERR_ARG
    assert L.ffm_p1_marshak_coeffs_d(mesh.h, SIG, g, r, f, _ptr(outs["fb"]), None) == ERR_ARG
    assert L.ffm_p1_wall_flux_d(None, g, f, r, G, _ptr(outs["Gb"]), _ptr(outs["qr"])) == ERR_ARG
    for i in range(6):
        args = [g, f, r, G, _ptr(outs["Gb"]), _ptr(outs["qr"])]
        args[i] = None
        assert L.ffm_p1_wall_flux_d(mesh.h, *args) == ERR_ARG, i
    assert L.ffm_p1_gamma_d(None, N, None, 0.5, 0.0, _ptr(outs["gam"])) == ERR_ARG
    assert L.ffm_p1_gamma_d(ctx.h, N, None, 0.5, 0.0, None) == ERR_ARG
    assert L.ffm_p1_gamma_d(ctx.h, -1, None, 0.5, 0.0, _ptr(outs["gam"])) == ERR_ARG
    assert L.ffm_p1_gamma_d(ctx.h, 0, None, 0.5, 0.0, _ptr(outs["gam"])) == 0          # n == 0: a no-op
    ctx.sync()
    for k, t in outs.items():
        assert np.all(t.cpu().numpy() == POISON), k
    assert assemble() == 0                                                            # ... and the same call with everything given runs
    ctx.sync()
    assert np.all(outs["dg"].cpu().numpy() != POISON)
    mesh.close(); s["A"].close()


@pytest.mark.parametrize("which", ["hex", "w32multi"])
def test_system_solve_and_wall_flux_against_the_restatement(O, ffm, ctx, which):
    s = _device(ffm, ctx, which, n=(7, 8, 6))
    m, mesh, A, N, B, cOrd = s["m"], s["mesh"], s["A"], s["N"], s["B"], s["cOrd"]
    # inputs in the oracle's numbering; the device takes the cells in its own order, the boundary faces patch after patch as they are
    a, e, E = _h(O, 51, N, 0.05, 3.0), _h(O, 52, N, 0.05, 3.0), _h(O, 53, N, 0.0, 5e4)
    x, y = m.C[:, 0], m.C[:, 1]
    T = 400.0 + 900.0 * np.exp(-((x - x.mean()) ** 2 + (y - 0.4 * y.max()) ** 2) / 0.03)
    split = lambda v: np.split(v, np.cumsum([p.size for p in m.patches])[:-1])
    Tb, a_b, em = _h(O, 55, B, 300.0, 900.0), _h(O, 56, B, 0.05, 3.0), _emissivity(O, B)
    sigma_s, Cs = 0.35, 0.2
    S = P1.system(m, a, e, E, T, split(Tb), split(em), sigma_s, Cs, a_b=split(a_b))
    got, (up, dg, sr, gb, fb, rb) = _assemble(ctx, s, sigma_s * (3.0 - Cs), a[cOrd], 0.0, a_b, e[cOrd], 0.0, E[cOrd], T[cOrd], Tb, em)
    cells = lambda v: _cells_o(s, v)
    upper_o = np.empty(s["F"]); upper_o[s["fOrd"]] = got["upper"]
    errs = dict(upper=rel_l2(upper_o, S.upper), diag=rel_l2(cells(got["diag"]), S.d), source=rel_l2(cells(got["source"]), S.s),
                f=rel_l2(got["f"], np.concatenate(S.bc.f)), ref=rel_l2(got["ref"], np.concatenate(S.bc.ref)))
    print("%s: %s" % (which, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert all(v < 1e-14 for v in errs.values()), errs
    # the solve: PCG + DIC at the `G` entry's controls from G = 0
    G = ctx.zeros(N)
    A.bind_coeffs_native(dg, up, None)
    perf = A.solve(G, sr, solver="PCG", preconditioner="DIC", tolerance=1e-6, relTol=0.0)
    A.unbind_coeffs()
    Gref, pref = P1.solve(O, m, S, np.zeros(N), tolerance=1e-6)
    print("%s: %d iterations (restatement %d), G %.2e" % (which, perf["nIterations"], pref["nIterations"], rel_l2(cells(G.cpu().numpy()), Gref)))
    assert perf["nIterations"] == pref["nIterations"] and perf["converged"]
    assert rel_l2(cells(G.cpu().numpy()), Gref) < 1e-8
    # the wall flux
    Gb, qr = ctx.zeros(B), ctx.zeros(B)
    mesh.call("p1_wall_flux_d", gb, fb, rb, G, Gb, qr)
    Gb2, sn = ctx.zeros(B), ctx.zeros(B)
    mesh.call("bc_values", fb, rb, ctx.zeros(B), G, Gb2)
    mesh.call("fvc_snGrad_b", G, Gb2, sn)
    assert np.array_equal(Gb.cpu().numpy(), Gb2.cpu().numpy())
    assert np.array_equal(qr.cpu().numpy(), -gb.cpu().numpy() * sn.cpu().numpy())
    Gb_ref, qr_ref = P1.wall(m, S, Gref)
    eG, eq = rel_l2(Gb.cpu().numpy(), np.concatenate(Gb_ref)), rel_l2(qr.cpu().numpy(), np.concatenate(qr_ref))
    print("%s: G_b %.2e, qr %.2e" % (which, eG, eq))
    assert eG < 1e-8 and eq < 1e-8
    assert np.abs(qr.cpu().numpy()).max() > 0
    mesh.close(); A.close()


def _cells_o(s, a):
    out = np.empty(s["N"]); out[s["cOrd"]] = a
    return out


def test_equilibrium_on_the_device(O, ffm, ctx):
    s = _device(ffm, ctx, "hex", n=(7, 8, 6))
    mesh, A, N, B = s["mesh"], s["A"], s["N"], s["B"]
    T, a = 1200.0, 0.5
    got, (up, dg, sr, gb, fb, rb) = _assemble(ctx, s, 0.0, None, a, None, None, a, None, np.full(N, T), np.full(B, T), np.ones(B))
    G = ctx.zeros(N)
    A.bind_coeffs_native(dg, up, None)
    perf = A.solve(G, sr, solver="PCG", preconditioner="DIC", tolerance=1e-12, relTol=0.0)
    A.unbind_coeffs()
    err = np.abs(G.cpu().numpy() / (4.0 * SIG * T ** 4) - 1.0).max()
    print("equilibrium: %d iterations, final residual %.2e, max |G/(4 sigma T^4) - 1| = %.3e" % (perf["nIterations"], perf["finalResidual"], err))
    assert perf["converged"] and err < 1e-9
    Gb, qr = ctx.zeros(B), ctx.zeros(B)
    mesh.call("p1_wall_flux_d", gb, fb, rb, G, Gb, qr)
    assert np.abs(qr.cpu().numpy()).max() < 1e-7 * SIG * T ** 4                       # (the solve's 1e-9 on G, over gamma_b*delta_b*f of order 10)
    mesh.close(); A.close()
