"""The two kernels the compiled step gains with the janaf thermo, on their own.

ffm_thermo_step_d (csrc/ffm_thermo.hip), the fused thermo.correct(): bit for bit the pair it replaces, ffm_thermo_correct_d +
ffm_thermo_Cp_d -- same mixture, same Newton iteration, Cp at the new T evaluated once -- on the edge table and inputs of
tests/physics_edge_inputs.py (eight species that differ in every constant, absent leading species, enthalpies outside the range, start
temperatures across Tcommon), at launches of 0, 1, 255, 257 cells and of 524291, more than one pass of the grid covers; guards around
every output stay intact; the failure flag is raised, and only raised, on the table whose enthalpy jumps at Tcommon.

ffm_les_face_diffusivity_v (csrc/ffm_fused.hip): both modes with and without x, against numpy bit for bit (the operations are + - * /,
correctly rounded on both sides, contraction off) on one mesh per row-width bucket -- the meshes of tests/test_les_row_kernels_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import physics_edge_inputs as E
from test_les_row_kernels_gpu import MESHES, SENTINEL, _bits, _inputs, meshes  # noqa: F401  (meshes: the module fixture)
from test_thermo_edges_gpu import GRID_PASS, GUARD, _P, _guarded, _guards_intact

pytestmark = pytest.mark.gpu

FILL = -12345.0


@pytest.fixture(scope="module")
def syn8(ffm, ctx):
    from oracle import thermo as TH
    names, tab = E.synthetic_table(8)
    th = ffm.Thermo(ctx, names, tab, TH.RR)
    yield th, TH.Species(names, tab)
    th.close()


def _edge_inputs(sp, n):
    """compositions with absent leading species; enthalpies inside the range, below Hs(Tlow), above Hs(Thigh) and at Tcommon; start
    temperatures on both sides of Tcommon and off the answer by up to 5 % (more than one Newton iteration)"""
    m = max(n, 1)
    Y = E.compositions(8, m, seed=21)
    mx = sp.mixture(Y)
    Tt = E.hashed(22, m, 300.0, 2500.0)
    he = mx.Hs(0.0, Tt)
    he[5::15] = mx.Hs(0.0, np.full(m, 1000.0))[5::15]
    he[3::7] = mx.Hs(0.0, mx.Tlow * np.ones(m))[3::7] - 1.0e5           # (after the line above: cell 80 is in both sets)
    he[4::7] = mx.Hs(0.0, mx.Thigh * np.ones(m))[4::7] + 1.0e5
    T0 = Tt * (1.0 + 0.05 * (E.hashed(23, m) - 0.5))
    return Y, he, T0


@pytest.mark.parametrize("n", [0, 1, 255, 257, GRID_PASS + 3])
def test_fused_thermo_pass_is_bitwise_the_pair_it_replaces(ffm, ctx, syn8, n):
    th, sp = syn8
    L = ffm.lib()
    D = lambda a: ctx.to_device(np.ascontiguousarray(a, np.float64))
    Y, he, T0 = _edge_inputs(sp, n)
    if n > GRID_PASS:
        i = np.arange(n - GRID_PASS)
        assert np.all(he[i] != he[i + GRID_PASS]) and np.all(T0[i] != T0[i + GRID_PASS])
    Yd, hed = [D(y) for y in Y], D(he)
    Yp = (C.c_void_p * 8)(*[y.data_ptr() for y in Yd])
    # ---- the pair
    pair = [_guarded(ctx, n, FILL) for _ in range(5)]
    (Tb, Tp), (pb, pp), (mb, mp), (ab, ap), (cb, cp) = pair
    if n:
        Tb[GUARD:GUARD + n] = D(T0[:n])
    ctx._ready()
    assert L.ffm_thermo_correct_d(th.h, n, Yp, _P(hed), None, Tp, pp, mp, ap) == 0
    assert L.ffm_thermo_Cp_d(th.h, n, Yp, Tp, cp) == 0
    ctx.sync()
    # ---- the fused pass
    one = [_guarded(ctx, n, FILL) for _ in range(5)]
    (Tb1, Tp1), (_, pp1), (_, mp1), (_, ap1), (_, cp1) = one
    if n:
        Tb1[GUARD:GUARD + n] = D(T0[:n])
    flag = ctx.zeros(1)
    ctx._ready()
    assert L.ffm_thermo_step_d(th.h, n, Yp, _P(hed), Tp1, pp1, mp1, ap1, cp1, _P(flag)) == 0
    ctx.sync()
    assert flag.cpu().numpy().view(np.int32)[0] == 0
    for name, (a, _), (b, _) in zip(("T", "psi", "mu", "alpha", "Cp"), pair, one):
        assert _guards_intact(b, n, FILL), (n, name)
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), (n, name)
    if n == 0:
        assert all(np.all(b.cpu().numpy() == FILL) for b, _ in one)
        return
    # and the pair is what the oracle says (so equal does not mean equally empty): T and Cp, with the edges where they were put
    mxn = sp.mixture(Y[:, :n])
    Tr = mxn.THs(he[:n], 0.0, T0[:n])
    T = Tb1.cpu().numpy()[GUARD:GUARD + n]
    assert np.abs(T - Tr).max() <= 1e-13 * np.abs(Tr).max()
    assert np.array_equal(one[4][0].cpu().numpy()[GUARD:GUARD + n], mxn.Cp(0.0, T))
    if n > 16:
        assert np.array_equal(T[3::7], (mxn.Tlow * np.ones(n))[3::7]) and np.array_equal(T[4::7], (mxn.Thigh * np.ones(n))[4::7])
        assert (T < 1000.0).any() and (T > 1000.0).any()


def test_fused_thermo_pass_raises_its_flag_and_never_clears_it(ffm, ctx):
    from oracle import thermo as TH
    names, tab, he_mid, _ = E.jump_table()
    th = ffm.Thermo(ctx, names, tab, TH.RR)
    L = ffm.lib()
    n = 300
    D = lambda a: ctx.to_device(np.ascontiguousarray(a, np.float64))
    Y = [D(np.ones(n))]
    Yp = (C.c_void_p * 1)(Y[0].data_ptr())
    mx = TH.Species(names, tab).single(0)
    he = mx.Hs(0.0, np.full(n, 600.0)) * np.ones(n)
    bad = he.copy(); bad[137] = he_mid                            # one cell whose enthalpy no temperature has
    out = [ctx.empty(n) for _ in range(4)]
    flag = ctx.zeros(1)
    for h, want in ((he, 0), (bad, 1), (he, 1)):                  # clean; raised; a clean pass after it leaves it raised
        T = D(np.full(n, 900.0))
        ctx._ready()
        assert L.ffm_thermo_step_d(th.h, n, Yp, _P(D(h)), _P(T), *[_P(o) for o in out], _P(flag)) == 0      # no read-back: the call itself is OK
        ctx.sync()
        assert flag.cpu().numpy().view(np.int32)[0] == want
    assert np.abs(T.cpu().numpy() - 600.0).max() < 1e-6
    th.close()


@pytest.mark.parametrize("variant", ["mode0", "mode1", "mode0,laminar", "mode1,laminar"])
@pytest.mark.parametrize("name", list(MESHES))
def test_face_diffusivity_v_against_numpy(meshes, O, ctx, name, variant):  # noqa: F811
    from oracle import fv
    s = meshes(name); m, mesh, N, c, f = s["m"], s["mesh"], s["N"], s["cOrd"], s["fOrd"]
    d = _inputs(s, O)
    lam = 1.2e-5 + 6.0e-5 * O.hash_u(77, np.arange(N))            # a laminar part that varies from cell to cell (mu, alpha of a flame)
    lamb = [lam[p.faceCells] for p in m.patches]                  # zero-gradient
    dev = ctx.to_device
    cat = lambda bs: dev(np.concatenate(bs))
    outf, outb = ctx.zeros(mesh.nNative) + SENTINEL, ctx.zeros(s["B"]) + SENTINEL
    mode = 0 if variant.startswith("mode0") else 1
    if variant.endswith("laminar"):
        mesh.call("les_face_diffusivity_v", mode, dev(lam[c]), None, None, None, None, outf, outb)
        cell, patch = lam, lamb
    elif mode == 0:
        mesh.call("les_face_diffusivity_v", 0, dev(lam[c]), dev(d["rho"][c]), cat(d["rhob"]), dev(d["nut"][c]), cat(d["nutb"]), outf, outb)
        cell = d["rho"] * (d["nut"] + lam / d["rho"])
        patch = [r * (n + lb / r) for r, n, lb in zip(d["rhob"], d["nutb"], lamb)]
    else:
        mesh.call("les_face_diffusivity_v", 1, dev(lam[c]), None, None, dev(d["alphat"][c]), cat(d["alphatb"]), outf, outb)
        cell = lam + d["alphat"]
        patch = [lb + b for lb, b in zip(lamb, d["alphatb"])]
    want, _ = fv.interpolate(m, cell, patch)
    assert np.array_equal(_bits(mesh.from_native(outf)), _bits(want[f]))
    assert np.array_equal(_bits(outb.cpu().numpy()), _bits(np.concatenate(patch)))
    # only real faces are written (as ffm_fvc_interpolate)
    assert np.array_equal(_bits(outf.cpu().numpy()[s["pad"]]), _bits(np.full(int(s["pad"].sum()), SENTINEL)))
