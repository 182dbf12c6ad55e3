"""The two radiation cell passes of csrc/ffm_rad.hip on their own, against numpy, BITWISE: only + - * / occur, correctly rounded on both
sides, in a stated order, contraction off.

ffm_radiation_sh_d -- radiation->Sh(thermo, he) of solver/YEEqn.H:101 in the operation order of oracle/plume.py:464-468:
    Rp = 4 a sigma, Ru = a G - radFraction*Qdot, T3 = T*T*T, sp = 4.0*Rp*T3/Cp, su = Ru - Rp*T3*(T - 4.0*he/Cp)
with Cp a field or (Cp_d NULL) a constant, radFraction 0 and non-zero, T from 250 to 2500 K, G and Qdot with exact zeros.

ffm_fvdom_G_d -- fvDOM::updateG's cell part: ((0 + I_0 w_0) + I_1 w_1) + ... in ray-index order, the bytes of the sequential passes
G = G + I_i*omega_i over a zeroed G; nRay 1, 8, 32, 33 (and 128).

n in {1, 63, 64, 65, 255, 256, 257, 1000, 4099}: below, at and above a wave and a workgroup, several workgroups, no multiple of either.
Output buffers lie between guards filled with a sentinel, which stay untouched; n == 0 writes nothing; argument refusals return
FFM_ERR_ARG without a launch (the outputs keep the sentinel)."""

import numpy as np
import pytest

from test_thermo_edges_gpu import GUARD, _P, _guarded, _guards_intact

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, 4099]
FILL = -12345.0
SIGMA = 5.670367e-8
CP_CONST = 1005.0
ERR_ARG = -1


def _sh_inputs(n, seed):
    r = np.random.RandomState(seed)
    T = r.uniform(250.0, 2500.0, n); T[0] = 250.0; T[-1] = 2500.0
    G = r.uniform(0.0, 4.0e5, n); G[::3] = 0.0
    Q = r.uniform(0.0, 5.0e6, n); Q[1::4] = 0.0
    he = r.uniform(-6.0e4, 3.5e6, n)
    Cp = r.uniform(900.0, 2500.0, n)
    return G, T, he, Q, Cp


def _sh_numpy(a, frac, G, T, he, Q, Cp):
    Rp = 4.0 * a * SIGMA
    T3 = T * T * T
    Ru = a * G - frac * Q
    return Ru - Rp * T3 * (T - 4.0 * he / Cp), 4.0 * Rp * T3 / Cp


def _inner(buf, n):
    return buf.cpu().numpy()[GUARD:GUARD + n]


@pytest.mark.parametrize("n", SIZES)
def test_radiation_sh_against_numpy_bitwise(ffm, ctx, n):
    L = ffm.lib()
    G, T, he, Q, Cp = _sh_inputs(n, 100 + n)
    dev = [ctx.to_device(x) for x in (G, T, he, Q, Cp)]
    for a, frac, field in [(0.1, 0.36, True), (0.1, 0.36, False), (0.1, 0.0, True), (0.0, 0.22, False), (0.08, 0.0, False)]:
        (sub, sup), (spb, spp) = _guarded(ctx, n, FILL), _guarded(ctx, n, FILL)
        ctx._ready()
        assert L.ffm_radiation_sh_d(ctx.h, n, a, SIGMA, frac, *[_P(d) for d in dev[:4]], _P(dev[4]) if field else None, CP_CONST, sup, spp) == 0
        ctx.sync()
        su, sp = _sh_numpy(a, frac, G, T, he, Q, Cp if field else CP_CONST)
        assert _guards_intact(sub, n, FILL) and _guards_intact(spb, n, FILL), (n, a, frac, field)
        assert _inner(sub, n).tobytes() == su.tobytes(), (n, a, frac, field, "su")
        assert _inner(spb, n).tobytes() == sp.tobytes(), (n, a, frac, field, "sp")


def _rays(n, nRay, seed):
    r = np.random.RandomState(seed)
    I = r.uniform(0.0, 3.0e4, (nRay, n)); I[:, 1::5] = 0.0
    I[nRay // 2] = -I[nRay // 2]                                       # mixed signs: the order of the additions shows
    omega = r.uniform(0.05, 0.8, nRay)
    return I, omega


def _ray_table(ctx, I):
    rays = [ctx.to_device(row) for row in I]
    table = ctx.torch.as_tensor(np.array([t.data_ptr() for t in rays], dtype=np.int64), device=ctx.device)
    return rays, table


@pytest.mark.parametrize("n", SIZES)
def test_fvdom_G_against_the_sequential_passes_bitwise(ffm, ctx, n):
    L = ffm.lib()
    for nRay in (1, 8, 32, 33) + ((128,) if n == 257 else ()):
        I, omega = _rays(n, nRay, 1000 * nRay + n)
        rays, table = _ray_table(ctx, I)
        om = ctx.to_device(omega)
        Gb, Gp = _guarded(ctx, n, FILL)
        ctx._ready()
        assert L.ffm_fvdom_G_d(ctx.h, n, nRay, _P(table), _P(om), Gp) == 0
        ctx.sync()
        G = np.zeros(n)
        for i in range(nRay):
            G = G + I[i] * omega[i]
        assert _guards_intact(Gb, n, FILL), (n, nRay)
        assert _inner(Gb, n).tobytes() == G.tobytes(), (n, nRay)


def test_no_cells_and_refused_arguments_write_nothing(ffm, ctx):
    L = ffm.lib()
    n = 65
    G, T, he, Q, Cp = _sh_inputs(n, 7)
    dev = [_P(ctx.to_device(x)) for x in (G, T, he, Q, Cp)]
    (sub, sup), (spb, spp) = _guarded(ctx, n, FILL), _guarded(ctx, n, FILL)
    I, omega = _rays(n, 8, 8)
    rays, table = _ray_table(ctx, I)
    om = ctx.to_device(omega)
    Gb, Gp = _guarded(ctx, n, FILL)
    ctx._ready()
    sh = lambda c, m, g, t, h, q, su, sp: L.ffm_radiation_sh_d(c, m, 0.1, SIGMA, 0.3, g, t, h, q, dev[4], CP_CONST, su, sp)
    ok = (ctx.h, n, dev[0], dev[1], dev[2], dev[3], sup, spp)
    assert sh(*((ctx.h, 0) + ok[2:])) == 0                            # n == 0: a no-op
    for k in (0, 2, 3, 4, 5, 6, 7):
        assert sh(*[None if j == k else v for j, v in enumerate(ok)]) == ERR_ARG, k
    assert sh(*((ctx.h, -1) + ok[2:])) == ERR_ARG
    g_ok = (ctx.h, n, 8, _P(table), _P(om), Gp)
    assert L.ffm_fvdom_G_d(ctx.h, 0, 8, _P(table), _P(om), Gp) == 0
    for k in (0, 3, 4, 5):
        assert L.ffm_fvdom_G_d(*[None if j == k else v for j, v in enumerate(g_ok)]) == ERR_ARG, k
    assert L.ffm_fvdom_G_d(ctx.h, -1, 8, _P(table), _P(om), Gp) == ERR_ARG
    assert L.ffm_fvdom_G_d(ctx.h, n, 0, _P(table), _P(om), Gp) == ERR_ARG
    assert L.ffm_fvdom_G_d(ctx.h, n, -3, _P(table), _P(om), Gp) == ERR_ARG
    ctx.sync()
    for b in (sub, spb, Gb):
        assert np.all(b.cpu().numpy() == FILL)
