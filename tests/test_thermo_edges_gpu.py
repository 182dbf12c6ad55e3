"""csrc/ffm_thermo.hip at its range edges, against oracle/thermo.py and the numpy formulas of tests/test_thermo_gpu.py: a synthetic
table whose species differ in Tlow, Thigh, As and Ts (on the golden table all are equal, and any mixing of equal numbers passes);
1, 2 and 8 species and the refusal of 9; cells whose leading species are absent; enthalpies outside [Hs(Tlow), Hs(Thigh)]; T exactly
Tcommon; launches of 0, 1, 255, 256, 257 cells and of more cells than one pass of the grid covers (2048 blocks of 256: 524288); a NaN
enthalpy, which has to come out as NaN; the failure return of the Newton iteration; EDC with the diffusion branch and k = 0.  Inputs:
tests/physics_edge_inputs.py, whose edges tests/test_physics_edge_inputs_cpu.py checks on the oracle.  Tolerance 1e-13 relative, as
tests/test_thermo_gpu.py; what is built from + - * / alone (Cp, he, the limits of T, nut) is bitwise."""
import ctypes as C

import numpy as np
import pytest

import physics_edge_inputs as E

pytestmark = pytest.mark.gpu

GRID_PASS = 2048 * 256          # cells one pass of the grid-stride loop covers
GUARD = 64


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def syn(ffm, ctx):
    """thermo handles and oracle species of the synthetic tables of 1, 2 and 8 species"""
    from oracle import thermo as TH
    out = {}
    for n in (1, 2, 8):
        names, tab = E.synthetic_table(n)
        out[n] = (ffm.Thermo(ctx, names, tab, TH.RR), TH.Species(names, tab))
    yield out
    for th, _ in out.values():
        th.close()


def _check_all(ctx, th, sp, Y, he, T0, what):
    """correct() from the start temperatures T0, then he, Cp and properties at the result, against the oracle"""
    n = Y.shape[1]
    D = lambda a: ctx.to_device(np.ascontiguousarray(a, np.float64))
    mx = sp.mixture(Y)
    Tr = mx.THs(he, 0.0, T0 * np.ones(n))
    Yd = [D(y) for y in Y]
    Td, psi, mu, al = D(T0 * np.ones(n)), ctx.empty(n), ctx.empty(n), ctx.empty(n)
    th.correct(Yd, D(he), None, Td, psi, mu, al)
    T = Td.cpu().numpy()
    errs = dict(T=_rel(T, Tr), psi=_rel(psi.cpu().numpy(), mx.psi(0.0, Tr)), mu=_rel(mu.cpu().numpy(), mx.mu(0.0, Tr)),
                alpha=_rel(al.cpu().numpy(), mx.alphah(0.0, Tr)))
    print(what, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert max(errs.values()) < 1e-13, (what, errs)
    # at the oracle's temperature: he and Cp are polynomials (bitwise), properties has one sqrt
    Trd, out = D(Tr), ctx.empty(n)
    th.he(Yd, Trd, out)
    assert _rel(out.cpu().numpy(), mx.Hs(0.0, Tr)) < 1e-13, what
    th.Cp(Yd, Trd, out)
    assert _rel(out.cpu().numpy(), mx.Cp(0.0, Tr)) < 1e-13, what
    p2, m2, a2 = ctx.empty(n), ctx.empty(n), ctx.empty(n)
    th.properties(Yd, Trd, p2, m2, a2)
    assert _rel(p2.cpu().numpy(), mx.psi(0.0, Tr)) < 1e-13 and _rel(m2.cpu().numpy(), mx.mu(0.0, Tr)) < 1e-13, what
    assert _rel(a2.cpu().numpy(), mx.alphah(0.0, Tr)) < 1e-13, what
    return T, Tr, mx


@pytest.mark.parametrize("nSp", [1, 2, 8])
def test_species_counts_and_absent_leading_species(ctx, syn, nSp):
    th, sp = syn[nSp]
    n = 300
    Y = E.compositions(nSp, n, seed=5)
    Tt = E.hashed(3, n, 300.0, 2500.0)
    he = sp.mixture(Y).Hs(0.0, Tt)
    T, Tr, mx = _check_all(ctx, th, sp, Y, he, Tt * (1.0 + 0.08 * np.cos(11.0 * np.arange(n))), "nSp=%d" % nSp)
    assert np.abs(Tr - Tt).max() < 0.3
    # the cells without the first, the first two, all but the last species on their own: the maximum over 300 cells must not hide them
    for c in range(3):
        assert abs(T[c] - Tr[c]) <= 1e-13 * abs(Tr[c]), (nSp, c)
    # nullable outputs
    D = lambda a: ctx.to_device(np.ascontiguousarray(a, np.float64))
    Td, mu = D(Tt), ctx.empty(n)
    th.correct([D(y) for y in Y], D(he), None, Td, None, mu, None)
    assert _rel(Td.cpu().numpy(), mx.THs(he, 0.0, Tt)) < 1e-13 and _rel(mu.cpu().numpy(), mx.mu(0.0, mx.THs(he, 0.0, Tt))) < 1e-13


def test_nine_species_are_refused(ffm, ctx):
    from oracle import thermo as TH
    names, tab = E.synthetic_table(9)
    col = lambda k: np.ascontiguousarray([float(tab[s][k]) for s in names], np.float64)
    hi = np.ascontiguousarray([tab[s]["high"] for s in names]); lo = np.ascontiguousarray([tab[s]["low"] for s in names])
    hp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    h = C.c_void_p()
    keep = [col(k) for k in ("W", "Tlow", "Thigh", "Tcommon")] + [hi, lo, col("As"), col("Ts")]
    assert ffm.lib().ffm_thermo_create(ctx.h, 9, *[hp(a) for a in keep], float(TH.RR), C.byref(h)) == -1      # FFM_ERR_ARG
    assert not h.value and b"at most 8 species" in ffm.lib().ffm_last_error()
    with pytest.raises(ffm.FfmError, match="at most 8 species"):
        ffm.Thermo(ctx, names, tab, TH.RR)


@pytest.mark.parametrize("T0", [250.0, 3000.0, 5900.0])
@pytest.mark.parametrize("nSp", [1, 8])
def test_range_edges_and_start_temperatures(ctx, syn, nSp, T0):
    """he below Hs(Tlow) / above Hs(Thigh) of the cell's mixture: the iterate sits on the limit, T comes out as that limit bit for bit;
    he = Hs(Tcommon); start temperatures below the range, far from the answer and above the range"""
    th, sp = syn[nSp]
    n = 300
    Y = E.compositions(nSp, n, seed=5)
    mx = sp.mixture(Y)
    Tt = E.hashed(3, n, 300.0, 2500.0)
    he = mx.Hs(0.0, Tt)
    he[0::3] = mx.Hs(0.0, mx.Tlow * np.ones(n))[0::3] - 1.0e5
    he[1::3] = mx.Hs(0.0, mx.Thigh * np.ones(n))[1::3] + 1.0e5
    he[5::15] = mx.Hs(0.0, np.full(n, 1000.0))[5::15]
    T, Tr, _ = _check_all(ctx, th, sp, Y, he, T0, "edges nSp=%d T0=%g" % (nSp, T0))
    assert np.array_equal(T[0::3], (mx.Tlow * np.ones(n))[0::3]) and np.array_equal(T[1::3], (mx.Thigh * np.ones(n))[1::3])
    assert np.abs(T[5::15] - 1000.0).max() < 1e-3
    if nSp == 8:            # the limits are the mixture's, and they differ from cell to cell and from species 0's
        assert len(np.unique(mx.Tlow)) > 1 and mx.Tlow.max() > E.SYN_TLOW[0] and mx.Thigh.min() < E.SYN_THIGH[0]


@pytest.mark.parametrize("nSp", [1, 8])
def test_T_exactly_Tcommon_takes_the_high_coefficients(ctx, syn, nSp):
    th, sp = syn[nSp]
    n = 64
    Y = E.compositions(nSp, n, seed=9)
    mx = sp.mixture(Y)
    Tc = np.full(n, 1000.0); Tc[1::2] = np.nextafter(1000.0, 0.0)          # odd cells just below: the low set
    D = lambda a: ctx.to_device(np.ascontiguousarray(a, np.float64))
    Yd, Td, out = [D(y) for y in Y], D(Tc), ctx.empty(n)
    th.he(Yd, Td, out)
    assert np.array_equal(out.cpu().numpy(), mx.Hs(0.0, Tc))
    th.Cp(Yd, Td, out)
    cp = out.cpu().numpy()
    assert np.array_equal(cp, mx.Cp(0.0, Tc))
    a = mx.high                                                             # Cp of the high set, written out
    assert np.array_equal(cp[0::2], (((((a[:, 4] * 1000.0 + a[:, 3]) * 1000.0 + a[:, 2]) * 1000.0 + a[:, 1]) * 1000.0 + a[:, 0]))[0::2])
    psi, mu, al = ctx.empty(n), ctx.empty(n), ctx.empty(n)
    th.properties(Yd, Td, psi, mu, al)
    assert _rel(psi.cpu().numpy(), mx.psi(0.0, Tc)) < 1e-13 and _rel(mu.cpu().numpy(), mx.mu(0.0, Tc)) < 1e-13
    assert _rel(al.cpu().numpy(), mx.alphah(0.0, Tc)) < 1e-13
    # properties with null outputs writes only what it is given
    al2 = D(np.full(n, -7.0))
    th.properties(Yd, Td, None, None, al2)
    assert np.array_equal(al2.cpu().numpy(), al.cpu().numpy())


def _guarded(ctx, n, fill):
    """a buffer of n values between two guards of GUARD values; returns (buffer, pointer to the n values)"""
    buf = ctx.to_device(np.full(n + 2 * GUARD, fill))
    return buf, C.c_void_p(buf.data_ptr() + 8 * GUARD)


def _guards_intact(buf, n, fill):
    a = buf.cpu().numpy()
    return np.all(a[:GUARD] == fill) and np.all(a[GUARD + n:] == fill)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, GRID_PASS + 3])
def test_launch_sizes_of_correct(ffm, ctx, syn, n):
    """n = 0 returns OK and writes nothing; above 524288 cells the grid-stride loop goes round twice"""
    th, sp = syn[8]
    L = ffm.lib()
    D = lambda a: ctx.to_device(np.ascontiguousarray(a, np.float64))
    m = max(n, 1)
    Y = E.compositions(8, m, seed=21)
    Tt = E.hashed(22, m, 300.0, 2500.0)
    mx = sp.mixture(Y)
    he = mx.Hs(0.0, Tt)
    T0 = Tt * (1.0 + 0.05 * (E.hashed(23, m) - 0.5))
    if n > GRID_PASS:
        i = np.arange(n - GRID_PASS)
        assert np.all(he[i] != he[i + GRID_PASS]) and np.all(T0[i] != T0[i + GRID_PASS]) and np.all((Y[:, i] != Y[:, i + GRID_PASS]).any(axis=0))
    Yd, hed = [D(y) for y in Y], D(he)
    Yp = (C.c_void_p * 8)(*[y.data_ptr() for y in Yd])
    FILL = -12345.0
    bufs = [_guarded(ctx, n, FILL) for _ in range(4)]
    (Tb, Tp), (pb, pp), (mb, mp), (ab, ap) = bufs
    if n:
        Tb[GUARD:GUARD + n] = D(T0[:n])
    ctx._ready()
    assert L.ffm_thermo_correct_d(th.h, n, Yp, _P(hed), None, Tp, pp, mp, ap) == 0
    ctx.sync()
    for b, _ in bufs:
        assert _guards_intact(b, n, FILL)
    if n == 0:
        assert all(np.all(b.cpu().numpy() == FILL) for b, _ in bufs)
        for fn, args in ((L.ffm_thermo_he_d, (Tp, pp)), (L.ffm_thermo_Cp_d, (Tp, pp)), (L.ffm_thermo_properties_d, (Tp, pp, mp, ap))):
            assert fn(th.h, 0, Yp, *args) == 0
        ctx.sync()
        assert all(np.all(b.cpu().numpy() == FILL) for b, _ in bufs)
        return
    mxn = sp.mixture(Y[:, :n])
    Tr = mxn.THs(he[:n], 0.0, T0[:n])
    got = [b.cpu().numpy()[GUARD:GUARD + n] for b, _ in bufs]
    for name, g, r in zip(("T", "psi", "mu", "alpha"), got, (Tr, mxn.psi(0.0, Tr), mxn.mu(0.0, Tr), mxn.alphah(0.0, Tr))):
        assert _rel(g, r) < 1e-13, (n, name)
        assert _rel(g[-3:], r[-3:]) < 1e-13, (n, name)              # the last cells (the second round of the large launch) on their own
    # he, Cp, properties at the same sizes
    Trd = D(Tr)
    for fn, r in ((L.ffm_thermo_he_d, mxn.Hs(0.0, Tr)), (L.ffm_thermo_Cp_d, mxn.Cp(0.0, Tr))):
        ob, op = _guarded(ctx, n, FILL)
        ctx._ready()
        assert fn(th.h, n, Yp, _P(Trd), op) == 0
        ctx.sync()
        assert _guards_intact(ob, n, FILL) and np.array_equal(ob.cpu().numpy()[GUARD:GUARD + n], r), n
    ob, op = _guarded(ctx, n, FILL)
    ctx._ready()
    assert L.ffm_thermo_properties_d(th.h, n, Yp, _P(Trd), None, op, None) == 0
    ctx.sync()
    assert _guards_intact(ob, n, FILL) and _rel(ob.cpu().numpy()[GUARD:GUARD + n], mxn.mu(0.0, Tr)) < 1e-13


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, GRID_PASS + 3])
def test_edc_and_nut_branches_and_launch_sizes(ffm, ctx, n):
    """C_Diff > 0: the diffusion branch of rt = max(rtTurb, rtDiff) wins in some cells and the turbulent one in others; k = 0 (the
    max(k, SMALL) guard); fuel- and oxygen-limited cells; Qdot and alphat null"""
    L, c = ffm.lib(), E.EDC
    D = lambda a: ctx.to_device(np.ascontiguousarray(a, np.float64))
    m = max(n, 7)
    f = E.edc_fields(m)
    rho, k, delta, alpha, Yf, Yo = f
    w, rtT, rtD = E.edc_reference(*f)
    if n >= 255:
        s = slice(0, n)
        assert ((rtD[s] > rtT[s]) & (k[s] > 0)).sum() > 0 and (rtT[s] > rtD[s]).sum() > 0 and (k[s] == 0).sum() > 0
        assert ((Yf[s] < Yo[s] / c["s"]) & (Yf[s] > 0)).sum() > 0 and (Yf[s] > Yo[s] / c["s"]).sum() > 0
    if n == 1:
        assert k[0] == 0.0
    if n > GRID_PASS:
        i = np.arange(n - GRID_PASS)
        assert all(np.all(a[i] != a[i + GRID_PASS]) for a in (rho, delta, alpha, Yo))
    fd = [D(a) for a in f]
    FILL = -12345.0
    args = [_P(t) for t in fd] + [c["s"], c["dt"], c["Ce"], c["C_EDC"], c["C_Diff"], c["C_Stiff"], c["qFuel"]]
    (wb, wp), (qb, qp), (w2b, w2p) = [_guarded(ctx, n, FILL) for _ in range(3)]
    ctx._ready()
    assert L.ffm_edc_correct_d(ctx.h, n, *args, wp, qp) == 0
    assert L.ffm_edc_correct_d(ctx.h, n, *args, w2p, None) == 0                # Qdot null
    (nb, np_), (ab, ap), (n2b, n2p) = [_guarded(ctx, n, FILL) for _ in range(3)]
    ctx._ready()
    assert L.ffm_les_keqn_nut_d(ctx.h, n, c["Ck"], c["Prt"], _P(fd[1]), _P(fd[2]), _P(fd[0]), np_, ap) == 0
    assert L.ffm_les_keqn_nut_d(ctx.h, n, c["Ck"], c["Prt"], _P(fd[1]), _P(fd[2]), None, n2p, None) == 0      # alphat (and rho) null
    ctx.sync()
    for b in (wb, qb, w2b, nb, ab, n2b):
        assert _guards_intact(b, n, FILL)
    if n == 0:
        assert all(np.all(b.cpu().numpy() == FILL) for b in (wb, qb, w2b, nb, ab, n2b))
        return
    inner = lambda b: b.cpu().numpy()[GUARD:GUARD + n]
    wr = w[:n]
    scale = max(np.abs(wr).max(), 1e-300)
    assert np.abs(inner(wb) - wr).max() < 1e-13 * scale and np.abs(inner(qb) - c["qFuel"] * wr).max() < 1e-13 * c["qFuel"] * scale
    assert np.array_equal(inner(w2b), inner(wb))
    assert np.all(inner(wb)[Yf[:n] == 0.0] == 0.0) and np.isfinite(inner(wb)).all()
    nr = c["Ck"] * np.sqrt(k[:n]) * delta[:n]
    assert _rel(inner(nb), nr) < 1e-15
    assert np.all(inner(nb)[k[:n] == 0.0] == 0.0)
    assert np.abs(inner(ab) - rho[:n] * nr / c["Prt"]).max() <= 1e-15 * max((rho[:n] * nr / c["Prt"]).max(), 1e-300)
    assert np.array_equal(inner(n2b), inner(nb))


def test_a_nan_enthalpy_comes_out_as_nan_in_that_cell_only(ctx, syn):
    """janafThermo::limit returns T unchanged unless T < Tlow || T > Thigh, so a NaN iterate stays NaN (and so does oracle/thermo.py's
    limit); tests/test_pool_poison_gpu.py relies on NaNs surviving.  A limit written as fmin(fmax(T, Tlow), Thigh) gave T = Tlow with
    finite psi, mu, alpha and status OK: this test failed on that kernel."""
    th, sp = syn[8]
    n = 300
    D = lambda a: ctx.to_device(np.ascontiguousarray(a, np.float64))
    Y = E.compositions(8, n, seed=5)
    Tt = E.hashed(3, n, 300.0, 2500.0)
    he = sp.mixture(Y).Hs(0.0, Tt)
    Yd = [D(y) for y in Y]
    outs = {}
    for tag, h in (("clean", he), ("nan", np.where(np.arange(n) == 7, np.nan, he))):
        Td, psi, mu, al = D(np.full(n, 900.0)), ctx.empty(n), ctx.empty(n), ctx.empty(n)
        th.correct(Yd, D(h), None, Td, psi, mu, al)                             # status OK: no exception
        outs[tag] = [t.cpu().numpy() for t in (Td, psi, mu, al)]
    for name, a, b in zip(("T", "psi", "mu", "alpha"), outs["clean"], outs["nan"]):
        assert np.isnan(b[7]), (name, b[7])
        assert np.array_equal(np.delete(a, 7), np.delete(b, 7)) and np.isfinite(a).all(), name


def test_the_failure_return_and_its_rearming(ffm, ctx, syn):
    """an enthalpy inside a jump of Hs at Tcommon has no temperature: the iteration alternates across Tcommon, is bounded at 102
    iterates and returns an error, as thermo::T's FatalError; the next call on the same handle computes a normal field"""
    from oracle import thermo as TH
    names, tab, hmid, _ = E.jump_table()
    th = ffm.Thermo(ctx, names, tab, TH.RR)
    sp = TH.Species(names, tab)
    n = 300
    D = lambda a: ctx.to_device(np.ascontiguousarray(a, np.float64))
    Y = np.ones((1, n))
    Tt = E.hashed(3, n, 300.0, 900.0)                                           # below the jump
    he = sp.mixture(Y).Hs(0.0, Tt)
    bad = he.copy(); bad[123] = hmid
    Yd = [D(Y[0])]
    with pytest.raises(ffm.FfmError, match="maximum number of iterations exceeded"):
        th.correct(Yd, D(bad), None, D(np.full(n, 900.0)), ctx.empty(n), None, None)
    _check_all(ctx, th, sp, Y, he, 600.0, "after the failure")                  # the flag is re-armed
    th8, sp8 = syn[8]                                                           # and another handle of the context is not affected
    Y8 = E.compositions(8, n, seed=5)
    _check_all(ctx, th8, sp8, Y8, sp8.mixture(Y8).Hs(0.0, E.hashed(3, n, 300.0, 2500.0)), 900.0, "other handle after the failure")
    th.close()
