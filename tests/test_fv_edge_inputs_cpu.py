"""The designed inputs of the limiter edge tests (tests/fv_edge_inputs.py) do, on the oracle alone, what they were designed for -- on
every mesh and parameter set that tests/test_fv_limiter_edges_gpu.py runs through the kernels:

  (a) gradf and gradcf of the float restatement ARE the exact values (fractions.Fraction) on every face: nothing is rounded before
      the division of NVDTVD::r, which is what makes a bitwise comparison of a kernel with the restatement legitimate whatever order
      (or contraction) the kernel's dot product has;
  (b) the restatement takes the branch the exact computation takes on every face, and its limiter and weight stay within a derived
      bound of the exact ones;
  (c) oracle.fv.limited_limiter / limited_weights equal the restatement bitwise on these inputs;
  (d) every class of face (fv_edge_inputs.CLASSES) is reached on every mesh: >= 3 on the hex box, >= 1 on each merged mesh.

The same for the inputs of filteredLinear2V and of the tiled multivariate weights."""
from fractions import Fraction

import numpy as np
import pytest

import fv_edge_inputs as E
from oracle import fv

U_ = Fraction(1, 2 ** 53)


@pytest.fixture(scope="module", params=E.MESHES)
def case(request):
    name = request.param
    m = E.host_mesh(name)
    return name, m, E.fields(m, name)


def test_meshes_are_dyadic_and_claim_their_buckets(case):
    name, m, f = case
    assert E.MM.bucket(max(E.MM.widths(m.l, m.u))) == E.BUCKET[name]
    assert np.array_equal(np.rint(m.C * 32.0) / 32.0, m.C)
    assert set(np.unique(f["vf"])) <= set(E.VALUES) and set(np.unique(f["grad"])) <= set(E.GRADS)
    assert np.array_equal(np.rint(f["vf"] * 64.0) / 64.0, f["vf"])


@pytest.mark.parametrize("k,lo,hi", E.PARAMS)
def test_restatement_is_exact_before_the_division_and_bounded_after_it(case, k, lo, hi):
    """(a), (b), (c).  The bound of (b), with u = 2^-53 and starred values exact: the operands of the division are exact (a), so
    q = q*(1 + e1); 2q is exact and r = (2q - 1)(1 + e2) = r* + 2 q* e1 + r* e2 + O(u^2), |r - r*| <= u (2|q*| + |r*|)(1 + u);
    t = twoByk r (1 + e3), |t - t*| <= twoByk u (2|q*| + |r*|)(1 + u) + |t*| u <= 2 u twoByk (2|q*| + |r*|); on the large-ratio branch r is
    an integer and only e3 remains (q* := 0 there).  The clamp and the bound test are 1-Lipschitz or exact:
        |limiter - limiter*| <= 4 u (twoByk (2|q*| + |r*|) + 1)
    with a factor 2 to spare.  weight = limiter w + (1 - limiter) pos0 has slope w - pos0 in [-1, 1] and three roundings (the product,
    1 - limiter, the sum; the product with pos0 in {0, 1} is exact) of results in [0, 1]: |weight - weight*| <= the above + 4 u."""
    name, m, f = case
    tk = Fraction(E.two_by_k(k))
    for i in range(E.NF):
        for sch in (2, 3):
            a = E.restate_parts(m, sch, f["phi"], f["vf"][i], f["grad"][i], k, (lo, hi))
            x = E.exact(m, sch, f["phi"], f["vf"][i], f["grad"][i], k, (lo, hi))
            # (a)
            assert all(Fraction(float(v)) == w for v, w in zip(a["gradf"], x["gradf"])), (name, i, "gradf")
            assert all(Fraction(float(v)) == w for v, w in zip(a["gradcf"], x["gradcf"])), (name, i, "gradcf")
            # (b): the same branch and the same classes
            assert np.array_equal(a["big"], x["big"])
            for c in E.RATIO_CLASSES + E.LIMITER_CLASSES + E.BOUND_CLASSES:
                assert np.array_equal(a["classes"][c], x["classes"][c]), (name, i, sch, c)
            qs = np.where(x["big"], Fraction(0), x["q"])
            bound = 4 * U_ * (tk * (2 * np.abs(qs) + np.abs(x["r"])) + 1)
            el = np.abs(E.frac(a["lim"]) - x["lim"]); ew = np.abs(E.frac(a["w"]) - x["w"])
            assert np.all((el <= bound).astype(bool)), (name, i, sch)
            assert np.all((ew <= bound + 4 * U_).astype(bool)), (name, i, sch)
            # (c)
            sname = E.SCHEME_NAME[sch]
            assert np.array_equal(fv.limited_limiter(m, sname, f["phi"], f["vf"][i], f["grad"][i], k, (lo, hi)), a["lim"])
            assert np.array_equal(fv.limited_weights(m, sname, f["phi"], f["vf"][i], f["grad"][i], k, (lo, hi)), a["w"])
            assert a["lim"].min() >= 0.0 and a["lim"].max() <= 1.0 and a["w"].min() >= 0.0 and a["w"].max() <= 1.0


@pytest.mark.parametrize("k,lo,hi", E.PARAMS)
def test_every_class_is_reached(case, k, lo, hi):
    """(d): conditions on the inputs, counted on the exact computation (which (b) shows the restatement to share)"""
    name, m, f = case
    cnt = E.class_counts(m, name, k, lo, hi, parts=E.exact)
    assert cnt == E.class_counts(m, name, k, lo, hi)
    print("\n%s k=%g [%g, %g]: " % (name, k, lo, hi) + ", ".join("%s: %d" % (c, cnt[c]) for c in E.CLASSES))
    need = 3 if name == "hex" else 1
    missing = [(c, cnt[c]) for c in E.required(k) if cnt[c] < need]
    assert not missing, missing
    # a face the bound test must leave alone at zero flux keeps its limiter; one it fires on is upwind
    for i in range(E.NF):
        a = E.restate_parts(m, 3, f["phi"], f["vf"][i], f["grad"][i], k, (lo, hi))
        c = a["classes"]
        assert np.all(a["lim"][c["flux0 out of bounds"]] > 0.0)
        for keep in ("flux>0 P==lo", "flux>0 N==hi", "flux<0 N==lo", "flux<0 P==hi"):
            other = {"flux>0 P==lo": "flux>0 N>hi", "flux>0 N==hi": "flux>0 P<lo", "flux<0 N==lo": "flux<0 P>hi", "flux<0 P==hi": "flux<0 N<lo"}[keep]
            assert np.all(a["lim"][c[keep] & ~c[other]] > 0.0)
        for fire in ("flux>0 P<lo", "flux>0 N>hi", "flux<0 N<lo", "flux<0 P>hi"):
            assert np.all(a["lim"][c[fire]] == 0.0)


def test_the_ghost_block_cut_faces_carry_every_flux_class():
    """the block of tests/test_fv_limiter_edges_gpu.py: the last z-plane of the hex box as ghost cells.  Every flux class sits on a cut
    face, and some cut face with a non-positive flux (its upwind cell is the ghost cell: the ghostUp branch of k_mv_weights) has a common
    limiter above 0, for one field and for one of the sets of several fields the GPU module passes"""
    m = E.host_mesh("hex")
    f = E.fields(m, "hex")
    nOwn, nGhost, keep, cut = E.ghost_block(m)
    assert nOwn + nGhost == m.nCells and cut.sum() == m.n[0] * m.n[1] and not (m.l[keep] >= nOwn).any()
    fc = E.flux_classes(f["phi"])
    cnt = {c: int((fc[c] & cut).sum()) for c in E.FLUX_CLASSES}
    print("\ncut faces: ", cnt)
    assert min(cnt.values()) >= 1
    for k, lo, hi in E.PARAMS:
        _, lims = E.common_limiter(m, E.MV_SCHEMES, f["phi"], f["vf"], f["grad"], k, (lo, hi))
        ghost_up = cut & ~(f["phi"] > 0)
        n = [int((ghost_up & (lims[idx].min(axis=0) > 0)).sum()) for idx in ([0], [0, 1], [4, 5], list(range(E.NF)))]
        print("k=%g: cut faces with a ghost upwind cell and a positive common limiter, for 1, 2, 2 and 6 fields: %s" % (k, n))
        assert n[0] >= 1 and max(n[1:]) >= 1 and (cut & (f["phi"] > 0)).any()


def test_filteredLinear2V_inputs_reach_their_classes(case):
    """fl2v_parts is oracle.fv.filtered_linear2V_weights with its intermediates (bitwise the same weights); every class of
    FL2V_CLASSES is reached on every mesh -- the unclamped limiter exactly 0 only at the dyadic (k, l), where the planted faces land on
    1 and on 0 -- and df, tcP, tcN are exact (Fraction)"""
    name, m, _ = case
    f = E.fl2v_fields(m, name)
    assert np.array_equal(np.unique(f["phi"][f["phi"] != 0]), np.unique(E.FLUXES[E.FLUXES != 0]))
    C_, U, G = E.frac(m.C), E.frac(f["U"]), E.frac(f["gradU"])
    gV, d = U[m.u] - U[m.l], C_[m.u] - C_[m.l]
    df = (gV * gV).sum(axis=1)
    tc = [2 * sum(gV[:, j] * sum(d[:, i] * G[c, i, j] for i in range(3)) for j in range(3)) for c in (m.l, m.u)]
    for k, l in E.FL2V_PARAMS:
        p = E.fl2v_parts(m, f["phi"], f["U"], f["gradU"], k, l)
        assert np.array_equal(p["w"].view(np.uint64), fv.filtered_linear2V_weights(m, f["phi"], f["U"], f["gradU"], k, l).view(np.uint64))
        for got, want in ((p["df"], df), (p["tcP"], tc[0]), (p["tcN"], tc[1])):
            assert all(Fraction(float(a)) == b for a, b in zip(got, want))
        cnt = {c: int(v.sum()) for c, v in p["classes"].items()}
        print("\n%s k=%g l=%g: " % (name, k, l) + ", ".join("%s: %d" % (c, cnt[c]) for c in E.FL2V_CLASSES))
        dyadic = (k, l) == E.FL2V_PARAMS[0]
        assert not [c for c in E.FL2V_CLASSES if cnt[c] < 1 and (dyadic or c != "limiter==0 unclamped")]
        if dyadic:
            assert list(p["raw"][f["planted"]]) == [1.0, 0.0]
        # a uniform vector: the denominator is SMALL alone, the limiter clamps to 1 and the weights are the linear ones
        u0 = p["classes"]["df==0"]
        assert np.all(p["lim"][u0] == 1.0) and np.array_equal(p["w"][u0], m.weights[u0])


@pytest.mark.parametrize("n,nf", E.TILED_BOXES)
def test_tiled_fields_reach_the_classes_through_their_own_gradient(n, nf):
    """the tiled kernel forms its gradients itself, so the classes come from the planted cell values: oracle.fv.grad of them is exact
    (against integer arithmetic on every cell and against Fraction on every 97th), and on that gradient every class is reached for every
    parameter set; on every 37th face the Fraction computation takes the restatement's branches and has its gradf and gradcf"""
    from types import SimpleNamespace
    from oracle import plume
    m = plume.make_mesh(n, h=E.H)
    f = E.tiled_fields(m, nf)
    g = np.array([fv.grad(m, f["vf"][i], f["vb"][i]) for i in range(nf)])
    cells = np.arange(0, m.nCells, 97)
    for i in range(nf):
        assert np.array_equal(g[i] * 16.0, E.grad_exact_int(m, f["vf"][i], f["vb"][i]).astype(float)), i
        # Fraction: V grad = sum Sf vf_face over the faces of the sampled cells
        acc = {int(c): [Fraction(0)] * 3 for c in cells}
        F_ = lambda x: Fraction(float(x))
        for sel, sign, other in ((np.isin(m.l, cells), 1, m.l), (np.isin(m.u, cells), -1, m.u)):
            for fc in np.nonzero(sel)[0]:
                ff = F_(m.weights[fc]) * F_(f["vf"][i][m.l[fc]]) + (1 - F_(m.weights[fc])) * F_(f["vf"][i][m.u[fc]])
                a = acc[int(other[fc])]
                for dd in range(3):
                    a[dd] = a[dd] + sign * F_(m.Sf[fc, dd]) * ff
        for p, b in zip(m.patches, f["vb"][i]):
            for q in np.nonzero(np.isin(p.faceCells, cells))[0]:
                a = acc[int(p.faceCells[q])]
                for dd in range(3):
                    a[dd] = a[dd] + F_(p.Sf[q, dd]) * F_(b[q])
        for c in cells:
            assert [F_(x) for x in g[i][c]] == [a / F_(m.V[c]) for a in acc[int(c)]], (i, c)
    fcl = E.flux_classes(f["phi"])
    sub = np.arange(0, m.nFaces, 37)
    ms = SimpleNamespace(l=m.l[sub], u=m.u[sub], C=m.C, weights=m.weights[sub])
    for k, lo, hi in E.PARAMS:
        cnt = {c: int(v.sum()) for c, v in fcl.items()}
        lims = []
        for i in range(nf):
            p = E.restate_parts(m, 3, f["phi"], f["vf"][i], g[i], k, (lo, hi))
            for c in E.RATIO_CLASSES + E.LIMITER_CLASSES + E.BOUND_CLASSES:
                cnt[c] = cnt.get(c, 0) + int(p["classes"][c].sum())
            lims.append(p["lim"] if E.MV_SCHEMES[i] == 3 else E.restate(m, 2, f["phi"], f["vf"][i], g[i], k, (lo, hi))[0])
        cnt.update({c: int(v.sum()) for c, v in E.mv_classes(np.array(lims)).items()})
        print("\n%s k=%g [%g, %g]: " % (n, k, lo, hi) + ", ".join("%s: %d" % (c, cnt[c]) for c in E.CLASSES))
        assert not [(c, cnt[c]) for c in E.required(k) if cnt[c] < 3]
    k, lo, hi = E.PARAMS[0]
    for i in (0, nf - 1):
        a = E.restate_parts(ms, 3, f["phi"][sub], f["vf"][i], g[i], k, (lo, hi))
        x = E.exact(ms, 3, f["phi"][sub], f["vf"][i], g[i], k, (lo, hi))
        assert all(Fraction(float(v)) == w for v, w in zip(a["gradf"], x["gradf"]))
        assert all(Fraction(float(v)) == w for v, w in zip(a["gradcf"], x["gradcf"]))
        for c in E.RATIO_CLASSES + E.LIMITER_CLASSES + E.BOUND_CLASSES:
            assert np.array_equal(a["classes"][c], x["classes"][c]), (i, c)
