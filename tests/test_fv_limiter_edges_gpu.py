"""The limited convection schemes on the device at their switch points: the five copies of limitedLinear k / limitedLinear01 k
(k_limited_weights<0/1/2> and k_weights_from_limiter of csrc/ffm_fv.hip; limited_weight() in k_scalar_eqns and k_div_phiK, mv_limiter()
in k_mv_weights and k_mv_tile of csrc/ffm_fused.hip) and filteredLinear2V against the straight-line restatement of the reference's C++
(tests/fv_edge_inputs.py: restate), on designed inputs: zero, signed-zero and denormal fluxes, values exactly on and beyond the bounds,
uniform regions, gradf == 0, |gradcf| == 1000 |gradf| with every sign pair and just below, twoByk r below 0, exactly 0, between,
exactly 1 and above.  tests/test_fv_edge_inputs_cpu.py shows without a GPU that every such class of face is reached on every mesh and
parameter set used here and that the restatement's operands are exact up to the division of NVDTVD::r -- so every comparison here is
of BITS (uint64 views: -0.0 is not +0.0), whatever the order or contraction of a kernel's dot product.

Meshes: the hex box 7 x 6 x 5 (bucket 3 of FFM_DISPATCH_W) and the merged meshes w8, w16u14, w32l30, w32multi, w32u18 (k_mv_weights walks
its second, third and fourth chunk of 8 slots), spacing 1/8; parameter sets (k, lo, hi) = (1, 0, 1), (1/2, 0, 1), (2, 1/4, 3/4), (0, 0, 1)."""
import ctypes as C

import numpy as np
import pytest

import fv_edge_inputs as E
import merged_mesh as MM

pytestmark = pytest.mark.gpu

UNSUPPORTED = r"failed \(-5\)"                 # FFM_ERR_UNSUPPORTED through binding._check
PARAMS = pytest.mark.parametrize("k,lo,hi", E.PARAMS)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def where_not(a, b):
    """for the assertion message: how many entries differ, and the first few (index, got, expected)"""
    bad = np.nonzero(bits(a) != bits(b))[0]
    return len(bad), [(int(i), float(a[i]), float(b[i])) for i in bad[:5]]


class Dev:
    """a mesh on the device with the fields of fv_edge_inputs in both orders.  cmap / fmap: the oracle's cell / face of every device
    cell / LDU face (for one block of a box: the block's cells and faces only)"""

    def __init__(self, ctx, mesh, m, cmap, fmap, f):
        self.ctx, self.mesh, self.m, self.cmap, self.fmap, self.f = ctx, mesh, m, cmap, fmap, f
        self.nf = len(f["vf"])
        self.phi = self.face(f["phi"])
        self.vf = [self.cell(v) for v in f["vf"]]
        self.g = [[self.cell(f["grad"][i][:, d]) for d in range(3)] for i in range(self.nf)] if "grad" in f else None
        self._ref = {}

    def cell(self, a): return self.ctx.to_device(np.asarray(a)[self.cmap])
    def face(self, a): return self.mesh.to_native(np.asarray(a)[self.fmap])
    def back(self, t): return self.mesh.from_native(t)                 # the block's faces in LDU order
    def want(self, a): return np.asarray(a)[self.fmap]
    def nan_faces(self): return self.ctx.zeros(self.mesh.nNative) + float("nan")
    def gcol(self, d, idx): return [self.g[i][d] for i in idx]

    def ref(self, sch, i, k, lo, hi):
        """(limiter, weights) of the restatement for field i on the oracle's whole mesh"""
        key = (sch, i, k, lo, hi)
        if key not in self._ref:
            self._ref[key] = E.restate(self.m, sch, self.f["phi"], self.f["vf"][i], self.f["grad"][i], k, (lo, hi))
        return self._ref[key]

    def common(self, idx, sch, k, lo, hi):
        lim = np.min([self.ref(sch[j], i, k, lo, hi)[0] for j, i in enumerate(idx)], axis=0)
        return lim, E.weights_from_limiter(self.m, self.f["phi"], lim)


@pytest.fixture(scope="module", params=E.MESHES)
def setup(request, O, ffm, ctx):
    name = request.param
    s = MM.device_mesh(ffm, ctx, E.host_mesh(name))
    # the row-width instantiation this mesh claims, from the addressing the library was given
    assert MM.bucket(max(np.bincount(s["l"]).max(), np.bincount(s["u"]).max())) == E.BUCKET[name]
    if name != "hex":
        assert (s["wu"], s["wl"]) == MM.CASES[name][4:6]
    d = Dev(ctx, s["mesh"], s["m"], s["cOrd"], s["fOrd"], E.fields(s["m"], name))
    d.name, d.s = name, s
    yield d
    s["mesh"].close(); s["A"].close()


# ------------------------------------------------------------------------------------------------------ (a) the limiter entry points
def _limited_weights(d, k, lo, hi):
    for sch in (2, 3):
        for i in range(d.nf):
            w = d.nan_faces()
            d.mesh.call("fv_limited_weights", sch, k, lo, hi, d.phi, d.vf[i], *d.g[i], w)
            got, ref = d.back(w), d.want(d.ref(sch, i, k, lo, hi)[1])
            assert same(got, ref), (sch, i, where_not(got, ref))


@PARAMS
def test_limited_weights(setup, k, lo, hi):
    """ffm_fv_limited_weights (k_limited_weights<0>), schemes 2 and 3, every field"""
    _limited_weights(setup, k, lo, hi)


def test_upwind_linear_lust_weights_at_zero_and_denormal_fluxes(setup):
    """schemes 0, 1, 4, 5 on the same fluxes: pos0(+-0) = 1, pos0(-2^-1074) = 0"""
    d, m, phi = setup, setup.m, setup.f["phi"]
    p0 = np.where(phi >= 0, 1.0, 0.0)
    for sch, ref in ((0, p0), (5, p0), (1, m.weights), (4, 0.75 * m.weights + 0.25 * p0)):
        w = d.nan_faces()
        d.mesh.call("fv_limited_weights", sch, 1.0, 0.0, 1.0, d.phi, None, None, None, None, w)
        assert same(d.back(w), d.want(ref)), sch


def _limiters(d, k, lo, hi):
    # plain
    for sch in (2, 3):
        for i in range(d.nf):
            lim = d.nan_faces()
            d.mesh.call("fv_limited_limiter", sch, k, lo, hi, d.phi, d.vf[i], *d.g[i], lim, 0)
            got, ref = d.back(lim), d.want(d.ref(sch, i, k, lo, hi)[0])
            assert same(got, ref), (sch, i, where_not(got, ref))
    # the running minimum over 2 and 6 fields with mixed schemes, and the weights made of it
    for idx in ([0, 1], list(range(d.nf))):
        sch = [E.MV_SCHEMES[i] for i in idx]
        lim, w = d.nan_faces(), d.nan_faces()
        for j, i in enumerate(idx):
            d.mesh.call("fv_limited_limiter", sch[j], k, lo, hi, d.phi, d.vf[i], *d.g[i], lim, 0 if j == 0 else 1)
        d.mesh.call("fv_weights_from_limiter", d.phi, lim, w)
        rl, rw = d.common(idx, sch, k, lo, hi)
        assert same(d.back(lim), d.want(rl)), (len(idx), where_not(d.back(lim), d.want(rl)))
        assert same(d.back(w), d.want(rw)), (len(idx), where_not(d.back(w), d.want(rw)))


@PARAMS
def test_limited_limiter_plain_and_running_minimum(setup, k, lo, hi):
    """ffm_fv_limited_limiter (k_limited_weights<1>, <2>) and ffm_fv_weights_from_limiter"""
    _limiters(setup, k, lo, hi)


# ---------------------------------------------------------------------------------------------- (b) ffm_fv_multivariate_weights
def _multivariate(d, k, lo, hi):
    for idx in ([0], [0, 1], [4, 5], list(range(d.nf))):
        nf = len(idx)
        sch = [E.MV_SCHEMES[i] for i in idx]
        w = d.nan_faces()                      # a face that no cell claims keeps its NaN
        d.mesh.call("fv_multivariate_weights", nf, (C.c_int * nf)(*sch), k, lo, hi, d.phi, [d.vf[i] for i in idx],
                    d.gcol(0, idx), d.gcol(1, idx), d.gcol(2, idx), w)
        got, ref = d.back(w), d.want(d.common(idx, sch, k, lo, hi)[1])
        assert not np.isnan(got).any(), (idx, np.nonzero(np.isnan(got))[0][:8])
        assert same(got, ref), (idx, where_not(got, ref))


@PARAMS
def test_multivariate_weights(setup, k, lo, hi):
    """k_mv_weights: every face written once, by its upwind cell (zero, signed-zero and denormal fluxes included), with the blend of
    the face-wise minimum of the restatement's limiters; nf = 1, 2, 6"""
    _multivariate(setup, k, lo, hi)


# ------------------------------------------------------------------- (c) the limiter inside the fused assembly and inside div(phi, K)
GAMMAS = [0.0, 0.25, 0.5, 1.0, 2.0]


def _transport_coefficients(d, O, k, lo, hi, N, B):
    """upper and lower of ffm_fvm_scalar_transport_multi.  N: entries of a cell field, B: boundary faces"""
    ctx, m = d.ctx, d.m
    dev = ctx.to_device
    h = lambda seed, n, a=0.0, b=1.0: dev(a + (b - a) * O.hash_u(seed, np.arange(n)))
    gam = E.dyadic_face_field(m, d.name, 5, GAMMAS)
    G = np.multiply(np.multiply(gam, m.magSf), m.deltaCoeffs)
    phi = d.f["phi"]
    rho, rho0, phib, gamb = h(60, N, 1.0, 2.0), h(61, N, 1.0, 2.0), h(70, B, -0.1, 0.1), h(64, B, 0.01, 0.02)
    gamd = d.face(gam)
    for sch in (2, 3):
        for idx in ([0, 1, 2, 3], [2, 3, 4, 5], [0], [4], [5]):
            nf = len(idx)
            vf0, f, ref, rg = ([h(s + i, n) for i in range(nf)] for s, n in ((62, N), (80, B), (84, B), (88, B)))
            f = [(x * 2).round() / 2 for x in f]
            D, S = [ctx.zeros(N) for _ in idx], [ctx.zeros(N) for _ in idx]
            Up, Lo = [d.nan_faces() for _ in idx], [d.nan_faces() for _ in idx]
            none = [None] * nf
            d.mesh.call("fvm_scalar_transport_multi", nf, sch, k, lo, hi, 1000.0, rho, rho0, d.phi, phib, gamd, gamb,
                        [d.vf[i] for i in idx], d.gcol(0, idx), d.gcol(1, idx), d.gcol(2, idx), vf0, f, ref, rg, none, none, none, None, D, Up, Lo, S)
            for j, i in enumerate(idx):
                w = d.ref(sch, i, k, lo, hi)[1]
                lo0 = np.multiply(np.negative(w), phi)
                rl, ru = d.want(np.subtract(lo0, G)), d.want(np.subtract(np.add(lo0, phi), G))
                gl, gu = d.back(Lo[j]), d.back(Up[j])
                assert same(gl, rl), (sch, idx, i, "lower", where_not(gl, rl))
                assert same(gu, ru), (sch, idx, i, "upper", where_not(gu, ru))


@PARAMS
def test_scalar_transport_multi_coefficients(setup, O, k, lo, hi):
    """limited_weight() in k_scalar_eqns: upper = (-w phi + phi) - Gamma, lower = -w phi - Gamma with w of the restatement and
    Gamma = gamma magSf deltaCoeffs of a dyadic gamma (0 included: the sign of a zero coefficient is compared too), one rounded operation
    each as in the kernel; nf = 1 and 4"""
    d = setup
    _transport_coefficients(d, O, k, lo, hi, d.s["N"], d.s["B"])


@PARAMS
@pytest.mark.parametrize("sch", [2, 3])
def test_div_phiK(setup, O, ffm, k, lo, hi, sch):
    """limited_weight() in k_div_phiK: divK against the face sum of phi (w K_P + (1 - w) K_N) with w of the restatement, summed by
    oracle.fv.surface_integrate on the mesh in the library's numbering.  BITWISE, although the row sums are not exact on these inputs (a
    product with a denormal flux is rounded): every term is formed by the kernel's own operations from a bit-equal weight, and a row's
    terms are added in the kernel's order -- the faces where the cell is the neighbour, those it owns, its boundary faces, each in face
    order -- so both sides round alike; nothing is left to a tolerance.  Rows wider than 8 are refused."""
    d, m, mesh, ctx = setup, setup.m, setup.mesh, setup.ctx
    N, B = d.s["N"], d.s["B"]
    dev = ctx.to_device
    h = lambda seed, n, a=0.0, b=1.0: dev(a + (b - a) * O.hash_u(seed, np.arange(n)))
    Kb, phib = E.boundary_field(m, d.name, 300, E.VALUES), E.boundary_field(m, d.name, 320, [0.0, -0.0, 0.25, -0.25, 0.5])
    i = 0
    out = [ctx.zeros(N) + float("nan") for _ in range(3)]
    args = (sch, k, lo, hi, 1000.0, d.phi, dev(np.concatenate(phib)), d.vf[i], dev(np.concatenate(Kb)), *d.g[i],
            h(60, N, 1.0, 2.0), h(61, N, 1.0, 2.0), h(62, N), h(63, N, -50.0, 50.0), *out)
    if E.BUCKET[d.name] > 8:
        with pytest.raises(ffm.FfmError, match=UNSUPPORTED):
            mesh.call("fvc_div_phiK_terms", *args)
        assert all(np.isnan(o.cpu().numpy()).all() for o in out)
        return
    mesh.call("fvc_div_phiK_terms", *args)
    from oracle import fv
    K, phi = d.f["vf"][i], d.f["phi"]
    w = d.ref(sch, i, k, lo, hi)[1]
    tf = phi * (w * K[m.l] + (1.0 - w) * K[m.u])
    ref = fv.surface_integrate(m, tf, [a * b for a, b in zip(phib, Kb)])
    got = np.empty(N); got[d.cmap] = out[0].cpu().numpy()
    assert same(got, ref), where_not(got, ref)


# ------------------------------------------------------------------------------------ (d) ffm_fv_multivariate_weights_tiled
@pytest.mark.parametrize("n,nf", E.TILED_BOXES)
def test_tiled_multivariate_weights(O, ffm, ctx, n, nf):
    """k_mv_tile forms its own gradients: the classes come from planted cell values (tests/fv_edge_inputs.py: tiled_fields).  The Gauss
    gradient of these fields is exact, so ffm_fvc_grad_multi must give oracle.fv.grad's bits; the tiled form and the two-pass form must
    both give the blend of the restatement's common limiter on that gradient, for every parameter set, and leave no face unwritten."""
    from oracle import fv, plume
    m = plume.make_mesh(n, h=E.H)
    s = MM.device_mesh(ffm, ctx, m)
    try:
        assert s["A"].sweep_mode == 2 and s["W"] == 3
        f = E.tiled_fields(m, nf)
        f["grad"] = np.array([fv.grad(m, f["vf"][i], f["vb"][i]) for i in range(nf)])
        d = Dev(ctx, s["mesh"], m, s["cOrd"], s["fOrd"], f)
        N = s["N"]
        vb = [ctx.to_device(np.concatenate(b)) for b in f["vb"]]
        g = [[ctx.zeros(N) for _ in range(3)] for _ in range(nf)]
        for a in range(0, nf, 4):
            b = min(a + 4, nf)
            d.mesh.call("fvc_grad_multi", b - a, d.vf[a:b], vb[a:b], [x[0] for x in g[a:b]], [x[1] for x in g[a:b]], [x[2] for x in g[a:b]])
        for i in range(nf):
            for c in range(3):
                assert same(g[i][c].cpu().numpy(), f["grad"][i][:, c][s["cOrd"]]), (i, c)
        sch = E.MV_SCHEMES[:nf]
        csch = (C.c_int * nf)(*sch)
        for k, lo, hi in E.PARAMS:
            ref = d.want(d.common(list(range(nf)), sch, k, lo, hi)[1])
            two, one = d.nan_faces(), d.nan_faces()
            d.mesh.call("fv_multivariate_weights", nf, csch, k, lo, hi, d.phi, d.vf, [x[0] for x in g], [x[1] for x in g], [x[2] for x in g], two)
            d.mesh.call("fv_multivariate_weights_tiled", nf, csch, k, lo, hi, d.phi, d.vf, vb, one)
            two, one = d.back(two), d.back(one)
            assert not np.isnan(two).any() and not np.isnan(one).any(), (k, int(np.isnan(two).sum()), int(np.isnan(one).sum()))
            assert same(two, ref), (k, "two-pass", where_not(two, ref))
            assert same(one, ref), (k, "tiled", where_not(one, ref))
    finally:
        s["mesh"].close(); s["A"].close()


# ---------------------------------------------------------------------------------- (e) one block with ghost cells, one process
@pytest.fixture(scope="module")
def block(O, ffm, ctx):
    """the last z-plane of the hex box as the ghost cells of the rest (tests/test_tile_coef_direct_gpu.py builds its refused block
    so): ghost values and ghost gradients are written by the test, nothing is exchanged.  The cut faces carry every flux class."""
    m = E.host_mesh("hex")
    nOwn, nGhost, keep, cut = E.ghost_block(m)
    l, u = m.l[keep], m.u[keep]
    hint = np.zeros(nOwn, np.int32)
    cOrd, fOrd = ffm.renumber_levels(nOwn, l, u, groupHint=hint, nGhost=nGhost)
    l2, u2, oldToNew = ffm.hexmesh.apply_renumbering(m.nCells, l, u, cOrd, fOrd)
    A = ffm.lduMatrix(ctx, nOwn, l2, u2, groupHint=hint[cOrd[:nOwn]], nGhost=nGhost)
    gface = np.nonzero(keep)[0][fOrd]
    pk = [p.faceCells < nOwn for p in m.patches]
    patches = [(oldToNew[p.faceCells[q]].astype(np.int32), p.Sf[q].T.copy(), p.deltaCoeffs[q]) for p, q in zip(m.patches, pk)]
    mesh = ffm.fvMesh(A, m.V[cOrd], m.C[cOrd].T.copy(), m.Sf[gface].T.copy(), m.magSf[gface], m.weights[gface], m.deltaCoeffs[gface], patches)
    d = Dev(ctx, mesh, m, cOrd, gface, E.fields(m, "hex"))
    d.name, d.A, d.nOwn, d.nAll, d.B = "hex", A, nOwn, m.nCells, sum(int(q.sum()) for q in pk)
    fc = E.flux_classes(d.f["phi"])
    assert all((fc[c] & cut).any() for c in E.FLUX_CLASSES) and A.sweep_mode == 2
    yield d
    mesh.close(); A.close()


@PARAMS
def test_block_with_ghost_cells(block, O, ffm, k, lo, hi):
    """the ghost-side gather of k_limited_weights and k_scalar_eqns and the ghostUp branch of k_mv_weights (a cut face whose upwind cell
    is a ghost cell is written by its owner) meet the restatement on the whole box, restricted to the block's faces; the tiled form
    answers FFM_ERR_UNSUPPORTED on a block of a decomposed mesh and writes nothing"""
    d = block
    _limited_weights(d, k, lo, hi)
    _limiters(d, k, lo, hi)
    _multivariate(d, k, lo, hi)
    _transport_coefficients(d, O, k, lo, hi, d.nAll, d.B)
    nf = 3
    out = d.nan_faces()
    vb = [d.ctx.zeros(max(d.B, 1)) for _ in range(nf)]
    with pytest.raises(ffm.FfmError, match=UNSUPPORTED):
        d.mesh.call("fv_multivariate_weights_tiled", nf, (C.c_int * nf)(*E.MV_SCHEMES[:nf]), k, lo, hi, d.phi, d.vf[:nf], vb, out)
    assert np.isnan(out.cpu().numpy()).all()


# ------------------------------------------------------------------------------------------ (f) ffm_fv_filtered_linear2V_weights
@pytest.mark.parametrize("k,l", E.FL2V_PARAMS)
def test_filtered_linear2V_weights(setup, k, l):
    """k_filtered_linear2V_weights against oracle.fv.filtered_linear2V_weights, whose expression order is the kernel's, on dyadic U and
    gradients: uniform vectors (df == 0, the denominator is SMALL), df == tcP and df == tcN exactly, tc of both signs, the unclamped
    limiter exactly 1 and (at the dyadic k, l) exactly 0, fluxes +-0 and +-2^-1074"""
    from oracle import fv
    d, m = setup, setup.m
    f = E.fl2v_fields(m, d.name)
    ref = fv.filtered_linear2V_weights(m, f["phi"], f["U"], f["gradU"], k, l)
    Ud = [d.cell(f["U"][:, j]) for j in range(3)]
    gd = [[d.cell(f["gradU"][:, i, j]) for j in range(3)] for i in range(3)]           # gd[i][j] = d_i U_j
    w = d.nan_faces()
    d.mesh.call("fv_filtered_linear2V_weights", k, l, d.face(f["phi"]), Ud, gd[0], gd[1], gd[2], w)
    got = d.back(w)
    assert same(got, d.want(ref)), where_not(got, d.want(ref))
