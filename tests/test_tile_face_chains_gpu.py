"""The two gradient chains that run as tile passes (csrc/ffm_fused.hip: k_mv_tile<MVT_WK>, k_mv_tile<MVT_LUST>, k_phiK_sum, k_lust_sum)
against the per-operator entry points they replace, every comparison of BITS (uint64 views):

  A  ffm_fv_multivariate_weights_phiK_tiled + ffm_fvc_div_phiK_sum  ==  ffm_fvc_grad + ffm_fvc_div_phiK_terms  (divK, ddtK, -dpdt), and
     the common weights are those of ffm_fv_multivariate_weights_tiled: the seventh staged field does not touch them;
  B  ffm_fv_lust_phi_correction3_tiled + ffm_fvm_lust_source3_sum   ==  ffm_fvc_grad_multi + ffm_fvm_lust_source3  (the three sources).

Boxes of spacing 1/8 (tests/fv_edge_inputs.py).  The tile hint of a box makes 16 x 16 tiles in (y, z) with the columns along x
(csrc/ffm_ldu_analysis.cpp: pick_mode); a level of a tile is one entry, 32 entries are one run (one workgroup):
  20 x 18 x 40   2 x 3 tiles, partial ones in both directions, 50 levels in a full tile: two runs
  40 x 20 x 18   2 x 2 tiles, 70 levels in a full tile: three runs
  8 x 8 x 8      one partial tile, one run
  33 x 17 x 5    two tiles, the second one cell wide, 52 levels
  5 x 33 x 17    3 x 2 tiles, columns of five cells
Inputs: the designed fields and fluxes of fv_edge_inputs.tiled_fields (+0, -0, +-2^-1074, uniform regions, the limiter's switch points;
on the boxes wider than 11 cells also whole planes of +0 and -0 fluxes) and hashed fields.  tests/test_tile_face_classes_cpu.py shows on
the host that the designed fluxes reach every class of face of the tile walk on the first two boxes."""
import ctypes as C

import numpy as np
import pytest

import fv_edge_inputs as E
import merged_mesh as MM

pytestmark = pytest.mark.gpu

UNSUPPORTED = r"failed \(-5\)"                 # FFM_ERR_UNSUPPORTED through binding._check
BOXES = [(20, 18, 40), (40, 20, 18), (8, 8, 8), (33, 17, 5), (5, 33, 17)]
K_PARAMS = [(2, 1.0, 0.0, 1.0), (3, 1.0, 0.0, 1.0), (3, 0.5, 0.0, 1.0), (3, 2.0, 0.25, 0.75), (2, 0.0, 0.0, 1.0)]      # (scheme, k, lo, hi) of K


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def where_not(a, b):
    bad = np.nonzero(bits(a) != bits(b))[0]
    return len(bad), [(int(i), float(a[i]), float(b[i])) for i in bad[:5]]


@pytest.fixture(scope="module", params=BOXES, ids=lambda n: "x".join(map(str, n)))
def box(request, O, ffm, ctx):
    from oracle import plume
    n = request.param
    m = plume.make_mesh(n, h=E.H)
    s = MM.device_mesh(ffm, ctx, m, face_centres=True)
    assert s["A"].sweep_mode == 2 and s["W"] == 3
    s["n"] = n
    yield s
    s["mesh"].close(); s["A"].close()


class Fields:
    """six fields under the common limiter + K (A), three velocity components (B), the fluxes and the cell fields of the sum passes"""

    def __init__(self, s, O, ctx, designed):
        m, N, B, F = s["m"], s["N"], s["B"], s["F"]
        cOrd, fOrd, mesh = s["cOrd"], s["fOrd"], s["mesh"]
        dev = ctx.to_device
        if designed:
            f = E.tiled_fields(m, E.NF)
            vf, vb, phi = f["vf"], [np.concatenate(b) for b in f["vb"]], f["phi"]
            ck = E.cell_keys(m, E.TILED_SEED + 1)
            K = E.TILED_UNITS[E._pick(ck, 5, len(E.TILED_UNITS))] / 64.0
            Kb = np.concatenate([E.VALUES[E._pick(ck[p.faceCells], 7 + q, len(E.VALUES))] for q, p in enumerate(m.patches)])
            U, Ub = vf[:3], vb[:3]
        else:
            h = lambda seed, n: O.hash_u(seed, np.arange(n))
            vf = [1.1 * (0.2 + h(31 + 7 * i, N)) - 0.2 for i in range(E.NF)]
            a = 0.2 + h(31, N); vf[0] = np.where(a > 0.9, a, 0.25)
            vb = [0.1 + h(133 + i, B) for i in range(E.NF)]
            phi = 0.3 * (h(32, F) - 0.5); phi[::7] = 0.0; phi[3::11] = -0.0
            K, Kb = 2.0 * h(71, N), 2.0 * h(72, B)
            U, Ub = [h(81 + i, N) - 0.5 for i in range(3)], [h(91 + i, B) - 0.5 for i in range(3)]
        self.phi_h = phi
        self.phi = mesh.to_native(np.asarray(phi)[fOrd])
        self.vf, self.vb = [dev(np.asarray(v)[cOrd]) for v in vf], [dev(v) for v in vb]
        self.K, self.Kb = dev(np.asarray(K)[cOrd]), dev(Kb)
        self.U, self.Ub = [dev(np.asarray(v)[cOrd]) for v in U], [dev(v) for v in Ub]
        h = lambda seed, n: O.hash_u(seed, np.arange(n))
        self.phib = dev(0.2 * (h(41, B) - 0.5))
        self.rho, self.rho0, self.K0, self.dpdt = dev(0.5 + h(42, N)), dev(0.5 + h(43, N)), dev(h(44, N)), dev(h(45, N) - 0.5)
        self.U0 = [dev(h(46 + i, N) - 0.5) for i in range(3)]
        self.rdt = 1000.0


@pytest.fixture(scope="module", params=["designed", "hashed"])
def fields(request, box, O, ctx):
    return Fields(box, O, ctx, request.param == "designed")


def _nan(ctx, n):
    return ctx.zeros(n) + float("nan")


def test_div_phiK_on_the_multivariate_tile_pass(box, fields, ctx):
    """A: divK, ddtK, -dpdt from the face products of the tile pass == ffm_fvc_grad + ffm_fvc_div_phiK_terms; the common weights ==
    ffm_fv_multivariate_weights_tiled's; every internal face's product is written"""
    s, f, mesh, N = box, fields, box["mesh"], box["N"]
    nf = E.NF
    sch = (C.c_int * nf)(*E.MV_SCHEMES)
    g = [ctx.zeros(N) for _ in range(3)]
    mesh.call("fvc_grad", f.K, f.Kb, *g)
    wRef = _nan(ctx, mesh.nNative)
    mesh.call("fv_multivariate_weights_tiled", nf, sch, 1.0, 0.0, 1.0, f.phi, f.vf, f.vb, wRef)
    for schK, k, lo, hi in K_PARAMS:
        ref = [_nan(ctx, N) for _ in range(3)]
        mesh.call("fvc_div_phiK_terms", schK, k, lo, hi, f.rdt, f.phi, f.phib, f.K, f.Kb, *g, f.rho, f.rho0, f.K0, f.dpdt, *ref)
        w, q = _nan(ctx, mesh.nNative), _nan(ctx, mesh.nNative)
        mesh.call("fv_multivariate_weights_phiK_tiled", nf, sch, 1.0, 0.0, 1.0, f.phi, f.vf, f.vb, w, schK, k, lo, hi, f.K, f.Kb, q)
        assert np.array_equal(bits(w.cpu().numpy()), bits(wRef.cpu().numpy())), (schK, k)
        assert not np.isnan(mesh.from_native(q)).any()
        out = [_nan(ctx, N) for _ in range(3)]
        mesh.call("fvc_div_phiK_sum", f.rdt, q, f.phib, f.K, f.Kb, f.rho, f.rho0, f.K0, f.dpdt, *out)
        for name, a, b in zip(("divK", "ddtK", "ndpdt"), out, ref):
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert not np.isnan(b).any() and np.array_equal(bits(a), bits(b)), (schK, k, name, where_not(a, b))


def test_lust_source_by_the_upwind_cell(box, fields, ctx):
    """B: the three sources from the face products of the tile pass == ffm_fvc_grad_multi + ffm_fvm_lust_source3"""
    s, f, mesh, N = box, fields, box["mesh"], box["N"]
    g = [[ctx.zeros(N) for _ in range(3)] for _ in range(3)]
    gx, gy, gz = [x[0] for x in g], [x[1] for x in g], [x[2] for x in g]
    mesh.call("fvc_grad_multi", 3, f.U, f.Ub, gx, gy, gz)
    ref = [_nan(ctx, N) for _ in range(3)]
    mesh.call("fvm_lust_source3", f.rdt, f.phi, f.rho0, f.U0, gx, gy, gz, ref)
    q = [_nan(ctx, mesh.nNative) for _ in range(3)]
    mesh.call("fv_lust_phi_correction3_tiled", f.phi, f.U, f.Ub, q)
    assert not any(np.isnan(mesh.from_native(x)).any() for x in q)
    out = [_nan(ctx, N) for _ in range(3)]
    mesh.call("fvm_lust_source3_sum", f.rdt, f.rho0, f.U0, q, out)
    for c, (a, b) in enumerate(zip(out, ref)):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert not np.isnan(b).any() and np.array_equal(bits(a), bits(b)), (c, where_not(a, b))


# ---------------------------------------------------------------------------------------------------------------------- refusals
def _refused(ffm, ctx, mesh, N, B):
    nat = mesh.nNative
    cellf = lambda: ctx.zeros(N) + 0.5
    bf = lambda: ctx.zeros(max(B, 1)) + 0.5
    phi = ctx.zeros(nat) + 0.25
    nf = 3
    w, q = _nan(ctx, nat), _nan(ctx, nat)
    with pytest.raises(ffm.FfmError, match=UNSUPPORTED):
        mesh.call("fv_multivariate_weights_phiK_tiled", nf, (C.c_int * nf)(2, 3, 3), 1.0, 0.0, 1.0, phi, [cellf() for _ in range(nf)],
                  [bf() for _ in range(nf)], w, 2, 1.0, 0.0, 1.0, cellf(), bf(), q)
    q3 = [_nan(ctx, nat) for _ in range(3)]
    with pytest.raises(ffm.FfmError, match=UNSUPPORTED):
        mesh.call("fv_lust_phi_correction3_tiled", phi, [cellf() for _ in range(3)], [bf() for _ in range(3)], q3)
    for t in [w, q] + q3:
        assert np.isnan(t.cpu().numpy()).all()


def test_refused_on_rows_wider_than_a_hex_cells(O, ffm, ctx):
    """a w8 mesh of tests/merged_mesh.py: FFM_ERR_UNSUPPORTED, the NaN-filled outputs untouched"""
    s = MM.device_mesh(ffm, ctx, MM.case("w8", h=E.H), face_centres=True)
    try:
        assert s["W"] == 8
        _refused(ffm, ctx, s["mesh"], s["N"], s["B"])
    finally:
        s["mesh"].close(); s["A"].close()


def test_refused_on_a_block_with_ghost_cells(O, ffm, ctx):
    """the last z-plane of the hex box as the ghost cells of the rest (tests/test_fv_limiter_edges_gpu.py builds its block so)"""
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
    mesh.set_face_centres(m.Cf[gface].T.copy())
    try:
        assert A.sweep_mode == 2
        _refused(ffm, ctx, mesh, m.nCells, sum(int(q.sum()) for q in pk))
    finally:
        mesh.close(); A.close()
