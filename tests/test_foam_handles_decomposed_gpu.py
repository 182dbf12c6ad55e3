"""The class layer's physics handles (include/fireFoamHandles.H: hePsiThermoJanaf, kEqnLES, eddyDissipationEDC, P1), the patch
conditions of mixedBC::update (flowRateInletVelocity, totalFlowRateAdvectiveDiffusive, inletOutlet), the reductions gMin / gMax /
gAverage / min / max / fvc::domainIntegrate and the included compressibleCourantNo.H / compressibleContinuityErrs.H on a DECOMPOSED
mesh: examples/b1_demo.C's b1_physics runs unchanged on every rank's sub-domain (owned cells + ghost cells), ranks one process each
on cuda:0 over the host (gloo) transport, as tests/test_foam_layer_decomposed_gpu.py runs b1_demo.

What a wrong number would be here: a result whose ghost entries nobody refreshed (kEqnLES::gradU feeds face interpolations of the
nine gradients), a reduction over owned + ghost cells or divided by this rank's count, the burner's mass flow divided by this rank's
share of the inlet area.  The partitions split the inlet over the ranks and leave one rank without any inlet face.

Where every bar comes from:
 * equal as bytes: per-cell and per-face functions of the inputs, no neighbour access -- a rank evaluates the same expression on
   the same operands;
 * rel_l2 < 1e-14 for cell sums over faces, 1e-15 for values of single faces: tests/test_foam_layer_decomposed_gpu.py (rAU, rho);
 * rel_l2 < 1e-8 after a Krylov solve to 1e-10, equal iteration counts on every rank: the same test (Yi, K, U);
 * 1e-13 relative for the scalars against the single-rank run: the a-priori bound n eps of a sum of n = 504 same-signed terms in
   any order is 5.6e-14; exact for min / max;
 * single rank against closed forms in numpy: 1e-13 (max-norm) for the thermo and the EDC rate, 1e-15 for nut / alphat:
   tests/test_thermo_gpu.py; 1e-13 for G and 1e-12 for the stress divergence: tests/test_les_terms_gpu.py; rtol 1e-14 for the
   patch conditions: tests/test_foam_layer_gpu.py::test_burner_patch_conditions_on_the_device.
Single-rank comparisons that exist elsewhere and are not repeated: k, U and Yi after their solves and the thermo at class-layer
level (tests/test_steckler_case_gpu.py, tests/test_foam_layer_gpu.py, tests/test_thermo_gpu.py::test_thermo_correct_through_the_handle_
of_the_foam_layer), P1's G, Ru = a G - E and wall flux (tests/test_p1_foam_gpu.py)."""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import foam_case
from common import rel_l2, free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MESH = (9, 8, 7)
SMALL = 1e-15


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


class _Case:
    """the mesh, the inputs and the single-rank run, made once for every test of this file"""

    def __init__(self, O, ffm, ctx):
        from oracle import plume
        self.m = m = plume.make_mesh(MESH, h=0.1)
        self.I = foam_case.physics_inputs(O, m)
        self.one = foam_case.run_b1_physics(ffm, ctx, m, self.I)
        assert np.array_equal(self.one["cells"], np.arange(m.nCells))
        self.B = sum(p.size for p in m.patches)
        assert np.array_equal(self.one["bpos"], np.arange(self.B))
        cat = np.concatenate
        self.fc = cat([p.faceCells for p in m.patches]); self.magSf = cat([p.magSf for p in m.patches])
        self.delta_b = cat([p.deltaCoeffs for p in m.patches])


@pytest.fixture(scope="module")
def case(O, ffm, ctx):
    return _Case(O, ffm, ctx)


def _avgU(case, rho_b):
    I = case.I
    t0, v0, t1, v1 = I["table"]
    mdot = v0 + (v1 - v0) * (I["t"] - t0) / (t1 - t0)
    inlet = I["inletMask"] > 0.5
    return -mdot / np.sum((rho_b * case.magSf)[inlet])


def test_single_rank_against_closed_forms(case):
    """Every output of b1_physics that no other test compares at class-layer level, on one rank, against numpy
    restatements.  Each stage is given the device's own upstream fields (the k it solved, the thermo fields it returned), so that a
    stage's bar is the bar of its own operation."""
    from oracle import steckler_case as SC, thermo as TH
    import plume_thermo_ref as PT
    m, I, one = case.m, case.I, case.one
    N, B, fc, magSf = m.nCells, case.B, case.fc, case.magSf
    inlet = I["inletMask"] > 0.5
    per_patch = lambda a: np.split(a, np.cumsum([p.size for p in m.patches])[:-1], axis=0)
    # a: thermo.  Patch faces: T is either fixed or the Newton solve of he_b = Hs(T_b) started at T_b, which returns T_b
    sp = PT.species()
    mx = sp.mixture(I["Y"]); he = mx.Hs(I["p"], I["T"]); Tr = mx.THs(he, I["p"], I["Tstart"])
    assert np.abs(Tr - I["T"]).max() < 0.5 and np.abs(I["Tstart"] - I["T"]).max() > 10.0         # the Newton iteration had work to do
    T, psi, mu, alpha = one["thermo"]
    for got, want in ((T, Tr), (psi, mx.psi(I["p"], Tr)), (mu, mx.mu(I["p"], Tr)), (alpha, mx.alphah(I["p"], Tr))):
        assert _rel(got, want) < 1e-13
    mb = sp.mixture(I["Yb"])
    Tb, psib, mub, alphab = one["thermob"]
    for got, want in ((Tb, I["Tb"]), (psib, mb.psi(I["pb"], I["Tb"])), (mub, mb.mu(I["pb"], I["Tb"])), (alphab, mb.alphah(I["pb"], I["Tb"]))):
        assert _rel(got, want) < 1e-13
    rho = (psi * I["p"]) * I["rhoFac"]; rho_b = (psib * I["pb"]) * I["rhoFacb"]
    # b: correctNut() from k0, cells and patch faces (alphatWallFunction with nut_b = 0 on the floor)
    nut0 = I["Ck"] * np.sqrt(I["k0"]) * I["delta"]
    assert _rel(one["nut0"][0], nut0) < 1e-15 and _rel(one["nut0"][1], rho * nut0 / I["Prt"]) < 1e-15
    zg = I["nutZeroGrad"]
    nut0b = zg * one["nut0"][0][fc]
    assert np.array_equal(one["nut0b"][0], nut0b)
    assert _rel(one["nut0b"][1], I["alphatZeroGrad"] * one["nut0"][1][fc] + (1.0 - I["alphatZeroGrad"]) * (rho_b * nut0b / I["PrtWall"])) < 1e-15
    # U's patch values before its solve: flowRateInletVelocity on the inlet, mixed elsewhere
    avgU = _avgU(case, rho_b)
    Ub0 = np.stack([np.where(inlet, avgU * I["inletNf"][d], I["bcU"][3 * d] * I["bcU"][3 * d + 1] + (1.0 - I["bcU"][3 * d]) * I["U0"][d][fc]) for d in range(3)])
    gU, gUb = SC.grad_vector(m, I["U0"].T.copy(), per_patch(Ub0.T.copy()))
    twoSymm = gU + np.swapaxes(gU, 1, 2)
    tr = (twoSymm[:, 0, 0] + twoSymm[:, 1, 1]) + twoSymm[:, 2, 2]
    dev = twoSymm.copy()
    for a in range(3):
        dev[:, a, a] = dev[:, a, a] - (1.0 / 3.0) * tr
    assert rel_l2(one["G"], one["nut0"][0] * np.einsum("nij,nij->n", gU, dev)) < 1e-13
    # c: the EDC rate (C_Diff 0, C_Stiff 1) on the state before the k solve
    eps = I["Ce"] * I["k0"] * np.sqrt(I["k0"]) / I["delta"]
    rt = np.maximum(I["C_EDC"] * eps / np.maximum(I["k0"], SMALL), 0.0)
    w = rho * np.minimum(I["Y"][I["fuel"]], I["Y"][I["o2"]] / one["s"]) / I["dt"] * (1.0 - np.exp(-I["dt"] * rt))
    assert w.min() > 0 and _rel(one["wFuel"], w) < 1e-13
    # the specie's patch condition: totalFlowRateAdvectiveDiffusive on the inlet, inletOutlet on the open patches, zeroGradient on the floor
    alphaEff_b = alphab + one["nut0b"][1]
    f = np.where(inlet, 1.0 / (1.0 + alphaEff_b * case.delta_b * magSf / np.maximum(np.abs(I["phib"]), SMALL)),
                 np.where(I["bcY"][0] < 0, 1.0 - (I["phib"] >= 0), 0.0))
    assert np.allclose(one["f"], f, rtol=1e-14, atol=0)
    assert np.allclose(one["Yb"], f * I["bcY"][1] + (1.0 - f) * one["Yi"][fc], rtol=1e-14, atol=0)
    noflux = inlet & (I["phib"] == 0.0)
    assert noflux.sum() >= 3 and np.all(one["f"][noflux] < 1e-8) and np.all(one["f"][inlet & ~noflux] > 0.5)
    assert set(np.unique(one["f"][I["bcY"][0] < 0])) == {0.0, 1.0}                      # inletOutlet: both directions occur
    # the explicit stress term of divDevRhoReff(U), with the nut of k0; then, after the k solve, nut / alphat of the solved k
    gam = rho * (one["nut0"][0] + mu / rho); gamb = rho_b * (nut0b + mub / rho_b)
    X = gam[:, None, None] * SC.dev2T(gU); Xb = [g[:, None, None] * SC.dev2T(t) for g, t in zip(per_patch(gamb), gUb)]
    div_ref = SC.div_tensor(m, X, Xb)
    for d in range(3):
        assert rel_l2(one["src"][d], m.V * div_ref[:, d]) < 1e-12, d
    nut = I["Ck"] * np.sqrt(one["k"]) * I["delta"]
    assert one["k"].min() > 1e-6 and _rel(one["nut"][0], nut) < 1e-15 and _rel(one["nut"][1], rho * nut / I["Prt"]) < 1e-15
    assert np.array_equal(one["nutb"][0], zg * one["nut"][0][fc])
    # U's patch values after its solve
    for d in range(3):
        want = np.where(inlet, avgU * I["inletNf"][d], I["bcU"][3 * d] * I["bcU"][3 * d + 1] + (1.0 - I["bcU"][3 * d]) * one["U"][d][fc])
        assert np.allclose(one["Ub"][d], want, rtol=1e-14, atol=1e-300), d
    assert one["Ub"][1][inlet].min() > 0                                               # inflow: against the outward normal (0 -1 0)
    # e: the scalars.  Sums: |device - fsum| <= n eps sum|terms| (any order of summation), carried through the quotient
    sc = one["scalars"]
    eps_n = N * np.finfo(float).eps
    absphi = np.abs(I["phi"])
    sumPhi = np.zeros(N); np.add.at(sumPhi, m.l, absphi); np.add.at(sumPhi, m.u, absphi); np.add.at(sumPhi, fc, np.abs(I["phib"]))
    sumPhi = sumPhi / rho
    assert abs(sc[0] - 0.5 * (sumPhi / m.V).max() * I["dt"]) <= 1e-13 * sc[0]
    assert abs(sc[1] - 0.5 * (math.fsum(sumPhi) / math.fsum(m.V)) * I["dt"]) <= 4 * eps_n * sc[1]
    rhoT = psi * I["p"]
    mass = math.fsum(m.V * rho)
    assert abs(sc[2] - math.fsum(m.V * np.abs(rho - rhoT)) / mass) <= 4 * eps_n * sc[2]
    assert abs(sc[3] - math.fsum(m.V * (rho - rhoT)) / mass) <= 4 * eps_n * sc[2]      # sum|terms|/mass is sc[2]
    assert sc[4] == 0.25 + sc[3] and sc[5] == 4.0 * I["e"] * 5.670367e-8
    for k, (c, b) in enumerate(((I["fa"], I["fab"]), (I["fc"], I["fcb"]))):
        o = sc[6 + 5 * k: 11 + 5 * k]
        assert o[0] == c.min() and o[1] == c.max() and o[3] == min(c.min(), b.min()) and o[4] == max(c.max(), b.max())
        assert abs(o[2] - math.fsum(c) / N) <= eps_n * np.abs(c).sum() / N
    assert sc[9] == -1.5 and sc[10] == 2.5 and sc[6] >= 0 and sc[7] < 1                # `fa`: the extremes are boundary faces
    assert sc[11] == sc[14] == -2.0 and sc[12] == sc[15] == 3.0                         # `fc`: they are cells
    assert abs(sc[16] - math.fsum(m.V * I["fa"])) <= eps_n * np.sum(m.V * np.abs(I["fa"]))
    assert sc[8] == sc[17] / N


@pytest.mark.parametrize("world,partitioner", [(2, "rcb"), (3, "graph"), (4, "graph")])
def test_physics_handles_on_a_decomposed_mesh(case, ffm, world, partitioner):
    """Every rank's owned cells and boundary faces assembled into global fields, against the single-rank
    run of the same code; the scalars of every rank against each other and against the single rank; every rank ends by itself and
    leaves its file (a rank waiting in a collective the others skipped would be killed at the time limit instead).

    Conditions on the inputs, asserted here from the host-only partitioner: at least two ranks own inlet faces; with 3 and 4 ranks
    one rank owns none; every rank has ghost cells; both extremes of the boundary-extreme field lie on a rank other than 0."""
    m, I, one = case.m, case.I, case.one
    N, B, fc = m.nCells, case.B, case.fc
    inlet = I["inletMask"] > 0.5
    part = ffm.decompose.partition_rcb(m.C, world) if partitioner == "rcb" else ffm.decompose.partition_graph(m.nCells, m.l, m.u, world)
    inletFaces = np.bincount(part[fc[inlet]], minlength=world)
    assert (inletFaces > 0).sum() >= 2
    if world > 2:
        assert (inletFaces == 0).any()
    assert part[fc[B - 1]] != 0 and part[fc[B - 2]] != 0 and I["fab"][B - 1] == I["fab"].max() and I["fab"][B - 2] == I["fab"].min()
    port = free_port()
    with tempfile.TemporaryDirectory() as tmp:
        procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "workers", "foam_rank.py"), str(r), str(world), str(port)] + [str(v) for v in MESH]
                                  + [partitioner, tmp, "physics"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE) for r in range(world)]
        try:
            outs = [p.communicate(timeout=150) for p in procs]
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
        assert [p.returncode for p in procs] == [0] * world, [o[1][-1500:] for o in outs]
        assert all(os.path.exists(os.path.join(tmp, "rank%d.npz" % r)) for r in range(world))
        parts = [dict(np.load(os.path.join(tmp, "rank%d.npz" % r))) for r in range(world)]
    assert sorted(np.concatenate([p["cells"] for p in parts]).tolist()) == list(range(N))              # a partition of the cells
    assert sorted(np.concatenate([p["bpos"] for p in parts]).tolist()) == list(range(B))               # ... and of the boundary faces
    assert all(int(p["nGhost"]) > 0 for p in parts)
    assert [int((I["inletMask"][p["bpos"]] > 0.5).sum()) for p in parts] == inletFaces.tolist()
    full = {}
    for k in ("thermo", "nut0", "wFuel", "G", "k", "nut", "src", "U", "Yi", "p1"):
        full[k] = np.full_like(one[k], np.nan)
        for p in parts:
            full[k][..., p["cells"]] = p[k]
    for k in ("thermob", "nut0b", "nutb", "Ub", "Yb", "f"):
        full[k] = np.full_like(one[k], np.nan)
        for p in parts:
            full[k][..., p["bpos"]] = p[k]
    # per cell / per face, no neighbour access: equal as bytes
    for k in ("thermo", "thermob", "wFuel", "nut0", "nut0b"):
        assert full[k].tobytes() == one[k].tobytes(), k
    # gathers of neighbours, no Krylov solve
    assert rel_l2(full["G"], one["G"]) < 1e-14
    # (the stress divergence interpolates the nine gradients to the cut faces: their ghost entries are those kEqnLES::gradU refreshed)
    for d in range(3):
        assert rel_l2(full["src"][d], one["src"][d]) < 1e-14, d
    assert rel_l2(full["f"], one["f"]) < 1e-15                                          # value fraction: a function of one face
    for d in range(3):
        assert rel_l2(full["Ub"][d][inlet], one["Ub"][d][inlet]) < 1e-14, d             # avgU: one sum over the inlet, in the ranks' order
    # after a Krylov solve
    assert len({tuple(p["nit"].tolist()) for p in parts}) == 1                          # every rank saw the same (global) solver performance
    for k in ("k", "Yi"):
        assert rel_l2(full[k], one[k]) < 1e-8, k
    for k in ("U", "nut", "p1", "nutb", "Ub"):
        for c in range(one[k].shape[0]):
            assert rel_l2(full[k][c], one[k][c]) < 1e-8, (k, c)
    assert rel_l2(full["Yb"], one["Yb"]) < 1e-8
    # the scalars: the same on every rank; the single rank's to 1e-13; min / max exactly
    for p in parts[1:]:
        assert p["scalars"].tobytes() == parts[0]["scalars"].tobytes()
    sc, s1 = parts[0]["scalars"], one["scalars"]
    for i in (0, 1, 2, 3, 4, 8, 13, 16, 17):
        assert abs(sc[i] - s1[i]) <= 1e-13 * abs(s1[i]), (i, sc[i], s1[i])
    for i in (5, 6, 7, 9, 10, 11, 12, 14, 15):
        assert sc[i] == s1[i], (i, sc[i], s1[i])
    # gAverage: the sum over all ranks by the cell count of ALL ranks
    assert sc[8] == sc[17] / N and abs(sc[8] - math.fsum(I["fa"]) / N) <= N * np.finfo(float).eps * np.abs(I["fa"]).sum() / N
    # flowRateInletVelocity: one average velocity, from the mass flow over the WHOLE inlet, on every rank that owns inlet faces
    rho_b = (one["thermob"][1] * I["pb"]) * I["rhoFacb"]
    avgU = _avgU(case, rho_b)
    seen = []
    for p in parts:
        mine = I["inletMask"][p["bpos"]] > 0.5
        if mine.any():
            a = p["Ub"][1][mine] / I["inletNf"][1][p["bpos"]][mine]
            assert np.all(a == a[0])
            seen.append(a[0])
    assert len(seen) == (inletFaces > 0).sum() and len(set(seen)) == 1
    assert abs(seen[0] - avgU) <= 1e-14 * abs(avgU)
