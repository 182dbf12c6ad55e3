"""The flow-ordered exact solve (csrc/ffm_solve.hip: ffm_flow_order_create, ffm_solve_ordered_d) on upwind ray matrices
(tests/ray_matrix.py): psi is BITWISE the serial forward substitution restated in tests/ray_matrix.py -- no tolerance, the
arithmetic is fully specified -- on a box of two chunks of 256 positions in the library's numbering and in a random one, on
polyhedral meshes of every row-width bucket above a hex's and on the steckler room; for four rays of different octants and
(1,0,0).  Orders are reused and swapped on one matrix handle; an order that does not fit the matrix, a matrix that is not
triangular, a decomposed matrix and the order of a matrix of another size are refused before any sweep is launched.  The
perf records -- the norms of the rank's rows alone, which the row kernels form -- are bit for bit those recorded from the commit
before the single-rank solve became the one-stage case of the staged one (tests/golden/solve_ordered_perf.json, written by
scripts/record_solve_ordered_perf.py); ffm_solve_triangular_rows_d shares the prologue and the epilogue and is pinned with it."""
import ctypes as C
import heapq
import json
import os

import numpy as np
import pytest

import ray_matrix as R
from common import laplacian_like

pytestmark = pytest.mark.gpu

CASES = ["box", "box_random", "w8", "w16u14", "w32l30", "w32multi", "w32u18", "steckler"]
_cache = {}


def random_relabelling(m, seed=11):
    """new->old cell and face orders of a random relabelling that keeps every face's owner below its neighbour (a random
    linear extension of the owner -> neighbour graph), faces sorted upper-triangular: far from any level order"""
    N = m.nCells
    key = np.random.RandomState(seed).permutation(N)
    succ = [[] for _ in range(N)]
    indeg = np.zeros(N, np.int64)
    for a, b in zip(m.l.tolist(), m.u.tolist()):
        succ[a].append(b); indeg[b] += 1
    heap = [(int(key[c]), c) for c in range(N) if indeg[c] == 0]
    heapq.heapify(heap)
    cOrd = []
    while heap:
        _, c = heapq.heappop(heap)
        cOrd.append(c)
        for b in succ[c]:
            indeg[b] -= 1
            if indeg[b] == 0:
                heapq.heappush(heap, (int(key[b]), b))
    cOrd = np.array(cOrd)
    oldToNew = np.empty(N, np.int64); oldToNew[cOrd] = np.arange(N)
    fOrd = np.lexsort((oldToNew[m.u], oldToNew[m.l]))
    return cOrd, fOrd


def relabelled(m, cOrd, fOrd):
    """what merged_mesh.renumbered does, for the fields a ray matrix needs (a hex box has no merged-face fields)"""
    import types
    oldToNew = np.empty(m.nCells, np.int64); oldToNew[cOrd] = np.arange(m.nCells)
    r = types.SimpleNamespace(nCells=m.nCells, l=oldToNew[m.l[fOrd]], u=oldToNew[m.u[fOrd]], Sf=m.Sf[fOrd], V=m.V[cOrd])
    assert np.all(r.l < r.u) and np.all(np.diff(r.l * r.nCells + r.u) > 0)
    return r


def case(ffm, O, name):
    """the mesh as the library is given it, its five ray systems and their serial solutions: computed once, never changed"""
    if name in _cache:
        return _cache[name]
    if name == "box":
        m = R.mesh("box7x8x6")
        m = relabelled(m, *ffm.renumber_levels(m.nCells, m.l, m.u))
    elif name == "box_random":
        m = R.mesh("box7x8x6")
        m = relabelled(m, *random_relabelling(m))
    else:
        m = R.mesh(name)
    N = m.nCells
    l, u = np.asarray(m.l, np.int64), np.asarray(m.u, np.int64)
    rays = []
    for i, (tag, d, omega) in enumerate(R.five_directions()):
        diag, upper, lower = R.ray_matrix(m, d, omega)
        source = 0.5 + O.hash_u(40 + i, np.arange(N))
        order, nLevels = ffm.flow_levels(N, l, u, upper, lower)
        want = R.forward_substitution(N, l, u, diag, upper, lower, source, order)
        assert np.isfinite(want).all()
        rays.append(dict(tag=tag, d=d, omega=omega, diag=diag, upper=upper, lower=lower, source=source, nLevels=nLevels, want=want))
    _cache[name] = dict(m=m, N=N, l=l, u=u, rays=rays)
    return _cache[name]


PERF_CASES = ["box", "box_random", "w32multi"]
PERF_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_ordered_perf.json")


def perf_records(ffm, O, ctx):
    """{key: [initialResidual.hex(), finalResidual.hex()]} of ffm_solve_ordered_d on the five rays of PERF_CASES from a finite
    hashed start value, and of ffm_solve_triangular_rows_d on the all-positive ray of `box` (triangular in the library's order).
    The ray matrices are asymmetric, so the tiled symmetric Amul is never theirs; `box` (336 cells) stands for the hex box"""
    out = {}
    for name in PERF_CASES:
        k = case(ffm, O, name)
        A = ffm.lduMatrix(ctx, k["N"], k["l"], k["u"])
        for i, r in enumerate(k["rays"]):
            A.set_coeffs(r["diag"], r["upper"], r["lower"])
            order = A.flow_order()
            psi = ctx.to_device(O.hash_u(90 + i, np.arange(k["N"])) - 0.25)
            perf = A.solve_ordered(order, psi, ctx.to_device(r["source"]))
            assert perf["nIterations"] == 1 and perf["converged"] == 1, perf
            out["ordered/%s/%s" % (name, r["tag"])] = [perf["initialResidual"].hex(), perf["finalResidual"].hex()]
            order.close()
        A.close()
    k = case(ffm, O, "box")
    r = k["rays"][0]
    assert not r["upper"].any()                                      # the all-positive ray: lower-triangular as numbered
    A = ffm.lduMatrix(ctx, k["N"], k["l"], k["u"]).set_coeffs(r["diag"], r["upper"], r["lower"])
    assert A.native_order
    psi, src = ctx.to_device(O.hash_u(97, np.arange(k["N"])) - 0.25), ctx.to_device(r["source"])
    fn, perf = ffm.lib().ffm_solve_triangular_rows_d, ffm.binding.Perf()
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ffm.binding.Perf)], C.c_int
    assert fn(A.h, C.c_void_p(psi.data_ptr()), C.c_void_p(src.data_ptr()), C.byref(perf)) == 0
    assert perf.nIterations == 1 and perf.converged == 1
    assert np.allclose(psi.cpu().numpy(), r["want"], rtol=1e-12, atol=0)      # (the DILU sweep multiplies by 1/diag: not bitwise)
    out["triangular_rows/box/%s" % r["tag"]] = [perf.initialResidual.hex(), perf.finalResidual.hex()]
    A.close()
    return out


def bits(t):
    return t.cpu().numpy().view(np.int64)


def solve(ctx, A, order, source):
    psi = ctx.to_device(np.full(len(source), np.nan))
    perf = A.solve_ordered(order, psi, ctx.to_device(source))
    return psi, perf


@pytest.mark.parametrize("name", CASES)
def test_bitwise_forward_substitution(O, ffm, ctx, name):
    k = case(ffm, O, name)
    N = k["N"]
    if name in ("box", "box_random"):
        assert N == 336                                              # two chunks of 256 positions
    A = ffm.lduMatrix(ctx, N, k["l"], k["u"])
    if name == "box":
        assert A.native_order
    if name == "box_random":
        assert not A.native_order                                    # the vectors go through the library's permutation
    for r in k["rays"]:
        A.set_coeffs(r["diag"], r["upper"], r["lower"])
        order = A.flow_order()
        assert order.nLevels == r["nLevels"]
        psi, perf = solve(ctx, A, order, r["source"])
        assert np.array_equal(bits(psi), r["want"].view(np.int64)), (name, r["tag"])
        assert perf["nIterations"] == 1 and perf["converged"] == 1, perf
        res = A.residual(psi, ctx.to_device(r["source"])).cpu().numpy()
        assert np.abs(res).sum() <= 1e-10 * np.abs(r["source"]).sum()
        order.close()
    A.close()


@pytest.mark.parametrize("name", ["box", "box_random", "w32multi"])
def test_orders_are_reused_and_swapped_on_one_handle(O, ffm, ctx, name):
    k = case(ffm, O, name)
    A = ffm.lduMatrix(ctx, k["N"], k["l"], k["u"])
    r0, r1 = k["rays"][0], k["rays"][1]
    A.set_coeffs(r0["diag"], r0["upper"], r0["lower"]); o0 = A.flow_order()
    A.set_coeffs(r1["diag"], r1["upper"], r1["lower"]); o1 = A.flow_order()
    A.set_coeffs(r0["diag"], r0["upper"], r0["lower"])
    first, _ = solve(ctx, A, o0, r0["source"])
    A.set_coeffs(r1["diag"], r1["upper"], r1["lower"])
    second, _ = solve(ctx, A, o1, r1["source"])
    A.set_coeffs(r0["diag"], r0["upper"], r0["lower"])
    third, _ = solve(ctx, A, o0, r0["source"])
    assert np.array_equal(bits(first), r0["want"].view(np.int64))
    assert np.array_equal(bits(second), r1["want"].view(np.int64))
    assert np.array_equal(bits(first), bits(third))
    o0.close(); o1.close(); A.close()


@pytest.mark.parametrize("name", ["box", "box_random"])
def test_the_order_of_the_opposite_ray_is_refused_and_psi_untouched(O, ffm, ctx, name):
    k = case(ffm, O, name)
    N, m, r = k["N"], k["m"], k["rays"][0]
    A = ffm.lduMatrix(ctx, N, k["l"], k["u"])
    A.set_coeffs(r["diag"], r["upper"], r["lower"])
    order = A.flow_order()
    A.set_coeffs(*R.ray_matrix(m, -r["d"], r["omega"]))
    start = np.full(N, np.nan); start[::3] = O.hash_u(7, np.arange(N))[::3]
    psi = ctx.to_device(start)
    with pytest.raises(ffm.FfmError, match=r"\(-5\)"):
        A.solve_ordered(order, psi, ctx.to_device(r["source"]))
    assert np.array_equal(bits(psi), start.view(np.int64))
    A.set_coeffs(r["diag"], r["upper"], r["lower"])
    psi, perf = solve(ctx, A, order, r["source"])
    assert np.array_equal(bits(psi), r["want"].view(np.int64)) and perf["converged"] == 1
    order.close(); A.close()


def test_perf_records_are_those_of_the_commit_before_the_unification(O, ffm, ctx):
    want = json.load(open(PERF_GOLDEN))
    got = perf_records(ffm, O, ctx)
    for key in sorted(got):
        print(key, got[key], "recorded", want["records"].get(key))
    assert len(got) == 16 and got == want["records"]
    assert all(float.fromhex(a) > 0 and float.fromhex(a) > float.fromhex(b) >= 0 for a, b in got.values())


def test_the_order_of_a_matrix_of_another_size_is_refused_and_psi_untouched(O, ffm, ctx):
    k, k2 = case(ffm, O, "box"), case(ffm, O, "w8")
    assert k["N"] != k2["N"]
    r, r2 = k["rays"][0], k2["rays"][0]
    A = ffm.lduMatrix(ctx, k["N"], k["l"], k["u"]).set_coeffs(r["diag"], r["upper"], r["lower"])
    B = ffm.lduMatrix(ctx, k2["N"], k2["l"], k2["u"]).set_coeffs(r2["diag"], r2["upper"], r2["lower"])
    order = A.flow_order()
    start = O.hash_u(8, np.arange(k2["N"]))
    psi = ctx.to_device(start)
    with pytest.raises(ffm.FfmError, match=r"\(-5\)"):
        B.solve_ordered(order, psi, ctx.to_device(r2["source"]))
    assert np.array_equal(bits(psi), start.view(np.int64))
    order.close(); A.close(); B.close()


def test_a_laplacian_has_no_flow_order(O, ffm, ctx):
    k = case(ffm, O, "box")
    A = ffm.lduMatrix(ctx, k["N"], k["l"], k["u"])
    diag, up, lo = laplacian_like(O, k["N"], k["l"], k["u"], asym=0.3)
    A.set_coeffs(diag, up, lo)
    with pytest.raises(ffm.FfmError, match=r"\(-5\).*cycle"):
        A.flow_order()
    A.close()


def test_a_matrix_with_ghost_cells_is_refused(O, ffm, ctx):
    k = case(ffm, O, "box")
    N = k["N"]
    assert not np.any(k["l"] == N - 1)                               # the last cell owns no face: it can stand in as a ghost cell
    l, u = np.ascontiguousarray(k["l"], np.int32), np.ascontiguousarray(k["u"], np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    A = ffm.lduMatrix.__new__(ffm.lduMatrix)                        # the binding's constructor goes through ffm_ldu_create_hint
    A.ctx, A.h, A.nOwned, A.nCells, A.nFaces = ctx, C.c_void_p(), N - 1, N, len(l)
    assert ffm.lib().ffm_ldu_create_ext(ctx.h, N - 1, 1, len(l), ip(l), ip(u), C.byref(A.h)) == 0
    r = k["rays"][0]
    A.set_coeffs(r["diag"], r["upper"], r["lower"])
    with pytest.raises(ffm.FfmError, match=r"\(-5\).*single rank"):
        A.flow_order()
    A.close()
