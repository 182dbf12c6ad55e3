"""The flow-ordered exact solve (csrc/ffm_solve.hip: ffm_flow_order_create, ffm_solve_ordered_d) on upwind ray matrices
(tests/ray_matrix.py): psi is BITWISE the serial forward substitution restated in tests/ray_matrix.py -- no tolerance, the
arithmetic is fully specified -- on a box of two chunks of 256 positions in the library's numbering and in a random one, on
polyhedral meshes of every row-width bucket above a hex's and on the steckler room; for four rays of different octants and
(1,0,0).  Orders are reused and swapped on one matrix handle; an order that does not fit the matrix, a matrix that is not
triangular and a decomposed matrix are refused before any sweep is launched."""
import ctypes as C
import heapq

import numpy as np
import pytest

import ray_matrix as R
from common import laplacian_like

pytestmark = pytest.mark.gpu

CASES = ["box", "box_random", "w8", "w16u14", "w32l30", "w32multi", "steckler"]
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
