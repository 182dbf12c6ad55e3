"""The cases of tests/iface_cases.py without a device: the oracle's ranks in OpenFOAM's processor-interface form, fed by the
in-process exchange, assemble the global operator (Amul, Tmul, residual, sumA gathered over the ranks against the global
O.Ldu at rel-L2 1e-14, the bar of tests/test_partition_gpu.py) -- so the reference side of tests/test_ldu_interfaces_gpu.py is
right -- and the decompositions have the shapes those tests rely on."""
import numpy as np
import pytest

import iface_cases as IC
from common import rel_l2


@pytest.mark.parametrize("name", [n for n in IC.CASES if n != "slab"])
def test_oracle_ranks_assemble_the_global_operator(O, ffm, name):
    case = IC.build(O, ffm, name)
    G = case.global_oracle(O)
    x, b = IC.vectors(O, case.N)
    ref = {"amul": G.amul(x), "tmul": G.tmul(x), "residual": G.residual(x, b), "sumA": G.sumA()}
    got = {k: np.full(case.N, np.nan) for k in ref}
    for rk in case.ranks:
        A = rk.oracle(O, case.N)
        ex = IC.Exchange(rk, x)
        A.comm, keep = ex.oracle_comm(O)
        xl, bl = x[rk.gcell], b[rk.gcell]
        got["amul"][rk.gcell] = A.amul(xl)
        assert np.array_equal(ex.sent, np.concatenate([xl[fc] for fc in rk.faceCells]))
        got["tmul"][rk.gcell] = A.tmul(xl)
        got["residual"][rk.gcell] = A.residual(xl, bl)
        assert ex.calls == 3
        got["sumA"][rk.gcell] = A.sumA()
        assert ex.calls == 3
    for k in ref:
        assert rel_l2(got[k], ref[k]) < 1e-14, (k, rel_l2(got[k], ref[k]))
    if case.glob[4] is not None:        # the transpose is another operator, and the interface terms are part of the difference
        assert rel_l2(ref["tmul"], ref["amul"]) > 1e-3
        assert any(not np.array_equal(i, b_) for rk in case.ranks for i, b_ in zip(rk.int_, rk.bou))


def test_decompositions_have_the_shapes_the_device_tests_rely_on(O, ffm):
    cases = {n: IC.build(O, ffm, n) for n in IC.CASES if n != "slab"}
    most = lambda c: max(int(rk.patches_per_cell().max()) for rk in c.ranks)
    for n in ("blocks222", "dag4g", "w32multi3"):
        assert most(cases[n]) >= 2, n
    # every block of the 2 x 2 x 2 grid has a corner cell in three patches
    assert all(int(rk.patches_per_cell().max()) == 3 and len(rk.faceCells) == 3 for rk in cases["blocks222"].ranks)
    d4 = cases["dag4g"]
    assert any(np.bincount(fc).max() >= 2 for rk in d4.ranks for fc in rk.faceCells)          # a cell with two faces in one patch
    assert any(len({len(fc) for fc in rk.faceCells}) >= 2 for rk in d4.ranks)                 # patches of different sizes
    assert any(len(rk.nbrRank) >= 3 for rk in d4.ranks)
    for n in ("dag4g", "dag2r"):
        for rk in cases[n].ranks:
            cOrd, _ = ffm.renumber_levels(rk.nOwned, rk.l, rk.u)
            assert not np.array_equal(cOrd, np.arange(rk.nOwned)), (n, rk.rank)                 # the library renumbers the rank
    assert merged_mesh_rows(cases["w32multi3"]) >= 17
    for c in cases.values():
        assert sorted(np.concatenate([rk.gcell for rk in c.ranks]).tolist()) == list(range(c.N))
        for rk in c.ranks:
            assert all(len(a) == len(b_) for a, b_ in zip(rk.faceCells, rk.nbrCells)) and len(rk.faceCells) == len(rk.nbrRank)


def merged_mesh_rows(case):
    """the widest row (upper or lower side) any rank of the case keeps"""
    return max(max(np.bincount(rk.l, minlength=1).max(), np.bincount(rk.u, minlength=1).max()) for rk in case.ranks)


def test_slab_middle_block_exceeds_the_halo_kernels_grid_cap(O, ffm):
    """k_halo_pack / k_halo_apply launch at most 1024 blocks of 256 threads: more items, and more boundary cells, than that
    make their grid-stride loops run"""
    rk = IC.build(O, ffm, "slab").ranks[1]
    assert rk.nOwned == 520 * 512 and rk.nOwned > 1024 * 256
    assert sum(len(fc) for fc in rk.faceCells) == 2 * rk.nOwned
    assert int(rk.patches_per_cell().min()) == 2 and rk.nbrRank == [0, 2]
