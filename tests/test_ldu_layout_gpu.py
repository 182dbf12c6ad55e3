"""The handles ffm_ldu_create* makes from the analysis and the layout of csrc/ffm_ldu_analysis.cpp: what their getters report must be what
the library reported before analysis, layout and upload were separated (commit 89df91d, recorded on an MI355X with
`python tests/test_ldu_layout_gpu.py`), and a handle made from what ffm_renumber_hint left behind must be the handle a fresh analysis gives.
The arithmetic on these layouts is held bit for bit by tests/test_ldu_gpu.py."""
import numpy as np
import pytest

import test_ldu_analysis_cpu as LA

pytestmark = pytest.mark.gpu

# (sweep_mode, nLevels, nNative, native_order, SHA-256 of cell_order(), SHA-256 of face_map()), recorded from commit 89df91d
GETTERS = {
    "box_auto": (2, 53, 18048, False, 'db4e2d4c21437de468a779e68c15a35c4b21b0056a645734d6a3cc2ca30c2b68', '19b3be88c14683ac54e2287a96ebdac98cab5c914ebed983cb6eb9cd380e42f8'),
    "hint_baffled": (2, 34, 5184, False, 'e285edf3859d5536ed389126ec84516a5d0d054d8af6b13bc1b482a0b5b65dd8', '76ed5189125613e3ef61774f3b0447d730e9eb9cecf1f4e7bc7a0fd08f85efd8'),
    "wall_split": (2, 38, 12288, False, '6266b1a1f26b9f266c319d01feb050be15f0faf5e8b23a8e063febcceeebff49', 'dc10efa282020166c50964666d4e7aed2eb59a7997d6cb6bc59ea42592f50c86'),
    "w16u14": (0, 13, 1088, False, 'c337a92517a21460a5b5e8d9450457fff1f47c23c23025d4d923271a57976a9a', 'ea2c40df85d2ae80c1cb76cc845add2f7b5a30d29e1264d4028087404d01d508'),
    "w32l30": (0, 16, 768, False, '03dbdc8bf7d70a3aab3f75d1b94a27dbc93f5ddfea7e3f9f025149ccd4ceef45', '35f2db3df3dda5164cca888dd535d24efa9d2003284b0a438837013b5a950efb'),
    "ghost_block": (0, 7, 192, False, '25acac6d520f82d4dd72b6e07a3160f7eaca9e9f5a7ca536bc6a10549555c56e', '8860cfc0ec3e7b38ee732128f43196a7bdc4645a7024e0314385339525f090a3'),
}
CASES = ["box_auto", "hint_baffled", "wall_split", "w16u14", "w32l30", "ghost_block"]


def _build(ffm, name):
    if name in ("w16u14", "w32l30"):              # the merged meshes of tests/merged_mesh.py in their own numbering
        import merged_mesh as MM
        m = MM.case(name)
        return dict(nOwn=m.nCells, nGhost=0, l=m.l.astype(np.int32), u=m.u.astype(np.int32), hint=None, env={})
    return LA._build(ffm, name)


def _getters(ffm, ctx, m):
    with LA._env(m["env"]):
        A = ffm.lduMatrix(ctx, m["nOwn"], m["l"], m["u"], groupHint=m["hint"], nGhost=m["nGhost"])
    try:
        return (A.sweep_mode, A.nLevels, A.nNative, A.native_order, LA._digest(A.cell_order()), LA._digest(A.face_map()))
    finally:
        A.close()


@pytest.mark.parametrize("name", CASES)
def test_getters_are_the_recorded_ones(ffm, ctx, name):
    got = _getters(ffm, ctx, _build(ffm, name))
    assert got == GETTERS[name]


@pytest.mark.parametrize("name", ["hint_baffled", "wall_split"])
def test_handle_from_the_renumbering_memo(ffm, ctx, name):
    """the plume driver's route: renumber with a hint, renumber the mesh, create the matrix on it with the renumbered hint.
    (No getter tells whether a handle came from the memo; the test holds what matters: with or without it the handle is the same.)"""
    m = LA._build(ffm, name)
    N = m["nOwn"]
    cOrd, fOrd = ffm.renumber_levels(N, m["l"], m["u"], groupHint=m["hint"])
    l2, u2, _ = ffm.hexmesh.apply_renumbering(N, m["l"], m["u"], cOrd, fOrd)
    hint2 = np.asarray(m["hint"])[cOrd]
    A = ffm.lduMatrix(ctx, N, l2, u2, groupHint=hint2)                # takes the analysis the renumbering left behind
    # an unrelated hinted renumbering empties the slot: the second handle comes from a fresh analysis of the same arrays
    n3, l3, u3 = ffm.hexmesh.hex_ldu(3, 3, 3)
    ffm.renumber_levels(n3, l3, u3, groupHint=np.arange(n3) % 2)
    B = ffm.lduMatrix(ctx, N, l2, u2, groupHint=hint2)
    try:
        assert A.native_order and B.native_order
        assert A.sweep_mode == B.sweep_mode == 2
        assert A.nLevels == B.nLevels and A.nNative == B.nNative
        assert np.array_equal(A.face_map(), B.face_map())
    finally:
        A.close(); B.close()


if __name__ == "__main__":
    ffm = LA._ffm()
    ctx = ffm.Context(0)
    print("GETTERS = {")
    for name in CASES:
        print('    "%s": %r,' % (name, _getters(ffm, ctx, _build(ffm, name))))
    print("}")
    ctx.close()
