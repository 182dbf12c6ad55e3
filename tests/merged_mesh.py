"""Polyhedral test meshes with rows wider than a hex cell's (a helper, not a test).

merged(n, bars, bars_first, h) takes the hex box of oracle.plume.make_mesh(n, h) (patches inlet, floor, top, sides) and merges runs
of fine cells along x into single cells: a bar (i0, j, k, L) turns the cells (i0..i0+L-1, j, k) into one box-shaped cell with hanging
nodes, a polyhedron with 4L+2 faces.  The result is duck-typed like oracle.fv.HexMesh for everything oracle/fv.py uses.

  cells       V = sum V, C = sum V*C / sum V
  faces       one face per pair of merged cells: Sf = sum of the fine area vectors (owner -> neighbour), Cf area-weighted;
              sorted upper-triangular by (l, u)
  factors     weights, deltaCoeffs (nonOrthDeltaCoeffs with the 0.05 clamp) and nonOrthCorrectionVectors as oracle.fv.shear makes them
  patches     the fine boundary faces (a merged cell has several faces on one patch), deltaCoeffs = 1/(n & (Cf - C))
  numbering   bars_first: the bars, then the unit cells in natural order (wide upper rows); otherwise the bars come last (wide lower
              rows)

CASES are the named meshes of the GPU tests with the widths (max upper, max lower faces of a cell) and the row-width bucket of
FFM_DISPATCH_W (csrc/ffm_device.hpp) they were built for; tests/test_merged_mesh_cpu.py checks them without a GPU.  Each has one
wide row among rows of 3 or 4 in a mesh of 2 to 4 slices of 64 cells: non-uniform slice widths, nearly all slots padding."""
import numpy as np

# name: (n, bars, bars_first, cells, max upper, max lower, bucket)
CASES = {
    "w4": ((6, 5, 1), [(2, 2, 0, 1)], True, 30, 4, 3, 4),
    "w8": ((5, 5, 4), [(2, 2, 2, 1)], True, 100, 6, 4, 8),
    "w16u10": ((6, 5, 4), [(2, 2, 2, 2)], True, 119, 10, 4, 16),
    "w16u14": ((6, 5, 4), [(1, 2, 2, 3)], True, 118, 14, 4, 16),
    "w32l18": ((7, 5, 4), [(1, 2, 2, 4)], False, 137, 4, 18, 32),
    "w32u18": ((7, 5, 4), [(1, 2, 2, 4)], True, 137, 18, 4, 32),                # owner slots 16 and 17: five-bit slot field of the lower entries
    "w32l30": ((9, 5, 4), [(1, 2, 2, 7)], False, 174, 4, 30, 32),
    "w32multi": ((9, 5, 5), [(1, 2, 2, 7), (1, 2, 3, 7), (1, 1, 1, 3)], False, 211, 4, 24, 32),      # bars adjacent to bars
}
# meshes the library refuses: more than 32 faces on one side, upper or lower
REFUSED = {
    "u34": ((10, 5, 4), [(1, 2, 2, 8)], True, 193, 34, 4, None),
    "l34": ((10, 5, 4), [(1, 2, 2, 8)], False, 193, 4, 34, None),
}


def bucket(maxW):
    """the row width FFM_DISPATCH_W instantiates for a mesh whose widest row (lower or upper) has maxW faces"""
    return next(W for W in (3, 4, 8, 16, 32) if maxW <= W)


def widths(l, u):
    """(max upper, max lower) faces of a cell"""
    return int(np.bincount(l).max()), int(np.bincount(u).max())


class MergedMesh:
    def patch(self, name):
        return next(p for p in self.patches if p.name == name)


def merged(n, bars, bars_first, h=0.1):
    from oracle import fv, plume
    f = plume.make_mesh(n, h)
    nx, ny, nz = n
    N0 = f.nCells
    bar_of = np.full(N0, -1)
    for b, (i0, j, k, L) in enumerate(bars):
        assert 0 <= i0 and i0 + L <= nx and L >= 1
        cells = np.arange(i0, i0 + L) + nx * (j + ny * k)
        assert (bar_of[cells] == -1).all(), "bars overlap"
        bar_of[cells] = b
    unit = np.nonzero(bar_of < 0)[0]                         # natural order
    nb, nu = len(bars), len(unit)
    g = np.empty(N0, np.int64)                               # fine cell -> merged cell
    g[unit] = np.arange(nu) + (nb if bars_first else 0)
    g[bar_of >= 0] = bar_of[bar_of >= 0] + (0 if bars_first else nu)
    N = nb + nu
    m = MergedMesh()
    m.nCells = N
    m.fine, m.cellMap = f, g
    m.V = np.zeros(N); np.add.at(m.V, g, f.V)
    VC = np.zeros((N, 3)); np.add.at(VC, g, f.V[:, None] * f.C)
    m.C = VC / m.V[:, None]
    # internal faces: one per pair of merged cells
    gl, gu = g[f.l], g[f.u]
    keep = gl != gu
    gl, gu, Sf, Cf, mag = gl[keep], gu[keep], f.Sf[keep], f.Cf[keep], f.magSf[keep]
    flip = gl > gu
    lo, hi = np.where(flip, gu, gl), np.where(flip, gl, gu)
    Sf = np.where(flip[:, None], -Sf, Sf)
    pairs, inv = np.unique(lo * N + hi, return_inverse=True)           # sorted by (l, u)
    F = len(pairs)
    m.nFaces = F
    m.l, m.u = pairs // N, pairs % N
    m.Sf = np.zeros((F, 3)); np.add.at(m.Sf, inv, Sf)
    area = np.zeros(F); np.add.at(area, inv, mag)
    aC = np.zeros((F, 3)); np.add.at(aC, inv, mag[:, None] * Cf)
    m.Cf = aC / area[:, None]
    m.sumMagSf = area                                         # == magSf where the merged face is planar
    m.magSf = np.linalg.norm(m.Sf, axis=1)
    # interpolation factors: oracle.fv.shear's expressions
    own = np.abs(np.einsum("fd,fd->f", m.Sf, m.Cf - m.C[m.l]))
    nei = np.abs(np.einsum("fd,fd->f", m.Sf, m.C[m.u] - m.Cf))
    m.weights = nei / (own + nei)
    d = m.C[m.u] - m.C[m.l]
    nf = m.Sf / m.magSf[:, None]
    m.deltaCoeffs = 1.0 / np.maximum(np.einsum("fd,fd->f", nf, d), 0.05 * np.linalg.norm(d, axis=1))
    m.nonOrthCorrectionVectors = nf - d * m.deltaCoeffs[:, None]
    # patches: the fine boundary faces
    m.patches = []
    for p in f.patches:
        fc = g[p.faceCells]
        nfb = p.Sf / p.magSf[:, None]
        m.patches.append(fv.Patch(p.name, fc, p.Sf, p.Cf, 1.0 / np.einsum("fd,fd->f", nfb, p.Cf - m.C[fc])))
    return m


def case(name, h=0.1):
    n, bars, first = {**CASES, **REFUSED}[name][:3]
    return merged(n, bars, first, h)


def renumbered(m, cOrd, fOrd):
    """m with its cells and faces in the new->old orders cOrd, fOrd (what ffm.renumber_levels returns): the mesh the library is given.
    A row's faces then come in the order of the NEW numbering, which is the reference's face loop on that mesh -- on a hex box the
    level order keeps the relative order of a cell's three lower and three upper neighbours, around a bar it does not, so an oracle run
    on the original numbering would add a wide row's terms in another order than any implementation given the renumbered mesh."""
    from oracle import fv
    oldToNew = np.empty(m.nCells, np.int64); oldToNew[cOrd] = np.arange(m.nCells)
    r = MergedMesh()
    r.nCells, r.nFaces = m.nCells, m.nFaces
    r.l, r.u = oldToNew[m.l[fOrd]], oldToNew[m.u[fOrd]]
    assert np.all(r.l < r.u) and np.all(np.diff(r.l * r.nCells + r.u) > 0)
    r.V, r.C = m.V[cOrd], m.C[cOrd]
    for k in ("Sf", "Cf", "magSf", "sumMagSf", "weights", "deltaCoeffs", "nonOrthCorrectionVectors"):
        setattr(r, k, getattr(m, k)[fOrd])
    r.patches = [fv.Patch(p.name, oldToNew[p.faceCells], p.Sf, p.Cf, p.deltaCoeffs) for p in m.patches]
    return r


def device_mesh(ffm, ctx, m, face_centres=False):
    """the fixture of the operator tests: the library's cell order, lduMatrix and fvMesh of m (a HexMesh, or a merged mesh, which also gets
    its non-orthogonal correction vectors and is handed back renumbered: see renumbered()); returns a dict with the handles, the
    oracle's mesh `m`, the new->old orders from m to the device's numbering and the widths of the addressing the library was given"""
    N, F = m.nCells, m.nFaces
    cOrd, fOrd = ffm.renumber_levels(N, m.l, m.u)
    if isinstance(m, MergedMesh):
        m = renumbered(m, cOrd, fOrd)
        cOrd, fOrd = np.arange(N, dtype=np.int32), np.arange(F, dtype=np.int32)
    l2, u2, oldToNew = ffm.hexmesh.apply_renumbering(N, m.l, m.u, cOrd, fOrd)
    A = ffm.lduMatrix(ctx, N, l2, u2)
    assert A.native_order
    patches = [(oldToNew[p.faceCells].astype(np.int32), p.Sf.T.copy(), p.deltaCoeffs) for p in m.patches]
    mesh = ffm.fvMesh(A, m.V[cOrd], m.C[cOrd].T.copy(), m.Sf[fOrd].T.copy(), m.magSf[fOrd], m.weights[fOrd], m.deltaCoeffs[fOrd], patches)
    if hasattr(m, "nonOrthCorrectionVectors"):
        mesh.set_nonorth_correction(m.nonOrthCorrectionVectors[fOrd].T.copy())
    if face_centres:
        mesh.set_face_centres(m.Cf[fOrd].T.copy())
    wu, wl = widths(l2, u2)
    return dict(m=m, A=A, mesh=mesh, cOrd=cOrd, fOrd=fOrd, N=N, F=F, B=sum(p.size for p in m.patches), l=l2, u=u2, wu=wu, wl=wl,
                W=bucket(max(wu, wl)))
