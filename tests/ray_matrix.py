"""Upwind ray matrices on the test meshes (a helper, not a test): the implicit part of a discrete-ordinates ray equation
fvm::div(Ji, Ii) + fvm::Sp(k omega, Ii) with Ji = Sf & d, discretised `upwind`, as LDU coefficients

    upper = min(Ji, 0)        lower = -max(Ji, 0)        diag = sum of the cell's outflow over its internal faces + k omega V

so that on every face at most one of upper, lower is non-zero.  Shared by tests/test_flow_order_cpu.py and
tests/test_solve_ordered_gpu.py, with the restatements both check against: Kahn's levels and the serial forward substitution."""
import numpy as np

ABSORPTION = 0.3


def directions():
    """[(name, d, omega)]: the 32 dAve of nPhi 2, nTheta 4 and (1,0,0), along which the transverse faces carry no coefficient"""
    from oracle import fvdom
    out = [("ray%02d" % i, dAve, omega) for i, (_, dAve, omega) in enumerate(fvdom.ray_set(2, 4))]
    out.append(("x", np.array([1.0, 0.0, 0.0]), 1.0))
    return out


def octant(d):
    return int(d[0] < 0) | int(d[1] < 0) << 1 | int(d[2] < 0) << 2


def five_directions():
    """four of the 32 rays from different octants (the first ray of the octants 0, 3, 5, 6) plus (1,0,0)"""
    D = directions()
    return [next(x for x in D[:32] if octant(x[1]) == o) for o in (0, 3, 5, 6)] + [D[32]]


def mesh(name):
    """the named test mesh: a merged_mesh.CASES name, box7x8x6, box14x18x1 (z empty) or steckler (with its baffles)"""
    import merged_mesh
    from oracle import plume, steckler
    if name in merged_mesh.CASES:
        return merged_mesh.case(name)
    if name == "box7x8x6":
        return plume.make_mesh((7, 8, 6))
    if name == "box14x18x1":
        return plume.make_mesh((14, 18, 1), empty=("zmin", "zmax"))
    if name == "steckler":
        return steckler.build_mesh()
    raise KeyError(name)


def ray_matrix(m, d, omega):
    """(diag, upper, lower) of the ray along d on mesh m"""
    Ji = (d[0] * m.Sf[:, 0] + d[1] * m.Sf[:, 1]) + d[2] * m.Sf[:, 2]
    upper, lower = np.minimum(Ji, 0.0), -np.maximum(Ji, 0.0)
    diag = ABSORPTION * omega * m.V
    np.add.at(diag, m.l, np.maximum(Ji, 0.0))
    np.add.at(diag, m.u, np.maximum(-Ji, 0.0))
    return diag, upper + 0.0, lower + 0.0          # (+ 0.0: no negative zeros)


def edges(l, u, upper, lower):
    """(src, dst): row dst needs cell src"""
    lo, up = lower != 0, upper != 0
    return np.concatenate([l[lo], u[up]]), np.concatenate([u[lo], l[up]])


def kahn_levels(N, src, dst):
    """Kahn's algorithm by levels: (level of every cell or -1, number of levels, acyclic)"""
    indeg = np.bincount(dst, minlength=N)
    by = np.argsort(src, kind="stable")
    succ = dst[by]
    start = np.searchsorted(src[by], np.arange(N + 1))
    lev = np.full(N, -1)
    frontier = np.nonzero(indeg == 0)[0]
    k = done = 0
    while len(frontier):
        lev[frontier] = k
        done += len(frontier)
        cnt = start[frontier + 1] - start[frontier]
        idx = np.repeat(start[frontier] - (np.cumsum(cnt) - cnt), cnt) + np.arange(cnt.sum())
        s = succ[idx]
        np.subtract.at(indeg, s, 1)
        frontier = np.unique(s[indeg[s] == 0])
        k += 1
    return lev, k, done == N


def forward_substitution(N, l, u, diag, upper, lower, source, order):
    """the serial solve in `order`: per row the lower faces, then the upper faces, in face order, zero coefficients skipped, one
    division -- plain Python floats, one rounding per operation"""
    lof, upf = [[] for _ in range(N)], [[] for _ in range(N)]
    for f in range(len(l)):
        upf[l[f]].append(f)
        lof[u[f]].append(f)
    l, u, diag, upper, lower, source = (a.tolist() for a in (l, u, diag, upper, lower, source))
    psi = [float("nan")] * N
    for c in (int(c) for c in order):
        val = source[c]
        for f in lof[c]:
            if lower[f] != 0.0:
                val -= lower[f] * psi[l[f]]
        for f in upf[c]:
            if upper[f] != 0.0:
                val -= upper[f] * psi[u[f]]
        psi[c] = val / diag[c]
    return np.array(psi)
