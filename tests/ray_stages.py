"""Stages of an upwind ray matrix on a decomposed mesh (a helper, not a test): the restatement on the merged mesh that
tests/test_flow_stages_cpu.py and tests/test_solve_ordered_decomposed_gpu.py check ffm_flow_stages and
ffm_flow_order_create_staged against, the fixpoint over simulated ranks in one process, and the stage-by-stage forward substitution
of one rank's rows."""
import numpy as np

import ray_matrix as R


def merged_stages(N, l, u, upper, lower, part):
    """stage of every cell of the merged mesh: the largest number of rank crossings (part[src] != part[dst]) on any upstream path,
    taken level by level over Kahn's order"""
    src, dst = R.edges(l, u, upper, lower)
    lev, nLev, acyclic = R.kahn_levels(N, src, dst)
    assert acyclic
    cross = (np.asarray(part)[src] != np.asarray(part)[dst]).astype(np.int64)
    by = np.argsort(lev[src], kind="stable")
    src, dst, cross = src[by], dst[by], cross[by]
    start = np.searchsorted(lev[src], np.arange(nLev + 1))
    stage = np.zeros(N, np.int64)
    for k in range(nLev):                      # every edge into a cell of level k leaves a cell of a lower level: src is final
        s = slice(start[k], start[k + 1])
        np.maximum.at(stage, dst[s], stage[src[s]] + cross[s])
    return stage


def fixpoint(ffm, subs, coeffs, maxRounds=None):
    """ffm.flow_stages per simulated rank with the ghost stages carried between the ranks in numpy until nothing changes (or, with
    maxRounds, until a stage exceeds the ghost cells of all ranks: returns None then).
    subs: decompose.SubDomain per rank; coeffs: (upper, lower) per rank on the rank's faces.
    Returns (per rank (stage, order, nLevels), rounds)."""
    totalGhost = sum(s.nGhost for s in subs)
    ghost = [np.zeros(s.nGhost, np.int32) for s in subs]
    glob = np.zeros(subs[0].globalCells, np.int64)
    rounds = 0
    while True:
        rounds += 1
        out = [ffm.flow_stages(s.nOwned, s.nGhost, s.l, s.u, up, lo, g) for s, (up, lo), g in zip(subs, coeffs, ghost)]
        for s, (stage, _, _) in zip(subs, out):
            glob[s.gcell[:s.nOwned]] = stage
        new = [glob[s.gcell[s.nOwned:]].astype(np.int32) for s in subs]
        changed = any(not np.array_equal(a, b) for a, b in zip(new, ghost))
        ghost = new
        if glob.max() > totalGhost:
            return None, rounds
        if not changed:
            return out, rounds
        assert maxRounds is None or rounds < maxRounds


def staged_substitution(nOwned, l, u, diag, upper, lower, source, psi, order):
    """one rank's rows recomputed in `order` from the ghost entries psi holds: per row the lower, then the upper faces in the rank's
    face order, zero coefficients skipped, one division -- plain Python floats.  By induction over the stages this is the whole
    algorithm: a row of stage s reads owned cells recomputed before it and ghost cells of a stage < s, whose final values are
    the ones a neighbour's stage-(< s) sweep produced.  Returns psi's owned entries."""
    lof, upf = [[] for _ in range(nOwned)], [[] for _ in range(nOwned)]
    for f in range(len(l)):
        if l[f] < nOwned:
            upf[l[f]].append(f)
        if u[f] < nOwned:
            lof[u[f]].append(f)
    l, u, diag, upper, lower, source = (np.asarray(a).tolist() for a in (l, u, diag, upper, lower, source))
    val = np.asarray(psi).tolist()
    for c in range(nOwned):
        val[c] = float("nan")
    for c in (int(c) for c in order):
        v = source[c]
        for f in lof[c]:
            if lower[f] != 0.0:
                v -= lower[f] * val[l[f]]
        for f in upf[c]:
            if upper[f] != 0.0:
                v -= upper[f] * val[u[f]]
        val[c] = v / diag[c]
    return np.array(val[:nOwned])
