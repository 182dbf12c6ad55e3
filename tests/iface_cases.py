"""Decomposed matrices in OpenFOAM's processor-interface form (ffm_ldu_set_interfaces: faceCells, interfaceBouCoeffs,
interfaceIntCoeffs, neighbProcNo per processor patch) and an exchange that needs no second process -- shared by
tests/test_ldu_interfaces_cpu.py (the oracle's ranks against the global operator) and tests/test_ldu_interfaces_gpu.py (the
device's ranks against the oracle's, bit for bit).

Every case is one global matrix, a decomposition and, per rank, the LDU of the owned cells alone plus its patches.  A rank
also knows the GLOBAL labels of the cells behind each patch, so what the neighbour ranks would send of a global vector x is
x[nbrCells[p]]: one process can then run every rank one after the other."""
import numpy as np

import common
import merged_mesh
import part_cases

CASES = ("blocks222", "dag4g", "dag2r", "w32multi3", "slab")


class Rank:
    """one rank: nOwned, l, u, diag, upper, lower (None: symmetric), gcell [nOwned] and per patch faceCells, bou, int_ (None:
    = bou), nbrRank, nbrCells (global labels of the cells on the far side, face by face)"""

    def __init__(self, rank, world, gcell, l, u, diag, upper, lower, faceCells, bou, int_, nbrRank, nbrCells):
        self.rank, self.world, self.gcell = rank, world, np.asarray(gcell, np.int64)
        self.nOwned, self.l, self.u = len(self.gcell), np.ascontiguousarray(l, np.int32), np.ascontiguousarray(u, np.int32)
        self.diag, self.upper, self.lower = diag, upper, lower
        self.faceCells = [np.ascontiguousarray(a, np.int32) for a in faceCells]
        self.bou, self.int_ = bou, int_
        self.nbrRank, self.nbrCells = [int(r) for r in nbrRank], [np.asarray(a, np.int64) for a in nbrCells]

    def patches_per_cell(self):
        """[nOwned]: in how many patches a cell lies"""
        n = np.zeros(self.nOwned, int)
        for fc in self.faceCells:
            n[np.unique(fc)] += 1
        return n

    def oracle(self, O, N):
        A = O.Ldu(self.nOwned, self.l, self.u).set_coeffs(self.diag, self.upper, self.lower)
        A.set_interfaces(self.faceCells, self.bou, self.int_)
        return A.set_global_cells(N)

    def device(self, ffm, ctx, N):
        A = ffm.lduMatrix(ctx, self.nOwned, self.l, self.u).set_coeffs(self.diag, self.upper, self.lower)
        return A.set_interfaces(self.faceCells, self.bou, self.nbrRank, intCoeffs=self.int_, globalCells=N)


class Case:
    """N global cells, ranks [Rank or None (a rank the case does not build)], glob = (l, u, diag, upper, lower) or None"""

    def __init__(self, name, N, ranks, glob):
        self.name, self.N, self.ranks, self.glob, self.world = name, N, ranks, glob, len(ranks)

    def global_oracle(self, O):
        l, u, diag, up, lo = self.glob
        return O.Ldu(self.N, l, u).set_coeffs(diag, up, lo)


class Exchange:
    """The exchange of one rank inside one process: the neighbours' values of the global vector self.x.  Counts its calls and
    keeps the last send buffer (patch after patch).  oracle_fn(O) / device_fn() wrap it for the two callers."""

    def __init__(self, rank, x=None):
        self.rank, self.x, self.calls, self.sent, self.sizes, self.ranks = rank, x, 0, None, None, None

    def _recv(self, sizes):
        assert list(sizes) == [len(a) for a in self.rank.nbrCells], (list(sizes), [len(a) for a in self.rank.nbrCells])
        self.calls += 1
        self.sizes = list(sizes)
        return [np.asarray(self.x, np.float64)[a] for a in self.rank.nbrCells]

    def oracle_fn(self, O):
        def fn(user, nIf, size, send, recv):
            sizes = [size[p] for p in range(nIf)]
            self.sent = np.concatenate([np.ctypeslib.as_array(send[p], shape=(sizes[p],)).copy() if sizes[p] else np.zeros(0) for p in range(nIf)]) if nIf else np.zeros(0)
            for p, vals in enumerate(self._recv(sizes)):
                if sizes[p]:
                    np.ctypeslib.as_array(recv[p], shape=(sizes[p],))[:] = vals
        return O.EXCHANGE_FN(fn)

    def oracle_comm(self, O):
        """the O.Comm of the rank (keep the returned tuple alive as long as the matrix uses it)"""
        cb = (O.ALLREDUCE_FN(lambda user, vals, n: None), self.oracle_fn(O))
        return O.Comm(None, self.rank.rank, self.rank.world, cb[0], cb[1]), cb

    def device_fn(self):
        def fn(sizes, ranks, offs, send, recv):
            self.sent, self.ranks = np.array(send, np.float64, copy=True), list(ranks)
            assert list(offs) == np.concatenate(([0], np.cumsum(sizes)))[:-1].astype(int).tolist()
            for p, vals in enumerate(self._recv(sizes)):
                recv[offs[p]:offs[p] + sizes[p]] = vals
        return fn

    @staticmethod
    def allreduce(a, op):       # one process: the sums are taken over this rank alone
        pass


def _from_blocks(ffm, name, glob, grid, only=None):
    H = ffm.hexmesh
    blocks, nbr = H.decompose(glob, grid)
    itfs = [b.interfaces() for b in blocks]
    ranks = []
    for r, blk in enumerate(blocks):
        if only is not None and r not in only:
            ranks.append(None)
            continue
        s = H.synth_p_rgh(blk)
        nbrCells = []
        for itf, nr in zip(itfs[r], nbr[r]):
            # the neighbour block's interface with the same global faces: same direction, the other side, same (global face) order
            other = next(o for o in itfs[nr] if o["dir"] == itf["dir"] and o["side"] != itf["side"] and np.array_equal(o["gface"], itf["gface"]))
            nbrCells.append(blocks[nr].gcell[other["faceCells"]])
        ranks.append(Rank(r, len(blocks), blk.gcell, blk.l, blk.u, s["diag"], s["upper"], None, [i["faceCells"] for i in itfs[r]], s["bouCoeffs"], None,
                          nbr[r], nbrCells))
    N = int(np.prod(glob))
    g = None
    if only is None:
        whole = H.HexBlock(glob)
        sg = H.synth_p_rgh(whole)
        g = (whole.l, whole.u, sg["diag"], sg["upper"], None)
    return Case(name, N, ranks, g)


def _from_partition(ffm, name, N, l, u, diag, up, lo, part, world):
    ranks = []
    for r in range(world):
        sub = ffm.decompose.SubDomain(N, l, u, part, world, r)
        keep, pat = sub.interface_form(up, lo)
        d, upl, lol = sub.coeffs(diag, up, lo)
        int_, nbrCells = None if lo is None else [], []
        for q in range(len(sub.nbrRank)):
            s, e = sub.cutStart[q], sub.cutStart[q + 1]
            gf, fl = sub.cutFace[s:e], sub.cutFlip[s:e].astype(bool)
            if lo is not None:          # interfaceIntCoeffs: the cut face's coefficient in the NEIGHBOUR cell's row (what bou is, upper and lower swapped)
                int_.append(-np.where(fl, np.asarray(up)[gf], np.asarray(lo)[gf]))
            own = sub.gcell[sub.cutCell[s:e]]
            nbrCells.append(np.where(l[gf] == own, u[gf], l[gf]))       # the far end of every cut face
        ranks.append(Rank(r, world, sub.gcell[:sub.nOwned], sub.l[keep], sub.u[keep], d[:sub.nOwned], upl[keep], None if lol is None else lol[keep],
                          [p[0] for p in pat], [p[1] for p in pat], int_, sub.nbrRank, nbrCells))
    return Case(name, N, ranks, (l, u, diag, up, lo))


_cache = {}


def build(O, ffm, name):
    """the case `name`, built once per process"""
    if name in _cache:
        return _cache[name]
    if name == "blocks222":
        c = _from_blocks(ffm, name, (6, 5, 4), (2, 2, 2))
    elif name == "slab":
        # only the middle block is built: 520 x 512 cells, each in two patches (-z and +z)
        c = _from_blocks(ffm, name, (520, 512, 3), (1, 1, 3), only=(1,))
    elif name in ("dag4g", "dag2r"):
        N, l, u, centres, diag, up, lo, source = part_cases.build(O, "dag_random", asym=0.3)
        world, partitioner = (4, "graph") if name == "dag4g" else (2, "rcb")
        part = part_cases.partition(ffm, partitioner, N, l, u, centres, world)
        c = _from_partition(ffm, name, N, l, u, diag, up, lo, part, world)
    elif name == "w32multi3":
        m = merged_mesh.case("w32multi")
        N, l, u = m.nCells, m.l.astype(np.int32), m.u.astype(np.int32)
        diag, up, lo = common.laplacian_like(O, N, l, u, seed=3, asym=0.3, shift=0.05)
        # three parts: with two, every rank has one patch and no cell can lie in two; the graph partitioner leaves a row of 19 faces
        # whole (the W = 32 instantiation of the row kernels), coordinate bisection cuts the wide rows down to 10
        part = part_cases.partition(ffm, "graph", N, l, u, m.C, 3)
        c = _from_partition(ffm, name, N, l, u, diag, up, lo, part, 3)
    else:
        raise ValueError(name)
    _cache[name] = c
    return c


def vectors(O, N):
    """x and b of the row operations: hashed, not of one sign"""
    return 2 * O.hash_u(0xF4, np.arange(N)) - 0.7, O.hash_u(0xF3, np.arange(N))
