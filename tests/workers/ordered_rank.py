"""One rank of the staged flow-ordered solves (ffm_flow_order_create_staged, ffm_solve_ordered_staged_d) on a mesh partitioned by the
product's partitioner, all ranks sharing cuda:0 through the host (gloo) transport: tests/test_solve_ordered_decomposed_gpu.py.
For each of the five directions of tests/ray_matrix.py: the staged order, one solve from a NaN-laced start value, the rank's rows
recomputed in numpy from the ghost entries psi holds afterwards, the exchange callback's calls during the solve; for the first
direction also the collective refusal: rank 0 alone holds the opposite ray's coefficients.
usage: ordered_rank.py rank world port mesh partitioner outdir"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ffm_import import ffm  # noqa: E402
from oracle import oracle as O  # noqa: E402   (hash only)
import ray_matrix as R  # noqa: E402
import ray_stages as S  # noqa: E402

rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
meshName, partitioner, outdir = sys.argv[4], sys.argv[5], sys.argv[6]
gloo = ffm.gloo_comm
gloo.init(rank, world, port)
m = R.mesh(meshName)
N = m.nCells
l, u = np.asarray(m.l, np.int64), np.asarray(m.u, np.int64)
part = ffm.decompose.partition_rcb(m.C, world) if partitioner == "rcb" else ffm.decompose.partition_graph(N, l, u, world)
sub = ffm.decompose.SubDomain(N, l, u, part, world, rank)
nOwn, nLoc = sub.nOwned, sub.nOwned + sub.nGhost
calls = [0]


def counted_exchange(ranks, sends, recvs):
    calls[0] += 1
    gloo.exchange_var(ranks, sends, recvs)


ctx = ffm.Context(0)
ctx.comm_init_host(rank, world, gloo.allreduce, gloo.exchange, counted_exchange)
A = ffm.lduMatrix(ctx, nOwn, sub.l, sub.u, nGhost=sub.nGhost)
A.set_ghost_exchange(sub.nbrRank, sub.sendCount, sub.sendCells, sub.recvCount, tags=sub.tags, globalCells=N)
bits = lambda a: np.ascontiguousarray(a).view(np.int64)
out = dict(gcell=sub.gcell[:nOwn], nGhost=sub.nGhost, native=int(A.native_order),
           maxW=max(int(np.bincount(sub.l, minlength=nOwn)[:nOwn].max()), int(np.bincount(sub.u[sub.u < nOwn], minlength=nOwn).max())))


def solve(order, source, start):
    psi = ctx.to_device(start)
    before = calls[0]
    perf = A.solve_ordered_staged(order, psi, ctx.to_device(source))
    return psi.cpu().numpy(), perf, calls[0] - before


for i, (tag, d, omega) in enumerate(R.five_directions()):
    diag, upper, lower = R.ray_matrix(m, d, omega)
    dl, upl, lol = sub.coeffs(diag, upper, lower)
    source = sub.field(0.5 + O.hash_u(40 + i, np.arange(N)))
    start = np.full(nLoc, np.nan); start[::3] = O.hash_u(7, np.arange(nLoc))[::3]
    A.set_coeffs(dl, upl, lol)
    order = A.flow_order_staged()
    psi, perf, nEx = solve(order, source, start)
    # the rank's rows again, in an order of ffm_flow_stages with the ghost stages of the merged restatement
    want = S.merged_stages(N, l, u, upper, lower, part)
    stage, ord_, _ = ffm.flow_stages(nOwn, sub.nGhost, sub.l, sub.u, upl, lol, want[sub.gcell[nOwn:]].astype(np.int32))
    again = S.staged_substitution(nOwn, sub.l, sub.u, dl, upl, lol, source, psi, ord_)
    out.update({"psi%d" % i: psi[:nOwn], "bitwise%d" % i: int(np.array_equal(bits(again), bits(psi[:nOwn]))), "nStages%d" % i: order.nStages,
                "wantStages%d" % i: int(want.max()) + 1, "stagesMatch%d" % i: int(np.array_equal(stage, want[sub.gcell[:nOwn]])),
                "nIter%d" % i: perf["nIterations"], "conv%d" % i: perf["converged"], "res%d" % i: perf["finalResidual"], "exchanges%d" % i: nEx})
    if i == 0:
        # only rank 0 holds the opposite ray: every rank must refuse, psi untouched, nobody left waiting
        if rank == 0:
            A.set_coeffs(*sub.coeffs(*R.ray_matrix(m, -d, omega)))
        refused, untouched, nEx = 0, 0, -1
        psi_d = ctx.to_device(start)
        before = calls[0]
        try:
            A.solve_ordered_staged(order, psi_d, ctx.to_device(source))
        except ffm.FfmError as e:
            refused = int("(-5)" in str(e))
            untouched = int(np.array_equal(bits(psi_d.cpu().numpy()), bits(start)))
            nEx = calls[0] - before
        if rank == 0:
            A.set_coeffs(dl, upl, lol)
        psi2, perf2, _ = solve(order, source, start)
        again2 = S.staged_substitution(nOwn, sub.l, sub.u, dl, upl, lol, source, psi2, ord_)
        out.update(refused=refused, untouched=untouched, refusedExchanges=nEx, conv_after=perf2["converged"],
                   bitwise_after=int(np.array_equal(bits(again2), bits(psi2[:nOwn])) and np.array_equal(bits(psi2[:nOwn]), bits(psi[:nOwn]))))
    order.close()
A.close()
np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
ctx.close()
