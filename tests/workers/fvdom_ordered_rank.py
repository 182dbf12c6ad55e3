"""One rank of a decomposed run of b1_fvdom_ordered (examples/b1_demo.C: the fvDOM handle with setOrderedSolves(true), every ray by
fvScalarMatrix::solveOrdered -- on a sub-domain the staged pair ffm_flow_order_create_staged / ffm_solve_ordered_staged_d), all ranks
sharing cuda:0 through the host (gloo) transport; div(Ji,Ii_h) upwind, then linearUpwind.  The Foam layer's log goes to stdout, a
line "== scheme <n>" in front of each run.   usage: fvdom_ordered_rank.py rank world port nx ny nz partitioner outdir"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ffm_import import ffm  # noqa: E402
from oracle import plume  # noqa: E402   (mesh builder only)
import foam_case  # noqa: E402
import fvdom_ordered_case  # noqa: E402

rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
n = tuple(int(v) for v in sys.argv[4:7]); partitioner, outdir = sys.argv[7], sys.argv[8]
gloo = ffm.gloo_comm
gloo.init(rank, world, port)
m = plume.make_mesh(n, h=0.1)
part = ffm.decompose.partition_rcb(m.C, world) if partitioner == "rcb" else ffm.decompose.partition_graph(m.nCells, m.l, m.u, world)
sub = ffm.decompose.SubDomain(m.nCells, m.l, m.u, part, world, rank)
ctx = ffm.Context(0)
ctx.comm_init_host(rank, world, gloo.allreduce, gloo.exchange, gloo.exchange_var)
T, Tb, E, emis = foam_case.fvdom_inputs(m)
out = dict(nGhost=sub.nGhost)
for scheme in (0, 5):
    print("== scheme %d" % scheme, flush=True)
    (I, G, qp), cells, its, nSolves, maxIts = fvdom_ordered_case.run(ffm, ctx, m, T, Tb, E, emis, sub=sub, part=part, scheme=scheme)
    sys.stdout.flush()
    out.update({"cells": cells, "I_%d" % scheme: I, "G_%d" % scheme: G, "its_%d" % scheme: np.array(its), "nSolves_%d" % scheme: nSolves,
                "maxIts_%d" % scheme: maxIts}, **{"pos_" + k: v[0] for k, v in qp.items()}, **{"qin_%d_%s" % (scheme, k): v[1] for k, v in qp.items()})
np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
ctx.close()
