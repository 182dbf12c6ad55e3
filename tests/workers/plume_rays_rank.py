"""One rank of a decomposed plume run with the fvDOM rays on (solverFreq 1), sharing cuda:0 with the other ranks (host transport
over gloo): one time step, then a second one with the absorption / emission model coupled into h, once per radiation ordering
asked for (0: every ray a PBiCGStab solve over all ranks, 1: the staged direction-ordered sweep).
usage: plume_rays_rank.py rank world port gx gy gz bx by bz modes outdir      (modes: "0", "1" or "01")"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
glob = tuple(int(v) for v in sys.argv[4:7]); grid = tuple(int(v) for v in sys.argv[7:10])
modes, outdir = sys.argv[10], sys.argv[11]
from ffm_import import ffm  # noqa: E402
from oracle import plume as oplume  # noqa: E402
gloo_comm = ffm.gloo_comm
gloo_comm.init(rank, world, port)
ctx = ffm.Context(0)
ctx.comm_init_host(rank, world, gloo_comm.allreduce, gloo_comm.exchange)
lo, hi, nbr = ffm.hexmesh.block_of_rank(glob, grid, rank)
FIELDS = ["T", "p_rgh", "Ux", "Uy", "Uz", "O2", "C3H8", "CO2", "H2O"]
out = {}
for mode in modes:
    case = ffm.Plume(ctx, glob, lo=lo, hi=hi, nbrRank=nbr)
    case.set_radiation(solverFreq=1, rays=oplume.ray_set())
    if mode != "0":
        case.set_radiation_ordering(int(mode))
    for step in range(2):
        if step == 1:
            case.set_radiation_model(0.08, 0.3, 0.3)
        case.step()
        out["m%s_s%d_iters" % (mode, step)] = np.array([(n, p["nIterations"]) for n, p in case.solves()], dtype=object)
        out["m%s_s%d_res" % (mode, step)] = np.array([(p["initialResidual"], p["finalResidual"], p["converged"]) for n, p in case.solves() if n.startswith("I")])
        for name in ["G"] + ["I%d" % i for i in range(32)] + (FIELDS if step == 1 else []):
            out["m%s_s%d_%s" % (mode, step, name)] = case.field(name)
    case.close()
np.savez(os.path.join(outdir, "rank%d.npz" % rank), lo=np.array(lo), hi=np.array(hi), **out)
ctx.close()
