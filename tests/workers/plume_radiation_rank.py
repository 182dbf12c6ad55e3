"""One rank of a decomposed plume run with kEqn, the janaf thermo, the reference's EDC and the coupled fvDOM rays
(ffm_plume_set_radiation_thermo) from the default start state (the only one a block can be given), sharing cuda:0 with the other ranks
(host transport over gloo); one case per ray ordering in `modes`.
usage: plume_radiation_rank.py rank world port gx gy gz bx by bz nSteps modes outdir [coupleAt [absorption Ehrr1 Ehrr2]]     (modes: "0", "1" or "01")"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
glob = tuple(int(v) for v in sys.argv[4:7]); grid = tuple(int(v) for v in sys.argv[7:10])
nSteps, modes, outdir = int(sys.argv[10]), sys.argv[11], sys.argv[12]
from ffm_import import ffm  # noqa: E402
from oracle import plume  # noqa: E402
from oracle import thermo as TH  # noqa: E402
from plume_keqn_ref import smooth_k0  # noqa: E402
from plume_radiation_ref import RAD_MODEL  # noqa: E402
coupleAt = int(sys.argv[13]) if len(sys.argv) > 13 else 0          # the step before which the absorption / emission model is coupled
model = tuple(float(v) for v in sys.argv[14:17]) if len(sys.argv) > 16 else RAD_MODEL
from plume_thermo_ref import DATA, TABLE, single_step  # noqa: E402
gloo_comm = ffm.gloo_comm
gloo_comm.init(rank, world, port)
ctx = ffm.Context(0)
ctx.comm_init_host(rank, world, gloo_comm.allreduce, gloo_comm.exchange)
lo, hi, nbr = ffm.hexmesh.block_of_rank(glob, grid, rank)
# the block's part of the global k0, in the block's own natural order
k0 = smooth_k0(plume.make_mesh(glob)).reshape(glob[2], glob[1], glob[0])[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].ravel()
th = ffm.Thermo(ctx, DATA["species"], TABLE, TH.RR)
rx = single_step()
names = ["rho", "p", "p_rgh", "T", "h", "Ux", "Uy", "Uz", "O2", "C3H8", "CO2", "k", "nut", "alphat", "psi", "mu", "alpha", "Cp", "wFuel", "Qdot",
         "G", "ShSu", "ShSp"] + ["I%d" % i for i in range(32)]
out = {}
for mode in modes:
    case = ffm.Plume(ctx, glob, lo=lo, hi=hi, nbrRank=nbr)
    case.set_turbulence(k0=k0)
    case.set_thermo(th)
    case.set_combustion(s=rx.s, qFuel=rx.qFuel)
    case.set_radiation_thermo(True)
    case.set_radiation(solverFreq=1)
    case.set_radiation_ordering(int(mode))
    for step in range(nSteps):
        if step == coupleAt:
            case.set_radiation_model(*model)
        case.step()
    log = case.solves()
    assert [n for n, _ in log][-2:] == ["p_rgh", "k"]
    out["m%s_rayIters" % mode] = np.array([pf["nIterations"] for n, pf in log if n.startswith("I")])
    for name in names:
        out["m%s_%s" % (mode, name)] = case.field(name)
    case.close()
np.savez(os.path.join(outdir, "rank%d.npz" % rank), lo=np.array(lo), hi=np.array(hi), **out)
th.close(); ctx.close()
