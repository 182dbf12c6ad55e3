"""One rank of a decomposed plume run with kEqn, the janaf thermo and the reference's EDC, sharing cuda:0 with the other ranks (host
transport over gloo).  usage: plume_thermo_rank.py rank world port gx gy gz bx by bz nSteps outdir"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
glob = tuple(int(v) for v in sys.argv[4:7]); grid = tuple(int(v) for v in sys.argv[7:10])
nSteps, outdir = int(sys.argv[10]), sys.argv[11]
from ffm_import import ffm  # noqa: E402
from oracle import plume  # noqa: E402
from oracle import thermo as TH  # noqa: E402
from plume_keqn_ref import smooth_k0  # noqa: E402
from plume_thermo_ref import DATA, TABLE, single_step  # noqa: E402
gloo_comm = ffm.gloo_comm
gloo_comm.init(rank, world, port)
ctx = ffm.Context(0)
ctx.comm_init_host(rank, world, gloo_comm.allreduce, gloo_comm.exchange)
lo, hi, nbr = ffm.hexmesh.block_of_rank(glob, grid, rank)
case = ffm.Plume(ctx, glob, lo=lo, hi=hi, nbrRank=nbr)
# the block's part of the global k0, in the block's own natural order
k0 = smooth_k0(plume.make_mesh(glob)).reshape(glob[2], glob[1], glob[0])[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].ravel()
case.set_turbulence(k0=k0)
th = ffm.Thermo(ctx, DATA["species"], TABLE, TH.RR)
case.set_thermo(th)
rx = single_step()
case.set_combustion(s=rx.s, qFuel=rx.qFuel)
for _ in range(nSteps):
    case.step()
assert [n for n, _ in case.solves()][-2:] == ["p_rgh", "k"]
names = ["rho", "p", "p_rgh", "T", "h", "Ux", "Uy", "Uz", "O2", "C3H8", "CO2", "k", "nut", "alphat", "psi", "mu", "alpha", "Cp", "wFuel", "Qdot"]
out = {name: case.field(name) for name in names}
np.savez(os.path.join(outdir, "rank%d.npz" % rank), lo=np.array(lo), hi=np.array(hi), **out)
case.close(); th.close(); ctx.close()
