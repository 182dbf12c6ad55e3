"""Cost of one fvDOM ray sweep (radiation_correct, 32 rays) of the plume driver on a decomposed box: ranks share cuda:0 over the
host / gloo transport.  The sweep is timed as the difference between a time step with the rays on (solverFreq 1) and the same
step with them off, over REPEATS steps each.  The per-tick exchange cost of the staged sweep comes from a SECOND run with FFM_TIMING=1:
the sweep itself then prints the wall time of its ticks' exchanges (the ghost exchange plus the copies into the rays' ghost layers) to
stderr, "ffm timing: staged ray sweep rank r: ..." -- that run's sweep time is inflated by two synchronisations per tick and is not the
one to quote.  The plain ghost refresh timed here is for comparison only.

  python scripts/rays_decomposed_timing.py --n 96 --grid 2 1 1 --ordering 1      # staged sweep, 2 ranks
  python scripts/rays_decomposed_timing.py --n 96 --grid 2 1 1 --ordering 0      # block-Jacobi PBiCGStab per ray, 2 ranks
  python scripts/rays_decomposed_timing.py --n 96 --grid 1 1 1                   # one block: the direction-ordered sweep
Two ranks on one GPU over gloo do not model 8 devices: the number to read is the ratio of ordering 1 to ordering 0."""
import argparse
import ctypes as C
import os
import socket
import subprocess
import sys
import time

REPEATS = 5          # timed steps after one warm-up step
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step_time(ffm, ctx, glob, lo, hi, nbr, rays, ordering):
    kw = {} if nbr is None else dict(lo=lo, hi=hi, nbrRank=nbr)
    case = ffm.Plume(ctx, glob, **kw)
    if rays:
        case.set_radiation(solverFreq=1)
        if ordering:
            case.set_radiation_ordering(ordering)
    case.step(); ctx.sync()
    dts = []
    for _ in range(REPEATS):
        t0 = time.perf_counter(); case.step(); ctx.sync(); dts.append(time.perf_counter() - t0)
    its = [p["nIterations"] for n, p in case.solves() if n.startswith("I")]
    tEx = 0.0
    if rays and nbr is not None:
        n = ffm.lib().ffm_ldu_ncells(C.c_void_p(case.ldu_handle()))          # owned + ghost cells
        x = ctx.zeros(n)
        reps = 40
        ctx.sync(); t0 = time.perf_counter()
        for _ in range(reps):
            ffm.lib().ffm_halo_refresh_d(C.c_void_p(case.ldu_handle()), C.c_void_p(x.data_ptr()))
        ctx.sync(); tEx = (time.perf_counter() - t0) / reps
    case.close()
    return dts, its, tEx


def rank_main(a):
    from ffm_import import ffm
    glob, grid = (a.n,) * 3, tuple(a.grid)
    world = grid[0] * grid[1] * grid[2]
    ctx = ffm.Context(0)
    lo = hi = nbr = None
    if world > 1:
        ffm.gloo_comm.init(a.rank, world, a.port)
        ctx.comm_init_host(a.rank, world, ffm.gloo_comm.allreduce, ffm.gloo_comm.exchange)
        lo, hi, nbr = ffm.hexmesh.block_of_rank(glob, grid, a.rank)
    tOff, _, _ = step_time(ffm, ctx, glob, lo, hi, nbr, False, 0)
    tOn, its, tEx = step_time(ffm, ctx, glob, lo, hi, nbr, True, a.ordering)
    if a.rank == 0:
        nTicks = 0
        if world > 1 and a.ordering == 1:
            import numpy as np
            from oracle import plume as oplume
            _, nTicks = ffm.ray_schedule(grid, (0, 0, 0), np.array([d for d, _ in oplume.ray_set()]))
        fmt = lambda v: " ".join("%.4f" % x for x in v)      # noqa: E731
        print("RAYS n=%d grid=%s ordering=%d: steps with rays [%s] s, without [%s] s -> sweep of %d rays %.4f s (medians; spread of the "
              "difference %.4f .. %.4f); iterations per ray mean %.1f; ticks %d; one plain ghost refresh %.3f ms"
              % (a.n, "x".join(map(str, grid)), a.ordering, fmt(tOn), fmt(tOff), len(its), sorted(tOn)[len(tOn) // 2] - sorted(tOff)[len(tOff) // 2],
                 min(tOn) - max(tOff), max(tOn) - min(tOff), sum(its) / max(len(its), 1), nTicks, 1e3 * tEx), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=96); ap.add_argument("--grid", type=int, nargs=3, default=[2, 1, 1])
    ap.add_argument("--ordering", type=int, default=0); ap.add_argument("--rank", type=int, default=-1); ap.add_argument("--port", type=int, default=0)
    a = ap.parse_args()
    world = a.grid[0] * a.grid[1] * a.grid[2]
    if a.rank >= 0 or world == 1:
        a.rank = max(a.rank, 0)
        return rank_main(a)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--grid", *map(str, a.grid), "--ordering", str(a.ordering),
                               "--rank", str(r), "--port", str(port)]) for r in range(world)]
    try:
        rcs = [p.wait(timeout=500) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    sys.exit(0 if rcs == [0] * world else 1)


if __name__ == "__main__":
    main()
