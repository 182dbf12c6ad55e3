"""Cost of the staged flow-ordered ray solves on a decomposed mesh (ffm_solve_ordered_staged_d; fvDOM::setOrderedSolves on a
sub-domain) against the iterative ones on the same decomposition.

  python scripts/rays_ordered_decomposed_timing.py            # all configurations, writes profiles/rays_ordered_decomposed_timing.txt

A 96^3 box, 32 rays (nPhi 2, nTheta 4), emissivity 1, maxIter 1: radiation->correct() of the fvDOM handle on every rank's sub-domain,
one process per rank, ALL RANKS SHARING ONE GPU over the host (gloo) transport -- every ghost exchange and every all-reduce is a
device-to-host copy, a gloo message and a copy back, and the ranks' kernels take turns on the one device.  This does not model 8
devices: read the ratio of the ordered to the iterative figure on the same set-up, not the seconds.
Configurations: RCB into 2 and into 4, graph growing into 4; each a set of rank processes under one `timeout` (a configuration that
fails ends the job: nothing further is started on the GPU).  Per configuration, timed on rank 0 between barriers:
  iterative first     b1_fvdom, PBiCGStab + DILU to 1e-6 per ray from I = 0 (the same code on the parent commit: the baseline):
                      t(1 call) - t(0 calls)
  ordered first       b1_fvdom_ordered, t(1 call) - t(0 calls): makes the 32 staged orders and solves every ray once
  ordered repeated    (t(1 + K calls) - t(1 call)) / K: the staged solves with the orders in place (an ordered solve costs the same
                      whatever it starts from)
                      (a difference of runs that each make their 32 orders: where that cost varies by more than the solves, on a
                      jagged partition, it is not resolved, and ordered first less the separately timed creation is given as an estimate)
  create              ffm_flow_order_create_staged alone on the 32 ray matrices (download of the off-diagonals, the fixpoint rounds of
                      ffm_flow_stages + one ghost exchange + one all-reduce each, upload), with the stage count of every ray
REPEATS runs of each after a warm-up run: the median, and [lo .. hi] from the extremes."""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS, K = 3, 2
CONFIGS = [(2, "rcb", 420), (4, "rcb", 420), (4, "graph", 560)]


def stats(ts):
    return dict(median=float(np.median(ts)), lo=float(min(ts)), hi=float(max(ts)), n=len(ts))


def rank_main(rank, world, port, partitioner, n, out):
    from ffm_import import ffm
    from oracle import plume, fvdom
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ray_matrix as R
    gloo = ffm.gloo_comm
    gloo.init(rank, world, port)
    barrier = lambda: gloo.allreduce(np.zeros(1), 0)
    m = plume.make_mesh((n, n, n))
    N, F = m.nCells, m.nFaces
    part = ffm.decompose.partition_rcb(m.C, world) if partitioner == "rcb" else ffm.decompose.partition_graph(N, m.l, m.u, world)
    sub = ffm.decompose.SubDomain(N, m.l, m.u, part, world, rank)
    ctx = ffm.Context(0)
    ctx.comm_init_host(rank, world, gloo.allreduce, gloo.exchange, gloo.exchange_var)
    gcell, nOwn, nGhost, gface = sub.gcell, sub.nOwned, sub.nGhost, sub.gface
    nLoc = nOwn + nGhost
    sign = np.where(sub.flip.astype(bool), -1.0, 1.0)
    pmask = [part[p.faceCells] == rank for p in m.patches]
    g2l = np.full(N, -1, np.int64); g2l[gcell[:nOwn]] = np.arange(nOwn)
    cOrd, fOrd = ffm.renumber_levels(nOwn, sub.l, sub.u, nGhost=nGhost)
    l2, u2, oldToNew = ffm.hexmesh.apply_renumbering(nLoc, sub.l, sub.u, cOrd, fOrd)
    A = ffm.lduMatrix(ctx, nOwn, l2, u2, nGhost=nGhost)
    A.set_ghost_exchange(sub.nbrRank, sub.sendCount, oldToNew[sub.sendCells], sub.recvCount, tags=sub.tags, globalCells=N)
    wgt = np.where(sign < 0, 1.0 - m.weights[gface], m.weights[gface])
    patches = [(oldToNew[g2l[p.faceCells[k]]].astype(np.int32), p.Sf[k].T.copy(), p.deltaCoeffs[k]) for p, k in zip(m.patches, pmask)]
    Sf = (m.Sf[gface] * sign[:, None])[fOrd]
    mesh = ffm.fvMesh(A, m.V[gcell][cOrd], m.C[gcell][cOrd].T.copy(), Sf.T.copy(), m.magSf[gface][fOrd], wgt[fOrd], m.deltaCoeffs[gface][fOrd], patches)
    B = sum(int(k.sum()) for k in pmask)
    x, y = m.C[:, 0], m.C[:, 1]
    T = 500.0 + 600.0 * np.exp(-((x - x.mean()) ** 2 + (y - 0.3 * y.max()) ** 2) / 0.5)
    E = 2.0e5 * np.exp(-((x - x.mean()) ** 2 + (y - 0.3 * y.max()) ** 2) / 0.25)
    Tb = [np.full(p.size, 900.0 if p.name == "inlet" else 320.0) for p in m.patches]
    P = lambda v: np.ascontiguousarray(v, np.float64)
    dp = C.POINTER(C.c_double)
    Tc, Ec = P(T[gcell][cOrd]), P(E[gcell][cOrd])
    Tbb = P(np.concatenate([t[k] for t, k in zip(Tb, pmask)])) if B else np.zeros(1)
    emb = np.ones(max(B, 1))
    lib = C.CDLL(os.path.join(os.path.dirname(ffm.libpath()), "libffm_b1demo.so"))
    base = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_double, C.c_int, C.c_double, C.c_double] + [dp] * 4 + [C.c_int] + [dp] * 5 + [C.POINTER(C.c_int)] * 2
    lib.b1_fvdom.restype = lib.b1_fvdom_ordered.restype = C.c_int
    lib.b1_fvdom.argtypes = base
    lib.b1_fvdom_ordered.argtypes = base + [C.POINTER(C.c_int)]
    os.environ["FFM_FOAM_QUIET"] = "1"
    IOut, GOut, q = np.empty((32, nLoc)), np.empty(nLoc), [np.empty(max(B, 1)) for _ in range(3)]
    maxIts = C.c_int(0)

    def run(ordered, nCalls):
        fn = lib.b1_fvdom_ordered if ordered else lib.b1_fvdom
        iters, nSolves = (C.c_int * max(nCalls, 1))(), C.c_int()
        extra = [C.byref(maxIts)] if ordered else []
        ctx.sync(); barrier(); t0 = time.perf_counter()
        r = fn(ctx.h, A.h, mesh.h, 0, 2, 4, 1, 0.0, 0, 0.3, 1e-6, Tc.ctypes.data_as(dp), Tbb.ctypes.data_as(dp), Ec.ctypes.data_as(dp),
               emb.ctypes.data_as(dp), nCalls, IOut.ctypes.data_as(dp), GOut.ctypes.data_as(dp), *(a.ctypes.data_as(dp) for a in q), iters,
               C.byref(nSolves), *extra)
        ctx.sync(); barrier(); dt = time.perf_counter() - t0
        assert r == 32 and nSolves.value == (32 if nCalls else 0)
        return dt

    def series(ordered, calls):
        run(ordered, 1)
        return {c: [run(ordered, c) for _ in range(REPEATS)] for c in calls}
    res = dict(cells=N, owned=nOwn, ghost=nGhost, world=world, partitioner=partitioner)
    it = series(False, (0, 1))
    res["iterative_first"] = dict(median=np.median(it[1]) - np.median(it[0]), lo=min(it[1]) - max(it[0]), hi=max(it[1]) - min(it[0]))
    res["G_sum_iterative"] = float(GOut[:nOwn].sum())          # (the renumbering keeps the owned cells in front)
    od = series(True, (0, 1, 1 + K))
    res["ordered_first"] = dict(median=np.median(od[1]) - np.median(od[0]), lo=min(od[1]) - max(od[0]), hi=max(od[1]) - min(od[0]))
    res["ordered_repeated"] = dict(median=(np.median(od[1 + K]) - np.median(od[1])) / K, lo=(min(od[1 + K]) - max(od[1])) / K, hi=(max(od[1 + K]) - min(od[1])) / K)
    res["G_sum_ordered"] = float(GOut[:nOwn].sum()); res["maxSolveIterations"] = maxIts.value
    res["t0"] = [float(np.median(it[0])), float(np.median(od[0]))]
    # order creation alone, every ray: the ray matrix of tests/ray_matrix.py on the rank's own faces
    mm = type("M", (), dict(nCells=nLoc, l=l2, u=u2, Sf=Sf, V=m.V[gcell][cOrd]))
    ts, stages, levels = [], [], []
    for _, dAve, omega in fvdom.ray_set(2, 4):
        A.set_coeffs(*R.ray_matrix(mm, dAve, omega))
        ctx.sync(); barrier(); t0 = time.perf_counter(); o = A.flow_order_staged(); ctx.sync(); barrier(); ts.append(time.perf_counter() - t0)
        stages.append(o.nStages); levels.append(o.nLevels); o.close()
    res["create"] = stats(ts); res["create_total"] = float(sum(ts)); res["stages"] = stages; res["levels"] = [min(levels), max(levels)]
    mesh.close(); A.close(); ctx.close()
    if rank == 0:
        json.dump(res, open(out, "w"))


def report(results):
    f = lambda s: "%9.4f   [%.4f .. %.4f]" % (s["median"], s["lo"], s["hi"])
    L = ["Staged flow-ordered ray solves on a decomposed mesh against the iterative ones", "=" * 78,
         "Script: scripts/rays_ordered_decomposed_timing.py.  One MI355X SHARED by all ranks of a configuration, one process per rank, host",
         "(gloo) transport: every ghost exchange and all-reduce goes through host memory, the ranks' kernels take turns on the device.  This",
         "does not model several devices: read the ratio ordered / iterative of a row, not the seconds.  Medians of %d runs after a warm-up" % REPEATS,
         "run, [min .. max]; wall time on rank 0 between barriers.",
         "radiation->correct() of the fvDOM handle, 96^3 box, 32 rays, emissivity 1, maxIter 1 (b1_fvdom / b1_fvdom_ordered on every sub-domain):",
         "  iterative first  = t(1 call) - t(0 calls), PBiCGStab + block-Jacobi DILU to 1e-6 per ray from I = 0 (unchanged code: the parent's figure)",
         "  ordered first    = t(1 call) - t(0 calls): makes the 32 staged orders, then one staged solve per ray",
         "  ordered repeated = (t(%d calls) - t(1 call)) / %d: the staged solves with the orders in place" % (1 + K, K), ""]
    for r in results:
        st = r["stages"]
        L += ["%s into %d: %d cells, rank 0 owns %d (+ %d ghost cells); stages per ray %d .. %d (median %d), levels on rank 0 %d .. %d"
              % (r["partitioner"], r["world"], r["cells"], r["owned"], r["ghost"], min(st), max(st), int(np.median(st)), r["levels"][0], r["levels"][1]),
              "    iterative first correct() [s]        %s" % f(r["iterative_first"]),
              "    ordered first correct() [s]          %s" % f(r["ordered_first"]),
              ("    ordered repeated correct() [s]       %s     ratio to iterative first %.3f" % (f(r["ordered_repeated"]), r["ordered_repeated"]["median"] / r["iterative_first"]["median"]))
              if r["ordered_repeated"]["lo"] > 0 else
              ("    ordered repeated correct() [s]       not resolved (%s): every run makes its 32 orders anew, and their cost varies by more\n"
               "                                         than a solve.  Estimate: ordered first less the 32 orders below = %.2f s, ratio to iterative first %.2f"
               % (f(r["ordered_repeated"]).strip(), r["ordered_first"]["median"] - r["create_total"],
                  (r["ordered_first"]["median"] - r["create_total"]) / r["iterative_first"]["median"])),
              "    ffm_flow_order_create_staged [s]     %s     per order; all 32 once per case: %.3f s" % (f(r["create"]), r["create_total"]),
              "    largest iteration count of an ordered ray solve: %d;  sum(G) on rank 0: iterative %.10e, ordered %.10e"
              % (r["maxSolveIterations"], r["G_sum_iterative"], r["G_sum_ordered"]), ""]
    return "\n".join(L)


def free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int)
    ap.add_argument("--world", type=int)
    ap.add_argument("--port", type=int)
    ap.add_argument("--partitioner")
    ap.add_argument("--out")
    ap.add_argument("--n", type=int, default=96)
    ap.add_argument("--only", help="world:partitioner of the one configuration to run, e.g. 2:rcb")
    a = ap.parse_args()
    if a.rank is not None:
        rank_main(a.rank, a.world, a.port, a.partitioner, a.n, a.out)
        sys.exit(0)
    tmp = os.path.join(ROOT, "prof_out"); os.makedirs(tmp, exist_ok=True)
    results, rc = [], 0
    for world, partitioner, limit in CONFIGS:
        if a.only and a.only != "%d:%s" % (world, partitioner):
            continue
        out = os.path.join(tmp, "rays_ordered_decomposed_%d_%s.json" % (world, partitioner))
        port = free_port()
        procs = [subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--rank", str(r), "--world", str(world),
                                   "--port", str(port), "--partitioner", partitioner, "--n", str(a.n), "--out", out]) for r in range(world)]
        rcs = []
        for p in procs:
            try:
                rcs.append(p.wait(timeout=limit + 30))
            except subprocess.TimeoutExpired:
                rcs.append(124)
        for p in procs:                              # never leave a rank behind
            if p.poll() is None:
                p.kill()
        rc = next((c for c in rcs if c != 0), 0)
        if rc != 0:
            print("%s into %d ended with statuses %r: nothing further is started" % (partitioner, world, rcs)); break
        results.append(json.load(open(out)))
        print(json.dumps(results[-1]), flush=True)
    txt = report(results)
    print(txt)
    if rc == 0 and a.n == 96 and not a.only:
        open(os.path.join(ROOT, "profiles", "rays_ordered_decomposed_timing.txt"), "w").write(txt)
    sys.exit(rc)
