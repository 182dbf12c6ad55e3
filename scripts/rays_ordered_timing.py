"""Cost of the flow-ordered exact ray solves (ffm_solve_ordered_d; fvDOM::setOrderedSolves) against today's iterative ones.

  python scripts/rays_ordered_timing.py            # all steps, writes profiles/rays_ordered_timing.txt

Steps, each a child process under its own `timeout` (a step that fails ends the job: nothing further is started on the GPU):
  correct_iterative   96^3 box, 32 rays (nPhi 2, nTheta 4), emissivity 1, maxIter 1: radiation->correct() of the fvDOM handle through
                      b1_fvdom (PBiCGStab + DILU to 1e-6 per ray -- the same code on the parent commit: the baseline)
  correct_ordered     the same through b1_fvdom_ordered; and ffm_flow_order_create alone on ray matrices of that mesh
  solves200           200^3 box: one ffm_solve_ordered_d and one ffm_solve_d (PBiCGStab + DILU, 1e-6) on a ray of mixed signs, one
                      ffm_solve_ordered_d and one ffm_solve_triangular_rows_d on an all-positive ray
b1_fvdom* build the handle, run nCalls calls of correct() on the SAME fields and copy the results out.  The first correct() of a
handle starts from I = 0 and is timed as t(1 call) - t(0 calls); a repeated correct() as (t(1 + K calls) - t(1 call)) / K: there the
iterative solves start from the converged intensities of the call before and return after 0 iterations -- the cheapest case they
have -- while an ordered solve costs the same whatever it starts from.  A time step of a fire case lies between the two.
REPEATS runs of each after a warm-up run: the median, and [lo .. hi] from the extremes.
A single solve: WARMUP calls, then the median and min .. max of REPEATS calls (every solve ends with a read-back, so wall time
brackets it)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS, WARMUP, K = 5, 2, 3
STEPS = [("correct_iterative", 420), ("correct_ordered", 420), ("solves200", 420)]


def stats(ts):
    return dict(median=float(np.median(ts)), lo=float(min(ts)), hi=float(max(ts)), n=len(ts))


def ray_dirs():
    from oracle import fvdom
    return fvdom.ray_set(2, 4)


def correct96(ordered):
    from ffm_import import ffm
    from oracle import plume
    n = 96
    ctx = ffm.Context(0)
    m = plume.make_mesh((n, n, n))
    N, B = m.nCells, sum(p.size for p in m.patches)
    cOrd, fOrd = ffm.renumber_levels(N, m.l, m.u)
    l2, u2, oldToNew = ffm.hexmesh.apply_renumbering(N, m.l, m.u, cOrd, fOrd)
    A = ffm.lduMatrix(ctx, N, l2, u2)
    patches = [(oldToNew[p.faceCells].astype(np.int32), p.Sf.T.copy(), p.deltaCoeffs) for p in m.patches]
    mesh = ffm.fvMesh(A, m.V[cOrd], m.C[cOrd].T.copy(), m.Sf[fOrd].T.copy(), m.magSf[fOrd], m.weights[fOrd], m.deltaCoeffs[fOrd], patches)
    x, y = m.C[:, 0], m.C[:, 1]
    T = 500.0 + 600.0 * np.exp(-((x - x.mean()) ** 2 + (y - 0.3 * y.max()) ** 2) / 0.5)
    E = 2.0e5 * np.exp(-((x - x.mean()) ** 2 + (y - 0.3 * y.max()) ** 2) / 0.25)
    Tb = np.concatenate([np.full(p.size, 900.0 if p.name == "inlet" else 320.0) for p in m.patches])
    P = lambda v: np.ascontiguousarray(v, np.float64)
    dp = C.POINTER(C.c_double)
    Tc, Tbb, Ec, emb = P(T[cOrd]), P(Tb), P(E[cOrd]), np.ones(B)
    lib = C.CDLL(os.path.join(os.path.dirname(ffm.libpath()), "libffm_b1demo.so"))
    base = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_double, C.c_int, C.c_double, C.c_double] + [dp] * 4 + [C.c_int] + [dp] * 5 + [C.POINTER(C.c_int)] * 2
    fn = lib.b1_fvdom_ordered if ordered else lib.b1_fvdom
    fn.restype, fn.argtypes = C.c_int, base + ([C.POINTER(C.c_int)] if ordered else [])
    os.environ["FFM_FOAM_QUIET"] = "1"
    IOut, GOut, q = np.empty((32, N)), np.empty(N), [np.empty(B) for _ in range(3)]
    maxIts = C.c_int(0)

    def run(nCalls):
        iters, nSolves = (C.c_int * nCalls)(), C.c_int()
        extra = [C.byref(maxIts)] if ordered else []
        ctx.sync(); t0 = time.perf_counter()
        r = fn(ctx.h, A.h, mesh.h, 0, 2, 4, 1, 0.0, 0, 0.3, 1e-6, Tc.ctypes.data_as(dp), Tbb.ctypes.data_as(dp), Ec.ctypes.data_as(dp),
               emb.ctypes.data_as(dp), nCalls, IOut.ctypes.data_as(dp), GOut.ctypes.data_as(dp), *(a.ctypes.data_as(dp) for a in q), iters,
               C.byref(nSolves), *extra)
        ctx.sync(); dt = time.perf_counter() - t0
        assert r == 32 and nSolves.value == (32 if nCalls else 0)
        return dt
    run(1)
    t0 = [run(0) for _ in range(REPEATS)]
    t1 = [run(1) for _ in range(REPEATS)]
    tK = [run(1 + K) for _ in range(REPEATS)]
    out = dict(cells=N, t0=stats(t0), t1=stats(t1), tK=stats(tK),
               first=dict(median=np.median(t1) - np.median(t0), lo=min(t1) - max(t0), hi=max(t1) - min(t0)),
               steady=dict(median=(np.median(tK) - np.median(t1)) / K, lo=(min(tK) - max(t1)) / K, hi=(max(tK) - min(t1)) / K),
               G_sum=float(GOut.sum()))
    if ordered:
        out["maxSolveIterations"] = maxIts.value
        # order creation alone: three rays of different octants
        import importlib
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        R = importlib.import_module("ray_matrix")
        mm = type("M", (), dict(nCells=N, l=l2, u=u2, Sf=m.Sf[fOrd], V=m.V[cOrd]))
        ts, levels = [], []
        for i in (0, 3, 21):
            _, dAve, omega = ray_dirs()[i]
            A.set_coeffs(*R.ray_matrix(mm, dAve, omega))
            for _ in range(3):
                ctx.sync(); t0 = time.perf_counter(); o = A.flow_order(); ctx.sync(); ts.append(time.perf_counter() - t0)
                levels.append(o.nLevels); o.close()
        out["create"] = stats(ts); out["create_levels"] = sorted(set(levels))
    mesh.close(); A.close(); ctx.close()
    return out


def solves200():
    from ffm_import import ffm
    n, h = 200, 0.05
    ctx = ffm.Context(0)
    blk = ffm.hexmesh.HexBlock((n, n, n))
    N = blk.nCells
    cOrd, fOrd = ffm.renumber_levels(N, blk.l, blk.u)
    step = (blk.u - blk.l)[fOrd]
    axis = np.where(step == 1, 0, np.where(step == n, 1, 2))
    l2, u2, _ = ffm.hexmesh.apply_renumbering(N, blk.l, blk.u, cOrd, fOrd)
    A = ffm.lduMatrix(ctx, N, l2, u2)
    assert A.native_order
    rays = ray_dirs()
    lib = ffm.lib()
    lib.ffm_solve_triangular_rows_d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ffm.binding.Perf)]
    lib.ffm_solve_triangular_rows_d.restype = C.c_int
    src = ctx.to_device(0.5 + ffm.hexmesh.hash_u(3, np.arange(N)))
    out = dict(cells=N, sweep_mode=A.sweep_mode)

    def matrix(dAve, omega):
        Ji = np.asarray(dAve)[axis] * (h * h)
        diag = 0.3 * omega * h ** 3 + np.bincount(l2, np.maximum(Ji, 0.0), N) + np.bincount(u2, np.maximum(-Ji, 0.0), N)
        A.set_coeffs(diag, np.minimum(Ji, 0.0) + 0.0, -np.maximum(Ji, 0.0) + 0.0)

    def timed(fn):
        ts = []
        for i in range(WARMUP + REPEATS):
            psi = ctx.zeros(N)
            ctx.sync(); t0 = time.perf_counter(); perf = fn(psi); ctx.sync(); dt = time.perf_counter() - t0
            if i >= WARMUP:
                ts.append(dt)
        return dict(stats(ts), **{k: perf[k] for k in ("nIterations", "converged", "finalResidual")})

    def tri(psi):
        p = ffm.binding.Perf()
        rc = lib.ffm_solve_triangular_rows_d(A.h, C.c_void_p(psi.data_ptr()), C.c_void_p(src.data_ptr()), C.byref(p))
        assert rc == 0, lib.ffm_last_error()
        return p.as_dict()
    mixed = next(r for r in rays if r[1][0] < 0 and r[1][1] > 0 and r[1][2] > 0)
    matrix(mixed[1], mixed[2])
    t0 = time.perf_counter(); o = A.flow_order(); out["create_mixed"] = time.perf_counter() - t0; out["levels_mixed"] = o.nLevels
    out["ordered_mixed"] = timed(lambda psi: A.solve_ordered(o, psi, src))
    out["pbicgstab_mixed"] = timed(lambda psi: A.solve(psi, src, solver="PBiCGStab", preconditioner="DILU", tolerance=1e-6))
    o.close()
    pos = next(r for r in rays if min(r[1]) > 0)
    matrix(pos[1], pos[2])
    o = A.flow_order(); out["levels_positive"] = o.nLevels
    out["ordered_positive"] = timed(lambda psi: A.solve_ordered(o, psi, src))
    out["triangular_rows_positive"] = timed(tri)
    o.close(); A.close(); ctx.close()
    return out


def report(r):
    f = lambda s: "%9.4f   [%.4f .. %.4f]" % (s["median"], s["lo"], s["hi"])
    ms = lambda s: "%9.3f   [%.3f .. %.3f]" % (1e3 * s["median"], 1e3 * s["lo"], 1e3 * s["hi"])
    L = ["Flow-ordered exact ray solves against the iterative ones", "=" * 56,
         "Script: scripts/rays_ordered_timing.py.  MI355X, one process per step.  Medians of %d runs after warm-up, [min .. max]." % REPEATS, ""]
    it, od = r.get("correct_iterative"), r.get("correct_ordered")
    if it and od:
        L += ["radiation->correct() of the fvDOM handle, 96^3 = %d cells, 32 rays, emissivity 1, maxIter 1 (b1_fvdom / b1_fvdom_ordered)" % it["cells"],
              "first correct() of a handle (from I = 0) = t(1 call) - t(0 calls); ordered, it includes making the 32 orders",
              "repeated correct() on unchanged fields = (t(%d calls) - t(1 call)) / %d: the iterative solves then start converged, 0 iterations" % (1 + K, K), "",
              "                                         first correct() [s]               repeated correct(), unchanged fields [s]",
              "iterative (PBiCGStab + DILU, 1e-6)      %s   %s" % (f(it["first"]), f(it["steady"])),
              "ordered (one forward substitution)      %s   %s" % (f(od["first"]), f(od["steady"])),
              "ordered first correct() less 32 x the order creation below: %.4f s" % (od["first"]["median"] - 32 * od["create"]["median"]),
              "ratios ordered / iterative (medians): first %.3f, repeated %.3f;  largest iteration count of an ordered ray solve: %d"
              % (od["first"]["median"] / it["first"]["median"], od["steady"]["median"] / it["steady"]["median"], od["maxSolveIterations"]),
              "set-up and copy-out of b1_fvdom* alone, t(0 calls): %.4f / %.4f s" % (it["t0"]["median"], od["t0"]["median"]),
              "sum(G) iterative %.10e, ordered %.10e" % (it["G_sum"], od["G_sum"]), "",
              "ffm_flow_order_create alone on that mesh (download of the off-diagonals, Kahn on the host, upload of int[N]):",
              "    per order [s]                        %s   x 32 rays = %.3f s once per case; levels %s" % (f(od["create"]), 32 * od["create"]["median"], od["create_levels"]), ""]
    s = r.get("solves200")
    if s:
        L += ["single solves, 200^3 = %d cells (sweep mode of the matrix: %d)                      [ms]" % (s["cells"], s["sweep_mode"]),
              "mixed-sign ray (%d levels):   ffm_solve_ordered_d                     %s   1 iteration, converged %d" % (s["levels_mixed"], ms(s["ordered_mixed"]), s["ordered_mixed"]["converged"]),
              "                               ffm_solve_d PBiCGStab + DILU, 1e-6      %s   %d iterations" % (ms(s["pbicgstab_mixed"]), s["pbicgstab_mixed"]["nIterations"]),
              "all-positive ray (%d levels): ffm_solve_ordered_d                     %s" % (s["levels_positive"], ms(s["ordered_positive"])),
              "                               ffm_solve_triangular_rows_d             %s   converged %d" % (ms(s["triangular_rows_positive"]), s["triangular_rows_positive"]["converged"]),
              "order creation for the mixed-sign ray: %.3f s" % s["create_mixed"],
              "(every figure includes the solve's validation pass, its two residual passes and the read-backs; the triangular-rows solve",
              "includes calcReciprocalD and its residual passes)", ""]
    return "\n".join(L)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.step:
        res = correct96(False) if a.step == "correct_iterative" else correct96(True) if a.step == "correct_ordered" else solves200()
        json.dump(res, open(a.out, "w"))
        sys.exit(0)
    results, rc = {}, 0
    tmp = os.path.join(ROOT, "prof_out"); os.makedirs(tmp, exist_ok=True)
    for name, limit in STEPS:
        out = os.path.join(tmp, "rays_ordered_%s.json" % name)
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--out", out])
        if rc != 0:
            print("step %s ended with status %d: nothing further is started" % (name, rc)); break
        results[name] = json.load(open(out))
        print(name, json.dumps(results[name]), flush=True)
    txt = report(results)
    print(txt)
    if rc == 0:
        open(os.path.join(ROOT, "profiles", "rays_ordered_timing.txt"), "w").write(txt)
    sys.exit(rc)
