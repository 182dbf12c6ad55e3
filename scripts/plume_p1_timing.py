"""Times the compiled plume step with the P1 radiation model beside the janaf thermo and the EDC (profiles/plume_p1_timing.txt).
Usage:  python scripts/plume_p1_timing.py <checkout root> <mode> <windows> [steps per window] [n] [warm-up steps]
  off        every model off (runs on any checkout: the yardstick is the parent commit's); windows of steps
  p1         kEqn + thermo + EDC + ffm_plume_set_radiation_thermo + set_radiation_p1(solverFreq 100, 0.1, 0.5, 0.22, emissivity 1): every
             step timed on its own over <windows> * 100 + 1 steps after the warm-up; the steps whose number is a multiple of 100 are the
             correct() steps (the P1 assembly, the G solve, qr, the separate EEqn), the others carry the Sh source in the five-system pass
  rad        the same physics with the 32 rays of set_radiation(solverFreq 100) + set_radiation_model(0.1, 0.5, 0.22) instead (any checkout
             that has ffm_plume_set_radiation_thermo: the parent's figure beside P1's)
  assemble   ffm_p1_assemble_d alone on the plume's n^3 mesh (constant a and e, an emission field: the plume's form) against the chain of
             entry points it restates, the chain's cell algebra as torch passes; TB/s of the algorithmic bytes computed from the shapes
  all <out>  the whole measurement in one command: processes of _variants/parent and of this checkout in turn (off, three pairs), p1, the
             parent's rad, assemble, and assemble once more under `rocprofv3 --kernel-trace --stats` for the kernel's own time; every
             process' JSON line is appended to <out> (the figures at the head of profiles/plume_p1_timing.txt are read off these lines)
FFM_PLUME_UNFUSED=1 in the environment gives the per-operator form of a step mode.  One process is one case; host clock around steps that
end in the step's stream synchronise."""
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import time

root, mode = sys.argv[1], sys.argv[2]
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
FREQ = 100

if mode == "all":
    out = sys.argv[3]
    me = os.path.abspath(__file__)
    parent = os.path.join(REPO, "_variants", "parent")

    def run(args, env=None, pre=()):
        p = subprocess.run(list(pre) + [sys.executable, me] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=600)
        line = [l for l in p.stdout.splitlines() if l.startswith("{")]
        with open(out, "a") as f:
            f.write((line[-1] if line else json.dumps(dict(args=args, failed=p.returncode, stderr=p.stderr[-400:]))) + "\n")
        if p.returncode != 0:
            sys.exit("a process failed (%d): %s\n%s" % (p.returncode, args, p.stderr[-2000:]))      # nothing more is started on the GPU
    for _ in range(3):
        run([parent, "off", "4", "10"]); run([REPO, "off", "4", "10"])
    run([REPO, "p1", "2"])
    run([parent, "rad", "2"])
    run([REPO, "assemble", "5", "50"])
    prof = os.path.join(os.path.dirname(os.path.abspath(out)), "p1_assemble_trace")
    run([REPO, "assemble", "2", "20"], pre=["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "p1", "--output-format", "csv", "--"])
    for path in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
        rows = [l for l in open(path).read().splitlines() if "k_p1_" in l or "k_fvm_transport" in l or "k_interpolate" in l or "k_add_boundary" in l or "k_boundary_coeffs" in l]
        with open(out, "a") as f:
            f.write("kernel trace (%s): name, calls, total ns, average ns, ...\n" % os.path.basename(path) + "\n".join(rows) + "\n")
    sys.exit(0)

windows = int(sys.argv[3])
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 10
n = int(sys.argv[5]) if len(sys.argv) > 5 else 200
warm = int(sys.argv[6]) if len(sys.argv) > 6 else 3
sys.path.insert(0, root)
import numpy as np  # noqa: E402
from ffm_import import ffm  # noqa: E402

DATA = json.load(open(os.path.join(REPO, "tests", "golden", "steckler_case_data.json")))
RR = 6.0221417930e26 * 1.38065e-23                      # J/(kmol K), oracle/thermo.py's
S_O2, Q_FUEL = 3.6282945015670283, 46357150.94670516    # thermo.SingleStep of the committed reaction
SIGMA = 5.670367e-8

ctx = ffm.Context(0)
case = ffm.Plume(ctx, (n, n, n))

if mode == "assemble":
    mesh = case.mesh()
    N, B, nNat, F = case.nCells, mesh.nBoundary, mesh.nNative, case.nFaces
    r = np.random.RandomState(1)
    T, E, Tb, em = ctx.to_device(r.uniform(300, 1500, N)), ctx.to_device(r.uniform(0, 5e4, N)), ctx.to_device(r.uniform(300, 900, B)), ctx.to_device(np.ones(B))
    up, dg, sr, gb, fb, rb = ctx.zeros(nNat), ctx.zeros(N), ctx.zeros(N), ctx.zeros(B), ctx.zeros(B), ctx.zeros(B)
    a = 0.1
    L, P = ffm.lib(), (lambda t: C.c_void_p(t.data_ptr()))

    def one_pass():
        assert L.ffm_p1_assemble_d(mesh.h, 0.0, SIGMA, None, a, None, None, a, P(E), P(T), P(Tb), P(em), P(up), P(dg), P(sr), P(gb), P(fb), P(rb)) == 0
    gam, gf, d1, u1, f1, r1, ic, bc, zb, d2, s2 = (ctx.zeros(N), ctx.zeros(nNat), ctx.zeros(N), ctx.zeros(nNat), ctx.zeros(B), ctx.zeros(B), ctx.zeros(B),
                                                   ctx.zeros(B), ctx.zeros(B), ctx.zeros(N), ctx.zeros(N))
    V = ctx.to_device(np.full(N, 0.05 ** 3))               # (the plume's default cell size)
    stream = ctx.torch.cuda.ExternalStream(L.ffm_ctx_stream(ctx.h))

    def chain():
        assert L.ffm_p1_gamma_d(ctx.h, N, None, a, 0.0, P(gam)) == 0 and L.ffm_p1_gamma_d(ctx.h, B, None, a, 0.0, P(gb)) == 0
        assert L.ffm_fvc_interpolate(mesh.h, None, P(gam), P(gf)) == 0
        assert L.ffm_fvm_transport(mesh.h, 0.0, None, None, None, P(gf), 1, P(d1), P(u1), None) == 0
        assert L.ffm_p1_marshak_coeffs_d(mesh.h, SIGMA, P(gb), P(Tb), P(em), P(f1), P(r1)) == 0
        assert L.ffm_fvm_boundary_coeffs(mesh.h, None, P(gb), 1, P(f1), P(r1), P(zb), P(ic), P(bc)) == 0
        with ctx.torch.cuda.stream(stream):                # the cell algebra on the library's stream: diag -= V a; source = V su
            d1.sub_(V * a)
            T2 = T * T
            su = V * (-(4.0 * ((a * SIGMA) * (T2 * T2))) - E)
        assert L.ffm_fvm_add_boundary(mesh.h, P(ic), P(bc), P(d1), P(su), None, P(d2), P(s2)) == 0

    def timed(launch, per_window):
        ms = []
        for w in range(windows + 1):                        # (the first window warms up)
            ctx._ready(); ctx.sync()
            t0 = time.perf_counter()
            for _ in range(per_window):
                launch()
            ctx.sync()
            if w:
                ms.append((time.perf_counter() - t0) / per_window * 1e3)
        return ms
    m1 = timed(one_pass, steps)
    mc = timed(chain, max(steps // 5, 1))
    # algorithmic bytes of the one-pass form from the shapes: per cell T, E, V read and diag, source written; per face the weight, |Sf| and
    # delta read, the neighbour index read by both cells of the face, the coefficient written; per boundary face T_b, emissivity, |Sf_b|,
    # delta_b and the face's place in its cell's list read, gamma_b, valueFraction, refValue written
    nbytes = N * 8 * (3 + 2) + F * (8 * 3 + 4 * 2 + 8) + B * (8 * 4 + 4 + 8 * 3)
    best = min(m1)
    print(json.dumps(dict(root=root, mode=mode, n=n, cells=N, faces=F, boundary_faces=B, launches=steps, ms_one_pass=[round(v, 4) for v in m1],
                          min_one_pass=round(best, 4), bytes_per_cell=round(nbytes / N, 1), TBps=round(nbytes / (best * 1e-3) / 1e12, 3),
                          share_of_8TBps=round(nbytes / (best * 1e-3) / 8e12, 3), ms_chain=[round(v, 4) for v in mc],
                          min_chain=round(min(mc), 4) if mc else None)), flush=True)
    case.close(); ctx.close()
    sys.exit(0)

th = None
if mode != "off":
    i = np.arange(n ** 3)
    x, y, z = (i % n + 0.5) / n, ((i // n) % n + 0.5) / n, (i // (n * n) + 0.5) / n
    case.set_turbulence(k0=2.0e-3 * (1.0 + 0.5 * (0.3 * x + 0.45 * y + 0.25 * z)))
    th = ffm.Thermo(ctx, DATA["species"], DATA["table"], RR)
    case.set_thermo(th)
    case.set_combustion("EDC", 4.0, 0.0, 1.0, s=S_O2, qFuel=Q_FUEL)
    case.set_radiation_thermo(True)
    if mode == "p1":
        case.set_radiation_p1(FREQ, 0.1, 0.5, 0.22, wallEmissivity=1.0)
    else:
        case.set_radiation(solverFreq=FREQ)
        case.set_radiation_model(0.1, 0.5, 0.22)
for _ in range(warm):
    case.step()
if mode == "off":
    ms = []
    for _ in range(windows):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            case.step()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    out = dict(ms_per_step=[round(v, 3) for v in ms], min=round(min(ms), 3), median=round(float(np.median(ms)), 3))
else:
    each, corr, logs = [], [], []
    for k in range(warm, warm + windows * FREQ + 1):
        ctx.sync()
        t0 = time.perf_counter()
        case.step()
        dt = (time.perf_counter() - t0) * 1e3
        if k % FREQ == 0:
            corr.append(dt); logs.append(case.solves())
        else:
            each.append(dt)
    out = dict(steps=len(each), min=round(min(each), 3), median=round(float(np.median(each)), 3), last_20_median=round(float(np.median(each[-20:])), 3),
               correct_steps_ms=[round(v, 3) for v in corr],
               correct_step_solves=[[(nm, p["nIterations"]) for nm, p in log if not nm.startswith("I")] for log in logs],
               G_iterations=[p["nIterations"] for log in logs for nm, p in log if nm == "G"],
               ray_iterations=sorted(set(p["nIterations"] for log in logs for nm, p in log if nm.startswith("I"))))
print(json.dumps(dict(root=root, mode=mode, unfused=bool(os.environ.get("FFM_PLUME_UNFUSED")), n=n, **out,
                      solves=[(nm, p["nIterations"]) for nm, p in case.solves()])), flush=True)
case.close()
if th is not None:
    th.close()
ctx.close()
