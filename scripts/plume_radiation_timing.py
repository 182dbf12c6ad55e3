"""Times the compiled plume step with the fvDOM rays and radiation->Sh beside the janaf thermo and the EDC (profiles/plume_radiation_timing.txt).
Usage:  python scripts/plume_radiation_timing.py <checkout root> <mode> <windows> [steps per window] [n] [warm-up steps]
  off       every model off (runs on any checkout: the yardstick is the parent commit's); windows of steps, as scripts/plume_thermo_timing.py
  full      kEqn + thermo + EDC, no radiation; every step timed on its own
  rad       full + ffm_plume_set_radiation_thermo, set_radiation(solverFreq 100), set_radiation_model(0.1, 0.5, 0.22); every step timed on
            its own over <windows> * 100 + 1 steps after the warm-up: the steps whose number is a multiple of 100 are the sweep steps
            (32 ray solves, the separate EEqn), the others carry the Sh source in the five-system pass
  sh        ffm_radiation_sh_d alone on n^3 cells with a Cp field: <windows> windows of <steps> launches, GB/s of its 56 B/cell
  G         ffm_fvdom_G_d over 32 rays on n^3 cells against 32 one-pass launches G' = G + I_i*omega_i (ffm_field_eval, ping-pong between two
            buffers: the 3 doubles per cell and launch of the passes it replaces, whose kernel is private to the driver)
FFM_PLUME_UNFUSED=1 in the environment gives the per-operator form of a step mode.  One process is one case; host clock around steps that
end in the step's stream synchronise.  Two checkouts are compared by alternating processes of this script in one job."""
import ctypes as C
import json
import os
import sys
import time

root, mode, windows = sys.argv[1], sys.argv[2], int(sys.argv[3])
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 10
n = int(sys.argv[5]) if len(sys.argv) > 5 else 200
warm = int(sys.argv[6]) if len(sys.argv) > 6 else 3
sys.path.insert(0, root)
import numpy as np  # noqa: E402
from ffm_import import ffm  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = json.load(open(os.path.join(os.path.dirname(HERE), "tests", "golden", "steckler_case_data.json")))
RR = 6.0221417930e26 * 1.38065e-23                      # J/(kmol K), oracle/thermo.py's
S_O2, Q_FUEL = 3.6282945015670283, 46357150.94670516    # thermo.SingleStep of the committed reaction
SIGMA = 5.670367e-8
FREQ = 100

ctx = ffm.Context(0)
P = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731
L = ffm.lib()


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


if mode in ("sh", "G"):
    N = n ** 3
    r = np.random.RandomState(1)
    if mode == "sh":
        G, T, he, Q, Cp = [ctx.to_device(r.uniform(lo, hi, N)) for lo, hi in ((0, 4e5), (250, 2500), (-6e4, 3.5e6), (0, 5e6), (900, 2500))]
        su, sp = ctx.empty(N), ctx.empty(N)

        def launch():
            assert L.ffm_radiation_sh_d(ctx.h, N, 0.1, SIGMA, 0.36, P(G), P(T), P(he), P(Q), P(Cp), 1005.0, P(su), P(sp)) == 0
        ms = timed(launch, steps)
        print(json.dumps(dict(root=root, mode=mode, n=n, launches=steps, ms_per_pass=[round(v, 4) for v in ms], min=round(min(ms), 4),
                              GBps_at_56B_per_cell=round(56.0 * N / (min(ms) * 1e-3) / 1e9, 1))), flush=True)
    else:
        nRay = 32
        rays = [ctx.to_device(r.uniform(0.0, 3e4, N)) for _ in range(nRay)]
        omega = r.uniform(0.05, 0.8, nRay)
        table = ctx.torch.as_tensor(np.array([t.data_ptr() for t in rays], dtype=np.int64), device=ctx.device)
        om = ctx.to_device(omega)
        G, G2 = ctx.zeros(N), ctx.zeros(N)

        def one_pass():
            assert L.ffm_fvdom_G_d(ctx.h, N, nRay, P(table), P(om), P(G)) == 0
        code = (C.c_ushort * 5)(1 << 12 | 0, 1 << 12 | 1, 2 << 12 | 0, 3 << 12 | 2, 3 << 12 | 0)      # G I omega * +
        imms = [(C.c_double * 1)(w) for w in omega]

        def passes():
            a, b = G, G2
            for i in range(nRay):
                ptrs = (C.c_void_p * 2)(a.data_ptr(), rays[i].data_ptr())
                assert L.ffm_field_eval(ctx.h, N, 2, ptrs, 1, imms[i], 5, code, P(b)) == 0
                a, b = b, a
        one_pass(); ctx.sync(); g1 = G.cpu().numpy().copy()
        G.zero_(); G2.zero_(); ctx._ready(); passes(); ctx.sync()
        same = bool(g1.tobytes() == G.cpu().numpy().tobytes())                  # (32 passes: an even count ends in G)
        m1, m32 = timed(one_pass, steps), timed(passes, max(steps // 8, 1))
        print(json.dumps(dict(root=root, mode=mode, n=n, nRay=nRay, bitwise_equal=same, ms_one_pass=[round(v, 4) for v in m1],
                              ms_32_passes=[round(v, 4) for v in m32], min_one_pass=round(min(m1), 4), min_32_passes=round(min(m32), 4),
                              GBps_one_pass_at_264B_per_cell=round(264.0 * N / (min(m1) * 1e-3) / 1e9, 1),
                              GBps_32_passes_at_768B_per_cell=round(768.0 * N / (min(m32) * 1e-3) / 1e9, 1))), flush=True)
    ctx.close()
    sys.exit(0)

case = ffm.Plume(ctx, (n, n, n))
th = None
if mode != "off":
    i = np.arange(n ** 3)
    x, y, z = (i % n + 0.5) / n, ((i // n) % n + 0.5) / n, (i // (n * n) + 0.5) / n
    case.set_turbulence(k0=2.0e-3 * (1.0 + 0.5 * (0.3 * x + 0.45 * y + 0.25 * z)))
    th = ffm.Thermo(ctx, DATA["species"], DATA["table"], RR)
    case.set_thermo(th)
    case.set_combustion("EDC", 4.0, 0.0, 1.0, s=S_O2, qFuel=Q_FUEL)
if mode == "rad":
    case.set_radiation_thermo(True)
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
    total = windows * FREQ + 1 if mode == "rad" else windows * steps
    each, sweeps, log = [], [], None
    for k in range(warm, warm + total):
        ctx.sync()
        t0 = time.perf_counter()
        case.step()
        dt = (time.perf_counter() - t0) * 1e3
        if mode == "rad" and k % FREQ == 0:
            sweeps.append(dt); log = case.solves()
        else:
            each.append(dt)
    out = dict(steps=len(each), min=round(min(each), 3), median=round(float(np.median(each)), 3), last_20_median=round(float(np.median(each[-20:])), 3))
    if sweeps:
        out.update(sweep_steps_ms=[round(v, 3) for v in sweeps], sweep_step_solves=[(nm, p["nIterations"]) for nm, p in log if not nm.startswith("I")],
                   ray_iterations=sorted(set(p["nIterations"] for nm, p in log if nm.startswith("I"))))
print(json.dumps(dict(root=root, mode=mode, unfused=bool(os.environ.get("FFM_PLUME_UNFUSED")), n=n, **out,
                      solves=[(nm, p["nIterations"]) for nm, p in case.solves()])), flush=True)
case.close()
if th is not None:
    th.close()
ctx.close()
