"""Times the compiled plume step with the janaf thermo and the reference's EDC (profiles/plume_thermo_timing.txt).
Usage:  python scripts/plume_thermo_timing.py <checkout root> <mode> <windows> [steps per window] [n] [warm-up steps]
  off       every model off (runs on any checkout: the yardstick is the parent commit's)
  keqn      ffm_plume_set_turbulence(kEqn) only, smooth non-uniform k0
  full      kEqn + ffm_plume_set_thermo(the committed species table) + ffm_plume_set_combustion(EDC 4, 0, 1)
  pass      the fused thermo pass alone (ffm_thermo_step_d) on n^3 cells of a flame-like state: <windows> windows of <steps> launches,
            achieved GB/s against the 96 B/cell it has to move (five Y, h and T read; T, psi, mu, alpha, Cp written)
FFM_PLUME_UNFUSED=1 in the environment gives the per-operator form of a step mode.  One process is one case: n^3 cells (default 200),
the warm-up steps discarded, then <windows> windows of <steps> steps; host clock around steps that end in the step's stream
synchronise.  Two checkouts are compared by alternating processes of this script in one job."""
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

ctx = ffm.Context(0)
if mode == "pass":
    th = ffm.Thermo(ctx, DATA["species"], DATA["table"], RR)
    N = n ** 3
    i = np.arange(N)
    g = np.exp(-(((i % n + 0.5) / n - 0.5) ** 2 + (((i // n) % n + 0.5) / n - 0.5) ** 2 + ((i // (n * n) + 0.5) / n - 0.5) ** 2) / 0.05)
    Y = [0.22 * (1 - 0.5 * g), 0.012 + 0.05 * g, 0.006 + 0.3 * g, 0.015 + 0.08 * g]
    Y.append(1.0 - sum(Y))
    Yd = [ctx.to_device(np.ascontiguousarray(y)) for y in Y]
    T0 = ctx.to_device(300.0 + 1100.0 * g)
    he, T = ctx.empty(N), ctx.empty(N)
    th.he(Yd, T0, he)                                   # the enthalpy of that temperature field; the pass starts 3 % off it
    out = [ctx.empty(N) for _ in range(4)]
    flag = ctx.zeros(1)
    Yp = (C.c_void_p * 5)(*[y.data_ptr() for y in Yd])
    P = lambda t: C.c_void_p(t.data_ptr())
    L = ffm.lib()
    ms = []
    for w in range(windows + 1):
        T.copy_(T0 * 1.03)
        ctx._ready(); ctx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):                          # (from the second launch on T is converged: one Newton iteration, the step's usual case)
            rc = L.ffm_thermo_step_d(th.h, N, Yp, P(he), P(T), *[P(o) for o in out], P(flag))
            assert rc == 0
        ctx.sync()
        if w:
            ms.append((time.perf_counter() - t0) / steps * 1e3)
    print(json.dumps(dict(root=root, mode=mode, n=n, launches=steps, ms_per_pass=[round(v, 4) for v in ms], min=round(min(ms), 4),
                          GBps_at_96B_per_cell=round(96.0 * N / (min(ms) * 1e-3) / 1e9, 1))), flush=True)
    th.close(); ctx.close()
    sys.exit(0)

case = ffm.Plume(ctx, (n, n, n))
th = None
if mode != "off":
    i = np.arange(n ** 3)
    x, y, z = (i % n + 0.5) / n, ((i // n) % n + 0.5) / n, (i // (n * n) + 0.5) / n
    case.set_turbulence(k0=2.0e-3 * (1.0 + 0.5 * (0.3 * x + 0.45 * y + 0.25 * z)))
if mode == "full":
    th = ffm.Thermo(ctx, DATA["species"], DATA["table"], RR)
    case.set_thermo(th)
    case.set_combustion("EDC", 4.0, 0.0, 1.0, s=S_O2, qFuel=Q_FUEL)
for _ in range(warm):
    case.step()
ms = []
for _ in range(windows):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        case.step()
    ms.append((time.perf_counter() - t0) / steps * 1e3)
print(json.dumps(dict(root=root, mode=mode, unfused=bool(os.environ.get("FFM_PLUME_UNFUSED")), n=n, steps=steps,
                      ms_per_step=[round(v, 3) for v in ms], min=round(min(ms), 3), median=round(float(np.median(ms)), 3),
                      solves=[(nm, p["nIterations"]) for nm, p in case.solves()])), flush=True)
case.close()
if th is not None:
    th.close()
ctx.close()
