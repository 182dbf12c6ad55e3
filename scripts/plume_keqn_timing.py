"""Times the compiled plume step with and without the LES kEqn model (profiles/plume_keqn_timing.txt).
Usage:  python scripts/plume_keqn_timing.py <checkout root> <mode> <windows> [steps per window] [n] [warm-up steps]
  off       no sub-grid model (runs on any checkout: the yardstick is the parent commit's)
  on        ffm_plume_set_turbulence(kEqn), smooth non-uniform k0
  trace     `on`, three steps only, h assembled apart from the species (FFM_PLUME_SEPARATE_H=1): the run a kernel trace is taken of
FFM_PLUME_UNFUSED=1 in the environment gives the per-operator form of either.  One process is one case: n^3 cells (default 200),
the warm-up steps discarded, then <windows> windows of <steps> steps; host clock around steps that end in the step's stream
synchronise.  Two checkouts are compared by alternating processes of this script in one job."""
import json
import os
import sys
import time

root, mode, windows = sys.argv[1], sys.argv[2], int(sys.argv[3])
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 10
n = int(sys.argv[5]) if len(sys.argv) > 5 else 200
warm = int(sys.argv[6]) if len(sys.argv) > 6 else 3
if mode == "trace":
    os.environ["FFM_PLUME_SEPARATE_H"] = "1"
sys.path.insert(0, root)
import numpy as np  # noqa: E402
from ffm_import import ffm  # noqa: E402

ctx = ffm.Context(0)
case = ffm.Plume(ctx, (n, n, n))
if mode != "off":
    i = np.arange(n ** 3)
    x, y, z = (i % n + 0.5) / n, ((i // n) % n + 0.5) / n, (i // (n * n) + 0.5) / n
    case.set_turbulence(k0=2.0e-3 * (1.0 + 0.5 * (0.3 * x + 0.45 * y + 0.25 * z)))
if mode == "trace":
    for _ in range(3):
        case.step()
    print(json.dumps(dict(root=root, mode=mode, n=n, solves=[(nm, p["nIterations"]) for nm, p in case.solves()])), flush=True)
else:
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
case.close(); ctx.close()
