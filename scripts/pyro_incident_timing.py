"""Times the pyrolysis column kernels on a panel of 2^20 columns x 8 layers over 100 steps of 0.2 s with config 1's selections
(profiles/pyro_incident_timing.txt).  Usage:  python scripts/pyro_incident_timing.py <checkout root> <modes> <repeats> [log2 nCol]
  a  ffm_pyro_step loop with a given flux (runs on any checkout that has the column kernel: the yardstick is the parent commit's)
  b  ffm_pyro_step_incident loop          c  one ffm_pyro_run_incident, no history          d  the same with sampleEvery = 10
Every window starts from a fresh panel; window 0 of every mode is the warm-up; host clock around work that ends in a device
synchronise.  Two checkouts are compared by alternating processes of this script in one job."""
import ctypes as C
import json
import sys
import time

root, modes, reps = sys.argv[1], sys.argv[2], int(sys.argv[3])
lg = int(sys.argv[4]) if len(sys.argv) > 4 else 20
sys.path.insert(0, root)
import numpy as np  # noqa: E402
from ffm_import import ffm  # noqa: E402

nCol, nLay, nSteps, dt = 1 << lg, 8, 100, 0.2
ctx = ffm.Context(0)
SEL = dict(model="reactingOneDim", alphaScheme="harmonic", kappaScheme="harmonic", back=("constH", 0.0, 298.15),
           radiation=dict(v=(0.17, 0.17), char=(0.85, 0.85)))


def panel():
    p = ffm.PyrolysisPanel(ctx, nCol, nLay, thickness=0.0234, area=0.01)
    p.set_model(**SEL)
    if hasattr(p, "set_incident_radiation"):
        p.set_incident_radiation(6.0e4)
    return p


qd = ctx.to_device(np.full(nCol, 1.0e4))
histCap = (nSteps // 10) * (2 + 4 * nLay) * nCol
hist = ctx.zeros(histCap) if "d" in modes else None


def window(mode, p):
    ctx.sync()
    t0 = time.perf_counter()
    if mode == "a":
        for _ in range(nSteps):
            p.step(dt, qd)
    elif mode == "b":
        for _ in range(nSteps):
            p.step_incident(dt)
    elif mode == "c":
        assert ffm.lib().ffm_pyro_run_incident(p.h, dt, nSteps, 1, None, 0) == 0
    elif mode == "d":
        assert ffm.lib().ffm_pyro_run_incident(p.h, dt, nSteps, 10, C.c_void_p(hist.data_ptr()), histCap) == 0
    ctx.sync()
    return time.perf_counter() - t0


res, final = {m: [] for m in modes}, {}
for r in range(reps + 1):
    for m in modes:
        p = panel()
        t = window(m, p)
        if r:
            res[m].append(t)
        if r == reps:
            final[m] = (p.field("T")[::4097], p.field("Yw")[::4097])
        p.close()
for m in modes:
    v = np.array(res[m]) * 1e3
    print(json.dumps(dict(root=root, mode=m, nCol=nCol, nSteps=nSteps, ms_per_100_steps=[round(x, 3) for x in v], min=round(v.min(), 3),
                          median=round(float(np.median(v)), 3))), flush=True)
same = lambda x, y: all(np.array_equal(u, w) for u, w in zip(final[x], final[y]))
if "b" in final and "c" in final:
    print("final state b == c bitwise:", same("b", "c"), flush=True)
if "c" in final and "d" in final:
    print("final state c == d bitwise:", same("c", "d"), flush=True)
ctx.close()
