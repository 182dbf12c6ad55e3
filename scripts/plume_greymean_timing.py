"""Times the greyMeanAbsorptionEmission kernels and the plume step beside them (profiles/plume_greymean_timing.txt).
Usage:  python scripts/plume_greymean_timing.py <checkout root> <mode> <windows> [launches or steps per window] [n] [warm-up steps]
  off     the compiled plume step with every model off (runs on any checkout: the yardstick is the parent commit's, whose launches this
          change leaves as they are); windows of steps, as scripts/plume_radiation_timing.py
  a       ffm_greymean_a_d alone on n^3 cells of a flame-like five-species state with the case's CO2 / H2O / CH4 table: windows of launches,
          GB/s of its own (nSpecies + 3) doubles per cell
  sh      ffm_radiation_sh_greymean_d (one pass, a written) against the chain ffm_greymean_a_d, ffm_greymean_E_d, ffm_radiation_sh_v_d in the
          same process, alternating windows: ms and GB/s of each form's own bytes, and whether the outputs are bitwise equal
  rays, rays+gm, p1, p1+gm
          the plume step with kEqn + janaf thermo + EDC and the rays (32, solverFreq 20, model 0.1 / 0.5 / 0.22) or P1 (solverFreq 20, 0.1 /
          0.3 / 0.3, wall emissivity 0.8), with the constant or (+gm) with greyMeanAbsorptionEmission (CO2, H2O of the case data, EhrrCoeff
          0.3): every step timed on its own over <windows> * 20 + 1 steps after the warm-up; the steps whose number is a multiple of 20
          carry a correct().  Iteration counts differ with the physics: information, not a claim
One process is one case; host clock around launches that end in a stream synchronise.  Two checkouts are compared by alternating
processes of this script in one job."""
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
SIGMA = 5.670367e-8
SPECIES = ["CH4", "O2", "N2", "H2O", "CO2"]
W = {"O2": 31.9988, "N2": 28.0134, "CO2": 44.01, "H2O": 18.0153, "CH4": 16.04276}

ctx = ffm.Context(0)
P = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731
L = ffm.lib()


def timed(launch, per_window):
    ctx._ready(); ctx.sync()
    t0 = time.perf_counter()
    for _ in range(per_window):
        launch()
    ctx.sync()
    return (time.perf_counter() - t0) / per_window * 1e3


if mode == "off":
    case = ffm.Plume(ctx, (n, n, n))
    for _ in range(warm):
        case.step()
    ms = []
    for _ in range(windows):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            case.step()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    print(json.dumps(dict(root=root, mode=mode, n=n, ms_per_step=[round(v, 3) for v in ms], min=round(min(ms), 3), median=round(float(np.median(ms)), 3),
                          solves=[(nm, p["nIterations"]) for nm, p in case.solves()])), flush=True)
    case.close(); ctx.close()
    sys.exit(0)

FX = json.load(open(os.path.join(os.path.dirname(HERE), "tests", "golden", "greymean_case_data.json")))
if mode in ("rays", "rays+gm", "p1", "p1+gm"):
    DATA = json.load(open(os.path.join(os.path.dirname(HERE), "tests", "golden", "steckler_case_data.json")))
    RR = 6.0221417930e26 * 1.38065e-23                      # J/(kmol K), oracle/thermo.py's
    S_O2, Q_FUEL = 3.6282945015670283, 46357150.94670516    # thermo.SingleStep of the committed reaction
    FREQ = 20
    case = ffm.Plume(ctx, (n, n, n))
    i = np.arange(n ** 3)
    x, y, z = (i % n + 0.5) / n, ((i // n) % n + 0.5) / n, (i // (n * n) + 0.5) / n
    case.set_turbulence(k0=2.0e-3 * (1.0 + 0.5 * (0.3 * x + 0.45 * y + 0.25 * z)))
    th = ffm.Thermo(ctx, DATA["species"], DATA["table"], RR)
    case.set_thermo(th)
    case.set_combustion("EDC", 4.0, 0.0, 1.0, s=S_O2, qFuel=Q_FUEL)
    case.set_radiation_thermo(True)
    if mode.startswith("rays"):
        case.set_radiation(solverFreq=FREQ); case.set_radiation_model(0.1, 0.5, 0.22)
    else:
        case.set_radiation_p1(FREQ, 0.1, 0.3, 0.3, wallEmissivity=0.8)
    gm = None
    if mode.endswith("+gm"):
        part = [sp for sp in FX["species"] if sp in DATA["species"]]
        gm = ffm.GreyMean(ctx, DATA["species"], {sp: DATA["table"][sp]["W"] for sp in DATA["species"]}, {sp: FX["coeffs"][sp] for sp in part}, 0.3, order=part)
        case.set_absorption_emission(gm)
    for _ in range(warm):
        case.step()
    each, sweeps, log = [], [], None
    for k in range(warm, warm + windows * FREQ + 1):
        ctx.sync()
        t0 = time.perf_counter()
        case.step()
        dt = (time.perf_counter() - t0) * 1e3
        if k % FREQ == 0:
            sweeps.append(dt); log = case.solves()
        else:
            each.append(dt)
    print(json.dumps(dict(root=root, mode=mode, n=n, steps=len(each), min=round(min(each), 3), median=round(float(np.median(each)), 3),
                          correct_steps_ms=[round(v, 3) for v in sweeps], correct_step_solves=[(nm, p["nIterations"]) for nm, p in log if not nm.startswith("I")],
                          ray_iterations=sorted(set(p["nIterations"] for nm, p in log if nm.startswith("I"))),
                          solves=[(nm, p["nIterations"]) for nm, p in case.solves()])), flush=True)
    case.close(); th.close()
    if gm is not None:
        gm.close()
    ctx.close()
    sys.exit(0)
N = n ** 3
r = np.random.RandomState(1)
T = r.uniform(300.0, 2400.0, N)
burnt = (T - 300.0) / 2100.0
Y = np.array([0.02 * (1.0 - burnt), 0.23 * (1.0 - burnt) + 0.01, 0.72 - 0.05 * burnt, 0.01 + 0.09 * burnt, 0.01 + 0.15 * burnt])
Y = Y / Y.sum(axis=0)
Yd = [ctx.to_device(np.ascontiguousarray(y)) for y in Y]
Yp = (C.c_void_p * 5)(*[y.data_ptr() for y in Yd])
Td, pd = ctx.to_device(T), ctx.to_device(r.uniform(1.0e5, 1.02e5, N))
gm = ffm.GreyMean(ctx, SPECIES, W, FX["coeffs"], 0.3, order=FX["species"])
flag = ctx.torch.zeros(1, dtype=ctx.torch.int32, device=ctx.device)
a = ctx.empty(N)
nS = len(SPECIES)

if mode == "a":
    def launch():
        assert L.ffm_greymean_a_d(gm.h, N, Yp, P(pd), P(Td), P(a), P(flag)) == 0
    ms = [timed(launch, steps) for _ in range(windows + 1)][1:]                  # (the first window warms up)
    B = 8.0 * (nS + 3)
    print(json.dumps(dict(root=root, mode=mode, n=n, launches=steps, ms_per_pass=[round(v, 4) for v in ms], min=round(min(ms), 4),
                          bytes_per_cell=B, GBps=round(B * N / (min(ms) * 1e-3) / 1e9, 1), flag=int(flag.cpu()[0]))), flush=True)
else:
    G, he, Q, Cp = [ctx.to_device(r.uniform(lo, hi, N)) for lo, hi in ((0, 4e5), (-6e4, 3.5e6), (0, 5e6), (900, 2500))]
    E, su, sp, a1, su1, sp1 = (ctx.empty(N) for _ in range(6))

    def fused():
        assert L.ffm_radiation_sh_greymean_d(gm.h, N, Yp, P(pd), P(Td), SIGMA, P(G), P(he), P(Q), P(Cp), 1005.0, P(a1), P(su1), P(sp1), P(flag)) == 0

    def chain():
        assert L.ffm_greymean_a_d(gm.h, N, Yp, P(pd), P(Td), P(a), P(flag)) == 0
        assert L.ffm_greymean_E_d(gm.h, N, P(Q), P(E)) == 0
        assert L.ffm_radiation_sh_v_d(ctx.h, N, P(a), P(a), SIGMA, P(E), P(G), P(Td), P(he), P(Cp), 1005.0, P(su), P(sp)) == 0
    ctx._ready(); fused(); chain(); ctx.sync()
    same = all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in ((a, a1), (su, su1), (sp, sp1)))
    mf, mc = [], []
    for w in range(windows + 1):
        f, c = timed(fused, steps), timed(chain, steps)
        if w:
            mf.append(f); mc.append(c)
    Bf, Bc = 8.0 * (nS + 6 + 3), 8.0 * ((nS + 3) + 2 + 8)          # fused: Y p T G he Qdot Cp in, a su sp out; chain: a pass, E pass, a E G T he Cp in + su sp out
    print(json.dumps(dict(root=root, mode=mode, n=n, launches=steps, bitwise_equal=bool(same), ms_fused=[round(v, 4) for v in mf], ms_chain=[round(v, 4) for v in mc],
                          min_fused=round(min(mf), 4), min_chain=round(min(mc), 4), bytes_per_cell_fused=Bf, bytes_per_cell_chain=Bc,
                          GBps_fused=round(Bf * N / (min(mf) * 1e-3) / 1e9, 1), GBps_chain=round(Bc * N / (min(mc) * 1e-3) / 1e9, 1))), flush=True)
gm.close(); ctx.close()
