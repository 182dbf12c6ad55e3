"""The P1 handle of include/fireFoamHandles.H (class P1: correct() in the reference's vocabulary through the class layer's operators,
G's patch condition a mixedBC whose hook is ffm_p1_marshak_coeffs_d, qr from ffm_p1_wall_flux_d) driven through b1_p1 of
examples/b1_demo.C, against tests/p1_ref.py: the (7, 8, 6) box with a flame-like hot spot, an emission field handed in through the
handle's emission provider, scattering, and one emissivity per patch (0.3, 0.85, 1.0, 0.55, as tests/test_fvdom_gpu.py has them), three
calls of correct() with solverFreq 1 -- the same PCG iteration count in every call, G, G_b and qr within 1e-8.  And the system the class
layer's operators leave for the solver equals the one-pass kernel's (ffm_p1_assemble_d) bit for bit.  Unpinned by reference data: the
reference ships no output of a P1 run."""
import ctypes as C
import os

import numpy as np
import pytest

import foam_case
import merged_mesh as MM
import p1_ref as P1
from common import rel_l2

pytestmark = pytest.mark.gpu


def test_p1_handle_against_the_restatement(O, ffm, ctx):
    from oracle import plume
    lib = C.CDLL(os.path.join(os.path.dirname(ffm.libpath()), "libffm_b1demo.so"))
    s = MM.device_mesh(ffm, ctx, plume.make_mesh((7, 8, 6)))
    m, mesh, A, N, B, cOrd = s["m"], s["mesh"], s["A"], s["N"], s["B"], s["cOrd"]
    T, Tb, E, emis = foam_case.fvdom_inputs(m)
    E = 0.02 * E                                                 # a few percent of 4 e sigma T^4 in the hot spot
    a, e, sigma_s, Cs, tol, nCalls = 0.3, 0.45, 0.2, 0.5, 1e-6, 3
    ref = P1.P1(O, m, a, e, sigma_s, Cs, solverFreq=1, tolerance=tol, emissivity=emis)
    for _ in range(nCalls):
        assert ref.correct(T, Tb, E)
    dp = C.POINTER(C.c_double)
    h = lambda v: np.ascontiguousarray(v, np.float64)
    P = lambda v: v.ctypes.data_as(dp)
    Tc, Tbb, Ec, emb = h(T[cOrd]), h(np.concatenate(Tb)), h(E[cOrd]), h(np.concatenate(emis))
    G, Gb, qr = np.empty(N), np.empty(B), np.empty(B)
    nSys = mesh.nNative + 2 * N
    sysC, sysF = np.empty(nSys), np.empty(nSys)
    iters = (C.c_int * nCalls)()
    lib.b1_p1.restype = C.c_int
    lib.b1_p1.argtypes = [C.c_void_p] * 3 + [C.c_double] * 4 + [dp] * 4 + [C.c_double, C.c_int] + [dp] * 3 + [C.POINTER(C.c_int)] + [dp] * 2
    os.environ["FFM_FOAM_QUIET"] = "1"
    ctx._ready()
    n = lib.b1_p1(ctx.h, A.h, mesh.h, a, e, sigma_s, Cs, P(Tc), P(Tbb), P(Ec), P(emb), tol, nCalls, P(G), P(Gb), P(qr), iters, P(sysC), P(sysF))
    assert n == nCalls                                           # one solve logged per call
    want = [pf["nIterations"] for pf in ref.log]
    print("iterations %s (restatement %s)" % (list(iters), want))
    assert list(iters) == want and want[0] > 3
    Go = np.empty(N); Go[cOrd] = G
    errs = dict(G=rel_l2(Go, ref.G), G_b=rel_l2(Gb, np.concatenate(ref.G_b)), qr=rel_l2(qr, np.concatenate(ref.qr)))
    print(", ".join("%s %.2e" % kv for kv in errs.items()))
    assert all(v < 1e-8 for v in errs.values()), errs
    assert np.abs(qr).max() > 0 and np.ptp(Go) > 0
    # the class layer's system == the one-pass kernel's
    # (upper in the native layout: the faces' own entries are compared, the layout's padding entries belong to nobody)
    nNat, fm = mesh.nNative, A.face_map()
    assert len(fm) == s["F"] and len(np.unique(fm)) == s["F"]
    for name, c, f in (("upper", sysC[:nNat][fm], sysF[:nNat][fm]), ("diag", sysC[nNat:nNat + N], sysF[nNat:nNat + N]),
                       ("source", sysC[nNat + N:], sysF[nNat + N:])):
        assert np.isfinite(c).all() and np.array_equal(c, f), name
    assert np.abs(sysC[:nNat][fm]).min() > 0
    mesh.close(); A.close()
