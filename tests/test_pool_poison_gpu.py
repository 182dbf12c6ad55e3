"""A step must not depend on the contents of recycled memory (csrc/ffm_ctx.hip: pool_alloc; include/ffm.h: ffm_debug_pool_poison).

ffm_malloc_uninit hands out blocks of the caching allocator as they are: the Foam layer's arrays (dField::Store -- the coefficient
arrays ffm_fvm_transport fills, the lock-step solve's diagonals and sources), the pyrolysis column's scratch, GAMG's set-up vector.
The padding slots of the native face layout and the ghost rows of such an array hold whatever the previous owner left; every consumer
must gate them by a select, never let them into arithmetic that reaches a real slot or into a reduction.  With
ffm_debug_pool_poison on, every such block -- fresh or recycled, also in the middle of a step -- is filled with one quiet-NaN pattern
first.  Each case runs once with the switch off and once with it on, in the same process, the allocator's cache given back in between
(ffm_ctx_trim): everything returned to the host must be equal BIT FOR BIT, with equal iteration counts.  A NaN that got through would
also show as a solve that runs into maxIter.  The switch counts the blocks it filled, so that no case passes without any."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


def _both(ctx, run):
    """run() with the switch off, then on: (result off, result on, blocks poisoned)"""
    ctx.sync(); ctx.trim()
    assert ctx.debug_pool_poison(False) >= 0
    off = run()
    ctx.sync(); ctx.trim()
    ctx.debug_pool_poison(True)
    try:
        on = run()
        ctx.sync()
    finally:
        n = ctx.debug_pool_poison(False)
        ctx.trim()
    return off, on, n


def _equal(tag, a, b):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            _equal((tag, k), a[k], b[k])
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), tag
        for k, (x, y) in enumerate(zip(a, b)):
            _equal((tag, k), x, y)
    elif isinstance(a, np.ndarray) and a.dtype == np.float64:
        assert not np.isnan(a).any(), tag
        assert np.array_equal(bits(a), bits(b)), tag
    else:
        assert a == b, (tag, a, b)


@pytest.mark.parametrize("n", [(9, 8, 7), (24, 20, 18)])
def test_b1_demo_with_poisoned_allocations(O, ffm, ctx, n):
    """the inputs of test_foam_layer_gpu.py::test_b1_demo_matches_oracle, and the same on a box whose sweeps are tiled"""
    from b1_case import b1_inputs, run_b1_demo

    def run():
        I = b1_inputs(O, ffm, ctx, n)
        if n[0] > 20:
            assert I.A.sweep_mode == 2
        ns, out, nit = run_b1_demo(ffm, ctx, I)
        I.mesh.close(); I.A.close()
        return ns, out, nit
    off, on, poisoned = _both(ctx, run)
    print("b1_demo %s: %d blocks handed out poisoned, iterations %s" % (n, poisoned, on[2][:6]))
    assert off[0] == on[0] == 6 and poisoned > 0
    _equal("b1_demo", off, on)


def test_dfield_semantics_with_poisoned_allocations(ffm, ctx):
    lib = C.CDLL(os.path.join(os.path.dirname(ffm.libpath()), "libffm_b1demo.so"))
    dp = C.POINTER(C.c_double)
    lib.b1_dfield_semantics.restype = C.c_int
    lib.b1_dfield_semantics.argtypes = [C.c_void_p, C.c_int, dp, dp, C.POINTER(C.c_int)]
    rng = np.random.default_rng(11)
    os.environ["FFM_FOAM_QUIET"] = "1"
    for n in (1, 777, 300001):
        a = rng.standard_normal(n); b = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
        ev = C.c_int()
        run = lambda: lib.b1_dfield_semantics(ctx.h, n, a.ctypes.data_as(dp), b.ctypes.data_as(dp), C.byref(ev))
        off, on, poisoned = _both(ctx, run)
        assert off == 0 and on == 0 and poisoned > 0, (n, off, on, poisoned)


def test_class_layer_sequence_with_poisoned_allocations(O, ffm, ctx):
    """examples/b1_demo.C: b1_solve_sequence -- scalar solves sharing coefficient arrays, the lock-step vector solve (its diagonals and
    sources are uninitialised blocks), GAMG and PCG on the pressure-like equation -- on a box whose sweeps are tiled"""
    from b1_case import run_solve_sequence, sequence_inputs

    def run():
        I = sequence_inputs(O, ffm, ctx)
        assert I.A.sweep_mode == 2
        r = run_solve_sequence(ffm, ctx, I)
        I.G.close(); I.mesh.close(); I.A.close()
        return r
    off, on, poisoned = _both(ctx, run)
    print("b1_solve_sequence: %d blocks handed out poisoned, iterations %s" % (poisoned, on[3]))
    assert off[0] == on[0] == 14 and poisoned > 0
    assert max(on[3]) < 1000                       # no solve ran into maxIter
    _equal("b1_solve_sequence", off, on)


def test_pyrolysis_incident_with_poisoned_allocations(ffm, ctx):
    """config 1 (tests/golden/pyrolysis1d_case_data.json): step_incident and run_incident, and solidRegionDiffNo of the stepped panel
    (ffm_pyro_diff_no: a maximum over an uninitialised scratch block whose size class is larger than the panel)"""
    from test_pyrolysis_incident_gpu import FIELDS, _columns_Qr, _config1
    nCol = 257
    names = FIELDS + ("Twall", "qSurf", "phiGas", "Tsurf")

    def run():
        _, stepped, dt, n, every = _config1(ffm, ctx, nCol, _columns_Qr(nCol))
        _, one, _, _, _ = _config1(ffm, ctx, nCol, _columns_Qr(nCol))
        for _ in range(100):
            stepped.step_incident(dt)
        H = one.run_incident(dt, n, sampleEvery=every)
        r = ({k: stepped.field(k) for k in names}, {k: one.field(k) for k in names}, H, np.array([stepped.diff_no(dt), one.diff_no(dt)]))
        stepped.close(); one.close()
        return r
    off, on, poisoned = _both(ctx, run)
    print("pyrolysis config 1: %d blocks handed out poisoned" % poisoned)
    assert off[1]["Yw"].min() < 0.5 and poisoned > 0               # the run reached charring
    _equal("pyrolysis", off, on)


@pytest.mark.parametrize("smoother", ["GaussSeidel", "DIC"])
def test_gamg_through_the_foam_layer_with_poisoned_allocations(O, ffm, ctx, smoother):
    from b1_case import gamg_layer_inputs, run_gamg_layer

    def run():
        I = gamg_layer_inputs(O, ffm, ctx)           # (the agglomeration is built inside: ffm_gamg_create's set-up vector)
        r = run_gamg_layer(ffm, ctx, I, smoother)
        I.G.close(); I.mesh.close(); I.A.close()
        return r
    off, on, poisoned = _both(ctx, run)
    print("GAMG %s through the Foam layer: %d blocks handed out poisoned, %d V-cycles" % (smoother, poisoned, on[0]))
    assert 2 <= on[0] < 1000 and poisoned > 0
    _equal("b1_gamg_solve", off, on)
