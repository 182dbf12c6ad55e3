"""A solve of the Foam layer must not inherit the previous solve's layouts (include/ffmFoam.H: fvMatrix::solve, fvMesh::boundUpper /
boundLower / boundEpoch; csrc/ffm_tile.hip: tile_coef).

fvMatrix::solve() binds its coefficient arrays into the mesh's one matrix handle and may tell the library `the off-diagonals are those
of the previous call` (ffm_ldu_bind_coeffs_native_d, offDiagUnchanged), which keeps the gathered tile layouts of the sweeps.  That is
only true while nobody else has used the handle in between: the lock-step solve of a vector equation, GAMG, or a direct
ffm_ldu_set_coeffs* all give it other off-diagonals.  examples/b1_demo.C: b1_solve_sequence runs the orders that expose it on a box
whose sweeps are tiled (otherwise offDiagUnchanged has no effect and the test would be vacuous):

    R1 YiEqn -> UEqn (lock step) -> R2 the same YiEqn again
    R3 YjEqn (coefficient arrays shared with YiEqn: fvMesh::transportCache) -> UEqn -> R4 YjEqn again
    R5 p_rghEqn (PCG + DIC) -> another user sets and solves its own system on mesh.ldu -> R6 p_rghEqn again -> GAMG -> R7 p_rghEqn again

Required: R1 == R2, R3 == R4, R5 == R6 == R7 bit for bit with equal iteration counts and residuals (the same kernels on the same
inputs: deterministic two-stage reductions, bitwise sweeps); R1 and R5 equal to the oracle's solve of the same system at the bars of
test_foam_layer_gpu.py::test_b1_demo_matches_oracle (1e-8 rel-L2, identical iteration counts).  The shared-coefficient fast path must
survive the fix: between R2 and R3 -- two consecutive specie solves on the same arrays -- the library's off-diagonal generation
(ffm_ldu_offdiag_epoch) does not move, i.e. nothing was gathered again; after every vector solve and after the other user it does."""
import numpy as np
import pytest

from common import rel_l2

pytestmark = pytest.mark.gpu


def test_solves_after_other_users_of_the_matrix_handle(O, ffm, ctx):
    from oracle import fv
    from b1_case import run_solve_sequence, sequence_inputs
    I = sequence_inputs(O, ffm, ctx)
    A, mesh, G, m, N, cOrd = I.A, I.mesh, I.G, I.m, I.N, I.cOrd
    assert A.sweep_mode == 2 and A.native_order
    alphaY, rdt, ctl, phi, phib, rho_old, rho_now = I.alphaY, I.rdt, I.ctl, I.phi, I.phib, I.rho_old, I.rho_now
    Yi0, Yj0, dEff, Ri, bcY, bcP, psi, gam, p0, S = I.Yi0, I.Yj0, I.dEff, I.Ri, I.bcY, I.bcP, I.psi, I.gam, I.p0, I.S

    # ------------------------------------------------------------------ the oracle's R1 and R5
    Yb, Yjb = bcY.values(m, Yi0), bcY.values(m, Yj0)
    lim = np.minimum(fv.limited_limiter(m, "limitedLinear01", phi, Yi0, fv.grad(m, Yi0, Yb), 1.0),
                     fv.limited_limiter(m, "limitedLinear01", phi, Yj0, fv.grad(m, Yj0, Yjb), 1.0))     # the common limiter of the two species
    w = lim * m.weights + (1.0 - lim) * fv.pos0(phi)
    dEf, dEb = fv.interpolate(m, dEff, [dEff[p.faceCells] for p in m.patches])
    M = fv.fvm_ddt(m, rdt, rho_now, rho_old, Yi0); M += fv.fvm_div(m, phi, phib, w, [bcY]); M -= fv.fvm_laplacian(m, dEf, dEb, [bcY])
    M.add_su(Ri)
    M.relax(alphaY, Yi0[None])
    d, s = M.solve_system(0)
    Yi_ref, pfY = O.Ldu(N, m.l, m.u).set_coeffs(d, M.upper, M.lower).solve(O.PBICGSTAB, O.DILU, Yi0, s, **ctl)
    gf, gfb = fv.interpolate(m, gam, [gam[p.faceCells] for p in m.patches])
    E = fv.fvm_ddt(m, rdt, psi, psi, p0)
    E -= fv.fvm_laplacian(m, gf, gfb, [bcP])
    E.add_su(S)
    d, s = E.solve_system()
    p_ref, pfP = O.Ldu(N, m.l, m.u).set_coeffs(d, E.upper, None).solve(O.PCG, O.DIC, p0, s, **ctl)
    assert pfY["nIterations"] >= 2 and pfP["nIterations"] >= 5

    # ------------------------------------------------------------------ the C++ layer on the device
    ns, fields, gamgOut, nit, res, ep = run_solve_sequence(ffm, ctx, I)
    assert ns == 14                  # R1, U x 3, R2, R3, U x 3, R4, R5, R6, GAMG, R7
    R = [fields[k] for k in range(7)]
    iR = [0, 4, 5, 9, 10, 11, 13]    # where R1 .. R7 stand in the log
    print("iterations", nit, "\noff-diagonal generations", ep)
    for a, b in ((0, 1), (2, 3), (4, 5), (4, 6)):
        print("R%d vs R%d: rel-L2 %.3e, iterations %d / %d" % (a + 1, b + 1, rel_l2(R[b], R[a]), nit[iR[a]], nit[iR[b]]))
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    for a, b in ((0, 1), (2, 3), (4, 5), (4, 6)):
        assert nit[iR[a]] == nit[iR[b]], (a + 1, b + 1, nit)
        assert np.array_equal(bits(res[iR[a]]), bits(res[iR[b]])), (a + 1, b + 1, res[iR[a]], res[iR[b]])
        assert np.array_equal(bits(R[a]), bits(R[b])), (a + 1, b + 1, rel_l2(R[b], R[a]))
    # against the oracle
    back = lambda a: (lambda o: (o.__setitem__((Ellipsis, cOrd), a), o)[1])(np.empty_like(a))
    assert nit[0] == pfY["nIterations"] and nit[10] == pfP["nIterations"], (nit, pfY, pfP)
    assert rel_l2(back(R[0]), Yi_ref) < 1e-8
    assert rel_l2(back(R[4]), p_ref) < 1e-8
    assert min(nit[1:4]) >= 1 and nit[12] >= 2               # the vector solve and GAMG did work in between
    assert np.all(np.isfinite(gamgOut)) and not np.array_equal(gamgOut, p0[cOrd])
    # the library's off-diagonal generation: after R1, UEqn, R2, R3, UEqn, R4, R5, the other user, R6
    assert ep[1] > ep[0] and ep[2] > ep[1]                   # the vector solve took the layouts, YiEqn's second solve renewed them
    assert ep[3] == ep[2]                                    # YjEqn on YiEqn's arrays right after it: nothing gathered again
    assert ep[4] > ep[3] and ep[5] > ep[4]
    assert ep[7] > ep[6] and ep[8] > ep[7]                   # the other user, then p_rghEqn renewed
    G.close(); mesh.close(); A.close()
