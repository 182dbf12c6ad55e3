// ffm_plume.hip -- the synthetic buoyant-plume case of SURVEY 8(d): the handle's life (create / destroy), the hydrostatic start-up
// (solver/phrghEqn.H:25-56), the setters and the getters.  The time step is in ffm_plume_step.hip, the fvDOM stand-in in
// ffm_plume_rad.hip; the handle and what the three share in ffm_plume.hpp.
#include "ffm_plume.hpp"

static int hydrostatic_init(ffm_plume *P)
{
    ffm_mesh *m = P->mesh; const int N = P->N, B = P->B;
    double *ph = P->ph_rgh, *rhof = P->wF[0], *sg = P->wF[1], *phig = P->wF[2], *rhob = P->wB[0], *fTop = P->wB[1], *div = P->wN[0];
    const double *gh = P->gh, *ghf = P->ghf, *magSf = ffm_mesh_geom(m, 1);
    double *p = P->p, *rho = P->rho; const double *psi = P->psi;
    // top fixedValue 0, everything else fixedFluxPressure with zero gradient
    const double *kind = P->kind_d;
    forN(P, B, [=] __device__(long k) { fTop[k] = (kind[k] > 1.5 && kind[k] < 2.5) ? 1.0 : 0.0; });
    forN(P, N, [=] __device__(long i) { p[i] = ph[i] + rho[i] * gh[i] + PREF; });
    FFM_TRY(thermo_correct(P)); mul(P, rho, psi, p, N);
    const long nNat = P->nNat;
    for (int corr = 0; corr < 5; corr++) {
        FFM_TRY(ffm_fvc_interpolate(m, nullptr, rho, rhof));
        zg(P, rhob, rho);
        FFM_TRY(ffm_fvc_snGrad(m, rho, sg));
        forN(P, nNat, [=] __device__(long e) { phig[e] = -rhof[e] * ghf[e] * sg[e] * magSf[e]; });
        FFM_TRY(ffm_fvm_transport(m, 0.0, nullptr, nullptr, nullptr, rhof, +1, P->diag, P->upper, P->lower));
        FFM_TRY(ffm_fvm_boundary_coeffs(m, nullptr, rhob, +1, fTop, P->zeroB, P->zeroB, P->ic[0], P->bc[0]));
        FFM_TRY(ffm_fvc_surface_integrate(m, phig, P->zeroB, div));
        {
            double *s0 = P->src[0]; const double *dv = div, *V = ffm_mesh_geom(m, 0);
            forN(P, N, [=] __device__(long i) { s0[i] = V[i] * dv[i]; });
        }
        FFM_TRY(ffm_fvm_add_boundary(m, P->ic[0], P->bc[0], P->diag, P->src[0], nullptr, P->dWork, P->sWork));
        FFM_TRY(solve_named(P, "ph_rgh", FFM_PCG, FFM_DIC, 1e-6, 0.01, P->dWork, P->upper, nullptr, ph, P->sWork));
        FFM_TRY(HX(P, ph));
        forN(P, N, [=] __device__(long i) { p[i] = ph[i] + rho[i] * gh[i] + PREF; });
        FFM_TRY(thermo_correct(P)); mul(P, rho, psi, p, N);
    }
    FFM_TRY(ffm_bc_values(m, fTop, P->zeroB, P->zeroB, ph, P->ph_rgh_b));
    dcopy(P, P->p_rgh, ph, N);
    return FFM_OK;
}

extern "C" int ffm_plume_create(ffm_ctx *ctx, int nx, int ny, int nz, double h, double dt, ffm_plume **out)
{
    const int lo[3] = {0, 0, 0}, hi[3] = {nx, ny, nz}, nbr[6] = {-1, -1, -1, -1, -1, -1};
    return ffm_plume_create_block(ctx, nx, ny, nz, lo, hi, nbr, h, dt, out);
}

// One rank's block [lo,hi) of the global (gx,gy,gz) box.  nbrRank[6] = rank across the -x,+x,-y,+y,-z,+z side of the
// block, or -1 where that side is a physical boundary of the box.  Ghost layers carry the neighbour ranks' cells.
extern "C" int ffm_plume_create_block(ffm_ctx *ctx, int gx, int gy, int gz, const int *lo, const int *hi, const int *nbrRank,
                                      double h, double dt, ffm_plume **out)
{
    if (!ctx || !out || !lo || !hi || !nbrRank) return FFM_ERR_ARG;
    const int nx = hi[0] - lo[0], ny = hi[1] - lo[1], nz = hi[2] - lo[2];
    if (nx < 2 || ny < 2 || nz < 2) { ffm_set_error("plume block must be at least 2 cells wide in every direction"); return FFM_ERR_ARG; }
    for (int d = 0; d < 3; d++) {
        const int G = d == 0 ? gx : d == 1 ? gy : gz;
        if ((lo[d] == 0) != (nbrRank[2 * d] < 0) || (hi[d] == G) != (nbrRank[2 * d + 1] < 0)) { ffm_set_error("plume block: neighbour ranks inconsistent with the block position"); return FFM_ERR_ARG; }
    }
    PL_HIP(hipSetDevice(ctx->device));
    FfmStageTimer tmAll_("plume_create: total");
    ffm_plume *P = new ffm_plume;
    P->ctx = ctx; P->nx = nx; P->ny = ny; P->nz = nz; P->h = h; P->dt = dt; P->rdt = 1.0 / dt;
    P->tight = getenv("FFM_PLUME_TIGHT") != nullptr;      // tests only: see ffm_plume_set_tight
    if (const char *e = getenv("FFM_PLUME_SOLVERS")) P->stecklerSolvers = e[0] == 's';     // "steckler": see ffm_plume_set_solvers
    const long nOwn = (long)nx * ny * nz;
    // ---- ghost layers, one per coupled side, in side order -x,+x,-y,+y,-z,+z; inside a layer in natural order
    const int cnt[6] = {ny * nz, ny * nz, nx * nz, nx * nz, nx * ny, nx * ny};
    int gOff[7]; gOff[0] = 0;
    for (int s6 = 0; s6 < 6; s6++) gOff[s6 + 1] = gOff[s6] + (nbrRank[s6] >= 0 ? cnt[s6] : 0);
    const long nGhost = gOff[6], N = nOwn + nGhost;
    P->N = (int)N; P->nOwn = (int)nOwn; P->oneBlock = nGhost == 0;
    auto cellOf = [&](int i, int j, int k) { return i + nx * (j + ny * k); };
    auto ghostOf = [&](int side, int i, int j, int k) -> int {     // ghost across `side` of owned cell (i,j,k)
        switch (side >> 1) {
        case 0: return (int)nOwn + gOff[side] + j + ny * k;
        case 1: return (int)nOwn + gOff[side] + i + nx * k;
        default: return (int)nOwn + gOff[side] + i + nx * j;
        }
    };
    FfmStageTimer *tmS_ = new FfmStageTimer("plume_create: natural LDU");
    // ---- LDU in local natural order + cut faces owned by the owned cell (ghost index > every owned index)
    std::vector<int> l, u; std::vector<signed char> fd, fsgn;
    l.reserve(3 * nOwn + nGhost); u.reserve(3 * nOwn + nGhost); fd.reserve(3 * nOwn + nGhost); fsgn.reserve(3 * nOwn + nGhost);
    for (int k = 0; k < nz; k++) for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) {
        const int c = cellOf(i, j, k);
        if (i < nx - 1) { l.push_back(c); u.push_back(c + 1); fd.push_back(0); fsgn.push_back(1); }
        if (j < ny - 1) { l.push_back(c); u.push_back(c + nx); fd.push_back(1); fsgn.push_back(1); }
        if (k < nz - 1) { l.push_back(c); u.push_back(c + nx * ny); fd.push_back(2); fsgn.push_back(1); }
        const int at[6] = {i == 0, i == nx - 1, j == 0, j == ny - 1, k == 0, k == nz - 1};
        for (int s6 = 0; s6 < 6; s6++) if (at[s6] && nbrRank[s6] >= 0) {    // ascending ghost index = ascending side
            l.push_back(c); u.push_back(ghostOf(s6, i, j, k)); fd.push_back((signed char)(s6 >> 1)); fsgn.push_back((s6 & 1) ? 1 : -1);
        }
    }
    const int F = (int)l.size(); P->F = F;
    delete tmS_; tmS_ = nullptr;
    // ---- renumber once to the library's cell order (no permutation pass ever after)
    // group hint for the tiled sweeps: 2-D tiles of x-columns, TILE_EDGE x TILE_EDGE cells in (y,z) (ignored by the level mode)
    std::vector<int> hint(nOwn);
    for (int k = 0; k < nz; k++) for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) hint[cellOf(i, j, k)] = ffm_tile_label(j / TILE_EDGE, k / TILE_EDGE);
    std::vector<int> c2(N), f2(F);
    { FfmStageTimer tm_("plume_create: renumber_hint"); FFM_TRY(ffm_renumber_hint((int)nOwn, (int)nGhost, F, l.data(), u.data(), hint.data(), c2.data(), f2.data())); }
    P->newToOld = c2; P->faceNewToOld = f2;
    tmS_ = new FfmStageTimer("plume_create: renumbered addressing");
    std::vector<int> oldToNew(N);
    for (long c = 0; c < N; c++) oldToNew[c2[c]] = (int)c;
    std::vector<int> l2(F), u2(F); std::vector<signed char> fd2(F), sg2(F);
    { const int *o2n = oldToNew.data(), *lp = l.data(), *up_ = u.data(), *f2p = f2.data(); const signed char *fdp = fd.data(), *sgp = fsgn.data();
      int *l2p = l2.data(), *u2p = u2.data(); signed char *fd2p = fd2.data(), *sg2p = sg2.data();
      ffm_parallel_for(F, [=](long a, long b) { for (long f = a; f < b; f++) { l2p[f] = o2n[lp[f2p[f]]]; u2p[f] = o2n[up_[f2p[f]]]; fd2p[f] = fdp[f2p[f]]; sg2p[f] = sgp[f2p[f]]; } }); }
    delete tmS_; tmS_ = nullptr;
    {
        std::vector<int> hintNew(nOwn);
        for (long c = 0; c < nOwn; c++) hintNew[c] = hint[c2[c]];
        FfmStageTimer tm_("plume_create: ldu_create");
        FFM_TRY(ffm_ldu_create_hint(ctx, (int)nOwn, (int)nGhost, F, l2.data(), u2.data(), hintNew.data(), &P->A));
    }
    if (!P->A->identity) { ffm_set_error("plume: renumbered mesh is not native"); return FFM_ERR_ADDR; }
    if (nGhost == 0) { P->hL2 = l2; P->hU2 = u2; P->hOldToNew = oldToNew; }      // for the direction-ordered ray solves (a decomposed block rebuilds them if the staged sweep is asked for: plume_host_addressing)
    for (int q = 0; q < 6; q++) P->nbrRank[q] = nbrRank[q];
    for (int q = 0; q < 7; q++) P->gOff[q] = gOff[q];
    FFM_TRY(ffm_ldu_set_global_cells(P->A, (long)gx * gy * gz));
    P->nNat = P->A->upTotal;
    tmS_ = new FfmStageTimer("plume_create: geometry + patches");
    // ---- geometry (global coordinates)
    ffm_hvec<double> V = ffm_hvec_fill<double>(N, h * h * h), C(3 * N), Sf = ffm_hvec_fill<double>(3 * (size_t)F, 0.0), magSf = ffm_hvec_fill<double>(F, h * h),
                     wgt = ffm_hvec_fill<double>(F, 0.5), del = ffm_hvec_fill<double>(F, 1.0 / h), Cfy(F);      // C, Cfy: every entry written below
    {
        double *Cp = C.data(), *Sfp = Sf.data(), *Cfyp = Cfy.data(); const int *c2p = c2.data(), *l2p = l2.data(); const signed char *fd2p = fd2.data(), *sg2p = sg2.data();
        const int lo0 = lo[0], lo1 = lo[1], lo2 = lo[2]; int gO[7]; for (int q = 0; q < 7; q++) gO[q] = gOff[q];
        ffm_parallel_for(N, [=](long a, long b) { for (long cn = a; cn < b; cn++) {
            const int co = c2p[cn];
            int i, j, k;
            if (co < nOwn) { i = co % nx; j = (co / nx) % ny; k = co / (nx * ny); }
            else {
                int side = 0; while (co - nOwn >= gO[side + 1]) side++;
                const int r = co - (int)nOwn - gO[side];
                switch (side >> 1) {
                case 0: j = r % ny; k = r / ny; i = (side & 1) ? nx : -1; break;
                case 1: i = r % nx; k = r / nx; j = (side & 1) ? ny : -1; break;
                default: i = r % nx; j = r / nx; k = (side & 1) ? nz : -1; break;
                }
            }
            Cp[cn] = (lo0 + i + 0.5) * h; Cp[N + cn] = (lo1 + j + 0.5) * h; Cp[2 * N + cn] = (lo2 + k + 0.5) * h;
        } });
        ffm_parallel_for(F, [=](long a, long b) { for (long f = a; f < b; f++) { Sfp[(size_t)fd2p[f] * F + f] = sg2p[f] * h * h; Cfyp[f] = Cp[N + l2p[f]] + (fd2p[f] == 1 ? sg2p[f] * 0.5 * h : 0.0); } });
    }
    // ---- ghost exchange plan: side s sends the owned layer adjacent to it, receives the ghost layer across it
    {
        std::vector<int> ranks, sc, rc, cells;
        for (int s6 = 0; s6 < 6; s6++) if (nbrRank[s6] >= 0) {
            ranks.push_back(nbrRank[s6]); sc.push_back(cnt[s6]); rc.push_back(cnt[s6]);
            const int d = s6 >> 1, pos = (s6 & 1) ? (d == 0 ? nx : d == 1 ? ny : nz) - 1 : 0;
            if (d == 0) for (int k = 0; k < nz; k++) for (int j = 0; j < ny; j++) cells.push_back(oldToNew[cellOf(pos, j, k)]);
            else if (d == 1) for (int k = 0; k < nz; k++) for (int i = 0; i < nx; i++) cells.push_back(oldToNew[cellOf(i, pos, k)]);
            else for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) cells.push_back(oldToNew[cellOf(i, j, pos)]);
        }
        if (!ranks.empty()) FFM_TRY(ffm_ldu_set_ghost_exchange(P->A, (int)ranks.size(), ranks.data(), sc.data(), cells.data(), rc.data()));
    }
    // ---- patches on the physical sides of the block: inlet, floor, top, sides(xmin,xmax,zmin,zmax)
    const double Lx = gx * h, Lz = gz * h, hwx = std::min(0.5, Lx / 4), hwz = std::min(0.5, Lz / 4);
    std::vector<int> pc[4]; std::vector<double> pS[4][3];
    auto addFace = [&](int patch, int cOld, double sx, double sy, double sz) {
        pc[patch].push_back(oldToNew[cOld]); pS[patch][0].push_back(sx); pS[patch][1].push_back(sy); pS[patch][2].push_back(sz);
    };
    if (nbrRank[2] < 0) for (int k = 0; k < nz; k++) for (int i = 0; i < nx; i++) {          // ymin in natural cell order
        const bool in = std::fabs((lo[0] + i + 0.5) * h - Lx / 2) < hwx && std::fabs((lo[2] + k + 0.5) * h - Lz / 2) < hwz;
        addFace(in ? P_INLET : P_FLOOR, cellOf(i, 0, k), 0, -h * h, 0);
    }
    if (nbrRank[3] < 0) for (int k = 0; k < nz; k++) for (int i = 0; i < nx; i++) addFace(P_TOP, cellOf(i, ny - 1, k), 0, h * h, 0);
    if (nbrRank[0] < 0) for (int k = 0; k < nz; k++) for (int j = 0; j < ny; j++) addFace(P_SIDES, cellOf(0, j, k), -h * h, 0, 0);
    if (nbrRank[1] < 0) for (int k = 0; k < nz; k++) for (int j = 0; j < ny; j++) addFace(P_SIDES, cellOf(nx - 1, j, k), h * h, 0, 0);
    if (nbrRank[4] < 0) for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) addFace(P_SIDES, cellOf(i, j, 0), 0, 0, -h * h);
    if (nbrRank[5] < 0) for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) addFace(P_SIDES, cellOf(i, j, nz - 1), 0, 0, h * h);
    int sizes[4]; const int *fcs[4]; const double *pSf[4]; const double *pDel[4];
    std::vector<double> pSflat[4], pD[4];
    int Btot = 0;
    for (int p = 0; p < 4; p++) {
        sizes[p] = (int)pc[p].size(); fcs[p] = pc[p].data(); Btot += sizes[p];
        for (int d = 0; d < 3; d++) pSflat[p].insert(pSflat[p].end(), pS[p][d].begin(), pS[p][d].end());
        pD[p].assign(sizes[p], 2.0 / h); pSf[p] = pSflat[p].data(); pDel[p] = pD[p].data();
    }
    P->B = Btot;
    delete tmS_; tmS_ = nullptr;
    { FfmStageTimer tm_("plume_create: mesh_create"); FFM_TRY(ffm_mesh_create(P->A, V.data(), C.data(), Sf.data(), magSf.data(), wgt.data(), del.data(), 4, sizes, fcs, pSf, pDel, &P->mesh)); }
    tmS_ = new FfmStageTimer("plume_create: face centres");
    {
        // face centres (LUST correction): owner's centre + half a cell towards the neighbour
        ffm_hvec<double> Cf(3 * (size_t)F);                // every entry written below
        { double *Cfp = Cf.data(); const double *Cp = C.data(); const int *l2p = l2.data(); const signed char *fd2p = fd2.data(), *sg2p = sg2.data();
          ffm_parallel_for(F, [=](long a, long b) { for (long f = a; f < b; f++) for (int d = 0; d < 3; d++) Cfp[(size_t)d * F + f] = Cp[(size_t)d * N + l2p[f]] + (fd2p[f] == d ? sg2p[f] * 0.5 * h : 0.0); }); }
        FFM_TRY(ffm_mesh_set_face_centres(P->mesh, Cf.data()));
    }
    delete tmS_; tmS_ = new FfmStageTimer("plume_create: fields + tables");
    const int ny_glob = gy;
    const int B = Btot; const long nNat = P->nNat;
    // ---- fields
    auto NN = [&]() { return dalloc(P, N); };
    for (int i = 0; i < NSP; i++) { P->Y[i] = dfill(P, N, Y_AMB[i]); P->Y0[i] = i == INERT ? nullptr : NN(); }      // nothing reads the inert specie's old time
    P->T = dfill(P, N, TREF); P->hs = NN(); P->hs0 = NN();
    for (int c = 0; c < 3; c++) { P->U[c] = NN(); P->U0[c] = NN(); }
    P->p = dfill(P, N, PREF); P->p0 = NN(); P->p_rgh = NN(); P->p_rgh0 = NN(); P->psi = NN(); P->psi0 = NN();
    P->rho = NN(); P->rho0 = NN(); P->K = NN(); P->K0 = NN(); P->dpdt = NN(); P->ph_rgh = NN();
    P->phi = dalloc(P, nNat); P->phib = dalloc(P, B); P->ph_rgh_b = dalloc(P, B);
    {
        const double ghRef = -9.81 * (ny_glob * h);
        std::vector<double> gh(N), ghf(std::max<long>(nNat, 1), 0.0);
        for (long c = 0; c < N; c++) gh[c] = -9.81 * C[N + c] - ghRef;
        for (int f = 0; f < F; f++) ghf[P->A->h_callerToNative[f]] = -9.81 * Cfy[f] - ghRef;
        P->gh = dupload(P, gh); P->ghf = dupload(P, ghf);
    }
    // ---- boundary-condition templates
    std::vector<double> kind(B), fsU[3], rU[3], fsS(B), fsH(B), rY[NSP], rH(B);
    for (int c = 0; c < 3; c++) { fsU[c].assign(B, 0.0); rU[c].assign(B, 0.0); }
    for (int i = 0; i < NSP; i++) rY[i].assign(B, 0.0);
    int k0 = 0;
    for (int p = 0; p < 4; p++) for (int q = 0; q < sizes[p]; q++, k0++) {
        kind[k0] = p;
        for (int c = 0; c < 3; c++) {
            if (p == P_INLET) { fsU[c][k0] = 1.0; rU[c][k0] = (c == 1) ? U_IN : 0.0; }
            else if (p == P_FLOOR) fsU[c][k0] = 1.0;
            else fsU[c][k0] = (pS[p][c][q] != 0.0) ? 0.0 : -1.0;      // normal: zeroGradient; tangential: inletOutlet(0)
        }
        fsH[k0] = (p == P_INLET || p == P_FLOOR) ? 1.0 : -1.0;
        if (p == P_INLET) { fsS[k0] = 1.0; rH[k0] = CP * (T_IN - TREF); for (int i = 0; i < NSP; i++) rY[i][k0] = Y_IN[i]; }
        else if (p == P_FLOOR) { fsS[k0] = 0.0; }                     // species zeroGradient; h handled below
        else { fsS[k0] = -1.0; rH[k0] = 0.0; for (int i = 0; i < NSP; i++) rY[i][k0] = Y_AMB[i]; }
    }
    P->kind_d = dupload(P, kind);
    for (int c = 0; c < 3; c++) { P->fStaticU[c] = dupload(P, fsU[c]); P->refU[c] = dupload(P, rU[c]); P->fU[c] = dalloc(P, B); }
    P->fStaticS = dupload(P, fsS); P->fS = dalloc(P, B); P->refH = dupload(P, rH);
    P->fStaticH = dupload(P, fsH); P->fH = dalloc(P, B);
    for (int i = 0; i < NSP; i++) P->refY[i] = dupload(P, rY[i]);
    P->fP = dalloc(P, B); P->refP = dalloc(P, B); P->gradP = dalloc(P, B); P->zeroB = dalloc(P, B);
    P->oneB = dupload(P, std::vector<double>(std::max(B, 1), 1.0));
    // ---- matrix + work
    P->diag = NN(); P->upper = dalloc(P, nNat); P->lower = dalloc(P, nNat); P->dWork = NN(); P->sWork = NN();
    P->Udiag = NN(); P->Uupper = dalloc(P, nNat); P->Ulower = dalloc(P, nNat);
    for (int c = 0; c < 3; c++) { P->src[c] = NN(); P->ic[c] = dalloc(P, B); P->bc[c] = dalloc(P, B); P->Usrc[c] = NN(); P->Uic[c] = dalloc(P, B); P->Ubc[c] = dalloc(P, B); }
    for (auto &w : P->wN) w = NN();
    for (auto &w : P->wF) w = dalloc(P, nNat);
    P->ddtCorrF = dalloc(P, nNat);
    for (auto &w : P->wB) w = dalloc(P, B);
    for (int c = 0; c < 3; c++) { P->UdW[c] = NN(); P->UsW[c] = NN(); P->Ub[c] = P->wB[1 + c]; }
    P->wFuel = P->wN[8]; P->Qdot = P->wN[9]; P->Yt = P->wN[10]; P->alphaEff_f = P->wF[0]; P->alphaEff_b = P->wB[4];      // (the slot table: ffm_plume.hpp)
    const bool fused = P->fused = getenv("FFM_PLUME_UNFUSED") == nullptr;
    P->mvSelection = getenv("FFM_PLUME_INDEPENDENT_LIMITERS") == nullptr;
    { const char *e = getenv("FFM_PLUME_SEPARATE_H"); P->separateH = e && atoi(e) != 0; }
    if (P->mvSelection) { P->wMv = dalloc(P, nNat); if (fused) for (int j = 0; j < 2; j++) for (int d = 0; d < 3; d++) P->mvG[j][d] = NN(); }
    if (P->mvSelection && fused && P->oneBlock) { P->phiKf = dalloc(P, nNat); P->KbM = dalloc(P, B); }
    for (int j = 0; j < 4; j++) {
        for (int d = 0; d < 3; d++) P->gM[j][d] = fused ? NN() : nullptr;
        P->spD[j] = fused ? NN() : nullptr; P->spS[j] = fused ? NN() : nullptr; P->suM[j] = fused ? NN() : nullptr;
        const bool ownOffDiag = fused && (j == 0 || !P->mvSelection);       // common limiter: the species share one pair of off-diagonal arrays
        P->spU[j] = ownOffDiag ? dalloc(P, nNat) : nullptr; P->spL[j] = ownOffDiag ? dalloc(P, nNat) : nullptr; P->spB[j] = (fused || P->mvSelection) ? dalloc(P, B) : nullptr;
    }
    for (double *p : P->pool) if (!p) { ffm_set_error("plume: out of device memory"); return FFM_ERR_HIP; }
    PL_HIP(hipDeviceSynchronize());
    delete tmS_; tmS_ = new FfmStageTimer("plume_create: hydrostatic init");
    // ---- initial state: quiescent ambient, then hydrostatic initialisation
    standin_thermo(P);
    mul(P, P->rho, P->psi, P->p, N);
    FFM_TRY(hydrostatic_init(P));
    PL_HIP(hipStreamSynchronize(ctx->stream));
    delete tmS_; tmS_ = nullptr;
    if (const char *e = getenv("FFM_PLUME_RADIATION")) { if (atoi(e) > 0) FFM_TRY(ffm_plume_set_radiation(P, atoi(e), 2, 4, nullptr, nullptr)); }   // solverFreq
    if (const char *e = getenv("FFM_PLUME_RADIATION_ORDERING")) FFM_TRY(ffm_plume_set_radiation_ordering(P, atoi(e)));           // 1: staged ray sweep
    *out = P;
    return FFM_OK;
}

extern "C" int ffm_plume_destroy(ffm_plume *P)
{
    if (!P) return FFM_OK;
    hipStreamSynchronize(P->ctx->stream);
    for (double *p : P->pool) hipFree(p);
    for (int a = 0; a < 3; a++) { hipFree(P->radCm[a]); hipFree(P->radFm[a]); }
    hipFree(P->radHaloCells);
    hipFree(P->thermoFail); if (P->thermoFailH) hipHostFree(P->thermoFailH);
    hipFree(P->gmFlag); if (P->gmFlagH) hipHostFree(P->gmFlagH);
    ffm_mesh_destroy(P->mesh); ffm_ldu_destroy(P->A);
    delete P;
    return FFM_OK;
}

// h's patch reference values: the inlet's enthalpy, hAmb on the inletOutlet patches, 0 on the floor.  Stand-in thermo: CP (T_IN - TREF);
// janaf: Hs(inlet mixture, T_IN) from the inlet faces' species values (ffm_thermo_he_d over all patch faces: the others' are not kept)
static int plume_inlet_enthalpy(ffm_plume *P)
{
    const int B = P->B; const double *kind = P->kind_d; double *rH = P->refH; const double hAmb = P->hAmb;
    if (!P->thermo) { forN(P, B, [=] __device__(long k) { rH[k] = kind[k] < 0.5 ? CP * (T_IN - TREF) : kind[k] > 1.5 ? hAmb : 0.0; }); return FFM_OK; }
    double *Tin = P->wB[0], *hin = P->wB[2];
    forN(P, B, [=] __device__(long k) { Tin[k] = T_IN; });
    FFM_TRY(ffm_thermo_he_d(P->thermo, B, P->refY, Tin, hin));
    forN(P, B, [=] __device__(long k) { rH[k] = kind[k] < 0.5 ? hin[k] : kind[k] > 1.5 ? hAmb : 0.0; });
    return FFM_OK;
}
// The start-up from the Y and h the handle holds: p = pRef, ph_rgh = 0, thermo.correct() (janaf: from T = TREF, the Newton start),
// rho = psi p, the hydrostatic initialisation; reNut: correctNut() of the kEqn model again, with the new rho
static int plume_startup(ffm_plume *P, bool reNut)
{
    const int N = P->N;
    double *p = P->p, *ph = P->ph_rgh, *T = P->T;
    forN(P, N, [=] __device__(long c) { p[c] = PREF; ph[c] = 0.0; });
    if (P->thermo) forN(P, N, [=] __device__(long c) { T[c] = TREF; });
    P->log.clear();
    FFM_TRY(thermo_correct(P));
    mul(P, P->rho, P->psi, P->p, N);
    FFM_TRY(hydrostatic_init(P));
    if (reNut && P->turbModel) FFM_TRY(plume_turbulence_init(P));
    thermo_flag_fetch(P);
    PL_HIP(hipStreamSynchronize(P->ctx->stream));
    return thermo_flag_check(P);
}

extern "C" int ffm_plume_set_tight(ffm_plume *P, int on) { if (!P) return FFM_ERR_ARG; P->tight = on != 0; return FFM_OK; }
// Start state and boundary values other than the quiescent ambient / pure-fuel inflow (tests: a state in which no transported
// field is uniform, tests/test_plume_gpu.py).  Y[5], h: cell fields in natural blockMesh order of the (single) block; Yamb / Yin:
// the inletOutlet and inlet values of the species, hAmb the inletOutlet value of h.  The hydrostatic initialisation
// (solver/phrghEqn.H) is redone from the new state; after steps have been taken the case starts again from it (time 0).
extern "C" int ffm_plume_set_initial_state(ffm_plume *P, const double *const *Y, const double *h, const double *Yamb, const double *Yin, double hAmb)
{
    if (!P || !Y || !h || !Yamb || !Yin) return FFM_ERR_ARG;
    if (!P->oneBlock) { ffm_set_error("plume: the start state can be set on a single block only"); return FFM_ERR_ARG; }
    PL_HIP(hipSetDevice(P->ctx->device));
    const int N = P->N, B = P->B;
    if (P->stepNo != 0) {       // restart: what the steps have changed and the start state does not set goes back to its value at creation
        PL_HIP(hipStreamSynchronize(P->ctx->stream));
        for (int c = 0; c < 3; c++) FFM_TRY(ffm_dzero(P->ctx, P->U[c], sizeof(double) * N));
        FFM_TRY(ffm_dzero(P->ctx, P->K, sizeof(double) * N)); FFM_TRY(ffm_dzero(P->ctx, P->dpdt, sizeof(double) * N));
        FFM_TRY(ffm_dzero(P->ctx, P->phi, sizeof(double) * std::max<long>(P->nNat, 1))); FFM_TRY(ffm_dzero(P->ctx, P->phib, sizeof(double) * std::max(B, 1)));
        P->stepNo = 0; P->time = 0.0; P->radHaveG = false; P->mvOverride = false; P->ddtCorrValid = false;
        if (P->p1G) { FFM_TRY(ffm_dzero(P->ctx, P->p1G, sizeof(double) * N)); P->p1HaveQr = false; }      // P1 starts again from G = 0
    }
    std::vector<double> v(N);
    auto up = [&](double *dst, const double *nat) -> int {
        for (int c = 0; c < N; c++) v[c] = nat[P->newToOld[c]];
        return ffm_memcpy_h2d(P->ctx, dst, v.data(), sizeof(double) * N);
    };
    for (int i = 0; i < NSP; i++) FFM_TRY(up(P->Y[i], Y[i]));
    FFM_TRY(up(P->hs, h));
    P->hAmb = hAmb;
    const double *kind = P->kind_d;
    for (int i = 0; i < NSP; i++) {
        double *r = P->refY[i]; const double a = Yamb[i], b = Yin[i];
        forN(P, B, [=] __device__(long k) { r[k] = kind[k] < 0.5 ? b : kind[k] > 1.5 ? a : 0.0; });
    }
    FFM_TRY(plume_inlet_enthalpy(P));
    return plume_startup(P, P->thermo != nullptr);
}

// Tests (the deciding test of the multi-step parity question): the NEXT ffm_plume_step convects the species and h with these face
// weights instead of evaluating the multivariateSelection limiter; w[F] in natural blockMesh face order of the (single) block.
extern "C" int ffm_plume_override_mv_weights(ffm_plume *P, const double *w)
{
    if (!P || !w) return FFM_ERR_ARG;
    if (!P->mvSelection || !P->oneBlock) { ffm_set_error("plume: weights can be handed in on a single block with the common limiter only"); return FFM_ERR_ARG; }
    PL_HIP(hipSetDevice(P->ctx->device));
    std::vector<double> v(std::max<long>(P->nNat, 1), 0.0);
    const std::vector<int> &c2n = P->A->h_callerToNative;
    for (int f = 0; f < P->F; f++) v[c2n[f]] = w[P->faceNewToOld[f]];
    FFM_TRY(ffm_memcpy_h2d(P->ctx, P->wMv, v.data(), sizeof(double) * P->nNat));
    P->mvOverride = true;
    return FFM_OK;
}
extern "C" int ffm_plume_set_solvers(ffm_plume *P, int stecklerSelection) { if (!P) return FFM_ERR_ARG; P->stecklerSolvers = stecklerSelection != 0; return FFM_OK; }

// give a buffer of the handle back (ffm_plume_set_turbulence 0); the caller has synchronised the stream
static void dfree(ffm_plume *P, double *&p)
{
    if (!p) return;
    P->pool.erase(std::remove(P->pool.begin(), P->pool.end(), p), P->pool.end());
    hipFree(p); p = nullptr;
}
// the sub-grid model of the step: see include/ffm.h
extern "C" int ffm_plume_set_turbulence(ffm_plume *P, int model, double Ck, double Ce, double Prt, double kInlet, const double *k0)
{
    if (!P) return FFM_ERR_ARG;
    if (model != 0 && model != 1) { ffm_set_error("ffm_plume_set_turbulence: unknown model %d (0 none, 1 kEqn)", model); return FFM_ERR_ARG; }
    const int N = P->N, nOwn = P->nOwn, B = P->B;
    if (model == 1) {
        if (!(Ck >= 0) || !(Ce >= 0) || !(Prt > 0) || !(kInlet > 0) || !std::isfinite(Ck) || !std::isfinite(Ce) || !std::isfinite(Prt) || !std::isfinite(kInlet)) {
            ffm_set_error("ffm_plume_set_turbulence: Ck >= 0, Ce >= 0, Prt > 0, kInlet > 0 wanted"); return FFM_ERR_ARG;
        }
        if (k0) for (int c = 0; c < nOwn; c++) if (!(k0[c] > 0) || !std::isfinite(k0[c])) {
            ffm_set_error("ffm_plume_set_turbulence: k0[%d] is not finite and positive", c); return FFM_ERR_ARG;
        }
    }
    if (model == 0 && P->combModel == 1) {
        ffm_set_error("ffm_plume_set_turbulence: the EDC of ffm_plume_set_combustion reads the kEqn model's Ce and delta; switch it off first");
        return FFM_ERR_UNSUPPORTED;
    }
    PL_HIP(hipSetDevice(P->ctx->device));
    PL_HIP(hipStreamSynchronize(P->ctx->stream));
    if (model == 0) {
        P->turbModel = 0;
        dfree(P, P->kSgs); dfree(P, P->nut); dfree(P, P->alphat); dfree(P, P->lesDelta);
        dfree(P, P->kb); dfree(P, P->nutb); dfree(P, P->alphatb); dfree(P, P->refK);
        for (auto &gc : P->lesG) for (double *&g : gc) dfree(P, g);
        return FFM_OK;
    }
    if (!P->kSgs) {
        const size_t nPool = P->pool.size();
        P->kSgs = dalloc(P, N); P->nut = dalloc(P, N); P->alphat = dalloc(P, N); P->lesDelta = dalloc(P, N);
        P->kb = dalloc(P, B); P->nutb = dalloc(P, B); P->alphatb = dalloc(P, B); P->refK = dalloc(P, B);
        if (!P->fused) for (auto &gc : P->lesG) for (double *&g : gc) g = dalloc(P, N);
        if (P->pool.size() != nPool + (P->fused ? 8 : 17)) { ffm_set_error("plume: out of device memory"); return FFM_ERR_HIP; }
        // delta cubeRootVol, on the host as the oracle forms it
        std::vector<double> v(N);
        FFM_TRY(ffm_d2h(P->ctx, v.data(), ffm_mesh_geom(P->mesh, 0), sizeof(double) * N));
        for (int c = 0; c < N; c++) v[c] = std::cbrt(v[c]);
        FFM_TRY(ffm_memcpy_h2d(P->ctx, P->lesDelta, v.data(), sizeof(double) * N));
    }
    P->Ck = Ck; P->Ce = Ce; P->Prt = Prt; P->kInlet = kInlet;
    {
        std::vector<double> v(N, kInlet);
        if (k0) for (int c = 0; c < nOwn; c++) v[c] = k0[P->newToOld[c]];
        FFM_TRY(ffm_memcpy_h2d(P->ctx, P->kSgs, v.data(), sizeof(double) * N));
        if (k0) FFM_TRY(HX(P, P->kSgs));
    }
    const double *kind = P->kind_d; double *rK = P->refK;
    forN(P, B, [=] __device__(long q) { rK[q] = (kind[q] < 0.5 || kind[q] > 1.5) ? kInlet : 0.0; });
    P->turbModel = 1;
    FFM_TRY(plume_turbulence_init(P));
    PL_HIP(hipStreamSynchronize(P->ctx->stream));
    return FFM_OK;
}
// buffers that live while a model wants them.  alphaStd: the alpha EDC reads with the stand-in thermo, a cell field of mu/Pr.  wFuel and
// Qdot: with either model on they get arrays of their own and stay readable after the step ("wFuel", "Qdot"); otherwise they are the
// scratch slots they always were, which later stages of the step reuse
static int plume_model_buffers(ffm_plume *P)
{
    const bool wantA = P->combModel == 1 && !P->thermo, wantS = P->combModel == 1 || P->thermo;
    if ((!wantA && P->alphaStd) || (!wantS && P->wFuelOwn)) PL_HIP(hipStreamSynchronize(P->ctx->stream));
    if (wantA && !P->alphaStd) P->alphaStd = dfill(P, P->N, MU / PR);
    if (!wantA) dfree(P, P->alphaStd);
    if (wantS && !P->wFuelOwn) { P->wFuelOwn = dalloc(P, P->N); P->QdotOwn = dalloc(P, P->N); }
    if (!wantS) { dfree(P, P->wFuelOwn); dfree(P, P->QdotOwn); }
    if ((wantA && !P->alphaStd) || (wantS && (!P->wFuelOwn || !P->QdotOwn))) { ffm_set_error("plume: out of device memory"); return FFM_ERR_HIP; }
    P->wFuel = wantS ? P->wFuelOwn : P->wN[8]; P->Qdot = wantS ? P->QdotOwn : P->wN[9];
    return FFM_OK;
}
// the thermo model of the step: see include/ffm.h
extern "C" int ffm_plume_set_thermo(ffm_plume *P, ffm_thermo *thermo)
{
    if (!P) return FFM_ERR_ARG;
    if (P->stepNo != 0) { ffm_set_error("ffm_plume_set_thermo: steps have been taken; restart with ffm_plume_set_initial_state first"); return FFM_ERR_ARG; }
    if (thermo) {
        int n = 0; double W[8];
        FFM_TRY(ffm_thermo_species(thermo, &n, nullptr));
        if (n != NSP) { ffm_set_error("ffm_plume_set_thermo: the table holds %d species, the plume %d", n, NSP); return FFM_ERR_ARG; }
        FFM_TRY(ffm_thermo_species(thermo, &n, W));
        for (int i = 0; i < NSP; i++) if (!(std::fabs(W[i] - WMOL[i]) <= 1e-3 * WMOL[i])) {
            ffm_set_error("ffm_plume_set_thermo: species %d has molecular weight %g, the plume's %s %g", i, W[i], SPN[i], WMOL[i]); return FFM_ERR_ARG;
        }
        if (!P->radThermo && (P->radFreq > 0 || P->radCoupled || P->radOrdering != 0)) {
            ffm_set_error("ffm_plume_set_thermo: not with ffm_plume_set_radiation* on (ffm_plume_set_radiation_thermo is off)"); return FFM_ERR_UNSUPPORTED;
        }
    }
    PL_HIP(hipSetDevice(P->ctx->device));
    PL_HIP(hipStreamSynchronize(P->ctx->stream));
    if (thermo && !P->mu) {
        const size_t nPool = P->pool.size();
        P->mu = dalloc(P, P->N); P->alpha = dalloc(P, P->N); P->Cp = dalloc(P, P->N);
        if (P->pool.size() != nPool + 3) { ffm_set_error("plume: out of device memory"); return FFM_ERR_HIP; }
        PL_HIP(hipMalloc((void **)&P->thermoFail, sizeof(int)));
        PL_HIP(hipMemsetAsync(P->thermoFail, 0, sizeof(int), P->ctx->stream));
        PL_HIP(hipHostMalloc((void **)&P->thermoFailH, sizeof(int), hipHostMallocDefault));
        *P->thermoFailH = 0;
    }
    if (!thermo && P->mu) {
        dfree(P, P->mu); dfree(P, P->alpha); dfree(P, P->Cp);
        hipFree(P->thermoFail); P->thermoFail = nullptr; hipHostFree(P->thermoFailH); P->thermoFailH = nullptr;
    }
    P->thermo = thermo;
    FFM_TRY(plume_model_buffers(P));
    FFM_TRY(plume_inlet_enthalpy(P));
    return plume_startup(P, true);
}
// the rays and radiation->Sh together with the thermo package: see include/ffm.h
extern "C" int ffm_plume_set_radiation_thermo(ffm_plume *P, int on)
{
    if (!P) return FFM_ERR_ARG;
    if (!on && P->thermo && (P->radFreq > 0 || P->radCoupled || P->radOrdering != 0)) {
        ffm_set_error("ffm_plume_set_radiation_thermo: the thermo package and ffm_plume_set_radiation* are both on; unset one of them first");
        return FFM_ERR_UNSUPPORTED;
    }
    P->radThermo = on != 0;
    return FFM_OK;
}
// the combustion model of the step: see include/ffm.h
extern "C" int ffm_plume_set_combustion(ffm_plume *P, int model, double C_EDC, double C_Diff, double C_Stiff, double s, double qFuel)
{
    if (!P) return FFM_ERR_ARG;
    if (model != 0 && model != 1) { ffm_set_error("ffm_plume_set_combustion: unknown model %d (0 stand-in, 1 EDC)", model); return FFM_ERR_ARG; }
    if (model == 1) {
        if (!std::isfinite(C_EDC) || !std::isfinite(C_Diff) || !std::isfinite(C_Stiff) || !std::isfinite(s) || !std::isfinite(qFuel) ||
            !(s > 0) || !(C_Stiff > 0) || !(C_EDC >= 0) || !(C_Diff >= 0) || !(qFuel > 0)) {
            ffm_set_error("ffm_plume_set_combustion: finite C_EDC >= 0, C_Diff >= 0, C_Stiff > 0, s > 0, qFuel > 0 wanted"); return FFM_ERR_ARG;
        }
        if (!P->turbModel) {
            ffm_set_error("ffm_plume_set_combustion: the EDC reads the kEqn model's Ce and delta; ffm_plume_set_turbulence first"); return FFM_ERR_UNSUPPORTED;
        }
    }
    PL_HIP(hipSetDevice(P->ctx->device));
    P->combModel = model;
    if (model == 1) { P->C_EDC = C_EDC; P->C_Diff = C_Diff; P->C_Stiff = C_Stiff; P->edcS = s; P->qFuel = qFuel; }
    return plume_model_buffers(P);
}
extern "C" int ffm_plume_ncells(const ffm_plume *P) { return P ? P->nOwn : FFM_ERR_ARG; }
extern "C" int ffm_plume_nfaces(const ffm_plume *P) { return P ? P->F : FFM_ERR_ARG; }

// copy a cell field to the host in NATURAL blockMesh cell order; name in rho,p,p_rgh,T,h,K,Ux,Uy,Uz,psi,<specie>,
// and k,nut,alphat with the kEqn model on
extern "C" int ffm_plume_get_field(ffm_plume *P, const char *name, double *out)
{
    if (!P || !name || !out) return FFM_ERR_ARG;
    const std::string n(name);
    const double *src = nullptr;
    if (n == "qr") {        // P1's wall flux: [nBoundary] in patch-face order, an error before the first correct()
        if (!(P->p1Freq > 0 && P->p1HaveQr)) { ffm_set_error("unknown field %s", name); return FFM_ERR_ARG; }
        PL_HIP(hipStreamSynchronize(P->ctx->stream));
        return ffm_d2h(P->ctx, out, P->p1Qr, sizeof(double) * P->B);
    }
    if (n == "rho") src = P->rho; else if (n == "p") src = P->p; else if (n == "p_rgh") src = P->p_rgh; else if (n == "T") src = P->T;
    else if (n == "h") src = P->hs; else if (n == "K") src = P->K; else if (n == "Ux") src = P->U[0]; else if (n == "Uy") src = P->U[1];
    else if (n == "Uz") src = P->U[2]; else if (n == "psi") src = P->psi; else if (n == "ph_rgh") src = P->ph_rgh;
    else if (n == "mu") src = P->mu; else if (n == "alpha") src = P->alpha; else if (n == "Cp") src = P->Cp;      // (null while the stand-in thermo is on)
    else if (n == "wFuel") src = P->wFuelOwn; else if (n == "Qdot") src = P->QdotOwn;      // (null while both are scratch slots: no model of theirs on)
    else if (n == "k") src = P->kSgs; else if (n == "nut") src = P->nut; else if (n == "alphat") src = P->alphat;      // (null while the model is off)
    else if (n == "G") src = P->radG(); else if (n == "ShSu") src = P->radHaveSh ? P->radShSu : nullptr; else if (n == "ShSp") src = P->radHaveSh ? P->radShSp : nullptr; else if (n == "radE") src = P->radE; else if (n == "aRad") src = (P->gm && P->gmHaveA) ? P->aRad : nullptr;      // (ShSu, ShSp: null before the first radiation->Sh pass)
    else if (n.size() > 1 && n[0] == 'I' && isdigit((unsigned char)n[1])) { const int i = atoi(n.c_str() + 1); if (i < (int)P->I.size()) src = P->I[i]; }
    else for (int i = 0; i < NSP; i++) if (n == SPN[i]) src = P->Y[i];
    if (!src) { ffm_set_error("unknown field %s", name); return FFM_ERR_ARG; }
    std::vector<double> v(P->N);
    PL_HIP(hipStreamSynchronize(P->ctx->stream));
    FFM_TRY(ffm_d2h(P->ctx, v.data(), src, sizeof(double) * P->N));
    for (int c = 0; c < P->nOwn; c++) out[P->newToOld[c]] = v[c];      // owned cells, local natural (blockMesh) order
    return FFM_OK;
}

// Raw state of the case for a driver that runs the SAME case through another path (bench.py: the reference's equation files over the
// Foam layer, libffm_refsnippets.so): cell fields [N] in the library's cell order, face fields [F] in the renumbered LDU face order
// (what ffm_faces_to_native takes), boundary arrays [B] in (patch, face) order -- inlet, floor, top, sides.  Returns the count.
extern "C" long ffm_plume_get_raw(ffm_plume *P, const char *name, double *out, long cap)
{
    if (!P || !name || !out) return FFM_ERR_ARG;
    if (!P->oneBlock) { ffm_set_error("ffm_plume_get_raw: single block only"); return FFM_ERR_ARG; }
    const std::string n(name);
    const long N = P->N, F = P->F, B = P->B;
    auto cellF = [&](const double *src) -> long { if (cap < N) return FFM_ERR_ARG; return ffm_d2h(P->ctx, out, src, sizeof(double) * N) == FFM_OK ? N : FFM_ERR_HIP; };
    auto bndF = [&](const double *src) -> long { if (cap < B) return FFM_ERR_ARG; return ffm_d2h(P->ctx, out, src, sizeof(double) * B) == FFM_OK ? B : FFM_ERR_HIP; };
    auto faceF = [&](const double *src) -> long {
        if (cap < F) return FFM_ERR_ARG;
        std::vector<double> v(std::max<long>(P->nNat, 1));
        if (ffm_d2h(P->ctx, v.data(), src, sizeof(double) * P->nNat) != FFM_OK) return FFM_ERR_HIP;
        const std::vector<int> &c2n = P->A->h_callerToNative;
        for (long f = 0; f < F; f++) out[f] = v[c2n[f]];
        return F;
    };
    if (n == "rho") return cellF(P->rho); if (n == "p") return cellF(P->p); if (n == "p_rgh") return cellF(P->p_rgh); if (n == "h") return cellF(P->hs);
    if (n == "K") return cellF(P->K); if (n == "dpdt") return cellF(P->dpdt); if (n == "gh") return cellF(P->gh); if (n == "T") return cellF(P->T);
    if (n == "Ux") return cellF(P->U[0]); if (n == "Uy") return cellF(P->U[1]); if (n == "Uz") return cellF(P->U[2]);
    for (int i = 0; i < NSP; i++) if (n == SPN[i]) return cellF(P->Y[i]);
    // old-time fields as the last step left them (rho0, K0 and psi0 trade buffers with rho, K and psi at every step)
    if (n == "rho0") return cellF(P->rho0); if (n == "K0") return cellF(P->K0); if (n == "psi0") return cellF(P->psi0); if (n == "psi") return cellF(P->psi);
    if (n == "h0") return cellF(P->hs0); if (n == "p0") return cellF(P->p0); if (n == "p_rgh0") return cellF(P->p_rgh0);
    for (int c = 0; c < 3; c++) if (n == std::string("U0") + char('x' + c)) return cellF(P->U0[c]);
    for (int i = 0; i < NSP; i++) if (i != INERT && n == std::string(SPN[i]) + "_0") return cellF(P->Y0[i]);
    if (n == "phi") return faceF(P->phi); if (n == "ghf") return faceF(P->ghf);
    if (n == "phib") return bndF(P->phib); if (n == "ph_rgh_b") return bndF(P->ph_rgh_b); if (n == "kind") return bndF(P->kind_d);
    if (n == "fStaticS") return bndF(P->fStaticS); if (n == "fStaticH") return bndF(P->fStaticH); if (n == "refH") return bndF(P->refH);
    for (int c = 0; c < 3; c++) { if (n == std::string("fStaticU") + char('0' + c)) return bndF(P->fStaticU[c]); if (n == std::string("refU") + char('0' + c)) return bndF(P->refU[c]); }
    for (int i = 0; i < NSP; i++) if (n == std::string("refY") + char('0' + i)) return bndF(P->refY[i]);
    if (n == "ghfB") {      // gh on the boundary faces: the owner cell's gh moved by half a cell along the face normal
        if (cap < B) return FFM_ERR_ARG;
        std::vector<double> gh(N), sy(B), mg(B); std::vector<int> bc(B);
        if (ffm_d2h(P->ctx, gh.data(), P->gh, sizeof(double) * N) != FFM_OK || ffm_d2h(P->ctx, sy.data(), ffm_mesh_geom(P->mesh, 7), sizeof(double) * B) != FFM_OK ||
            ffm_d2h(P->ctx, mg.data(), ffm_mesh_geom(P->mesh, 4), sizeof(double) * B) != FFM_OK || ffm_d2h(P->ctx, bc.data(), ffm_mesh_bcells(P->mesh), sizeof(int) * B) != FFM_OK) return FFM_ERR_HIP;
        for (long k = 0; k < B; k++) out[k] = gh[bc[k]] + (-9.81) * (0.5 * P->h * (sy[k] / mg[k]));
        return B;
    }
    ffm_set_error("ffm_plume_get_raw: unknown array %s", name);
    return FFM_ERR_ARG;
}

// steps so far that assembled and solved h with the species (tests)
extern "C" int ffm_plume_joint_steps(const ffm_plume *P) { return P ? P->jointSteps : FFM_ERR_ARG; }
extern "C" int ffm_plume_nsolves(const ffm_plume *P) { return P ? (int)P->log.size() : FFM_ERR_ARG; }
extern "C" int ffm_plume_get_solve(const ffm_plume *P, int i, char *name16, ffm_perf *perf)
{
    if (!P || i < 0 || i >= (int)P->log.size()) return FFM_ERR_ARG;
    if (name16) memcpy(name16, P->log[i].name, 16);
    if (perf) *perf = P->log[i].perf;
    return FFM_OK;
}
extern "C" ffm_ldu *ffm_plume_ldu(ffm_plume *P) { return P ? P->A : nullptr; }
extern "C" ffm_mesh *ffm_plume_mesh(ffm_plume *P) { return P ? P->mesh : nullptr; }
