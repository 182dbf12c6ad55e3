/*---------------------------------------------------------------------------*\
  fireFoam_snippets.C -- one time step of the reference's solver loop (solver/fireFoam.C:97-119) in which the four equation
  files are the REFERENCE'S OWN, included unchanged from where they lie under /root/reference/solver:

      #include "rhoEqn.H"   #include "UEqn.H"   #include "YEEqn.H"   #include "pEqn.H"      (and #include "phrghEqn.H", start-up;
      #include "solidRegionDiffusionNo.H"   #include "setMultiRegionDeltaT.H", time-step control)

  compiled against include/ffmFoam.H (the fvMesh / fvMatrix / fvm:: / fvc:: layer over the C ABI) and include/fireFoamHandles.H
  (the physics handles with the stand-ins of the synthetic plume case).  This file is what solver/createFields.H is to the
  reference: it declares the objects the snippets expect to find in scope.  Nothing of the reference is copied: the build
  (oracle/Makefile, target ref; only where the reference can be read) passes -I$(REFDIR), the reference's solver/ directory,
  and the output oracle/_ref/libffm_refsnippets.so is git-ignored.

  tests/test_reference_snippets_cpu.py builds it (the "compiles unchanged" check of SURVEY 8b B1);
  tests/test_reference_snippets_gpu.py runs the step on the device and compares the fields with the oracle.
\*---------------------------------------------------------------------------*/
#include "fireFoamHandles.H"

using namespace Foam;

struct snippetCase          // host arrays: cell fields [N] in the library's cell order, face fields [F] LDU order, boundary [B]
{
    double deltaT;
    // constants of the synthetic case (oracle/plume.py)
    double RR, Cp, Tref, pRef, mu, Pr, sO2, HC, tau;
    int nSpecies, inertIndex, fuelIndex, o2Index;
    const double* W; const double* nu;
    // state at the start of the step
    const double* rho; const double* U; const double* p; const double* p_rgh; const double* h; const double* const* Y;
    const double* K; const double* dpdt; const double* phiF; const double* phiB;
    const double* gh; const double* ghfF; const double* ghfB;
    // boundary conditions: value fraction f (-1 = inletOutlet: 1 - pos0(phi_b)), refValue; U: 3 components
    const double* fU; const double* refU; const double* fixesU;
    const double* fY; const double* const* refY; const double* fH; const double* refH;
    const double* fluxMaskP; const double* totalMaskP; const double* ph_rgh_b; const double* p_rghB;
    // results
    double* rhoOut; double* UOut; double* pOut; double* p_rghOut; double* hOut; double* const* YOut; double* TOut; double* KOut;
    double* dpdtOut; double* phiOutF; double* phiOutB; double* p_rghBOut; int* nIterOut; int nIterCap;
    // fvDOM stand-in (0 = no radiation model): 32 rays, directions / solid angles optional (NULL: built from nPhi 2, nTheta 4)
    int radiationFreq; double kAbs, sigmaSB; const double* dAve; const double* omega; double* GOut;
    // psiB != NULL: compressibility on the boundary faces (patch-face mixtures differing from the cells', e.g. the steckler
    // case's start state); the thermo object then keeps them and rho_b = psi_b*p_b.  resOut: {initial, final} residual per solve
    const double* psiB; double* resOut;
    // time-step control (controlDict adjustTimeStep / maxCo / maxDeltaT) for firefoam_snippets_time_step; dtOut: the deltaT used
    int adjustTimeStep; double maxCo, maxDeltaT; double* dtOut;
    int emptyDirections;        // bit d set: direction d is not solved (a 2-D case's `empty` patches): mesh.solutionD[d] = -1
    // wallFireSelection != 0: the solver / scheme selection of cases/wallFireSpread2D/system (BASELINE config 5) instead of the
    // steckler one: p_rgh, ph_rgh GAMG + GaussSeidel (fvSolution:36-60; gamg = the mesh's agglomeration, ffm_gamg_create), U / Yi / h
    // PBiCG + DILU (:67-75,115-152), div(phi,U) Gauss filteredLinear2V 0.2 0.05 (fvSchemes:41)
    int wallFireSelection; ffm_gamg* gamg;
    // pyro != NULL: a reactingOneDim panel (ffm_pyro_*, cases/wallFireSpread2D's pyrolysis region) behind the boundary faces
    // pyroMap[0..pyroCols): its columns are evolved by the reference's `pyrolysis.evolve()` call (solver/fireFoam.C:90-93, in
    // firefoam_snippets_time_step) with the mapped patch conditions of lib/fvPatchFieldsPyrolysis between the two regions;
    // pyroQin [B]: incident radiative flux on the wall faces
    ffm_pyro* pyro; int pyroCols; const int* pyroMap; const double* pyroQin; double pyroEmissivity, pyroAbsorptivity, pyroHocSolid, pyroQFuel;
    // fvdomReal != 0: the reference's fvDOM itself (handle `fvDOM` of include/fireFoamHandles.H: the iteration of calculate(), grey-diffusive
    // walls) as the radiation model, with fvDOMCoeffs nPhi / nTheta / maxIter / convergence, solverFreq = radiationFreq, constRadFractionEmission
    // (a = kAbs, Ehrr1, Ehrr2, radScaling over the faces of radMlrMask) and the div(Ji,Ii_h) scheme radDivScheme (0 upwind, 5 linearUpwind):
    // cases/wallFireSpread2D/constant/radiationProperties:28-60, system/fvSchemes:66.  radEmissivity [B]: the walls' `lookup` emissivities.
    // pyroInStep != 0: the panel is evolved in the reference's order of evaluation (coupled wall condition inside the solid's step, gas
    // patches from the new solid state); with fvdomReal the solid reads the model's qin and writes its surface emissivity into the
    // model's wall emissivities (emissivityMode solidRadiation); pyroMaxDi: controlDict maxDi
    int fvdomReal, radNPhi, radNTheta, radMaxIter, radDivScheme; double radTolerance, radEhrr1, radEhrr2; const double* radMlrMask; const double* radMlrMask2; const double* radEmissivity;
    double* qinOut; int* radItersOut;
    int pyroInStep; double pyroMaxDi;
};

// ---- what solver/createFields.H declares, as the members of one object so that the state stays on the device from one time
// step to the next: fvSolution / fvSchemes of the synthetic case (cf. cases/steckler/system/fvSolution:19-101, fvSchemes:28-61),
// thermo / composition / Y, the fields, the physics handles.  Objects boundary conditions look up by name are registered with
// mesh.store() (inletOutlet: phi; prghTotalHydrostaticPressure: rho, U, phi).  The member functions are the reference's loop:
// inside them the members are in scope under the names the equation files use.
struct snippetSolver
{
    ffm_ctx* ctx; ffm_mesh* msh;
    fvMesh mesh;
    const label N, B;
    std::vector<double> zeroBh;
    pimpleControl pimple;
    perfectGasConstCpThermo thermoObj;
    psiReactionThermo& thermo;
    basicMultiComponentMixture& composition;
    PtrList<volScalarField>& Y;
    const label inertIndex;
    volScalarField& p;
    volScalarField& T;
    const volScalarField& psi;
    volScalarField rho;
    volVectorField U;
    surfaceScalarField phi;
    volScalarField p_rgh, gh;
    surfaceScalarField ghf;
    const dimensionedScalar pRef;
    volScalarField K, dpdt, Qdot;
    multivariateSurfaceInterpolationScheme<scalar>::fieldTable fields;
    autoPtr<compressible::turbulenceModel> turbulence;
    autoPtr<combustionModels::psiCombustionModel> combustion;
    autoPtr<radiation::radiationModel> radiation;
    noParcels parcels;
    noSurfaceFilm surfaceFilm;
    noFvOptions fvOptions;
    noMRF MRF;
    const scalar lewisNo = 1;                                   // solver/readAdditionalThermo.H:32
    dimensionedScalar DM;
    const bool constD = false;
    scalar cumulativeContErr = 0;
    Time runTime;
    struct { bool adjustTimeStep; scalar maxCo, maxDeltaT; } timeControls;
    pyrolysisModelCollection pyrolysis;
    scalar maxDi;                                               // solver/readPyrolysisTimeControls.H:32
    const bool solvePyrolysisRegion = true, solvePrimaryRegion = true;      // solver/createFields.H:134-145

    static pimpleDict pimpleOf()
    {
        pimpleDict pd; pd.nOuterCorrectors = 1; pd.nCorrectors = 2; pd.nNonOrthogonalCorrectors = 0;      // fvSolution:84-92
        pd.hydrostaticInitialization = true; pd.nHydrostaticCorrectors = 5;
        return pd;
    }
    std::shared_ptr<mixedBC> zeroGradient() { return std::make_shared<mixedBC>(ctx, B, zeroBh.data(), zeroBh.data(), zeroBh.data()); }

    snippetSolver(ffm_ctx* c, ffm_ldu* ldu, ffm_mesh* m, const snippetCase* cs)
    : ctx(c), msh(m), mesh(c, ldu, m, cs->deltaT), N(mesh.nCells), B(mesh.nBoundary), zeroBh(B, 0.0), pimple(mesh, pimpleOf()),
      thermoObj(mesh, cs->RR, cs->Cp, cs->Tref), thermo(thermoObj), composition(thermo.composition()), Y(composition.Y()),
      inertIndex(cs->inertIndex), p(thermo.p()), T(thermo.T()), psi(thermo.psi()), rho("rho", mesh), U("U", mesh), phi(mesh),
      p_rgh("p_rgh", mesh), gh("gh", mesh), ghf(mesh), pRef("pRef", cs->pRef), K("K", mesh), dpdt("dpdt", mesh), Qdot("Qdot", mesh),
      parcels(mesh), surfaceFilm(mesh), DM("DM", 0.0), runTime(0, cs->deltaT),
      timeControls{cs->adjustTimeStep != 0, cs->maxCo, cs->maxDeltaT}, maxDi(pyrolysis.maxDiff())
    {
        runTime.link(mesh.deltaT);
        for (int d = 0; d < 3; d++) if (cs->emptyDirections & (1 << d)) mesh.solutionD[d] = -1;
        mesh.solvers["rho"] = mesh.solvers["rhoFinal"] = {FFM_DIAGONAL, FFM_NONE, 1e-6, 0, 0, 1000, 1};
        mesh.solvers["U"] = mesh.solvers["UFinal"] = {FFM_PBICGSTAB, FFM_DILU, 1e-6, 0, 0, 1000, 1};
        mesh.solvers["Yi"] = mesh.solvers["YiFinal"] = {FFM_PBICGSTAB, FFM_DILU, 1e-8, 0, 0, 1000, 1};
        mesh.solvers["h"] = mesh.solvers["hFinal"] = {FFM_PBICGSTAB, FFM_DILU, 1e-8, 0, 0, 1000, 1};
        mesh.solvers["p_rgh"] = mesh.solvers["ph_rgh"] = {FFM_PCG, FFM_DIC, 1e-6, 0.01, 0, 1000, 1};     // fvSolution:29-46
        mesh.solvers["p_rghFinal"] = {FFM_PCG, FFM_DIC, 1e-6, 0, 0, 1000, 1};
        if (cs->wallFireSelection) {
            solverControls g; g.solver = FFM_GAMG; g.preconditioner = FFM_GS; g.tolerance = 1e-5; g.relTol = 0.01;
            mesh.solvers["p_rgh"] = mesh.solvers["ph_rgh"] = g;
            g.tolerance = 1e-6; g.relTol = 0; mesh.solvers["p_rghFinal"] = g;
            mesh.solvers["U"] = {FFM_PBICG, FFM_DILU, 1e-6, 0, 0, 1000, 1}; mesh.solvers["UFinal"] = {FFM_PBICG, FFM_DILU, 1e-7, 0, 0, 1000, 1};
            mesh.solvers["Yi"] = mesh.solvers["YiFinal"] = mesh.solvers["h"] = mesh.solvers["hFinal"] = {FFM_PBICG, FFM_DILU, 1e-8, 0, 0, 1000, 1};
            mesh.gamg = cs->gamg;
        }
        if (std::getenv("FFM_PLUME_TIGHT")) for (auto& kv : mesh.solvers) if (kv.second.solver != FFM_DIAGONAL) { kv.second.tolerance = 1e-13; kv.second.relTol = 0; }
        mesh.divSchemes["div(phi,U)"] = {4, 1, 0, 1};                                   // Gauss LUST grad(U)
        if (cs->wallFireSelection) mesh.divSchemes["div(phi,U)"] = {6, 0.2, 0.05, 1};   // Gauss filteredLinear2V 0.2 0.05
        mesh.divSchemes["div(phi,K)"] = {2, 1, 0, 1};                                   // Gauss limitedLinear 1
        mesh.divSchemes["div(phiv,p)"] = {2, 1, 0, 1};
        mesh.multivariateSelection["div(phi,Yi_h)"]["h"] = {2, 1, 0, 1};                // h limitedLinear 1
        static const char* specieNames[] = {"O2", "H2O", "C3H8", "CO2", "N2"};
        for (label i = 0; i < cs->nSpecies; i++) {
            composition.species_.push_back(specieNames[i]); composition.active_.push_back(true);
            thermoObj.W_.push_back(cs->W[i]);
            Y.append(new volScalarField(specieNames[i], mesh));
            Y[i].v.assignHost(cs->Y[i]);
            Y[i].bc = std::make_shared<mixedBC>(ctx, B, cs->fY, cs->refY[i], zeroBh.data());
            mesh.multivariateSelection["div(phi,Yi_h)"][specieNames[i]] = {3, 1, 0, 1};  // Yi limitedLinear01 1
        }
        p.v.assignHost(cs->p); p.b = mesh.patchInternal(p.v);
        if (cs->psiB) { thermoObj.zeroGradientBoundaries_ = false; thermoObj.psi_.b.assignHost(cs->psiB); }
        thermo.he().v.assignHost(cs->h);
        thermo.he().bc = std::make_shared<mixedBC>(ctx, B, cs->fH, cs->refH, zeroBh.data());
        rho.v.assignHost(cs->rho); rho.bc = zeroGradient(); rho.correctBoundaryConditions();
        for (int d = 0; d < 3; d++) { U.v[d].assignHost(cs->U + (size_t)d*N); U.bc[d] = std::make_shared<mixedBC>(ctx, B, cs->fU + (size_t)d*B, cs->refU + (size_t)d*B, zeroBh.data()); }
        U.fixesValue = std::make_shared<dField>(ctx, B); U.fixesValue->assignHost(cs->fixesU);
        FFM_FOAM_CHK(ffm_faces_to_native(msh, cs->phiF, phi.v.data())); phi.b.assignHost(cs->phiB);
        // p_rgh: fixedFluxPressure where fluxMaskP = 1 (gradient from constrainPressure), prghTotalHydrostaticPressure where
        // totalMaskP = 1 (value ph_rgh - 0.5*rho*(1 - pos0(phi))*|U|^2); boundary values as the last evaluate() left them
        p_rgh.v.assignHost(cs->p_rgh); p_rgh.b.assignHost(cs->p_rghB);
        p_rgh.bc = std::make_shared<mixedBC>(ctx, B, cs->totalMaskP, zeroBh.data(), zeroBh.data());
        p_rgh.bc->totalMask = std::make_shared<dField>(ctx, B); p_rgh.bc->totalMask->assignHost(cs->totalMaskP);
        p_rgh.bc->ph_rgh_b = std::make_shared<dField>(ctx, B); p_rgh.bc->ph_rgh_b->assignHost(cs->ph_rgh_b);
        p_rgh.fixedFluxMask = std::make_shared<dField>(ctx, B); p_rgh.fixedFluxMask->assignHost(cs->fluxMaskP);
        gh.v.assignHost(cs->gh); gh.b.assignHost(cs->ghfB);
        FFM_FOAM_CHK(ffm_faces_to_native(msh, cs->ghfF, ghf.v.data())); ghf.b.assignHost(cs->ghfB);
        K.v.assignHost(cs->K); dpdt.v.assignHost(cs->dpdt);
        forAll(Y, i) { fields.add(Y[i]); }
        fields.add(thermo.he());
        turbulence = autoPtr<compressible::turbulenceModel>(new constantViscosity(mesh, cs->mu, cs->Pr));
        std::vector<scalar> nu(cs->nu, cs->nu + cs->nSpecies);
        combustion = autoPtr<combustionModels::psiCombustionModel>(new singleStepEDC(thermo, rho, cs->fuelIndex, cs->o2Index, cs->sO2, cs->tau, cs->HC, nu));
        if (cs->radiationFreq > 0 && cs->fvdomReal) {
            mesh.divSchemes["div(Ji,Ii_h)"] = {cs->radDivScheme, 1, 0, 1};
            if (cs->wallFireSelection) { solverControls g; g.solver = FFM_GAMG; g.preconditioner = FFM_DILU; g.tolerance = 1e-4; g.relTol = 0; mesh.solvers["Ii"] = mesh.solvers["IiFinal"] = g; }   // fvSolution:160-170
            else mesh.solvers["Ii"] = mesh.solvers["IiFinal"] = {FFM_PBICGSTAB, FFM_DILU, 1e-4, 0, 0, 1000, 1};
            fvDOM* dom = new fvDOM(mesh, T, cs->radNPhi, cs->radNTheta, cs->radiationFreq, cs->sigmaSB,
                                   std::make_shared<constRadFractionEmission>(mesh, cs->kAbs, cs->radEhrr1, cs->radEhrr2, cs->radMlrMask, cs->radMlrMask2));
            dom->setIteration(cs->radMaxIter, cs->radTolerance);
            if (cs->radEmissivity) dom->emissivity().assignHost(cs->radEmissivity);
            const scalar Cp = cs->Cp;
            dom->Cpv = [this, Cp]() { return uniformField("Cpv", mesh, Cp); };
            radiation = autoPtr<radiation::radiationModel>(dom);
            mesh.store("Qdot", Qdot);
        }
        else if (cs->radiationFreq > 0) {
            mesh.divSchemes["div(Ji,Ii_h)"] = {0, 1, 0, 1};                                     // Gauss upwind (fvSchemes:60)
            mesh.solvers["Ii"] = mesh.solvers["IiFinal"] = {FFM_PBICGSTAB, FFM_DILU, 1e-4, 0, 0, 1000, 1};
            radiation = autoPtr<radiation::radiationModel>(new fvDOMStandIn(mesh, T, 2, 4, cs->radiationFreq, cs->kAbs, cs->sigmaSB, cs->Tref, cs->dAve, cs->omega));
        }
        else radiation = autoPtr<radiation::radiationModel>(new noRadiation());
        mesh.store("phi", phi); mesh.store("rho", rho); mesh.store("U", U);
        if (cs->pyro) {
            pyrolysis.attach(mesh, cs->pyro, cs->pyroCols, cs->pyroMap, cs->pyroQin, cs->pyroEmissivity, cs->pyroAbsorptivity, cs->pyroHocSolid, cs->pyroQFuel,
                             U, thermo.he(), T, rho);
            const scalar Cp = cs->Cp, Tref = cs->Tref;
            // gas side of the wall: kappaEff = Cp*alphaEff (the stand-in thermo's constant Cp), he = Cp*(T - Tref)
            pyrolysis.kappaDelta = [this, Cp]() { return binary(FFM_OP_MUL, scalarOp(FFM_OP_MUL, turbulence->alphaEff().b, Cp), mesh.boundaryGeometry(5)); };
            pyrolysis.heOfT = [Cp, Tref](const dField& Tw) { return scalarOp(FFM_OP_MUL, scalarOp(FFM_OP_SUB, Tw, Tref), Cp); };
            pyrolysis.setCoupledInStep(cs->pyroInStep != 0);
            if (cs->pyroMaxDi > 0) { pyrolysis.setMaxDi(cs->pyroMaxDi); maxDi = pyrolysis.maxDiff(); }
            if (cs->pyroInStep && cs->radiationFreq > 0 && cs->fvdomReal) {
                fvDOM* dom = static_cast<fvDOM*>(&radiation());
                pyrolysis.qinOfRadiation = [dom]() -> const dField& { return dom->qin_; };
                pyrolysis.wallEmissivity = &dom->emissivity();
            }
        }
        thermo.correct();                                           // T, psi of the start state
        U.correctBoundaryConditions(); thermo.he().correctBoundaryConditions();
        forAll(Y, i) { Y[i].correctBoundaryConditions(); }
    }

    // one time step: solver/fireFoam.C:84,97-119 with the reference's equation files
    void step()
    {
        mesh.log.clear();
        // runTime++: old-time levels
        rho.storeOldTime(); U.storeOldTime(); thermo.he().storeOldTime(); K.storeOldTime(); p.storeOldTime(); p_rgh.storeOldTime();
        thermoObj.psi_.storeOldTime(); phi.storeOldTime();
        forAll(Y, i) { Y[i].storeOldTime(); }

        #include "rhoEqn.H"

        // --- PIMPLE loop
        while (pimple.loop())
        {
            #include "UEqn.H"
            #include "YEEqn.H"

            // --- Pressure corrector loop
            while (pimple.correct())
            {
                #include "pEqn.H"
            }

            if (pimple.turbCorr())
            {
                turbulence->correct();
            }
        }

        rho = thermo.rho();
        FFM_FOAM_CHK(ffm_ctx_sync(ctx));
    }

    // the body of the time loop, solver/fireFoam.C:76-121: time-step control (the reference's solidRegionDiffusionNo.H and
    // setMultiRegionDeltaT.H between this layer's versions of the OpenFOAM headers), then the step
    void timeStep()
    {
        #include "readTimeControls.H"
        #include "compressibleCourantNo.H"
        #include "solidRegionDiffusionNo.H"
        #include "setMultiRegionDeltaT.H"
        #include "setDeltaT.H"

        runTime++;

        parcels.evolve();

        surfaceFilm.evolve();

        if(solvePyrolysisRegion)
        {
            pyrolysis.evolve();
        }

        if (solvePrimaryRegion)
        {
            step();
        }
        (void)meanCoNum;
    }

    // solver/createFields.H:100-104 -> solver/phrghEqn.H: hydrostatic initialisation (nHydrostaticCorrectors solves of
    // fvm::laplacian(rhof, ph_rgh) == fvc::div(phig)); the case's 0/ph_rgh: fixedValue 0 where topMask = 1, fixedFluxPressure elsewhere
    void hydrostatic(const double* topMask, const double* fluxMask)
    {
        mesh.log.clear();
        {
            std::shared_ptr<volScalarField> f(new volScalarField("ph_rgh", mesh));
            f->bc = std::make_shared<mixedBC>(ctx, B, topMask, zeroBh.data(), zeroBh.data());
            f->fixedFluxMask = std::make_shared<dField>(ctx, B); f->fixedFluxMask->assignHost(fluxMask);
            mesh.fieldFiles["ph_rgh"] = f;
        }
        thermo.correct();
        rho = thermo.rho();

        #include "phrghEqn.H"

        FFM_FOAM_CHK(ffm_ctx_sync(ctx));
    }

    void download(const snippetCase* cs, bool all)
    {
        rho.v.toHost(cs->rhoOut); p.v.toHost(cs->pOut); p_rgh.v.toHost(cs->p_rghOut); p_rgh.b.toHost(cs->p_rghBOut);
        if (!all) return;
        thermo.he().v.toHost(cs->hOut); T.v.toHost(cs->TOut); K.v.toHost(cs->KOut); dpdt.v.toHost(cs->dpdtOut);
        for (int d = 0; d < 3; d++) U.v[d].toHost(cs->UOut + (size_t)d*N);
        forAll(Y, i) { Y[i].v.toHost(cs->YOut[i]); }
        FFM_FOAM_CHK(ffm_faces_from_native(msh, phi.v.data(), cs->phiOutF)); phi.b.toHost(cs->phiOutB);
        if (cs->radiationFreq > 0 && cs->fvdomReal) {
            fvDOM& dom = static_cast<fvDOM&>(radiation());
            if (cs->GOut) dom.G_.v.toHost(cs->GOut);
            if (cs->qinOut) dom.qin_.toHost(cs->qinOut);
            if (cs->radItersOut) *cs->radItersOut = dom.lastIterations_;
        }
        else if (cs->radiationFreq > 0 && cs->GOut) static_cast<fvDOMStandIn&>(radiation()).G_.v.toHost(cs->GOut);
    }
    int iterations(const snippetCase* cs, bool skipRho)
    {
        int n = 0;
        for (const solverPerformance& sp : mesh.log) if (!(skipRho && sp.fieldName == "rho") && n < cs->nIterCap) {
            if (cs->resOut) { cs->resOut[2*n] = sp.initialResidual; cs->resOut[2*n + 1] = sp.finalResidual; }
            cs->nIterOut[n++] = sp.nIterations;
        }
        return n;
    }
};

// ---- C entry points -------------------------------------------------------------------------------------------------------
extern "C" snippetSolver* firefoam_snippets_create(ffm_ctx* ctx, ffm_ldu* ldu, ffm_mesh* msh, const snippetCase* cs) { return new snippetSolver(ctx, ldu, msh, cs); }
extern "C" void firefoam_snippets_destroy(snippetSolver* s) { delete s; }
// one time step on the device-resident state; returns the number of linear solves (iteration counts in cs->nIterOut, diagonal
// solves left out); results are downloaded only if download != 0
extern "C" int firefoam_snippets_advance(snippetSolver* s, const snippetCase* cs, int download)
{
    s->step();
    if (download) s->download(cs, true);
    return s->iterations(cs, true);
}
// the same with the time-step control of the reference's loop in front (adjustTimeStep / maxCo / maxDeltaT of the case)
extern "C" int firefoam_snippets_time_step(snippetSolver* s, const snippetCase* cs, int download)
{
    s->timeStep();
    if (cs->dtOut) *cs->dtOut = s->runTime.deltaTValue();
    if (download) s->download(cs, true);
    return s->iterations(cs, true);
}
extern "C" int firefoam_snippets_step(ffm_ctx* ctx, ffm_ldu* ldu, ffm_mesh* msh, const snippetCase* cs)
{
    snippetSolver s(ctx, ldu, msh, cs);
    s.step();
    s.download(cs, true);
    return s.iterations(cs, true);
}
// inputs: p (uniform pRef), h, Y, U = 0; totalMaskP = the fixedValue-0 patch of ph_rgh (the top), fluxMaskP = its fixedFluxPressure
// patches.  Results: p_rghOut (= ph_rgh), pOut, rhoOut, p_rghBOut (boundary values of ph_rgh)
extern "C" int firefoam_snippets_hydrostatic(ffm_ctx* ctx, ffm_ldu* ldu, ffm_mesh* msh, const snippetCase* cs)
{
    snippetSolver s(ctx, ldu, msh, cs);
    std::cout.precision(8);              // Time::readDict: IOstream::defaultPrecision(writePrecision 8) (cases/steckler/system/controlDict:36-38)
    s.hydrostatic(cs->totalMaskP, cs->fluxMaskP);
    s.download(cs, false);
    return s.iterations(cs, false);
}
