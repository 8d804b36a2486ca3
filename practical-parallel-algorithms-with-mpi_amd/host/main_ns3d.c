/*
 * main_ns3d.c -- the assignment-6 driver (src/main.c:21-118) on libmisor's 3D
 * path:  exe-ns3d <file.par>  (assignment-6's dcavity.par / canal.par).
 * Same loop (no normalizePressure), same progress bar, same "Solution took
 * %.2fs" line, same <problem>.vtk output (ASCII, as the reference's
 * VtkOptions default; MISOR_VTK_FORMAT=binary selects the BINARY variant).
 * MISOR_ITERLOG=<file> additionally writes one line per time step:
 * "nt t dt iterations".  MISOR_RANKS=N (or a launcher's WORLD_SIZE/RANK,
 * host/ranks.h) runs it decomposed into N slabs of planes like the
 * reference's mpirun -np N; rank 0 prints and writes the collected result.
 * MISOR_DIMS=XxYxZ splits the box over that 3D Cartesian process grid instead
 * of slabs, as the reference's MPI_Dims_create / MPI_Cart_create does (a 0
 * entry is chosen automatically: MISOR_DIMS=0x0x0 with 8 ranks is 2x2x2).
 * MISOR_PSOLVE=mg replaces the step's red-black SOR by multigrid V-cycles
 * (misor3_solve_mg, default parameters; single rank only) and prints one line
 * naming the solver; MISOR_PSOLVE=mgdist is the same on any number of slabs
 * (misor3_solve_mg_dist, defaults; not with MISOR_DIMS); unset or "sor" is the
 * reference's solve.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "parameter.h"
#include "progress.h"
#include "ranks.h"
#include "solver_ns3d.h"
#include "util.h"
#include "vtk_writer.h"

static int rank_main(const RankCtx* rk, void* arg)
{
    Parameter p = *(Parameter*)arg;
    const int root = rk->rank == 0;
    double timeStart, timeStop;
    Solver s;
    initSolver(&s, &p);
#ifndef VERBOSE
    if (root) initProgress(s.te);
#endif
    const char* logname = getenv("MISOR_ITERLOG");
    FILE* ilog = (root && logname) ? fopen(logname, "w") : NULL;

    double tau = s.tau;
    double te = s.te;
    double t = 0.0;
    int nt = 0;

    timeStart = getTimeStamp();
    while (t <= te) { /* dt is all-reduced: every rank takes the same steps */
        if (tau > 0.0) computeTimestep(&s);
        setBoundaryConditions(&s);
        setSpecialBoundaryCondition(&s);
        computeFG(&s);
        computeRHS(&s);
        solve(&s);
        adaptUV(&s);
        if (ilog) fprintf(ilog, "%d %.17g %.17g %d\n", nt, t, s.dt, s.lastIterations);
        t += s.dt;
        nt++;
#ifdef VERBOSE
        if (root) printf("TIME %f , TIMESTEP %f\n", t, s.dt);
#else
        if (root) printProgress(t);
#endif
    }
    timeStop = getTimeStamp();
    if (root) {
#ifndef VERBOSE
        stopProgress();
#endif
        printf("Solution took %.2fs\n", timeStop - timeStart);
    }
    if (ilog) fclose(ilog);

    double *pg = NULL, *ug = NULL, *vg = NULL, *wg = NULL;
    if (root) {
        size_t bytesize = (size_t)s.grid.imax * s.grid.jmax * s.grid.kmax * sizeof(double);
        pg = allocate(64, bytesize);
        ug = allocate(64, bytesize);
        vg = allocate(64, bytesize);
        wg = allocate(64, bytesize);
    }
    collectResult(&s, pg, ug, vg, wg);
    if (root) {
        const char* fmt = getenv("MISOR_VTK_FORMAT");
        VtkOptions opts = { .grid = s.grid };
        if (fmt && strcmp(fmt, "binary") == 0) opts.fmt = BINARY;
        vtkOpen(&opts, s.problem);
        vtkScalar(&opts, "pressure", pg);
        vtkVector(&opts, "velocity", (VtkVector){ ug, vg, wg });
        vtkClose(&opts);
        free(pg);
        free(ug);
        free(vg);
        free(wg);
    }
    freeSolver(&s);
    return 0;
}

int main(int argc, char** argv)
{
    Parameter p;
    initParameter(&p);
    if (argc != 2) {
        printf("Usage: %s <configFile>\n", argv[0]);
        exit(EXIT_SUCCESS);
    }
    readParameter(&p, argv[1]);
    int dims[3];
    (void)rankDims(dims); /* a malformed MISOR_DIMS ends the program here, before any rank starts */
    /* MISOR_PSOLVE: a bad value, mg on more than one rank, or mgdist on a
     * Cartesian process grid ends the program here, before any rank starts */
    const char* nr = getenv("MISOR_RANKS");
    const char* ws = getenv("WORLD_SIZE");
    const int ranks = nr ? atoi(nr) : (ws ? atoi(ws) : 1);
    const int psolve = pressureSolver(ranks);
    const char* r = getenv("RANK");
    if (!r || atoi(r) == 0) printParameter3D(&p);
    if (psolve == PSOLVE_MG)
        printf("Pressure solver: geometric multigrid V-cycles (misor3_solve_mg)\n");
    if (psolve == PSOLVE_MGDIST)
        printf("Pressure solver: geometric multigrid V-cycles on %d slab%s "
               "(misor3_solve_mg_dist)\n", ranks > 1 ? ranks : 1, ranks > 1 ? "s" : "");
    fflush(stdout);
    return runRanks(rank_main, &p) ? EXIT_FAILURE : EXIT_SUCCESS;
}
