/*
 * main_poisson_mg.c -- exe-poisson (main_poisson.c, assignment-4/src/main.c:18-41)
 * with the solve replaced by multigrid V-cycles:
 *   exe-poisson-mg <file.par>  ->  prints the parameters and the cycle count
 *   (where exe-poisson prints the iteration count), writes p.dat in the same
 *   format and prints "Walltime %.2fs".  The .par's eps is the tolerance;
 *   omg and itermax are not used (misor_solve_mg's defaults).  Under
 *   MISOR_RANKS=N (host/ranks.h) the domain is decomposed and the cycles are
 *   misor_solve_mg_dist's, with its defaults; rank 0 prints.
 */
#include <stdio.h>
#include <stdlib.h>

#include "parameter.h"
#include "ranks.h"
#include "solver_poisson.h"
#include "util.h"

static int rank_main(const RankCtx* rk, void* arg)
{
    Parameter params = *(Parameter*)arg;
    double startTime, endTime;
    Solver solver;
    int cycles = 0;
    double res = 0.0;

    initSolver(&solver, &params, 2);
    startTime = getTimeStamp();
    misorCheck(misor_solve_mg_dist(solver.dev, NULL, -1, &cycles, &res), "misor_solve_mg_dist");
    if (rk->rank == 0) printf("%d ", cycles);
    endTime = getTimeStamp();
    writeResult(&solver, "p.dat");

    if (rk->rank == 0) printf("Walltime %.2fs\n", endTime - startTime);
    misor_destroy(solver.dev);
    return 0;
}

int main(int argc, char** argv)
{
    Parameter params;
    initParameterPoisson(&params);

    if (argc < 2) {
        printf("Usage: %s <configFile>\n", argv[0]);
        exit(EXIT_SUCCESS);
    }
    readParameter(&params, argv[1]);
    printParameterPoisson(&params);
    fflush(stdout);
    return runRanks(rank_main, &params) ? EXIT_FAILURE : EXIT_SUCCESS;
}
