/*
 * main_poisson_scan.c -- the relaxation-factor study around a .par file's omg
 * as ONE batched solve (misor_batch_*, include/misor.h):
 *   exe-poisson-scan <file.par> <omg_lo> <omg_hi> <n>
 * n problems that differ only in omega -- omg_lo + m (omg_hi - omg_lo) / (n - 1),
 * omg_lo alone for n = 1 -- each with initSolver's fields (problem 2, as
 * exe-poisson) and the file's eps and itermax, solved by solveRB; prints
 * "%f %d\n" per member: omega and its iteration count.  Single rank.
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>

#include "misor.h"
#include "parameter.h"
#include "util.h"

static void usage(const char* prog)
{
    fprintf(stderr, "Usage: %s <configFile> <omg_lo> <omg_hi> <n>\n", prog);
    exit(EXIT_FAILURE);
}

static double parseDouble(const char* s, const char* prog)
{
    char* end = NULL;
    errno = 0;
    double v = strtod(s, &end);
    if (errno || end == s || *end) usage(prog);
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 5) usage(argv[0]);
    const double lo = parseDouble(argv[2], argv[0]);
    const double hi = parseDouble(argv[3], argv[0]);
    char* end = NULL;
    errno = 0;
    const long n = strtol(argv[4], &end, 10);
    if (errno || end == argv[4] || *end || n < 1 || n > 1000000) usage(argv[0]);

    Parameter params;
    initParameterPoisson(&params);
    readParameter(&params, argv[1]);

    misor_batch_desc d = { 0 };
    d.imax = params.imax;
    d.jmax = params.jmax;
    d.dx = params.xlength / params.imax;
    d.dy = params.ylength / params.jmax;
    d.nbatch = (int)n;
    d.variant = MISOR_SOLVE_RB;
    d.device = -1;
    misor_batch* b = NULL;
    misorCheck(misor_batch_create(&b, &d), "misor_batch_create");

    double* omega = allocate(64, (size_t)n * sizeof(double));
    double* eps = allocate(64, (size_t)n * sizeof(double));
    int* itermax = allocate(64, (size_t)n * sizeof(int));
    int* iters = allocate(64, (size_t)n * sizeof(int));
    for (long m = 0; m < n; m++) {
        omega[m] = n > 1 ? lo + m * (hi - lo) / (n - 1) : lo;
        eps[m] = params.eps;
        itermax[m] = params.itermax;
    }
    misorCheck(misor_batch_set_params(b, omega, eps, itermax), "misor_batch_set_params");
    misorCheck(misor_batch_poisson_init(b, params.xlength, params.ylength, 2),
               "misor_batch_poisson_init");
    misorCheck(misor_batch_solve_rb(b, iters, NULL), "misor_batch_solve_rb");
    for (long m = 0; m < n; m++) printf("%f %d\n", omega[m], iters[m]);

    misor_batch_destroy(b);
    free(omega);
    free(eps);
    free(itermax);
    free(iters);
    return EXIT_SUCCESS;
}
