/*
 * misor.h -- C ABI of libmisor: MI355X-native red-black SOR for the 2D
 * pressure Poisson equation and the 2D Navier-Stokes step kernels around it.
 *
 * This is the drop-in boundary for the reference's L4 solver layer.  The
 * reference has no FFI: its C `main` calls plain functions declared in
 * solver.h.  Each entry point below replaces one of them (cited per function);
 * the host programs in practical-parallel-algorithms-with-mpi_amd/host/ keep
 * the reference's own names (initSolver, solveRB, computeFG, ...) as thin
 * wrappers over these calls, see INTEGRATION.md.
 *
 * Conventions
 *  - Plain C: pointers, sizes, scalars.  No HIP/torch types in signatures.
 *  - Host arrays exchanged with the library use the reference layout:
 *    (ni+2) x (nj+2) doubles, row-major, i fastest, A(i,j) = a[j*(ni+2)+i]
 *    (assignment-4/src/solver.c:16), where (ni,nj) is the LOCAL block of this
 *    rank (= (imax,jmax) on one GPU).
 *  - Every function returns MISOR_OK (0) or a negative MISOR_E* code;
 *    misor_last_error() describes the last failure of the calling thread.
 *    The reference prints and exit(EXIT_FAILURE)s instead (allocate.c:18-35,
 *    parameter.c:32-35); the host wrappers map a non-zero return to exactly
 *    that.
 *  - Device fields live in HBM for the lifetime of the grid; nothing is
 *    copied across the boundary except by misor_upload / misor_download.
 */
#ifndef MISOR_H
#define MISOR_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MISOR_OK 0
#define MISOR_EINVAL (-1)   /* bad argument */
#define MISOR_EHIP (-2)     /* HIP runtime error */
#define MISOR_ENOMEM (-3)   /* device allocation failed */
#define MISOR_ECOMM (-4)    /* RCCL error */
#define MISOR_ESTATE (-5)   /* call not valid in this state */

/* field ids */
enum { MISOR_P = 0, MISOR_RHS = 1, MISOR_U = 2, MISOR_V = 3, MISOR_F = 4, MISOR_G = 5 };

/* boundary flags, assignment-5/sequential/src/solver.h:11 */
enum { MISOR_NOSLIP = 1, MISOR_SLIP = 2, MISOR_OUTFLOW = 3, MISOR_PERIODIC = 4 };

/* special boundary condition, selected in the reference by strcmp on the
 * problem name (assignment-5/sequential/src/solver.c:345,349) */
enum { MISOR_PROBLEM_NONE = 0, MISOR_PROBLEM_DCAVITY = 1, MISOR_PROBLEM_CANAL = 2 };

/* SOR update form: solveRB (P -= factor*r, factor includes omega,
 * assignment-4/src/solver.c:189,211) or solveRBA (P -= omega*factor*r,
 * :250,273) */
enum { MISOR_SOLVE_RB = 0, MISOR_SOLVE_RBA = 1 };

typedef struct misor_grid misor_grid;

typedef struct {
    /* global grid and the SOR parameters of Solver
     * (assignment-4/src/solver.h:11-22, assignment-5/sequential/src/solver.h:13-32) */
    int imax, jmax;     /* interior cells, whole domain */
    double dx, dy;      /* xlength/imax, ylength/jmax */
    double omega, eps;
    int itermax;
    int variant;        /* MISOR_SOLVE_RB or MISOR_SOLVE_RBA */
    int device;         /* HIP device ordinal; -1 = current device */
    /* 2D domain decomposition (assignment-5/skeleton/src/solver.c:445-473).
     * nranks = 1 for a single GPU; then the rest is ignored. */
    int nranks, rank;
    int dims[2];        /* process grid {x, y}; {0,0} = MPI_Dims_create rule */
    const void* comm_id; /* MISOR_COMM_ID_BYTES from misor_comm_unique_id() on rank 0:
                          * one process per GPU, halos and reductions over RCCL.
                          * Bytes starting with "LOCAL:<name>" select the in-process
                          * transport instead: the nranks grids of group <name> are
                          * created and driven by nranks host threads of ONE process
                          * (any devices, also all on one GPU); every member must make
                          * the same sequence of calls, as with RCCL. */
} misor_desc;

#define MISOR_COMM_ID_BYTES 128

/* NS physics parameters (assignment-5/sequential/src/solver.h:13-32) */
typedef struct {
    double xlength, ylength;
    double re, gx, gy, gamma, tau;
    int bcLeft, bcRight, bcBottom, bcTop;
    int problem;        /* MISOR_PROBLEM_* */
} misor_ns_desc;

/* what this rank owns (for uploads/downloads and tests) */
typedef struct {
    int ni, nj;         /* local interior cells */
    int ioff, joff;     /* global index of local cell (0,0) */
    int coords[2], dims[2];
    int neighbours[4];  /* left, right, bottom, top rank or -1 */
    long long pitch;    /* device row pitch in doubles */
} misor_local;

/* per-grid counters; sweep_ms is summed from HIP events recorded around
 * every sweep pass when timing is enabled (misor_enable_timing).  A pass is
 * one sweep kernel launch (two for an overlapped decomposed pass: interior
 * blocks, then boundary blocks) doing iters_per_pass red+black iterations
 * (MISOR_TUNE_TSTEPS). */
typedef struct {
    long long sweeps;       /* red+black iterations executed on the device */
    long long launches;     /* passes launched (incl. early-exited) */
    double sweep_ms;        /* total device time of timed passes (timing on) */
    long long timed_sweeps; /* iterations computed by the timed passes */
    long long timed_passes; /* passes covered by sweep_ms */
    int iters_per_pass;     /* T of the last multi-block solve (1: single sweep) */
    int tb_variant;         /* its TB variant (MISOR_TUNE_TB_VARIANT; -1: single sweep) */
    /* decomposed solves, timing on: HIP events around every halo exchange
     * (pack + transport + unpack) and every residual all-reduce (+ loop test)
     * on the stream that runs it (the communication stream when overlapped) */
    double halo_ms;         /* total device time of the solve's halo exchanges */
    long long halos;        /* exchanges covered by halo_ms */
    double allreduce_ms;    /* total device time of the residual all-reduces */
    long long allreduces;   /* all-reduces covered by allreduce_ms */
    int chained;            /* 1: the last multi-block solve's passes were chained runs
                             * (sor_tb.h rb_tbc_kernel / sor_tbh.h rb_tbhc_kernel) */
    /* NS step kernels, timing on: HIP events on the grid stream around each
     * launch.  [0] computeFG (+ the fused computeRHS, ns_kernels.hip
     * fg_rhs_kernel), [1] adaptUV (+ the next dt's max |u|, |v| partials,
     * adapt_absmax_kernel), [2] normalizePressure (max |p|, exact sum,
     * subtract: absmax2 + finish_reduce, exact_sum, sub_mean kernels) */
    double ns_ms[3];
    long long ns_calls[3];
    /* solves whose residual lower bounds (MISOR_TUNE_RES_LITE) missed once: the
     * pass redone counting every cell, the rest of the solve so */
    long long lite_misses;
    /* the last misor_solve_mg of this grid: cycles run and levels of its
     * hierarchy; with timing on, the device time of the two transfer kernels
     * of level 0 ([0] residual + restriction, [1] prolongation + correction),
     * summed over the solves since the last reset, and the launches it covers
     * (level 0's smoothing is in sweep_ms like any solve's) */
    int mg_cycles, mg_levels;
    double mg_transfer_ms[2];
    long long mg_transfers;
    /* the fused tail (misor_mg_tail, MISOR_TUNE_MG_TAIL): levels the last
     * misor_solve_mg cycled in one launch (0: none -- the tail has fewer than
     * two levels, the knob is off, or no cycle ran); its launches, and the
     * cycles the host finished level by level because the coarsest solve came
     * near its threshold, both since the last reset; with timing on, the device
     * time of those launches.  The iterations the fused levels run are in no
     * other counter: where level 0 is in the tail, sweeps and sweep_ms do not
     * count its smoothing */
    int mg_tail_levels;
    long long mg_tail_launches;
    long long mg_tail_fallbacks;
    double mg_tail_ms;
    /* the last multigrid solve of this grid: the levels misor_solve_mg_dist kept
     * distributed over the ranks (misor_mg_dist_levels' ndist); 0 after
     * misor_solve_mg and on a grid that is not decomposed.  After
     * misor_solve_mg_dist on a decomposed grid mg_tail_levels counts the fused
     * levels of the gathered part, and the tail's other counters stay as they
     * were */
    int mg_dist_levels;
} misor_stats;

const char* misor_last_error(void);
const char* misor_version(void);

/* decomposition rule of MPI_Dims_create(n, 2) + sizeOfRank
 * (assignment-5/skeleton/src/solver.c:30-32,445,472-473); host-only */
int misor_decompose(int nranks, int rank, int imax, int jmax, const int dims_in[2],
                    misor_local* out);

/* rank 0 calls this and ships the bytes to the other ranks out of band */
int misor_comm_unique_id(void* id_out /* MISOR_COMM_ID_BYTES */);

/* replaces the allocation half of initSolver (assignment-4/src/solver.c:83-97,
 * assignment-5/sequential/src/solver.c:59-91): all six fields, zeroed */
int misor_create(misor_grid** out, const misor_desc* desc);
void misor_destroy(misor_grid* g);
int misor_local_info(const misor_grid* g, misor_local* out);

/* stream the grid's kernels run on (hipStream_t as void*); NULL = own stream */
int misor_set_stream(misor_grid* g, void* hip_stream);
int misor_synchronize(misor_grid* g);

int misor_upload(misor_grid* g, int field, const double* host);
int misor_download(misor_grid* g, int field, double* host);
/* collectResult / assembleResult (assignment-5/skeleton/src/solver.c:234-359):
 * collective over the ranks of a decomposed grid.  Rank 0 receives the whole
 * field, (imax+2) x (jmax+2) doubles in the reference layout, in `host_global`;
 * every rank contributes its interior plus the ghost layer on its physical
 * sides; other ranks pass NULL.  With one rank it is misor_download. */
int misor_gather(misor_grid* g, int field, double* host_global);
/* exchange (assignment-5/skeleton/src/solver.c:137-165): collective over the
 * ranks of a decomposed grid.  The `depth`-deep halo of `field` (1 <= depth <=
 * the deepest halo the grid supports, >= 2) receives the neighbours' owned
 * cells, edges and corners, from all 8 neighbours; ghost cells on physical
 * sides are not touched.  MISOR_P is the current pressure buffer.  With one
 * rank it does nothing.  The solve and the NS steps exchange internally;
 * this entry point is the skeleton's own call (and its printExchange check). */
int misor_exchange(misor_grid* g, int field, int depth);
/* number of visible GPUs (host programs map rank -> device) */
int misor_device_count(int* n);
/* ranks of the grid's communicator as its transport counts them: ncclCommCount
 * of the RCCL communicator (MPI_Comm_size of the reference's solver->comm,
 * assignment-5/skeleton/src/solver.c:408,452), the member count of an
 * in-process group, 1 for a single-rank grid */
int misor_comm_ranks(const misor_grid* g, int* n);
/* fill a field (incl. ghosts) with a constant; initSolver of NS (solver.c:92-99) */
int misor_fill(misor_grid* g, int field, double value);

/* initSolver of assignment-4 (solver.c:99-123): p = sin(4 pi i dx) +
 * sin(4 pi j dy), rhs = sin(2 pi i dx) for problem 2 else 0, incl. ghosts.
 * The 1-D sine tables are evaluated on the host with libm exactly as the
 * reference does, so the fields are bit-identical to it. */
int misor_poisson_init(misor_grid* g, double xlength, double ylength, int problem);

/* solveRB / solveRBA (assignment-4/src/solver.c:179-299): red-black SOR
 * with Neumann ghost copy after each iteration, until res < eps^2 or itermax.
 * *iters = iterations done (the reference prints it, :237), *res = final
 * residual (sum r^2 / (imax*jmax)).  Either output may be NULL.
 * Decomposed: as the reference's MPI loop (assignment-5/skeleton/src/
 * solver.c:603-607, an exchange opens every iteration) the solve leaves the
 * final field's inter-rank halo to its next reader: misor_adapt_uv and a
 * misor_download of MISOR_P exchange it first (2 deep), the next solve at its
 * start; misor_gather reads owned cells only. */
int misor_solve_rb(misor_grid* g, int* iters, double* res);
/* the same with an explicit cap that overrides desc.itermax for this call */
int misor_solve_rb_n(misor_grid* g, int itermax, int* iters, double* res);
/* The reference's lexicographic Gauss-Seidel SOR `solve` (what its programs
 * call): assignment-4/src/solver.c:126-177 (xorder = MISOR_LEX_A4) and
 * assignment-5/sequential/src/solver.c:140-191 (xorder = MISOR_LEX_SEQ; the
 * two differ only in the order of the stencil terms), bit for bit, as an
 * anti-diagonal wavefront: in one workgroup on grids below 512^2 cells (all
 * the reference's .par grids), as a wavefront of tiles over the whole device
 * from there on (MISOR_TUNE_LEX_TILED and the keys after it).  p and the
 * iteration count never depend on the form; res may differ in its last bits
 * between the two forms and between tile sizes, because r^2 is summed in
 * another order (for one form and tile size it is the same bits on every
 * run).  Single rank, variant RB only.  MISOR_EHIP "wavefront stalled": a
 * bounded wait inside the tiled launch gave up; p is then undefined. */
enum { MISOR_LEX_A4 = 0, MISOR_LEX_SEQ = 1 };
int misor_solve_lex(misor_grid* g, int xorder, int* iters, double* res);

/* ------------------------------------------------------------ multigrid ---
 * Geometric multigrid V-cycles for the same problem (lap p = rhs, Neumann by
 * ghost copy), cell-centred, with the red-black iteration of misor_solve_rb as
 * smoother and as coarsest-level solver (DESIGN.md "Geometric multigrid" has
 * the full definition).  misor_solve_mg is the single-rank form, misor_solve_mg_dist
 * below it cycles a decomposed grid; variant RB only.
 *
 * Levels: level 0 is the grid; level l+1 has (imax/2, jmax/2) cells of
 * (2dx, 2dy).  Coarsening stops at the first level with an odd side, a side
 * below 4, or imax*jmax <= coarse_cells: that level is the coarsest.  A grid
 * that cannot be coarsened has one level and its cycle is the coarsest solve.
 *
 * One cycle on a level that is not the coarsest: nu1 solveRB iterations with
 * omega_smooth (no early exit); r = rhs - lap p; rc = the mean of r over each
 * coarse cell's four fine cells; e = 0; one cycle on the next level for
 * lap e = rc; p += the bilinear interpolation of e (weights 9, 3, 3, 1 over
 * 16, coarse neighbours mirrored at the boundary), then p's ghost copy; nu2
 * iterations.  The coarsest level runs solveRB with omega_coarse, eps_coarse
 * and itermax_coarse.
 *
 * misor_solve_mg runs cycles while res >= eps^2 (desc.eps) and fewer than
 * maxcycles are done; res is solveRB's own residual as the last smoothing
 * iteration on level 0 reports it (post-smoothing; pre-smoothing when nu2 =
 * 0; the coarsest solve's on a one-level hierarchy), 1.0 before the first
 * cycle.  desc.omega and desc.itermax are not used, and a later
 * misor_solve_rb of the grid is what it would have been without this call.
 * The hierarchy is built by the first call, rebuilt when coarse_cells
 * changes and freed by misor_destroy.  The levels' solves test their loops as
 * the grid's own do (MISOR_TUNE_NEAR_BAND of the grid holds on every level).
 *
 * The tail of the hierarchy -- its trailing levels that each fit the LDS of one
 * workgroup, misor_mg_tail -- is cycled by one launch a cycle instead of two
 * solves a level, and a grid that itself fits is solved, loop over the cycles
 * included, in one launch (MISOR_TUNE_MG_TAIL; the same bits either way). */
typedef struct {
    int nu1, nu2;           /* pre- / post-smoothing iterations; nu1 + nu2 >= 1 */
    double omega_smooth;    /* relaxation factor of the smoothing iterations */
    int coarse_cells;       /* a level of at most this many cells is not coarsened */
    double omega_coarse, eps_coarse;  /* the coarsest level's solveRB ... */
    int itermax_coarse;               /* ... and its cap */
    int maxcycles;
} misor_mg_params;
/* nu1 = nu2 = 2, omega_smooth 1.0, coarse_cells 64, omega_coarse 1.7,
 * eps_coarse 0.1 * desc.eps, itermax_coarse 1000, maxcycles 100 */
int misor_mg_default_params(const misor_grid* g, misor_mg_params* out);
/* host-only: the levels of an imax x jmax grid.  *nlevels = their number;
 * shapes (2 * cap ints, may be NULL with cap 0) receives {imax, jmax} of the
 * first min(cap, *nlevels) levels.  MISOR_EINVAL: a side below 2, a negative
 * coarse_cells or cap, a null nlevels */
int misor_mg_levels(int imax, int jmax, int coarse_cells, int* nlevels, int* shapes, int cap);
/* host-only: the tail of the hierarchy misor_mg_levels gives for these
 * arguments -- its maximal run of trailing levels that each fit the LDS of one
 * workgroup (the rule of MISOR_TUNE_SMALL_SOLVE: (imax+2)(jmax+2) doubles and
 * 256 bytes within 160 KB, and at most 8192 cell pairs jmax * ceil(imax/2)).
 * *first = index of the first level held in LDS, *count = levels in the tail
 * (0: none fits, then *first = nlevels).  A tail of two or more levels is
 * cycled by one kernel launch a cycle, one workgroup walking the levels down
 * and up in LDS; where *first = 0 the whole misor_solve_mg is one launch and
 * one read-back of its state (MISOR_TUNE_MG_TAIL).  Same MISOR_EINVAL cases as
 * misor_mg_levels, and a null first or count. */
int misor_mg_tail(int imax, int jmax, int coarse_cells, int* first, int* count);
/* prm NULL: the defaults.  cycles and res may be NULL.  Found before any
 * device call, in this order: MISOR_EINVAL for a negative nu1 or nu2,
 * nu1 + nu2 < 1, omega_smooth or omega_coarse not > 0, a negative
 * coarse_cells, itermax_coarse, maxcycles, a null grid, variant RBA; then
 * MISOR_ESTATE for a decomposed grid */
int misor_solve_mg(misor_grid* g, const misor_mg_params* prm, int* cycles, double* res);

/* The same cycle on a decomposed grid: collective over the ranks of g; with one
 * rank (a grid that is not decomposed) it is misor_solve_mg.  Levels, smoothing,
 * residual, restriction, interpolation weights, ghost copy, res and the loop
 * over the cycles are those defined above, and p is bit for bit the
 * single-rank misor_solve_mg's on every partition.
 *
 * The first levels of the hierarchy stay distributed: level 0 always; level
 * l >= 1 iff level l-1 is, every rank's block of level l-1 has even sides, the
 * halved blocks have both sides >= 4 and more than gather_cells cells
 * (gather_cells < 0: the default, 65536), and level l is the coarsest level or
 * has even block sides again.  A distributed level is a decomposed grid on the
 * same process grid (the halved blocks are misor_decompose of the halved
 * grid), smoothed -- or, as the coarsest level, solved -- by the decomposed
 * red-black iteration.  The remaining levels are gathered: every rank holds
 * them whole.  At the hand-over the ranks' restricted blocks are all-gathered
 * into the whole-domain rhs and every rank runs the single-rank cycle on the
 * gathered levels redundantly (the same bits everywhere, nothing is sent
 * back); the correction reads the rank's window of the whole-domain e.
 *
 * res is level 0's all-reduced residual as misor_solve_rb_n returns it on a
 * decomposed grid, the same bits on every rank, so all ranks run the same
 * number of cycles.  It can differ from the single-rank res in its last bits,
 * as misor_solve_rb's does outside the near band (MISOR_TUNE_NEAR_BAND): the
 * cycle count is the single-rank one except where res lands within those bits
 * of eps^2.
 *
 * Found before any device or collective call, by every rank from the same
 * arithmetic: misor_solve_mg's MISOR_EINVAL cases in its order; then
 * MISOR_ESTATE for a hierarchy of two or more levels on level-0 blocks with an
 * odd side.  A later misor_solve_rb of the grid is unaffected. */
int misor_solve_mg_dist(misor_grid* g, const misor_mg_params* prm, int gather_cells,
                        int* cycles, double* res);
/* host-only: how misor_solve_mg_dist splits the hierarchy of an imax x jmax grid
 * over nranks (dims_in as misor_decompose): *nlevels = misor_mg_levels' count,
 * the first *ndist of them distributed.  MISOR_EINVAL: misor_decompose's and
 * misor_mg_levels' cases, a null nlevels or ndist; MISOR_ESTATE: the refusal
 * above.  The outputs are untouched on an error. */
int misor_mg_dist_levels(int nranks, const int dims_in[2], int imax, int jmax,
                         int coarse_cells, int gather_cells, int* nlevels, int* ndist);

/* NS step kernels (assignment-5/sequential/src/solver.c) */
int misor_ns_setup(misor_grid* g, const misor_ns_desc* ns);
int misor_compute_timestep(misor_grid* g, double dt_bound, double tau, double* dt_out); /* :219-234 */
int misor_set_dt(misor_grid* g, double dt);
int misor_set_boundary_conditions(misor_grid* g);          /* :236-337 */
int misor_set_special_boundary_condition(misor_grid* g);   /* :339-358 */
int misor_compute_fg(misor_grid* g);                        /* :360-436 */
int misor_compute_rhs(misor_grid* g);                       /* :122-138 */
int misor_normalize_pressure(misor_grid* g);                /* :204-217 */
int misor_adapt_uv(misor_grid* g);                          /* :438-455 */
/* max |u| and max |v| over all cells incl. ghosts (maxElement, :193-202) */
int misor_max_uv(misor_grid* g, double* umax, double* vmax);

/* launch-geometry knobs of the sweep kernel (defaults chosen by measurement,
 * DESIGN.md); results are bit-identical for every setting */
enum {
    MISOR_TUNE_SWEEP_VARIANT = 1,  /* 0..14 (default 7), an index into kSweepVariants
                                    * (csrc/misor_internal.h): 4, 8 or 16 strips per
                                    * workgroup x 1..3 rows in flight x non-temporal
                                    * stores / loads; anything else is MISOR_EINVAL */
    MISOR_TUNE_ROWS_PER_BLOCK = 2, /* rows one workgroup marches; <= 0: automatic */
    MISOR_TUNE_XCD_REMAP = 3,      /* 1: adjacent blocks on one XCD (shared L2 halos) */
    MISOR_TUNE_SMALL_SOLVE = 4,    /* 1 (default): whole solve in one workgroup, p in LDS,
                                    * when the grid fits (single rank, <= 128^2 cells) */
    MISOR_TUNE_OVERLAP = 5,        /* decomposed: 1 (default) = halo exchange and residual
                                    * all-reduce on a second stream, overlapped with the
                                    * interior blocks of the sweep; 0 = serial */
    MISOR_TUNE_TSTEPS = 6,         /* iterations per pass over HBM, 1..12: 1 = single-
                                    * iteration sweep kernel, T >= 2 = temporally blocked
                                    * kernel (T iterations per read of p and rhs); the
                                    * iteration count and every bit of p are unchanged.
                                    * A request binds every pass to T (no short pass
                                    * plan); <= 0 returns to the default rule */
    MISOR_TUNE_TB_VARIANT = 7,     /* temporally blocked kernel: 0..4 strips per workgroup x
                                    * rows in flight */
    MISOR_TUNE_TB_ROWS = 8,        /* temporally blocked kernel: rows per block; <= 0: auto
                                    * (a multiple of the kernel's rhs ring) */
    MISOR_TUNE_TB_PERSISTENT = 9,  /* temporally blocked kernel: 1 (default) = as many
                                    * workgroups as are resident, taking blocks from per-XCD
                                    * work queues; 0 = one workgroup per block */
    MISOR_TUNE_NS_FUSE = 10,       /* 1 (default): misor_compute_fg also computes RHS in the
                                    * same pass over u, v (computeRHS then only completes the
                                    * cells next to a neighbour rank); 0 = separate kernels */
    MISOR_TUNE_FINISH2 = 11,       /* single rank: 1 (default) = two-level loop test
                                    * (partial sums, then the test); 0 = one kernel */
    MISOR_TUNE_TB_RESERVE = 12,    /* decomposed, overlapped: workgroup slots the persistent
                                    * interior launch leaves to the exchange / all-reduce /
                                    * edge-block streams (default 16) */
    MISOR_TUNE_TB_CHAIN = 13,      /* temporally blocked kernel, persistent, default variant:
                                    * 1 = chained vertical runs of short blocks with work
                                    * stealing (no warm-up rows between the blocks of a
                                    * run); 0 = one block per work item; -1 (default) =
                                    * chained on local blocks below 2^28 cells.  Get: 1 if
                                    * chained passes are in effect */
    MISOR_TUNE_NEAR_BAND = 14      /* solveRB's loop test near its threshold: when an
                                    * iteration's res lies within a relative 10^-value of
                                    * eps^2, that iteration and the rest of the solve are
                                    * recomputed one sweep at a time with an exact
                                    * (order-independent) sum of r^2, so the iteration count
                                    * and res do not depend on the partition.  Default 10;
                                    * >= 300: off (set by tests to force the path: -30) */,
    MISOR_TUNE_RES_LITE = 15,      /* 10-iteration split-ring passes, one rank or
                                    * decomposed: 1 (default) = the steady chunks count the
                                    * residual of a pass's iterations but its last on one
                                    * row in S, a lower bound that the loop test accepts
                                    * only where it proves the loop goes on (not converged,
                                    * not near the threshold; decomposed: the all-reduced
                                    * sum of the ranks' bounds decides); otherwise the pass
                                    * is redone counting every cell and the solve continues
                                    * so.  The iteration count, res and p are the same bits
                                    * either way.  0 = every iteration counted in full */
    MISOR_TUNE_EDGE_STEAL = 16     /* whole passes of the split ring (TB variant 13): 1
                                    * (default) = the edge kernel's workgroups, their own
                                    * list done, steal runs of 4 or more blocks from the
                                    * main kernel's list while it runs; 0 = they never
                                    * steal; 2 (diagnostics) = the main kernel is launched
                                    * in stream order behind the edge kernel, which so
                                    * splits every main segment down to fewer than 4
                                    * unclaimed blocks before the main kernel starts (the
                                    * steals forced, for tests).  p and res are the same
                                    * bits for every value */,
    MISOR_TUNE_LEX_TILED = 17,     /* misor_solve_lex: -1 (default) = the automatic rule
                                    * (the tiled wavefront from 512^2 interior cells on,
                                    * where it measured faster; the one-workgroup kernel
                                    * below, and always when p fits in its LDS);
                                    * 0 = always the one-workgroup kernel; 1 = always
                                    * tiled, also on grids that fit in LDS and on a grid of
                                    * one tile.  Get: 1 if the next misor_solve_lex of this
                                    * grid would run tiled.  p and the iteration count are
                                    * the same bits for every value */
    MISOR_TUNE_LEX_TILE_W = 18,    /* tiled lexicographic solve: tile width in cells ... */
    MISOR_TUNE_LEX_TILE_H = 19,    /* ... and height (defaults 96 x 96).  Sides from 8 up
                                    * to what LDS holds (tile + one-cell halo + the tile's
                                    * rhs within 160 KB: 96 x 96, 128 x 64 fit); <= 0 returns
                                    * to the default; a pair that does not fit is
                                    * MISOR_EINVAL and changes nothing.  p and the
                                    * iteration count are the same bits for every value */
    MISOR_TUNE_LEX_WGS = 20        /* tiled lexicographic solve: workgroups of its
                                    * persistent grid (at most one per tile); <= 0
                                    * (default) = automatic: at most the tiles of the
                                    * longest tile anti-diagonal and at most what the device
                                    * holds resident.  Progress needs no residency: 1
                                    * runs the tiles one after the other.  p and the
                                    * iteration count are the same bits for every value
                                    * (res too) */,
    MISOR_TUNE_MG_TAIL = 21        /* misor_solve_mg: 1 (default) = the tail of the
                                    * hierarchy (misor_mg_tail) is cycled in one launch
                                    * when it has two or more levels; 0 = every level by
                                    * its own launches.  Get returns the setting.  p, the
                                    * cycle count and res are the same bits for either
                                    * value */
};
int misor_set_tuning(misor_grid* g, int key, int value);
int misor_get_tuning(const misor_grid* g, int key, int* value);

/* diagnostics: with MISOR_CHAIN_TRACE=1 in the environment when the grid is
 * configured, the per-block timeline of the last chained pass (3 words per
 * block L = by * nbx + bx: start and end on the 100 MHz wall clock, workgroup
 * | 1 << 32 for the first block of a run | 1 << 33 for a block run by the
 * edge kernel, whose workgroups are numbered from 0 like the main kernel's);
 * *n = words available */
int misor_chain_trace(misor_grid* g, unsigned long long* out, long long cap, long long* n);

int misor_enable_timing(misor_grid* g, int on);
int misor_get_stats(const misor_grid* g, misor_stats* out);
int misor_reset_stats(misor_grid* g);

/* --------------------------------------------------------------- batch ---
 * Many small Poisson problems of ONE shape solved in one launch: nbatch
 * independent members, each with its own p, rhs, omega, eps and itermax, one
 * workgroup per member with its p resident in LDS (the whole-solve kernel of
 * MISOR_TUNE_SMALL_SOLVE; the relaxation-factor study around poisson.par's
 * omg, a sweep over eps, many right-hand sides on one mesh).  Single rank.
 *
 * Contract
 *  - For every member m, p, iters[m] and res[m] are the same bits as
 *    misor_solve_rb gives on a single-rank misor_grid of that shape with
 *    member m's omega, eps, itermax, p and rhs, at the same
 *    MISOR_TUNE_NEAR_BAND.  (A member whose residual comes within the near
 *    band of eps^2 is finished through that very path on an internal grid.)
 *  - Members are independent: one member's convergence, cap or data never
 *    affects another.
 *  - The batch holds LDS-resident problems only: a shape the whole-solve
 *    kernel does not hold (more than 128^2 cells) is MISOR_EINVAL; use
 *    misor_create for those.  imax or jmax of 1 is accepted; misor_create
 *    has no such grid, so there the batch's own fixed-order residual sum
 *    decides the loop test and MISOR_TUNE_NEAR_BAND has no effect.
 *  - Argument errors (below) are found before any device call.  The device
 *    is first touched, and its memory allocated, by the first call that moves
 *    or computes data, which may so return MISOR_EHIP / MISOR_ENOMEM. */
typedef struct misor_batch misor_batch;

typedef struct {
    int imax, jmax;      /* one shape for the whole batch */
    double dx, dy;
    int nbatch;          /* >= 1 */
    int variant;         /* MISOR_SOLVE_RB / MISOR_SOLVE_RBA, whole batch */
    int device;          /* -1: current */
} misor_batch_desc;

/* MISOR_EINVAL: a null pointer, imax or jmax < 1, dx or dy <= 0, nbatch < 1,
 * an unknown variant, a shape that does not fit in LDS */
int misor_batch_create(misor_batch** out, const misor_batch_desc* d);
void misor_batch_destroy(misor_batch* b);
/* per-member SOR parameters, arrays of nbatch; a NULL array keeps what is set.
 * Defaults after create: omega 1.0, eps 0.0, itermax 0 */
int misor_batch_set_params(misor_batch* b, const double* omega, const double* eps,
                           const int* itermax);
/* field = MISOR_P or MISOR_RHS; member in [0, nbatch) moves one (imax+2)(jmax+2)
 * array in the reference layout; member = -1 moves nbatch of them, contiguous.
 * MISOR_EINVAL: null pointer, another field, a member out of range */
int misor_batch_upload(misor_batch* b, int field, int member, const double* host);
int misor_batch_download(misor_batch* b, int field, int member, double* host);
/* assignment-4 initSolver fields into every member (as misor_poisson_init) */
int misor_batch_poisson_init(misor_batch* b, double xlength, double ylength, int problem);
/* solveRB / solveRBA on every member; iters / res: arrays of nbatch, either may be NULL */
int misor_batch_solve_rb(misor_batch* b, int* iters, double* res);
/* stream the batch's kernel runs on (hipStream_t as void*); NULL = own stream */
int misor_batch_set_stream(misor_batch* b, void* hip_stream);
/* MISOR_TUNE_NEAR_BAND only (as on a grid); any other key is MISOR_EINVAL */
int misor_batch_set_tuning(misor_batch* b, int key, int value);
int misor_batch_get_tuning(const misor_batch* b, int key, int* value);

/* ------------------------------------------------------------------ 3D ---
 * assignment-6's 3D Navier-Stokes solver (assignment-6/src/solver.c) on one
 * GPU: the same step as solver.h's computeTimestep / setBoundaryConditions /
 * setSpecialBoundaryCondition / computeFG / computeRHS / solve / adaptUV, with
 * a 7-point red-black pressure solve.  Fields keep the reference layout:
 * (imax+2)(jmax+2)(kmax+2) doubles, i fastest, then j, then k (solver.c:19-34).
 * Every cell value is bit-identical to the reference's; the solve's residual
 * is summed in a fixed tree order (the reference sums sequentially). */
typedef struct misor_grid3 misor_grid3;

typedef struct {
    int imax, jmax, kmax;               /* interior cells */
    double xlength, ylength, zlength;   /* domain size */
    double re, gamma, tau, omega, eps;  /* Reynolds number, upwind factor, CFL
                                         * safety, SOR relaxation, tolerance */
    double gx, gy, gz;                  /* body force */
    int itermax;                        /* solve iteration cap */
    int bcTop, bcBottom, bcLeft, bcRight, bcFront, bcBack; /* MISOR_NOSLIP ... */
    int problem;                        /* MISOR_PROBLEM_* */
    int device;                         /* HIP device; < 0: the current one */
    /* decomposition: slabs of planes along k (misor3_decompose); nranks <= 1 =
     * one GPU.  comm_id as misor_desc.comm_id (RCCL id from
     * misor_comm_unique_id, or "LOCAL:<name>" for ranks as host threads) */
    int nranks, rank;
    const void* comm_id;
} misor3_desc;

/* field ids of misor3_upload / misor3_download / misor3_fill */
enum { MISOR3_P = 0, MISOR3_RHS = 1, MISOR3_U = 2, MISOR3_V = 3, MISOR3_W = 4,
       MISOR3_F = 5, MISOR3_G = 6, MISOR3_H = 7 };

/* the slab of `rank`: kloc planes from global plane koff+1 (sizeOfRank rule,
 * assignment-6/src/comm.c:24-101, along k only); at least 2 planes per rank.
 * The reference splits over a 3D process grid; see DESIGN.md 6b.  host-only */
int misor3_decompose(int nranks, int rank, int kmax, int* kloc, int* koff);
/* initSolver (solver.c:60-143): device fields, all zero; dx = xlength/imax ...
 * Decomposed grids hold their slab: local arrays (imax+2)(jmax+2)(kloc+2) */
int misor3_create(misor_grid3** out, const misor3_desc* d);
int misor3_local_info(const misor_grid3* g, int* kloc, int* koff);
void misor3_destroy(misor_grid3* g);
/* whole field incl. ghosts, (imax+2)(jmax+2)(kmax+2) doubles */
int misor3_upload(misor_grid3* g, int field, const double* host);
int misor3_download(misor_grid3* g, int field, double* host);
int misor3_fill(misor_grid3* g, int field, double value);
/* commCollectResult's gather (assignment-6/src/comm.c:246-384) of a whole
 * field, collective: rank 0 receives (imax+2)(jmax+2)(kmax+2) doubles, the
 * other ranks pass NULL.  One rank: misor3_download */
int misor3_gather(misor_grid3* g, int field, double* host_global);
int misor3_set_dt(misor_grid3* g, double dt);
/* computeTimestep (solver.c:340-362): dt = tau * min(dtBound, dx/umax, dy/vmax,
 * dz/wmax), dtBound = 0.5*re/(1/dx^2+1/dy^2+1/dz^2) (solver.c:136-139) */
int misor3_compute_timestep(misor_grid3* g, double* dt_out);
/* max |u|, |v|, |w| over every cell incl. ghosts (maxElement, solver.c:299-310) */
int misor3_max_uvw(misor_grid3* g, double* mx3);
int misor3_set_boundary_conditions(misor_grid3* g);       /* solver.c:364-577 */
int misor3_set_special_boundary_condition(misor_grid3* g); /* solver.c:579-604 */
int misor3_compute_fg(misor_grid3* g);                    /* solver.c:606-824 */
int misor3_compute_rhs(misor_grid3* g);                   /* solver.c:145-173 */
/* solve (solver.c:175-297): red-black SOR until res < eps^2 or itermax;
 * decomposed: halos and the residual sum cross the ranks, p and the
 * iteration count are those of the single-domain solve */
int misor3_solve(misor_grid3* g, int* iters, double* res);
int misor3_adapt_uvw(misor_grid3* g);                     /* solver.c:826-853 */
int misor3_normalize_pressure(misor_grid3* g);            /* solver.c:312-338 */
int misor3_synchronize(misor_grid3* g);
/* device time of the solves (HIP events on the grid's stream around each
 * misor3_solve: its colour-pass and loop-test kernels), accumulated while
 * timing is on; enabling resets the counters */
int misor3_enable_timing(misor_grid3* g, int on);
/* launch-geometry knobs of the 3D solve; results are bit-identical for every
 * setting */
enum {
    MISOR3_TUNE_SWEEP = 1,  /* 1 (default): one fused red+black sweep launch per iteration
                             * (k-march, LDS plane ring, ping-pong p); 0: two colour-pass
                             * launches, in place */
    MISOR3_TUNE_ROWS = 2,   /* fused sweep: rows per workgroup tile, 4 / 8 / 12 */
    MISOR3_TUNE_KCHUNK = 3, /* fused sweep: planes per workgroup (>= 4; 0: automatic) */
    MISOR3_TUNE_FOLD = 4,   /* single rank, fused sweep: 1 (default) = each sweep launch first
                             * applies the previous sweep's loop test (one launch per
                             * iteration); 0 = a finish kernel after every sweep */
    MISOR3_TUNE_RHS_AHEAD = 5, /* fused sweep: plane steps between an rhs load and its first
                                * use, 1 or 2; 0 (default) = 2 on marches of >= 16 planes */
    MISOR3_TUNE_RESIDENT = 6  /* single rank: the whole solve in one cooperative launch with
                               * p resident in LDS (boxes of 32x16x16 cells, grid barriers
                               * between the colour passes) when the grid fits the device
                               * (128^3 on 256 CUs); 1 / -1 (default) = when it fits, 0 = never.
                               * misor3_get_tuning returns whether the next solve uses it */
};
int misor3_set_tuning(misor_grid3* g, int key, int value);
int misor3_get_tuning(const misor_grid3* g, int key, int* value);
int misor3_get_solve_time(const misor_grid3* g, double* ms, long long* iters);

/* --- 3D multigrid: the V-cycle of misor_solve_mg above for lap p = rhs on one
 * misor_grid3 (DESIGN.md "Geometric multigrid, 3D" has the full definition).
 * Neumann by misor3_solve's ghost copy (faces only); smoother and coarsest
 * solver are misor3_solve's red-black iteration.  misor3_solve_mg is the
 * single-rank form, misor3_solve_mg_dist below the one for slabs.
 *
 * Levels: level l+1 has (imax/2, jmax/2, kmax/2) cells of (2dx, 2dy, 2dz);
 * the coarsest is the first with an odd side, a side below 4, or
 * imax*jmax*kmax <= coarse_cells.
 *
 * A cycle on a level that is not the coarsest: nu1 iterations with
 * omega_smooth (no early exit); r = rhs - lap p in the solve's own expression;
 * rc = the mean of r over a coarse cell's eight fine cells; e = 0; a cycle on
 * the next level for lap e = rc; p += the trilinear interpolation of e
 * (weights 27, 9, 3, 1 over 64, coarse neighbours mirrored at the boundary),
 * then p's ghost copy; nu2 iterations.  The coarsest level runs the solve's
 * loop with omega_coarse, eps_coarse, itermax_coarse, its residual carry
 * seeded with 1.0 like misor3_solve's.  The reference carries res from one
 * iteration into the next (res <- (res + sum r^2) / N), so nu iterations
 * seeded with 1.0 cannot report less than N^-nu: smoothing calls seed the
 * carry with 0.0.
 *
 * misor3_solve_mg runs cycles while res >= eps^2 (desc.eps) and fewer than
 * maxcycles are done; res is what the last smoothing call on level 0 leaves
 * (post-smoothing; pre-smoothing when nu2 = 0; the coarsest solve's on a
 * one-level hierarchy), 1.0 before the first cycle.  desc.omega and
 * desc.itermax are not used, and a later misor3_solve is what it would have
 * been without this call.  The MISOR3_TUNE_* knobs apply to level 0 only.  The
 * hierarchy is built by the first call, rebuilt when coarse_cells changes and
 * freed by misor3_destroy. */
/* nu1 = nu2 = 2, omega_smooth 1.0, coarse_cells 512, omega_coarse 1.7,
 * eps_coarse 0.1 * desc.eps, itermax_coarse 1000, maxcycles 100 */
int misor3_mg_default_params(const misor_grid3* g, misor_mg_params* out);
/* host-only: the levels of an imax x jmax x kmax grid.  *nlevels = their
 * number; shapes (3 * cap ints, may be NULL with cap 0) receives {imax, jmax,
 * kmax} of the first min(cap, *nlevels) levels.  MISOR_EINVAL: a side below 2,
 * a negative coarse_cells or cap, a null nlevels */
int misor3_mg_levels(int imax, int jmax, int kmax, int coarse_cells, int* nlevels, int* shapes,
                     int cap);
/* prm NULL: the defaults.  cycles and res may be NULL.  Found before any
 * device call, in this order: MISOR_EINVAL for bad parameters (as
 * misor_solve_mg's) or a null grid; then MISOR_ESTATE for a decomposed grid,
 * slabs or Cartesian */
int misor3_solve_mg(misor_grid3* g, const misor_mg_params* prm, int* cycles, double* res);
/* the last misor3_solve_mg of this grid: cycles run and levels of its
 * hierarchy; while misor3_enable_timing is on, the device time of level 0's
 * two transfer kernels ([0] residual + restriction, [1] prolongation +
 * correction + ghost copy) and the launches it covers, summed since timing was
 * enabled (level 0's smoothing is in misor3_get_solve_time) */
typedef struct {
    int cycles, levels;
    double transfer_ms[2];
    long long transfers;
    /* the levels the last multigrid solve kept distributed over the ranks
     * (misor3_mg_dist_levels' ndist); 0 after misor3_solve_mg and on a grid that
     * is not decomposed */
    int dist_levels;
} misor3_mg_info;
int misor3_get_mg_info(const misor_grid3* g, misor3_mg_info* out);

/* The same cycle on a grid decomposed into slabs (misor3_create with nranks >
 * 1): collective over the ranks of g; with one rank it is misor3_solve_mg, the
 * same bits and the same misor3_mg_info.  Levels, smoothing, residual,
 * restriction, trilinear weights, ghost copy, res and the loop over the cycles
 * are those defined above, and p is bit for bit the single-rank
 * misor3_solve_mg's for every slab count.  p's 2-deep halo is left current, as
 * misor3_solve leaves it, and a later misor3_solve of the grid is what it would
 * have been without this call.
 *
 * The first levels of the hierarchy stay distributed: level 0 always; level
 * l >= 1 iff level l-1 is, every slab of level l-1 has an even number of
 * planes, the halved slabs have at least 4 planes and more than gather_cells
 * cells (imax_l * jmax_l * kloc_l; gather_cells < 0: the default, 2097152, the
 * fastest value measured, DESIGN.md "Geometric multigrid, 3D, decomposed"),
 * and level l is the coarsest level or its slabs have even plane counts again.
 * "Every slab even" means nranks divides the level's kmax with an even
 * quotient, so the slabs of a distributed level are equal and are
 * misor3_decompose of the halved grid.  A distributed level is smoothed -- or,
 * as the coarsest level, solved -- by the slab misor3_solve.  The remaining
 * levels are gathered: every rank holds them whole.  At the hand-over the
 * ranks' restricted slabs are all-gathered into the whole-domain rhs and every
 * rank runs the single-rank cycle on the gathered levels redundantly (the same
 * bits everywhere, nothing is sent back; these levels run the streaming sweep,
 * not the resident launch); the correction reads the rank's window of the
 * whole-domain e.
 *
 * res is level 0's all-reduced residual carry as misor3_solve reports it on
 * slabs, the same bits on every rank, so all ranks run the same number of
 * cycles.  It can differ from the single-rank res in its last bits (the sum's
 * order differs): the cycle count is the single-rank one except where res
 * lands within those bits of eps^2.
 *
 * Found before any device or collective call, by every rank from the same
 * arithmetic, in this order: misor3_solve_mg's MISOR_EINVAL cases in its order;
 * MISOR_ESTATE for a Cartesian grid (misor3_create_cart); MISOR_ESTATE for a
 * hierarchy of two or more levels on level-0 slabs with an odd plane count (a
 * one-level hierarchy on odd slabs is fine: its cycle is the decomposed
 * coarsest solve).  The hierarchy is built by the first call, rebuilt when
 * coarse_cells or the split changes and freed by misor3_destroy. */
int misor3_solve_mg_dist(misor_grid3* g, const misor_mg_params* prm, int gather_cells,
                         int* cycles, double* res);
/* host-only: how misor3_solve_mg_dist splits the hierarchy of an imax x jmax x
 * kmax grid over nranks slabs: *nlevels = misor3_mg_levels' count, the first
 * *ndist of them distributed.  MISOR_EINVAL: misor3_decompose's and
 * misor3_mg_levels' cases, a null nlevels or ndist; MISOR_ESTATE: the refusal
 * above.  The outputs are untouched on an error. */
int misor3_mg_dist_levels(int nranks, int imax, int jmax, int kmax, int coarse_cells,
                          int gather_cells, int* nlevels, int* ndist);

/* --- the box over a 3D Cartesian process grid (assignment-6/src/comm.c:24-101,
 * 476-513), a second decomposition beside the slabs.  A rank owns a block of
 * {ni, nj, nk} cells; its local array is the reference's, (ni+2)(nj+2)(nk+2)
 * doubles, whose one ghost layer is the 1-deep halo on the sides that face
 * another rank. */
typedef struct {
    int n[3];            /* local interior cells {ni, nj, nk} */
    int off[3];          /* global index of local cell 0 per axis (as koff) */
    int coords[3], dims[3];            /* {x, y, z} */
    int neighbours[6];   /* left, right, bottom, top, front, back rank or -1
                          * (the reference's Direction order, comm.h:20) */
} misor3_local;

/* MPI_Dims_create(nranks, 3) + sizeOfRank per axis.  Entries of dims_in that
 * are 0 (or dims_in == NULL) are filled with the most balanced factorisation,
 * the largest factor to z, then y, then x (the reference indexes its dims
 * KDIM = 0, JDIM = 1, IDIM = 2); non-zero entries are kept, and a product
 * that is not nranks (with zeros left: does not divide it) is MISOR_EINVAL.  rank = (cz*dims[1] + cy)*dims[0] + cx
 * (MPI_Cart_create without reorder, z slowest).  Every rank owns at least 2
 * cells per axis.  host-only */
int misor3_decompose_cart(int nranks, int rank, const int dims_in[3],
                          int imax, int jmax, int kmax, misor3_local* out);
/* as misor3_create, on the process grid dims {x, y, z} ({0,0,0} or NULL:
 * automatic); nranks <= 1 is misor3_create.  On such a grid
 *  - upload / download / fill move the rank's local array, gather assembles
 *    the global field on rank 0 (owned cells plus the ghost cells on each
 *    rank's physical sides), misor3_local_info reports nk and off[2];
 *  - misor3_solve is the reference's own loop (solver.c:199-291): exchange p,
 *    colour pass 0, exchange p, colour pass 1, all-reduce and test.  p and the
 *    iteration count are those of the single-domain solve.  The solve ends
 *    with one more exchange, so p's halo holds the neighbours' final values
 *    when misor3_adapt_uvw or misor3_download reads it;
 *  - MISOR3_TUNE_SWEEP reads 0; setting it or MISOR3_TUNE_RESIDENT to 1 is
 *    MISOR_EINVAL; the other knobs are accepted and ignored. */
int misor3_create_cart(misor_grid3** out, const misor3_desc* d, const int dims[3]);
int misor3_local_info_cart(const misor_grid3* g, misor3_local* out);
/* the reference's commExchange, collective: the 1-deep halo of `field` on the
 * sides that face another rank, axis by axis (x, then y, then z), each face
 * spanning the ghost layers already filled -- so the block's edge and corner
 * ghosts arrive too.  Ghost cells on physical sides are not touched.  A no-op
 * on one rank; MISOR_ESTATE on a slab grid */
int misor3_exchange(misor_grid3* g, int field);

#ifdef __cplusplus
}
#endif
#endif
