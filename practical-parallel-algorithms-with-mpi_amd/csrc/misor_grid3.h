// misor_grid3.h -- the state of a 3D grid (misor_grid3) and what the
// host units of the 3D path share: misor3d_api.hip (lifecycle, transfers, the
// Navier-Stokes step, tuning, timing), misor3_comm.hip (halo exchange,
// all-reduce and gather over RCCL or the in-process transport),
// misor3_solve.hip (misor3_solve, one function per schedule) and misor3_mg.hip
// (multigrid).  The decomposition arithmetic is in decomp3.h.
// Not part of the public ABI (include/misor.h).
#pragma once

#include <memory>

#include "decomp3.h"  // kHalo: halo planes per side in storage
#include "local_group.h"
#include "misor_err.h"

constexpr int kSlack = 2;         // spare doubles before / after every buffer: the sweep's
                                  // 16-byte column-pair loads reach one past a row end
constexpr int kBufs = 9;          // the 8 fields + the ping-pong partner of P
constexpr int kAlt = 8;

struct Mg3Hierarchy;  // the multigrid levels below a grid (misor3_mg.hip)

struct misor_grid3 {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;    // false: a multigrid level on its user's grid's stream
    misor3_desc desc{};
    misor::G3 g{};             // this rank's slab: g.K planes, g.koff, physical flags
    long long n = 0;           // cells of the reference's local array (planes 0 .. K+1)
    long long nalloc = 0;      // cells allocated per field (planes -1 .. K+2)
    double* alloc[kBufs] = {}; // allocations: nalloc + 2*kSlack doubles
    double* mem[kBufs] = {};   // plane -1 of each buffer (alloc + kSlack)
    double* fld[kBufs] = {};   // plane-0 origins: MISOR3_P .. MISOR3_H, kAlt = P's partner
    bool alt_stale = true;     // the partner's edge/corner ghosts may differ from P's
    int sweep = 1;             // MISOR3_TUNE_SWEEP
    int rows = 8;              // MISOR3_TUNE_ROWS
    int kchunk = 0;            // MISOR3_TUNE_KCHUNK (0: automatic)
    int fold = 1;              // MISOR3_TUNE_FOLD: single rank, loop test inside the sweep
    int resident = -1;         // MISOR3_TUNE_RESIDENT: whole solve in one launch when it fits
    void* rbar = nullptr;      // its grid-barrier state and partials, uncached memory
    double* rmbox = nullptr;   // its exchange mailboxes (2 x p's layout), uncached memory
    int rhs_ahead = 0;         // MISOR3_TUNE_RHS_AHEAD: fused sweep's rhs loads 1 or 2 steps
                               // ahead; 0: 2 on marches of >= 16 planes, else 1
    double dx = 0, dy = 0, dz = 0, dt = 0, dt_bound = 0;
    double* partials = nullptr;  // per-block partial sums / maxima
    long long partials_cap = 0;
    double* out = nullptr;      // 4 doubles on the device (maxima / sum)
    double* out_host = nullptr; // pinned
    misor::DevState* st = nullptr;
    misor::DevState* st2 = nullptr;  // the folded loop test's second state buffer
    misor::DevState* st_host = nullptr;
    int last_iters = 0;
    double res_seed = 1.0;        // the residual carry a solve starts from (solver.c:196);
                                  // other than 1.0 only inside solve3_with
    bool timing = false;          // misor3_enable_timing
    hipEvent_t ev[2] = {};        // around each solve, on the grid's stream
    double solve_ms = 0;          // accumulated device time of timed solves
    long long solve_iters = 0;    // iterations of the timed solves
    // decomposition
    int nranks = 1, rank = 0, prev = -1, next = -1;
    ncclComm_t comm = nullptr;
    std::shared_ptr<LocalGroup<misor_grid3>> local;  // in-process transport; vals: 4 per rank
    double* gstage = nullptr;     // rank 0: receive staging of misor3_gather (RCCL)
    // Cartesian process grid (misor3_create_cart)
    bool cart = false;
    misor3_local loc{};
    double* hbuf = nullptr;       // staging of the x / y faces, one allocation
    double* hsend[4] = {};        // left, right, bottom, top: packed owned layer
    double* hrecv[4] = {};        // the neighbour's, before it is unpacked into the ghost layer
    double* gbuf = nullptr;       // the box this rank contributes to misor3_gather
    // multigrid (misor3_mg.hip)
    Mg3Hierarchy* mg = nullptr;
    misor3_mg_info mg_info{};     // the last misor3_solve_mg; transfer times while timing
};

// misor3d_api.hip
// a single-rank grid holding p, its partner and rhs only (no u, v, w, f, g,
// h), on stream s: a multigrid level
MISOR_HIDDEN int create3_level(misor_grid3** out, const misor3_desc* d, hipStream_t s);

inline bool dist(const misor_grid3* g) { return g->nranks > 1; }
// plane kk of buffer b
inline double* plane_ptr(misor_grid3* g, int b, int kk) {
    return g->fld[b] + (long long)kk * g->g.sxy;
}
// what a rank contributes to the global array (decomp3.h own_span), as a box
// of its local array
inline misor::Box3 own_box(const misor3_local& L) {
    const misor::Span3 x = misor::own_span(L, 0), y = misor::own_span(L, 1),
                       z = misor::own_span(L, 2);
    return {x.lo, y.lo, z.lo, x.count, y.count, z.count, L.n[0] + 2,
            (long long)(L.n[0] + 2) * (L.n[1] + 2)};
}

// misor3_comm.hip: no-ops on a single rank
// d-deep halo of buffer b of a slab grid: planes K-d+1..K to the next rank's
// 1-d..0, planes 1..d to the previous rank's K+1..K+d
MISOR_HIDDEN int exchange3(misor_grid3* g, int b, int d);
// the 1-deep halo of buffer b of a Cartesian block on the axes of `axes` (bit
// 0 x, 1 y, 2 z), in that order; an axis the process grid does not cut is
// skipped by every rank alike
MISOR_HIDDEN int exchange_cart(misor_grid3* g, int b, int axes);
// all-reduce of n <= 4 device doubles (sum or max)
MISOR_HIDDEN int allreduce3(misor_grid3* g, double* dev, int n, bool is_max);
// misor3_gather of a decomposed grid: slabs / Cartesian blocks
MISOR_HIDDEN int gather_slabs(misor_grid3* g, int field, double* host_global);
MISOR_HIDDEN int gather_cart(misor_grid3* g, int field, double* host_global);

// misor3_solve.hip
// planes a workgroup of the fused sweep marches (MISOR3_TUNE_KCHUNK = 0)
MISOR_HIDDEN int auto_kchunk(const misor::G3& g, int rows);
// misor3_solve with omega, eps, itermax and the starting residual carry
// res_seed in place of desc.omega, desc.eps, desc.itermax and 1.0; they and
// the batch-size hint are put back, so the grid's next solve is unaffected
MISOR_HIDDEN int solve3_with(misor_grid3* g, double omega, double eps, int itermax,
                             double res_seed, int* iters, double* res);

// misor3_mg.hip
MISOR_HIDDEN void mg3_free(misor_grid3* g);
