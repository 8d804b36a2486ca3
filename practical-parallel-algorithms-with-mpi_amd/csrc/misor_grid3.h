// misor_grid3.h -- the state of a 3D grid (misor_grid3) and what the
// host units of the 3D path share: misor3d_api.hip (lifecycle, transfers, the
// Navier-Stokes step, tuning, timing), misor3_comm.hip (halo exchange,
// all-reduce and gather over RCCL or the in-process transport),
// misor3_solve.hip (misor3_solve, one function per schedule), misor3_mg.hip
// (multigrid) and misor3_mg_dist.hip (multigrid on slabs).  The decomposition
// arithmetic is in decomp3.h.
// Not part of the public ABI (include/misor.h).
#pragma once

#include <memory>
#include <vector>

#include "decomp3.h"  // kHalo: halo planes per side in storage
#include "local_group.h"
#include "misor_err.h"

constexpr int kSlack = 2;         // spare doubles before / after every buffer: the sweep's
                                  // 16-byte column-pair loads reach one past a row end
constexpr int kBufs = 9;          // the 8 fields + the ping-pong partner of P
constexpr int kAlt = 8;

struct misor_grid3;

// the multigrid levels below a grid (misor3_mg.hip, misor3_mg_dist.hip)
struct Mg3Hierarchy {
    int coarse_cells = -1;
    std::vector<misor_grid3*> lv;  // lv[0] is the user's grid (not owned)
    // timing of level 0's transfer kernels (misor3_mg_info.transfer_ms): pair k
    // is ev[2 * k] (start), ev[2 * k + 1] (stop) around a launch of kind[k]
    // (0 restriction, 1 prolongation); ev_used pairs are complete
    std::vector<hipEvent_t> ev;
    std::vector<int> kind;
    size_t ev_used = 0;
    // the decomposed form (misor3_solve_mg_dist): the distributed levels,
    // dlv[0] the user's grid (not owned), and the gathered level (null where
    // every level is distributed), whose own hierarchy holds the rest
    int dist_coarse_cells = -1, dist_ndist = -1;
    std::vector<misor_grid3*> dlv;
    misor_grid3* gath = nullptr;
};

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
    bool levels_inherit_resident = false;  // the multigrid levels built below this grid take
                               // its `resident` (the gathered level of misor3_solve_mg_dist);
                               // false: they keep the default, whatever the grid's own knob
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
    bool own_comm = true;      // false: a multigrid level on its user's grid's communicator
    char local_name[MISOR_COMM_ID_BYTES + 1] = {};  // the in-process group's name
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
    misor_grid3* peer_gath = nullptr;  // on the last distributed level of a decomposed
                                       // hierarchy: this rank's gathered level, where the
                                       // in-process all-gather of its peers finds it
};

// misor3d_api.hip
// a single-rank grid holding p, its partner and rhs only (no u, v, w, f, g,
// h), on stream s: a multigrid level
MISOR_HIDDEN int create3_level(misor_grid3** out, const misor3_desc* d, hipStream_t s);
// the same decomposed into slabs over parent's ranks (d->nranks, d->rank are
// parent's), on parent's stream and communicator -- the same ncclComm_t, not
// owned, or an in-process group of its own named from parent's group and
// `level`: a distributed multigrid level.  Collective.
MISOR_HIDDEN int create3_level_slab(misor_grid3** out, const misor3_desc* d, misor_grid3* parent,
                                    int level);

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
// The hand-over of misor3_solve_mg_dist: f is a slab grid, G the whole-domain
// single-rank grid every rank holds of the level below it, whose kmax is
// nranks equal slabs of kc planes.  Rank r's planes r kc + 1 .. (r + 1) kc of
// G's rhs, whole planes with their ghost columns and rows, go to every rank's G.
MISOR_HIDDEN int allgather_slabs3(misor_grid3* f, misor_grid3* G, int kc);

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
// `who`: the entry point named in the message
MISOR_HIDDEN int mg3_check_params(const misor_mg_params& q, const char* who);
MISOR_HIDDEN misor_mg_params mg3_default_params(const misor_grid3* g);
// nu iterations of the solve without early exit, the carry seeded with 0.0
MISOR_HIDDEN int mg3_smooth(misor_grid3* g, double omega, int nu, double* res);
// (re)build the single-rank levels below g for coarse_cells, on g's stream
MISOR_HIDDEN int mg3_ensure_hierarchy(misor_grid3* g, int coarse_cells);
// one cycle on level l of g0's single-rank hierarchy
MISOR_HIDDEN int mg3_cycle(misor_grid3* g0, const misor_mg_params& q, size_t l, double* res);
// the start (kind 0 / 1) or stop (kind < 0) event around a timed transfer
// launch of level 0; the times so far into mg_info
MISOR_HIDDEN int mg3_record_transfer(misor_grid3* g, int kind);
MISOR_HIDDEN int mg3_collect_transfer_times(misor_grid3* g);
// misor3_solve_mg past its checks, on a grid that is not decomposed
MISOR_HIDDEN int mg3_solve_single(misor_grid3* g, const misor_mg_params& q, int* cycles,
                                  double* res);
// misor3_mg_dist.hip: the levels of the decomposed form
MISOR_HIDDEN void mg3_dist_free(Mg3Hierarchy* h);
