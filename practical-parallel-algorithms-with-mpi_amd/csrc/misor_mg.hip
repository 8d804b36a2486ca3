// misor_mg.hip -- geometric multigrid on top of the red-black solve
// (include/misor.h "multigrid", DESIGN.md "Geometric multigrid"): the level
// rule, the hierarchy and the V-cycle.
//
// Levels 1 .. L-1 are internal single-rank misor_grids on the user's grid's
// stream: a level's rhs field is the restricted residual rc of the level
// above, its current pressure buffer the correction e.  Smoothing and the
// coarsest solve are misor_solve_rb_n itself, run with other coefficients for
// the duration of the call (solve_with), so every level takes the kernel the
// existing rule gives its size -- temporally blocked passes, the single sweep
// or the whole-solve LDS kernel.  The only kernels of its own are the two
// transfers of mg_kernels.hip; they add no host round trip to a cycle.
//
// The tail of the hierarchy -- its trailing levels that each fit the LDS of a
// workgroup -- is cycled by ONE launch of mg_tail.hip's kernel instead, when it
// has two levels or more (MISOR_TUNE_MG_TAIL): cycle() hands the cycle to
// tail_run at the tail's first level, and where that is level 0 the loop over
// the cycles runs in the kernel too.  The bits are those of the level-by-level
// path.
//
// A decomposed grid is cycled by misor_solve_mg_dist (DESIGN.md "Geometric
// multigrid, decomposed"; the level split is mg_dist_plan.h's): its first
// levels are decomposed grids themselves, on the same process grid and the
// communicator of level 0, smoothed and solved by the same solve_with; below
// them every rank holds the whole domain -- an internal single-rank grid with
// a hierarchy of its own, cycled by cycle() redundantly on every rank after
// the restricted blocks have been all-gathered into its rhs.
//
// Every argument check precedes the first HIP call.

#include "misor_grid.h"
#include "mg_dist_plan.h"

struct MgHierarchy {
    int coarse_cells = -1;
    std::vector<misor_grid*> lv;  // lv[0] is the user's grid (not owned)
    // timing of level 0's transfer kernels (misor_stats.mg_transfer_ms): pair k
    // is ev[2 * k] (start), ev[2 * k + 1] (stop) around a launch of kind[k]
    // (0 restriction, 1 prolongation); ev_used pairs are complete
    std::vector<hipEvent_t> ev;
    std::vector<int> kind;
    size_t ev_used = 0;
    // the tail (misor_mg_tail): levels lv[tail_first ..], tail_count of them;
    // their descriptors and the launch's state on the device with a pinned host
    // mirror, and what the device holds of both (tail_up: the input fields)
    int tail_first = 0, tail_count = 0;
    MgTailLevel* tail_lv = nullptr;
    MgTailLevel* tail_lv_host = nullptr;
    MgTailState* tail_st = nullptr;
    MgTailState* tail_st_host = nullptr;
    std::vector<MgTailLevel> tail_lv_up;
    MgTailState tail_up{};
    bool tail_st_valid = false;
    // the decomposed form (misor_solve_mg_dist): the distributed levels,
    // dlv[0] the user's grid (not owned), and the first gathered level (null:
    // every level is distributed), whose own hierarchy holds the rest
    int dist_coarse_cells = -1, dist_gather_cells = -1;
    std::vector<misor_grid*> dlv;
    misor_grid* gath = nullptr;
};

namespace {

constexpr size_t kMgEventPairs = 64;  // pairs held before they are resolved

int check_params(const misor_mg_params& q) {
    if (q.nu1 < 0 || q.nu2 < 0)
        return fail(MISOR_EINVAL, "misor_solve_mg: nu1 = %d, nu2 = %d: counts must be >= 0", q.nu1,
                    q.nu2);
    if (q.nu1 + q.nu2 < 1)
        return fail(MISOR_EINVAL, "misor_solve_mg: nu1 + nu2 must be >= 1 (a cycle smooths)");
    if (!(q.omega_smooth > 0.0) || !(q.omega_coarse > 0.0))
        return fail(MISOR_EINVAL, "misor_solve_mg: omega_smooth and omega_coarse must be > 0");
    if (q.coarse_cells < 0)
        return fail(MISOR_EINVAL, "misor_solve_mg: coarse_cells = %d must be >= 0",
                    q.coarse_cells);
    if (q.itermax_coarse < 0)
        return fail(MISOR_EINVAL, "misor_solve_mg: itermax_coarse = %d must be >= 0",
                    q.itermax_coarse);
    if (q.maxcycles < 0)
        return fail(MISOR_EINVAL, "misor_solve_mg: maxcycles = %d must be >= 0", q.maxcycles);
    return MISOR_OK;
}

misor_mg_params default_params(const misor_grid* g) {
    misor_mg_params q{};
    q.nu1 = q.nu2 = 2;
    q.omega_smooth = 1.0;
    q.coarse_cells = 64;
    q.omega_coarse = 1.7;
    q.eps_coarse = 0.1 * g->desc.eps;
    q.itermax_coarse = 1000;
    q.maxcycles = 100;
    return q;
}

// solveRB on grid g with relaxation factor omega and tolerance eps instead of
// the grid's own, capped at itermax; what the solve reads of them (the update
// coefficient of both sweep geometries, desc.eps) and the batch-size hint are
// put back before returning, so the grid's next solve is unaffected.
int solve_with(misor_grid* g, double omega, double eps, int itermax, int* iters, double* res) {
    const double coef_sp = g->sp.coef, coef_tp = g->tp.coef, eps0 = g->desc.eps;
    const int last = g->last_iters;
    g->sp.coef = g->tp.coef = sor_consts(g->desc.dx, g->desc.dy, omega, g->desc.variant).coef;
    g->desc.eps = eps;
    const int rc = misor_solve_rb_n(g, itermax, iters, res);
    g->sp.coef = coef_sp;
    g->tp.coef = coef_tp;
    g->desc.eps = eps0;
    g->last_iters = last;
    return rc;
}

// nu iterations without early exit (eps 0: res < 0 never holds); *res only
// where an iteration ran
int smooth(misor_grid* g, double omega, int nu, double* res) {
    if (nu < 1) return MISOR_OK;
    int it = 0;
    return solve_with(g, omega, 0.0, nu, &it, res);
}

void free_levels(MgHierarchy* h) {
    for (size_t l = 1; l < h->lv.size(); ++l) misor_destroy(h->lv[l]);
    h->lv.clear();
    (void)hipFree(h->tail_lv);
    (void)hipFree(h->tail_st);
    (void)hipHostFree(h->tail_lv_host);
    (void)hipHostFree(h->tail_st_host);
    h->tail_lv = h->tail_lv_host = nullptr;
    h->tail_st = h->tail_st_host = nullptr;
    h->tail_lv_up.clear();
    h->tail_st_valid = false;
    h->tail_first = h->tail_count = 0;
}

void free_dist_levels(MgHierarchy* h) {
    for (size_t l = 1; l < h->dlv.size(); ++l) misor_destroy(h->dlv[l]);
    h->dlv.clear();
    misor_destroy(h->gath);
    h->gath = nullptr;
}

// first index and length of the maximal run of trailing levels that fit the
// one-workgroup LDS kernel (n levels, shape(l, &ni, &nj)); none: first = n
template <class Shape>
void tail_rule(int n, Shape shape, int* first, int* count) {
    int f = n;
    for (int l = n - 1; l >= 0; --l) {
        int ni = 0, nj = 0;
        shape(l, &ni, &nj);
        if (!small_solve_fits(ni, nj)) break;
        f = l;
    }
    *first = f;
    *count = n - f;
}

// the tail's device blocks (a tail of one level is the coarsest solve alone
// and stays on the level-by-level path: nothing to allocate)
int ensure_tail(misor_grid* g) {
    MgHierarchy* h = g->mg;
    tail_rule((int)h->lv.size(),
              [&](int l, int* ni, int* nj) {
                  *ni = h->lv[l]->desc.imax;
                  *nj = h->lv[l]->desc.jmax;
              },
              &h->tail_first, &h->tail_count);
    if (h->tail_count < 2) return MISOR_OK;
    const size_t bytes = (size_t)h->tail_count * sizeof(MgTailLevel);
    HIPCHK(hipMalloc(&h->tail_lv, bytes));
    HIPCHK(hipMalloc(&h->tail_st, sizeof(MgTailState)));
    HIPCHK(hipHostMalloc(&h->tail_lv_host, bytes));
    HIPCHK(hipHostMalloc(&h->tail_st_host, sizeof(MgTailState)));
    HIPCHK(mg_tail_prepare());
    return MISOR_OK;
}

// (re)build the levels below g for coarse_cells.  A new level comes with a
// stream of its own and is moved to g's here; misor_set_stream of g moves the
// levels along (mg_set_stream), so they never hold a stream g has given up.
int ensure_hierarchy(misor_grid* g, int coarse_cells) {
    if (!g->mg) g->mg = new MgHierarchy();
    MgHierarchy* h = g->mg;
    if (h->coarse_cells != coarse_cells || h->lv.empty()) {
        HIPCHK(hipStreamSynchronize(g->stream));
        free_levels(h);
        h->coarse_cells = coarse_cells;
        h->lv.push_back(g);
        int ni = g->desc.imax, nj = g->desc.jmax, nic = 0, njc = 0;
        double dx = g->desc.dx, dy = g->desc.dy;
        while (mg_coarsen(ni, nj, coarse_cells, &nic, &njc)) {
            misor_desc d{};
            d.imax = ni = nic;
            d.jmax = nj = njc;
            d.dx = dx = 2.0 * dx;
            d.dy = dy = 2.0 * dy;
            d.omega = 1.0;
            d.variant = MISOR_SOLVE_RB;
            d.device = g->device;
            d.nranks = 1;
            // a level holds e (both pressure buffers) and rc only
            misor_grid* c = nullptr;
            const int rc = grid_create(&c, &d, true);
            if (rc) {
                free_levels(h);
                return rc;
            }
            h->lv.push_back(c);
        }
        const int rc = ensure_tail(g);
        if (rc) {
            free_levels(h);
            return rc;
        }
    }
    for (size_t l = 1; l < h->lv.size(); ++l) {
        if (h->lv[l]->stream != g->stream) MISOR_TRY(misor_set_stream(h->lv[l], g->stream));
        // the levels' solves test their loops as the grid's own do
        // (MISOR_TUNE_NEAR_BAND), on either path
        h->lv[l]->near_rel = g->near_rel;
        h->lv[l]->near_exp = g->near_exp;
    }
    return MISOR_OK;
}

// the timed transfer launches of level 0 so far into the stats
int collect_transfer_times(misor_grid* g) {
    MgHierarchy* h = g->mg;
    if (!h->ev_used) return MISOR_OK;
    HIPCHK(hipStreamSynchronize(g->stream));
    for (size_t k = 0; k < h->ev_used; ++k) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, h->ev[2 * k], h->ev[2 * k + 1]));
        if (h->kind[k] == 2) {
            g->stats.mg_tail_ms += ms;
        } else {
            g->stats.mg_transfer_ms[h->kind[k]] += ms;
            g->stats.mg_transfers += 1;
        }
    }
    h->ev_used = 0;
    return MISOR_OK;
}

// the start (kind 0 / 1; 2: a tail launch) or stop (kind < 0) event of the next
// pair around a timed launch, recorded on the stream.  A pair counts once its stop
// is recorded: a start whose stop never came (an error in between) is reused.
int record_transfer(misor_grid* g, int kind) {
    MgHierarchy* h = g->mg;
    while (h->ev.size() < 2 * kMgEventPairs) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        h->ev.push_back(e);
    }
    h->kind.resize(kMgEventPairs);
    const bool stop = kind < 0;
    if (!stop && h->ev_used == kMgEventPairs) MISOR_TRY(collect_transfer_times(g));
    if (!stop) h->kind[h->ev_used] = kind;
    HIPCHK(hipEventRecord(h->ev[2 * h->ev_used + (stop ? 1 : 0)], g->stream));
    if (stop) ++h->ev_used;
    return MISOR_OK;
}

// The downward half of a cycle on level l (not the coarsest): pre-smoothing,
// rc into the next level's rhs, e = 0 there.  *res: solveRB's residual of the
// last smoothing iteration, untouched if none ran.
int cycle_down(misor_grid* g0, const misor_mg_params& q, size_t l, double* res) {
    MgHierarchy* h = g0->mg;
    misor_grid* f = h->lv[l];
    misor_grid* c = h->lv[l + 1];
    const bool timed = l == 0 && g0->timing;
    MISOR_TRY(smooth(f, q.omega_smooth, q.nu1, res));
    // rc = R (rhs - lap p) from the current pressure buffer, into the coarse rhs
    if (timed) MISOR_TRY(record_transfer(g0, 0));
    launch_mg_residual_restrict(g0->stream, pbuf(f, f->cur), f->fld[kRhs], c->fld[kRhs],
                                c->loc.ni, c->loc.nj, f->pitch, c->pitch, f->sp.idx2, f->sp.idy2);
    HIPCHK(hipGetLastError());
    if (timed) MISOR_TRY(record_transfer(g0, -1));
    // e = 0, ghosts included: the cells of the current buffer.  (The other
    // buffer is written whole -- interior and ghosts -- by the first pass that
    // uses it; corners and padding are zero in both and never written.)
    HIPCHK(hipMemset2DAsync(pbuf(c, c->cur) + (long long)kYOff * c->pitch + kXOff,
                            (size_t)c->pitch * sizeof(double), 0,
                            (size_t)(c->loc.ni + 2) * sizeof(double), (size_t)c->loc.nj + 2,
                            g0->stream));
    return MISOR_OK;
}

// ... and the upward half: the correction from the next level, post-smoothing
int cycle_up(misor_grid* g0, const misor_mg_params& q, size_t l, double* res) {
    MgHierarchy* h = g0->mg;
    misor_grid* f = h->lv[l];
    misor_grid* c = h->lv[l + 1];
    const bool timed = l == 0 && g0->timing;
    if (timed) MISOR_TRY(record_transfer(g0, 1));
    launch_mg_prolong_correct(g0->stream, pbuf(f, f->cur), pbuf(c, c->cur), c->loc.ni, c->loc.nj,
                              f->pitch, c->pitch);
    HIPCHK(hipGetLastError());
    if (timed) MISOR_TRY(record_transfer(g0, -1));
    return smooth(f, q.omega_smooth, q.nu2, res);
}

bool tail_fused(const misor_grid* g0) { return g0->mg_tail && g0->mg->tail_count >= 2; }

// The tail's cycles in one launch.  *n cycles are done with residual *res (of
// the tail's first level); below level 0 the launch runs one cycle, at level 0
// misor_solve_mg's loop to eps^2 = epssq and maxcycles.  Where the coarsest
// solve came near its threshold the kernel has stopped inside a cycle, its
// downward half done and e zero on the coarsest level: that cycle is finished
// level by level here -- the coarsest solve (with its exact tail) and the
// upward halves -- and counted; the caller's loop goes on from there.
int tail_run(misor_grid* g0, const misor_mg_params& q, double epssq, int maxcycles, int* n,
             double* res) {
    MgHierarchy* h = g0->mg;
    const size_t first = (size_t)h->tail_first, count = (size_t)h->tail_count;
    // the descriptors: the current buffers and the coefficients of this call,
    // the same bits as solve_with gives the level's solve
    std::vector<MgTailLevel> lv(count);
    for (size_t k = 0; k < count; ++k) {
        misor_grid* f = h->lv[first + k];
        MgTailLevel& d = lv[k];
        memset(&d, 0, sizeof d);
        d.p = pbuf(f, f->cur);
        d.rhs = f->fld[kRhs];
        d.ni = f->loc.ni;
        d.nj = f->loc.nj;
        d.pitch = f->pitch;
        d.idx2 = f->sp.idx2;
        d.idy2 = f->sp.idy2;
        d.cells = (double)f->desc.imax * (double)f->desc.jmax;
        d.coef_smooth = sor_consts(f->desc.dx, f->desc.dy, q.omega_smooth, f->desc.variant).coef;
        d.coef_coarse = sor_consts(f->desc.dx, f->desc.dy, q.omega_coarse, f->desc.variant).coef;
    }
    if (h->tail_lv_up.size() != count ||
        memcmp(h->tail_lv_up.data(), lv.data(), count * sizeof(MgTailLevel)) != 0) {
        memcpy(h->tail_lv_host, lv.data(), count * sizeof(MgTailLevel));
        HIPCHK(hipMemcpyAsync(h->tail_lv, h->tail_lv_host, count * sizeof(MgTailLevel),
                              hipMemcpyHostToDevice, g0->stream));
        h->tail_lv_up = lv;
    }
    MgTailState s;
    memset(&s, 0, sizeof s);
    s.nu1 = q.nu1;
    s.nu2 = q.nu2;
    s.maxcycles = maxcycles;
    s.cycles0 = *n;
    s.itermax_coarse = q.itermax_coarse;
    s.epssq = epssq;
    s.res0 = *res;
    s.epssq_coarse = q.eps_coarse * q.eps_coarse;
    s.nband_coarse = near_band_abs(h->lv.back()->near_rel, s.epssq_coarse);
    if (!h->tail_st_valid || memcmp(&h->tail_up, &s, sizeof s) != 0) {
        *h->tail_st_host = s;
        HIPCHK(hipMemcpyAsync(h->tail_st, h->tail_st_host, sizeof s, hipMemcpyHostToDevice,
                              g0->stream));
        memcpy(&h->tail_up, &s, sizeof s);
        h->tail_st_valid = true;
    }
    if (g0->timing) MISOR_TRY(record_transfer(g0, 2));
    launch_mg_tail(g0->stream, h->tail_lv, (int)count, h->tail_st,
                   mg_tail_lds(lv[0].ni, lv[0].nj));
    HIPCHK(hipGetLastError());
    if (g0->timing) MISOR_TRY(record_transfer(g0, -1));
    HIPCHK(hipMemcpyAsync(h->tail_st_host, h->tail_st, sizeof s, hipMemcpyDeviceToHost,
                          g0->stream));
    MISOR_TRY(wait_stream(g0, g0->stream));
    const MgTailState out = *h->tail_st_host;
    g0->stats.mg_tail_levels = (int)count;
    g0->stats.mg_tail_launches += 1;
    *n = out.cycles;
    *res = out.res;
    if (!out.near) return MISOR_OK;
    double r = out.res_part, unused = 0.0;
    int it = 0;
    MISOR_TRY(solve_with(h->lv.back(), q.omega_coarse, q.eps_coarse, q.itermax_coarse, &it,
                         &unused));
    for (size_t l = h->lv.size() - 1; l-- > first;)
        MISOR_TRY(cycle_up(g0, q, l, l == first ? &r : &unused));
    g0->stats.mg_tail_fallbacks += 1;
    *n = out.cycles + 1;
    *res = r;
    return MISOR_OK;
}

// One cycle on level l; *res: solveRB's residual of the level's last smoothing
// iteration (the coarsest level: of its solve), untouched if none ran.
int cycle(misor_grid* g0, const misor_mg_params& q, size_t l, double* res) {
    MgHierarchy* h = g0->mg;
    if (tail_fused(g0) && l == (size_t)h->tail_first) {
        int n = 0;
        double r = 1.0;  // one cycle: 1 >= 0 and 0 < 1
        MISOR_TRY(tail_run(g0, q, 0.0, 1, &n, &r));
        *res = r;
        return MISOR_OK;
    }
    if (l + 1 == h->lv.size()) {
        int it = 0;
        return solve_with(h->lv[l], q.omega_coarse, q.eps_coarse, q.itermax_coarse, &it, res);
    }
    MISOR_TRY(cycle_down(g0, q, l, res));
    double rc_unused = 0.0;
    MISOR_TRY(cycle(g0, q, l + 1, &rc_unused));
    return cycle_up(g0, q, l, res);
}

// ---- the decomposed form (misor_solve_mg_dist) ----

// a level of the hierarchy of g: nic x njc cells of (dx, dy), one rank's whole
// grid (parent null) or decomposed like g on its communicator
int create_level(misor_grid* g, int nic, int njc, double dx, double dy, misor_grid* parent,
                 int level, misor_grid** out) {
    misor_desc d{};
    d.imax = nic;
    d.jmax = njc;
    d.dx = dx;
    d.dy = dy;
    d.omega = 1.0;
    d.variant = MISOR_SOLVE_RB;
    d.device = g->device;
    d.nranks = 1;
    if (parent) {
        d.nranks = g->desc.nranks;
        d.rank = g->desc.rank;
        d.dims[0] = g->loc.dims[0];
        d.dims[1] = g->loc.dims[1];
    }
    return grid_create(out, &d, true, parent, level);
}

// (re)build the levels below the decomposed grid g for plan P: collective, and
// every rank rebuilds at the same calls (the plan's arguments are the same on
// every rank).  Streams as in ensure_hierarchy.
int ensure_dist_hierarchy(misor_grid* g, int coarse_cells, int gather_cells, const MgDistPlan& P) {
    if (!g->mg) g->mg = new MgHierarchy();
    MgHierarchy* h = g->mg;
    if (h->dist_coarse_cells != coarse_cells || h->dist_gather_cells != gather_cells ||
        h->dlv.empty()) {
        HIPCHK(hipStreamSynchronize(g->stream));
        free_dist_levels(h);
        h->dist_coarse_cells = coarse_cells;
        h->dist_gather_cells = gather_cells;
        h->dlv.push_back(g);
        int ni = g->desc.imax, nj = g->desc.jmax;
        double dx = g->desc.dx, dy = g->desc.dy;
        int rc = MISOR_OK;
        for (int l = 1; l <= P.ndist && l < P.nlevels && !rc; ++l) {
            ni /= 2;
            nj /= 2;
            dx *= 2.0;
            dy *= 2.0;
            misor_grid* c = nullptr;
            const bool dist = l < P.ndist;
            rc = create_level(g, ni, nj, dx, dy, dist ? g : nullptr, l, &c);
            if (rc) break;
            if (!dist) {
                h->gath = c;
                break;
            }
            const misor_grid* f = h->dlv.back();
            h->dlv.push_back(c);
            // the halved block is the block of the halved grid (mg_dist_plan.h)
            if (2 * c->loc.ni != f->loc.ni || 2 * c->loc.nj != f->loc.nj ||
                2 * c->loc.ioff != f->loc.ioff || 2 * c->loc.joff != f->loc.joff)
                rc = fail(MISOR_ESTATE, "misor_solve_mg_dist: level %d is not the halved block", l);
        }
        if (rc) {
            free_dist_levels(h);
            return rc;
        }
    }
    for (size_t l = 1; l < h->dlv.size(); ++l) {
        misor_grid* c = h->dlv[l];
        if (c->stream != g->stream) MISOR_TRY(misor_set_stream(c, g->stream));
        c->near_rel = g->near_rel;
        c->near_exp = g->near_exp;
    }
    if (misor_grid* G = h->gath) {
        if (G->stream != g->stream) MISOR_TRY(misor_set_stream(G, g->stream));
        G->near_rel = g->near_rel;
        G->near_exp = g->near_exp;
        G->mg_tail = g->mg_tail;
        MISOR_TRY(ensure_hierarchy(G, coarse_cells));
    }
    return MISOR_OK;
}

int phys_mask(const misor_grid* f) {
    int m = 0;
    for (int k = 0; k < 4; ++k)
        if (f->loc.neighbours[k] < 0) m |= 1 << k;
    return m;
}

// One cycle on distributed level l of the decomposed grid g0; *res as cycle()'s.
int cycle_dist(misor_grid* g0, const misor_mg_params& q, size_t l, double* res) {
    MgHierarchy* h = g0->mg;
    misor_grid* f = h->dlv[l];
    const bool last = l + 1 == h->dlv.size();
    if (last && !h->gath) {  // the coarsest level, decomposed
        int it = 0;
        return solve_with(f, q.omega_coarse, q.eps_coarse, q.itermax_coarse, &it, res);
    }
    const bool timed = l == 0 && g0->timing;
    const int nic = f->loc.ni / 2, njc = f->loc.nj / 2;
    MISOR_TRY(smooth(f, q.omega_smooth, q.nu1, res));
    // the residual of a cell at a block edge reads the neighbour's p
    MISOR_TRY(p_halo(f));
    double unused = 0.0;
    if (!last) {
        misor_grid* c = h->dlv[l + 1];
        if (timed) MISOR_TRY(record_transfer(g0, 0));
        launch_mg_residual_restrict(g0->stream, pbuf(f, f->cur), f->fld[kRhs], c->fld[kRhs], nic,
                                    njc, f->pitch, c->pitch, f->sp.idx2, f->sp.idy2);
        HIPCHK(hipGetLastError());
        if (timed) MISOR_TRY(record_transfer(g0, -1));
        c->rhs_halo = 0;  // rc is new: its halo is exchanged by the level's next solve
        // e = 0 over the whole local array, the inter-rank halo included
        HIPCHK(hipMemsetAsync(pbuf(c, c->cur), 0, (size_t)c->elems * sizeof(double), g0->stream));
        c->p_stale = false;
        MISOR_TRY(cycle_dist(g0, q, l + 1, &unused));
        // the interpolation at a block edge reads the neighbours' e, corners too
        double* e = pbuf(c, c->cur);
        MISOR_TRY(exchange(c, e, 1));
        if (timed) MISOR_TRY(record_transfer(g0, 1));
        launch_mg_prolong_correct_dist(g0->stream, pbuf(f, f->cur), e, 0, phys_mask(f), nic, njc,
                                       f->pitch, c->pitch);
    } else {
        // the hand-over: my restricted block into my window of the whole-domain
        // rhs, everybody else's by the all-gather; then every rank cycles the
        // gathered levels alone, the same bits everywhere
        misor_grid* G = h->gath;
        const long long win = (long long)(f->loc.joff / 2) * G->pitch + f->loc.ioff / 2;
        if (timed) MISOR_TRY(record_transfer(g0, 0));
        launch_mg_residual_restrict(g0->stream, pbuf(f, f->cur), f->fld[kRhs],
                                    G->fld[kRhs] + win, nic, njc, f->pitch, G->pitch, f->sp.idx2,
                                    f->sp.idy2);
        HIPCHK(hipGetLastError());
        if (timed) MISOR_TRY(record_transfer(g0, -1));
        MISOR_TRY(allgather_blocks(f, G->fld[kRhs], G->pitch, nic, njc));
        HIPCHK(hipMemset2DAsync(pbuf(G, G->cur) + (long long)kYOff * G->pitch + kXOff,
                                (size_t)G->pitch * sizeof(double), 0,
                                (size_t)(G->loc.ni + 2) * sizeof(double), (size_t)G->loc.nj + 2,
                                g0->stream));
        MISOR_TRY(cycle(G, q, 0, &unused));
        if (timed) MISOR_TRY(record_transfer(g0, 1));
        launch_mg_prolong_correct_dist(g0->stream, pbuf(f, f->cur), pbuf(G, G->cur), win,
                                       phys_mask(f), nic, njc, f->pitch, G->pitch);
    }
    HIPCHK(hipGetLastError());
    if (timed) MISOR_TRY(record_transfer(g0, -1));
    f->p_stale = true;  // p changed up to the block edge: its halo is the neighbours' old p
    return smooth(f, q.omega_smooth, q.nu2, res);
}

// misor_solve_mg past its checks, on a grid that is not decomposed
int solve_mg_single(misor_grid* g, const misor_mg_params& q, int* cycles, double* res) {
    HIPCHK(hipSetDevice(g->device));
    MISOR_TRY(ensure_hierarchy(g, q.coarse_cells));
    const double epssq = g->desc.eps * g->desc.eps;
    int n = 0;
    double r = 1.0;  // as solveRB's loop (solver.c:196)
    int rc = MISOR_OK;
    g->stats.mg_tail_levels = 0;
    g->stats.mg_dist_levels = 0;
    if (tail_fused(g) && g->mg->tail_first == 0) {
        // the grid itself fits: the loop runs in the kernel, which comes back
        // before the end only where the host had a cycle to finish
        while (!rc && (r >= epssq) && (n < q.maxcycles))
            rc = tail_run(g, q, epssq, q.maxcycles, &n, &r);
    } else {
        while ((r >= epssq) && (n < q.maxcycles)) {
            rc = cycle(g, q, 0, &r);
            if (rc) break;
            ++n;
        }
    }
    g->stats.mg_cycles = n;
    g->stats.mg_levels = (int)g->mg->lv.size();
    if (rc) return rc;
    MISOR_TRY(collect_transfer_times(g));
    if (cycles) *cycles = n;
    if (res) *res = r;
    return MISOR_OK;
}

}  // namespace

void mg_free(misor_grid* g) {
    if (!g->mg) return;
    free_levels(g->mg);
    free_dist_levels(g->mg);
    for (hipEvent_t e : g->mg->ev) (void)hipEventDestroy(e);
    delete g->mg;
    g->mg = nullptr;
}

int mg_set_stream(misor_grid* g, hipStream_t s) {
    if (!g->mg) return MISOR_OK;
    for (size_t l = 1; l < g->mg->lv.size(); ++l)
        MISOR_TRY(misor_set_stream(g->mg->lv[l], s));
    for (size_t l = 1; l < g->mg->dlv.size(); ++l)
        MISOR_TRY(misor_set_stream(g->mg->dlv[l], s));
    if (g->mg->gath) MISOR_TRY(misor_set_stream(g->mg->gath, s));
    return MISOR_OK;
}

int misor_mg_default_params(const misor_grid* g, misor_mg_params* out) {
    if (!g || !out) return fail(MISOR_EINVAL, "misor_mg_default_params: null argument");
    *out = default_params(g);
    return MISOR_OK;
}

int misor_mg_levels(int imax, int jmax, int coarse_cells, int* nlevels, int* shapes, int cap) {
    if (!nlevels) return fail(MISOR_EINVAL, "misor_mg_levels: null nlevels");
    if (imax < 2 || jmax < 2) return fail(MISOR_EINVAL, "misor_mg_levels: imax, jmax must be >= 2");
    if (coarse_cells < 0 || cap < 0 || (cap > 0 && !shapes))
        return fail(MISOR_EINVAL, "misor_mg_levels: coarse_cells, cap >= 0; shapes for cap > 0");
    int n = 0, ni = imax, nj = jmax;
    for (;;) {
        if (n < cap) {
            shapes[2 * n] = ni;
            shapes[2 * n + 1] = nj;
        }
        ++n;
        int nic = 0, njc = 0;
        if (!mg_coarsen(ni, nj, coarse_cells, &nic, &njc)) break;
        ni = nic;
        nj = njc;
    }
    *nlevels = n;
    return MISOR_OK;
}

int misor_mg_tail(int imax, int jmax, int coarse_cells, int* first, int* count) {
    if (!first || !count) return fail(MISOR_EINVAL, "misor_mg_tail: null first or count");
    int shapes[2 * 64], n = 0;  // a side halves per level: far fewer than 64 levels
    MISOR_TRY(misor_mg_levels(imax, jmax, coarse_cells, &n, shapes, 64));
    tail_rule(n,
              [&](int l, int* ni, int* nj) {
                  *ni = shapes[2 * l];
                  *nj = shapes[2 * l + 1];
              },
              first, count);
    return MISOR_OK;
}

int misor_solve_mg(misor_grid* g, const misor_mg_params* prm, int* cycles, double* res) {
    if (prm) MISOR_TRY(check_params(*prm));
    if (!g) return fail(MISOR_EINVAL, "misor_solve_mg: null grid");
    if (g->desc.variant != MISOR_SOLVE_RB)
        return fail(MISOR_EINVAL, "misor_solve_mg smooths with solveRB (variant RB)");
    if (g->dist)
        return fail(MISOR_ESTATE,
                    "misor_solve_mg is the single-rank form: a decomposed grid is cycled by "
                    "misor_solve_mg_dist");
    return solve_mg_single(g, prm ? *prm : default_params(g), cycles, res);
}

int misor_mg_dist_levels(int nranks, const int dims_in[2], int imax, int jmax, int coarse_cells,
                         int gather_cells, int* nlevels, int* ndist) {
    if (!nlevels || !ndist) return fail(MISOR_EINVAL, "misor_mg_dist_levels: null nlevels or ndist");
    MgDistPlan P{};
    char err[kDecompErr];
    const int rc = mg_dist_plan(nranks, dims_in, imax, jmax, coarse_cells, gather_cells, &P, err);
    if (rc) return fail(rc, "%s", err);
    *nlevels = P.nlevels;
    *ndist = P.ndist;
    return MISOR_OK;
}

int misor_solve_mg_dist(misor_grid* g, const misor_mg_params* prm, int gather_cells, int* cycles,
                        double* res) {
    if (prm) MISOR_TRY(check_params(*prm));
    if (!g) return fail(MISOR_EINVAL, "misor_solve_mg_dist: null grid");
    if (g->desc.variant != MISOR_SOLVE_RB)
        return fail(MISOR_EINVAL, "misor_solve_mg_dist smooths with solveRB (variant RB)");
    const misor_mg_params q = prm ? *prm : default_params(g);
    if (!g->dist) return solve_mg_single(g, q, cycles, res);
    if (gather_cells < 0) gather_cells = kMgGatherCells;
    MgDistPlan P{};
    char err[kDecompErr];
    const int prc = mg_dist_plan(g->desc.nranks, g->loc.dims, g->desc.imax, g->desc.jmax,
                                 q.coarse_cells, gather_cells, &P, err);
    if (prc) return fail(prc, "%s", err);
    HIPCHK(hipSetDevice(g->device));
    MISOR_TRY(ensure_dist_hierarchy(g, q.coarse_cells, gather_cells, P));
    if (g->mg->gath) g->mg->gath->stats.mg_tail_levels = 0;
    const double epssq = g->desc.eps * g->desc.eps;
    int n = 0;
    double r = 1.0;  // as solveRB's loop (solver.c:196)
    int rc = MISOR_OK;
    // res is level 0's all-reduced residual, the same bits on every rank: all
    // ranks leave the loop after the same cycle
    while ((r >= epssq) && (n < q.maxcycles)) {
        rc = cycle_dist(g, q, 0, &r);
        if (rc) break;
        ++n;
    }
    const misor_grid* G = g->mg->gath;
    g->stats.mg_cycles = n;
    g->stats.mg_levels = P.nlevels;
    g->stats.mg_dist_levels = P.ndist;
    g->stats.mg_tail_levels = G && n > 0 ? G->stats.mg_tail_levels : 0;
    if (rc) return rc;
    MISOR_TRY(collect_transfer_times(g));
    if (cycles) *cycles = n;
    if (res) *res = r;
    return MISOR_OK;
}
