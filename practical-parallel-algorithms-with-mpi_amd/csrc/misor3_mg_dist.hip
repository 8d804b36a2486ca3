// misor3_mg_dist.hip -- the 3D multigrid cycle on a slab-decomposed grid
// (misor3_solve_mg_dist, include/misor.h; DESIGN.md "Geometric multigrid, 3D,
// decomposed").  The level split is mg3_dist_plan.h's.
//
// A distributed level l >= 1 is an internal slab misor_grid3 holding p, its
// ping-pong partner and rhs only, on level 0's stream and communicator.
// Smoothing and a distributed coarsest solve are the slab misor3_solve
// (solve3_with), which is the single domain's bit for bit at global colour
// parity and exchanges the 2-deep halo of p and the 1-deep halo of rhs itself
// on every call (rhs is new every cycle; nothing caches its halo).  The
// restriction is the single-rank kernel on the slab's local planes: the slabs'
// koff is even, so the 2 x 2 x 2 groups stay aligned.  The prolongation is the
// slab form of mg3_kernels.hip.
//
// The last distributed level restricts straight into this rank's planes of the
// gathered level's whole-domain rhs; the other ranks' planes arrive by one
// all-gather (allgather_slabs3).  Every rank then runs the single-rank cycle
// (mg3_cycle) on the gathered levels, the same bits everywhere, and corrects
// its slab from its window of the whole-domain e: nothing is sent back.
//
// Every argument check precedes the first HIP or collective call, and every
// rank makes it from the same arithmetic.

#include "mg3_dist_plan.h"
#include "misor_grid3.h"

using namespace misor;

namespace {

// a level of g's hierarchy: shape n[] in g's box, decomposed like g (slab) or whole
int create_level(misor_grid3* g, const int n[3], bool slab, int level, misor_grid3** out) {
    // the same box with fewer cells each way: dx, dy, dz double exactly per level
    misor3_desc d = g->desc;
    d.imax = n[0];
    d.jmax = n[1];
    d.kmax = n[2];
    d.device = g->device;
    d.comm_id = nullptr;
    if (slab) {
        d.nranks = g->nranks;
        d.rank = g->rank;
        return create3_level_slab(out, &d, g, level);
    }
    d.nranks = 1;
    d.rank = 0;
    return create3_level(out, &d, g->stream);
}

// (re)build the levels below the decomposed grid g for plan P: collective, and
// every rank rebuilds at the same calls (the plan is the same on every rank)
int ensure_dist_hierarchy(misor_grid3* g, int coarse_cells, const Mg3DistPlan& P) {
    if (!g->mg) g->mg = new Mg3Hierarchy();
    Mg3Hierarchy* h = g->mg;
    if (h->dist_coarse_cells != coarse_cells || h->dist_ndist != P.ndist || h->dlv.empty()) {
        HIPCHK(hipStreamSynchronize(g->stream));
        mg3_dist_free(h);
        h->dist_coarse_cells = coarse_cells;
        h->dist_ndist = P.ndist;
        h->dlv.push_back(g);
        int n[3] = {g->desc.imax, g->desc.jmax, g->desc.kmax};
        int rc = MISOR_OK;
        for (int l = 1; l <= P.ndist && l < P.nlevels && !rc; ++l) {
            for (int a = 0; a < 3; ++a) n[a] /= 2;
            misor_grid3* c = nullptr;
            const bool slab = l < P.ndist;
            rc = create_level(g, n, slab, l, &c);
            if (rc) break;
            if (!slab) {
                // The gathered levels take the streaming sweep, not the resident solve
                // (the same bits).  resident3_boxes sizes that cooperative grid against
                // the whole device (CUs x workgroups per CU), and every rank cycles its
                // gathered levels at the same moment: in process, several such grids on
                // one device cannot all be co-resident, and their spinning grid barriers
                // can time out or deadlock.  With one process per GPU (RCCL) there is no
                // such concurrency and this only costs launches: an open item.
                c->resident = 0;
                c->levels_inherit_resident = true;
                h->gath = c;
                break;
            }
            h->dlv.push_back(c);
            // the halved slab is the slab of the halved grid (mg3_dist_plan.h)
            int kl = 0, ko = 0;
            mg3_dist_slab(P, g->rank, l, &kl, &ko);
            if (c->g.K != kl || c->g.koff != ko)
                rc = fail(MISOR_ESTATE, "misor3_solve_mg_dist: level %d is not the halved slab", l);
        }
        if (rc) {
            mg3_dist_free(h);
            return rc;
        }
        h->dlv.back()->peer_gath = h->gath;
        // in process: every rank's gathered level exists before a peer copies from it
        if (g->local && h->gath) g->local->barrier();
    }
    if (h->gath) MISOR_TRY(mg3_ensure_hierarchy(h->gath, coarse_cells));
    return MISOR_OK;
}

// the coarse grid under slab f as the transfer launches see it: c's columns,
// rows and strides, half of f's planes
G3 coarse_view(const misor_grid3* f, const misor_grid3* c) {
    G3 v = c->g;
    v.K = f->g.K / 2;
    return v;
}

// One cycle on distributed level l of the decomposed grid g0; *res as mg3_cycle's.
int cycle_dist(misor_grid3* g0, const misor_mg_params& q, size_t l, double* res) {
    Mg3Hierarchy* h = g0->mg;
    misor_grid3* f = h->dlv[l];
    const bool last = l + 1 == h->dlv.size();
    if (last && !h->gath) {  // the coarsest level, decomposed
        int it = 0;
        return solve3_with(f, q.omega_coarse, q.eps_coarse, q.itermax_coarse, 1.0, &it, res);
    }
    const bool timed = l == 0 && g0->timing;
    MISOR_TRY(mg3_smooth(f, q.omega_smooth, q.nu1, res));
    // the residual of a slab's first and last plane reads the neighbours' p: the
    // slab solve leaves that halo current; without one since p last changed
    // (the first cycle, or the correction of the cycle before) it is exchanged
    if (q.nu1 < 1) MISOR_TRY(exchange3(f, MISOR3_P, 1));
    const double dx2 = f->dx * f->dx, dy2 = f->dy * f->dy, dz2 = f->dz * f->dz;
    // the coarse level, its rhs planes under this slab and its e seen from them
    misor_grid3* c = last ? h->gath : h->dlv[l + 1];
    const long long win = last ? f->g.koff / 2 : 0;  // local coarse plane 0 in c's arrays
    const G3 cv = coarse_view(f, c);
    if (timed) MISOR_TRY(mg3_record_transfer(g0, 0));
    launch_mg3_residual_restrict(g0->stream, f->g, cv, f->fld[MISOR3_P], f->fld[MISOR3_RHS],
                                 c->fld[MISOR3_RHS] + win * c->g.sxy, 1.0 / dx2, 1.0 / dy2,
                                 1.0 / dz2);
    HIPCHK(hipGetLastError());
    if (timed) MISOR_TRY(mg3_record_transfer(g0, -1));
    // the hand-over: everybody else's restricted planes into the whole-domain rhs
    if (last) MISOR_TRY(allgather_slabs3(f, c, cv.K));
    // e = 0 over the whole allocation, ghosts and the inter-rank halo included
    launch_fill(g0->stream, c->mem[MISOR3_P], c->nalloc, 0.0);
    HIPCHK(hipGetLastError());
    c->alt_stale = true;
    double unused = 0.0;
    if (last) {
        // every rank cycles the gathered levels alone, the same bits everywhere
        MISOR_TRY(mg3_cycle(c, q, 0, &unused));
    } else {
        MISOR_TRY(cycle_dist(g0, q, l + 1, &unused));
        // the interpolation at a slab's first and last plane reads the neighbours' e
        MISOR_TRY(exchange3(c, MISOR3_P, 1));
    }
    if (timed) MISOR_TRY(mg3_record_transfer(g0, 1));
    launch_mg3_prolong_correct_slab(g0->stream, f->g, cv, f->fld[MISOR3_P], c->fld[MISOR3_P], win,
                                    f->g.lo_phys, f->g.hi_phys);
    HIPCHK(hipGetLastError());
    if (timed) MISOR_TRY(mg3_record_transfer(g0, -1));
    f->alt_stale = true;  // p changed outside a sweep; its inter-rank halo is the old p's
    return mg3_smooth(f, q.omega_smooth, q.nu2, res);
}

}  // namespace

void mg3_dist_free(Mg3Hierarchy* h) {
    for (size_t l = 1; l < h->dlv.size(); ++l) misor3_destroy(h->dlv[l]);
    if (!h->dlv.empty()) h->dlv[0]->peer_gath = nullptr;
    h->dlv.clear();
    if (h->gath) misor3_destroy(h->gath);
    h->gath = nullptr;
}

extern "C" {

int misor3_mg_dist_levels(int nranks, int imax, int jmax, int kmax, int coarse_cells,
                          int gather_cells, int* nlevels, int* ndist) {
    if (!nlevels || !ndist)
        return fail(MISOR_EINVAL, "misor3_mg_dist_levels: null nlevels or ndist");
    Mg3DistPlan P{};
    char err[kDecompErr];
    const int rc = mg3_dist_plan(nranks, imax, jmax, kmax, coarse_cells, gather_cells, &P, err);
    if (rc) return fail(rc, "%s", err);
    *nlevels = P.nlevels;
    *ndist = P.ndist;
    return MISOR_OK;
}

int misor3_solve_mg_dist(misor_grid3* g, const misor_mg_params* prm, int gather_cells,
                         int* cycles, double* res) {
    if (prm) MISOR_TRY(mg3_check_params(*prm, "misor3_solve_mg_dist"));
    if (!g) return fail(MISOR_EINVAL, "misor3_solve_mg_dist: null grid");
    const misor_mg_params q = prm ? *prm : mg3_default_params(g);
    if (!dist(g)) return mg3_solve_single(g, q, cycles, res);
    if (g->cart)
        return fail(MISOR_ESTATE,
                    "misor3_solve_mg_dist runs on slabs (misor3_create), not on a Cartesian "
                    "process grid");
    Mg3DistPlan P{};
    char err[kDecompErr];
    const int prc = mg3_dist_plan(g->nranks, g->desc.imax, g->desc.jmax, g->desc.kmax,
                                  q.coarse_cells, gather_cells, &P, err);
    if (prc) return fail(prc, "%s", err);
    HIPCHK(hipSetDevice(g->device));
    MISOR_TRY(ensure_dist_hierarchy(g, q.coarse_cells, P));
    const double epssq = g->desc.eps * g->desc.eps;
    int n = 0;
    double r = 1.0;  // as the solve's loop (solver.c:196)
    int rc = MISOR_OK;
    // res is level 0's all-reduced carry, the same bits on every rank: all ranks
    // leave the loop after the same cycle
    while ((r >= epssq) && (n < q.maxcycles)) {
        rc = cycle_dist(g, q, 0, &r);
        if (rc) break;
        ++n;
    }
    // no smoothing after the last correction: p's 2-deep halo as misor3_solve leaves it
    if (!rc && n > 0 && q.nu2 < 1 && P.nlevels > 1) rc = exchange3(g, MISOR3_P, kHalo);
    g->mg_info.cycles = n;
    g->mg_info.levels = P.nlevels;
    g->mg_info.dist_levels = P.ndist;
    if (rc) return rc;
    MISOR_TRY(mg3_collect_transfer_times(g));
    if (cycles) *cycles = n;
    if (res) *res = r;
    return MISOR_OK;
}

}  // extern "C"
