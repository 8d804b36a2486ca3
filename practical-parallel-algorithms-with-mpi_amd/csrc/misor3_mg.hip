// misor3_mg.hip -- geometric multigrid on top of the 3D red-black solve
// (include/misor.h "3D multigrid", DESIGN.md "Geometric multigrid, 3D"): the
// level rule, the hierarchy and the V-cycle.
//
// Levels 1 .. L-1 are internal single-rank misor_grid3s on the user's grid's
// stream, holding p, its ping-pong partner and rhs only: a level's rhs is the
// restricted residual rc of the level above, its p the correction e.
// Smoothing and the coarsest solve are misor3_solve itself, run with other
// parameters for the duration of the call (solve3_with), so every level takes
// the form the existing rule gives its size -- the LDS-resident launch or the
// fused k-marching sweep.  The only kernels of its own are the two transfers
// of mg3_kernels.hip; they add no host round trip to a cycle.
//
// Every argument check precedes the first HIP call.

#include <vector>

#include "mg3_dist_plan.h"  // mg3_coarsen
#include "misor_grid3.h"

using namespace misor;

namespace {

constexpr size_t kMg3EventPairs = 64;  // pairs held before they are resolved

void free_levels(Mg3Hierarchy* h) {
    for (size_t l = 1; l < h->lv.size(); ++l) misor3_destroy(h->lv[l]);
    h->lv.clear();
}

}  // namespace

int mg3_check_params(const misor_mg_params& q, const char* who) {
    if (q.nu1 < 0 || q.nu2 < 0)
        return fail(MISOR_EINVAL, "%s: nu1 = %d, nu2 = %d: counts must be >= 0", who, q.nu1,
                    q.nu2);
    if (q.nu1 + q.nu2 < 1)
        return fail(MISOR_EINVAL, "%s: nu1 + nu2 must be >= 1 (a cycle smooths)", who);
    if (!(q.omega_smooth > 0.0) || !(q.omega_coarse > 0.0))
        return fail(MISOR_EINVAL, "%s: omega_smooth and omega_coarse must be > 0", who);
    if (q.coarse_cells < 0)
        return fail(MISOR_EINVAL, "%s: coarse_cells = %d must be >= 0", who, q.coarse_cells);
    if (q.itermax_coarse < 0)
        return fail(MISOR_EINVAL, "%s: itermax_coarse = %d must be >= 0", who,
                    q.itermax_coarse);
    if (q.maxcycles < 0)
        return fail(MISOR_EINVAL, "%s: maxcycles = %d must be >= 0", who, q.maxcycles);
    return MISOR_OK;
}

// The 3D defaults: as the 2D ones but coarse_cells = 512, i.e. 128^3 coarsens
// down to 8^3.
misor_mg_params mg3_default_params(const misor_grid3* g) {
    misor_mg_params q{};
    q.nu1 = q.nu2 = 2;
    q.omega_smooth = 1.0;
    q.coarse_cells = 512;
    q.omega_coarse = 1.7;
    q.eps_coarse = 0.1 * g->desc.eps;
    q.itermax_coarse = 1000;
    q.maxcycles = 100;
    return q;
}

// nu iterations without early exit.  The carry is seeded with 0.0 and eps is
// 0, so the entry test and every loop test (res >= 0) pass; *res only where an
// iteration ran
int mg3_smooth(misor_grid3* g, double omega, int nu, double* res) {
    if (nu < 1) return MISOR_OK;
    int it = 0;
    return solve3_with(g, omega, 0.0, nu, 0.0, &it, res);
}

// (re)build the levels below g for coarse_cells, on g's stream
int mg3_ensure_hierarchy(misor_grid3* g, int coarse_cells) {
    if (!g->mg) g->mg = new Mg3Hierarchy();
    Mg3Hierarchy* h = g->mg;
    if (h->coarse_cells == coarse_cells && !h->lv.empty()) return MISOR_OK;
    HIPCHK(hipStreamSynchronize(g->stream));
    free_levels(h);
    h->coarse_cells = coarse_cells;
    h->lv.push_back(g);
    int n[3] = {g->desc.imax, g->desc.jmax, g->desc.kmax}, nc[3];
    while (mg3_coarsen(n, coarse_cells, nc)) {
        // the same box with half the cells each way: dx, dy, dz double exactly
        misor3_desc d = g->desc;
        d.imax = n[0] = nc[0];
        d.jmax = n[1] = nc[1];
        d.kmax = n[2] = nc[2];
        d.device = g->device;
        d.nranks = 1;
        d.rank = 0;
        d.comm_id = nullptr;
        misor_grid3* c = nullptr;
        const int rc = create3_level(&c, &d, g->stream);
        if (rc) {
            free_levels(h);
            return rc;
        }
        // below a user's grid the levels keep the default, whatever its own knob
        if (g->levels_inherit_resident) c->resident = g->resident;
        h->lv.push_back(c);
    }
    return MISOR_OK;
}

// the timed transfer launches of level 0 so far into mg_info
int mg3_collect_transfer_times(misor_grid3* g) {
    Mg3Hierarchy* h = g->mg;
    if (!h->ev_used) return MISOR_OK;
    HIPCHK(hipStreamSynchronize(g->stream));
    for (size_t k = 0; k < h->ev_used; ++k) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, h->ev[2 * k], h->ev[2 * k + 1]));
        g->mg_info.transfer_ms[h->kind[k]] += ms;
    }
    g->mg_info.transfers += (long long)h->ev_used;
    h->ev_used = 0;
    return MISOR_OK;
}

// the start (kind 0 / 1) or stop (kind < 0) event of the next pair around a
// timed transfer launch, recorded on the stream.  A pair counts once its stop
// is recorded: a start whose stop never came (an error in between) is reused.
int mg3_record_transfer(misor_grid3* g, int kind) {
    Mg3Hierarchy* h = g->mg;
    while (h->ev.size() < 2 * kMg3EventPairs) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        h->ev.push_back(e);
    }
    h->kind.resize(kMg3EventPairs);
    const bool stop = kind < 0;
    if (!stop && h->ev_used == kMg3EventPairs) MISOR_TRY(mg3_collect_transfer_times(g));
    if (!stop) h->kind[h->ev_used] = kind;
    HIPCHK(hipEventRecord(h->ev[2 * h->ev_used + (stop ? 1 : 0)], g->stream));
    if (stop) ++h->ev_used;
    return MISOR_OK;
}

// One cycle on level l; *res: the residual the level's last smoothing call
// leaves (the coarsest level: its solve's), untouched if none ran.  The
// transfers take fld[MISOR3_P] after each solve: the fused sweep swaps the
// pointers so that it is the buffer with the result.
int mg3_cycle(misor_grid3* g0, const misor_mg_params& q, size_t l, double* res) {
    Mg3Hierarchy* h = g0->mg;
    misor_grid3* f = h->lv[l];
    if (l + 1 == h->lv.size()) {
        int it = 0;
        return solve3_with(f, q.omega_coarse, q.eps_coarse, q.itermax_coarse, 1.0, &it, res);
    }
    misor_grid3* c = h->lv[l + 1];
    const bool timed = l == 0 && g0->timing;
    MISOR_TRY(mg3_smooth(f, q.omega_smooth, q.nu1, res));
    // rc = R (rhs - lap p) into the coarse rhs
    const double dx2 = f->dx * f->dx, dy2 = f->dy * f->dy, dz2 = f->dz * f->dz;
    if (timed) MISOR_TRY(mg3_record_transfer(g0, 0));
    launch_mg3_residual_restrict(g0->stream, f->g, c->g, f->fld[MISOR3_P], f->fld[MISOR3_RHS],
                                 c->fld[MISOR3_RHS], 1.0 / dx2, 1.0 / dy2, 1.0 / dz2);
    HIPCHK(hipGetLastError());
    if (timed) MISOR_TRY(mg3_record_transfer(g0, -1));
    // e = 0 over the whole allocation, ghosts, edges and corners included; the
    // partner buffer is a copy of it before the first sweep that uses it
    launch_fill(g0->stream, c->mem[MISOR3_P], c->nalloc, 0.0);
    HIPCHK(hipGetLastError());
    c->alt_stale = true;
    double rc_unused = 0.0;
    MISOR_TRY(mg3_cycle(g0, q, l + 1, &rc_unused));
    if (timed) MISOR_TRY(mg3_record_transfer(g0, 1));
    launch_mg3_prolong_correct(g0->stream, f->g, c->g, f->fld[MISOR3_P], c->fld[MISOR3_P]);
    HIPCHK(hipGetLastError());
    if (timed) MISOR_TRY(mg3_record_transfer(g0, -1));
    f->alt_stale = true;  // p changed outside a sweep
    return mg3_smooth(f, q.omega_smooth, q.nu2, res);
}

int mg3_solve_single(misor_grid3* g, const misor_mg_params& q, int* cycles, double* res) {
    HIPCHK(hipSetDevice(g->device));
    MISOR_TRY(mg3_ensure_hierarchy(g, q.coarse_cells));
    const double epssq = g->desc.eps * g->desc.eps;
    int n = 0;
    double r = 1.0;  // as the solve's loop (solver.c:196)
    int rc = MISOR_OK;
    while ((r >= epssq) && (n < q.maxcycles)) {
        rc = mg3_cycle(g, q, 0, &r);
        if (rc) break;
        ++n;
    }
    g->mg_info.cycles = n;
    g->mg_info.levels = (int)g->mg->lv.size();
    g->mg_info.dist_levels = 0;
    if (rc) return rc;
    MISOR_TRY(mg3_collect_transfer_times(g));
    if (cycles) *cycles = n;
    if (res) *res = r;
    return MISOR_OK;
}

void mg3_free(misor_grid3* g) {
    if (!g->mg) return;
    free_levels(g->mg);
    mg3_dist_free(g->mg);
    for (hipEvent_t e : g->mg->ev) (void)hipEventDestroy(e);
    delete g->mg;
    g->mg = nullptr;
}

extern "C" {

int misor3_mg_default_params(const misor_grid3* g, misor_mg_params* out) {
    if (!g || !out) return fail(MISOR_EINVAL, "misor3_mg_default_params: null argument");
    *out = mg3_default_params(g);
    return MISOR_OK;
}

int misor3_mg_levels(int imax, int jmax, int kmax, int coarse_cells, int* nlevels, int* shapes,
                     int cap) {
    if (!nlevels) return fail(MISOR_EINVAL, "misor3_mg_levels: null nlevels");
    if (imax < 2 || jmax < 2 || kmax < 2)
        return fail(MISOR_EINVAL, "misor3_mg_levels: imax, jmax, kmax must be >= 2");
    if (coarse_cells < 0 || cap < 0 || (cap > 0 && !shapes))
        return fail(MISOR_EINVAL, "misor3_mg_levels: coarse_cells, cap >= 0; shapes for cap > 0");
    int cnt = 0, n[3] = {imax, jmax, kmax};
    for (;;) {
        if (cnt < cap)
            for (int a = 0; a < 3; ++a) shapes[3 * cnt + a] = n[a];
        ++cnt;
        int nc[3];
        if (!mg3_coarsen(n, coarse_cells, nc)) break;
        for (int a = 0; a < 3; ++a) n[a] = nc[a];
    }
    *nlevels = cnt;
    return MISOR_OK;
}

int misor3_solve_mg(misor_grid3* g, const misor_mg_params* prm, int* cycles, double* res) {
    if (prm) MISOR_TRY(mg3_check_params(*prm, "misor3_solve_mg"));
    if (!g) return fail(MISOR_EINVAL, "misor3_solve_mg: null grid");
    if (g->nranks > 1)
        return fail(MISOR_ESTATE,
                    "misor3_solve_mg has no decomposed form yet (single rank only)");
    return mg3_solve_single(g, prm ? *prm : mg3_default_params(g), cycles, res);
}

int misor3_get_mg_info(const misor_grid3* g, misor3_mg_info* out) {
    if (!g || !out) return fail(MISOR_EINVAL, "misor3_get_mg_info: null argument");
    *out = g->mg_info;
    return MISOR_OK;
}

}  // extern "C"
