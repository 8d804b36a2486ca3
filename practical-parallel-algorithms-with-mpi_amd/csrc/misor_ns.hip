// misor_ns.hip -- the NS step entry points of the C ABI (computeTimestep,
// boundary conditions, computeFG + computeRHS, normalizePressure, adaptUV)
// and their HIP-event timing (misor_grid.h).

#include "misor_grid.h"

// ---------------------------------------------------------------------------
// NS step
// ---------------------------------------------------------------------------

int misor_ns_setup(misor_grid* g, const misor_ns_desc* ns) {
    if (!g || !ns) return fail(MISOR_EINVAL, "null argument");
    NsLaunch& L = g->nl;
    L.s = g->stream;
    L.pitch = g->pitch;
    L.ni = g->loc.ni;
    L.nj = g->loc.nj;
    L.prm.dx = g->desc.dx;
    L.prm.dy = g->desc.dy;
    L.prm.dt = 0.0;
    L.prm.xlength = ns->xlength;
    L.prm.ylength = ns->ylength;
    L.prm.re = ns->re;
    L.prm.gx = ns->gx;
    L.prm.gy = ns->gy;
    L.prm.gamma = ns->gamma;
    L.prm.bc_left = ns->bcLeft;
    L.prm.bc_right = ns->bcRight;
    L.prm.bc_bottom = ns->bcBottom;
    L.prm.bc_top = ns->bcTop;
    L.prm.problem = ns->problem;
    L.wall_left = g->loc.neighbours[0] < 0;
    L.wall_right = g->loc.neighbours[1] < 0;
    L.wall_bottom = g->loc.neighbours[2] < 0;
    L.wall_top = g->loc.neighbours[3] < 0;
    L.ioff = g->loc.ioff;
    L.joff = g->loc.joff;
    L.imax_g = g->desc.imax;
    L.jmax_g = g->desc.jmax;
    ++g->uv_ver;
    g->ns_ready = true;
    return MISOR_OK;
}

#define NEED_NS(g)                                                                 \
    do {                                                                           \
        if (!(g)) return fail(MISOR_EINVAL, "null grid");                          \
        if (!(g)->ns_ready) return fail(MISOR_ESTATE, "misor_ns_setup not called"); \
        HIPCHK(hipSetDevice((g)->device));                                         \
    } while (0)

// add the NS kernel groups' timed launches so far to the stats
int collect_ns_times(misor_grid* g) {
    for (int k = 0; k < 3; ++k) {
        for (size_t q = 0; q < g->nev_used[k]; ++q) {
            float ms = 0.f;
            HIPCHK(hipEventSynchronize(g->nev[k][2 * q + 1]));
            HIPCHK(hipEventElapsedTime(&ms, g->nev[k][2 * q], g->nev[k][2 * q + 1]));
            g->stats.ns_ms[k] += ms;
        }
        g->nev_used[k] = 0;
    }
    return MISOR_OK;
}

// a start/stop event pair around launches of NS kernel group k (0 computeFG,
// 1 adaptUV, 2 normalizePressure) when timing is on; `call` counts a call
// (normalizePressure records three pairs per call)
static bool ns_pair(misor_grid* g, int k, bool call, hipEvent_t* e0, hipEvent_t* e1) {
    if (!g->timing) return false;
    if (g->nev_used[k] >= 512 && collect_ns_times(g) != MISOR_OK) return false;
    std::vector<hipEvent_t>& v = g->nev[k];
    size_t& u = g->nev_used[k];
    while (v.size() < 2 * (u + 1)) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return false;
        v.push_back(e);
    }
    *e0 = v[2 * u];
    *e1 = v[2 * u + 1];
    ++u;
    if (call) g->stats.ns_calls[k]++;
    return true;
}

int misor_max_uv(misor_grid* g, double* umax, double* vmax) {
    NEED_NS(g);
    // the partials adaptUV computed, when no u, v write came after it
    const double* part = g->max_partials;
    if (g->max_ver != g->uv_ver) {
        launch_absmax2(g->nl, g->fld[kU], g->fld[kV], g->red_partials);
        part = g->red_partials;
    }
    launch_finish_reduce(g->stream, part, reduce_blocks(g->loc.ni, g->loc.nj),
                         kReduceMax, 2, g->red_out);
    HIPCHK(hipGetLastError());
    if (g->dist)
    {
        int rc = allreduce(g, g->red_out, 2, 1);
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(g->red_host, g->red_out, 2 * sizeof(double), hipMemcpyDeviceToHost,
                          g->stream));
    MISOR_TRY(wait_stream(g, g->stream));
    if (umax) *umax = g->red_host[0];
    if (vmax) *vmax = g->red_host[1];
    return MISOR_OK;
}

int misor_compute_timestep(misor_grid* g, double dt_bound, double tau, double* dt_out) {
    double umax = 0, vmax = 0;
    int rc = misor_max_uv(g, &umax, &vmax);
    if (rc) return rc;
    // computeTimestep, assignment-5/sequential/src/solver.c:219-234
    double dt = dt_bound;
    const double dx = g->desc.dx, dy = g->desc.dy;
    if (umax > 0) dt = (dt > dx / umax) ? dx / umax : dt;
    if (vmax > 0) dt = (dt > dy / vmax) ? dy / vmax : dt;
    g->nl.prm.dt = dt * tau;
    if (dt_out) *dt_out = g->nl.prm.dt;
    return MISOR_OK;
}

int misor_set_dt(misor_grid* g, double dt) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    g->nl.prm.dt = dt;
    return MISOR_OK;
}

int misor_set_boundary_conditions(misor_grid* g) {
    NEED_NS(g);
    ++g->uv_ver;
    launch_set_bc(g->nl, g->fld[kU], g->fld[kV]);
    HIPCHK(hipGetLastError());
    return MISOR_OK;
}

int misor_set_special_boundary_condition(misor_grid* g) {
    NEED_NS(g);
    ++g->uv_ver;
    launch_special_bc(g->nl, g->fld[kU]);
    HIPCHK(hipGetLastError());
    return MISOR_OK;
}

int misor_compute_fg(misor_grid* g) {
    NEED_NS(g);
    int rc = exchange(g, g->fld[kU], 1);  // 9-point stencil incl. diagonals: corners too
    if (!rc) rc = exchange(g, g->fld[kV], 1);
    if (rc) return rc;
    ++g->fgr_ver;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    const bool timed = ns_pair(g, 0, true, &t0, &t1);
    if (timed) HIPCHK(hipEventRecord(t0, g->stream));
    if (g->ns_fuse) {  // computeRHS of the same f, g in the same pass (ns_kernels.hip)
        launch_compute_fg_rhs(g->nl, g->fld[kU], g->fld[kV], g->fld[kF], g->fld[kG],
                              g->fld[kRhs]);
        g->rhs_halo = 0;
        g->fused_ver = g->fgr_ver;
        g->fused_dt = g->nl.prm.dt;
    } else {
        launch_compute_fg(g->nl, g->fld[kU], g->fld[kV], g->fld[kF], g->fld[kG]);
    }
    if (timed) HIPCHK(hipEventRecord(t1, g->stream));
    HIPCHK(hipGetLastError());
    return MISOR_OK;
}

int misor_compute_rhs(misor_grid* g) {
    NEED_NS(g);
    // the fused computeFG already wrote rhs from these f, g and this dt: only
    // the cells that read a neighbour's F(0, j) / G(i, 0) are left
    // (decomposed: the exchange is collective, so every rank takes part, also
    // one with walls on its left and bottom whose rhs is complete already)
    const bool fused = g->fused_ver == g->fgr_ver && g->fused_dt == g->nl.prm.dt;
    ++g->fgr_ver;
    g->rhs_halo = 0;
    if (fused && !g->dist) return MISOR_OK;
    int rc = exchange(g, g->fld[kF], 1);  // F(i-1,j), G(i,j-1): the skeleton's shift()
    if (!rc) rc = exchange(g, g->fld[kG], 1);
    if (rc) return rc;
    if (fused) {
        if (!(g->nl.wall_left && g->nl.wall_bottom))
            launch_rhs_edges(g->nl, g->fld[kF], g->fld[kG], g->fld[kRhs]);
    } else {
        launch_compute_rhs(g->nl, g->fld[kF], g->fld[kG], g->fld[kRhs]);
    }
    HIPCHK(hipGetLastError());
    return MISOR_OK;
}

// normalizePressure (assignment-5/sequential/src/solver.c:204-217) with the
// sum exact (ns_kernels.hip launch_exact_sum): the mean, and so p, is the same
// for every decomposition -- the reference's MPI build all-reduces per-rank
// partial sums (assignment-5/skeleton/src/solver.c:697), whose rounding depends
// on the partition.  Two passes over p: the global max |p| (order-free) fixes
// the fixed-point scale, then the exact sum; one host round trip per call
// (every 100 time steps in the reference's main loop).
int misor_normalize_pressure(misor_grid* g) {
    NEED_NS(g);
    double* p = pbuf(g, g->cur);
    const int nb = reduce_blocks(g->loc.ni, g->loc.nj);
    hipEvent_t t0 = nullptr, t1 = nullptr;
    bool timed = ns_pair(g, 2, true, &t0, &t1);
    if (timed) HIPCHK(hipEventRecord(t0, g->stream));
    launch_absmax2(g->nl, p, p, g->red_partials);
    launch_finish_reduce(g->stream, g->red_partials, nb, kReduceMax, 2, g->red_out);
    if (timed) HIPCHK(hipEventRecord(t1, g->stream));
    HIPCHK(hipGetLastError());
    if (g->dist) {
        int rc = allreduce(g, g->red_out, 1, 1);
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(g->red_host, g->red_out, sizeof(double), hipMemcpyDeviceToHost,
                          g->stream));
    MISOR_TRY(wait_stream(g, g->stream));
    const double mx = g->red_host[0];
    int E = 0;
    (void)frexp(mx, &E);
    timed = ns_pair(g, 2, false, &t0, &t1);
    if (timed) HIPCHK(hipEventRecord(t0, g->stream));
    launch_exact_sum(g->nl, p, E, g->red_partials, g->red_out);
    if (timed) HIPCHK(hipEventRecord(t1, g->stream));
    HIPCHK(hipGetLastError());
    if (g->dist) {
        int rc = allreduce(g, g->red_out, 3, 0);  // integer limbs < 2^53: exact
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(g->red_host, g->red_out, 3 * sizeof(double), hipMemcpyDeviceToHost,
                          g->stream));
    MISOR_TRY(wait_stream(g, g->stream));
    const double cells = (double)(g->desc.imax + 2) * (double)(g->desc.jmax + 2);
    const double avg = exact_sum_value(g->red_host, E) / cells;  // solver.c:213
    timed = ns_pair(g, 2, false, &t0, &t1);
    if (timed) HIPCHK(hipEventRecord(t0, g->stream));
    launch_sub_mean(g->nl, p, avg);
    if (timed) HIPCHK(hipEventRecord(t1, g->stream));
    HIPCHK(hipGetLastError());
    return MISOR_OK;
}

int misor_adapt_uv(misor_grid* g) {
    NEED_NS(g);
    {
        int rc = p_halo(g);  // P(i+1,j), P(i,j+1) of the rank's last column / row
        if (rc) return rc;
    }
    hipEvent_t t0 = nullptr, t1 = nullptr;
    const bool timed = ns_pair(g, 1, true, &t0, &t1);
    if (timed) HIPCHK(hipEventRecord(t0, g->stream));
    launch_adapt_absmax(g->nl, g->fld[kF], g->fld[kG], pbuf(g, g->cur), g->fld[kU], g->fld[kV],
                        g->max_partials);
    if (timed) HIPCHK(hipEventRecord(t1, g->stream));
    g->max_ver = ++g->uv_ver;
    HIPCHK(hipGetLastError());
    return MISOR_OK;
}
