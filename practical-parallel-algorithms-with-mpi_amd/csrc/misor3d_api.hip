// misor3d_api.hip -- the C ABI of the 3D path (include/misor.h, misor3_*):
// assignment-6's 3D Navier-Stokes solver (assignment-6/src/solver.c).  The
// entry points mirror the reference's solver.h one to one; fields are
// device-resident in the reference layout.  This unit: grid lifecycle,
// transfers, the Navier-Stokes step, tuning and timing; the transport is in
// misor3_comm.hip, misor3_solve in misor3_solve.hip, the decomposition
// arithmetic in decomp3.h.
//
// Decomposition: slabs of planes along k, one rank per GPU (or per host
// thread with the in-process transport).  The reference splits the box over a
// 3D Cartesian process grid (assignment-6/src/comm.c:24-101, 476-513); on one
// MI355X node a 1D split of at most 8 slabs keeps every halo a run of whole
// planes -- contiguous in this layout, so halos move by ncclSend/ncclRecv
// straight from the field, no packing -- and each GPU still owns >= 16 planes
// at the reference's 128^3.  Colours are global (i+j+k with global k), so the
// fields are bit-identical to the single-domain solve for every slab count.
//
// Storage per field: planes -1 .. K+2 of the rank's slab (K = its plane count),
// i.e. the reference's local array (planes 0 .. K+1) plus one more plane on
// each side for the 2-deep halo the fused sweep reads.
//
// Second decomposition (misor3_create_cart): the reference's 3D Cartesian
// process grid itself.  A rank holds a block of ni x nj x nk cells as the
// reference's local array (ni+2)(nj+2)(nk+2), whose one ghost layer is the
// 1-deep halo; the allocation keeps the two spare planes -1 and K+2 of the
// slab storage (unused here), so plane_ptr, kSlack, fill and the gather treat
// both kinds of grid alike.  The solve on such a grid is the reference's two
// colour passes with an exchange before each.

#include <cstring>

#include "misor_grid3.h"

using namespace misor;

extern "C" {

void misor3_destroy(misor_grid3* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    mg3_free(g);  // the multigrid levels (they run on this grid's stream)
    for (auto& f : g->alloc)
        if (f) (void)hipFree(f);
    (void)hipFree(g->partials);
    (void)hipFree(g->rbar);
    (void)hipFree(g->rmbox);
    (void)hipFree(g->out);
    (void)hipHostFree(g->out_host);
    (void)hipFree(g->st);
    (void)hipFree(g->st2);
    (void)hipHostFree(g->st_host);
    (void)hipFree(g->gstage);
    (void)hipFree(g->hbuf);
    (void)hipFree(g->gbuf);
    for (auto& e : g->ev)
        if (e) (void)hipEventDestroy(e);
    if (g->comm && g->own_comm) ncclCommDestroy(g->comm);
    if (g->stream && g->own_stream) (void)hipStreamDestroy(g->stream);
    delete g;
}

// the decompositions themselves are in decomp3.h
int misor3_decompose(int nranks, int rank, int kmax, int* kloc, int* koff) {
    char err[kDecompErr];
    const int rc = decompose_slab(nranks, rank, kmax, kloc, koff, err);
    return rc == MISOR_OK ? rc : fail(rc, "%s", err);
}

int misor3_decompose_cart(int nranks, int rank, const int dims_in[3], int imax, int jmax,
                          int kmax, misor3_local* out) {
    char err[kDecompErr];
    const int rc = decompose_cart(nranks, rank, dims_in, imax, jmax, kmax, out, err);
    return rc == MISOR_OK ? rc : fail(rc, "%s", err);
}

// misor3_create (dims == nullptr: slabs) and misor3_create_cart; level_stream:
// create3_level's grid on that stream, with p, its partner and rhs only;
// parent: create3_level_slab's, on parent's communicator (d->comm_id is not read)
static int create3(misor_grid3** out, const misor3_desc* d, const int* dims, bool cart,
                   hipStream_t level_stream = nullptr, misor_grid3* parent = nullptr,
                   int level = 0) {
    if (!out || !d) return fail(MISOR_EINVAL, "null argument");
    *out = nullptr;
    if (d->imax < 2 || d->jmax < 2 || d->kmax < 2)
        return fail(MISOR_EINVAL, "imax, jmax, kmax must be >= 2");
    const int nranks = d->nranks > 0 ? d->nranks : 1;
    if (nranks <= 1) cart = false;
    int kloc = d->kmax, koff = 0;
    misor3_local loc{};
    if (nranks > 1) {
        if (!d->comm_id && !parent) return fail(MISOR_EINVAL, "nranks > 1 needs a comm_id");
        const int rc = cart ? misor3_decompose_cart(nranks, d->rank, dims, d->imax, d->jmax,
                                                    d->kmax, &loc)
                            : misor3_decompose(nranks, d->rank, d->kmax, &kloc, &koff);
        if (rc != MISOR_OK) return rc;
    }
    const int iloc = cart ? loc.n[0] : d->imax, jloc = cart ? loc.n[1] : d->jmax;
    if (cart) kloc = loc.n[2], koff = loc.off[2];
    misor_grid3* g = new misor_grid3();
    g->desc = *d;
    g->device = d->device;
    g->nranks = nranks;
    g->rank = nranks > 1 ? d->rank : 0;
    g->cart = cart;
    g->loc = loc;
    if (!cart) {
        g->prev = g->rank > 0 ? g->rank - 1 : -1;
        g->next = g->rank < nranks - 1 ? g->rank + 1 : -1;
    }
    if (d->device >= 0) {
        if (hipSetDevice(d->device) != hipSuccess) {
            delete g;
            return fail(MISOR_EHIP, "hipSetDevice(%d) failed", d->device);
        }
    } else {
        (void)hipGetDevice(&g->device);
    }
#define CF(code, ...)                        \
    do {                                     \
        int c_ = fail(code, __VA_ARGS__);   \
        misor3_destroy(g);                   \
        return c_;                           \
    } while (0)
    if (level_stream) {
        g->stream = level_stream;
        g->own_stream = false;
    } else if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess) {
        CF(MISOR_EHIP, "hipStreamCreate failed");
    }
    g->g.I = iloc;
    g->g.J = jloc;
    g->g.K = kloc;
    g->g.sx = iloc + 2;
    g->g.sxy = (long long)(iloc + 2) * (jloc + 2);
    g->g.Kg = d->kmax;
    g->g.koff = koff;
    g->g.lo_phys = g->prev < 0;
    g->g.hi_phys = g->next < 0;
    g->g.Ig = d->imax;
    g->g.Jg = d->jmax;
    if (cart) {
        g->g.ioff = loc.off[0];
        g->g.joff = loc.off[1];
        g->g.xlo_phys = loc.neighbours[0] < 0;
        g->g.xhi_phys = loc.neighbours[1] < 0;
        g->g.ylo_phys = loc.neighbours[2] < 0;
        g->g.yhi_phys = loc.neighbours[3] < 0;
        g->g.lo_phys = loc.neighbours[4] < 0;
        g->g.hi_phys = loc.neighbours[5] < 0;
        g->sweep = 0;     // the solve is the two colour passes
        g->resident = 0;
    }
    g->n = g->g.sxy * (kloc + 2);
    g->nalloc = g->g.sxy * (kloc + 2 * kHalo);
    // initSolver, solver.c:86-95
    g->dx = d->xlength / d->imax;
    g->dy = d->ylength / d->jmax;
    g->dz = d->zlength / d->kmax;
    {
        const double inv = 1.0 / (g->dx * g->dx) + 1.0 / (g->dy * g->dy) + 1.0 / (g->dz * g->dz);
        g->dt_bound = 0.5 * d->re * 1.0 / inv;  // solver.c:136-139
    }
    for (int b = 0; b < kBufs; ++b) {
        if (level_stream && b != MISOR3_P && b != MISOR3_RHS && b != kAlt) continue;
        const size_t bytes = sizeof(double) * (size_t)(g->nalloc + 2 * kSlack);
        if (hipMalloc(&g->alloc[b], bytes) != hipSuccess)
            CF(MISOR_ENOMEM, "hipMalloc of %lld doubles failed", g->nalloc);
        if (hipMemsetAsync(g->alloc[b], 0, bytes, g->stream) != hipSuccess)
            CF(MISOR_EHIP, "hipMemset failed");
        g->mem[b] = g->alloc[b] + kSlack;
        g->fld[b] = g->mem[b] + (long long)(kHalo - 1) * g->g.sxy;
    }
    g->partials_cap = 2LL * ns3_partials(g->g);
    if (g->partials_cap < 3LL * absmax3_blocks()) g->partials_cap = 3LL * absmax3_blocks();
    // the fused sweep's partials: the smallest rows / kchunk settings
    // (two sets: the folded loop test reads the previous sweep's partials)
    if (g->partials_cap < 2LL * sweep3_blocks(g->g, 4, 4))
        g->partials_cap = 2LL * sweep3_blocks(g->g, 4, 4);
    if (hipMalloc(&g->partials, sizeof(double) * (size_t)g->partials_cap) != hipSuccess ||
        hipMalloc(&g->out, sizeof(double) * 4) != hipSuccess ||
        hipHostMalloc(&g->out_host, sizeof(double) * 4, hipHostMallocDefault) != hipSuccess ||
        hipMalloc(&g->st, sizeof(DevState)) != hipSuccess ||
        hipMalloc(&g->st2, sizeof(DevState)) != hipSuccess ||
        hipHostMalloc(&g->st_host, sizeof(DevState), hipHostMallocDefault) != hipSuccess)
        CF(MISOR_ENOMEM, "allocation failed");
    if (cart) {
        // a send and a receive buffer per x / y side, each the size of its face
        // with the ghost rims: (nj+2)(nk+2) and (ni+2)(nk+2) doubles
        const size_t fx = (size_t)(jloc + 2) * (kloc + 2), fy = (size_t)(iloc + 2) * (kloc + 2);
        if (hipMalloc(&g->hbuf, sizeof(double) * 4 * (fx + fy)) != hipSuccess)
            CF(MISOR_ENOMEM, "allocation of the halo buffers failed");
        double* b = g->hbuf;
        for (int s = 0; s < 4; ++s) {
            const size_t f = s < 2 ? fx : fy;
            g->hsend[s] = b;
            g->hrecv[s] = b + f;
            b += 2 * f;
        }
    }
    if (nranks > 1) {
        // a multigrid level of an in-process group: a group of its own, whose
        // name every rank derives from the parent's group and the level
        char derived[MISOR_COMM_ID_BYTES + 1] = {};
        const void* id_bytes = d->comm_id;
        if (parent && parent->local) {
            if (snprintf(derived, sizeof derived, "%s/mg%d", parent->local_name, level) >=
                MISOR_COMM_ID_BYTES)
                CF(MISOR_EINVAL, "local group %s: name too long for its multigrid levels",
                   parent->local_name);
            id_bytes = derived;
        }
        char name[MISOR_COMM_ID_BYTES + 1] = {};
        const LocalJoin joined =
            (parent && !parent->local)
                ? LocalJoin::kNotLocal
                : join_local_group(id_bytes, nranks, g->rank, g, 4 * (size_t)nranks, g->local,
                                   name);
        if (joined == LocalJoin::kBadMember)
            CF(MISOR_EINVAL, "local group %s: bad rank/size", name);
        if (joined == LocalJoin::kJoined) {
            memcpy(g->local_name, name, sizeof name);
            g->local->barrier();  // every member registered before any exchange
        } else if (parent) {
            g->comm = parent->comm;
            g->own_comm = false;
        } else {
            ncclUniqueId id;
            memcpy(&id, d->comm_id, sizeof id);
            if (ncclCommInitRank(&g->comm, nranks, id, g->rank) != ncclSuccess)
                CF(MISOR_ECOMM, "ncclCommInitRank failed");
        }
    }
    if (hipStreamSynchronize(g->stream) != hipSuccess) CF(MISOR_EHIP, "sync failed");
#undef CF
    *out = g;
    return MISOR_OK;
}

int misor3_create(misor_grid3** out, const misor3_desc* d) {
    return create3(out, d, nullptr, false);
}

int misor3_create_cart(misor_grid3** out, const misor3_desc* d, const int dims[3]) {
    return create3(out, d, dims, true);
}

}  // extern "C"

int create3_level(misor_grid3** out, const misor3_desc* d, hipStream_t s) {
    return create3(out, d, nullptr, false, s);
}

int create3_level_slab(misor_grid3** out, const misor3_desc* d, misor_grid3* parent, int level) {
    return create3(out, d, nullptr, false, parent->stream, parent, level);
}

extern "C" {

int misor3_local_info(const misor_grid3* g, int* kloc, int* koff) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    if (kloc) *kloc = g->g.K;
    if (koff) *koff = g->g.koff;
    return MISOR_OK;
}

// one rank and slabs too: the block they hold on a 1 x 1 x nranks process grid
int misor3_local_info_cart(const misor_grid3* g, misor3_local* out) {
    if (!g || !out) return fail(MISOR_EINVAL, "null argument");
    if (g->cart) {
        *out = g->loc;
        return MISOR_OK;
    }
    *out = misor3_local{{g->g.I, g->g.J, g->g.K}, {0, 0, g->g.koff}, {0, 0, g->rank},
                        {1, 1, g->nranks}, {-1, -1, -1, -1, g->prev, g->next}};
    return MISOR_OK;
}

static double* fld3(misor_grid3* g, int field) {
    return (field >= 0 && field < 8) ? g->fld[field] : nullptr;
}

int misor3_exchange(misor_grid3* g, int field) {
    if (!g || !fld3(g, field)) return fail(MISOR_EINVAL, "bad exchange");
    HIPCHK(hipSetDevice(g->device));
    if (!dist(g)) return MISOR_OK;
    if (!g->cart)
        return fail(MISOR_ESTATE, "misor3_exchange needs a Cartesian grid (misor3_create_cart)");
    return exchange_cart(g, field, 7);
}

int misor3_upload(misor_grid3* g, int field, const double* host) {
    if (!g || !host || !fld3(g, field)) return fail(MISOR_EINVAL, "bad upload");
    HIPCHK(hipSetDevice(g->device));
    HIPCHK(hipMemcpyAsync(fld3(g, field), host, sizeof(double) * (size_t)g->n,
                          hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    if (field == MISOR3_P) g->alt_stale = true;
    return MISOR_OK;
}

int misor3_download(misor_grid3* g, int field, double* host) {
    if (!g || !host || !fld3(g, field)) return fail(MISOR_EINVAL, "bad download");
    HIPCHK(hipSetDevice(g->device));
    HIPCHK(hipMemcpyAsync(host, fld3(g, field), sizeof(double) * (size_t)g->n,
                          hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return MISOR_OK;
}

// commCollectResult's gather (assignment-6/src/comm.c:246-384) of one whole
// field: rank 0 receives (imax+2)(jmax+2)(kmax+2) doubles
int misor3_gather(misor_grid3* g, int field, double* host_global) {
    if (!g || !fld3(g, field)) return fail(MISOR_EINVAL, "bad gather");
    if (g->rank == 0 && !host_global) return fail(MISOR_EINVAL, "rank 0 needs a buffer");
    HIPCHK(hipSetDevice(g->device));
    if (!dist(g)) return misor3_download(g, field, host_global);
    return g->cart ? gather_cart(g, field, host_global) : gather_slabs(g, field, host_global);
}

int misor3_fill(misor_grid3* g, int field, double value) {
    if (!g || !fld3(g, field)) return fail(MISOR_EINVAL, "bad fill");
    HIPCHK(hipSetDevice(g->device));
    launch_fill(g->stream, g->mem[field], g->nalloc, value);
    HIPCHK(hipGetLastError());
    if (field == MISOR3_P) g->alt_stale = true;
    return MISOR_OK;
}

int misor3_set_dt(misor_grid3* g, double dt) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    g->dt = dt;
    return MISOR_OK;
}

// max |u|, |v|, |w| over every cell of the global array incl. ghosts: this
// rank's planes plus the physical ghost planes, then a max all-reduce
static int absmax_uvw(misor_grid3* g) {
    const int k_first = g->g.lo_phys ? 0 : 1, k_last = g->g.hi_phys ? g->g.K + 1 : g->g.K;
    const long long off = (long long)k_first * g->g.sxy;
    if (g->cart)  // owned cells and physical ghosts: no stale halo copy enters the maximum
        launch3_absmax_box(g->stream, g->fld[MISOR3_U], g->fld[MISOR3_V], g->fld[MISOR3_W],
                           own_box(g->loc), g->partials, g->out);
    else
        launch3_absmax(g->stream, g->fld[MISOR3_U] + off, g->fld[MISOR3_V] + off,
                       g->fld[MISOR3_W] + off, (long long)(k_last - k_first + 1) * g->g.sxy,
                       g->partials, g->out);
    HIPCHK(hipGetLastError());
    int rc = allreduce3(g, g->out, 3, true);
    if (rc != MISOR_OK) return rc;
    HIPCHK(hipMemcpyAsync(g->out_host, g->out, 3 * sizeof(double), hipMemcpyDeviceToHost,
                          g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return MISOR_OK;
}

// computeTimestep, solver.c:340-362 (maxElement over all cells incl. ghosts)
int misor3_compute_timestep(misor_grid3* g, double* dt_out) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    HIPCHK(hipSetDevice(g->device));
    int rc = absmax_uvw(g);
    if (rc != MISOR_OK) return rc;
    const double umax = g->out_host[0], vmax = g->out_host[1], wmax = g->out_host[2];
    double dt = g->dt_bound;
    if (umax > 0) dt = (dt > g->dx / umax) ? g->dx / umax : dt;
    if (vmax > 0) dt = (dt > g->dy / vmax) ? g->dy / vmax : dt;
    if (wmax > 0) dt = (dt > g->dz / wmax) ? g->dz / wmax : dt;
    g->dt = dt * g->desc.tau;
    if (dt_out) *dt_out = g->dt;
    return MISOR_OK;
}

int misor3_max_uvw(misor_grid3* g, double* mx /* 3 */) {
    if (!g || !mx) return fail(MISOR_EINVAL, "null argument");
    HIPCHK(hipSetDevice(g->device));
    int rc = absmax_uvw(g);
    if (rc != MISOR_OK) return rc;
    for (int q = 0; q < 3; ++q) mx[q] = g->out_host[q];
    return MISOR_OK;
}

// setBoundaryConditions, solver.c:364-577: top, bottom, left, right, front,
// back, in that order (a later wall reads cells an earlier one wrote); the
// front / back walls belong to the ranks holding the first / last plane
int misor3_set_boundary_conditions(misor_grid3* g) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    HIPCHK(hipSetDevice(g->device));
    const int I = g->g.I, J = g->g.J, K = g->g.K;
    double *u = g->fld[MISOR3_U], *v = g->fld[MISOR3_V], *w = g->fld[MISOR3_W];
    const misor3_desc& d = g->desc;
    // (a Cartesian block: only the walls on its physical sides, over its own cells)
    if (g->g.yhi_phys) launch3_wall(g->stream, g->g, v, u, w, 1, J + 1, J, J, J - 1, d.bcTop);
    if (g->g.ylo_phys) launch3_wall(g->stream, g->g, v, u, w, 1, 0, 1, 0, 1, d.bcBottom);
    if (g->g.xlo_phys) launch3_wall(g->stream, g->g, u, v, w, 0, 0, 1, 0, 1, d.bcLeft);
    if (g->g.xhi_phys) launch3_wall(g->stream, g->g, u, v, w, 0, I + 1, I, I, I - 1, d.bcRight);
    if (g->g.lo_phys) launch3_wall(g->stream, g->g, w, u, v, 2, 0, 1, 0, 1, d.bcFront);
    if (g->g.hi_phys) launch3_wall(g->stream, g->g, w, u, v, 2, K + 1, K, K, K - 1, d.bcBack);
    HIPCHK(hipGetLastError());
    return MISOR_OK;
}

int misor3_set_special_boundary_condition(misor_grid3* g) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    HIPCHK(hipSetDevice(g->device));
    launch3_special(g->stream, g->g, g->fld[MISOR3_U], g->desc.problem);
    HIPCHK(hipGetLastError());
    return MISOR_OK;
}

// computeFG reads u, v, w one plane beyond the slab: the reference's
// commExchange of u, v, w before it (assignment-6/src/solver.c:606-610)
int misor3_compute_fg(misor_grid3* g) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    HIPCHK(hipSetDevice(g->device));
    // (a Cartesian block: with the edge ghosts k3_fg reads, u[q-X+Y] and the like)
    for (int b : {MISOR3_U, MISOR3_V, MISOR3_W}) {
        int rc = g->cart ? exchange_cart(g, b, 7) : exchange3(g, b, 1);
        if (rc != MISOR_OK) return rc;
    }
    const misor3_desc& d = g->desc;
    Fg3 c;
    c.gamma = d.gamma;
    c.iRe = 1.0 / d.re;
    c.ix = 1.0 / g->dx;
    c.iy = 1.0 / g->dy;
    c.iz = 1.0 / g->dz;
    c.dt = g->dt;
    c.gx = d.gx;
    c.gy = d.gy;
    c.gz = d.gz;
    launch3_fg(g->stream, g->g, g->fld[MISOR3_U], g->fld[MISOR3_V], g->fld[MISOR3_W],
               g->fld[MISOR3_F], g->fld[MISOR3_G], g->fld[MISOR3_H], c);
    HIPCHK(hipGetLastError());
    return MISOR_OK;
}

// computeRHS reads h one plane below the slab (the reference's commShift)
int misor3_compute_rhs(misor_grid3* g) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    HIPCHK(hipSetDevice(g->device));
    int rc;
    if (g->cart) {  // f(0,j,k), g(i,0,k), h(i,j,0) next to a rank: f along x, g along y, h along z
        if ((rc = exchange_cart(g, MISOR3_F, 1)) != MISOR_OK) return rc;
        if ((rc = exchange_cart(g, MISOR3_G, 2)) != MISOR_OK) return rc;
        rc = exchange_cart(g, MISOR3_H, 4);
    } else {
        rc = exchange3(g, MISOR3_H, 1);
    }
    if (rc != MISOR_OK) return rc;
    launch3_rhs(g->stream, g->g, g->fld[MISOR3_F], g->fld[MISOR3_G], g->fld[MISOR3_H],
                g->fld[MISOR3_RHS], 1.0 / g->dx, 1.0 / g->dy, 1.0 / g->dz, 1.0 / g->dt);
    HIPCHK(hipGetLastError());
    return MISOR_OK;
}

int misor3_adapt_uvw(misor_grid3* g) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    HIPCHK(hipSetDevice(g->device));
    launch3_adapt(g->stream, g->g, g->fld[MISOR3_F], g->fld[MISOR3_G], g->fld[MISOR3_H],
                  g->fld[MISOR3_P], g->fld[MISOR3_U], g->fld[MISOR3_V], g->fld[MISOR3_W],
                  g->dt / g->dx, g->dt / g->dy, g->dt / g->dz);
    HIPCHK(hipGetLastError());
    return MISOR_OK;
}

int misor3_normalize_pressure(misor_grid3* g) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    HIPCHK(hipSetDevice(g->device));
    const double cells = (double)((long long)g->desc.imax * g->desc.jmax * g->desc.kmax);
    if (!dist(g)) {
        launch3_normalize(g->stream, g->g, g->fld[MISOR3_P], g->partials, g->out, cells);
    } else {
        launch3_interior_sum(g->stream, g->g, g->fld[MISOR3_P], g->partials, g->out);
        int rc = allreduce3(g, g->out, 1, false);
        if (rc != MISOR_OK) return rc;
        launch3_sub_mean(g->stream, g->g, g->fld[MISOR3_P], g->out, cells);
    }
    HIPCHK(hipGetLastError());
    return MISOR_OK;
}

int misor3_set_tuning(misor_grid3* g, int key, int value) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    switch (key) {
    case MISOR3_TUNE_SWEEP:
        if (value != 0 && value != 1) return fail(MISOR_EINVAL, "sweep must be 0 or 1");
        if (g->cart) {
            if (value == 1)
                return fail(MISOR_EINVAL,
                            "the fused sweep does not run on a Cartesian process grid");
            return MISOR_OK;
        }
        if (value == 0 && dist(g))
            return fail(MISOR_EINVAL, "the two-pass solve is single-rank only");
        g->sweep = value;
        return MISOR_OK;
    case MISOR3_TUNE_ROWS:
        if (value != 4 && value != 8 && value != 12)
            return fail(MISOR_EINVAL, "rows must be 4, 8 or 12");
        g->rows = value;
        return MISOR_OK;
    case MISOR3_TUNE_KCHUNK:
        if (value != 0 && value < 4) return fail(MISOR_EINVAL, "kchunk must be 0 or >= 4");
        g->kchunk = value;
        return MISOR_OK;
    case MISOR3_TUNE_FOLD: g->fold = value != 0; return MISOR_OK;
    case MISOR3_TUNE_RHS_AHEAD:
        if (value < 0 || value > 2) return fail(MISOR_EINVAL, "rhs_ahead must be 0, 1 or 2");
        g->rhs_ahead = value;
        return MISOR_OK;
    case MISOR3_TUNE_RESIDENT:
        if (value < -1 || value > 1) return fail(MISOR_EINVAL, "resident must be -1, 0 or 1");
        if (g->cart) {
            if (value == 1)
                return fail(MISOR_EINVAL,
                            "the resident solve does not run on a Cartesian process grid");
            return MISOR_OK;
        }
        g->resident = value;
        return MISOR_OK;
    }
    return fail(MISOR_EINVAL, "unknown tuning key %d", key);
}

int misor3_get_tuning(const misor_grid3* g, int key, int* value) {
    if (!g || !value) return fail(MISOR_EINVAL, "null argument");
    switch (key) {
    case MISOR3_TUNE_SWEEP: *value = g->sweep; return MISOR_OK;
    case MISOR3_TUNE_ROWS: *value = g->rows; return MISOR_OK;
    case MISOR3_TUNE_KCHUNK:
        *value = g->kchunk > 0 ? g->kchunk : auto_kchunk(g->g, g->rows);
        return MISOR_OK;
    case MISOR3_TUNE_FOLD: *value = g->fold; return MISOR_OK;
    case MISOR3_TUNE_RHS_AHEAD: *value = g->rhs_ahead; return MISOR_OK;
    case MISOR3_TUNE_RESIDENT:
        *value = !dist(g) && g->resident != 0 && resident3_boxes(g->g) > 0;
        return MISOR_OK;
    }
    return fail(MISOR_EINVAL, "unknown tuning key %d", key);
}

int misor3_enable_timing(misor_grid3* g, int on) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    HIPCHK(hipSetDevice(g->device));
    if (on && !g->ev[0])
        for (auto& e : g->ev) HIPCHK(hipEventCreate(&e));
    g->timing = on != 0;
    g->solve_ms = 0;
    g->solve_iters = 0;
    g->mg_info.transfer_ms[0] = g->mg_info.transfer_ms[1] = 0;
    g->mg_info.transfers = 0;
    return MISOR_OK;
}

int misor3_get_solve_time(const misor_grid3* g, double* ms, long long* iters) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    if (ms) *ms = g->solve_ms;
    if (iters) *iters = g->solve_iters;
    return MISOR_OK;
}

int misor3_synchronize(misor_grid3* g) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    HIPCHK(hipStreamSynchronize(g->stream));
    return MISOR_OK;
}

}  // extern "C"
