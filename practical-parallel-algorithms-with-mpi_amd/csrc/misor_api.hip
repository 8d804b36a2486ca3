// misor_api.hip -- the C ABI of include/misor.h, part 1: errors, grid lifecycle
// (create / destroy, streams), transfers (upload / download / exchange / fill /
// Poisson init, and gather's entry), tuning and statistics.  The decomposition
// arithmetic is in decomp2.h, the solve loop in misor_solve.hip, the NS step in
// misor_ns.hip, communication (gather's transport too) in misor_comm.hip,
// launch plans in tb_plan.h (their device side in misor_plan.hip); their
// shared state is struct misor_grid (misor_grid.h).

#include "misor_grid.h"

namespace {
thread_local std::string g_err;
}  // namespace

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

void misor::set_last_error(const char* msg) { g_err = msg; }

const char* misor_last_error(void) { return g_err.c_str(); }
const char* misor_version(void) { return "misor 0.1 (gfx950, fp64 red-black SOR)"; }

// the decomposition itself is in decomp2.h; the row pitch is the device layout's
int misor_decompose(int nranks, int rank, int imax, int jmax, const int dims_in[2],
                    misor_local* out) {
    char err[kDecompErr];
    const int rc = decompose2(nranks, rank, imax, jmax, dims_in, out, err);
    if (rc != MISOR_OK) return fail(rc, "%s", err);
    out->pitch = layout_pitch(out->ni);
    return MISOR_OK;
}

int misor_comm_unique_id(void* id_out) {
    if (!id_out) return fail(MISOR_EINVAL, "null id");
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    static_assert(sizeof(ncclUniqueId) == MISOR_COMM_ID_BYTES, "ncclUniqueId size");
    memcpy(id_out, &id, sizeof id);
    return MISOR_OK;
}

SorConsts sor_consts(double dx, double dy, double omega, int variant) {
    const double dx2 = dx * dx, dy2 = dy * dy;
    SorConsts c{};
    c.idx2 = 1.0 / dx2;
    c.idy2 = 1.0 / dy2;
    if (variant == MISOR_SOLVE_RBA) {
        const double factor = 0.5 * (dx2 * dy2) / (dx2 + dy2);  // solver.c:250
        c.coef = omega * factor;                                // (omega*factor)*r, :273
    } else {
        c.coef = omega * 0.5 * (dx2 * dy2) / (dx2 + dy2);  // solver.c:189
    }
    return c;
}

double near_band_rel(int value) { return value >= 300 ? 0.0 : pow(10.0, -(double)value); }

void misor_destroy(misor_grid* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    mg_free(g);  // the multigrid levels (they run on this grid's stream)
    for (auto& f : g->fld)
        if (f) (void)hipFree(f);
    (void)hipFree(g->partials);
    (void)hipFree(g->tb_queue);
    (void)hipFree(g->lex_work.buf);
    for (auto& v : g->chain_plan)
        for (auto& row : v)
            for (auto& pl : row) {
                (void)hipFree(pl.main.tmpl);
                (void)hipFree(pl.edge.tmpl);
            }
    for (int* w : g->tb_work) (void)hipFree(w);
    for (int k = 0; k < 2; ++k) {
        if (g->xstream[k]) {
            (void)hipStreamSynchronize(g->xstream[k]);
            (void)hipStreamDestroy(g->xstream[k]);
        }
        if (g->ev_fork[k]) (void)hipEventDestroy(g->ev_fork[k]);
        if (g->ev_join[k]) (void)hipEventDestroy(g->ev_join[k]);
    }
    (void)hipFree(g->chain_trace);
    (void)hipFree(g->st);
    (void)hipHostFree(g->st_host);
    (void)hipFree(g->red_partials);
    (void)hipFree(g->max_partials);
    (void)hipFree(g->red_out);
    (void)hipHostFree(g->red_host);
    (void)hipFree(g->sendbuf);
    (void)hipFree(g->recvbuf);
    (void)hipFree(g->gbuf);
    (void)hipFree(g->rsq);
    if (g->cstream) (void)hipStreamSynchronize(g->cstream);
    if (g->cstream) (void)hipStreamDestroy(g->cstream);
    for (int b = 0; b < 2; ++b) {
        if (g->ev_i[b]) (void)hipEventDestroy(g->ev_i[b]);
        if (g->ev_dk[b]) (void)hipEventDestroy(g->ev_dk[b]);
        if (g->ev_e2[b]) (void)hipEventDestroy(g->ev_e2[b]);
    }
    if (g->ev_s) (void)hipEventDestroy(g->ev_s);
    if (g->ev_x) (void)hipEventDestroy(g->ev_x);
    for (auto e : g->ev) (void)hipEventDestroy(e);
    for (auto& v : g->cev)
        for (auto e : v) (void)hipEventDestroy(e);
    for (auto& v : g->nev)
        for (auto e : v) (void)hipEventDestroy(e);
    for (hipEvent_t e : {g->lx_pk, g->lx_cp, g->la_val[0], g->la_val[1], g->la_rd[0], g->la_rd[1],
                         g->la_cmb[0], g->la_cmb[1], g->ag_pk, g->ag_cp})
        if (e) (void)hipEventDestroy(e);
    (void)hipFree(g->la_stage);
    (void)hipFree(g->la_gather);
    (void)hipFree(g->ag_send);
    (void)hipFree(g->ag_recv);
    if (g->comm && !g->comm_owner) ncclCommDestroy(g->comm);
    if (g->own_stream && g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
}


int misor_create(misor_grid** out, const misor_desc* d) { return grid_create(out, d, false); }

// grid_create's steps.  Each records its message through fail() and returns
// its code; grid_create destroys the half-built grid.

// the sweep's and the temporally blocked pass's geometry from the local block
// and the desc
static int set_geometry(misor_grid* g) {
    const misor_desc* d = &g->desc;
    const misor_local& L = g->loc;
    SweepParams& sp = g->sp;
    sp.pitch = g->pitch;
    sp.ni = L.ni;
    sp.nj = L.nj;
    sp.parity = (L.ioff + L.joff) & 1;
    sp.ghost_left = L.neighbours[0] < 0;
    sp.ghost_right = L.neighbours[1] < 0;
    sp.ghost_bottom = L.neighbours[2] < 0;
    sp.ghost_top = L.neighbours[3] < 0;
    sp.red_lo_i = sp.ghost_left ? 1 : 0;
    sp.red_hi_i = sp.ghost_right ? L.ni : L.ni + 1;
    sp.red_lo_j = sp.ghost_bottom ? 1 : 0;
    sp.red_hi_j = sp.ghost_top ? L.nj : L.nj + 1;
    const SorConsts sc = sor_consts(d->dx, d->dy, d->omega, d->variant);
    sp.idx2 = sc.idx2;
    sp.idy2 = sc.idy2;
    sp.coef = sc.coef;
    {
        // power-of-two spacing (sor_tb.h resid<true>): 1/dx^2 == 1/dy^2 == 2^m, m >= 0
        int e = 0;
        const double mant = frexp(sp.idx2, &e);
        sp.pow2 = sp.idx2 == sp.idy2 && mant == 0.5 && e >= 1;
    }
    if (configure_sweep(g, kDefaultSweepVariant, 0, 1) != MISOR_OK) return MISOR_ENOMEM;
    // the temporally blocked pass: the same physics, the bounds of tb_plan.h
    g->tp = sp;
    tb_bounds(g->tp);
    if (g->dist) sweep_interior_bounds(sp);
    return MISOR_OK;
}

// the loop state and the reduction buffers
static int alloc_state(misor_grid* g) {
    if (hipMalloc(&g->tb_queue, 16 * sizeof(int)) != hipSuccess ||
        hipMemsetAsync(g->tb_queue, 0, 16 * sizeof(int), g->stream) != hipSuccess ||
        hipMalloc(&g->st, sizeof(DevState)) != hipSuccess ||
        hipHostMalloc(&g->st_host, sizeof(DevState), hipHostMallocDefault) != hipSuccess)
        return fail(MISOR_ENOMEM, "state allocation failed");
    const int rb = reduce_blocks(g->loc.ni, g->loc.nj);
    if (hipMalloc(&g->red_partials, sizeof(double) * 2 * rb) != hipSuccess ||
        hipMalloc(&g->max_partials, sizeof(double) * 2 * rb) != hipSuccess ||
        hipMalloc(&g->red_out, sizeof(double) * 4) != hipSuccess ||
        hipHostMalloc(&g->red_host, sizeof(double) * 4, hipHostMallocDefault) != hipSuccess)
        return fail(MISOR_ENOMEM, "reduction allocation failed");
    return MISOR_OK;
}

// a decomposed grid's transport: neighbour table, halo plans, communication
// stream and events, halo buffers, and the in-process group or RCCL
static int comm_setup(misor_grid* g, bool proxy, misor_grid* parent, int level) {
    const misor_desc* d = &g->desc;
    const misor_local& L = g->loc;
    if (!d->comm_id && !parent) return fail(MISOR_EINVAL, "nranks > 1 needs comm_id");
    neighbours8(L.dims, L.coords, g->nbr);
    if (proxy) {  // (MISOR_PROXY_SIDES: every neighbour is rank 0; corners where both sides have one)
        const int* nb = L.neighbours;
        const int pn[kDirs] = {nb[0], nb[1], nb[2], nb[3],
                               nb[0] >= 0 && nb[2] >= 0 ? 0 : -1,
                               nb[1] >= 0 && nb[2] >= 0 ? 0 : -1,
                               nb[0] >= 0 && nb[3] >= 0 ? 0 : -1,
                               nb[1] >= 0 && nb[3] >= 0 ? 0 : -1};
        for (int k = 0; k < kDirs; ++k) g->nbr[k] = pn[k];
    }
    // halo plans up to depth 2*kMaxT + 1 (the skewed split ring's), as deep
    // as the smallest block allows
    g->max_depth = max_halo_depth(d->imax, d->jmax, L.dims);
    long long maxtot = 1;
    for (int dd = 1; dd <= g->max_depth; ++dd) {
        g->plan[dd] = halo_plan(L.ni, L.nj, g->nbr, dd);
        maxtot = std::max(maxtot, g->plan[dd].total);
    }
    // communication and edge blocks at high priority: their workgroups are
    // dispatched ahead of queued interior blocks as slots free up
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    bool ok = hipStreamCreateWithPriority(&g->cstream, hipStreamNonBlocking, prio_hi) ==
              hipSuccess;
    for (hipEvent_t* e : {&g->ev_s, &g->ev_x, &g->ev_i[0], &g->ev_i[1], &g->ev_e2[0],
                          &g->ev_e2[1], &g->ev_dk[0], &g->ev_dk[1]})
        ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    if (!ok) return fail(MISOR_EHIP, "comm stream/event creation failed");
    const size_t hb = (size_t)maxtot * sizeof(double);
    if (hipMalloc(&g->sendbuf, hb) != hipSuccess || hipMalloc(&g->recvbuf, hb) != hipSuccess)
        return fail(MISOR_ENOMEM, "halo buffer allocation failed");
    char name[MISOR_COMM_ID_BYTES + 1];
    // a multigrid level of an in-process group: a group of its own, whose name
    // every rank derives from the parent's group and the level
    char derived[MISOR_COMM_ID_BYTES + 1] = {};
    const void* id = d->comm_id;
    if (parent && parent->local) {
        if (snprintf(derived, sizeof derived, "%s/mg%d", parent->local_name, level) >=
            MISOR_COMM_ID_BYTES)
            return fail(MISOR_EINVAL, "local group %s: name too long for its multigrid levels",
                        parent->local_name);
        id = derived;
    } else if (parent) {
        g->comm = parent->comm;
        g->comm_owner = parent->comm_owner ? parent->comm_owner : parent;
        if (!g->comm) return fail(MISOR_ECOMM, "the communicator was aborted by an earlier error");
        return MISOR_OK;
    }
    // (no host scratch: this all-reduce stages on the device, la_stage / la_gather)
    const LocalJoin joined = join_local_group(id, d->nranks, d->rank, g, 0, g->local, name);
    if (joined == LocalJoin::kBadMember)
        return fail(MISOR_EINVAL, "local group %s: bad rank/size", name);
    if (joined == LocalJoin::kJoined) {
        memcpy(g->local_name, name, sizeof name);
        bool lok = hipMalloc(&g->la_stage, sizeof(double) * 2 * kMaxT) == hipSuccess &&
                   hipMalloc(&g->la_gather, sizeof(double) * 2 * kMaxT * (size_t)d->nranks) ==
                       hipSuccess;
        for (hipEvent_t* e : {&g->lx_pk, &g->lx_cp, &g->la_val[0], &g->la_val[1],
                              &g->la_rd[0], &g->la_rd[1], &g->la_cmb[0], &g->la_cmb[1],
                              &g->ag_pk, &g->ag_cp})
            lok = lok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
        g->local->barrier();  // every member registered before any exchange
        if (!lok) return fail(MISOR_EHIP, "in-process transport allocation failed");
    } else {
        ncclUniqueId id;
        memcpy(&id, d->comm_id, sizeof id);
        if (ncclCommInitRank(&g->comm, d->nranks, id, d->rank) != ncclSuccess)
            return fail(MISOR_ECOMM, "ncclCommInitRank failed");
    }
    return MISOR_OK;
}

int grid_create(misor_grid** out, const misor_desc* d, bool poisson_only, misor_grid* comm_parent,
                int level) {
    if (!out || !d) return fail(MISOR_EINVAL, "null argument");
    *out = nullptr;
    if (d->imax < 2 || d->jmax < 2) return fail(MISOR_EINVAL, "imax, jmax must be >= 2");
    if (!(d->dx > 0) || !(d->dy > 0)) return fail(MISOR_EINVAL, "dx, dy must be > 0");
    const int nranks = d->nranks < 1 ? 1 : d->nranks;
    misor_local L{};
    int rc = misor_decompose(nranks, nranks == 1 ? 0 : d->rank, d->imax, d->jmax, d->dims, &L);
    if (rc) return rc;
    // Measurement proxy, in an experiment build only (make ab B=build_proxy
    // L=lib_proxy XFLAGS=-DMISOR_PROXY; tools/scale_proxy.py --sides): one rank
    // on a one-rank communicator whose sides NOT named in MISOR_PROXY_SIDES (of
    // "LRBT") are treated as bordering another rank -- rank 0 itself: the
    // exchange sends each halo region to itself, sizes matching, contents
    // meaningless -- so the block runs the pass loop of a rank of a larger
    // decomposition (split launches, 2T-deep halo cones, exchanges, all-reduce)
    // on one GPU.  Timing only: the field it computes is not the reference's,
    // so misor_download / misor_gather refuse it (MISOR_ESTATE).
    bool proxy = false;
#ifdef MISOR_PROXY
    if (nranks == 1 && d->comm_id) {
        const char* ps = getenv("MISOR_PROXY_SIDES");
        if (ps) {
            proxy = true;
            const char* sides = "LRBT";
            for (int k = 0; k < 4; ++k)
                if (!strchr(ps, sides[k])) L.neighbours[k] = 0;
        }
    }
#endif

    misor_grid* g = new misor_grid();
#ifdef MISOR_PROXY
    g->proxy = proxy;
#endif
    g->desc = *d;
    g->desc.nranks = nranks;
    g->loc = L;
    // a comm id with nranks == 1 still runs the decomposed code path (one rank, no
    // neighbours): lets the RCCL / overlap machinery be exercised on one GPU
    g->dist = nranks > 1 || d->comm_id != nullptr || comm_parent != nullptr;
    g->np = g->dist ? 3 : 2;
    if (d->device >= 0) {
        g->device = d->device;
        if (hipSetDevice(g->device) != hipSuccess) {
            delete g;
            return fail(MISOR_EHIP, "hipSetDevice(%d) failed", d->device);
        }
    } else {
        (void)hipGetDevice(&g->device);
    }
#define CREATE_FAIL(code, ...)          \
    do {                                \
        int c_ = fail(code, __VA_ARGS__); \
        misor_destroy(g);               \
        return c_;                      \
    } while (0)
#define CREATE_STEP(x)        \
    do {                      \
        const int c_ = (x);   \
        if (c_) {             \
            misor_destroy(g); \
            return c_;        \
        }                     \
    } while (0)
    if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess)
        CREATE_FAIL(MISOR_EHIP, "hipStreamCreate failed");
    g->own_stream = true;

    g->pitch = layout_pitch(L.ni);
    g->rows = layout_rows(L.nj);
    g->elems = g->pitch * g->rows;
    for (int k = 0; k < kNumFields; ++k) {
        if (k == kP2 && g->np < 3) continue;
        if (poisson_only && (k == kU || k == kV || k == kF || k == kG)) continue;
        if (hipMalloc(&g->fld[k], (size_t)g->elems * sizeof(double)) != hipSuccess)
            CREATE_FAIL(MISOR_ENOMEM, "hipMalloc of %lld doubles failed", g->elems);
        if (hipMemsetAsync(g->fld[k], 0, (size_t)g->elems * sizeof(double), g->stream) !=
            hipSuccess)
            CREATE_FAIL(MISOR_EHIP, "hipMemset failed");
    }
    CREATE_STEP(set_geometry(g));
    CREATE_STEP(alloc_state(g));
    if (g->dist) CREATE_STEP(comm_setup(g, proxy, comm_parent, level));
    if (configure_tb(g, default_tsteps(tb_input(g), kDefaultTbVariant), kDefaultTbVariant, 0) !=
        MISOR_OK)
        CREATE_FAIL(MISOR_ENOMEM, "%s", g_err.c_str());
    if (hipStreamSynchronize(g->stream) != hipSuccess)
        CREATE_FAIL(MISOR_EHIP, "hipStreamSynchronize failed");
#undef CREATE_STEP
#undef CREATE_FAIL
    *out = g;
    return MISOR_OK;
}

int misor_local_info(const misor_grid* g, misor_local* out) {
    if (!g || !out) return fail(MISOR_EINVAL, "null argument");
    *out = g->loc;
    return MISOR_OK;
}

int misor_set_stream(misor_grid* g, void* s) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    HIPCHK(hipSetDevice(g->device));
    HIPCHK(hipStreamSynchronize(g->stream));
    hipStream_t next = (hipStream_t)s;
    if (!s) HIPCHK(hipStreamCreateWithFlags(&next, hipStreamNonBlocking));
    // the multigrid levels run on this grid's stream: they move to the new one
    // while the old one still exists
    const int rc = mg_set_stream(g, next);
    if (rc) {
        if (!s) (void)hipStreamDestroy(next);
        return rc;
    }
    if (g->own_stream) HIPCHK(hipStreamDestroy(g->stream));
    g->stream = next;
    g->own_stream = !s;
    g->nl.s = g->stream;
    return MISOR_OK;
}

int misor_synchronize(misor_grid* g) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    MISOR_TRY(wait_stream(g, g->stream));
    return MISOR_OK;
}

static double* field_ptr(misor_grid* g, int field) {
    switch (field) {
    case MISOR_P: return pbuf(g, g->cur);
    case MISOR_RHS: return g->fld[kRhs];
    case MISOR_U: return g->fld[kU];
    case MISOR_V: return g->fld[kV];
    case MISOR_F: return g->fld[kF];
    case MISOR_G: return g->fld[kG];
    default: return nullptr;
    }
}

// `field` was written from outside (upload, fill, initialisation, adoption):
// what the grid derived from its old contents no longer holds.  A write of P
// goes to every pressure buffer -- corners and ghosts must agree, and its halo
// is the caller's -- so the first one is current again.
static void note_write(misor_grid* g, int field) {
    if (field == MISOR_RHS) g->rhs_halo = 0;
    if (field == MISOR_U || field == MISOR_V) ++g->uv_ver;
    if (field == MISOR_F || field == MISOR_G || field == MISOR_RHS) ++g->fgr_ver;
    if (field == MISOR_P) {
        g->cur = 0;
        g->p_stale = false;
    }
}

int misor_upload(misor_grid* g, int field, const double* host) {
    if (!g || !host || !field_ptr(g, field)) return fail(MISOR_EINVAL, "bad upload");
    HIPCHK(hipSetDevice(g->device));
    const size_t w = (size_t)(g->loc.ni + 2) * sizeof(double);
    const size_t h = (size_t)(g->loc.nj + 2);
    note_write(g, field);
    if (field == MISOR_P) {
        for (int b = 0; b < g->np; ++b)
            HIPCHK(hipMemcpy2DAsync(origin(g, pbuf(g, b)), g->pitch * sizeof(double), host,
                                    w, w, h, hipMemcpyHostToDevice, g->stream));
    } else {
        HIPCHK(hipMemcpy2DAsync(origin(g, field_ptr(g, field)), g->pitch * sizeof(double), host,
                                w, w, h, hipMemcpyHostToDevice, g->stream));
    }
    HIPCHK(hipStreamSynchronize(g->stream));
    return MISOR_OK;
}

// A single-rank grid takes over one problem of its own shape that already lies
// on the device in the padded layout (a member of a misor_batch): what
// misor_create derives from omega, eps and itermax, then p and rhs as
// misor_upload leaves them.  Enqueued on the grid's stream.
int grid_adopt(misor_grid* g, const double* p_dev, const double* rhs_dev, double omega, double eps,
               int itermax) {
    g->desc.omega = omega;
    g->desc.eps = eps;
    g->desc.itermax = itermax;
    g->sp.coef = g->tp.coef = sor_consts(g->desc.dx, g->desc.dy, omega, g->desc.variant).coef;
    const size_t bytes = (size_t)g->elems * sizeof(double);
    note_write(g, MISOR_P);
    note_write(g, MISOR_RHS);
    for (int b = 0; b < g->np; ++b)
        HIPCHK(hipMemcpyAsync(pbuf(g, b), p_dev, bytes, hipMemcpyDeviceToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(g->fld[kRhs], rhs_dev, bytes, hipMemcpyDeviceToDevice, g->stream));
    return MISOR_OK;
}

#ifdef MISOR_PROXY
#define PROXYCHK(g)                                                                       \
    do {                                                                                   \
        if ((g)->proxy)                                                                    \
            return fail(MISOR_ESTATE, "a MISOR_PROXY_SIDES grid holds no meaningful field"); \
    } while (0)
#else
#define PROXYCHK(g) \
    do {            \
    } while (0)
#endif

int misor_download(misor_grid* g, int field, double* host) {
    if (!g || !host || !field_ptr(g, field)) return fail(MISOR_EINVAL, "bad download");
    PROXYCHK(g);
    HIPCHK(hipSetDevice(g->device));
    if (field == MISOR_P) {  // the local block with a consistent halo
        int rc = p_halo(g);
        if (rc) return rc;
    }
    const size_t w = (size_t)(g->loc.ni + 2) * sizeof(double);
    const size_t h = (size_t)(g->loc.nj + 2);
    HIPCHK(hipMemcpy2DAsync(host, w, origin(g, field_ptr(g, field)), g->pitch * sizeof(double), w,
                            h, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return MISOR_OK;
}

int misor_gather(misor_grid* g, int field, double* host) {
    if (!g || !field_ptr(g, field)) return fail(MISOR_EINVAL, "bad gather");
    PROXYCHK(g);
    const int rank = g->dist ? g->desc.rank : 0;
    if (rank == 0 && !host) return fail(MISOR_EINVAL, "gather: rank 0 needs the global array");
    if (g->desc.nranks == 1) return misor_download(g, field, host);
    return gather(g, field_ptr(g, field), host);
}

int misor_exchange(misor_grid* g, int field, int depth) {
    if (!g || !field_ptr(g, field)) return fail(MISOR_EINVAL, "bad exchange");
    if (!g->dist) return MISOR_OK;
    if (depth < 1 || depth > g->max_depth)
        return fail(MISOR_EINVAL, "exchange depth %d outside 1..%d", depth, g->max_depth);
    HIPCHK(hipSetDevice(g->device));
    int rc = exchange(g, field_ptr(g, field), depth);
    if (rc) return rc;
    if (field == MISOR_RHS) g->rhs_halo = std::max(g->rhs_halo, depth);  // now fresh to depth
    if (field == MISOR_P && depth >= 2) g->p_stale = false;
    return wait_stream(g, g->stream);
}

int misor_device_count(int* n) {
    if (!n) return fail(MISOR_EINVAL, "null argument");
    HIPCHK(hipGetDeviceCount(n));
    return MISOR_OK;
}

int misor_comm_ranks(const misor_grid* g, int* n) {
    if (!g || !n) return fail(MISOR_EINVAL, "null argument");
    if (g->comm) {
        NCCLCHK(ncclCommCount(g->comm, n));
    } else if (g->local) {
        *n = g->local->n;
    } else if (g->comm_dead) {
        return fail(MISOR_ECOMM, "the communicator was aborted by an earlier error");
    } else {
        *n = 1;
    }
    return MISOR_OK;
}

int misor_fill(misor_grid* g, int field, double value) {
    if (!g || !field_ptr(g, field)) return fail(MISOR_EINVAL, "bad fill");
    HIPCHK(hipSetDevice(g->device));
    // whole padded array: ghosts included, pads too (pads never feed results)
    note_write(g, field);
    if (field == MISOR_P) {
        for (int b = 0; b < g->np; ++b) launch_fill(g->stream, pbuf(g, b), g->elems, value);
    } else {
        launch_fill(g->stream, field_ptr(g, field), g->elems, value);
    }
    HIPCHK(hipGetLastError());
    return MISOR_OK;
}

std::vector<double> poisson_tables(const misor_local& loc, int imax, int jmax, double xlength,
                                   double ylength) {
    const int ni = loc.ni, nj = loc.nj;
    const double PI = 3.14159265358979323846;  // assignment-4/src/solver.c:15
    const double dx = xlength / imax, dy = ylength / jmax;
    // host tables with the reference's exact expressions (solver.c:107,114)
    std::vector<double> tab((size_t)(2 * (ni + 2) + (nj + 2)));
    double *sx = tab.data(), *rx = sx + (ni + 2), *sy = rx + (ni + 2);
    for (int i = 0; i < ni + 2; ++i) {
        const int gi = loc.ioff + i;
        sx[i] = sin(2.0 * PI * gi * dx * 2.0);
        rx[i] = sin(2.0 * PI * gi * dx);
    }
    for (int j = 0; j < nj + 2; ++j) sy[j] = sin(2.0 * PI * (loc.joff + j) * dy * 2.0);
    return tab;
}

int misor_poisson_init(misor_grid* g, double xlength, double ylength, int problem) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    HIPCHK(hipSetDevice(g->device));
    const int ni = g->loc.ni, nj = g->loc.nj;
    const std::vector<double> host =
        poisson_tables(g->loc, g->desc.imax, g->desc.jmax, xlength, ylength);
    double* tab = nullptr;
    HIPCHK(hipMalloc(&tab, host.size() * sizeof(double)));
    HIPCHK(hipMemcpyAsync(tab, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice,
                          g->stream));
    note_write(g, MISOR_P);
    note_write(g, MISOR_RHS);
    for (int b = 0; b < g->np; ++b)
        launch_poisson_init(g->stream, pbuf(g, b), g->fld[kRhs], tab, tab + 2 * (ni + 2),
                            tab + (ni + 2), ni, nj, g->pitch, problem);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g->stream));
    HIPCHK(hipFree(tab));
    return MISOR_OK;
}


int misor_enable_timing(misor_grid* g, int on) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    g->timing = on != 0;
    return MISOR_OK;
}

int misor_get_stats(const misor_grid* g, misor_stats* out) {
    if (!g || !out) return fail(MISOR_EINVAL, "null argument");
    {
        misor_grid* gm = const_cast<misor_grid*>(g);  // (pending NS kernel timings)
        HIPCHK(hipSetDevice(gm->device));
        int rc = collect_ns_times(gm);
        if (rc) return rc;
    }
    *out = g->stats;
    return MISOR_OK;
}

int misor_set_tuning(misor_grid* g, int key, int value) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    switch (key) {
    case MISOR_TUNE_SWEEP_VARIANT:
        return configure_sweep(g, value, g->sp.rows_per_block, g->sp.xcd_remap);
    case MISOR_TUNE_ROWS_PER_BLOCK:
        return configure_sweep(g, g->sp.variant, value, g->sp.xcd_remap);
    case MISOR_TUNE_XCD_REMAP:
        return configure_sweep(g, g->sp.variant, g->sp.rows_per_block, value != 0);
    case MISOR_TUNE_SMALL_SOLVE: g->small_solve = value != 0; return MISOR_OK;
    case MISOR_TUNE_OVERLAP: g->overlap = value != 0; return MISOR_OK;
    case MISOR_TUNE_TSTEPS: {
        // an explicit request binds: every pass runs T = value iterations (no
        // short plan, no re-pick by MISOR_TUNE_TB_CHAIN); value <= 0 returns
        // to the default rule.  A rejected request changes nothing.
        const bool prev = g->tsteps_set;
        g->tsteps_set = value > 0;
        const int T = value > 0 ? value : default_tsteps(tb_input(g), g->tp.variant);
        const int rc = configure_tb(g, T, g->tp.variant, g->tb_rows_req);
        if (rc) g->tsteps_set = prev;
        return rc;
    }
    case MISOR_TUNE_TB_VARIANT: return configure_tb(g, g->tsteps, value, g->tb_rows_req);
    case MISOR_TUNE_TB_ROWS: return configure_tb(g, g->tsteps, g->tp.variant, value);
    case MISOR_TUNE_TB_PERSISTENT: {
        const bool prev = g->tb_persistent;  // (a rejected request changes nothing)
        g->tb_persistent = value != 0;
        const int rc = configure_tb(g, g->tsteps, g->tp.variant, g->tb_rows_req);
        if (rc) g->tb_persistent = prev;
        return rc;
    }
    case MISOR_TUNE_TB_CHAIN:
        // without an explicit T request the default rule re-picks T (chained
        // small blocks run T = 8, unchained ones T = 7)
        g->tb_chain = value < 0 ? -1 : value != 0;
        return configure_tb(g,
                            g->tsteps_set ? g->tsteps : default_tsteps(tb_input(g), g->tp.variant),
                            g->tp.variant, g->tb_rows_req);
    case MISOR_TUNE_NS_FUSE: g->ns_fuse = value != 0; return MISOR_OK;
    case MISOR_TUNE_FINISH2: g->finish2 = value != 0; return MISOR_OK;
    case MISOR_TUNE_TB_RESERVE:
        if (value < 0) return fail(MISOR_EINVAL, "reserve must be >= 0");
        g->tb_reserve = value;
        drop_chain_plans(g);  // (the one-list plans count the workgroups left)
        return MISOR_OK;
    case MISOR_TUNE_NEAR_BAND:
        g->near_exp = value;
        g->near_rel = near_band_rel(value);
        return MISOR_OK;
    case MISOR_TUNE_RES_LITE:
        if (value != 0 && value != 1) return fail(MISOR_EINVAL, "RES_LITE is 0 or 1");
        g->res_lite = value != 0;
        return MISOR_OK;
    case MISOR_TUNE_EDGE_STEAL:
        if (value < 0 || value > 2) return fail(MISOR_EINVAL, "EDGE_STEAL is 0, 1 or 2");
        g->edge_steal = value;
        return MISOR_OK;
    case MISOR_TUNE_LEX_TILED:
        if (value < -1 || value > 1) return fail(MISOR_EINVAL, "LEX_TILED is -1, 0 or 1");
        g->lex_tiled = value;
        return MISOR_OK;
    case MISOR_TUNE_LEX_TILE_W:
    case MISOR_TUNE_LEX_TILE_H: {
        // the pair must fit (with the other at its current value); a rejected
        // request changes nothing
        const int v = value > 0 ? value : 0;
        const int tw = key == MISOR_TUNE_LEX_TILE_W ? v : g->lex_tw;
        const int th = key == MISOR_TUNE_LEX_TILE_H ? v : g->lex_th;
        if (!lex_tile_fits(tw ? tw : kLexTileW, th ? th : kLexTileH))
            return fail(MISOR_EINVAL,
                        "lexicographic tile %d x %d: sides from %d, tile + halo + rhs within LDS",
                        tw ? tw : kLexTileW, th ? th : kLexTileH, kLexMinTile);
        g->lex_tw = tw;
        g->lex_th = th;
        return MISOR_OK;
    }
    case MISOR_TUNE_LEX_WGS: g->lex_wgs = value > 0 ? value : 0; return MISOR_OK;
    case MISOR_TUNE_MG_TAIL:
        if (value != 0 && value != 1) return fail(MISOR_EINVAL, "MG_TAIL is 0 or 1");
        g->mg_tail = value != 0;
        return MISOR_OK;
    default: return fail(MISOR_EINVAL, "unknown tuning key %d", key);
    }
}

int misor_get_tuning(const misor_grid* g, int key, int* value) {
    if (!g || !value) return fail(MISOR_EINVAL, "null argument");
    switch (key) {
    case MISOR_TUNE_SWEEP_VARIANT: *value = g->sp.variant; return MISOR_OK;
    case MISOR_TUNE_ROWS_PER_BLOCK: *value = g->sp.rows_per_block; return MISOR_OK;
    case MISOR_TUNE_XCD_REMAP: *value = g->sp.xcd_remap; return MISOR_OK;
    case MISOR_TUNE_SMALL_SOLVE: *value = g->small_solve; return MISOR_OK;
    case MISOR_TUNE_OVERLAP: *value = g->overlap; return MISOR_OK;
    case MISOR_TUNE_TSTEPS: *value = g->tsteps; return MISOR_OK;
    case MISOR_TUNE_TB_VARIANT: *value = g->tp.variant; return MISOR_OK;
    case MISOR_TUNE_TB_ROWS: *value = g->tp.rows_per_block; return MISOR_OK;
    case MISOR_TUNE_TB_PERSISTENT: *value = g->tb_persistent; return MISOR_OK;
    case MISOR_TUNE_TB_CHAIN: *value = chain_on(tb_input(g), g->tp.variant); return MISOR_OK;
    case MISOR_TUNE_NEAR_BAND: *value = g->near_exp; return MISOR_OK;
    case MISOR_TUNE_RES_LITE: *value = g->res_lite; return MISOR_OK;
    case MISOR_TUNE_EDGE_STEAL: *value = g->edge_steal; return MISOR_OK;
    case MISOR_TUNE_LEX_TILED: *value = lex_tiled_on(g); return MISOR_OK;
    case MISOR_TUNE_LEX_TILE_W: *value = g->lex_tw ? g->lex_tw : kLexTileW; return MISOR_OK;
    case MISOR_TUNE_LEX_TILE_H: *value = g->lex_th ? g->lex_th : kLexTileH; return MISOR_OK;
    case MISOR_TUNE_LEX_WGS: *value = g->lex_wgs; return MISOR_OK;
    case MISOR_TUNE_MG_TAIL: *value = g->mg_tail; return MISOR_OK;
    case MISOR_TUNE_NS_FUSE: *value = g->ns_fuse; return MISOR_OK;
    case MISOR_TUNE_FINISH2: *value = g->finish2; return MISOR_OK;
    case MISOR_TUNE_TB_RESERVE: *value = g->tb_reserve; return MISOR_OK;
    default: return fail(MISOR_EINVAL, "unknown tuning key %d", key);
    }
}

int misor_chain_trace(misor_grid* g, unsigned long long* out, long long cap, long long* n) {
    if (!g || !n) return fail(MISOR_EINVAL, "null argument");
    *n = 0;
    if (!g->chain_trace) return MISOR_OK;
    HIPCHK(hipSetDevice(g->device));
    HIPCHK(hipDeviceSynchronize());
    const long long m = std::min(cap, 3 * g->chain_trace_last);
    if (out && m > 0)
        HIPCHK(hipMemcpy(out, g->chain_trace, m * sizeof(unsigned long long),
                         hipMemcpyDeviceToHost));
    *n = 3 * g->chain_trace_last;
    return MISOR_OK;
}

int misor_reset_stats(misor_grid* g) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    for (auto& u : g->nev_used) u = 0;  // (pending NS kernel timings dropped)
    g->stats = misor_stats{};
    return MISOR_OK;
}
