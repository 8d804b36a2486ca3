// misor3_solve.hip -- misor3_solve (solver.c:175-297): red-black SOR with the
// reference's residual (carried over between iterations), one function per
// schedule -- the Cartesian blocks' two colour passes (solve3_cart), the whole
// solve in one launch with p resident in LDS (solve3_resident), and the
// streaming sweep (solve3_stream).  Each starts with solve3_begin and ends
// with solve3_finish.

#include <utility>

#include "misor_grid3.h"

using namespace misor;

namespace {

// what every launch of a solve takes: 1/dx^2, 1/dy^2, 1/dz^2, the update's
// factor (omega inside) and the global cell count
struct Solve3Consts {
    double idx2, idy2, idz2, factor, cells;
};

// the loop state s0 to the device; the solve's first timing event
int solve3_begin(misor_grid3* g, const DevState& s0) {
    *g->st_host = s0;
    if (g->timing) HIPCHK(hipEventRecord(g->ev[0], g->stream));
    HIPCHK(hipMemcpyAsync(g->st, g->st_host, sizeof(DevState), hipMemcpyHostToDevice,
                          g->stream));
    return MISOR_OK;
}

// the final state is in st_host and ev[1] is recorded behind the last launch:
// the batch-size hint, the timing counters and the caller's results
int solve3_finish(misor_grid3* g, int* iters, double* res) {
    g->last_iters = g->st_host->it;
    if (g->timing) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, g->ev[0], g->ev[1]));
        g->solve_ms += ms;
        g->solve_iters += g->st_host->it;
    }
    if (iters) *iters = g->st_host->it;
    if (res) *res = g->st_host->res;
    return MISOR_OK;
}

// A Cartesian block: the reference's own loop (solver.c:199-291) -- exchange
// p, colour pass 0, exchange p, colour pass 1, then the ranks' sums of r^2
// all-reduced and the loop test on every rank.  Colours are global and the
// Neumann mirrors are written on physical sides only, so p is the
// single-domain solve's bit for bit; only the residual's summation order
// differs.  The state is read back after every iteration (no batches: the
// in-process transport synchronises with the host at every exchange anyway).
int solve3_cart(misor_grid3* g, const Solve3Consts& c, const DevState& s0, int* iters,
                double* res) {
    MISOR_TRY(solve3_begin(g, s0));
    do {
        for (int pass = 0; pass < 2; ++pass) {
            MISOR_TRY(exchange_cart(g, MISOR3_P, 7));
            launch3_rb_pass(g->stream, g->g, g->fld[MISOR3_P], g->fld[MISOR3_RHS], pass, c.idx2,
                            c.idy2, c.idz2, c.factor, g->partials, g->st);
        }
        launch3_rb_sum(g->stream, g->g, g->partials, g->st, c.cells);
        HIPCHK(hipGetLastError());
        MISOR_TRY(allreduce3(g, &g->st->sum[0], 1, false));
        launch3_decide(g->stream, g->st, c.cells);
        if (g->timing) HIPCHK(hipEventRecord(g->ev[1], g->stream));
        HIPCHK(hipMemcpyAsync(g->st_host, g->st, sizeof(DevState), hipMemcpyDeviceToHost,
                              g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
    } while (!g->st_host->done);
    // the final halo, for misor3_adapt_uvw and misor3_download (solver.c:288)
    MISOR_TRY(exchange_cart(g, MISOR3_P, 7));
    g->alt_stale = true;
    return solve3_finish(g, iters, res);
}

// p resident in LDS, one cooperative launch for the whole solve
// (ns3d_resident.hip); *refused: the device refused the cooperative grid and
// nothing ran -- the streaming sweep takes the solve
int solve3_resident(misor_grid3* g, const Solve3Consts& c, const DevState& s0, int* iters,
                    double* res, bool* refused) {
    // barrier state + 2 x 256 partials, and a mailbox of p's layout for the
    // box-surface cells, in uncached memory: coherent across the XCDs' L2s
    // without cache write-backs / invalidations at every barrier
    if (!g->rbar)
        HIPCHK(hipExtMallocWithFlags(&g->rbar, resident3_bar_bytes() + 2 * 256 * sizeof(double),
                                     hipDeviceMallocUncached));
    if (!g->rmbox)
        HIPCHK(hipExtMallocWithFlags(reinterpret_cast<void**>(&g->rmbox),
                                     2 * sizeof(double) * (size_t)g->nalloc,
                                     hipDeviceMallocUncached));
    double* const rpart =
        reinterpret_cast<double*>(static_cast<char*>(g->rbar) + resident3_bar_bytes());
    double* const mbox0 = g->rmbox + (g->fld[MISOR3_P] - g->mem[MISOR3_P]);
    MISOR_TRY(solve3_begin(g, s0));
    const int lr = launch3_resident(g->stream, g->g, g->fld[MISOR3_P], g->fld[MISOR3_RHS], c.idx2,
                                    c.idy2, c.idz2, c.factor, c.cells, rpart, g->st, g->rbar,
                                    mbox0);
    if (lr < 0) return fail(MISOR_EHIP, "resident solve: launch failed");
    *refused = lr == 1;
    if (*refused) return MISOR_OK;
    if (g->timing) HIPCHK(hipEventRecord(g->ev[1], g->stream));
    HIPCHK(hipMemcpyAsync(g->st_host, g->st, sizeof(DevState), hipMemcpyDeviceToHost,
                          g->stream));
    int aborted = 0;
    if (resident3_aborted(g->rbar, g->stream, &aborted) != 0)
        return fail(MISOR_EHIP, "resident solve: state readback failed");
    if (aborted)
        return fail(MISOR_EHIP, "resident solve: a grid barrier timed out (p undefined)");
    g->alt_stale = true;  // the fused sweep's partner buffer no longer matches p
    return solve3_finish(g, iters, res);
}

// Batches of iterations are enqueued and the device-resident state is read
// once per batch.  Default: the fused sweep, one launch per iteration,
// ping-ponging between fld[P] and its partner (launches after the loop test
// fails are no-ops, so the result is in the buffer of parity `it`; the
// pointers are swapped so fld[P] holds it).  The edge and corner ghosts are
// never written by a sweep, so the partner gets a copy of fld[P] whenever P
// was set from outside.
//
// Decomposed (slabs): the sweep writes its slab's sum of r^2, an all-reduce
// adds the ranks' sums and the decide kernel applies the loop test on every
// rank (so every rank stops after the same iteration); after each sweep the
// new buffer's 2-deep halo is exchanged.  The loop is the single-domain one,
// so p and the iteration count do not depend on the slab count (only the
// order of the residual's sum does).  After the loop test fails, the
// remaining launches of a batch are no-ops and their exchanges move final
// planes between buffers of the same parity on every rank.
int solve3_stream(misor_grid3* g, const Solve3Consts& c, const DevState& s0, int* iters,
                  double* res) {
    const int itermax = g->desc.itermax;
    const bool fused = g->sweep != 0;
    if (!fused && dist(g)) return fail(MISOR_ESTATE, "the two-pass solve is single-rank only");
    const int kc = g->kchunk > 0 ? g->kchunk : auto_kchunk(g->g, g->rows);
    // rhs two plane steps ahead pays on long marches (384^3, 32 planes: 0.384 ->
    // 0.376 ms per iteration) and costs on short ones (128^3, 8 planes: 27.4 ->
    // 28.1 us; profiles/r02_tune3d_ra2.txt)
    const bool ra2 = g->rhs_ahead ? g->rhs_ahead == 2 : kc >= 16;
    // single rank: the loop test of sweep m runs inside sweep m+1 (k3_sweep,
    // Fold3); the state alternates between st and st2, the partials between
    // the two halves of g->partials
    const bool fold = fused && !dist(g) && g->fold;
    DevState* const stb[2] = {g->st, g->st2};
    const long long half = g->partials_cap / 2;
    double* const part[2] = {g->partials, g->partials + half};
    int sx = 0;  // the state buffer that holds the current state
    MISOR_TRY(solve3_begin(g, s0));
    if (fused && g->alt_stale) {
        HIPCHK(hipMemcpyAsync(g->mem[kAlt], g->mem[MISOR3_P], sizeof(double) * (size_t)g->nalloc,
                              hipMemcpyDeviceToDevice, g->stream));
        g->alt_stale = false;
    }
    if (dist(g)) {  // halos of p (2 deep) and rhs (1 deep, red on halo planes)
        MISOR_TRY(exchange3(g, MISOR3_P, kHalo));
        MISOR_TRY(exchange3(g, MISOR3_RHS, 1));
    }
    const int bufs[2] = {MISOR3_P, kAlt};
    double* buf[2] = {g->fld[MISOR3_P], g->fld[kAlt]};
    long long launched = 0;
    int batch = g->last_iters > 8 ? g->last_iters : 8;
    if (dist(g) && g->local) batch = 1;  // host-synchronised transport: no batching gain
    for (;;) {
        if (batch > itermax - launched) batch = (int)(itermax - launched);
        if (batch < 1) batch = 1;
        for (int b = 0; b < batch; ++b) {
            const long long m = launched + b;
            if (fold) {
                launch3_sweep_folded(g->stream, g->g, buf[m & 1], buf[(m + 1) & 1],
                                     g->fld[MISOR3_RHS], c.idx2, c.idy2, c.idz2, c.factor,
                                     g->rows, kc, part[m & 1], b == 0 ? nullptr : part[(m - 1) & 1],
                                     stb[sx], stb[sx ^ 1], c.cells, ra2);
                sx ^= 1;
                continue;
            }
            if (!fused) {
                launch3_rb_iteration(g->stream, g->g, g->fld[MISOR3_P], g->fld[MISOR3_RHS],
                                     c.idx2, c.idy2, c.idz2, c.factor, g->partials, g->st,
                                     c.cells);
                continue;
            }
            launch3_sweep(g->stream, g->g, buf[m & 1], buf[(m + 1) & 1], g->fld[MISOR3_RHS],
                          c.idx2, c.idy2, c.idz2, c.factor, g->rows, kc, g->partials, g->st,
                          c.cells, dist(g), ra2);
            if (dist(g)) {
                MISOR_TRY(allreduce3(g, &g->st->sum[0], 1, false));
                launch3_decide(g->stream, g->st, c.cells);
                // the halo of the new buffer: by index, so the LOCAL transport finds
                // the same buffer on the neighbour (every rank swaps alike)
                MISOR_TRY(exchange3(g, bufs[(m + 1) & 1], kHalo));
            }
        }
        if (fold) {  // the loop test of the batch's last sweep
            launch3_fold_decide(g->stream, g->g, g->rows, kc, part[(launched + batch - 1) & 1],
                                stb[sx], stb[sx ^ 1], c.cells);
            sx ^= 1;
        }
        HIPCHK(hipGetLastError());
        launched += batch;
        if (g->timing) HIPCHK(hipEventRecord(g->ev[1], g->stream));
        HIPCHK(hipMemcpyAsync(g->st_host, stb[sx], sizeof(DevState), hipMemcpyDeviceToHost,
                              g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        if (g->st_host->done || launched >= itermax) break;
        batch = (dist(g) && g->local) ? 1 : (batch < 512 ? 2 * batch : 1024);
    }
    if (fused && (g->st_host->it & 1)) {
        std::swap(g->fld[MISOR3_P], g->fld[kAlt]);
        std::swap(g->mem[MISOR3_P], g->mem[kAlt]);
        std::swap(g->alloc[MISOR3_P], g->alloc[kAlt]);
    }
    return solve3_finish(g, iters, res);
}

}  // namespace

int auto_kchunk(const G3& g, int rows) {
    // enough workgroups to fill 256 CUs twice over, chunks of at least 8 planes
    int kc = 64;
    while (kc > 8 && sweep3_blocks(g, rows, kc) < 2048) kc /= 2;
    return kc;
}

int solve3_with(misor_grid3* g, double omega, double eps, int itermax, double res_seed,
                int* iters, double* res) {
    const double omega0 = g->desc.omega, eps0 = g->desc.eps;
    const int itermax0 = g->desc.itermax, last = g->last_iters;
    g->desc.omega = omega;
    g->desc.eps = eps;
    g->desc.itermax = itermax;
    g->res_seed = res_seed;
    const int rc = misor3_solve(g, iters, res);
    g->desc.omega = omega0;
    g->desc.eps = eps0;
    g->desc.itermax = itermax0;
    g->res_seed = 1.0;
    g->last_iters = last;
    return rc;
}

extern "C" int misor3_solve(misor_grid3* g, int* iters, double* res) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    HIPCHK(hipSetDevice(g->device));
    const misor3_desc& d = g->desc;
    const double dx2 = g->dx * g->dx, dy2 = g->dy * g->dy, dz2 = g->dz * g->dz;
    const Solve3Consts c{
        1.0 / dx2, 1.0 / dy2, 1.0 / dz2,
        d.omega * 0.5 * (dx2 * dy2 * dz2) / (dy2 * dz2 + dx2 * dz2 + dx2 * dy2),
        (double)((long long)d.imax * d.jmax * d.kmax)};
    DevState s0{};
    s0.res = g->res_seed;  // 1.0 (solver.c:196) outside solve3_with
    s0.epssq = d.eps * d.eps;
    s0.itermax = d.itermax;
    s0.done = !((s0.res >= s0.epssq) && (0 < d.itermax));
    if (s0.done) {
        if (iters) *iters = 0;
        if (res) *res = s0.res;
        return MISOR_OK;
    }
    if (g->cart) return solve3_cart(g, c, s0, iters, res);
    if (!dist(g) && g->resident != 0 && resident3_boxes(g->g) > 0) {
        bool refused = false;
        const int rc = solve3_resident(g, c, s0, iters, res, &refused);
        if (rc != MISOR_OK || !refused) return rc;
    }
    return solve3_stream(g, c, s0, iters, res);
}
