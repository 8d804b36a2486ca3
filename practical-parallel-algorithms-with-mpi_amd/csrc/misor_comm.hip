// misor_comm.hip -- communication of a decomposed grid: the depth-d halo
// exchange, the all-reduce and the gather to rank 0, over RCCL or the
// in-process transport (LOCAL: groups), with a progress timeout (misor_grid.h).
// Who sends which cells to whom is decided in decomp2.h.

#include "misor_grid.h"

// a start/stop event pair for timing one communication step (kind 0: halo
// exchange, 1: all-reduce) of the current batch; false when not timing
static bool comm_pair(misor_grid* g, int kind, hipEvent_t* e0, hipEvent_t* e1) {
    if (!g->comm_timing) return false;
    std::vector<hipEvent_t>& v = g->cev[kind];
    size_t& u = g->cev_used[kind];
    while (v.size() < 2 * (u + 1)) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return false;
        v.push_back(e);
    }
    *e0 = v[2 * u];
    *e1 = v[2 * u + 1];
    ++u;
    return true;
}

// add the timed communication steps of the batch just synchronised to the stats
int collect_comm_times(misor_grid* g) {
    for (int kind = 0; kind < 2; ++kind) {
        for (size_t k = 0; k < g->cev_used[kind]; ++k) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, g->cev[kind][2 * k], g->cev[kind][2 * k + 1]));
            if (kind == 0) {
                g->stats.halo_ms += ms;
                g->stats.halos++;
            } else {
                g->stats.allreduce_ms += ms;
                g->stats.allreduces++;
            }
        }
        g->cev_used[kind] = 0;
    }
    return MISOR_OK;
}

static double comm_timeout_s() {
    const char* e = getenv("MISOR_COMM_TIMEOUT");
    const double v = e && *e ? atof(e) : 0.0;
    return v > 0 ? v : 600.0;
}

// Wait for stream s.  With an RCCL communicator, poll instead of blocking:
// an asynchronous communicator error (a peer died, a link failed:
// ncclCommGetAsyncError) or no progress for MISOR_COMM_TIMEOUT seconds
// (default 600) aborts the communicator and returns MISOR_ECOMM on this rank,
// where the reference's MPI default (MPI_ERRORS_ARE_FATAL) would end the job;
// a blocked hipStreamSynchronize would hang instead.
int wait_stream(misor_grid* g, hipStream_t s) {
    if (!g->comm) {
        HIPCHK(hipStreamSynchronize(s));
        return MISOR_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const double limit = comm_timeout_s();
    for (long spins = 0;; ++spins) {
        const hipError_t e = hipStreamQuery(s);
        if (e == hipSuccess) return MISOR_OK;
        if (e != hipErrorNotReady)
            return fail(MISOR_EHIP, "stream wait: %s", hipGetErrorString(e));
        ncclResult_t ar = ncclSuccess;
        const bool bad = ncclCommGetAsyncError(g->comm, &ar) == ncclSuccess &&
                         ar != ncclSuccess && ar != ncclInProgress;
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (bad || el > limit) {
            (void)ncclCommAbort(g->comm);
            g->comm = nullptr;
            g->comm_dead = true;
            if (g->comm_owner) {  // (a multigrid level on the communicator of the grid above)
                g->comm_owner->comm = nullptr;
                g->comm_owner->comm_dead = true;
            }
            if (bad)
                return fail(MISOR_ECOMM, "RCCL asynchronous error: %s", ncclGetErrorString(ar));
            return fail(MISOR_ECOMM, "communication made no progress for %.0f s "
                                     "(MISOR_COMM_TIMEOUT)", limit);
        }
        if (spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

#define COMMCHK(g)                                                                        \
    do {                                                                                  \
        if ((g)->comm_dead)                                                               \
            return fail(MISOR_ECOMM, "the communicator was aborted by an earlier error"); \
    } while (0)

// one 8-neighbour exchange of `field` at depth d on stream s (default: the
// grid stream): pack kernel, transport, unpack kernel
int exchange(misor_grid* g, double* field, int d, hipStream_t s) {
    if (!g->dist) return MISOR_OK;
    COMMCHK(g);
    if (!s) s = g->stream;
    const HaloPlan& P = g->plan[d];
    hipEvent_t t0 = nullptr, t1 = nullptr;
    const bool timed = comm_pair(g, 0, &t0, &t1);
    if (timed) HIPCHK(hipEventRecord(t0, s));
    if (g->local) {
        // In-process transport.  Rank q's copies of my send buffer and my own
        // unpack of the previous exchange must be done before I pack again;
        // my copies of q's buffer wait for q's pack.  Barrier 1: every rank has
        // recorded its pack event; barrier 2: every rank has recorded its copy
        // event (so the next exchange waits on this exchange's records).
        static const int opposite[kDirs] = {1, 0, 3, 2, 7, 6, 5, 4};
        LocalGroup<misor_grid>& G = *g->local;
        HIPCHK(hipStreamWaitEvent(s, g->lx_cp, 0));
        for (int k = 0; k < kDirs; ++k)
            if (g->nbr[k] >= 0) HIPCHK(hipStreamWaitEvent(s, G.members[g->nbr[k]]->lx_cp, 0));
        launch_pack(s, field, g->pitch, P, g->sendbuf);
        HIPCHK(hipEventRecord(g->lx_pk, s));
        G.barrier();
        for (int k = 0; k < kDirs; ++k) {
            if (g->nbr[k] < 0) continue;
            const misor_grid* q = G.members[g->nbr[k]];
            const HaloRegion& sr = q->plan[d].send[opposite[k]];
            const HaloRegion& rr = P.recv[k];
            HIPCHK(hipStreamWaitEvent(s, q->lx_pk, 0));
            HIPCHK(hipMemcpyAsync(g->recvbuf + rr.off, q->sendbuf + sr.off,
                                  sizeof(double) * (size_t)rr.w * rr.h,
                                  hipMemcpyDeviceToDevice, s));
        }
        launch_unpack(s, field, g->pitch, P, g->recvbuf);
        HIPCHK(hipEventRecord(g->lx_cp, s));
        if (timed) HIPCHK(hipEventRecord(t1, s));
        HIPCHK(hipGetLastError());
        G.barrier();
        return MISOR_OK;
    }
    launch_pack(s, field, g->pitch, P, g->sendbuf);
    NCCLCHK(ncclGroupStart());
    for (int k = 0; k < kDirs; ++k) {
        if (g->nbr[k] < 0) continue;
        const size_t ns = (size_t)P.send[k].w * P.send[k].h;
        const size_t nr = (size_t)P.recv[k].w * P.recv[k].h;
        NCCLCHK(ncclSend(g->sendbuf + P.send[k].off, ns, ncclDouble, g->nbr[k], g->comm, s));
        NCCLCHK(ncclRecv(g->recvbuf + P.recv[k].off, nr, ncclDouble, g->nbr[k], g->comm, s));
    }
    NCCLCHK(ncclGroupEnd());
    launch_unpack(s, field, g->pitch, P, g->recvbuf);
    if (timed) HIPCHK(hipEventRecord(t1, s));
    HIPCHK(hipGetLastError());
    return MISOR_OK;
}

// the current pressure buffer's halo, exchanged 2 deep if a solve left it stale
int p_halo(misor_grid* g) {
    if (!g->dist || !g->p_stale) return MISOR_OK;
    int rc = exchange(g, pbuf(g, g->cur), 2);
    if (rc == MISOR_OK) g->p_stale = false;
    return rc;
}

// all-reduce of n <= kMaxT device doubles (sum or max) across the ranks, on
// stream s (default: the grid stream)
int allreduce(misor_grid* g, double* dev, int n, int is_max, hipStream_t s) {
    if (!g->dist) return MISOR_OK;
    COMMCHK(g);
    if (!s) s = g->stream;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    const bool timed = comm_pair(g, 1, &t0, &t1);
    if (timed) HIPCHK(hipEventRecord(t0, s));
    if (g->local) {
        // In-process transport: every rank stages its values (slot by parity,
        // reused two all-reduces later once every rank has read it), gathers
        // every rank's staged values after barrier 1 and combines them in rank
        // order on its device; barrier 2 publishes the read events.
        LocalGroup<misor_grid>& G = *g->local;
        const int par = (int)(g->la_gen++ & 1);
        double* stage = g->la_stage + par * kMaxT;
        double* gather = g->la_gather + (size_t)par * G.n * kMaxT;
        HIPCHK(hipStreamWaitEvent(s, g->la_cmb[par], 0));
        for (int q = 0; q < G.n; ++q) HIPCHK(hipStreamWaitEvent(s, G.members[q]->la_rd[par], 0));
        HIPCHK(hipMemcpyAsync(stage, dev, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipEventRecord(g->la_val[par], s));
        G.barrier();
        for (int q = 0; q < G.n; ++q) {
            const misor_grid* o = G.members[q];
            HIPCHK(hipStreamWaitEvent(s, o->la_val[par], 0));
            HIPCHK(hipMemcpyAsync(gather + (size_t)q * kMaxT, o->la_stage + par * kMaxT,
                                  sizeof(double) * n, hipMemcpyDeviceToDevice, s));
        }
        HIPCHK(hipEventRecord(g->la_rd[par], s));
        launch_local_combine(s, gather, G.n, n, is_max, dev);
        HIPCHK(hipEventRecord(g->la_cmb[par], s));
        if (timed) HIPCHK(hipEventRecord(t1, s));
        HIPCHK(hipGetLastError());
        G.barrier();
        return MISOR_OK;
    }
    NCCLCHK(ncclAllReduce(dev, dev, n, ncclDouble, is_max ? ncclMax : ncclSum, g->comm, s));
    if (timed) HIPCHK(hipEventRecord(t1, s));
    return MISOR_OK;
}

// The bw x bh blocks of all ranks into the whole-domain array `field`, of which
// every rank has filled in its own (misor_grid.h): pack kernel, transport,
// scatter kernel.  The blocks are equal, so RCCL's all-gather takes them as
// they are; in-process every rank copies its peers' packed blocks, ordered by
// events like exchange().
int allgather_blocks(misor_grid* g, double* field, long long pitch, int bw, int bh) {
    COMMCHK(g);
    hipStream_t s = g->stream;
    const int n = g->desc.nranks, rank = g->desc.rank, dims1 = g->loc.dims[1];
    const long long blk = (long long)bw * bh;
    if (g->ag_cap < blk * n) {
        HIPCHK(hipStreamSynchronize(s));
        if (g->local)  // (no peer still copies from the buffer given up: recorded before barrier 2)
            for (misor_grid* o : g->local->members) HIPCHK(hipEventSynchronize(o->ag_cp));
        (void)hipFree(g->ag_send);
        (void)hipFree(g->ag_recv);
        g->ag_send = g->ag_recv = nullptr;
        g->ag_cap = 0;
        if (hipMalloc(&g->ag_send, sizeof(double) * (size_t)blk) != hipSuccess ||
            hipMalloc(&g->ag_recv, sizeof(double) * (size_t)(blk * n)) != hipSuccess)
            return fail(MISOR_ENOMEM, "all-gather buffer allocation failed");
        g->ag_cap = blk * n;
    }
    if (g->local) {
        // as exchange(): my peers' copies of my packed block and my own scatter
        // of the previous call are done before I pack again; my copies of q's
        // block wait for q's pack.  Barrier 1: every rank has recorded its pack
        // event (and allocated its buffer); barrier 2: its copy event.
        LocalGroup<misor_grid>& G = *g->local;
        for (int q = 0; q < n; ++q) HIPCHK(hipStreamWaitEvent(s, G.members[q]->ag_cp, 0));
        launch_mg_block_pack(s, field, pitch, g->ag_send, bw, bh, dims1, rank);
        HIPCHK(hipEventRecord(g->ag_pk, s));
        G.barrier();
        for (int q = 0; q < n; ++q) {
            if (q == rank) continue;
            const misor_grid* o = G.members[q];
            HIPCHK(hipStreamWaitEvent(s, o->ag_pk, 0));
            HIPCHK(hipMemcpyAsync(g->ag_recv + q * blk, o->ag_send, sizeof(double) * (size_t)blk,
                                  hipMemcpyDeviceToDevice, s));
        }
        launch_mg_block_scatter(s, field, pitch, g->ag_recv, bw, bh, dims1, n, rank);
        HIPCHK(hipEventRecord(g->ag_cp, s));
        HIPCHK(hipGetLastError());
        G.barrier();
        return MISOR_OK;
    }
    launch_mg_block_pack(s, field, pitch, g->ag_send, bw, bh, dims1, rank);
    NCCLCHK(ncclAllGather(g->ag_send, g->ag_recv, (size_t)blk, ncclDouble, g->comm, s));
    launch_mg_block_scatter(s, field, pitch, g->ag_recv, bw, bh, dims1, n, rank);
    HIPCHK(hipGetLastError());
    return MISOR_OK;
}

// the block of every rank of g's decomposition, in rank order
static int peer_blocks(const misor_grid* g, std::vector<misor_local>& peers) {
    char err[kDecompErr];
    peers.resize((size_t)g->desc.nranks);
    for (int r = 0; r < g->desc.nranks; ++r) {
        const int rc = decompose2(g->desc.nranks, r, g->desc.imax, g->desc.jmax, g->loc.dims,
                                  &peers[r], err);
        if (rc) return fail(rc, "%s", err);
    }
    return MISOR_OK;
}

// misor_gather on more than one rank: `field` (device, one of g's) assembled
// into rank 0's global array `host`
int gather(misor_grid* g, const double* field, double* host) {
    HIPCHK(hipSetDevice(g->device));
    const int rank = g->desc.rank, nranks = g->desc.nranks;
    const size_t gw = (size_t)(g->desc.imax + 2);  // global row length (doubles)
    const OwnedBlock mine = owned_block(g->loc);
    // every rank packs its block contiguously (a strided 2D copy on the device)
    long long need = (long long)(g->loc.ni + 2) * (g->loc.nj + 2);
    std::vector<misor_local> peers;  // rank 0: whose block is which
    if (rank == 0) {
        MISOR_TRY(peer_blocks(g, peers));
        for (const misor_local& L : peers)
            need = std::max(need, (long long)(L.ni + 2) * (L.nj + 2));
    }
    // every rank allocates its packing buffer (rank 0: large enough for any
    // rank's block -- it is also the receive stage); all ranks agree on the
    // outcome before any send / receive is posted, so a failed allocation is
    // an error on every rank instead of a rank blocked in a send
    int alloc_ok = 1;
    if (need > g->gbuf_cap) {
        (void)hipFree(g->gbuf);
        g->gbuf = nullptr;
        g->gbuf_cap = 0;
        if (hipMalloc(&g->gbuf, sizeof(double) * (size_t)need) == hipSuccess)
            g->gbuf_cap = need;
        else
            alloc_ok = 0;
    }
    {
        g->red_host[3] = alloc_ok ? 0.0 : 1.0;
        HIPCHK(hipMemcpyAsync(g->red_out + 3, g->red_host + 3, sizeof(double),
                              hipMemcpyHostToDevice, g->stream));
        MISOR_TRY(allreduce(g, g->red_out + 3, 1, 1));
        HIPCHK(hipMemcpyAsync(g->red_host + 3, g->red_out + 3, sizeof(double),
                              hipMemcpyDeviceToHost, g->stream));
        MISOR_TRY(wait_stream(g, g->stream));
        if (g->red_host[3] != 0.0)
            return fail(MISOR_ENOMEM, "gather: a rank could not allocate its %s buffer",
                        alloc_ok ? "peer's" : "own");
    }
    const double* src = origin(g, const_cast<double*>(field)) + (long long)mine.j0 * g->pitch +
                        mine.i0;
    HIPCHK(hipMemcpy2DAsync(g->gbuf, sizeof(double) * mine.w, src, sizeof(double) * g->pitch,
                            sizeof(double) * mine.w, mine.h, hipMemcpyDeviceToDevice, g->stream));
    MISOR_TRY(wait_stream(g, g->stream));
    auto to_host = [&](const double* dev, const OwnedBlock& b) -> int {
        HIPCHK(hipMemcpy2DAsync(host + (size_t)b.gj0 * gw + b.gi0, sizeof(double) * gw, dev,
                                sizeof(double) * b.w, sizeof(double) * b.w, b.h,
                                hipMemcpyDeviceToHost, g->stream));
        MISOR_TRY(wait_stream(g, g->stream));
        return MISOR_OK;
    };
    if (g->local) {
        g->local->barrier();  // every block packed
        if (rank == 0)        // unified addressing: any member's device
            for (int r = 0; r < nranks; ++r)
                MISOR_TRY(to_host(g->local->members[r]->gbuf, owned_block(peers[r])));
        g->local->barrier();  // nobody repacks before rank 0 has read
        return MISOR_OK;
    }
    // RCCL: rank r sends its packed block to rank 0, one peer at a time; rank
    // 0 receives into its own packing buffer once its block is on the host
    if (rank == 0) {
        MISOR_TRY(to_host(g->gbuf, mine));
        for (int r = 1; r < nranks; ++r) {
            const OwnedBlock b = owned_block(peers[r]);
            if (ncclRecv(g->gbuf, (size_t)b.w * b.h, ncclDouble, r, g->comm, g->stream) !=
                ncclSuccess)
                return fail(MISOR_ECOMM, "gather: ncclRecv failed");
            MISOR_TRY(to_host(g->gbuf, b));
        }
    } else if (ncclSend(g->gbuf, (size_t)mine.w * mine.h, ncclDouble, 0, g->comm, g->stream) !=
               ncclSuccess) {
        return fail(MISOR_ECOMM, "gather: ncclSend failed");
    }
    MISOR_TRY(wait_stream(g, g->stream));
    return MISOR_OK;
}
