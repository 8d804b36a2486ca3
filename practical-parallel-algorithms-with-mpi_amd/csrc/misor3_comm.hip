// misor3_comm.hip -- the transport of the 3D path: halo exchange, all-reduce
// and gather of a decomposed grid, over RCCL or the in-process transport
// (local_group.h: the ranks are grids driven by host threads of one process;
// collectives are a host barrier plus device-to-device copies, sums combined
// in rank order).
//
// Slabs: every halo is a run of whole planes -- contiguous in the reference
// layout, so halos move by ncclSend / ncclRecv straight from the field, no
// packing.  Cartesian blocks: halos move axis by axis -- x, y, z, each face
// spanning the ghost layers already filled, so edges and corners need no
// messages of their own: x and y faces through pack / unpack kernels and
// staging buffers (halo3.hip), z faces as whole planes straight from the
// field.

#include <cstring>
#include <vector>

#include "misor_grid3.h"

using namespace misor;

int exchange3(misor_grid3* g, int b, int d) {
    if (!dist(g)) return MISOR_OK;
    const size_t cnt = (size_t)d * (size_t)g->g.sxy;
    const int K = g->g.K;
    if (g->local) {
        LocalGroup<misor_grid3>& G = *g->local;
        HIPCHK(hipStreamSynchronize(g->stream));
        G.barrier();  // every rank's sent planes are final
        if (g->prev >= 0) {
            misor_grid3* q = G.members[g->prev];
            HIPCHK(hipMemcpyAsync(plane_ptr(g, b, 1 - d), plane_ptr(q, b, q->g.K - d + 1),
                                  cnt * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
        }
        if (g->next >= 0) {
            misor_grid3* q = G.members[g->next];
            HIPCHK(hipMemcpyAsync(plane_ptr(g, b, K + 1), plane_ptr(q, b, 1),
                                  cnt * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
        }
        HIPCHK(hipStreamSynchronize(g->stream));
        G.barrier();  // nobody overwrites a sent plane before every copy is done
        return MISOR_OK;
    }
    NCCLCHK(ncclGroupStart());
    if (g->next >= 0) {
        NCCLCHK(ncclSend(plane_ptr(g, b, K - d + 1), cnt, ncclDouble, g->next, g->comm,
                         g->stream));
        NCCLCHK(ncclRecv(plane_ptr(g, b, K + 1), cnt, ncclDouble, g->next, g->comm, g->stream));
    }
    if (g->prev >= 0) {
        NCCLCHK(ncclSend(plane_ptr(g, b, 1), cnt, ncclDouble, g->prev, g->comm, g->stream));
        NCCLCHK(ncclRecv(plane_ptr(g, b, 1 - d), cnt, ncclDouble, g->prev, g->comm, g->stream));
    }
    NCCLCHK(ncclGroupEnd());
    return MISOR_OK;
}

int allreduce3(misor_grid3* g, double* dev, int n, bool is_max) {
    if (!dist(g)) return MISOR_OK;
    if (g->local) {
        LocalGroup<misor_grid3>& G = *g->local;
        double v[4];
        HIPCHK(hipMemcpyAsync(v, dev, sizeof(double) * n, hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        for (int k = 0; k < n; ++k) G.vals[4 * g->rank + k] = v[k];
        G.barrier();
        for (int k = 0; k < n; ++k) {
            double a = G.vals[k];
            for (int q = 1; q < G.n; ++q) {
                const double c = G.vals[4 * q + k];
                a = is_max ? ((a > c) ? a : c) : a + c;
            }
            v[k] = a;
        }
        G.barrier();
        HIPCHK(hipMemcpyAsync(dev, v, sizeof(double) * n, hipMemcpyHostToDevice, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        return MISOR_OK;
    }
    NCCLCHK(ncclAllReduce(dev, dev, n, ncclDouble, is_max ? ncclMax : ncclSum, g->comm,
                          g->stream));
    return MISOR_OK;
}

// The slabs are equal and contiguous, each whole planes with their ghost
// columns and rows: over RCCL one in-place all-gather straight in G's rhs, no
// pack kernel; in process, device-to-device copies from the peers' G between
// two host barriers, ordered by stream synchronisation like exchange3's.
int allgather_slabs3(misor_grid3* f, misor_grid3* G, int kc) {
    if (!dist(f)) return MISOR_OK;
    const size_t cnt = (size_t)kc * (size_t)G->g.sxy;
    double* const base = plane_ptr(G, MISOR3_RHS, 1);  // rank 0's slab
    if (f->local) {
        LocalGroup<misor_grid3>& L = *f->local;
        HIPCHK(hipStreamSynchronize(f->stream));
        L.barrier();  // every rank's restricted slab is final
        const long long own = base - G->fld[MISOR3_RHS];
        for (int q = 0; q < f->nranks; ++q) {
            if (q == f->rank) continue;
            // rank q's G: the gathered level of the user's grid its level belongs to
            const misor_grid3* Gq = static_cast<const misor_grid3*>(L.members[q]->peer_gath);
            HIPCHK(hipMemcpyAsync(base + (size_t)q * cnt,
                                  Gq->fld[MISOR3_RHS] + own + (size_t)q * cnt,
                                  cnt * sizeof(double), hipMemcpyDeviceToDevice, f->stream));
        }
        HIPCHK(hipStreamSynchronize(f->stream));
        L.barrier();  // nobody restricts into a slab that is still being copied
        return MISOR_OK;
    }
    NCCLCHK(ncclAllGather(base + (size_t)f->rank * cnt, base, cnt, ncclDouble, f->comm,
                          f->stream));
    return MISOR_OK;
}

// ------------------------------------------------ Cartesian process grid
// sides in the reference's Direction order: 0 left, 1 right, 2 bottom, 3 top,
// 4 front, 5 back; side s lies on axis s / 2, its opposite is s ^ 1

namespace {

// the x or y face of side s (0..3), ghost rims of the other two axes included:
// the ghost layer (halo) or the owned layer next to it
Box3 face_box(const misor_grid3* g, int s, bool halo) {
    const G3& G = g->g;
    Box3 b{0, 0, 0, G.I + 2, G.J + 2, G.K + 2, G.sx, G.sxy};
    const int layer = face_layer(s < 2 ? G.I : G.J, s, halo);
    if (s < 2) {
        b.x0 = layer;
        b.nx = 1;
    } else {
        b.y0 = layer;
        b.ny = 1;
    }
    return b;
}

// the 1-deep halo of buffer b along one axis, both directions
int exchange_cart_axis(misor_grid3* g, int b, int axis) {
    const int* nb = g->loc.neighbours;
    const int s0 = 2 * axis, K = g->g.K;
    const size_t plane = (size_t)g->g.sxy;
    double* f = g->fld[b];
    if (axis < 2) {
        for (int s = s0; s < s0 + 2; ++s)
            if (nb[s] >= 0) launch3_box_pack(g->stream, f, face_box(g, s, false), g->hsend[s]);
        HIPCHK(hipGetLastError());
    }
    if (g->local) {
        LocalGroup<misor_grid3>& G = *g->local;
        HIPCHK(hipStreamSynchronize(g->stream));
        G.barrier();  // every rank's send buffers / sent planes are final
        for (int s = s0; s < s0 + 2; ++s) {
            if (nb[s] < 0) continue;
            misor_grid3* q = G.members[nb[s]];
            if (axis < 2) {
                HIPCHK(hipMemcpyAsync(g->hrecv[s], q->hsend[s ^ 1],
                                      sizeof(double) * (size_t)face_box(g, s, true).cells(),
                                      hipMemcpyDeviceToDevice, g->stream));
            } else {  // front: the neighbour's plane K to plane 0; back: its plane 1 to K+1
                HIPCHK(hipMemcpyAsync(plane_ptr(g, b, s == 4 ? 0 : K + 1),
                                      plane_ptr(q, b, s == 4 ? q->g.K : 1),
                                      sizeof(double) * plane, hipMemcpyDeviceToDevice,
                                      g->stream));
            }
        }
    } else {
        NCCLCHK(ncclGroupStart());
        for (int s = s0; s < s0 + 2; ++s) {
            if (nb[s] < 0) continue;
            if (axis < 2) {
                const size_t cnt = (size_t)face_box(g, s, true).cells();
                NCCLCHK(ncclSend(g->hsend[s], cnt, ncclDouble, nb[s], g->comm, g->stream));
                NCCLCHK(ncclRecv(g->hrecv[s], cnt, ncclDouble, nb[s], g->comm, g->stream));
            } else {
                NCCLCHK(ncclSend(plane_ptr(g, b, s == 4 ? 1 : K), plane, ncclDouble, nb[s],
                                 g->comm, g->stream));
                NCCLCHK(ncclRecv(plane_ptr(g, b, s == 4 ? 0 : K + 1), plane, ncclDouble, nb[s],
                                 g->comm, g->stream));
            }
        }
        NCCLCHK(ncclGroupEnd());
    }
    if (axis < 2) {
        for (int s = s0; s < s0 + 2; ++s)
            if (nb[s] >= 0) launch3_box_unpack(g->stream, f, face_box(g, s, true), g->hrecv[s]);
        HIPCHK(hipGetLastError());
    }
    if (g->local) {
        HIPCHK(hipStreamSynchronize(g->stream));
        g->local->barrier();  // nobody repacks a buffer or overwrites a plane being copied
    }
    return MISOR_OK;
}

// host: one rank's packed box into the global array
void scatter_box(const misor3_local& L, const Box3& bx, const double* packed, const misor3_desc& d,
                 double* global) {
    const long long SX = d.imax + 2, SXY = SX * (d.jmax + 2);
    for (int z = 0; z < bx.nz; ++z)
        for (int y = 0; y < bx.ny; ++y)
            memcpy(global + (long long)(L.off[2] + bx.z0 + z) * SXY +
                       (long long)(L.off[1] + bx.y0 + y) * SX + (L.off[0] + bx.x0),
                   packed + ((long long)z * bx.ny + y) * bx.nx, sizeof(double) * (size_t)bx.nx);
}

}  // namespace

int exchange_cart(misor_grid3* g, int b, int axes) {
    if (!dist(g)) return MISOR_OK;
    for (int a = 0; a < 3; ++a)
        if (((axes >> a) & 1) && g->loc.dims[a] > 1) MISOR_TRY(exchange_cart_axis(g, b, a));
    return MISOR_OK;
}

// ------------------------------------------------------------------ gather
// commCollectResult's gather (assignment-6/src/comm.c:246-384) of one whole
// field: rank 0 receives (imax+2)(jmax+2)(kmax+2) doubles

// Cartesian blocks: rank r sends its own_box, packed
int gather_cart(misor_grid3* g, int field, double* host_global) {
    const Box3 mine = own_box(g->loc);
    if (!g->gbuf)
        HIPCHK(hipMalloc(&g->gbuf, sizeof(double) * (size_t)g->n));
    launch3_box_pack(g->stream, g->fld[field], mine, g->gbuf);
    HIPCHK(hipGetLastError());
    std::vector<double> stage;
    auto rank_box = [&](int r, misor3_local& L) {
        misor3_decompose_cart(g->nranks, r, g->loc.dims, g->desc.imax, g->desc.jmax, g->desc.kmax,
                              &L);
        return own_box(L);
    };
    if (g->local) {
        LocalGroup<misor_grid3>& G = *g->local;
        HIPCHK(hipStreamSynchronize(g->stream));
        G.barrier();  // every rank's box is packed
        if (g->rank == 0) {
            for (int r = 0; r < g->nranks; ++r) {
                misor3_local L;
                const Box3 bx = rank_box(r, L);
                misor_grid3* q = G.members[r];
                stage.resize((size_t)bx.cells());
                HIPCHK(hipSetDevice(q->device));
                HIPCHK(hipMemcpy(stage.data(), q->gbuf, sizeof(double) * stage.size(),
                                 hipMemcpyDeviceToHost));
                scatter_box(L, bx, stage.data(), g->desc, host_global);
            }
            HIPCHK(hipSetDevice(g->device));
        }
        G.barrier();
        return MISOR_OK;
    }
    if (g->rank != 0) {
        NCCLCHK(ncclSend(g->gbuf, (size_t)mine.cells(), ncclDouble, 0, g->comm, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        return MISOR_OK;
    }
    // rank 0 holds the largest block (sizeOfRank), so its local array bounds every box
    if (!g->gstage) HIPCHK(hipMalloc(&g->gstage, sizeof(double) * (size_t)g->n));
    for (int r = 0; r < g->nranks; ++r) {
        misor3_local L;
        const Box3 bx = rank_box(r, L);
        stage.resize((size_t)bx.cells());
        const double* src = g->gbuf;
        if (r != 0) {
            NCCLCHK(ncclRecv(g->gstage, stage.size(), ncclDouble, r, g->comm, g->stream));
            src = g->gstage;
        }
        HIPCHK(hipMemcpyAsync(stage.data(), src, sizeof(double) * stage.size(),
                              hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        scatter_box(L, bx, stage.data(), g->desc, host_global);
    }
    return MISOR_OK;
}

// slabs: rank r sends its planes 1..K, plus plane 0 / K+1 where they are the
// physical ghost planes (slab_gather_span), straight from the field
int gather_slabs(misor_grid3* g, int field, double* host_global) {
    const long long sxy = g->g.sxy;
    auto range = [&](int r, int& k_first, int& k_count, long long& goff) {
        int ko;
        const Span3 s = slab_gather_span(g->nranks, r, g->desc.kmax, &ko);
        k_first = s.lo, k_count = s.count;
        goff = (long long)(ko + k_first) * sxy;  // global plane of local plane k_first
    };
    if (g->local) {
        LocalGroup<misor_grid3>& G = *g->local;
        HIPCHK(hipStreamSynchronize(g->stream));
        G.barrier();
        if (g->rank == 0) {
            for (int r = 0; r < g->nranks; ++r) {
                int kf, kc;
                long long goff;
                range(r, kf, kc, goff);
                misor_grid3* q = G.members[r];
                HIPCHK(hipSetDevice(q->device));
                HIPCHK(hipMemcpy(host_global + goff, plane_ptr(q, field, kf),
                                 sizeof(double) * (size_t)kc * sxy, hipMemcpyDeviceToHost));
            }
            HIPCHK(hipSetDevice(g->device));
        }
        G.barrier();
        return MISOR_OK;
    }
    int kf, kc;
    long long goff;
    range(g->rank, kf, kc, goff);
    if (g->rank != 0) {
        NCCLCHK(ncclSend(plane_ptr(g, field, kf), (size_t)kc * sxy, ncclDouble, 0, g->comm,
                         g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        return MISOR_OK;
    }
    HIPCHK(hipMemcpyAsync(host_global + goff, plane_ptr(g, field, kf),
                          sizeof(double) * (size_t)kc * sxy, hipMemcpyDeviceToHost, g->stream));
    if (!g->gstage) {
        int kmaxloc = 0;
        misor3_decompose(g->nranks, 0, g->desc.kmax, &kmaxloc, nullptr);  // rank 0 is largest
        HIPCHK(hipMalloc(&g->gstage, sizeof(double) * (size_t)(kmaxloc + 2) * sxy));
    }
    for (int r = 1; r < g->nranks; ++r) {
        range(r, kf, kc, goff);
        NCCLCHK(ncclRecv(g->gstage, (size_t)kc * sxy, ncclDouble, r, g->comm, g->stream));
        HIPCHK(hipMemcpyAsync(host_global + goff, g->gstage, sizeof(double) * (size_t)kc * sxy,
                              hipMemcpyDeviceToHost, g->stream));
    }
    HIPCHK(hipStreamSynchronize(g->stream));
    return MISOR_OK;
}
