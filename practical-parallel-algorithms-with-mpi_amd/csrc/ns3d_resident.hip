// ns3d_resident.hip -- the whole 3D red-black solve (assignment-6/src/
// solver.c:175-297) in ONE launch for grids whose pressure field fits in the
// GPU's combined LDS (256 CUs x 160 KB = 40 MB: p of the reference's 128^3 is
// 17 MB).
//
// Why: at 128^3 an iteration of the streaming sweep (k3_sweep, one launch per
// iteration) is a single resident round whose length is its k-march's latency
// chain, ~26 us for 2M cells.  Here every workgroup keeps one
// box of p (32 x 16 x 16 cells) and a two-cell shell around it in LDS
// (36 x 20 x 20 doubles, 115 KB) for the whole solve, its rhs in registers,
// and the iterations are separated by ONE grid barrier and ONE exchange
// instead of kernel boundaries:
//
//   the red cells of the shell's inner layer (the face-neighbours' cells next
//   to the box, recomputed here with their owners' arithmetic) -> red pass ->
//   black pass, which finds every red neighbour locally -> the box's black
//   cells within two of its surface to the mailbox of the iteration's parity
//   + the workgroup's residual partial -> grid barrier -> the shell's black
//   cells (both face layers and the inner layer's edges) from the mailbox;
//   every workgroup sums all partials in the same fixed order and applies the
//   loop test (res = (res + sum)/N, solver.c:283-289), so all stop after the
//   same iteration.
//
// Only black cells cross box boundaries.  The mailboxes (two buffers of p's
// layout in uncached memory) alternate by iteration parity: a box may write
// iteration n+1's cells while a slower neighbour still reads iteration n's.
// p itself is only read at the start and written at the end.
//
// Semantics are solve()'s, cell by cell: red cells (i+j+k odd) only read
// black ones and vice versa; the Neumann ghost-face copy of the iteration's
// end (solver.c:237-278, faces only, edges and corners never touched) is done
// right after a face cell gets its value -- by its owner when it updates the
// cell, by a neighbour when it recomputes or receives it; the ghost is read
// by that cell alone.
// Launched cooperatively (hipLaunchCooperativeKernel refuses a grid that cannot
// be co-resident, and the host then falls back to k3_sweep); the barrier wait
// is bounded: on a timeout the kernel raises an abort flag that every
// workgroup checks, all of them exit, and the host reports the failure.
//
// The XCDs' L2s are not coherent with each other: how the mailbox cells and
// the partials cross them is described at rgrid_arrive_sum / rgrid_wait.  The
// forms tried and removed, with their times: DESIGN.md 6b.

#include "misor_internal.h"

namespace misor {

namespace {

constexpr int kRbx = 32, kRby = 16, kRbz = 16;  // box of cells per workgroup
// LDS strides of the box with its two-cell shell
constexpr int kTsx = kRbx + 4, kTsy = (kRby + 4) * kTsx, kTcells = (kRbz + 4) * kTsy;
constexpr int kTring = 2 * (kRby * kRbz + kRbx * kRbz + kRbx * kRby);  // inner-layer face cells
constexpr int kTshell = 2 * kTring + 4 * (kRbx + kRby + kRbz);  // received positions
constexpr int kTrx = kTshell / 2 + 128;  // black cells of the shell, at most
// threads per box: thread t owns the column pair t & 15 of row (t >> 4) & 15 in
// the kTpz planes from (t >> 8) * kTpz -- four waves per SIMD to cover the LDS
// and FP64 latency of the passes
constexpr int kTthreads = 1024;
constexpr int kTwaves = kTthreads / 64;
constexpr int kTpz = kRbz * 256 / kTthreads;  // planes per thread
// planes per group of a colour pass: every LDS read of a group is issued
// before its stores (a store may alias a later read as far as the compiler
// knows, so one cell at a time would serialise on LDS latency)
constexpr int kTg = 2;
static_assert(kRbx == 32 && kRby == 16 && kTthreads % 256 == 0,
              "a plane of the box is 256 column pairs");
static_assert(kTpz % kTg == 0 && kTg % 2 == 0, "plane groups start on even planes");
constexpr long long kSpinLimit = 1ll << 22;  // polls (~1 us each) before the barrier gives up

struct Bar3 {
    unsigned count;       // groups that have arrived (zeroed before each launch)
    int abort;            // 1: a barrier timed out -- every workgroup leaves
    unsigned pad[14];
    unsigned xcd[8 * 16];  // arrivals per group blockIdx % 8, one 64-B line each
};

__device__ __forceinline__ double rwave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The exchanged data (mailbox cells, partials) is moved by relaxed
// agent-scope atomics, which go to memory past the XCDs' L2s: no cache
// write-back or invalidate at the barrier
__device__ __forceinline__ double xload(const double* a) {
    return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void xstore(double* a, double v) {
    __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Grid barrier number n (1-based) in two halves, arrival and wait; between
// them a workgroup may do anything that reads no exchanged data and writes
// none.
//
// The hand-off across workgroups has no agent-scope fence.  It is the
// "sc1 stores drained, sc1 loads" form of MI355X_MICROARCH.md (Workgroup
// dispatch ... Valid forms, table row 1), a gfx950 property measured there and
// not an architectural guarantee of HIP's memory-ordering rules; the library
// is built for gfx950 only.  It rests on four conditions, (1) - (4), each
// marked at the line that fulfils it.  (Agent-scope release / acquire fences
// instead are correct by those rules and cost an L2 write-back + invalidate
// per barrier: DESIGN.md 6b.)
//
// Arrival, with the workgroup's residual partial folded in: every wave has put
// its wave sum in sh[]; after the workgroup barrier thread 0 adds them in wave
// order, stores the partial and arrives.  Arrivals are counted in two levels:
// per group blockIdx % 8, whose last arriver -- told by the value its own add
// returned -- adds to the global counter.
__device__ void rgrid_arrive_sum(Bar3* bar, unsigned n, const double* sh, double* part) {
    // (2) every store of exchanged data is an xstore (sc1): the pass's mailbox
    //     stores before this call and the partial below
    // (3) every storing wave waits for its stores to be acknowledged ...
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();  // ... before the workgroup barrier, and only behind it
    if (threadIdx.x == 0) {  // does ONE lane arrive for all of them
        double s = sh[0];
#pragma unroll
        for (int w = 1; w < kTwaves; ++w) s += sh[w];
        xstore(part, s);
        __builtin_amdgcn_s_waitcnt(0);  // (3) for the partial, stored by the arriving lane
        const unsigned x = blockIdx.x & 7, nb = gridDim.x;
        const unsigned cx = (nb - x + 7) / 8;  // workgroups in group x
        const unsigned old = __hip_atomic_fetch_add(&bar->xcd[16 * x], 1u, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
        if (old + 1 == n * cx)
            __hip_atomic_fetch_add(&bar->count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the wait: false if the solve was aborted
__device__ bool rgrid_wait(Bar3* bar, unsigned n, int* sh_flag) {
    if (threadIdx.x == 0) {
        const unsigned nb = gridDim.x;
        const unsigned target = n * (nb < 8 ? nb : 8);  // every group, n times
        int ab = 0;
        long long polls = 0;
        // (4) ONE lane polls the counter with relaxed agent-scope atomic
        //     loads (sc1) ...
        while (__hip_atomic_load(&bar->count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <
               target) {
            if (__hip_atomic_load(&bar->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                ab = 1;
                break;
            }
            if (++polls > kSpinLimit) {
                __hip_atomic_store(&bar->abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ab = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        *sh_flag = ab;
    }
    __syncthreads();  // ... and the other waves load only behind the barrier it joins
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // (1) every load of exchanged data after this is an xload (sc1), never a
    //     plain load (plain loads of the mailbox read stale lines): the
    //     partials in the main loop and the mailbox cells in receive()
    return *sh_flag == 0;
}

// shell position f (0 .. kTshell): face layers 0/1 and B+2/B+3, then the
// inner layer's 12 edges; LDS coordinates (shell offset 2)
__device__ __forceinline__ void shell_pos(int f, int& lx, int& ly, int& lz) {
    constexpr int FX = kRby * kRbz, FY = kRbx * kRbz, FZ = kRbx * kRby;
    if (f < 4 * FX) {
        const int l = f / FX, r = f % FX;
        lx = l < 2 ? l : kRbx + l;  // 0, 1, B+2, B+3
        ly = 2 + r % kRby;
        lz = 2 + r / kRby;
    } else if (f < 4 * (FX + FY)) {
        const int h = f - 4 * FX, l = h / FY, r = h % FY;
        ly = l < 2 ? l : kRby + l;
        lx = 2 + r % kRbx;
        lz = 2 + r / kRbx;
    } else if (f < 4 * (FX + FY + FZ)) {
        const int h = f - 4 * (FX + FY), l = h / FZ, r = h % FZ;
        lz = l < 2 ? l : kRbz + l;
        lx = 2 + r % kRbx;
        ly = 2 + r / kRbx;
    } else {  // edges of the inner layer: two coordinates in {1, B+2}
        const int h = f - 4 * (FX + FY + FZ);
        if (h < 4 * kRbx) {
            const int c = h / kRbx;
            lx = 2 + h % kRbx;
            ly = (c & 1) ? kRby + 2 : 1;
            lz = (c & 2) ? kRbz + 2 : 1;
        } else if (h < 4 * (kRbx + kRby)) {
            const int q = h - 4 * kRbx, c = q / kRby;
            ly = 2 + q % kRby;
            lx = (c & 1) ? kRbx + 2 : 1;
            lz = (c & 2) ? kRbz + 2 : 1;
        } else {
            const int q = h - 4 * (kRbx + kRby), c = q / kRbz;
            lz = 2 + q % kRbz;
            lx = (c & 1) ? kRbx + 2 : 1;
            ly = (c & 2) ? kRby + 2 : 1;
        }
    }
}

// inner-layer face position f (0 .. kTring)
__device__ __forceinline__ void ring_pos(int f, int& lx, int& ly, int& lz) {
    constexpr int FX = kRby * kRbz, FY = kRbx * kRbz, FZ = kRbx * kRby;
    if (f < 2 * FX) {
        const int r = f % FX;
        lx = f < FX ? 1 : kRbx + 2;
        ly = 2 + r % kRby;
        lz = 2 + r / kRby;
    } else if (f < 2 * (FX + FY)) {
        const int h = f - 2 * FX, r = h % FY;
        ly = h < FY ? 1 : kRby + 2;
        lx = 2 + r % kRbx;
        lz = 2 + r / kRbx;
    } else {
        const int h = f - 2 * (FX + FY), r = h % FZ;
        lz = h < FZ ? 1 : kRbz + 2;
        lx = 2 + r % kRbx;
        ly = 2 + r / kRbx;
    }
    (void)FZ;
}

// one SOR update of a cell c with right-hand side rv (solver.c:206-221, its
// operations in its order; the library is built with -ffp-contract=off)
struct Upd3 {
    double r, v;  // the residual and the cell's new value
};
__device__ __forceinline__ Upd3 sor_update(double rv, double c, double xm, double xp, double ym,
                                           double yp, double zm, double zp, double idx2,
                                           double idy2, double idz2, double factor) {
    const double tx = (xp - 2.0 * c) + xm;
    const double ty = (yp - 2.0 * c) + ym;
    const double tz = (zp - 2.0 * c) + zm;
    const double r = rv - ((tx * idx2 + ty * idy2) + tz * idz2);
    return {r, c - (factor * r)};
}

}  // namespace

// REG: every box lies wholly inside the domain (I, J, K multiples of the box:
// the reference's 128^3) -- the thread's own cells are kept in registers, so
// its z-neighbours and pair partner skip LDS: 128^3 at 12.2-12.6 us per
// iteration against 12.7-13.2 for the LDS-only form, same box
// (profiles/r04_res3d_forms.txt)
template <bool REG>
__global__ __launch_bounds__(kTthreads, 1) void k3_resident1(
    G3 g, double* __restrict__ p, const double* __restrict__ rhs, double idx2, double idy2,
    double idz2, double factor, double cells, double* __restrict__ partials,
    DevState* __restrict__ st, Bar3* __restrict__ bar, int nbx, int nby,
    double* __restrict__ mbox, int mstride) {
    constexpr int NT = kTthreads, PZ = kTpz, G = kTg;
    __shared__ double L[kTcells];
    __shared__ double sh[kTwaves];
    __shared__ double sh_W[4];
    __shared__ int sh_flag;
    // built once: the shell's black cells to receive (LDS index | ghost-face bits
    // << 16, global offset) and the inner layer's red cells (LDS index | ghost
    // bits << 16, rhs) -- the loops below then touch only real cells
    __shared__ int2 rx_list[kTrx];
    __shared__ int ring_o[kTring / 2 + 64];
    __shared__ double ring_r[kTring / 2 + 64];
    __shared__ int n_rx, n_ring;
    const int t = threadIdx.x;
    const int b = blockIdx.x;
    const int ox = 1 + (b % nbx) * kRbx;  // global coordinates of the box's first cell
    const int oy = 1 + (b / nbx % nby) * kRby;
    const int oz = 1 + b / (nbx * nby) * kRbz;
    const int I = g.I, J = g.J, K = g.K;
    const int sx = (int)g.sx, sxy = (int)g.sxy;  // resident grids are < 2^31 cells
    auto gof = [&](int i, int jj, int k) { return k * sxy + jj * sx + i; };
    auto inner = [&](int i, int jj, int k) {
        return i >= 1 && i <= I && jj >= 1 && jj <= J && k >= 1 && k <= K;
    };

    // p: the box and its two-cell shell (ghosts included; outside the array: 0)
    for (int q = t; q < kTcells; q += NT) {
        const int lz = q / kTsy, ly = q / kTsx % (kRby + 4), lx = q % kTsx;
        const int i = ox - 2 + lx, jj = oy - 2 + ly, k = oz - 2 + lz;
        L[q] = (i >= 0 && jj >= 0 && k >= 0 && i <= I + 1 && jj <= J + 1 && k <= K + 1)
                   ? p[gof(i, jj, k)]
                   : 0.0;
    }
    const int px = t & 15, y = (t >> 4) & 15, zb = (t >> 8) * PZ;
    const int i0 = ox + 2 * px, j = oy + y;
    double rh[PZ][2];  // rh[z - zb]
#pragma unroll
    for (int z = 0; z < PZ; ++z) {
        const int k = oz + zb + z;
#pragma unroll
        for (int e = 0; e < 2; ++e)
            rh[z][e] = (i0 + e <= I && j <= J && k <= K) ? rhs[gof(i0 + e, j, k)] : 0.0;
    }
    // the Neumann ghost faces next to cell (i, jj, k), one bit each, and their
    // copy: the ghost beside the cell at LDS index o gets the cell's value v
    auto gbits = [&](int i, int jj, int k) {
        return (i == 1 ? 1 : 0) | (i == I ? 2 : 0) | (jj == 1 ? 4 : 0) | (jj == J ? 8 : 0) |
               (k == 1 ? 16 : 0) | (k == K ? 32 : 0);
    };
    auto ghosts = [&](int o, int gb, double v) {
        if (gb & 1) L[o - 1] = v;
        if (gb & 2) L[o + 1] = v;
        if (gb & 4) L[o - kTsx] = v;
        if (gb & 8) L[o + kTsx] = v;
        if (gb & 16) L[o - kTsy] = v;
        if (gb & 32) L[o + kTsy] = v;
    };
    if (t == 0) n_rx = n_ring = 0;
    __syncthreads();
    for (int f = t; f < kTring; f += NT) {
        int lx, ly, lz;
        ring_pos(f, lx, ly, lz);
        const int i = ox - 2 + lx, jj = oy - 2 + ly, k = oz - 2 + lz;
        if (inner(i, jj, k) && ((i + jj + k) & 1)) {
            const int q = atomicAdd(&n_ring, 1);
            ring_o[q] = ((lz * (kRby + 4) + ly) * kTsx + lx) | (gbits(i, jj, k) << 16);
            ring_r[q] = rhs[gof(i, jj, k)];
        }
    }
    for (int f = t; f < kTshell; f += NT) {
        int lx, ly, lz;
        shell_pos(f, lx, ly, lz);
        const int i = ox - 2 + lx, jj = oy - 2 + ly, k = oz - 2 + lz;
        if (inner(i, jj, k) && !((i + jj + k) & 1)) {
            const int q = atomicAdd(&n_rx, 1);
            // ghost faces only for the inner layer's cells (the outer layer's are never read)
            const bool outer = lx == 0 || lx == kRbx + 3 || ly == 0 || ly == kRby + 3 || lz == 0 ||
                               lz == kRbz + 3;
            rx_list[q] = make_int2(((lz * (kRby + 4) + ly) * kTsx + lx) |
                                       ((outer ? 0 : gbits(i, jj, k)) << 16),
                                   gof(i, jj, k));
        }
    }
    __syncthreads();
    const int nring = n_ring, nrx = n_rx;
    double acc = 0.0;
    double own[PZ][2];  // REG: the thread's cells
    // the box's cells of colour col (1: red, i+j+k odd); black cells within two
    // of the box surface go to the mailbox xm
    auto pass = [&](int col, double* xm) {
        const int e0 = ((i0 + j + oz) & 1) == col ? 0 : 1;  // pair element of colour col, z = 0
#pragma unroll
        for (int z0 = 0; z0 < PZ; z0 += G) {
            double c[G], am[G], ap[G], bm[G], bp[G], cm[G], cp[G];
#pragma unroll
            for (int u = 0; u < G; ++u) {
                const int z = zb + z0 + u, e = e0 ^ (u & 1);  // zb, z0 even
                const int o = ((z + 2) * (kRby + 4) + (y + 2)) * kTsx + 2 * px + e + 2;
                if (REG) {
                    const int w = z0 + u;
                    const double far = L[e ? o + 1 : o - 1];
                    const double mine = e ? own[w][1] : own[w][0];
                    const double part = e ? own[w][0] : own[w][1];
                    c[u] = mine;
                    am[u] = e ? part : far;
                    ap[u] = e ? far : part;
                    bm[u] = L[o - kTsx];
                    bp[u] = L[o + kTsx];
                    cm[u] = w > 0 ? (e ? own[w - 1][1] : own[w - 1][0]) : L[o - kTsy];
                    cp[u] = w < PZ - 1 ? (e ? own[w + 1][1] : own[w + 1][0]) : L[o + kTsy];
                } else {
                    c[u] = L[o];
                    am[u] = L[o - 1];
                    ap[u] = L[o + 1];
                    bm[u] = L[o - kTsx];
                    bp[u] = L[o + kTsx];
                    cm[u] = L[o - kTsy];
                    cp[u] = L[o + kTsy];
                }
            }
#pragma unroll
            for (int u = 0; u < G; ++u) {
                const int z = zb + z0 + u, k = oz + z, e = e0 ^ (u & 1), i = i0 + e;
                if (i > I || j > J || k > K) continue;
                const int x = 2 * px + e;
                const int o = ((z + 2) * (kRby + 4) + (y + 2)) * kTsx + x + 2;
                const Upd3 n = sor_update(e ? rh[z0 + u][1] : rh[z0 + u][0], c[u], am[u], ap[u],
                                          bm[u], bp[u], cm[u], cp[u], idx2, idy2, idz2, factor);
                L[o] = n.v;
                ghosts(o, gbits(i, j, k), n.v);
                acc += (n.r * n.r);
                if (REG) {
                    if (e) own[z0 + u][1] = n.v;
                    else   own[z0 + u][0] = n.v;
                }
                if (col == 0 && (x < 2 || x >= kRbx - 2 || y < 2 || y >= kRby - 2 || z < 2 ||
                                 z >= kRbz - 2))
                    xstore(xm + gof(i, j, k), n.v);
            }
        }
    };
    // the neighbours' red cells next to the box
    auto ring_red = [&]() {
        constexpr int RQ = (kTring / 2 + 64 + NT - 1) / NT;
        double c[RQ], am[RQ], ap[RQ], bm[RQ], bp[RQ], cm[RQ], cp[RQ];
        int oo[RQ];
#pragma unroll
        for (int m = 0; m < RQ; ++m) {
            const int q = t + NT * m;
            oo[m] = q < nring ? ring_o[q] : -1;
            const int o = oo[m] < 0 ? kTsy + kTsx + 1 : (oo[m] & 0xffff);
            c[m] = L[o];
            am[m] = L[o - 1];
            ap[m] = L[o + 1];
            bm[m] = L[o - kTsx];
            bp[m] = L[o + kTsx];
            cm[m] = L[o - kTsy];
            cp[m] = L[o + kTsy];
        }
#pragma unroll
        for (int m = 0; m < RQ; ++m) {
            if (oo[m] < 0) continue;
            const int o = oo[m] & 0xffff;
            const Upd3 n = sor_update(ring_r[t + NT * m], c[m], am[m], ap[m], bm[m], bp[m], cm[m],
                                      cp[m], idx2, idy2, idz2, factor);
            L[o] = n.v;
            ghosts(o, oo[m] >> 16, n.v);
        }
    };
    // the shell's black cells from mailbox xm, with their ghost faces
    auto receive = [&](const double* xm) {
        constexpr int RXQ = (kTrx + NT - 1) / NT;
        double v[RXQ];
        int2 e[RXQ];
#pragma unroll
        for (int m = 0; m < RXQ; ++m) {
            const int q = t + NT * m;
            e[m] = q < nrx ? rx_list[q] : make_int2(-1, 0);
            v[m] = e[m].x >= 0 ? xload(xm + e[m].y) : 0.0;
        }
#pragma unroll
        for (int m = 0; m < RXQ; ++m) {
            if (e[m].x < 0) continue;
            const int o = e[m].x & 0xffff;
            L[o] = v[m];
            ghosts(o, e[m].x >> 16, v[m]);
        }
    };

    double res = st->res;
    int it = st->it, done = st->done;
    const double epssq = st->epssq;
    const int itermax = st->itermax;
    unsigned nbar = 0;
    bool ok = true;
    __syncthreads();
    if (REG) {
#pragma unroll
        for (int u = 0; u < PZ; ++u) {
            const int o = ((zb + u + 2) * (kRby + 4) + (y + 2)) * kTsx + 2 * px + 2;
            own[u][0] = L[o];
            own[u][1] = L[o + 1];
        }
    }
    while (!done) {
        double* const xm = mbox + (it & 1) * (long long)mstride;
        ring_red();
        pass(1, xm);  // red: i+j+k odd (solver.c: the sweep starts at (1,1,1))
        __syncthreads();
        pass(0, xm);
        // the workgroup's residual: wave sums to sh[], added and published
        // with the arrival (rgrid_arrive_sum)
        {
            const double ws = rwave_sum(acc);
            if ((t & 63) == 0) sh[t >> 6] = ws;
        }
        acc = 0.0;
        double* part = partials + (it & 1) * gridDim.x;
        ++nbar;
        rgrid_arrive_sum(bar, nbar, sh, part + b);
        if (!(ok = rgrid_wait(bar, nbar, &sh_flag))) break;
        // the sum of all partials, the same bits in every workgroup: waves 0-3
        // take one chunk of 64 partials each (lane 0's wave tree) and the
        // chunks are added in order after the workgroup barrier -- the bits of
        // one wave doing the four chunks in turn, without their four loads
        // and trees in series on it
        if (t < 256) {
            const double v = t < (int)gridDim.x ? xload(part + t) : 0.0;
            const double ws = rwave_sum(v);
            if ((t & 63) == 0) sh_W[t >> 6] = ws;
        }
        receive(xm);
        __syncthreads();
        res = (res + (((sh_W[0] + sh_W[1]) + sh_W[2]) + sh_W[3])) / cells;
        ++it;
        done = !((res >= epssq) && (it < itermax));
    }
    if (!ok) return;
    // the box and the ghost faces next to it, back to p
#pragma unroll
    for (int z = zb; z < zb + PZ; ++z) {
        const int k = oz + z;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int i = i0 + e;
            if (i > I || j > J || k > K) continue;
            const int o = ((z + 2) * (kRby + 4) + (y + 2)) * kTsx + 2 * px + e + 2;
            const int go = gof(i, j, k);
            p[go] = L[o];
            if (i == 1) p[go - 1] = L[o - 1];
            if (i == I) p[go + 1] = L[o + 1];
            if (j == 1) p[go - sx] = L[o - kTsx];
            if (j == J) p[go + sx] = L[o + kTsx];
            if (k == 1) p[go - sxy] = L[o - kTsy];
            if (k == K) p[go + sxy] = L[o + kTsy];
        }
    }
    if (b == 0 && t == 0) {
        st->it = it;
        st->res = res;
        st->done = done;
    }
}

// boxes along each axis
struct BoxGrid3 {
    int x, y, z;
};
static BoxGrid3 resident_box_grid(const G3& g) {
    return {(g.I + kRbx - 1) / kRbx, (g.J + kRby - 1) / kRby, (g.K + kRbz - 1) / kRbz};
}

// full: every box lies wholly inside the domain
static bool resident_full(const G3& g) {
    return g.I % kRbx == 0 && g.J % kRby == 0 && g.K % kRbz == 0;
}

// the kernel for this grid: the register form when every box is full
static const void* resident_kernel(const G3& g) {
    return resident_full(g) ? reinterpret_cast<const void*>(k3_resident1<true>)
                            : reinterpret_cast<const void*>(k3_resident1<false>);
}

// boxes of the resident solve for this grid, or 0 if it cannot run here
int resident3_boxes(const G3& g) {
    if (g.koff != 0 || !g.lo_phys || !g.hi_phys) return 0;  // single domain only
    if ((long long)(g.K + 2) * g.sxy >= (1ll << 31)) return 0;
    const BoxGrid3 bg = resident_box_grid(g);
    const long long nb = (long long)bg.x * bg.y * bg.z;
    int dev = 0, cus = 0, per = 0;  // per: resident workgroups of the launched kernel per CU
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, resident_kernel(g), kTthreads, 0) !=
            hipSuccess)
        return 0;
    return nb <= (long long)cus * per && nb <= 256 ? (int)nb : 0;  // 256: partials slots
}

size_t resident3_bar_bytes() { return 1024; }
static_assert(sizeof(Bar3) <= 1024, "barrier state");

// 0: launched; 1: the device refused the cooperative grid (the caller falls
// back to the streaming sweep); < 0: error
int launch3_resident(hipStream_t s, const G3& g, double* p, const double* rhs, double idx2,
                     double idy2, double idz2, double factor, double cells, double* partials,
                     DevState* st, void* bar, double* mbox) {
    if (!mbox) return -1;
    const int nb = resident3_boxes(g);
    if (nb == 0) return 1;
    BoxGrid3 bg = resident_box_grid(g);
    if (hipMemsetAsync(bar, 0, sizeof(Bar3), s) != hipSuccess) return -1;
    G3 ga = g;
    Bar3* b = static_cast<Bar3*>(bar);
    int mstride = (int)((g.K + 4) * g.sxy);  // the host's mailboxes: two buffers of p's size
    void* args[] = {&ga, &p, const_cast<double**>(&rhs), &idx2, &idy2, &idz2, &factor, &cells,
                    &partials, &st, &b, &bg.x, &bg.y, &mbox, &mstride};
    const hipError_t e = hipLaunchCooperativeKernel(resident_kernel(g), dim3(nb), dim3(kTthreads),
                                                    args, 0, s);
    if (e == hipSuccess) return 0;
    (void)hipGetLastError();  // clear the refusal
    return 1;
}

int resident3_aborted(const void* bar, hipStream_t s, int* aborted) {
    Bar3 h{};
    if (hipMemcpyAsync(&h, bar, sizeof(Bar3), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return -1;
    *aborted = h.abort;
    return 0;
}

}  // namespace misor
