// lex_tiled.hip -- the reference's lexicographic Gauss-Seidel SOR `solve`
// (lex_kernels.hip has the sources and the one-workgroup form) as a tiled
// wavefront over the whole device, bit for bit.
//
// The interior 1..ni x 1..nj is cut into tiles of tw x th cells (the last tile
// of a row / column ragged, down to one cell).  Tile (a,b) of iteration k reads
// the NEW left column of (a-1,b) and bottom row of (a,b-1) and the OLD (k-1)
// right column of (a+1,b) and top row of (a,b+1): it may run once (a-1,b) and
// (a,b-1) have finished iteration k, and (a+1,b), (a,b+1) cannot have started
// theirs.  So the tiles of one tile anti-diagonal a+b run at once, each in one
// workgroup: tile + one-cell halo and the tile's rhs into LDS, the cell
// anti-diagonals with lex_cell (a barrier between them), the interior back to
// HBM, and on border tiles the Neumann ghost copy of the tile's own cells
// (ghost (i,0) is read by cell (i,1) alone, and so on each side: the copy
// needs no other tile; corners stay untouched).
//
// Schedule.  A persistent grid; every workgroup draws tickets from ONE counter.
// Ticket t is tile order[t % ntiles] of iteration t / ntiles, `order` listing
// the tiles by tile anti-diagonal, then along it: tickets are issued in a
// linear extension of the dependency order (iteration, then diagonal), so
// everything the holder of the smallest unfinished ticket waits for is
// finished: some workgroup can always go on, whatever the grid size (a grid
// of one workgroup runs the tiles in ticket order and never waits).
//
// Hand-off (agent-scope release / acquire; the memory model's form, no
// reliance on write-through stores): a tile's waves store p, the ghosts and the
// tile's sum r^2 with plain stores, each wave waits for its stores, workgroup
// barrier, then thread 0: release fence (agent), wait, flag[tile] = k+1
// (relaxed agent-scope atomic), fin += 1.  A consumer's thread 0 polls
// (relaxed agent-scope atomic loads) the iteration word and the two flags, then
// ONE acquire fence (agent), wait, workgroup barrier, and only then do the
// waves load the halo -- with plain vector loads (indexed by thread; p is
// never read through a const __restrict__ pointer, so never on the scalar
// path).  Every polled word is zeroed on the stream before each launch.
//
// Loop test.  The workgroup whose fin add completes iteration k (old + 1 ==
// (k+1) ntiles) acquires, sums partials[] in tile-index order (lane l of wave 0
// takes l, l+64, ... in order, then the xor tree), res = sum / (imax*jmax),
// the reference's test (res >= eps^2 && it < itermax), writes DevState and
// publishes phase = k+1 (go on) or kStop behind a release fence; holders of
// iteration k+1 tickets wait for that word.  For one tile geometry res has
// the same bits for any grid size and schedule (the in-tile order and the
// order over tiles are fixed).
//
// Every spin is bounded: on the limit the workgroup sets the abort word, all
// workgroups leave at their next wait, DevState.done stays 0 and
// misor_solve_lex reports the stall.

#include <algorithm>
#include <vector>

#include "lex_cell.h"

namespace misor {

namespace {

constexpr unsigned kStop = 0xffffffffu;
constexpr long long kLexSpinLimit = 1ll << 22;  // polls (~1 us each) before a wait gives up
constexpr size_t kLexLdsBytes = 160 * 1024;
constexpr int kLexBatch = 16;  // loads a thread keeps in flight while a tile comes in
constexpr int kLexHead = 32;  // doubles in front of the tile: wave partials, control words

// the words zeroed before every launch (then flags[ntiles])
struct LexHdr {
    unsigned long long ticket;  // next ticket
    unsigned long long fin;     // tiles finished, all iterations
    unsigned phase;             // iterations decided "go on"; kStop: the loop is over
    int abort;                  // 1: a wait ran into its limit -- every workgroup leaves
    unsigned pad[2];
};
static_assert(sizeof(LexHdr) == 32, "header block");

#define LEX_RLX(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// thread 0: wait until tile (a,b) of iteration k may run; 0: leave (the loop
// is over, or aborted)
__device__ int lex_wait(LexHdr* hdr, const unsigned* flags, int ntx, int a, int b, unsigned k) {
    const unsigned* fl = a > 0 ? flags + (long long)b * ntx + a - 1 : nullptr;
    const unsigned* fb = b > 0 ? flags + (long long)(b - 1) * ntx + a : nullptr;
    long long polls = 0;
    for (;;) {
        if (LEX_RLX(&hdr->abort)) return 0;
        const unsigned ph = LEX_RLX(&hdr->phase);
        if (ph == kStop) return 0;
        if (ph >= k && (!fl || LEX_RLX(fl) >= k + 1) && (!fb || LEX_RLX(fb) >= k + 1)) return 1;
        if (++polls > kLexSpinLimit) {
            __hip_atomic_store(&hdr->abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return 0;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

template <bool XORDER>
__global__ __launch_bounds__(1024) void lex_tiled_kernel(
    double* p_glob, const double* __restrict__ rhs_glob, int ni, int nj, long long pitch,
    double idx2, double idy2, double factor, double cells, int tw, int th, int ntx, int nty,
    LexHdr* hdr, unsigned* flags, double* partials, const int* __restrict__ order,
    DevState* st) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* red = lds;                  // 16 wave partials
    int* ctl = (int*)(lds + 16);        // go, a, b, k, last
    double* const P = lds + kLexHead;   // tile + halo, row stride W
    const long long W = tw + 2;
    double* const R = P + W * (th + 2);  // the tile's rhs, row stride tw
    const double* const rl = R - tw - 1;  // rl[j * tw + i] = R[(j-1) tw + i-1], i, j from 1
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nt = blockDim.x;
    double* const pg = p_glob + (long long)kYOff * pitch + kXOff;  // cell (0,0) in HBM
    const double* const rg = rhs_glob + (long long)kYOff * pitch + kXOff;
    const unsigned long long ntiles = (unsigned long long)ntx * nty;

    const double epssq = st->epssq;
    const int itermax = st->itermax;
    if (!((1.0 >= epssq) && (0 < itermax))) {  // the reference's test before iteration 1
        if (blockIdx.x == 0 && t == 0) {
            st->it = 0;
            st->res = 1.0;
            st->done = 1;
        }
        return;
    }

    for (;;) {
        __syncthreads();  // the last tile's reads of ctl and of the LDS tile are over
        if (t == 0) {
            const unsigned long long tk = __hip_atomic_fetch_add(
                &hdr->ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long k = tk / ntiles;
            int go = 0, a = 0, b = 0;
            if (k < (unsigned long long)itermax) {
                const long long o = (long long)(tk % ntiles);
                a = order[2 * o];
                b = order[2 * o + 1];
                go = lex_wait(hdr, flags, ntx, a, b, (unsigned)k);
            }
            ctl[0] = go;
            ctl[1] = a;
            ctl[2] = b;
            ctl[3] = (int)k;
            if (go) {
                // ONE acquire for the workgroup: the wait holds the barrier
                // below until this CU's L1 is invalidated
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        __syncthreads();
        if (!ctl[0]) return;
        const int a = ctl[1], b = ctl[2], k = ctl[3];
        const int i0 = a * tw, j0 = b * th;  // global cell of the tile's local (0,0)
        const int w = min(tw, ni - i0), h = min(th, nj - j0);

        // tile + halo (corners are loaded and never used), then the tile's rhs:
        // kLexBatch independent loads per thread in flight, then their LDS
        // writes (one load per trip would pay the memory latency per element)
        const int wp = w + 2, np = wp * (h + 2), nr = w * h;
        for (int c0 = t; c0 < np + nr; c0 += nt * kLexBatch) {
            double v[kLexBatch];
#pragma unroll
            for (int u = 0; u < kLexBatch; ++u) {
                // (past the end: the last element again -- a load under a
                // branch would be waited for at the branch's end)
                const int c = min(c0 + u * nt, np + nr - 1), cr = max(c - np, 0);
                const double* src =
                    c < np ? pg + ((long long)(j0 + c / wp) * pitch + i0 + c % wp)
                           : rg + ((long long)(j0 + 1 + cr / w) * pitch + i0 + 1 + cr % w);
                v[u] = *src;
            }
#pragma unroll
            for (int u = 0; u < kLexBatch; ++u) {
                const int c = c0 + u * nt;
                if (c < np)
                    P[(c / wp) * W + c % wp] = v[u];
                else if (c < np + nr)
                    R[((c - np) / w) * tw + (c - np) % w] = v[u];
            }
        }
        __syncthreads();

        double acc = 0.0;
        for (int d = 2; d <= w + h; ++d) {
            const int ilo = max(1, d - h), ihi = min(w, d - 1);
            for (int i = ilo + t; i <= ihi; i += nt) {
                const double r = lex_cell<XORDER>(P, rl, tw, W, i, d - i, idx2, idy2, factor);
                acc += r * r;
            }
            __syncthreads();
        }

        for (int c = t; c < w * h; c += nt) {
            const int li = 1 + c % w, lj = 1 + c / w;
            pg[(long long)(j0 + lj) * pitch + i0 + li] = P[lj * W + li];
        }
        // Neumann ghost copy of this tile's border cells (interior sources,
        // disjoint destinations: the reference's order is immaterial)
        if (b == 0)
            for (int li = 1 + t; li <= w; li += nt) pg[i0 + li] = P[W + li];
        if (b == nty - 1)
            for (int li = 1 + t; li <= w; li += nt)
                pg[(long long)(nj + 1) * pitch + i0 + li] = P[h * W + li];
        if (a == 0)
            for (int lj = 1 + t; lj <= h; lj += nt) pg[(long long)(j0 + lj) * pitch] = P[lj * W + 1];
        if (a == ntx - 1)
            for (int lj = 1 + t; lj <= h; lj += nt)
                pg[(long long)(j0 + lj) * pitch + ni + 1] = P[lj * W + w];

        acc = lex_wave_sum(acc);
        if (lane == 0) red[wave] = acc;
        // producer: every storing wave waits for its stores, then the barrier
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t == 0) {
            double s = 0.0;
            for (int x = 0; x < nt / 64; ++x) s += red[x];
            partials[(long long)b * ntx + a] = s;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(flags + (long long)b * ntx + a, (unsigned)k + 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long old = __hip_atomic_fetch_add(
                &hdr->fin, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = old + 1 == ((unsigned long long)k + 1) * ntiles;
            ctl[4] = last;
            if (last) {  // every tile of iteration k released its partial before its add
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        __syncthreads();
        if (ctl[4] && wave == 0) {
            double s = 0.0;
            for (unsigned long long m = lane; m < ntiles; m += 64) s += partials[m];
            s = lex_wave_sum(s);
            if (lane == 0) {
                const double res = s / cells;
                const int it = k + 1;
                const bool go_on = (res >= epssq) && (it < itermax);
                st->it = it;
                st->res = res;
                if (!go_on) st->done = 1;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(&hdr->phase, go_on ? (unsigned)it : kStop, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

size_t tile_lds_bytes(int tw, int th) {
    return sizeof(double) * (kLexHead + (size_t)(tw + 2) * (th + 2) + (size_t)tw * th);
}

int tile_threads(int tw, int th) {
    const int diag = tw < th ? tw : th;  // the longest cell anti-diagonal of a tile
    return std::min(1024, std::max(64, (diag + 63) / 64 * 64));
}

template <bool XORDER>
hipError_t resident(int nt, size_t lds, int* out) {
    hipError_t e = hipFuncSetAttribute((const void*)lex_tiled_kernel<XORDER>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    int per_cu = 0, dev = 0, cus = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, lex_tiled_kernel<XORDER>, nt, lds);
    if (e != hipSuccess) return e;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) !=
        hipSuccess)
        return e;
    *out = std::max(1, per_cu * cus);
    return hipSuccess;
}

}  // namespace

bool lex_tile_fits(int tw, int th) {
    return tw >= kLexMinTile && th >= kLexMinTile && tw <= 4096 && th <= 4096 &&
           tile_lds_bytes(tw, th) <= kLexLdsBytes;
}

hipError_t launch_solve_lex_tiled(hipStream_t s, double* p, const double* rhs, int ni, int nj,
                                  long long pitch, double idx2, double idy2, double factor,
                                  double cells, int xorder, DevState* st, int tw, int th,
                                  int wgs_cap, LexTiledWork& wk) {
    const int ntx = (ni + tw - 1) / tw, nty = (nj + th - 1) / th;
    const size_t ntiles = (size_t)ntx * nty;
    // work area: [header, flags] (zeroed per launch, padded to 16 bytes),
    // partials, order
    const size_t zero_bytes = (sizeof(LexHdr) + ntiles * sizeof(unsigned) + 15) / 16 * 16;
    const size_t part_off = zero_bytes, order_off = part_off + ntiles * sizeof(double);
    const size_t bytes = order_off + 2 * ntiles * sizeof(int);
    hipError_t e;
    if (wk.bytes < bytes) {
        (void)hipFree(wk.buf);
        wk.buf = nullptr;
        wk.bytes = 0;
        wk.ntx = wk.nty = 0;
        if ((e = hipMalloc(&wk.buf, bytes)) != hipSuccess) return e;
        wk.bytes = bytes;
    }
    char* base = (char*)wk.buf;
    if (wk.ntx != ntx || wk.nty != nty) {
        // tiles by tile anti-diagonal, then along it.  No launch that uses the
        // area is pending (misor_solve_lex ends with a stream synchronise).
        std::vector<int> order;
        order.reserve(2 * ntiles);
        for (int d = 0; d <= ntx + nty - 2; ++d)
            for (int a = std::max(0, d - (nty - 1)); a <= std::min(ntx - 1, d); ++a) {
                order.push_back(a);
                order.push_back(d - a);
            }
        if ((e = hipMemcpy(base + order_off, order.data(), 2 * ntiles * sizeof(int),
                           hipMemcpyHostToDevice)) != hipSuccess)
            return e;
        wk.ntx = ntx;
        wk.nty = nty;
    }
    const int nt = tile_threads(tw, th);
    const size_t lds = tile_lds_bytes(tw, th);
    int cap = 1;
    e = xorder ? resident<true>(nt, lds, &cap) : resident<false>(nt, lds, &cap);
    if (e != hipSuccess) return e;
    // automatic: no more workgroups than the longest tile diagonal has tiles
    // (more could only wait), nor than are resident at once (more would queue
    // behind them -- harmless, and useless)
    int grid = std::min(std::min(ntx, nty), cap);
    if (wgs_cap > 0) grid = std::min(wgs_cap, (int)std::min<size_t>(ntiles, 1 << 20));
    if ((e = hipMemsetAsync(base, 0, zero_bytes, s)) != hipSuccess) return e;
    LexHdr* hdr = (LexHdr*)base;
    unsigned* flags = (unsigned*)(base + sizeof(LexHdr));
    double* partials = (double*)(base + part_off);
    const int* order = (const int*)(base + order_off);
    if (xorder)
        hipLaunchKernelGGL(lex_tiled_kernel<true>, dim3(grid), dim3(nt), lds, s, p, rhs, ni, nj,
                           pitch, idx2, idy2, factor, cells, tw, th, ntx, nty, hdr, flags,
                           partials, order, st);
    else
        hipLaunchKernelGGL(lex_tiled_kernel<false>, dim3(grid), dim3(nt), lds, s, p, rhs, ni,
                           nj, pitch, idx2, idy2, factor, cells, tw, th, ntx, nty, hdr, flags,
                           partials, order, st);
    return hipGetLastError();
}

}  // namespace misor
