// mg_tail.hip -- the V-cycle on the LDS-resident levels of a multigrid
// hierarchy, in ONE launch of ONE workgroup (misor_mg.hip, DESIGN.md "The fused
// tail").  The tail is the run of trailing levels that each fit the LDS of a
// workgroup (small_solve_fits); on the level-by-level path every one of them
// costs two whole-solve launches with a state read-back a cycle, here the
// cycle walks them down and up without leaving the kernel.  Where the grid
// itself fits, misor_solve_mg's loop over the cycles runs here too and the
// whole multigrid solve is one launch.
//
// One level at a time lives in LDS, in rb_small.h's layout with its pair
// ownership, and is iterated by rb_small.h's small_iteration -- the function
// the whole-solve kernel runs, so p and the residual sum are its bits.  The
// transfers are mg_transfer.h's expressions in mg_kernels.hip's order, between
// the LDS-resident level and the other level's array in global memory (a few
// tens of KB, L2-resident; the workgroup's own stores, ordered by a barrier).
//
// Control flow is workgroup-uniform throughout: the loop bounds come from the
// descriptor and the state's input fields, which nothing writes while the
// kernel runs, and the only data-dependent decisions -- the coarsest solve's
// loop test and the cycle loop's -- are taken on the residual sum every thread
// reads from the LDS broadcast slot behind a barrier (small_iteration).
//
// Compiled with -ffp-contract=off like every unit.

#include "mg_transfer.h"
#include "misor_internal.h"
#include "rb_small.h"

namespace misor {

namespace {

// cell (i, j) of a field in the padded pitch layout
__device__ __forceinline__ long long gix(int i, int j, long long pitch) {
    return (long long)(j + kYOff) * pitch + (i + kXOff);
}

// rc = R (rhs - lap p) of the level in P into the next level's rhs: the
// residuals of a coarse cell's four fine cells in registers only, as
// mg_residual_restrict_kernel forms them (p from LDS, ghosts included)
__device__ __forceinline__ void tail_restrict(const double* P, const MgTailLevel& F,
                                              const MgTailLevel& C) {
    const int W = F.ni + 2;
    const int ncoarse = C.ni * C.nj;
    for (int k = threadIdx.x; k < ncoarse; k += kSmallThreads) {
        const int I = 1 + k % C.ni, J = 1 + k / C.ni;
        const int i = 2 * I - 1, j = 2 * J - 1;
        const double* a = P + j * W + i;  // row 2J-1; a + W: row 2J
        const double* b = a + W;
        const double fa0 = F.rhs[gix(i, j, F.pitch)], fa1 = F.rhs[gix(i + 1, j, F.pitch)];
        const double fb0 = F.rhs[gix(i, j + 1, F.pitch)], fb1 = F.rhs[gix(i + 1, j + 1, F.pitch)];
        const double r00 = mg_resid(fa0, a[0], a[-1], a[1], a[-W], b[0], F.idx2, F.idy2);
        const double r10 = mg_resid(fa1, a[1], a[0], a[2], a[1 - W], b[1], F.idx2, F.idy2);
        const double r01 = mg_resid(fb0, b[0], b[-1], b[1], a[0], b[W], F.idx2, F.idy2);
        const double r11 = mg_resid(fb1, b[1], b[0], b[2], a[1], b[1 + W], F.idx2, F.idy2);
        C.rhs[gix(I, J, C.pitch)] = mg_restrict4(r00, r10, r01, r11);
    }
}

// P += the interpolation of the next level's e (global), neighbour indices
// clamped to the coarse interior, as mg_prolong_correct_kernel weights it
__device__ __forceinline__ void tail_prolong(double* P, const MgTailLevel& F,
                                             const MgTailLevel& C) {
    const int W = F.ni + 2;
    const int nfine = F.ni * F.nj;
    for (int k = threadIdx.x; k < nfine; k += kSmallThreads) {
        const int i = 1 + k % F.ni, j = 1 + k / F.ni;
        const int I = (i + 1) >> 1, J = (j + 1) >> 1;
        const int Ix = (i & 1) ? max(I - 1, 1) : min(I + 1, C.ni);
        const int Jy = (j & 1) ? max(J - 1, 1) : min(J + 1, C.nj);
        const double c = C.p[gix(I, J, C.pitch)], x = C.p[gix(Ix, J, C.pitch)];
        const double y = C.p[gix(I, Jy, C.pitch)], xy = C.p[gix(Ix, Jy, C.pitch)];
        P[j * W + i] = P[j * W + i] + mg_interp(c, x, y, xy);
    }
}

// solveRB's ghost copy of P from its interior (solver.c:218-226; corners untouched)
__device__ __forceinline__ void tail_ghosts(double* P, int ni, int nj) {
    const int W = ni + 2;
    for (int i = 1 + threadIdx.x; i <= ni; i += kSmallThreads) {
        P[i] = P[W + i];
        P[(nj + 1) * W + i] = P[nj * W + i];
    }
    for (int j = 1 + threadIdx.x; j <= nj; j += kSmallThreads) {
        P[j * W] = P[j * W + 1];
        P[j * W + ni + 1] = P[j * W + ni];
    }
}

}  // namespace

// The cycles of one hierarchy's tail by one workgroup of kSmallThreads
// threads.  lds: mg_tail_lds(first level) bytes of the workgroup's own; levels,
// count and st describe the problem, so a batch kernel can call this once per
// workgroup with its member's.
__device__ __forceinline__ void mg_tail_body(double* lds, const MgTailLevel* levels, int count,
                                             MgTailState* st) {
    double* red = lds;     // 16 wave partials + broadcast slot
    double* P = lds + 32;  // the level being worked on
    const int nu1 = st->nu1, nu2 = st->nu2, maxcycles = st->maxcycles;
    const int itermax_coarse = st->itermax_coarse;
    const double epssq = st->epssq, epssq_coarse = st->epssq_coarse;
    const double nband_coarse = st->nband_coarse;
    int n = st->cycles0, near = 0;
    double res = st->res0, part = res;
    int ci[kSmallMaxPairs][2];
    double rh[kSmallMaxPairs][2];

    const int steps = 2 * count - 1;  // down levels 0 .. count-1, up levels count-2 .. 0
    while ((res >= epssq) && (n < maxcycles)) {
        part = res;  // the first level's residual: untouched where no iteration runs
        for (int s = 0; s < steps; ++s) {
            const bool down = s < count;
            const int l = down ? s : steps - 1 - s;
            const bool coarsest = l + 1 == count;
            const MgTailLevel L = levels[l];
            if (down && l > 0) {
                // e = 0, ghosts and corners included, in LDS and in its array
                const int W = L.ni + 2, ncell = W * (L.nj + 2);
                for (int k = threadIdx.x; k < ncell; k += kSmallThreads) {
                    P[k] = 0.0;
                    L.p[gix(k % W, k / W, L.pitch)] = 0.0;
                }
            } else {
                small_load(P, L.p, L.ni, L.nj, L.pitch);
            }
            small_pairs(L.rhs, L.ni, L.nj, L.pitch, ci, rh);
            __syncthreads();
            if (!down) {
                tail_prolong(P, L, levels[l + 1]);
                __syncthreads();
                tail_ghosts(P, L.ni, L.nj);
                __syncthreads();
            }
            // The level's iterations, all through this one loop: smoothing is
            // solveRB's loop with eps 0 and no band, capped at nu1 / nu2 (as
            // misor_solve_mg's smooth() runs it); the coarsest level's has its
            // own coefficient, eps, band and cap.
            const int itermax = coarsest ? itermax_coarse : down ? nu1 : nu2;
            int it = 0, stop = 0;
            double r = 1.0;  // solver.c:196
            small_solve_loop(red, P, L.ni, L.nj, ci, rh, L.idx2, L.idy2,
                             coarsest ? L.coef_coarse : L.coef_smooth, L.cells,
                             coarsest ? epssq_coarse : 0.0, coarsest ? nband_coarse : -1.0,
                             itermax, &it, &r, &stop);
            if (stop) {  // (the coarsest level only) e stays the zeros written above
                near = 1;
                break;
            }
            if (l == 0 && itermax >= 1) part = r;
            if (down && !coarsest) tail_restrict(P, L, levels[l + 1]);
            small_store(P, L.p, L.ni, L.nj, L.pitch);
            __syncthreads();  // P is free; p and rc are visible to the workgroup
        }
        if (near) break;
        res = part;
        ++n;
    }
    if (threadIdx.x == 0) {
        st->cycles = n;
        st->near = near;
        st->res = res;
        st->res_part = part;
    }
}

__global__ __launch_bounds__(kSmallThreads) void mg_tail_kernel(const MgTailLevel* levels,
                                                                int count, MgTailState* st) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    mg_tail_body(lds, levels, count, st);
}

size_t mg_tail_lds(int ni, int nj) {
    return sizeof(double) * (32 + (size_t)(ni + 2) * (nj + 2));
}

hipError_t mg_tail_prepare() {
    // what small_solve_fits allows: the whole LDS of a CU
    return hipFuncSetAttribute((const void*)mg_tail_kernel,
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

void launch_mg_tail(hipStream_t s, const MgTailLevel* levels, int count, MgTailState* st,
                    size_t lds) {
    hipLaunchKernelGGL(mg_tail_kernel, dim3(1), dim3(kSmallThreads), lds, s, levels, count, st);
}

}  // namespace misor
