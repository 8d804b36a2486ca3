// rb_small.h -- solveRB on a grid held in the LDS of ONE workgroup of
// kSmallThreads threads: the pieces rb_solve_small_body (sor_kernels.hip: the
// whole-solve kernel and the batch kernel) and mg_tail_body (mg_tail.hip: the
// V-cycle on LDS-resident levels) are both made of, so that an iteration is
// the same arithmetic in the same order -- p and the sum of r^2 the same bits
// -- wherever it runs.  Device code only; compile with -ffp-contract=off.
//
// LDS of the workgroup: lds[0 .. 15] the 16 wave partials of the residual sum,
// lds[16] the broadcast slot, P = lds + 32 the field, (ni+2) x (nj+2) cells
// with row stride ni + 2 (ghosts and corners included).
#pragma once

#include "misor_internal.h"

namespace misor {

constexpr int kSmallThreads = 1024;
constexpr int kSmallMaxPairs = 8;  // pairs per thread (128^2: exactly 8)

__device__ __forceinline__ double small_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// P <- all (ni+2)(nj+2) cells of a field in the padded pitch layout
__device__ __forceinline__ void small_load(double* P, const double* p_glob, int ni, int nj,
                                           long long pitch) {
    const int W = ni + 2;
    const long long ncell = (long long)W * (nj + 2);
    for (long long k = threadIdx.x; k < ncell; k += kSmallThreads) {
        const int i = (int)(k % W), j = (int)(k / W);
        P[k] = p_glob[(long long)(j + kYOff) * pitch + (i + kXOff)];
    }
}

// ... and back (the same thread owns the same cells as in small_load)
__device__ __forceinline__ void small_store(const double* P, double* p_glob, int ni, int nj,
                                            long long pitch) {
    const int W = ni + 2;
    const long long ncell = (long long)W * (nj + 2);
    for (long long k = threadIdx.x; k < ncell; k += kSmallThreads) {
        const int i = (int)(k % W), j = (int)(k / W);
        p_glob[(long long)(j + kYOff) * pitch + (i + kXOff)] = P[k];
    }
}

// This thread's cell pairs: pair e covers columns 1+2m, 2+2m of row 1 + e / half.
// ci: LDS index of (colour-0 cell, colour-1 cell), -1: none; rh: their rhs,
// kept in registers while the level is worked on.
__device__ __forceinline__ void small_pairs(const double* rhs_glob, int ni, int nj,
                                            long long pitch, int (&ci)[kSmallMaxPairs][2],
                                            double (&rh)[kSmallMaxPairs][2]) {
    const int W = ni + 2;
    const int half = (ni + 1) / 2;
    const int npairs = nj * half;
#pragma unroll
    for (int m = 0; m < kSmallMaxPairs; ++m) {
        const int e = (int)threadIdx.x + m * kSmallThreads;
        ci[m][0] = ci[m][1] = -1;
        rh[m][0] = rh[m][1] = 0.0;
        if (e < npairs) {
            const int j = 1 + e / half, i0 = 1 + 2 * (e % half);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                // colour c cell of this pair: (i + j) & 1 == c
                const int i = ((i0 + j) & 1) == c ? i0 : i0 + 1;
                if (i <= ni) {
                    ci[m][c] = j * W + i;
                    rh[m][c] = rhs_glob[(long long)(j + kYOff) * pitch + (i + kXOff)];
                }
            }
        }
    }
}

// One solveRB iteration on P: in-place red then black pass (a barrier after
// each), the Neumann ghost copy rows then columns (corners untouched), and the
// fixed-order sum of r^2 -- wave_sum, then the 16 wave partials added in order
// by thread 0.  Returns that sum, the same value in every thread (read from the
// broadcast slot behind a barrier).  Every thread of the workgroup calls it; on
// return all of P is written and visible.
__device__ __forceinline__ double small_iteration(double* red, double* P, int ni, int nj,
                                                  const int (&ci)[kSmallMaxPairs][2],
                                                  const double (&rh)[kSmallMaxPairs][2],
                                                  double idx2, double idy2, double coef) {
    const int W = ni + 2;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int m = 0; m < kSmallMaxPairs; ++m) {
            const int k = ci[m][c];
            if (k >= 0) {
                const double cc = P[k];
                const double r = rh[m][c] - (((P[k + 1] - 2.0 * cc) + P[k - 1]) * idx2 +
                                             ((P[k + W] - 2.0 * cc) + P[k - W]) * idy2);
                P[k] = cc - coef * r;
                acc += r * r;
            }
        }
        __syncthreads();
    }
    // Neumann ghost copy: rows, then columns (corners untouched)
    for (int i = 1 + t; i <= ni; i += kSmallThreads) {
        P[i] = P[W + i];
        P[(nj + 1) * W + i] = P[nj * W + i];
    }
    __syncthreads();
    for (int j = 1 + t; j <= nj; j += kSmallThreads) {
        P[j * W] = P[j * W + 1];
        P[j * W + ni + 1] = P[j * W + ni];
    }
    // fixed-order block sum of r^2
    acc = small_wave_sum(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int w = 0; w < kSmallThreads / 64; ++w) s += red[w];
        red[16] = s;
    }
    __syncthreads();
    return red[16];
}

// solveRB's loop (solver.c:197) on P from `it` iterations done with residual
// `res`, as the whole-solve kernel runs it: stopped BEFORE an iteration whose
// res lies within nband of eps^2 (*near = 1; nband < 0: no band).  That
// iteration has then been applied to P: the caller drops P.  All arguments are
// workgroup-uniform, and so is every branch around a barrier.
__device__ __forceinline__ void small_solve_loop(double* red, double* P, int ni, int nj,
                                                 const int (&ci)[kSmallMaxPairs][2],
                                                 const double (&rh)[kSmallMaxPairs][2],
                                                 double idx2, double idy2, double coef,
                                                 double cells, double epssq, double nband,
                                                 int itermax, int* it_io, double* res_io,
                                                 int* near) {
    int it = *it_io;
    double res = *res_io;
    while ((res >= epssq) && (it < itermax)) {
        const double rn = small_iteration(red, P, ni, nj, ci, rh, idx2, idy2, coef) / cells;
        if (fabs(rn - epssq) <= nband) {  // near the threshold: the host reruns
            *near = 1;                     // up to `it` iterations
            break;
        }
        res = rn;
        ++it;
    }
    *it_io = it;
    *res_io = res;
}

}  // namespace misor
