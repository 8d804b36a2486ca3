// lex_cell.h -- one cell of the reference's lexicographic Gauss-Seidel SOR,
// shared by its two kernels (lex_kernels.hip: one workgroup; lex_tiled.hip:
// the tiled wavefront over the whole device).
#pragma once

#include "misor_internal.h"

namespace misor {

__device__ __forceinline__ double lex_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// W: row stride of P (LDS: ni+2 or the tile's width + 2; HBM: pitch); P points
// at cell (0,0)
template <bool XORDER>
__device__ __forceinline__ double lex_cell(double* P, const double* rhs_glob, long long rpitch,
                                           long long W, int i, int j, double idx2, double idy2,
                                           double factor) {
    const long long k = (long long)j * W + i;
    const double c = P[k];
    double xt, yt;
    if (XORDER) {  // assignment-5/sequential/src/solver.c:162-164
        xt = (P[k + 1] - 2.0 * c) + P[k - 1];
        yt = (P[k + W] - 2.0 * c) + P[k - W];
    } else {  // assignment-4/src/solver.c:149-151
        xt = (P[k - 1] - 2.0 * c) + P[k + 1];
        yt = (P[k - W] - 2.0 * c) + P[k + W];
    }
    const double r = rhs_glob[(long long)j * rpitch + i] - (xt * idx2 + yt * idy2);
    P[k] = c - (factor * r);
    return r;
}

}  // namespace misor
