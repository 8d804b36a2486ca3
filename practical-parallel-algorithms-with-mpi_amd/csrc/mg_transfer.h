// mg_transfer.h -- the expressions of the multigrid transfers, shared by the
// streaming kernels of mg_kernels.hip and the LDS-resident cycle of
// mg_tail.hip, so that a transfer gives the same bits whichever runs it.
// Device code only; compile with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

namespace misor {

// solveRB's residual of one cell (assignment-4/src/solver.c:204-210): centre
// c, west / east / south / north
__device__ __forceinline__ double mg_resid(double rhs, double c, double w, double e, double s,
                                           double n, double idx2, double idy2) {
    return rhs - ((e - 2.0 * c + w) * idx2 + (n - 2.0 * c + s) * idy2);
}

// rc(I,J) from the residuals of its four fine cells: r00 = r(2I-1,2J-1),
// r10 = r(2I,2J-1), r01 = r(2I-1,2J), r11 = r(2I,2J)
__device__ __forceinline__ double mg_restrict4(double r00, double r10, double r01, double r11) {
    return 0.25 * ((r00 + r10) + (r01 + r11));
}

// the correction of a fine cell with parent c: x / y the parent's neighbour
// towards the cell along i / j, xy the diagonal one (indices clamped)
__device__ __forceinline__ double mg_interp(double c, double x, double y, double xy) {
    return (9.0 * c + 3.0 * (x + y) + xy) * 0.0625;
}

}  // namespace misor
