// halo3.hip -- pack / unpack of a box of cells of one 3D field (reference
// layout, i fastest) into / from a contiguous buffer: the x and y faces of a
// Cartesian block's halo exchange and the block a rank contributes to
// misor3_gather (misor3d_api.hip).  z faces are whole planes, contiguous in
// this layout, and never come through here.
//
// The buffer is packed x fastest, then y, then z, and consecutive threads take
// consecutive buffer elements, so the buffer side of every copy is coalesced.
// The field side:
//  - y face (ny = 1): nz runs of nx = ni+2 consecutive doubles, sxy apart --
//    a wavefront reads whole 512-byte stretches of a row;
//  - gather box: runs of nx consecutive doubles, the same;
//  - x face (nx = 1): consecutive lanes take consecutive j of one k, sx
//    doubles apart.  Each lane touches its own cache line on the field side --
//    that is the face's layout, one cell per row -- while the 64 values of a
//    wavefront leave (arrive) as one contiguous 512-byte store (load) on the
//    buffer side, so the message itself is dense.
// Bandwidth is not the point at these sizes (a 200x50x50 box on 2x2x2 ranks:
// x faces of 27 x 27 doubles); the launches are latency-bound.

#include "misor_internal.h"

namespace misor {

namespace {

template <bool PACK>
__global__ __launch_bounds__(256) void k3_box_copy(double* __restrict__ field, Box3 b,
                                                   double* __restrict__ buf) {
    const long long n = (long long)b.nx * b.ny * b.nz;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int x = (int)(e % b.nx);
    const long long r = e / b.nx;
    const int y = (int)(r % b.ny), z = (int)(r / b.ny);
    double* cell = field + (long long)(b.z0 + z) * b.sxy + (long long)(b.y0 + y) * b.sx +
                   (b.x0 + x);
    if (PACK)
        buf[e] = *cell;
    else
        *cell = buf[e];
}

}  // namespace

void launch3_box_pack(hipStream_t s, const double* field, const Box3& b, double* buf) {
    const long long n = b.cells();
    if (n <= 0) return;
    hipLaunchKernelGGL(k3_box_copy<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       const_cast<double*>(field), b, buf);
}

void launch3_box_unpack(hipStream_t s, double* field, const Box3& b, const double* buf) {
    const long long n = b.cells();
    if (n <= 0) return;
    hipLaunchKernelGGL(k3_box_copy<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       field, b, const_cast<double*>(buf));
}

}  // namespace misor
