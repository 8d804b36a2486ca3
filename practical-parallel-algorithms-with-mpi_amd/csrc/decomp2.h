// decomp2.h -- the integer arithmetic of the 2D decomposition: the block of a
// rank (misor_decompose), its 8 neighbours, the cells it contributes to a
// gather, the deepest halo a decomposition can exchange, and the regions a
// rank sends and receives at each halo depth.  Plain C++ with no device or
// communication headers, so that host/decomp2_check.cc checks it on the CPU.
// A refused decomposition returns MISOR_EINVAL with its message in err; the
// extern "C" entry point passes it to fail().
#pragma once

#include "decomp3.h"  // size_of_rank, balanced_factors, refuse

namespace misor {

// 8-neighbour halo exchange of one field (halo.hip): regions in local cell
// coordinates; direction order L, R, B, T, BL, BR, TL, TR
constexpr int kDirs = 8;
struct HaloRegion {
    int x0, y0, w, h;  // first cell and extent (local reference indices)
    long long off;     // offset in the packed buffer (doubles)
};
struct HaloPlan {
    HaloRegion send[kDirs], recv[kDirs];
    long long total;  // doubles in each of the send / recv buffers
};

}  // namespace misor

#pragma GCC visibility push(hidden)  // not exported from libmisor.so
namespace misor {

// the deepest halo any pass exchanges: 2 * kMaxT + 1, the skewed split ring's
// (misor_internal.h, which defines kMaxT, asserts the two agree)
constexpr int kMaxHaloDepth = 21;

// the ranks around process-grid position coords, in kDirs order, -1 where
// there is none (MPI_Cart_create's row-major rank order)
inline void neighbours8(const int dims[2], const int coords[2], int nbr[kDirs]) {
    const int cx = coords[0], cy = coords[1];
    auto at = [&](int x, int y) {
        return (x >= 0 && x < dims[0] && y >= 0 && y < dims[1]) ? x * dims[1] + y : -1;
    };
    const int n[kDirs] = {at(cx - 1, cy),     at(cx + 1, cy),     at(cx, cy - 1),
                          at(cx, cy + 1),     at(cx - 1, cy - 1), at(cx + 1, cy - 1),
                          at(cx - 1, cy + 1), at(cx + 1, cy + 1)};
    for (int k = 0; k < kDirs; ++k) nbr[k] = n[k];
}

// misor_decompose: the block of `rank` on the process grid dims_in (nullptr
// or an entry <= 0: MPI_Dims_create(nranks, 2), the larger factor first).
// out->pitch is the device layout's and is left 0 here (misor_decompose sets it).
inline int decompose2(int nranks, int rank, int imax, int jmax, const int dims_in[2],
                      misor_local* out, char (&err)[kDecompErr]) {
    if (!out || nranks < 1 || rank < 0 || rank >= nranks || imax < 2 || jmax < 2)
        return refuse(err, "misor_decompose: bad arguments");
    int dims[3] = {0, 0, 1};
    if (dims_in && dims_in[0] > 0 && dims_in[1] > 0) {
        dims[0] = dims_in[0];
        dims[1] = dims_in[1];
        if (dims[0] * dims[1] != nranks)
            return refuse(err, "dims %dx%d != nranks %d", dims[0], dims[1], nranks);
    } else {
        balanced_factors(nranks, 2, dims);
    }
    // MPI_Cart_create row-major rank order: coords = (rank / dims[1], rank % dims[1])
    const int cx = rank / dims[1], cy = rank % dims[1];
    misor_local L{};
    L.dims[0] = dims[0];
    L.dims[1] = dims[1];
    L.coords[0] = cx;
    L.coords[1] = cy;
    L.ni = size_of_rank(cx, dims[0], imax);
    L.nj = size_of_rank(cy, dims[1], jmax);
    for (int c = 0; c < cx; ++c) L.ioff += size_of_rank(c, dims[0], imax);
    for (int c = 0; c < cy; ++c) L.joff += size_of_rank(c, dims[1], jmax);
    int nbr[kDirs];
    neighbours8(L.dims, L.coords, nbr);
    for (int k = 0; k < 4; ++k) L.neighbours[k] = nbr[k];
    if (L.ni < 2 || L.nj < 2) return refuse(err, "local block smaller than 2x2");
    *out = L;
    return MISOR_OK;
}

// The block a rank contributes to the assembled global field: its interior
// plus the ghost layer on its physical sides (assembleResult,
// assignment-5/skeleton/src/solver.c:234-300), in local indices.
struct OwnedBlock {
    int i0, j0, w, h;    // first local cell and extent
    int gi0, gj0;        // first global cell
};
inline OwnedBlock owned_block(const misor_local& L) {
    OwnedBlock b{};
    b.i0 = L.neighbours[0] < 0 ? 0 : 1;
    b.j0 = L.neighbours[2] < 0 ? 0 : 1;
    const int i1 = L.neighbours[1] < 0 ? L.ni + 1 : L.ni;
    const int j1 = L.neighbours[3] < 0 ? L.nj + 1 : L.nj;
    b.w = i1 - b.i0 + 1;
    b.h = j1 - b.j0 + 1;
    b.gi0 = L.ioff + b.i0;
    b.gj0 = L.joff + b.j0;
    return b;
}

// halo plans exist up to this depth: kMaxHaloDepth, or as deep as the
// smallest block allows, and at least 2
inline int max_halo_depth(int imax, int jmax, const int dims[2]) {
    const int minb = imax / dims[0] < jmax / dims[1] ? imax / dims[0] : jmax / dims[1];
    const int d = kMaxHaloDepth < minb ? kMaxHaloDepth : minb;
    return d > 2 ? d : 2;
}

// Regions of the 8-neighbour exchange at halo depth d of an ni x nj block with
// neighbours nbr.  A rank sends the cells it owns (interior, plus ghost cells
// on its physical sides) next to each neighbour; ranks in one process row
// share nj and their physical top/bottom, ranks in one process column share
// ni, so send and receive extents match.
inline HaloPlan halo_plan(int ni, int nj, const int nbr[kDirs], int d) {
    const int* nb = nbr;
    const int cl = nb[0] >= 0 ? 1 : 0, ch = nb[1] >= 0 ? ni : ni + 1;
    const int rl = nb[2] >= 0 ? 1 : 0, rh = nb[3] >= 0 ? nj : nj + 1;
    HaloRegion S[kDirs] = {
        {1, rl, d, rh - rl + 1, 0},      {ni - d + 1, rl, d, rh - rl + 1, 0},
        {cl, 1, ch - cl + 1, d, 0},      {cl, nj - d + 1, ch - cl + 1, d, 0},
        {1, 1, d, d, 0},                 {ni - d + 1, 1, d, d, 0},
        {1, nj - d + 1, d, d, 0},        {ni - d + 1, nj - d + 1, d, d, 0}};
    HaloRegion R[kDirs] = {
        {1 - d, rl, d, rh - rl + 1, 0},  {ni + 1, rl, d, rh - rl + 1, 0},
        {cl, 1 - d, ch - cl + 1, d, 0},  {cl, nj + 1, ch - cl + 1, d, 0},
        {1 - d, 1 - d, d, d, 0},         {ni + 1, 1 - d, d, d, 0},
        {1 - d, nj + 1, d, d, 0},        {ni + 1, nj + 1, d, d, 0}};
    HaloPlan P{};
    long long so = 0, ro = 0;
    for (int k = 0; k < kDirs; ++k) {
        if (nb[k] < 0) S[k].w = S[k].h = R[k].w = R[k].h = 0;
        S[k].off = so;
        R[k].off = ro;
        so += (long long)S[k].w * S[k].h;
        ro += (long long)R[k].w * R[k].h;
        P.send[k] = S[k];
        P.recv[k] = R[k];
    }
    P.total = so > ro ? so : ro;
    return P;
}

}  // namespace misor
#pragma GCC visibility pop
