// decomp3.h -- the integer arithmetic of the decompositions: sizeOfRank (2D
// and 3D), the slabs along k and the 3D Cartesian process grid of the 3D path
// (misor3_decompose, misor3_decompose_cart), and which cells of a rank's local
// array are its own (gather) or a face layer (halo exchange).  Plain C++ with
// no device or communication headers, so that host/decomp3_check.cc checks it
// on the CPU.  A refused decomposition returns MISOR_EINVAL with its message
// in err; the extern "C" entry points pass it to fail().
#pragma once

#include <cstdarg>
#include <cstdio>

#include "misor.h"

constexpr int kHalo = 2;  // halo planes per side in a 3D field's storage: a slab's least planes

#pragma GCC visibility push(hidden)  // not exported from libmisor.so
namespace misor {

constexpr int kDecompErr = 128;  // bytes of a decomposition's error message

// the message of a refused decomposition into err; returns MISOR_EINVAL
__attribute__((format(printf, 2, 3)))
inline int refuse(char (&err)[kDecompErr], const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, sizeof err, fmt, ap);
    va_end(ap);
    return MISOR_EINVAL;
}

// sizeOfRank (assignment-5/skeleton/src/solver.c:30-32, assignment-6/src/comm.c)
inline int size_of_rank(int rank, int size, int n) {
    return n / size + ((n % size > rank) ? 1 : 0);
}

// most balanced factorisation of m into three factors f[0] >= f[1] >= f[2], of
// which the last 3 - k are 1: the smallest largest factor, then the smallest
// second one (MPI_Dims_create's rule); false if there is none
inline bool balanced_factors(int m, int k, int f[3]) {
    bool found = false;
    for (int a = 1; a <= m; ++a) {
        if (m % a) continue;
        for (int b = 1; b <= a; ++b) {
            if ((m / a) % b) continue;
            const int c = m / a / b;
            if (c > b) continue;
            if ((k < 3 && c != 1) || (k < 2 && b != 1) || (k < 1 && a != 1)) continue;
            if (!found) {  // a ascends, then b: the first hit is the lexicographic minimum
                f[0] = a, f[1] = b, f[2] = c;
                found = true;
            }
        }
    }
    return found;
}

// misor3_decompose: the slab of `rank`, kloc planes from global plane koff + 1
inline int decompose_slab(int nranks, int rank, int kmax, int* kloc, int* koff,
                          char (&err)[kDecompErr]) {
    if (nranks < 1 || rank < 0 || rank >= nranks)
        return refuse(err, "bad rank %d of %d", rank, nranks);
    if (kmax / nranks < kHalo)
        return refuse(err, "%d planes over %d ranks: fewer than %d per rank", kmax, nranks,
                      kHalo);
    int off = 0;
    for (int r = 0; r < rank; ++r) off += size_of_rank(r, nranks, kmax);
    if (kloc) *kloc = size_of_rank(rank, nranks, kmax);
    if (koff) *koff = off;
    return MISOR_OK;
}

// misor3_decompose_cart: the block of `rank` on the process grid dims_in
// (entries of 0, or dims_in == nullptr: filled in)
inline int decompose_cart(int nranks, int rank, const int dims_in[3], int imax, int jmax,
                          int kmax, misor3_local* out, char (&err)[kDecompErr]) {
    if (!out) return refuse(err, "null argument");
    if (nranks < 1 || rank < 0 || rank >= nranks)
        return refuse(err, "bad rank %d of %d", rank, nranks);
    int d[3] = {0, 0, 0};
    int fixed = 1, nfree = 0;
    for (int a = 0; a < 3; ++a) {
        if (dims_in) d[a] = dims_in[a];
        if (d[a] < 0) return refuse(err, "negative process-grid entry %d", d[a]);
        if (d[a] > 0 && fixed <= nranks) fixed *= d[a];  // (stops growing once it is too big)
        if (d[a] == 0) ++nfree;
    }
    int f[3];
    if (nranks % fixed || !balanced_factors(nranks / fixed, nfree, f))
        return refuse(err, "process grid %dx%dx%d does not hold %d ranks", d[0], d[1], d[2],
                      nranks);
    for (int a = 2, q = 0; a >= 0; --a)  // the largest free factor to z, then y, then x
        if (d[a] == 0) d[a] = f[q++];
    const int N[3] = {imax, jmax, kmax};
    for (int a = 0; a < 3; ++a)
        if (N[a] / d[a] < 2)
            return refuse(err, "%d cells along %c over %d ranks: fewer than 2 per rank", N[a],
                          "xyz"[a], d[a]);
    const int c[3] = {rank % d[0], (rank / d[0]) % d[1], rank / (d[0] * d[1])};
    const int step[3] = {1, d[0], d[0] * d[1]};
    for (int a = 0; a < 3; ++a) {
        out->dims[a] = d[a];
        out->coords[a] = c[a];
        out->n[a] = size_of_rank(c[a], d[a], N[a]);
        out->off[a] = 0;
        for (int r = 0; r < c[a]; ++r) out->off[a] += size_of_rank(r, d[a], N[a]);
        out->neighbours[2 * a] = c[a] > 0 ? rank - step[a] : -1;
        out->neighbours[2 * a + 1] = c[a] < d[a] - 1 ? rank + step[a] : -1;
    }
    return MISOR_OK;
}

// `count` layers of a local array from layer `lo`, along one axis
struct Span3 {
    int lo, count;
};

// what a rank contributes to the global array along axis a: its owned cells
// plus the ghost layer on its physical sides (so with the physical edges and
// corners it holds); the ranks' boxes of these spans tile the global array
// exactly once
inline Span3 own_span(const misor3_local& L, int a) {
    const int lo = L.neighbours[2 * a] < 0 ? 0 : 1;
    const int hi = L.neighbours[2 * a + 1] < 0 ? L.n[a] + 1 : L.n[a];
    return {lo, hi - lo + 1};
}

// the layer of side s (low side: s even) along its axis of n owned cells: the
// ghost layer (halo) or the owned layer next to it
inline int face_layer(int n, int s, bool halo) {
    return (s & 1) ? (halo ? n + 1 : n) : (halo ? 0 : 1);
}

// the planes slab r of nranks contributes to a gather: its planes 1 .. K, plus
// plane 0 / K + 1 where they are the physical ghost planes; local plane lo is
// global plane *koff + lo
inline Span3 slab_gather_span(int nranks, int r, int kmax, int* koff) {
    char err[kDecompErr];
    int kl = 0;
    *koff = 0;
    decompose_slab(nranks, r, kmax, &kl, koff, err);
    const int k_first = (r == 0) ? 0 : 1;
    const int k_last = (r == nranks - 1) ? kl + 1 : kl;
    return {k_first, k_last - k_first + 1};
}

}  // namespace misor
#pragma GCC visibility pop
