// mg3_dist_plan.h -- the integer arithmetic of the decomposed 3D multigrid
// hierarchy (misor3_solve_mg_dist, misor3_mg_dist_levels): the level rule of
// misor3_mg_levels and which of its levels stay distributed over the slabs of
// misor3_decompose.  Plain C++ with no device or communication headers, like
// mg_dist_plan.h and decomp3.h, so every rank finds the same split from the
// same arithmetic before any device or collective call, and
// host/mg3_dist_plan_check.cc checks it on the CPU.
//
// Level 0 is distributed.  Level l >= 1 is distributed iff level l-1 is, every
// slab of level l-1 has an even number of planes, the halved slabs have at
// least 4 planes and more than gather_cells cells (imax_l jmax_l kloc_l), and
// level l is the coarsest level or its slabs have even plane counts again.
// With size_of_rank "every slab even" means the rank count divides the level's
// kmax with an even quotient, so all slabs of a distributed level are equal,
// koff is even and the halved slabs are decompose_slab of the halved grid: a
// distributed level is an ordinary slab grid on the same ranks.  The remaining
// levels are gathered: every rank holds them whole.  A hierarchy of two or
// more levels on level-0 slabs with an odd plane count is refused
// (MISOR_ESTATE).
#pragma once

#include "decomp3.h"

#pragma GCC visibility push(hidden)  // not exported from libmisor.so
namespace misor {

// halved slabs of at most this many cells are gathered by default
// (gather_cells < 0): the fastest of the values measured
// (profiles/mg3_dist_ab.txt), which was the largest of them
constexpr int kMg3GatherCells = 2097152;

// next level's shape, or false where n[] is the coarsest
inline bool mg3_coarsen(const int n[3], int coarse_cells, int nc[3]) {
    for (int a = 0; a < 3; ++a)
        if ((n[a] & 1) || n[a] < 4) return false;
    if ((long long)n[0] * n[1] * n[2] <= (long long)coarse_cells) return false;
    for (int a = 0; a < 3; ++a) nc[a] = n[a] / 2;
    return true;
}

struct Mg3DistPlan {
    int nlevels;  // levels of the hierarchy (misor3_mg_levels)
    int ndist;    // the first ndist of them are distributed (>= 1)
    int nranks;
    int kslab;    // planes of every level-0 slab where nlevels > 1 (all slabs are equal)
};

// MISOR_EINVAL with its message in err for bad arguments (misor3_decompose's
// and misor3_mg_levels' cases), MISOR_ESTATE for the refused hierarchy
inline int mg3_dist_plan(int nranks, int imax, int jmax, int kmax, int coarse_cells,
                         int gather_cells, Mg3DistPlan* out, char (&err)[kDecompErr]) {
    if (!out || imax < 2 || jmax < 2 || kmax < 2 || coarse_cells < 0)
        return refuse(err, "misor3_mg_dist_levels: bad arguments");
    if (gather_cells < 0) gather_cells = kMg3GatherCells;
    const int rc = decompose_slab(nranks, nranks < 1 ? 0 : nranks - 1, kmax, nullptr, nullptr, err);
    if (rc) return rc;
    Mg3DistPlan P{};
    P.nranks = nranks;
    P.nlevels = 1;
    int n[3] = {imax, jmax, kmax}, nc[3];
    while (mg3_coarsen(n, coarse_cells, nc)) {
        ++P.nlevels;
        for (int a = 0; a < 3; ++a) n[a] = nc[a];
    }
    P.ndist = 1;
    auto even = [](int b) { return (b & 1) == 0; };
    if (P.nlevels > 1) {
        if (kmax % nranks != 0 || !even(kmax / nranks)) {
            snprintf(err, sizeof err,
                     "misor3_solve_mg_dist: %d planes over %d ranks has slabs with an odd plane "
                     "count",
                     kmax, nranks);
            return MISOR_ESTATE;
        }
        P.kslab = kmax / nranks;
    }
    // (ni, nj, ks): level l - 1, distributed and with even slabs
    for (int l = 1, ni = imax, nj = jmax, ks = P.kslab; l < P.nlevels; ++l) {
        ni /= 2;
        nj /= 2;
        ks /= 2;
        if (ks < 4) break;
        if ((long long)ni * nj * ks <= (long long)gather_cells) break;
        if (l != P.nlevels - 1 && !even(ks)) break;
        ++P.ndist;
    }
    *out = P;
    return MISOR_OK;
}

// the slab of `rank` on distributed level l >= 1 of plan P (on level 0 the
// slab is misor3_decompose's, even where the slabs differ): kloc planes from
// the level's global plane koff + 1
inline void mg3_dist_slab(const Mg3DistPlan& P, int rank, int l, int* kloc, int* koff) {
    const int ks = P.kslab >> l;
    *kloc = ks;
    *koff = rank * ks;
}

}  // namespace misor
#pragma GCC visibility pop
