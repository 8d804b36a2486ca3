// mg_dist_plan.h -- the integer arithmetic of the decomposed multigrid
// hierarchy (misor_solve_mg_dist, misor_mg_dist_levels): the level rule of
// misor_mg_levels and which of its levels stay distributed over the ranks of a
// 2D decomposition.  Plain C++ with no device or communication headers, like
// decomp2.h, so every rank finds the same split from the same arithmetic before
// any device or collective call.
//
// Level 0 is distributed.  Level l >= 1 is distributed iff level l-1 is, every
// rank's block of level l-1 has even sides, the halved blocks have both sides
// >= 4 and more than gather_cells cells, and level l is the coarsest level or
// again has even block sides.  With size_of_rank "every block even" means the
// rank count divides the side with an even quotient, so all blocks of a
// distributed level are equal and the halved blocks are decompose2 of the
// halved grid: a distributed level is an ordinary decomposed grid on the same
// process grid.  The remaining levels are gathered: every rank holds them
// whole.  A hierarchy of two or more levels whose level-0 blocks have an odd
// side is refused (MISOR_ESTATE).
#pragma once

#include "decomp2.h"

#pragma GCC visibility push(hidden)  // not exported from libmisor.so
namespace misor {

// blocks of at most this many cells are gathered by default (gather_cells < 0):
// the fastest of the values measured (profiles/mg_dist_ab.txt)
constexpr int kMgGatherCells = 65536;

// next level's shape, or false where (ni, nj) is the coarsest
inline bool mg_coarsen(int ni, int nj, int coarse_cells, int* nic, int* njc) {
    if ((ni & 1) || (nj & 1) || ni < 4 || nj < 4) return false;
    if ((long long)ni * nj <= (long long)coarse_cells) return false;
    *nic = ni / 2;
    *njc = nj / 2;
    return true;
}

struct MgDistPlan {
    int nlevels;   // levels of the hierarchy (misor_mg_levels)
    int ndist;     // the first ndist of them are distributed (>= 1)
    int dims[2];   // the process grid
    int bi, bj;    // block sides of level 0 where ndist > 1 (every block is equal)
};

// MISOR_EINVAL with its message in err for bad arguments (as misor_decompose's
// and misor_mg_levels'), MISOR_ESTATE for the refused hierarchy
inline int mg_dist_plan(int nranks, const int dims_in[2], int imax, int jmax, int coarse_cells,
                        int gather_cells, MgDistPlan* out, char (&err)[kDecompErr]) {
    if (!out || nranks < 1 || imax < 2 || jmax < 2 || coarse_cells < 0)
        return refuse(err, "misor_mg_dist_levels: bad arguments");
    if (gather_cells < 0) gather_cells = kMgGatherCells;
    misor_local last{};  // the last rank's block is the smallest
    const int rc = decompose2(nranks, nranks - 1, imax, jmax, dims_in, &last, err);
    if (rc) return rc;
    MgDistPlan P{};
    P.dims[0] = last.dims[0];
    P.dims[1] = last.dims[1];
    P.nlevels = 1;
    for (int ni = imax, nj = jmax, nic = 0, njc = 0; mg_coarsen(ni, nj, coarse_cells, &nic, &njc);
         ni = nic, nj = njc)
        ++P.nlevels;
    P.ndist = 1;
    auto even = [](int b) { return (b & 1) == 0; };
    const bool even0 = imax % P.dims[0] == 0 && jmax % P.dims[1] == 0 &&
                       even(imax / P.dims[0]) && even(jmax / P.dims[1]);
    if (P.nlevels > 1 && !even0) {
        snprintf(err, sizeof err,
                 "misor_solve_mg_dist: %d x %d over %d x %d ranks has blocks with an odd side",
                 imax, jmax, P.dims[0], P.dims[1]);
        return MISOR_ESTATE;
    }
    if (P.nlevels > 1) {
        P.bi = imax / P.dims[0];
        P.bj = jmax / P.dims[1];
    }
    // (bi, bj): the blocks of level l - 1, distributed and with even sides
    for (int l = 1, bi = P.bi, bj = P.bj; l < P.nlevels; ++l) {
        bi /= 2;
        bj /= 2;
        if (bi < 4 || bj < 4) break;
        if ((long long)bi * bj <= (long long)gather_cells) break;
        if (l != P.nlevels - 1 && !(even(bi) && even(bj))) break;
        ++P.ndist;
    }
    *out = P;
    return MISOR_OK;
}

}  // namespace misor
#pragma GCC visibility pop
