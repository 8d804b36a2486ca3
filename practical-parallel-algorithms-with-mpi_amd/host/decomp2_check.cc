// decomp2_check.cc -- the 2D decomposition and its halo plans (csrc/decomp2.h)
// on the CPU, under AddressSanitizer + UndefinedBehaviorSanitizer (make asan
// -> bin/asan/decomp2-check; tests/test_sanitize_cpu.py).  This arithmetic
// decides which cells a rank sends to which neighbour: a wrong region would
// put a neighbour's cells in the wrong place or leave halo cells stale.  Here
// every region of every rank at every depth is followed cell by cell.
// Exit 0 and "all checks passed" when every check holds.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "decomp2.h"

using namespace misor;

static int fails = 0;
static int ctx_n = 0, ctx_r = 0, ctx_d = 0, ctx_k = 0;
#define CHECK(c)                                                                            \
    do {                                                                                    \
        if (!(c)) {                                                                         \
            if (++fails <= 20)                                                              \
                fprintf(stderr, "check failed %s:%d: %s (ranks %d, rank %d, depth %d, "    \
                                "dir %d)\n",                                                \
                        __FILE__, __LINE__, #c, ctx_n, ctx_r, ctx_d, ctx_k);                \
        }                                                                                   \
    } while (0)

static char err[kDecompErr];
static const int opposite[kDirs] = {1, 0, 3, 2, 7, 6, 5, 4};
// the two side neighbours a corner neighbour lies between
static const int corner_sides[kDirs][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0},
                                           {0, 2}, {1, 2}, {0, 3}, {1, 3}};

// MPI_Dims_create(n, 2) for n = 1..64, recorded from the dims_create that
// balanced_factors(n, 2, f) replaced: its second (smaller) factor; the first
// is n over it
static const int dims1[65] = {0, 1, 1, 1, 2, 1, 2, 1, 2, 3, 2, 1, 3, 1, 2, 3, 4,
                              1, 3, 1, 4, 3, 2, 1, 4, 5, 2, 3, 4, 1, 5, 1, 4,
                              3, 2, 5, 6, 1, 2, 3, 5, 1, 6, 1, 4, 5, 2, 1, 6,
                              7, 5, 3, 4, 1, 6, 5, 7, 3, 2, 1, 6, 1, 2, 7, 8};

static void check_process_grid() {
    ctx_r = 0;
    for (int n = 1; n <= 64; ++n) {
        ctx_n = n;
        misor_local L;
        CHECK(decompose2(n, 0, 1024, 1024, nullptr, &L, err) == MISOR_OK);
        CHECK(L.dims[1] == dims1[n] && L.dims[0] == n / dims1[n]);
        const int zero[2] = {0, 0}, half[2] = {n, 0};  // an entry <= 0: filled in, both
        misor_local Z, H;
        CHECK(decompose2(n, 0, 1024, 1024, zero, &Z, err) == MISOR_OK);
        CHECK(decompose2(n, 0, 1024, 1024, half, &H, err) == MISOR_OK);
        CHECK(memcmp(&Z, &L, sizeof L) == 0 && memcmp(&H, &L, sizeof L) == 0);
    }
}

struct Cell {
    int gi, gj;
};

// one decomposition: n ranks on dims_in (nullptr: filled in) over imax x jmax.
// false: refused for some rank (a block under 2x2), nothing checked.
static bool check_case(int n, const int* dims_in, int imax, int jmax) {
    ctx_n = n, ctx_d = 0, ctx_k = -1;
    std::vector<misor_local> loc((size_t)n);
    for (int r = 0; r < n; ++r) {
        ctx_r = r;
        if (decompose2(n, r, imax, jmax, dims_in, &loc[r], err) != MISOR_OK) {
            CHECK(strcmp(err, "local block smaller than 2x2") == 0);
            return false;
        }
    }
    const int* dims = loc[0].dims;
    const int W = imax + 2, H = jmax + 2;

    // the block of every rank; the owned blocks tile the global array
    std::vector<int> mark((size_t)W * H, 0);
    for (int r = 0; r < n; ++r) {
        ctx_r = r;
        const misor_local& L = loc[r];
        CHECK(L.dims[0] == dims[0] && L.dims[1] == dims[1] && dims[0] * dims[1] == n);
        if (dims_in && dims_in[0] > 0 && dims_in[1] > 0)
            CHECK(dims[0] == dims_in[0] && dims[1] == dims_in[1]);
        CHECK(L.coords[0] == r / dims[1] && L.coords[1] == r % dims[1]);
        CHECK(L.ni == size_of_rank(L.coords[0], dims[0], imax));
        CHECK(L.nj == size_of_rank(L.coords[1], dims[1], jmax));
        CHECK(L.ni >= 2 && L.nj >= 2 && L.pitch == 0);
        const OwnedBlock b = owned_block(L);
        CHECK(b.gi0 == L.ioff + b.i0 && b.gj0 == L.joff + b.j0);
        for (int j = 0; j < b.h; ++j)
            for (int i = 0; i < b.w; ++i) {
                const int gi = b.gi0 + i, gj = b.gj0 + j;
                CHECK(0 <= gi && gi < W && 0 <= gj && gj < H);
                if (0 <= gi && gi < W && 0 <= gj && gj < H) ++mark[(size_t)gj * W + gi];
            }
    }
    ctx_r = -1;
    for (size_t q = 0; q < mark.size(); ++q) CHECK(mark[q] == 1);  // every cell exactly once

    // the 8-neighbour tables
    std::vector<int> nbr((size_t)n * kDirs);
    for (int r = 0; r < n; ++r) neighbours8(loc[r].dims, loc[r].coords, &nbr[(size_t)r * kDirs]);
    for (int r = 0; r < n; ++r)
        for (int k = 0; k < kDirs; ++k) {
            ctx_r = r, ctx_k = k;
            const int* nb = &nbr[(size_t)r * kDirs];
            const int q = nb[k];
            CHECK(q >= -1 && q < n && q != r);
            if (q >= 0 && q < n) CHECK(nbr[(size_t)q * kDirs + opposite[k]] == r);  // mutual
            if (k < 4) CHECK(loc[r].neighbours[k] == q);
            if (k >= 4)
                CHECK((q >= 0) == (nb[corner_sides[k][0]] >= 0 && nb[corner_sides[k][1]] >= 0));
        }

    // the halo plans of every depth
    const int maxd = max_halo_depth(imax, jmax, dims);
    {
        int minb = imax;
        for (int r = 0; r < n; ++r) minb = std::min(minb, std::min(loc[r].ni, loc[r].nj));
        CHECK(maxd == std::max(2, std::min(kMaxHaloDepth, minb)));
        CHECK(maxd <= minb);  // (a block is at least 2 x 2)
    }
    std::vector<HaloPlan> plan((size_t)n);
    for (int d = 1; d <= maxd; ++d) {
        ctx_d = d;
        for (int r = 0; r < n; ++r)
            plan[r] = halo_plan(loc[r].ni, loc[r].nj, &nbr[(size_t)r * kDirs], d);
        for (int r = 0; r < n; ++r) {
            ctx_r = r;
            const misor_local& L = loc[r];
            const HaloPlan& P = plan[r];
            const int* nb = &nbr[(size_t)r * kDirs];
            const OwnedBlock own = owned_block(L);
            auto owned_by = [](const OwnedBlock& b, int gi, int gj) {
                return b.gi0 <= gi && gi < b.gi0 + b.w && b.gj0 <= gj && gj < b.gj0 + b.h;
            };
            long long so = 0, ro = 0;
            std::fill(mark.begin(), mark.end(), 0);  // the cells r receives
            for (int k = 0; k < kDirs; ++k) {
                ctx_k = k;
                const HaloRegion &S = P.send[k], &R = P.recv[k];
                CHECK(S.off == so && R.off == ro);  // contiguous in direction order
                CHECK(S.w >= 0 && S.h >= 0 && R.w >= 0 && R.h >= 0);
                so += (long long)S.w * S.h;
                ro += (long long)R.w * R.h;
                if (nb[k] < 0) {
                    CHECK(S.w == 0 && S.h == 0 && R.w == 0 && R.h == 0);
                    continue;
                }
                CHECK(S.w > 0 && S.h > 0);
                // what r sends towards k is what its neighbour receives from the
                // opposite direction: same extent, same global cells
                const misor_local& Q = loc[nb[k]];
                const HaloRegion& T = plan[nb[k]].recv[opposite[k]];
                CHECK(S.w == T.w && S.h == T.h);
                for (int y = 0; y < S.h && y < T.h; ++y)
                    for (int x = 0; x < S.w && x < T.w; ++x) {
                        const Cell s = {L.ioff + S.x0 + x, L.joff + S.y0 + y};
                        const Cell t = {Q.ioff + T.x0 + x, Q.joff + T.y0 + y};
                        CHECK(s.gi == t.gi && s.gj == t.gj);
                        CHECK(owned_by(own, s.gi, s.gj));  // r sends only its own cells
                    }
                for (int y = 0; y < R.h; ++y)
                    for (int x = 0; x < R.w; ++x) {
                        const int gi = L.ioff + R.x0 + x, gj = L.joff + R.y0 + y;
                        CHECK(0 <= gi && gi < W && 0 <= gj && gj < H);
                        CHECK(!owned_by(own, gi, gj));  // never over its own cells
                        if (0 <= gi && gi < W && 0 <= gj && gj < H) ++mark[(size_t)gj * W + gi];
                    }
            }
            ctx_k = -1;
            CHECK(P.total == std::max(so, ro));
            // together, each cell once: the block grown by d, clipped to the
            // global array, without r's own cells
            const int bi0 = std::max(0, L.ioff + 1 - d), bi1 = std::min(W - 1, L.ioff + L.ni + d);
            const int bj0 = std::max(0, L.joff + 1 - d), bj1 = std::min(H - 1, L.joff + L.nj + d);
            for (int gj = 0; gj < H; ++gj)
                for (int gi = 0; gi < W; ++gi) {
                    const bool in_box = bi0 <= gi && gi <= bi1 && bj0 <= gj && gj <= bj1;
                    CHECK(mark[(size_t)gj * W + gi] == (in_box && !owned_by(own, gi, gj) ? 1 : 0));
                }
        }
    }
    return true;
}

// a refused decomposition: MISOR_EINVAL, its message, and `out` untouched
static void check_refused(int n, int r, int imax, int jmax, const int* dims, const char* what) {
    ctx_n = n, ctx_r = r, ctx_d = 0, ctx_k = -1;
    misor_local L, before;
    memset(&L, 0x5a, sizeof L);
    before = L;
    err[0] = '\0';
    CHECK(decompose2(n, r, imax, jmax, dims, &L, err) == MISOR_EINVAL);
    CHECK(strcmp(err, what) == 0);
    CHECK(memcmp(&L, &before, sizeof L) == 0);
}

int main() {
    check_process_grid();

    const int sizes[4][2] = {{64, 64}, {61, 43}, {45, 46}, {17, 11}};
    int ran = 0, skipped = 0;
    for (const auto& sz : sizes) {
        for (int n = 1; n <= 16; ++n) {
            const int row[2] = {1, n}, col[2] = {n, 1};
            (check_case(n, nullptr, sz[0], sz[1]) ? ran : skipped)++;
            (check_case(n, row, sz[0], sz[1]) ? ran : skipped)++;
            (check_case(n, col, sz[0], sz[1]) ? ran : skipped)++;
        }
        const int grids[3][2] = {{3, 2}, {2, 3}, {2, 4}};
        for (const auto& g : grids) (check_case(g[0] * g[1], g, sz[0], sz[1]) ? ran : skipped)++;
    }
    ctx_n = ran, ctx_r = skipped, ctx_d = 0, ctx_k = -1;
    // refused: only on 17 x 11 -- 1 x n from n = 6 (11 cells), n x 1 from n = 9
    // (17 cells), and the filled-in 11 x 1 and 13 x 1
    CHECK(ran + skipped == 4 * (3 * 16 + 3) && skipped == 11 + 8 + 2);
    {  // the two exchange tests' decompositions (tests/test_decomposed_gpu.py)
        const int d22[2] = {2, 2}, d32[2] = {3, 2};
        CHECK(check_case(4, d22, 44, 46) && max_halo_depth(44, 46, d22) == 21);
        CHECK(check_case(6, d32, 17, 11) && max_halo_depth(17, 11, d32) == 5);
    }

    {
        const int d32[2] = {3, 2}, d51[2] = {5, 1};
        check_refused(4, 4, 64, 64, nullptr, "misor_decompose: bad arguments");
        check_refused(4, -1, 64, 64, nullptr, "misor_decompose: bad arguments");
        check_refused(0, 0, 64, 64, nullptr, "misor_decompose: bad arguments");
        check_refused(1, 0, 1, 64, nullptr, "misor_decompose: bad arguments");
        check_refused(4, 0, 64, 64, d32, "dims 3x2 != nranks 4");
        check_refused(6, 0, 64, 64, d51, "dims 5x1 != nranks 6");
        check_refused(64, 63, 10, 10, nullptr, "local block smaller than 2x2");
        ctx_n = 1, ctx_r = 0;
        err[0] = '\0';
        CHECK(decompose2(1, 0, 8, 8, nullptr, nullptr, err) == MISOR_EINVAL);
        CHECK(strcmp(err, "misor_decompose: bad arguments") == 0);
    }

    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
