// decomp3_check.cc -- the decomposition arithmetic of the 3D path
// (csrc/decomp3.h) on the CPU, under AddressSanitizer +
// UndefinedBehaviorSanitizer (make asan -> bin/asan/decomp3-check;
// tests/test_sanitize_cpu.py).  A wrong owned box or gather range would leave
// cells of a gathered field unwritten or written twice; here the boxes and
// ranges are marked cell by cell.
// Exit 0 and "all checks passed" when every check holds.
#include <cstdio>
#include <cstring>
#include <vector>

#include "decomp3.h"

using namespace misor;

static int fails = 0;
static int ctx_n = 0, ctx_r = 0, ctx_arg = 0;
#define CHECK(c)                                                                         \
    do {                                                                                 \
        if (!(c)) {                                                                      \
            if (++fails <= 20)                                                           \
                fprintf(stderr, "check failed %s:%d: %s (ranks %d, rank %d, arg %d)\n",  \
                        __FILE__, __LINE__, #c, ctx_n, ctx_r, ctx_arg);                  \
        }                                                                                \
    } while (0)

static char err[kDecompErr];

// the process grid of n ranks with dims_in holds n ranks, the same for every rank
static void check_dims(int n, const int* dims_in, const int* want) {
    ctx_n = n;
    for (int r = 0; r < n; ++r) {
        ctx_r = r;
        misor3_local L;
        CHECK(decompose_cart(n, r, dims_in, 64, 64, 64, &L, err) == MISOR_OK);
        CHECK(L.dims[0] * L.dims[1] * L.dims[2] == n);
        for (int a = 0; a < 3; ++a) {
            if (dims_in && dims_in[a] > 0) CHECK(L.dims[a] == dims_in[a]);
            if (want) CHECK(L.dims[a] == want[a]);
        }
    }
}

// the ranks' owned boxes cover the global array, ghost layer included, exactly
// once; neighbours are mutual
static void check_tiling(int imax, int jmax, int kmax, int dx, int dy, int dz) {
    const int n = dx * dy * dz, dims[3] = {dx, dy, dz};
    ctx_n = n;
    const long long SX = imax + 2, SXY = SX * (jmax + 2);
    std::vector<unsigned char> mark((size_t)(SXY * (kmax + 2)), 0);
    std::vector<misor3_local> locs((size_t)n);
    for (int r = 0; r < n; ++r) {
        ctx_r = r;
        misor3_local& L = locs[(size_t)r];
        CHECK(decompose_cart(n, r, dims, imax, jmax, kmax, &L, err) == MISOR_OK);
        const Span3 x = own_span(L, 0), y = own_span(L, 1), z = own_span(L, 2);
        for (int k = 0; k < z.count; ++k)
            for (int j = 0; j < y.count; ++j)
                for (int i = 0; i < x.count; ++i) {
                    const int gi = L.off[0] + x.lo + i, gj = L.off[1] + y.lo + j,
                              gk = L.off[2] + z.lo + k;
                    CHECK(0 <= gi && gi <= imax + 1 && 0 <= gj && gj <= jmax + 1 && 0 <= gk &&
                          gk <= kmax + 1);
                    unsigned char& m = mark[(size_t)(gk * SXY + gj * SX + gi)];
                    CHECK(m == 0);  // no cell twice
                    m = 1;
                }
        // a face layer lies inside the local array: ghost 0 / n + 1, owned 1 / n
        for (int s = 0; s < 6; ++s) {
            const int na = L.n[s / 2];
            CHECK(face_layer(na, s, true) == ((s & 1) ? na + 1 : 0));
            CHECK(face_layer(na, s, false) == ((s & 1) ? na : 1));
        }
    }
    ctx_r = -1;
    for (size_t q = 0; q < mark.size(); ++q) {
        ctx_arg = (int)q;
        CHECK(mark[q] == 1);  // no cell left out
    }
    ctx_arg = -1;
    for (int r = 0; r < n; ++r)
        for (int s = 0; s < 6; ++s) {
            ctx_r = r, ctx_arg = s;
            const int q = locs[(size_t)r].neighbours[s];
            CHECK(q >= -1 && q < n);
            if (q >= 0 && q < n) CHECK(locs[(size_t)q].neighbours[s ^ 1] == r);
            // ... and only if: whoever names r on side s ^ 1 is r's neighbour on side s
            for (int p = 0; p < n; ++p)
                if (locs[(size_t)p].neighbours[s ^ 1] == r) CHECK(q == p);
        }
    ctx_arg = -1;
}

// the slabs' gather ranges cover planes 0 .. kmax + 1 exactly once, ascending
static void check_slabs(int kmax, int n) {
    ctx_n = n;
    std::vector<unsigned char> mark((size_t)kmax + 2, 0);
    int next = 0, sum = 0;
    for (int r = 0; r < n; ++r) {
        ctx_r = r;
        int kl = -1, ko = -1, koff = -1;
        CHECK(decompose_slab(n, r, kmax, &kl, &ko, err) == MISOR_OK);
        CHECK(kl == size_of_rank(r, n, kmax) && kl >= kHalo && ko == sum);
        sum += kl;
        const Span3 s = slab_gather_span(n, r, kmax, &koff);
        CHECK(koff == ko);
        CHECK(koff + s.lo == next);  // the global plane of the first one: ascending, no gap
        for (int k = 0; k < s.count; ++k) {
            const int gk = koff + s.lo + k;
            CHECK(0 <= gk && gk <= kmax + 1);
            if (0 <= gk && gk <= kmax + 1) {
                CHECK(mark[(size_t)gk] == 0);
                mark[(size_t)gk] = 1;
            }
        }
        next = koff + s.lo + s.count;
    }
    CHECK(sum == kmax && next == kmax + 2);
    for (int k = 0; k < kmax + 2; ++k) CHECK(mark[(size_t)k] == 1);
}

// a refused decomposition: MISOR_EINVAL, a message, and `out` untouched
static void check_refused(int n, int r, const int* dims, int imax, int jmax, int kmax,
                          const char* what) {
    ctx_n = n, ctx_r = r;
    misor3_local L, before;
    memset(&L, 0x5a, sizeof L);
    before = L;
    err[0] = '\0';
    CHECK(decompose_cart(n, r, dims, imax, jmax, kmax, &L, err) == MISOR_EINVAL);
    CHECK(strstr(err, what) != nullptr);
    CHECK(memcmp(&L, &before, sizeof L) == 0);
}

int main() {
    for (int n = 1; n <= 16; ++n) check_dims(n, nullptr, nullptr);
    {
        const int zero[3] = {0, 0, 0}, want12[3] = {2, 2, 3};
        check_dims(12, zero, want12);
        // the partly fixed process grids of tests/test_decompose3_cart_cpu.py
        const int in[5][3] = {{4, 0, 0}, {0, 3, 0}, {0, 0, 1}, {3, 2, 1}, {3, 2, 0}};
        const int ranks[5] = {8, 12, 12, 6, 6};
        const int want[5][3] = {{4, 1, 2}, {2, 3, 2}, {3, 4, 1}, {3, 2, 1}, {3, 2, 1}};
        for (int q = 0; q < 5; ++q) check_dims(ranks[q], in[q], want[q]);
    }

    check_tiling(7, 5, 6, 3, 2, 3);
    check_tiling(13, 9, 16, 2, 2, 2);
    check_tiling(200, 50, 50, 4, 1, 2);

    for (int kmax = 16; kmax <= 17; ++kmax)
        for (int n = 1; n <= 8; ++n) check_slabs(kmax, n);

    {
        const int neg[3] = {0, -1, 0}, three[3] = {3, 0, 0}, big[3] = {2, 2, 4},
                  x2[3] = {2, 1, 1}, z4[3] = {1, 1, 4};
        check_refused(4, 4, nullptr, 64, 64, 64, "bad rank");
        check_refused(4, -1, nullptr, 64, 64, 64, "bad rank");
        check_refused(0, 0, nullptr, 64, 64, 64, "bad rank");
        check_refused(4, 0, neg, 64, 64, 64, "negative process-grid entry -1");
        check_refused(8, 0, three, 64, 64, 64, "does not hold 8 ranks");
        check_refused(8, 0, big, 64, 64, 64, "does not hold 8 ranks");
        check_refused(2, 0, x2, 3, 50, 50, "along x");
        check_refused(4, 0, z4, 50, 50, 7, "along z");
        ctx_n = 1, ctx_r = 0;
        CHECK(decompose_cart(1, 0, nullptr, 8, 8, 8, nullptr, err) == MISOR_EINVAL);
        // slabs: a bad rank, fewer than kHalo planes per slab; kloc / koff untouched
        int kl = -7, ko = -7;
        CHECK(decompose_slab(4, 4, 16, &kl, &ko, err) == MISOR_EINVAL && strstr(err, "bad rank"));
        CHECK(decompose_slab(0, 0, 16, &kl, &ko, err) == MISOR_EINVAL);
        CHECK(decompose_slab(9, 0, 17, &kl, &ko, err) == MISOR_EINVAL &&
              strstr(err, "fewer than 2 per rank"));
        CHECK(kl == -7 && ko == -7);
        CHECK(decompose_slab(8, 7, 17, nullptr, nullptr, err) == MISOR_OK);  // null outputs: fine
    }

    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
