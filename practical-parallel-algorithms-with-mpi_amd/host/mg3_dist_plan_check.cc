// mg3_dist_plan_check.cc -- the level split of the decomposed 3D multigrid
// (csrc/mg3_dist_plan.h) on the CPU, under AddressSanitizer +
// UndefinedBehaviorSanitizer (make asan -> bin/asan/mg3-dist-plan-check;
// tests/test_mg3_dist_cpu.py).  The plan is swept over 1..8 ranks and up to 64
// planes against a brute-force restatement that walks every rank's slab of
// every level (size_of_rank, no divisibility shortcut), and every distributed
// level's slab is checked to be decompose_slab of the halved grid.
// Exit 0 and "all checks passed" when every check holds.
#include <cstdio>
#include <vector>

#include "mg3_dist_plan.h"

using namespace misor;

static int fails = 0;
static int ctx[6];
#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            if (++fails <= 20)                                                            \
                fprintf(stderr, "check failed %s:%d: %s (ranks %d, %d x %d x %d, cc %d, " \
                        "gc %d)\n", __FILE__, __LINE__, #c, ctx[0], ctx[1], ctx[2], ctx[3], \
                        ctx[4], ctx[5]);                                                  \
        }                                                                                 \
    } while (0)

static char err[kDecompErr];

struct Shape {
    int n[3];
};

// the rule of include/misor.h, level by level over every rank's slab; returns
// MISOR_ESTATE, or MISOR_OK with *nlevels and *ndist
static int brute(int nranks, int imax, int jmax, int kmax, int cc, int gc, int* nlevels,
                 int* ndist) {
    if (gc < 0) gc = kMg3GatherCells;
    std::vector<Shape> sh;
    sh.push_back({{imax, jmax, kmax}});
    for (;;) {
        const Shape s = sh.back();
        bool stop = (long long)s.n[0] * s.n[1] * s.n[2] <= (long long)cc;
        for (int a = 0; a < 3; ++a) stop = stop || (s.n[a] % 2) || s.n[a] < 4;
        if (stop) break;
        sh.push_back({{s.n[0] / 2, s.n[1] / 2, s.n[2] / 2}});
    }
    auto slabs = [&](const Shape& s) {
        std::vector<int> k;
        for (int r = 0; r < nranks; ++r) k.push_back(size_of_rank(r, nranks, s.n[2]));
        return k;
    };
    auto even = [&](const Shape& s) {
        for (int k : slabs(s))
            if (k % 2) return false;
        return true;
    };
    const int L = (int)sh.size();
    if (L > 1 && !even(sh[0])) return MISOR_ESTATE;
    int nd = 1;
    for (int l = 1; l < L; ++l) {
        if (!even(sh[l - 1])) break;
        bool ok = true;
        for (int k : slabs(sh[l - 1])) {
            const int h = k / 2;
            if (h < 4 || (long long)sh[l].n[0] * sh[l].n[1] * h <= (long long)gc) ok = false;
        }
        if (!ok) break;
        if (l != L - 1 && !even(sh[l])) break;
        ++nd;
    }
    *nlevels = L;
    *ndist = nd;
    return MISOR_OK;
}

int main() {
    long long cases = 0, refused = 0, split = 0, all_dist = 0;
    const int sides[] = {2, 4, 7, 8, 16, 24, 64};
    const int ccs[] = {0, 1, 64, 512, 5000};
    const int gcs[] = {-1, 0, 15, 16, 64, 4096, 1000000000};  // -1: the default
    for (int nranks = 1; nranks <= 8; ++nranks)
        for (int kmax = 2; kmax <= 64; ++kmax)
            for (int imax : sides)
                for (int jmax : sides)
                    for (int cc : ccs)
                        for (int gc : gcs) {
                            ctx[0] = nranks, ctx[1] = imax, ctx[2] = jmax, ctx[3] = kmax;
                            ctx[4] = cc, ctx[5] = gc;
                            Mg3DistPlan P{-7, -7, -7, -7};
                            const int rc = mg3_dist_plan(nranks, imax, jmax, kmax, cc, gc, &P, err);
                            if (kmax / nranks < kHalo) {
                                CHECK(rc == MISOR_EINVAL && P.nlevels == -7 && P.ndist == -7);
                                continue;
                            }
                            ++cases;
                            int nl = 0, nd = 0;
                            const int want = brute(nranks, imax, jmax, kmax, cc, gc, &nl, &nd);
                            CHECK(rc == want);
                            if (rc != MISOR_OK) {
                                CHECK(P.nlevels == -7 && P.ndist == -7);  // untouched
                                ++refused;
                                continue;
                            }
                            CHECK(P.nlevels == nl && P.ndist == nd);
                            CHECK(P.ndist >= 1 && P.ndist <= P.nlevels && P.nranks == nranks);
                            split += P.ndist > 1 && P.ndist < P.nlevels;
                            all_dist += P.ndist > 1 && P.ndist == P.nlevels;
                            // every distributed level below level 0: the halved slab is the slab
                            // of the halved grid, of >= 4 planes and more than gc cells
                            int kup = 0, oup = 0;
                            for (int l = 1; l < P.ndist; ++l)
                                for (int r = 0; r < nranks; ++r) {
                                    int kl = 0, ko = 0, kd = -1, od = -1;
                                    mg3_dist_slab(P, r, l, &kl, &ko);
                                    CHECK(decompose_slab(nranks, r, kmax >> l, &kd, &od, err) ==
                                          MISOR_OK);
                                    CHECK(kl == kd && ko == od && kl >= 4);
                                    CHECK(decompose_slab(nranks, r, kmax >> (l - 1), &kup, &oup,
                                                         err) == MISOR_OK);
                                    CHECK(2 * kl == kup && 2 * ko == oup);
                                    const int g = gc < 0 ? kMg3GatherCells : gc;
                                    CHECK((long long)(imax >> l) * (jmax >> l) * kl > (long long)g);
                                }
                        }
    // bad arguments: MISOR_EINVAL, the plan untouched
    Mg3DistPlan P{-7, -7, -7, -7};
    CHECK(mg3_dist_plan(0, 8, 8, 8, 1, 0, &P, err) == MISOR_EINVAL);
    CHECK(mg3_dist_plan(2, 1, 8, 8, 1, 0, &P, err) == MISOR_EINVAL);
    CHECK(mg3_dist_plan(2, 8, 1, 8, 1, 0, &P, err) == MISOR_EINVAL);
    CHECK(mg3_dist_plan(2, 8, 8, 8, -1, 0, &P, err) == MISOR_EINVAL);
    CHECK(mg3_dist_plan(5, 8, 8, 8, 1, 0, &P, err) == MISOR_EINVAL);  // fewer than 2 planes each
    CHECK(mg3_dist_plan(2, 8, 8, 8, 1, 0, nullptr, err) == MISOR_EINVAL);
    CHECK(P.nlevels == -7 && P.ndist == -7);
    CHECK(refused > 0 && split > 0 && all_dist > 0);  // the sweep meets every outcome
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("all checks passed (%lld plans, %lld refused, %lld split, %lld fully distributed)\n",
           cases, refused, split, all_dist);
    return 0;
}
