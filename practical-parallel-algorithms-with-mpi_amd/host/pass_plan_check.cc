// pass_plan_check.cc -- the pass-plan arithmetic of the red-black solve loop
// (csrc/pass_plan.h) on the CPU, under AddressSanitizer +
// UndefinedBehaviorSanitizer (make asan -> bin/asan/pass-plan-check;
// tests/test_sanitize_cpu.py).  An off-by-one in passes_for or covered would
// leave the solve's result in the wrong pressure buffer; here every plan of
// 1..400 iterations in passes of 1..10 is checked exhaustively.
// Exit 0 and "all checks passed" when every check holds.
#include <cstdio>

#include "pass_plan.h"

using misor::PassPlan;
using misor::short_plan_saves_passes;

static int fails = 0;
static long long ctx_todo = 0, ctx_T = 0, ctx_arg = 0;
#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            if (++fails <= 20)                                                            \
                fprintf(stderr, "check failed %s:%d: %s (todo %lld, T %lld, arg %lld)\n", \
                        __FILE__, __LINE__, #c, ctx_todo, ctx_T, ctx_arg);                \
        }                                                                                 \
    } while (0)

static void check_plan(long long todo, long long T) {
    ctx_todo = todo;
    ctx_T = T;
    ctx_arg = -1;
    const PassPlan p(todo, T);
    CHECK(p.todo == todo && p.T == T);
    CHECK(p.max_passes == (todo + T - 1) / T);
    long long sum = 0;
    for (long long k = 0; k < p.max_passes; ++k) {
        ctx_arg = k;
        const int n = p.iters_of(k);
        CHECK(1 <= n && n <= T);
        if (k + 1 < p.max_passes) {
            const int d = n - p.iters_of(k + 1);
            CHECK(d == 0 || d == 1);
        }
        sum += n;
        CHECK(p.covered(k + 1) == sum);
    }
    ctx_arg = -1;
    CHECK(sum == todo);
    CHECK(p.covered(p.max_passes) == todo);
    CHECK(p.covered(0) == 0);
    CHECK(p.passes_for(0) == 0);
    for (long long it = 1; it <= todo; ++it) {
        ctx_arg = it;
        const long long n = p.passes_for(it);
        CHECK(1 <= n && n <= p.max_passes);
        CHECK(p.covered(n) >= it);
        CHECK(it > p.covered(n - 1));
    }
}

static void check_known(long long todo, long long T, const int* want, long long n) {
    ctx_todo = todo;
    ctx_T = T;
    const PassPlan p(todo, T);
    ctx_arg = -1;
    CHECK(p.max_passes == n);
    for (long long k = 0; k < n && k < p.max_passes; ++k) {
        ctx_arg = k;
        CHECK(p.iters_of(k) == want[k]);
    }
}

int main() {
    for (long long T = 1; T <= 10; ++T)
        for (long long todo = 1; todo <= 400; ++todo) check_plan(todo, T);

    const int even20[] = {7, 7, 6}, short20[] = {10, 10};
    check_known(20, 8, even20, 3);
    check_known(20, 10, short20, 2);
    ctx_todo = 100, ctx_T = 8, ctx_arg = -1;
    CHECK(PassPlan(100, 8).max_passes == 13);

    // the short plan's rule for 10-iteration passes against 8-iteration ones,
    // todo = 1..40, recorded from the expression this function replaced
    // (7 * ceil(todo / 10) < 5 * ceil(todo / 8)): true for 9, 10 and 17..20
    static const int saves[41] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1,
                                  0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    ctx_T = 10;
    for (int todo = 1; todo <= 40; ++todo) {
        ctx_todo = ctx_arg = todo;
        CHECK(short_plan_saves_passes(todo, 10, 8) == (saves[todo] != 0));
    }

    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
