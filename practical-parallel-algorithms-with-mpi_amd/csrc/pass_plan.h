// pass_plan.h -- the integer arithmetic of the red-black solve loop's pass plan
// (misor_solve.hip): how the iterations still to do are dealt to passes, and
// when a capped solve takes the short plan.  Plain C++ with no device or
// communication headers, so that host/pass_plan_check.cc checks it on the CPU.
#pragma once

#include <algorithm>

namespace misor {

// The passes of a solve with `todo` (>= 1) iterations still to do and at most T
// (>= 1) iterations a pass.  The cap takes max_passes passes of at most T
// iterations (no pass overshoots it); they are made as even as possible --
// `extra` passes of base + 1, the rest of base -- because a pass costs nearly
// as much with fewer iterations (a T' = 4 pass at 32768^2 is HBM-bound at 5.06
// ms against 5.41 for T = 8), so 20 iterations run as 7 + 7 + 6 rather than
// 8 + 8 + 4.  A solve that converges earlier stops at the same iteration
// either way.
struct PassPlan {
    long long todo, T, max_passes, base, extra;

    PassPlan(long long todo_, long long T_)
        : todo(todo_),
          T(T_),
          max_passes((todo_ + T_ - 1) / T_),
          base(todo_ / max_passes),
          extra(todo_ % max_passes) {}

    // iterations pass k performs
    int iters_of(long long k) const { return (int)(base + (k < extra ? 1 : 0)); }
    // iterations covered by the first p passes
    long long covered(long long p) const { return p * base + std::min(p, extra); }
    // the passes that cover `it` iterations (0 for it = 0: a resumed solve
    // that is already done)
    long long passes_for(long long it) const {
        const long long head = extra * (base + 1);  // iterations of the longer passes
        if (it <= head) return (it + base) / (base + 1);
        return std::min(extra + (it - head + base - 1) / base, max_passes);
    }
};

// The short plan's rule where a short_t-iteration pass costs more than a
// default_t one: the split-ring kernel runs kShortT = 10 iterations a pass at
// ~1.4 x the time of a T = 8 pass (profiles/r04_ab_splitring.txt), so a solve
// of `todo` iterations takes it where its passes times 1.4 (7 / 5) undercut
// the default's pass count -- with 10 and 8, 9-10 and 17-20 iterations (the
// driver's 20-iteration solve: 2 passes instead of 7 + 7 + 6).
inline bool short_plan_saves_passes(int todo, int short_t, int default_t) {
    return 7LL * ((todo + short_t - 1) / short_t) < 5LL * ((todo + default_t - 1) / default_t);
}

}  // namespace misor
