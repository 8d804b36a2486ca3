// misor_plan.hip -- the device side of the launch plans (tb_plan.h holds their
// arithmetic): the partials buffer, the single-sweep configuration, the
// temporally blocked passes' configuration (streams, events, work areas) and
// the upload of the segment lists of chained passes (misor_grid.h).

#include "misor_grid.h"

int ensure_partials(misor_grid* g, int n) {
    if (n <= g->partials_cap) return MISOR_OK;
    if (g->partials) (void)hipFree(g->partials);
    g->partials = nullptr;
    g->partials_cap = 0;
    // two slots of n (by pass parity) + the two-level finish's chunk sums
    if (hipMalloc(&g->partials, sizeof(double) * (2 * (size_t)n + kMaxT * kFinishChunks)) !=
        hipSuccess)
        return fail(MISOR_ENOMEM, "partials allocation failed");
    g->partials_cap = n;
    return MISOR_OK;
}

// (re)derive the sweep launch geometry; partials are sized for the largest
int configure_sweep(misor_grid* g, int variant, int rows, int remap) {
    if (variant < 0 || variant >= kNumSweepVariants) return fail(MISOR_EINVAL, "bad variant");
    SweepParams& sp = g->sp;
    const int waves = sweep_waves(variant);
    sp.variant = variant;
    sp.rows_per_block = rows > 0 ? rows : pick_rows_per_block(g->loc.ni, g->loc.nj, waves);
    if (sp.rows_per_block < 1) sp.rows_per_block = 1;
    sp.xcd_remap = remap;
    int nby = 0;
    g->nparts = sweep_partials(g->loc.ni, g->loc.nj, sp.rows_per_block, waves, &g->nbx, &nby);
    g->nby = nby;
    sp.nbx = g->nbx;
    sp.nblocks = g->nparts;
    g->tp.xcd_remap = remap;
    return ensure_partials(g, g->nparts);
}

// the occupancy queries of every built variant and T, made once (the device
// of the first grid: the kernels' occupancy is the architecture's)
const TbResidency& tb_residency() {
    static const TbResidency table = [] {
        TbResidency t{};
        for (int k = 0; k < kBuiltTbVariants; ++k)
            for (int T = 1; T <= kTbVariants[k].max_t; ++T)
                t.n[k][T] = tb_resident(T, kTbVariants[k].id);
        return t;
    }();
    return table;
}

void drop_chain_plans(misor_grid* g) {
    for (auto& v : g->chain_plan)
        for (auto& row : v)
            for (auto& pl : row) {
                (void)hipFree(pl.main.tmpl);
                (void)hipFree(pl.edge.tmpl);
                pl = misor_grid::ChainPlan{};
            }
}

// the segment lists of a chained pass (tb_plan.h chain_lists), built and
// uploaded on first use
int chain_plan(misor_grid* g, int variant, int Tp, int part,
                      const misor_grid::ChainPlan** out) {
    auto& pl = g->chain_plan[variant == kHrTbVariant ? 1 : 0][Tp][part];
    *out = &pl;
    if (pl.built) return MISOR_OK;
    const ChainLists lists = chain_lists(tb_input(g), tb_residency(), g->tp, variant, Tp, part);
    auto upload = [](misor_grid::ChainList& L, const ChainSegs& segs) -> int {
        L.nseg0 = segs.nseg0;
        L.blocks = segs.blocks;
        std::copy(segs.run, segs.run + 9, L.run);
        if (segs.words.empty()) return MISOR_OK;
        const size_t bytes = segs.words.size() * sizeof(unsigned long long);
        if (hipMalloc(&L.tmpl, bytes) != hipSuccess ||
            hipMemcpy(L.tmpl, segs.words.data(), bytes, hipMemcpyHostToDevice) != hipSuccess)
            return fail(MISOR_ENOMEM, "chain plan allocation failed");
        return MISOR_OK;
    };
    if (lists.reserve >= 0) pl.reserve = lists.reserve;
    MISOR_TRY(upload(pl.main, lists.main));
    MISOR_TRY(upload(pl.edge, lists.edge));
    pl.built = true;
    return MISOR_OK;
}

int configure_tb(misor_grid* g, int T, int variant, int rows) {
    if (T < 1 || T > kMaxT) return fail(MISOR_EINVAL, "iterations per pass must be 1..%d", kMaxT);
    if (variant < 0 || variant >= kNumTbVariants) return fail(MISOR_EINVAL, "bad tb variant");
    if (tb_max_t(variant) == 0)  // measured slower, then not built
        return fail(MISOR_EINVAL, "TB variant %d is retired (measured slower; not built)",
                    variant);
    if (variant == kHrTbVariant && !g->tb_persistent)
        return fail(MISOR_EINVAL, "TB variant %d runs persistent chained passes only", variant);
    if (T > tb_max_t(variant))
        return fail(MISOR_EINVAL, "TB variant %d runs at most %d iterations per pass", variant,
                    tb_max_t(variant));
    g->tsteps = T;
    g->tb_rows_req = rows;
    SweepParams& tp = g->tp;
    tp.variant = variant;
    tp.xcd_remap = g->sp.xcd_remap;
    const TbInput in = tb_input(g);
    const TbSizing z = tb_sizing(in, tb_residency(), tp);
    if (z.err[0]) return fail(MISOR_EINVAL, "%s", z.err);
    tb_geometry(in, tb_residency(), std::max(2, z.T), tp);
    g->tb_nparts = tb_parts(tp);
    g->short_all = z.short_all;
    g->short_all_lite = z.short_all_lite;
    g->short_plan = z.short_plan;
    drop_chain_plans(g);  // geometry changed: rebuilt on first use
    if (z.chained) {
        for (int k = 0; k < 2; ++k) {  // the edge kernels' streams
            if (g->xstream[k]) continue;
            int lo = 0, hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
            if (hipStreamCreateWithPriority(&g->xstream[k], hipStreamNonBlocking, hi) !=
                    hipSuccess ||
                hipEventCreateWithFlags(&g->ev_fork[k], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&g->ev_join[k], hipEventDisableTiming) != hipSuccess)
                return fail(MISOR_EHIP, "edge stream creation failed");
        }
        const long long most = z.max_blocks;
        const char* et = getenv("MISOR_CHAIN_TRACE");
        if (et && et[0] == '1' && most > g->chain_trace_blocks) {
            (void)hipDeviceSynchronize();
            (void)hipFree(g->chain_trace);
            g->chain_trace = nullptr;
            g->chain_trace_blocks = 0;
            if (hipMalloc(&g->chain_trace, 3 * most * sizeof(unsigned long long)) != hipSuccess)
                return fail(MISOR_ENOMEM, "chain trace allocation failed");
            g->chain_trace_blocks = most;
        }
        // the work areas (main / edge x parts 0-1 / 2), kept while large enough
        for (int k = 0; k < 4; ++k) {
            if (z.work_bytes <= g->tb_work_bytes[k]) continue;
            if (g->tb_work[k]) {
                (void)hipDeviceSynchronize();
                (void)hipFree(g->tb_work[k]);
            }
            g->tb_work[k] = nullptr;
            g->tb_work_bytes[k] = 0;
            if (hipMalloc(&g->tb_work[k], z.work_bytes) != hipSuccess)
                return fail(MISOR_ENOMEM, "chain work area allocation failed");
            g->tb_work_bytes[k] = z.work_bytes;
        }
    }
    return ensure_partials(g, (int)z.partials);
}
