// misor_solve.hip -- the solve loop of the C ABI: batched passes with a
// device-resident convergence flag, the pipelined decomposed loop (interior
// and halo parts, exchange and all-reduce overlapped), the exact tail near the
// threshold, and the lexicographic solver entry (misor_grid.h).
//
// The red-black solve, top down: misor_solve_rb_n alternates solve_rb_from
// (batched passes) and exact_tail; solve_rb_from takes solve_small where the
// field fits one workgroup, else plans the solve (plan_solve: RbSolve, with
// the PassPlan of pass_plan.h), enqueues batches of passes through one of
// three schedules (enqueue_pipelined, enqueue_overlapped_t1, enqueue_serial)
// and reads the loop state back after each; launch_pass / launch_chained
// launch one pass's kernels.

#include "misor_grid.h"
#include "pass_plan.h"

// ---------------------------------------------------------------------------
// solve loop
// ---------------------------------------------------------------------------

static int ensure_events(misor_grid* g, size_t n) {
    while (g->ev.size() < n) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        g->ev.push_back(e);
    }
    return MISOR_OK;
}

// The device's loop state at the start of a solve or of a stretch of one: `it`
// iterations done with residual `res`, not done, the cap and the near band of
// the loop test (nband < 0: no band).
static int upload_state(misor_grid* g, int it, double res, int itermax, double nband) {
    DevState s{};
    s.it = it;
    s.res = res;
    s.epssq = g->desc.eps * g->desc.eps;
    s.itermax = itermax;
    s.nband = nband;
    *g->st_host = s;
    HIPCHK(hipMemcpyAsync(g->st, g->st_host, sizeof(DevState), hipMemcpyHostToDevice, g->stream));
    return MISOR_OK;
}

static int exact_tail(misor_grid* g, int itermax, int it0, double res0, int* iters, double* res,
                      bool* hand_off);

// The batched passes and the exact tail (below) hand the solve to each other
// (*hand_off) with the iterations done and the last residual; this loop runs
// them in turn, so the hand-overs of a long solve need no stack.
int misor_solve_rb_n(misor_grid* g, int itermax, int* iters, double* res) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    HIPCHK(hipSetDevice(g->device));
    int it = 0;
    double r = 1.0;  // solver.c:196
    for (bool tail = false;; tail = !tail) {
        bool hand_off = false;
        const int rc = tail ? exact_tail(g, itermax, it, r, &it, &r, &hand_off)
                            : solve_rb_from(g, itermax, it, r, &it, &r, &hand_off);
        if (rc) return rc;
        if (!hand_off) break;
    }
    if (iters) *iters = it;
    if (res) *res = r;
    return MISOR_OK;
}

// ---------------------------------------------------------------------------
// The loop test near its threshold (partition independence).
// The residual of a pass is a sum of per-workgroup (and, decomposed, per-rank)
// partials, so its last bits depend on the partition -- as the reference's own
// MPI_Allreduce of per-rank sums (assignment-5/skeleton/src/solver.c:651) does.
// An iteration count can only depend on that when res lies within a few ulps
// of eps^2.  The loop-test kernels therefore stop the solve BEFORE any
// iteration whose res lies within near_rel * eps^2 of eps^2 (DevState::near;
// far outside the rounding spread, so every partition stops at the same
// iteration), the pass is recomputed up to there from its untouched source,
// and exact_tail takes over: one sweep per iteration that stores r^2 of every
// cell, whose sum is formed exactly (fixed-point 128-bit limbs per cell --
// each truncation a function of the cell alone -- added in any order and
// all-reduced exactly, ns_kernels.hip exact_sum), so res and the loop test are
// bit for bit the same on every partition.  Once 2T consecutive iterations
// are outside the band again the batched passes resume.  Only solves that come
// near the threshold pay for it.
// ---------------------------------------------------------------------------
static int exact_residual(misor_grid* g, double cells, double* out) {
    NsLaunch L{};  // the reduction region: interior + physical ghost cells (zero in rsq)
    L.s = g->stream;
    L.pitch = g->pitch;
    L.ni = g->loc.ni;
    L.nj = g->loc.nj;
    L.wall_left = g->loc.neighbours[0] < 0;
    L.wall_right = g->loc.neighbours[1] < 0;
    L.wall_bottom = g->loc.neighbours[2] < 0;
    L.wall_top = g->loc.neighbours[3] < 0;
    const int nb = reduce_blocks(L.ni, L.nj);
    launch_absmax2(L, g->rsq, g->rsq, g->red_partials);
    launch_finish_reduce(g->stream, g->red_partials, nb, kReduceMax, 2, g->red_out);
    HIPCHK(hipGetLastError());
    if (g->dist) MISOR_TRY(allreduce(g, g->red_out, 1, 1));
    HIPCHK(hipMemcpyAsync(g->red_host, g->red_out, sizeof(double), hipMemcpyDeviceToHost,
                          g->stream));
    MISOR_TRY(wait_stream(g, g->stream));
    int E = 0;
    (void)frexp(g->red_host[0], &E);
    launch_exact_sum(L, g->rsq, E, g->red_partials, g->red_out);
    HIPCHK(hipGetLastError());
    if (g->dist) MISOR_TRY(allreduce(g, g->red_out, 3, 0));  // integer limbs < 2^53: exact
    HIPCHK(hipMemcpyAsync(g->red_host, g->red_out, 3 * sizeof(double), hipMemcpyDeviceToHost,
                          g->stream));
    MISOR_TRY(wait_stream(g, g->stream));
    *out = exact_sum_value(g->red_host, E) / cells;  // solver.c:229
    return MISOR_OK;
}

// iterations it0 + 1 .. of solveRB from the current field, one sweep each with
// the exact residual and the loop test on the host (solver.c:197)
static int exact_tail(misor_grid* g, int itermax, int it0, double res0, int* iters, double* res,
                      bool* hand_off) {
    const double epssq = g->desc.eps * g->desc.eps;
    const double cells = (double)g->desc.imax * (double)g->desc.jmax;
    if (!g->rsq) {
        if (hipMalloc(&g->rsq, (size_t)g->elems * sizeof(double)) != hipSuccess) {
            g->rsq = nullptr;
            return fail(MISOR_ENOMEM, "exact residual buffer allocation failed");
        }
        HIPCHK(hipMemsetAsync(g->rsq, 0, (size_t)g->elems * sizeof(double), g->stream));
    }
    // the sweep kernel runs while the device state says not done
    MISOR_TRY(upload_state(g, it0, res0, itermax, -1.0));
    SweepParams sp = g->sp;  // the default sweep variant's geometry
    if (sp.variant != kDefaultSweepVariant) {
        sp.variant = kDefaultSweepVariant;
        sp.rows_per_block = pick_rows_per_block(g->loc.ni, g->loc.nj, sweep_waves(sp.variant));
        int nby = 0, nbx = 0;
        sp.nblocks = sweep_partials(g->loc.ni, g->loc.nj, sp.rows_per_block,
                                    sweep_waves(sp.variant), &nbx, &nby);
        sp.nbx = nbx;
        if (sp.nblocks > g->partials_cap) MISOR_TRY(ensure_partials(g, sp.nblocks));
    }
    sp.part = 0;
    int it = it0, far = 0;
    double r = res0;
    const int T = effective_tsteps(tb_input(g), g->tp.variant);
    while ((r >= epssq) && (it < itermax)) {
        double* src = pbuf(g, g->cur);
        double* dst = pbuf(g, g->cur + 1);
        if (g->dist) MISOR_TRY(exchange(g, src, 2));  // the sweep reads the 2-deep halo
        launch_sweep_rsq(g->stream, sp, src, dst, g->fld[kRhs], g->partials, g->st, g->rsq);
        HIPCHK(hipGetLastError());
        g->cur = (g->cur + 1) % g->np;
        MISOR_TRY(exact_residual(g, cells, &r));
        ++it;
        g->stats.launches += 1;
        // back to the batched passes after 2T iterations outside the band
        far = fabs(r - epssq) > g->near_rel * epssq ? far + 1 : 0;
        if (far >= 2 * T && (r >= epssq) && (it < itermax)) {
            *hand_off = true;  // back to solve_rb_from (misor_solve_rb_n)
            break;
        }
    }
    g->p_stale = g->dist;  // (p_halo)
    MISOR_TRY(wait_stream(g, g->stream));
    g->stats.sweeps += it - it0;
    g->last_iters = it;
    *iters = it;
    *res = r;
    return MISOR_OK;
}

// ---------------------------------------------------------------------------
// The whole solve in one workgroup (p in LDS; one rank, small_solve_fits).
// The caller has uploaded the loop state.  Stopped before an iteration near
// the threshold, the kernel has left p untouched: it runs again up to that
// iteration and the exact tail goes on from there (*hand_off).
// ---------------------------------------------------------------------------
static int solve_small(misor_grid* g, int it0, double res0, double cells, int* iters, double* res,
                       bool* hand_off) {
    double* p = pbuf(g, g->cur);
    if (g->timing) {
        MISOR_TRY(ensure_events(g, 2));
        HIPCHK(hipEventRecord(g->ev[0], g->stream));
    }
    launch_solve_small(g->stream, p, g->fld[kRhs], g->loc.ni, g->loc.nj, g->pitch, g->sp.idx2,
                       g->sp.idy2, g->sp.coef, cells, g->st);
    HIPCHK(hipGetLastError());
    if (g->timing) HIPCHK(hipEventRecord(g->ev[1], g->stream));
    HIPCHK(hipMemcpyAsync(g->st_host, g->st, sizeof(DevState), hipMemcpyDeviceToHost, g->stream));
    MISOR_TRY(wait_stream(g, g->stream));
    const int it = g->st_host->it;
    if (g->timing) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, g->ev[0], g->ev[1]));
        g->stats.sweep_ms += ms;
        g->stats.timed_sweeps += it - it0;
    }
    g->stats.launches += 1;
    g->stats.sweeps += it - it0;
    *iters = it;
    *res = g->st_host->res;
    if (g->st_host->near) {
        // again from the same state, capped at the iteration before the near
        // one and without a band
        MISOR_TRY(upload_state(g, it0, res0, it, -1.0));
        launch_solve_small(g->stream, p, g->fld[kRhs], g->loc.ni, g->loc.nj, g->pitch, g->sp.idx2,
                           g->sp.idy2, g->sp.coef, cells, g->st);
        HIPCHK(hipGetLastError());
        // the exact tail writes its own loop state into the pinned st_host at
        // once: this run's copy of it must have left first (a grid's second
        // near-threshold solve, rsq already allocated, got there before it)
        MISOR_TRY(wait_stream(g, g->stream));
        *hand_off = true;  // the exact tail from iteration it (misor_solve_rb_n)
        return MISOR_OK;
    }
    g->last_iters = it;
    return MISOR_OK;
}

// ---------------------------------------------------------------------------
// The multi-block path: passes of T iterations (T = 1: single-iteration sweep
// kernel; T >= 2: temporally blocked kernel, sor_tb.hip).
// ---------------------------------------------------------------------------

// The short plan: a pass costs about the same for any T <= 8 (it streams
// its fields; profiles/r04_tcurve.txt), so a solve capped at few iterations
// is cheapest in as few passes as possible.  The split-ring kernel runs
// kShortT = 10 iterations a pass at ~1.4 x the time of a T = 8 pass: where its
// passes times 1.4 undercut the default's pass count the solve takes it
// (pass_plan.h short_plan_saves_passes).  With the chained split ring
// (round 5) a T = 10 pass costs about a T = 8 one on the blocks where
// configure_tb sets short_all, so there every solve of more than 8 iterations
// takes it.
static bool short_plan_on(const misor_grid* g, int todo) {
    const bool all = g->short_all || (g->short_all_lite && g->res_lite);
    // (decomposed: only where the smallest block holds the split ring's halo)
    const bool short_fits = !g->dist || tb_halo_depth(kShortT, kShortTbVariant) <= g->max_depth;
    return g->short_plan && short_fits &&
           effective_tsteps(tb_input(g), g->tp.variant) == kDefaultTsteps &&
           (all ? todo > kDefaultTsteps : short_plan_saves_passes(todo, kShortT, kDefaultTsteps));
}

// What the passes of one solve_rb_from call share.  Pass k (0 .. max_passes-1)
// reads src(k) and writes dst(k) = src(k + 1), round the pressure buffers from
// the one current at the start.
struct RbSolve {
    misor_grid* g;
    int T;            // iterations of a full pass (the plan's passes run T or fewer)
    SweepParams tpl;  // geometry of a T-iteration pass (T >= 2)
    int depth;        // halo of src a pass reads
    int nparts;       // block partials a T-iteration pass writes
    bool lite_on;     // residual lower bounds allowed (below)
    double cells;
    int cur0;         // g->cur at the start
    PassPlan plan;

    // Residual lower bounds (MISOR_TUNE_RES_LITE), one rank or decomposed: a
    // kShortT-iteration split-ring pass counts r^2 of its iterations but the
    // last on one row in S of its steady chunks (sor_tbh.h hrs_step LITE), one
    // FP64 FMA per update fewer on a VALU-bound pass.  Each such sum is a lower
    // bound of the iteration's residual; the loop test (rb_partsum_kernel) takes
    // it only where it proves the loop goes on -- >= eps^2, outside the near
    // band, before itermax -- and otherwise stops the pass before that
    // iteration (DevState::lite_miss): the pass is redone from its source up to
    // there and the rest of the solve counts every cell.  The pass's last
    // iteration is always counted in full, so res after every pass is exact.
    // (one rank: the loop test in the last workgroup of the partial sums;
    // decomposed: the decide kernel after the all-reduce -- the sum of the
    // ranks' lower bounds is one)
    bool lite_pass(int Tp, int force) const {
        return lite_on && force == 0 && Tp == kShortT && tpl.variant == kHrTbVariant;
    }
    // the iterations of a Tp-iteration pass whose sums are lower bounds (bit i: iteration i)
    int lite_mask(int Tp) const { return lite_pass(Tp, 0) ? (1 << (Tp - 1)) - 1 : 0; }
    // block partials of a Tk-iteration pass (a narrower cone: wider strips)
    int nparts_of(int Tk) const {
        if (T == 1 || Tk == T) return nparts;
        SweepParams tp = tpl;
        tb_geometry(tb_input(g), tb_residency(), Tk, tp);
        return tb_parts(tp);
    }
    const double* src(long long k) const { return pbuf(g, cur0 + k); }
    double* dst(long long k) const { return pbuf(g, cur0 + k + 1); }
    // pass k's block partials in the pipelined schedule, where the sums of pass
    // k - 1 are still being reduced: by pass parity (the others use slot 0)
    double* partials(long long k) const {
        return g->partials + (k & 1) * (long long)g->partials_cap;
    }
};

static RbSolve plan_solve(misor_grid* g, int todo, double cells) {
    const bool shortp = short_plan_on(g, todo);
    const int T = shortp ? kShortT : effective_tsteps(tb_input(g), g->tp.variant);
    SweepParams tpl = g->tp;  // the plan's geometry
    if (shortp) {
        tpl.variant = kShortTbVariant;
        tb_geometry(tb_input(g), tb_residency(), T, tpl);
    }
    // halo of src each pass needs: 2T, one row more for the skewed split ring
    // (tb_halo_depth).  effective_tsteps and short_plan_on keep it within the
    // halo plans: with a 2T-deep halo the split ring's leading stages would
    // count a stale row into their residuals (solve_rb_from checks)
    const int depth = tb_halo_depth(T, tpl.variant);
    const bool lite_on = g->res_lite && !g->lite_block && T > 1 && (g->dist || g->finish2);
    const int nparts = T == 1 ? g->nparts : tb_parts(tpl);
    return RbSolve{g, T, tpl, depth, nparts, lite_on, cells, g->cur, PassPlan(todo, T)};
}

static void use_chain_list(SweepParams& q, const misor_grid::ChainList& L) {
    q.seg_tmpl = L.tmpl;
    q.nseg0 = L.nseg0;
    q.chain_blocks = L.blocks;
    for (int x = 0; x < 9; ++x) q.seg_run[x] = L.run[x];
}

// One part of a chained pass (tp.chain: chained runs with work stealing): the
// main kernel and the edge kernel (the strips at a physical left / right
// side), each with its segment list, concurrently.  The edge kernel goes to
// stream s, the main kernel to xstream[k] (k = 1 for part 2, else 0) between
// ev_fork[k] (recorded on s) and ev_join[k] (waited on by s), so that s
// continues after both; parts 0 / 1 and part 2 use separate work areas and
// may run concurrently.
static int launch_chained(const RbSolve& c, hipStream_t s, int part, SweepParams tp,
                          const double* src, double* dst, int Tp, int force, double* partials) {
    misor_grid* g = c.g;
    double* const rhs = g->fld[kRhs];
    const misor_grid::ChainPlan* pl = nullptr;
    MISOR_TRY(chain_plan(g, tp.variant, Tp, part, &pl));
    const int k = part == 2 ? 1 : 0;
    tp.seg_cap = kChainSegCap;
    tp.trace = part == 2 ? nullptr : g->chain_trace;
    if (tp.trace) g->chain_trace_last = tp.nblocks;
    const int eg = pl->edge.nseg0;  // edge workgroups: one per initial segment
    // Where the two kernels run: the main kernel forked to xstream,
    // the edge kernel on s.  The other way round (the edge kernel on
    // xstream, launched first or after the main one) its 16-odd
    // workgroups did not start until the main kernel's workgroups
    // retired, in every pass of a multi-pass solve but the first,
    // though its slots were free (profiles/r03_chain_xmode.txt: 8.5-8.9
    // ms per 32768^2 pass against 6.0).
    SweepParams te = tp;
    use_chain_list(te, pl->edge);
    te.chain_edge = 1;
    te.reserve = std::max(0, tb_residency()(Tp, tp.variant) - eg);
    SweepParams tm = tp;
    use_chain_list(tm, pl->main);
    tm.chain_edge = 0;
    if (part == 1 && pl->reserve >= 0) tm.reserve = pl->reserve;
    tm.reserve += pl->edge.blocks > 0 ? eg : 0;
    const bool has_e = pl->edge.blocks > 0, has_m = pl->main.blocks > 0;
    // (no edge list: the main kernel alone, on s)
    const bool both = has_e && has_m;
    // MISOR_TUNE_EDGE_STEAL (whole split-ring passes): 0 = the edge
    // kernel never takes from the main list; 2 (diagnostics) = the
    // main kernel in stream order behind the edge kernel, whose
    // workgroups, their list done, find every main segment whole
    // and split each down to fewer than 4 unclaimed blocks.  The
    // edge kernel never waits for the main one (chain_acquire's
    // steal loop ends when no segment has 4 unclaimed blocks; the
    // main kernel's tickets are not its to take), so it ends
    // whether or not the main kernel has started.
    const int steal = !(both && part == 0) ? 0 : tp.variant == kHrTbVariant ? g->edge_steal : 1;
    const bool fork = both && steal != 2;
    hipStream_t ms = fork ? g->xstream[k] : s;
    if (both) {
        // A whole pass: the edge kernel's workgroups go on to steal
        // from the main list once the edge list is done (its 2.5x
        // block cost is an estimate: its kernel ended ~2.5 ms before
        // the main one in a 6.6 ms 32768^2 pass, its slots idle), so
        // the main list's work area is initialised here, before
        // either kernel starts.  Not in a pipelined pass's parts:
        // there the edge slots, once free, are part 2's
        // (profiles/r06_edge_steal_ab.txt: the 8-GPU rank's loop 3%
        // slower with them stealing)
        if (steal) {
            launch_chain_init(s, g->tb_work[k], pl->main.tmpl, pl->main.nseg0, tm.seg_cap);
            tm.no_init = 1;
            te.alt_work = g->tb_work[k];
            te.alt_nseg0 = pl->main.nseg0;
        }
        if (fork) {
            HIPCHK(hipEventRecord(g->ev_fork[k], s));
            HIPCHK(hipStreamWaitEvent(g->xstream[k], g->ev_fork[k], 0));
        }
    }
    if (has_e) launch_tb(s, Tp, te, src, dst, rhs, partials, g->st, force, g->tb_work[2 + k]);
    if (has_m) launch_tb(ms, Tp, tm, src, dst, rhs, partials, g->st, force, g->tb_work[k]);
    if (fork) {
        HIPCHK(hipEventRecord(g->ev_join[k], g->xstream[k]));
        HIPCHK(hipStreamWaitEvent(s, g->ev_join[k], 0));
    }
    return MISOR_OK;
}

// One pass, or one part of one (0: all blocks, 1: interior blocks, 2: edge
// blocks), of Tp <= T iterations from src to dst on stream s, its block
// partials to `partials`.  force: run whatever the device's loop state says
// (the redo of an overshooting pass).
static int launch_pass(const RbSolve& c, hipStream_t s, int part, const double* src, double* dst,
                       int Tp, int force, double* partials) {
    misor_grid* g = c.g;
    double* const rhs = g->fld[kRhs];
    if (c.T == 1) {
        SweepParams sp = g->sp;
        sp.part = part;
        launch_sweep(s, sp, src, dst, rhs, partials, g->st);
        return MISOR_OK;
    }
    SweepParams tp = c.tpl;
    tp.part = part;
    // the interior blocks of an overlapped pass leave workgroup slots to the
    // halo exchange, the residual all-reduce + loop test and the edge blocks
    // on the other streams: a persistent launch holds every slot it gets
    // until the pass is over, so without them the exchange would only start
    // at the end of the interior blocks
    tp.reserve = part == 1 ? g->tb_reserve : 0;
    if (Tp != c.T) tb_geometry(tb_input(g), tb_residency(), Tp, tp);  // narrower cone: wider strips
    tp.lite = c.lite_pass(Tp, force) ? 1 : 0;
    if (tp.chain) return launch_chained(c, s, part, tp, src, dst, Tp, force, partials);
    // persistent work-queue launch on the grid stream (whole passes and
    // interior blocks); the boundary blocks of a split pass are few
    int* q = (g->tb_persistent && part != 2 && s == g->stream) ? g->tb_queue : nullptr;
    launch_tb(s, Tp, tp, src, dst, rhs, partials, g->st, force, q);
    return MISOR_OK;
}

// ---------------------------------------------------------------------------
// The three schedules.  Each enqueues passes launched .. launched + batch - 1
// and leaves the main stream waiting for the last one's loop test, so that the
// caller's read-back of the loop state follows it.  With timing on, pass k's
// sweep lies between ev[2b] and ev[2b + 1] on the main stream (b = k -
// launched).
// ---------------------------------------------------------------------------

// Pipelined decomposed passes (T >= 2, overlap on; three pressure buffers):
// pass k reads src_k = pbuf(k), writes pbuf(k+1), which is the source of
// pass k-2 -- so pass k waits for the loop test of pass k-2 only (a pass that
// overshoots convergence is recomputed from its source), and the all-reduce
// + loop test of pass k-1 run while pass k sweeps.  Within a pass the
// interior blocks (part 1, main stream) and the edge blocks (part 2, on
// cstream: those whose cone reads src's halo; they alone write dst's send
// region) run concurrently; the exchange of dst's halo for pass k+1 follows
// the edge blocks on cstream, and so overlaps the interior blocks.
//
// Streams and events (by pass parity k & 1):
//   main     [wait ev_dk: decide k-2] part 1 of k, record ev_i
//            [wait ev_e2: part 2 of k]; after the batch's last pass [wait ev_dk]
//   cstream  (k = 0: [wait ev_s: state upload, rhs halo, prior work],
//            exchange of src) (first pass of a batch: part 2 of k, record
//            ev_e2) exchange of dst, [wait ev_i] partial sums, all-reduce,
//            decide, record ev_dk, (not the batch's last: part 2 of k+1,
//            record ev_e2)
static int enqueue_pipelined(const RbSolve& c, long long launched, int batch) {
    misor_grid* g = c.g;
    const long long max_passes = c.plan.max_passes;
    if (launched == 0) {
        HIPCHK(hipEventRecord(g->ev_s, g->stream));  // state upload, rhs halo, prior work
        HIPCHK(hipStreamWaitEvent(g->cstream, g->ev_s, 0));
    }
    for (int b = 0; b < batch; ++b) {
        const long long k = launched + b;
        const int Tk = c.plan.iters_of(k);
        const double* src = c.src(k);
        double* dst = c.dst(k);
        double* part = c.partials(k);
        // interior blocks: after pass k-1 (this stream, plus the edge blocks:
        // waited on at the end of the previous iteration) and decide k-2
        if (k >= 2) HIPCHK(hipStreamWaitEvent(g->stream, g->ev_dk[k & 1], 0));
        if (g->timing) HIPCHK(hipEventRecord(g->ev[2 * b], g->stream));
        MISOR_TRY(launch_pass(c, g->stream, 1, src, dst, Tk, 0, part));
        HIPCHK(hipEventRecord(g->ev_i[k & 1], g->stream));
        // Part 2 (the blocks whose cone reads the halo) on the comm stream,
        // right behind what it waits for: pass k+1's part 2 is enqueued here,
        // after pass k's exchange, loop test and part 1 (its source is pass
        // k's result), so no cross-stream wait stands between the exchange
        // and it.  (On a stream of its own, waiting for the exchange on the
        // comm stream and the interior blocks on this one, the second pass's
        // part 2 started ~0.5 ms late on the 8-GPU rank block:
        // profiles/r05_decomposed_loop_trace*.)  The first pass of a batch
        // enqueues its own part 2: the previous batch's last pass leaves it
        // out, so nothing of a batch is still queued on the comm stream
        // behind the decide the host reads -- a solve that stops there (or a
        // near-threshold hand-off to exact_tail, whose state upload would
        // re-arm the device flag) leaves no pending launch that could still
        // write a pressure buffer.
        //
        // The solve's first pass: src's halo, then its part 2.  (The exchange
        // follows the pass's interior launch on the host: RCCL's host side of
        // a grouped send / receive takes ~0.1 ms, which the interior blocks
        // need not wait for -- profiles/r05_decomposed_loop_trace.csv)
        if (k == 0) MISOR_TRY(exchange(g, const_cast<double*>(src), c.depth, g->cstream));
        if (b == 0) {
            MISOR_TRY(launch_pass(c, g->cstream, 2, src, dst, Tk, 0, part));
            HIPCHK(hipEventRecord(g->ev_e2[k & 1], g->cstream));
        }
        // dst's halo (part 2 of pass k, above, wrote its send region)
        if (k + 1 < max_passes) MISOR_TRY(exchange(g, dst, c.depth, g->cstream));
        HIPCHK(hipStreamWaitEvent(g->cstream, g->ev_i[k & 1], 0));
        // the pass's residual sums for the all-reduce: the two-level sum (many
        // workgroups, the last one writing st->sum) -- one workgroup summing
        // every block partial took 70-100 us, after the last pass on the
        // solve's critical path (profiles/r05_decomposed_loop_trace.csv)
        launch_finish2(g->cstream, part, c.nparts_of(Tk), Tk, g->st, c.cells,
                       g->partials + 2 * (long long)g->partials_cap, g->tb_queue + 10, 0);
        MISOR_TRY(allreduce(g, g->st->sum, Tk, 0, g->cstream));
        launch_decide(g->cstream, g->st, Tk, c.cells, c.lite_mask(Tk));
        HIPCHK(hipEventRecord(g->ev_dk[k & 1], g->cstream));
        if (k + 1 < max_passes && b + 1 < batch) {  // pass k+1's part 2: after both parts of pass k
            const long long k1 = k + 1;
            MISOR_TRY(launch_pass(c, g->cstream, 2, dst, c.dst(k1), c.plan.iters_of(k1), 0,
                                  c.partials(k1)));
            HIPCHK(hipEventRecord(g->ev_e2[k1 & 1], g->cstream));
        }
        // pass k+1's interior blocks read what part 2 of pass k wrote
        HIPCHK(hipStreamWaitEvent(g->stream, g->ev_e2[k & 1], 0));
        if (g->timing) HIPCHK(hipEventRecord(g->ev[2 * b + 1], g->stream));
        if (b == batch - 1)  // the host reads the loop state after the last decide
            HIPCHK(hipStreamWaitEvent(g->stream, g->ev_dk[k & 1], 0));
    }
    return MISOR_OK;
}

// Overlapped decomposed passes of one iteration (T = 1, overlap on; T >= 2
// takes the pipelined schedule).  Pass k:
//   cstream  [wait ev_s: pass k-1 on the main stream] all-reduce and decide of
//            k-1 (the first pass of a batch has none: the previous batch closed
//            its own), exchange of src_k, record ev_x
//   main     record ev_s; interior blocks of pass k (no halo reads) meanwhile,
//            [wait ev_x] boundary blocks, partial sums; the batch's last pass
//            closes the batch: record ev_s, and on cstream [wait ev_s]
//            all-reduce + decide, record ev_x, which the main stream waits for
// An interior pass launched after convergence (decide k-1 still in flight)
// only writes a buffer that is not the result.
static int enqueue_overlapped_t1(const RbSolve& c, long long launched, int batch) {
    misor_grid* g = c.g;
    for (int b = 0; b < batch; ++b) {
        const long long k = launched + b;
        const int Tk = c.plan.iters_of(k);
        const double* src = c.src(k);
        double* dst = c.dst(k);
        HIPCHK(hipEventRecord(g->ev_s, g->stream));
        HIPCHK(hipStreamWaitEvent(g->cstream, g->ev_s, 0));
        if (b > 0) {  // pass k-1 of this batch
            MISOR_TRY(allreduce(g, g->st->sum, c.plan.iters_of(k - 1), 0, g->cstream));
            launch_decide(g->cstream, g->st, c.plan.iters_of(k - 1), c.cells);
        }
        MISOR_TRY(exchange(g, const_cast<double*>(src), c.depth, g->cstream));
        HIPCHK(hipEventRecord(g->ev_x, g->cstream));
        if (g->timing) HIPCHK(hipEventRecord(g->ev[2 * b], g->stream));
        MISOR_TRY(launch_pass(c, g->stream, 1, src, dst, Tk, 0, g->partials));
        HIPCHK(hipStreamWaitEvent(g->stream, g->ev_x, 0));
        MISOR_TRY(launch_pass(c, g->stream, 2, src, dst, Tk, 0, g->partials));
        if (g->timing) HIPCHK(hipEventRecord(g->ev[2 * b + 1], g->stream));
        launch_finish(g->stream, g->partials, c.nparts_of(Tk), Tk, g->st, c.cells, 0);
        if (b == batch - 1) {  // close the batch: all-reduce + decide of the last one
            HIPCHK(hipEventRecord(g->ev_s, g->stream));
            HIPCHK(hipStreamWaitEvent(g->cstream, g->ev_s, 0));
            MISOR_TRY(allreduce(g, g->st->sum, Tk, 0, g->cstream));
            launch_decide(g->cstream, g->st, Tk, c.cells);
            HIPCHK(hipEventRecord(g->ev_x, g->cstream));
            HIPCHK(hipStreamWaitEvent(g->stream, g->ev_x, 0));
        }
    }
    return MISOR_OK;
}

// One rank, or decomposed without overlap: everything on the main stream in
// order, no events.  Pass k: (decomposed: exchange of src_k's halo) the whole
// pass, the partial sums, then the loop test -- decomposed after the
// all-reduce (decide), one rank in the sum's last workgroup (finish2) or in
// the one summing kernel.
static int enqueue_serial(const RbSolve& c, long long launched, int batch) {
    misor_grid* g = c.g;
    for (int b = 0; b < batch; ++b) {
        const long long k = launched + b;
        const int Tk = c.plan.iters_of(k);
        const double* src = c.src(k);
        // 2T-deep halo of src: one exchange per pass
        if (g->dist) MISOR_TRY(exchange(g, const_cast<double*>(src), c.depth));
        if (g->timing) HIPCHK(hipEventRecord(g->ev[2 * b], g->stream));
        MISOR_TRY(launch_pass(c, g->stream, 0, src, c.dst(k), Tk, 0, g->partials));
        if (g->timing) HIPCHK(hipEventRecord(g->ev[2 * b + 1], g->stream));
        if (g->dist) {
            launch_finish(g->stream, g->partials, c.nparts_of(Tk), Tk, g->st, c.cells, 0);
            MISOR_TRY(allreduce(g, g->st->sum, Tk, 0));
            launch_decide(g->stream, g->st, Tk, c.cells, c.lite_mask(Tk));
        } else if (g->finish2) {  // the loop test in the last workgroup (tb_queue[9])
            launch_finish2(g->stream, g->partials, c.nparts_of(Tk), Tk, g->st, c.cells,
                           g->partials + 2 * (long long)g->partials_cap, g->tb_queue + 9, 1,
                           c.lite_mask(Tk));
        } else {
            launch_finish(g->stream, g->partials, c.nparts_of(Tk), Tk, g->st, c.cells, 1);
        }
    }
    return MISOR_OK;
}

// sweep time of the batch that ended at pass `launched`, the loop state read
// back: passes after convergence exit at once; count only the real ones
static int attribute_sweep_times(const RbSolve& c, long long launched, int batch, int it0) {
    misor_grid* g = c.g;
    const long long real_before = launched - batch;
    const long long real_end = c.plan.passes_for(g->st_host->it - it0);
    for (int b = 0; b < batch; ++b) {
        if (real_before + b >= real_end) break;
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, g->ev[2 * b], g->ev[2 * b + 1]));
        g->stats.sweep_ms += ms;
        g->stats.timed_sweeps += c.plan.iters_of(real_before + b);
        g->stats.timed_passes++;
    }
    return MISOR_OK;
}

// Iterations it0 + 1 .. of solveRB from the current field in batched passes,
// until the loop test (on the device) ends the solve or hands it on.
int solve_rb_from(misor_grid* g, int itermax, int it0, double res0, int* iters, double* res,
                  bool* hand_off) {
    const double epssq = g->desc.eps * g->desc.eps;
    if (!((res0 >= epssq) && (it0 < itermax))) {  // loop test of solver.c:197
        *iters = it0;
        *res = res0;
        return MISOR_OK;
    }
    MISOR_TRY(upload_state(g, it0, res0, itermax, near_band_abs(g->near_rel, epssq)));
    const double cells = (double)g->desc.imax * (double)g->desc.jmax;
    if (!g->dist && g->small_solve && small_solve_fits(g->loc.ni, g->loc.nj))
        return solve_small(g, it0, res0, cells, iters, res, hand_off);
    // the passes plan the iterations still to do (it0 of them are done: a solve
    // resumed after an exact tail)
    const RbSolve c = plan_solve(g, itermax - it0, cells);
    const PassPlan& plan = c.plan;
    const int T = c.T;
    if (g->dist && c.depth > g->max_depth)
        return fail(MISOR_ESTATE, "halo depth %d of a %d-iteration pass exceeds %d", c.depth, T,
                    g->max_depth);
    // time the communication steps of the loop (collected after each batch)
    g->comm_timing = g->timing && g->dist;
    g->cev_used[0] = g->cev_used[1] = 0;
    const int rhs_depth = T == 1 ? 1 : c.depth;
    if (g->dist && g->rhs_halo < rhs_depth) {  // the halo-ring updates read rhs outside the block
        MISOR_TRY(exchange(g, g->fld[kRhs], rhs_depth));
        g->rhs_halo = rhs_depth;
    }
    // the schedule of every batch of this solve
    int (*const enqueue)(const RbSolve&, long long, int) = !(g->dist && g->overlap) ? enqueue_serial
                                                           : T > 1 ? enqueue_pipelined
                                                                   : enqueue_overlapped_t1;
    // passes enqueued before the host reads the loop state: as many as the last
    // solve took (rounded up: a solve capped at itermax = 100 with T = 8 --
    // NS config 5 -- enqueues its 13 passes at once), at least 8
    const int last_passes = (g->last_iters + T - 1) / T;
    int batch = last_passes > 8 ? last_passes : 8;
    long long launched = 0;  // passes enqueued
    for (;;) {
        if (batch > plan.max_passes - launched) batch = (int)(plan.max_passes - launched);
        if (batch < 1) batch = 1;
        if (g->timing) MISOR_TRY(ensure_events(g, 2 * (size_t)batch));
        MISOR_TRY(enqueue(c, launched, batch));
        HIPCHK(hipGetLastError());
        launched += batch;
        g->stats.launches += batch;
        HIPCHK(hipMemcpyAsync(g->st_host, g->st, sizeof(DevState), hipMemcpyDeviceToHost,
                              g->stream));
        MISOR_TRY(wait_stream(g, g->stream));
        if (g->comm_timing) MISOR_TRY(collect_comm_times(g));
        if (g->timing) MISOR_TRY(attribute_sweep_times(c, launched, batch, it0));
        if (g->st_host->done) break;
        if (launched >= plan.max_passes) break;  // cannot happen: done covers it
        batch = batch < 512 ? 2 * batch : 1024;
    }
    const int it = g->st_host->it;
    const long long passes = plan.passes_for(it - it0);
    const int over = (int)(plan.covered(passes) - (it - it0));
    g->cur = (int)((c.cur0 + passes) % g->np);
    if (over > 0) {
        // the last pass ran past the iteration that ended the loop: redo it
        // with T - over iterations from its source (untouched since)
        MISOR_TRY(launch_pass(c, g->stream, 0, c.src(passes - 1), pbuf(g, g->cur),
                              plan.iters_of(passes - 1) - over, 1, g->partials));
        HIPCHK(hipGetLastError());
    }
    g->comm_timing = false;
    g->p_stale = g->dist;  // the final field's halo: exchanged by its next reader (p_halo)
    MISOR_TRY(wait_stream(g, g->stream));
    g->last_iters = it;
    g->stats.sweeps += it - it0;
    g->stats.iters_per_pass = T;
    g->stats.tb_variant = T == 1 ? -1 : c.tpl.variant;
    g->stats.chained = T > 1 && c.tpl.chain ? 1 : 0;
    if (g->st_host->lite_miss) {
        // a residual lower bound proved nothing: the field is the state after
        // `it` iterations (the pass redone above), the rest counts every cell
        g->stats.lite_misses++;
        g->lite_block = true;
        const int rc = solve_rb_from(g, itermax, it, g->st_host->res, iters, res, hand_off);
        g->lite_block = false;
        return rc;
    }
    // stopped before an iteration near the threshold: the exact tail goes on
    // from it (misor_solve_rb_n)
    if (g->st_host->near) *hand_off = true;
    *iters = it;
    *res = g->st_host->res;
    return MISOR_OK;
}

// would the next misor_solve_lex of this grid run the tiled wavefront
// (MISOR_TUNE_LEX_TILED; automatic: p does not fit the one workgroup's LDS and
// the grid has at least kLexTiledCells cells, the smallest size at which the
// tiled kernel measured faster)
bool lex_tiled_on(const misor_grid* g) {
    if (g->lex_tiled >= 0) return g->lex_tiled == 1;
    return lex_use_lds(g->loc.ni, g->loc.nj) == 0 &&
           (long long)g->loc.ni * g->loc.nj >= kLexTiledCells;
}

int misor_solve_lex(misor_grid* g, int xorder, int* iters, double* res) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    if (g->desc.nranks != 1)
        return fail(MISOR_ESTATE, "lexicographic SOR has no decomposed form (use red-black)");
    if (g->desc.variant != MISOR_SOLVE_RB)
        return fail(MISOR_ESTATE, "lexicographic SOR uses the solveRB factor (variant RB)");
    HIPCHK(hipSetDevice(g->device));
    MISOR_TRY(upload_state(g, 0, 1.0, g->desc.itermax, -1.0));
    const double cells = (double)g->desc.imax * (double)g->desc.jmax;
    const bool tiled = lex_tiled_on(g);
    if (tiled) {
        HIPCHK(launch_solve_lex_tiled(g->stream, pbuf(g, g->cur), g->fld[kRhs], g->loc.ni,
                                      g->loc.nj, g->pitch, g->sp.idx2, g->sp.idy2, g->sp.coef,
                                      cells, xorder != 0, g->st, g->lex_tw ? g->lex_tw : kLexTileW,
                                      g->lex_th ? g->lex_th : kLexTileH, g->lex_wgs,
                                      g->lex_work));
    } else {
        launch_solve_lex(g->stream, pbuf(g, g->cur), g->fld[kRhs], g->loc.ni, g->loc.nj,
                         g->pitch, g->sp.idx2, g->sp.idy2, g->sp.coef, cells, xorder != 0, g->st);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(g->st_host, g->st, sizeof(DevState), hipMemcpyDeviceToHost,
                          g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    if (tiled && g->st_host->done != 1)  // a bounded wait of the wavefront gave up
        return fail(MISOR_EHIP,
                    "lexicographic wavefront stalled (a tile's wait ran into its limit); "
                    "p is undefined");
    const int it = g->st_host->it;
    g->last_iters = it;
    g->stats.sweeps += it;
    if (iters) *iters = it;
    if (res) *res = g->st_host->res;
    return MISOR_OK;
}

int misor_solve_rb(misor_grid* g, int* iters, double* res) {
    if (!g) return fail(MISOR_EINVAL, "null grid");
    return misor_solve_rb_n(g, g->desc.itermax, iters, res);
}
