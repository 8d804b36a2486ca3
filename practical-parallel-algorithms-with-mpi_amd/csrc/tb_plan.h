// tb_plan.h -- the launch plans of the sweeps and of the temporally blocked
// passes: what the plans are made of (the variants, the tuning constants,
// struct SweepParams), the block geometry of a pass (tb_geometry), the sizing
// of its buffers (tb_sizing) and the segment lists of chained passes
// (chain_lists).  Plain C++ with no device or communication headers and no
// misor_grid, so that host/tb_plan_check.cc checks it on the CPU: what is read
// off the grid comes in a TbInput, the occupancy queries in a TbResidency.
// misor_plan.hip stores the results and uploads the lists.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

// functions that device code calls too
#ifdef __HIPCC__
#define MISOR_HD __host__ __device__
#else
#define MISOR_HD
#endif

namespace misor {

constexpr int kMaxT = 10;                // iterations per temporally blocked pass (max)
constexpr int kLanes = 64;                 // wavefront
constexpr int kStripCells = 2 * kLanes;    // 128 columns per wave (2 per lane)

// temporally blocked sweep (sor_tb.hip): the built variants by their public
// number (id): strips per workgroup, rows in flight
// (x-neighbour shifts through ds_bpermute instead of DPP measured 5% slower:
// profiles/r02_tune_bperm.txt)
// 128-column strips (2 columns per lane), 2 waves per SIMD.
// skew: the split-ring march in two independent stage chains per step (sor_tbh.h
// hrs_step); hr: the split rhs ring, registers + LDS (sor_tbh.h)
// The other numbers below kNumTbVariants are retired -- measured slower and no
// longer built (DESIGN.md section 4:
// 1 / 3 eight / one strips per workgroup, 4 three rows in flight, 5 four
// columns per lane at one wave per SIMD, 6-8 strips exchanging edge columns
// through LDS, 9 the skewed register-ring march, 10/11 an LDS row queue, 12 the
// unskewed split ring); configuring one fails (tb_max_t = 0).  The register-ring
// kernels run T <= kMaxT2 (above that their rhs ring spills); the split ring
// (13) runs T up to kMaxT.
constexpr int kMaxT2 = 8;
struct TbVariant {
    int id, waves, ahead, max_t, skew, hr;
};
constexpr TbVariant kTbVariants[] = {
    {0, 4, 2, kMaxT2, 0, 0}, {2, 2, 2, kMaxT2, 0, 0}, {13, 4, 2, kMaxT, 1, 1}};
constexpr int kNumTbVariants = 14;
constexpr int kHrTbVariant = 13;   // the skewed split ring (T = 1 unskewed)
// the short plan of capped solves (misor_solve.hip short_plan_on, pass_plan.h)
constexpr int kShortTbVariant = kHrTbVariant;
constexpr int kShortT = 10;
constexpr long long kShortDistCells = 1LL << 28;  // decomposed: local blocks at least this big
constexpr long long kHrAllCells = 1LL << 26;      // chained blocks from here: every solve > 8
// iterations per pass: 8 on large local blocks, 7 below kTsteps8Cells cells
// (32768^2 0.744 vs 0.785 ms/iteration, profiles/r02_tune_t789.txt; one rank's
// 8192 x 16384 block at 8 GPUs 0.118-0.122 at T = 7 vs 0.125 at T = 8,
// profiles/r02_small_rows.txt, r02_tb_rows_t8.txt)
constexpr int kDefaultTsteps = 8;
constexpr int kSmallBlockTsteps = 7;
constexpr long long kTsteps8Cells = 1LL << 28;
constexpr int kDefaultTbVariant = 0;   // 4 strips, 2 rows in flight
// block heights tried, tallest first (pick_tb_rows)
constexpr int kTbRowLadder[] = {576, 384, 288, 192};
constexpr int kTbRowLadderLen = 4;
constexpr int kTbSmallRows = 32;       // short block rows the work order takes last ...
constexpr int kTbSmallRounds = 2;      // ... about this many resident rounds of them
constexpr int kTbReserve = 16;         // slots a pipelined interior launch leaves free
// the split rhs ring (sor_tbh.h): stages 0 .. K-1 read registers, the rest LDS;
// both rings have S slots, S = max(2K + D, 2(T - K) + 1) rounded up to even.
// K: as few register stages as the LDS allows -- S <= kHrMaxSlots rows of 1 KB
// per wave (two workgroups of four waves: 144 KB of the CU's 160)
constexpr int kHrMaxSlots = 18;
// The skewed form (sk = 1) keeps one more row in each ring.
MISOR_HD constexpr int hr_cost(int T, int D, int k, int sk = 0) {
    const int a = 2 * k + D + sk, b = 2 * (T - k) + 1 + sk;
    const int s = a > b ? a : b;
    return s + (s & 1);
}
MISOR_HD constexpr int hr_k(int T, int D, int sk = 0) {
    for (int k = 0; k <= T; ++k)
        if (hr_cost(T, D, k, sk) <= kHrMaxSlots) return k;
    return T;
}
MISOR_HD constexpr int hr_slots(int T, int D, int sk = 0) {
    return hr_cost(T, D, hr_k(T, D, sk), sk);
}

struct SweepParams {
    long long pitch;
    int ni, nj;          // local interior size
    int rows_per_block;  // H (temporally blocked: block rows 0 .. nby_big-1 are H tall)
    int nby;             // temporally blocked: block rows; rows nby_big .. nby-2 are
                         // h_small tall, the last one takes the rest (tb_geometry)
    int nby_big, h_small;
    int parity;          // (ioff + joff) & 1 : global colour of local cell (0,0)
    int ghost_left, ghost_right, ghost_bottom, ghost_top;  // physical boundary -> Neumann copy
    int red_lo_i, red_hi_i, red_lo_j, red_hi_j;  // cells whose red value is computed
    int variant;         // index into kSweepVariants
    int nbx, nblocks;    // launch geometry (logical blocks nbx x nby)
    int xcd_remap;       // deal consecutive logical blocks to one XCD
    int part;            // 0: all blocks, 1: interior blocks only, 2: boundary blocks only
    int int_lo_i, int_hi_i, int_lo_j, int_hi_j;  // footprint bounds of an interior block
    int upd_lo_i, upd_hi_i, upd_lo_j, upd_hi_j;  // temporally blocked: cells updated
                                                 // (1..n on physical sides, all on
                                                 // neighbour sides)
    double idx2, idy2, coef;  // 1/dx^2, 1/dy^2, factor (RB) or omega*factor (RBA)
    int pow2;                 // idx2 == idy2 == 2^m, m >= 0: the default TB kernel's P2 form
    int reserve;              // persistent launch: leave this many workgroup slots free
                              // (host only; the comm / edge streams' kernels run there)
    // chained passes (sor_tb.h rb_tbc_kernel): vertical runs of blocks taken
    // from the launch's segment list, with work stealing
    int chain;                // 1: blocks are 4 ring lengths tall, runs chain them
    int nseg0;                // segments of the launch's initial list
    int seg_cap;              // dynamic segment slots (created by steals)
    int chain_blocks;         // blocks in the launch (its part)
    int chain_edge;           // the edge list (strips at a physical left / right side)
    int lite;                 // the split ring's steady chunks count the residual of the
                              // stages before the last one on one row in S (a lower
                              // bound; misor_solve.hip kLite)
    int chain_grid;           // edge list: its workgroups (the first of the launch)
    int seg_run[9];           // XCD x takes the initial segments [seg_run[x], seg_run[x+1])
    unsigned long long* trace;  // diagnostics (MISOR_CHAIN_TRACE): per block L, 3 words --
                                // start and end (wall clock, 100 MHz), workgroup | run start
    const unsigned long long* seg_tmpl;  // the initial list (device; copied per launch)
    // the split ring's edge kernel: once its own list is done, its workgroups
    // steal from the main list's work area (initialised before either kernel
    // starts: no_init on the main launch); nullptr: no second list
    int* alt_work = nullptr;
    int alt_nseg0 = 0;
    int no_init = 0;          // the work area is initialised already (misor_solve.hip)
};

// Chained passes: a segment word holds the next unclaimed block row (bits
// 0..25), the end block row, exclusive (26..51), and the column (52..63).
// Work area of a chained launch: int head[kChainHead] (0..7: per-XCD tickets
// of the initial segments, 8: dynamic segments created), then the words.
constexpr int kChainBits = 26;
constexpr unsigned long long kChainMask = (1ull << kChainBits) - 1;
constexpr int kChainHead = 16;
constexpr int kChainSegCap = 4096;       // dynamic slots per launch
constexpr int kChainRingsPerBlock = 4;   // block height of a chained pass, in ring lengths
// the chained split-ring pass (sor_tbh.h rb_tbhc_kernel): blocks of 8 ring
// lengths (144 rows at T = 10), a block of a column at a physical left / right
// side costing ~2.5 others (its strip's kSteadyEdge chunks run ~1.8x a steady
// strip's; profiles/r05_hrsweep2_*.txt)
constexpr int kHrChainRingsPerBlock = 8;
constexpr double kHrChainEdgeCost = 2.5;
// the same on a decomposed rank's block (its passes split in two parts around
// the halo exchange): 10 ring lengths (180 rows) and an edge-column block at 3
// others -- wall ms per iteration of the pipelined loop, alternated on one box
// (profiles/r05_rank_geometry_ab.txt): the 8-GPU rank block with physical
// left + bottom sides 0.121 against 0.139 at 8 / 2.5, bottom only 0.125 vs
// 0.127, the 4-GPU block 0.204 vs 0.230, the 2-GPU block unchanged (sweeps:
// r05_edge_rings_ab*.txt; a single rank, without the split, stays at 144 rows)
constexpr int kHrChainRingsDist = 10;
constexpr double kHrChainEdgeCostDist = 3.0;
// chained passes by default on local blocks below this many cells: there the
// unchained blocks are short and their 4T warm-up rows cost most (one 8-GPU
// rank's 8192 x 16384 of the 32768^2 bench: 0.106 vs 0.110-0.118 ms per
// iteration); on larger blocks the unchained 576-row blocks are ahead
// (32768^2: 0.661 vs 0.695-0.709; profiles/r03_chain_rows.txt)
constexpr long long kChainCells = 1LL << 28;
constexpr double kChainEdgeCost = 2.0;   // a block of a column at a physical left / right
                                         // side, in steady blocks (segment lengths): a
                                         // kSteadyEdge block measures ~1.5; the edge
                                         // kernel's workgroups cannot steal from the main
                                         // one's, so it is given a few more than its share
                                         // (profiles/r03_chain_edge_cost.txt)
MISOR_HD inline unsigned long long chain_word(int col, int next, int end) {
    return ((unsigned long long)col << (2 * kChainBits)) |
           ((unsigned long long)end << kChainBits) | (unsigned long long)next;
}

}  // namespace misor

#pragma GCC visibility push(hidden)  // not exported from libmisor.so
namespace misor {

// ---------------------------------------------------------------------------
// The variant lookups
// ---------------------------------------------------------------------------

constexpr int kBuiltTbVariants = (int)(sizeof(kTbVariants) / sizeof(kTbVariants[0]));

// the built variant of that public number; a retired one: max_t = 0
inline const TbVariant& tb_variant(int variant) {
    static constexpr TbVariant retired = {-1, 4, 2, 0, 0, 0};
    for (const TbVariant& v : kTbVariants)
        if (v.id == variant) return v;
    return retired;
}

inline int tb_max_t(int variant) { return tb_variant(variant).max_t; }

// owned columns of one wave's strip
inline int tb_out_width(int T, int /*variant*/) { return kStripCells - 4 * T; }

inline int tb_waves(int variant) { return tb_variant(variant).waves; }

// rhs ring slots of the steady march: interior block heights are multiples of it
inline int tb_ring_slots(int T, int variant) {
    const TbVariant& v = tb_variant(variant);
    if (v.hr) return hr_slots(T, v.ahead, v.skew && T >= 2 ? 1 : 0);
    return 2 * T + v.ahead + (v.ahead & 1);  // sor_tb.h ring_slots
}

// block columns of a pass of T iterations
inline int tb_nbx(int ni, int T, int variant) {
    const int ow = tb_out_width(T, variant);
    const int strips = (ni + ow - 1) / ow;
    const int waves = tb_waves(variant);
    return (strips + waves - 1) / waves;
}

// the single sweep's blocks (sor_kernels.hip rb_sweep_kernel): one partial each
inline int sweep_partials(int ni, int nj, int rows_per_block, int waves, int* nbx, int* nby) {
    const int strips = (ni + kStripCells - 1) / kStripCells;
    *nbx = (strips + waves - 1) / waves;
    *nby = (nj + rows_per_block - 1) / rows_per_block;
    return (*nbx) * (*nby);
}

inline int pick_rows_per_block(int ni, int nj, int waves) {
    // enough workgroups to fill 256 CUs several times, but long enough row
    // marches that the two redundant halo rows per block stay cheap
    const int strips = (ni + kStripCells - 1) / kStripCells;
    const int nbx = (strips + waves - 1) / waves;
    const int target_blocks = 2048;
    int want_nby = (target_blocks + nbx - 1) / nbx;
    int h = (nj + want_nby - 1) / want_nby;
    if (h < 4) h = 4;
    if (h > 16) h = 16;  // measured optimum at 32768^2 (profiles/r01_tune_rows.txt)
    return h;
}

// ---------------------------------------------------------------------------
// What a plan is derived from
// ---------------------------------------------------------------------------

// what the plans read off a grid (misor_grid.h tb_input)
struct TbInput {
    int ni, nj;  // the local block
    bool dist;   // decomposed
    int imax, jmax, dims[2], max_depth;  // the global grid, the process grid, the deepest halo plan
    int tb_chain;        // MISOR_TUNE_TB_CHAIN: 1 on, 0 off, -1 automatic
    bool tb_persistent;  // MISOR_TUNE_TB_PERSISTENT
    int tb_rows_req;     // MISOR_TUNE_TB_ROWS (0: automatic)
    int tb_reserve;      // MISOR_TUNE_TB_RESERVE
    int tsteps;          // requested T
    bool tsteps_set;     // ... by MISOR_TUNE_TSTEPS (else the default rule)
};

// workgroups of a persistent pass resident on the device at once, by built
// variant (in kTbVariants order) and T <= its max_t: the occupancy query
// (sor_tb.hip tb_resident), made once by the library; the checker makes it up
struct TbResidency {
    int n[kBuiltTbVariants][kMaxT + 1];
    int operator()(int T, int variant) const {
        for (int k = 0; k < kBuiltTbVariants; ++k)
            if (kTbVariants[k].id == variant) return n[k][T];
        return 0;
    }
};

// The cells a temporally blocked pass updates and the footprint bounds of its
// interior blocks, from tp's size and physical-side flags: same physics as
// the sweep, its own geometry; every cell of a neighbour's 2T-deep halo is
// updated (identical arithmetic), only the physical sides are bounded
inline void tb_bounds(SweepParams& tp) {
    constexpr int kBig = 1 << 29;
    tp.upd_lo_i = tp.ghost_left ? 1 : -kBig;
    tp.upd_hi_i = tp.ghost_right ? tp.ni : kBig;
    tp.upd_lo_j = tp.ghost_bottom ? 1 : -kBig;
    tp.upd_hi_j = tp.ghost_top ? tp.nj : kBig;
    // an interior block (overlapped pass) streams no halo cell of src
    tp.int_lo_i = tp.ghost_left ? -kBig : 1;
    tp.int_hi_i = tp.ghost_right ? kBig : tp.ni;
    tp.int_lo_j = tp.ghost_bottom ? -kBig : 1;
    tp.int_hi_j = tp.ghost_top ? kBig : tp.nj;
}

// The single sweep on a decomposed grid: blocks whose footprint (rows
// j0-2..j1+1, columns c0-2..c_end+1) stays clear of the halo on neighbour
// sides AND of the 2-deep send region can sweep while the exchange is in
// flight
inline void sweep_interior_bounds(SweepParams& sp) {
    sp.int_lo_i = !sp.ghost_left ? 3 : -1000000000;
    sp.int_hi_i = !sp.ghost_right ? sp.ni - 2 : 2000000000;
    sp.int_lo_j = !sp.ghost_bottom ? 3 : -1000000000;
    sp.int_hi_j = !sp.ghost_top ? sp.nj - 2 : 2000000000;
}

// ---------------------------------------------------------------------------
// The rules
// ---------------------------------------------------------------------------

// halo depth a decomposed pass of T iterations of `variant` exchanges: 2T, one
// row more for the skewed split ring (its leading stages run one row ahead of
// the trailing ones; the top rows of their residual windows at a neighbour
// above read row nj + 2T + 1)
inline int tb_halo_depth(int T, int variant) {
    return 2 * T + (T >= 2 && variant == kHrTbVariant ? 1 : 0);
}

// T that a multi-block solve of `variant` uses: the requested one, limited so
// that the halo of a decomposed run (tb_halo_depth) fits inside the smallest
// neighbour block.  The skewed split ring never runs with a 2T-deep halo: on a
// block whose smallest side is exactly 2T it runs T - 1 iterations a pass
// (misor_stats.iters_per_pass reports the T in effect).
inline int effective_tsteps(const TbInput& in, int variant) {
    int T = in.tsteps;
    if (T < 1) T = 1;
    if (T > kMaxT) T = kMaxT;
    if (in.dist) {
        const int mi = in.imax / in.dims[0], mj = in.jmax / in.dims[1];
        const int cap = std::min(std::min(mi, mj), in.max_depth);
        while (T > 1 && tb_halo_depth(T, variant) > cap) --T;
    }
    return T;
}

// Block height H of a pass of T iterations.  A block streams H + 4T rows for
// its H, so tall blocks waste less; short ones give a launch more workgroups.
// With one workgroup per block, round-1 measurements put the optimum near 192
// rows (profiles/r01_shape_sweep*.txt); with the persistent work-queue passes
// (the 64 workgroups of an XCD stream neighbouring blocks of one block row,
// and the pass ends on a band of short blocks) taller blocks pay off: 384 rows
// 0.796 vs 0.821 ms per iteration at 32768^2, 576-768 within noise of 384,
// 1536 slower (profiles/r02_tb_rows_persistent.txt).  H is a multiple of the
// static ring's S slots (sor_tb.hip: interior blocks march in chunks of S
// steps); smaller grids halve it until the launch has ~1024 workgroups.  The last block row takes the rest
// (at most H rows) and marches in pairs.
inline int pick_tb_rows(int ni, int nj, int T, int variant) {
    const long long nbx = tb_nbx(ni, T, variant);
    const int S = tb_ring_slots(T, variant);
    auto on_ring = [&](int h) { return S * std::max(1, (h + S / 2) / S); };
    // the tallest of the ladder that still gives the launch ~6 blocks per
    // resident workgroup (3000 blocks)
    int h = kTbRowLadder[0];
    for (int k = 0; k < kTbRowLadderLen; ++k) {
        h = kTbRowLadder[k];
        if (nbx * ((nj + on_ring(h) - 1) / on_ring(h)) >= 3000) break;
    }
    return on_ring(h);
}

inline bool chain_on(const TbInput& in, int variant) {
    if (!in.tb_persistent) return false;
    // the split-ring passes are always chained runs (the warm-up rows they
    // save are VALU work of a VALU-bound pass, sor_tbh.h rb_tbhc_kernel; an
    // unchained form measured 2-15% slower, profiles/r05_hrsweep*.txt)
    if (variant == kHrTbVariant) return true;
    const bool want = in.tb_chain > 0 ||
                      (in.tb_chain < 0 && (long long)in.ni * in.nj < kChainCells);
    return want && variant == kDefaultTbVariant;
}

// T when none was requested: 8 on large local blocks; on small ones 8 with
// chained passes (the default there), 7 without (kTsteps8Cells)
inline int default_tsteps(const TbInput& in, int variant) {
    const long long cells = (long long)in.ni * in.nj;
    return cells >= kTsteps8Cells || chain_on(in, variant) ? kDefaultTsteps : kSmallBlockTsteps;
}

// residual partials per stage of a pass: one per block, or one per block and
// wave for a chained pass (sor_tb.h chain_block_end)
inline int tb_parts(const SweepParams& tp) {
    return tp.chain ? tp.nblocks * tb_waves(tp.variant) : tp.nblocks;
}

// geometry of the temporally blocked pass with T iterations into `tp`: block
// columns and block rows.  Automatic geometry (no MISOR_TUNE_TB_ROWS request):
// blocks of pick_tb_rows' height H, then about two resident rounds of short
// ones (~32 rows) -- the work order takes them last, so the pass ends on
// blocks a sixth as long (the makespan of a persistent pass runs ~half a
// block past its average), at the cost of their extra halo rows -- and a last
// block row of one to two short-block heights (the rest; round 1 left up to H
// rows there, a long row-tested block at the very end of the order).
// (tools/scale_proxy.py, profiles/r02_small_rows.txt: the short band took one
// rank's 8192 x 16384 at 8 GPUs from 0.149 to 0.118 ms per iteration.)  A
// three-level form -- the bulk in 576-row blocks, one round of H, then the
// short band -- ran up to 1.7x slower on the small grids (the tall blocks
// hold their slots for a whole pass; profiles/r02_tb_levels.txt) and was
// dropped.  An explicit request gives uniform blocks of that height, the last
// row taking the rest.
inline void tb_geometry(const TbInput& in, const TbResidency& resident, int T, SweepParams& tp) {
    const int nj = in.nj, req = in.tb_rows_req;
    tp.nbx = tb_nbx(in.ni, T, tp.variant);
    const int S = tb_ring_slots(T, tp.variant);
    tp.chain = chain_on(in, tp.variant);
    if (tp.chain) {
        // chained passes: short blocks (the unit of residual partials and of
        // work stealing), long runs; every block row but the last a multiple
        // of the ring
        const int rings = tp.variant == kHrTbVariant
                              ? (in.dist ? kHrChainRingsDist : kHrChainRingsPerBlock)
                              : kChainRingsPerBlock;
        int h = req > 0 ? S * std::max(1, (req + S / 2) / S) : rings * S;
        if (h > nj) h = nj;
        tp.rows_per_block = h;
        tp.nby = (nj + h - 1) / h;
        tp.nby_big = tp.nby - 1;
        tp.h_small = h;
        tp.nblocks = tp.nbx * tp.nby;
        return;
    }
    int h = req > 0 ? req : pick_tb_rows(in.ni, nj, T, tp.variant);
    if (h > nj) h = nj;
    const int small_rows = kTbSmallRows;
    const double band_rounds = kTbSmallRounds;
    const int hs = S * std::max(1, (small_rows + S / 2) / S);
    int nbig = 0, ns = 0;
    if (req > 0 || hs >= h || nj < 4 * hs) {  // uniform blocks, the last takes the rest
        nbig = nj / h;
        if (nbig * h == nj && nbig > 0) --nbig;
    } else {
        const int band = std::min(
            (int)((band_rounds * resident(T, tp.variant) + tp.nbx - 1) / tp.nbx), nj / 4 / hs);
        nbig = std::max(0, (nj - band * hs - hs) / h);
        ns = std::max(0, (nj - nbig * h) / hs - 1);  // the last row: [hs, 2 hs)
    }
    tp.rows_per_block = h;
    tp.nby_big = nbig;
    tp.h_small = hs;
    tp.nby = nbig + ns + 1;
    tp.nblocks = tp.nbx * tp.nby;
}

// ---------------------------------------------------------------------------
// Which block is what: each predicate once, with the formula of the kernel
// that applies it -- sor_tb.h block_rows, tb_block's part test, chain_rows_ok
// and tb_strip2's cols_in; sor_tbh.h hr_chain_rows_ok and hr_cols_in.  The
// kernels keep their own copies: with block_rows and the part test shared from
// here, the gfx950 code objects of the T <= 8 units (sor_tb_inst.hip) came out
// different from before, and a launched kernel's code is not this header's to
// change.
// ---------------------------------------------------------------------------

// rows [j0, j1) of block row by: nby_big of H = rows_per_block rows, then
// h_small-row ones, the last takes the rest
inline void tb_block_rows(const SweepParams& prm, int by, int& j0, int& j1) {
    const int H = prm.rows_per_block;
    j0 = by < prm.nby_big ? 1 + by * H : 1 + prm.nby_big * H + (by - prm.nby_big) * prm.h_small;
    j1 = by == prm.nby - 1 ? prm.nj + 1 : j0 + (by < prm.nby_big ? H : prm.h_small);
}

// block (bx, by) of a pass of T iterations is interior (part 1 of an
// overlapped decomposed pass): its cone reads no halo cell of src.  (The
// skewed split ring streams one row more each way: its leading stages run a
// row ahead, and the residual they count reads it.)
inline bool tb_interior(const SweepParams& prm, int T, int bx, int by) {
    const int W = tb_waves(prm.variant), OW = tb_out_width(T, prm.variant);
    const int sk = prm.variant == kHrTbVariant && T >= 2 ? 1 : 0;
    int j0, j1;
    tb_block_rows(prm, by, j0, j1);
    const int lo = 1 + bx * W * OW - 2 * T;
    const int hi = 1 + (bx * W + W - 1) * OW - 2 * T + kStripCells - 1;
    return lo >= prm.int_lo_i && hi <= prm.int_hi_i && j0 - 2 * T - sk >= prm.int_lo_j &&
           j1 - 1 + 2 * T + sk <= prm.int_hi_j;
}

// block row by can be part of a chained run (a steady-able row): its cone
// clear of the physical bottom / top sides and a height the ring divides
inline bool tb_steady_row(const SweepParams& prm, int T, int by) {
    const int S = tb_ring_slots(T, prm.variant);
    int j0, j1;
    tb_block_rows(prm, by, j0, j1);
    return j0 - 2 * T >= prm.upd_lo_j && j1 - 1 + 2 * T <= prm.upd_hi_j && (j1 - j0) % S == 0 &&
           j1 > j0;
}

// block column bx has a strip at a physical left / right side (an edge
// column): that strip marches the general, lane-masked way
inline bool tb_edge_col(const SweepParams& prm, int T, int bx) {
    const int W = tb_waves(prm.variant), OW = tb_out_width(T, prm.variant);
    for (int w = 0; w < W; ++w) {
        const int c_out = 1 + (bx * W + w) * OW;
        if (c_out > prm.ni) break;
        const int c_ld = c_out - 2 * T;
        if (!(c_ld >= prm.upd_lo_i && c_ld + kStripCells - 1 <= prm.upd_hi_i &&
              (c_out + OW - 1 <= prm.ni || (prm.ni & 1) == 0)))
            return true;
    }
    return false;
}

// ---------------------------------------------------------------------------
// Sizing: what configure_tb stores and allocates for
// ---------------------------------------------------------------------------

struct TbSizing {
    int T;                // the effective T
    bool short_plan;      // capped solves may run as kShortT-iteration split-ring passes
    bool short_all;       // ... every solve of more than kDefaultTsteps iterations
    bool short_all_lite;  // ... the same while the residual lower bounds are on
    bool chained;         // some pass is a chained one: edge streams and work areas
    long long partials;   // block partials of the largest pass (ensure_partials)
    long long max_blocks; // the most blocks of any pass length
    long long work_bytes; // one work area of a chained launch
    char err[96];         // not empty: refused
};

// a block row of rows_per_block rows within the steady march's reach: it
// addresses a block's rows with 32-bit buffer offsets and marks lanes that do
// not store with offset 2^30 (every block row is at most rows_per_block tall)
inline bool tb_rows_fit(int rows_per_block, long long pitch) {
    return (rows_per_block + 4LL * kMaxT + 8) * pitch * 8 < (1LL << 30);
}

// tp: the grid's pass parameters, its variant the one being configured
inline TbSizing tb_sizing(const TbInput& in, const TbResidency& resident, const SweepParams& tp) {
    TbSizing z{};
    const int variant = tp.variant;
    const int Te = z.T = effective_tsteps(in, variant);
    // every pass length a solve may launch (T, the last pass of a capped
    // solve, a pass recomputed after convergence) has its own geometry; the
    // partials hold the largest
    long long need = 1;
    for (int Tp = 1; Tp <= std::max(1, Te); ++Tp) {
        SweepParams q = tp;
        tb_geometry(in, resident, Tp, q);
        if (!tb_rows_fit(q.rows_per_block, tp.pitch)) {
            snprintf(z.err, sizeof z.err, "tb rows %d: a block of rows exceeds 1 GiB",
                     q.rows_per_block);
            return z;
        }
        need = std::max(need, (long long)Tp * tb_parts(q));
    }
    // The short plan (misor_solve.hip short_plan_on): a solve capped at few
    // iterations runs them in fewer, longer passes of the split-ring kernel
    // when that saves a pass; its geometries share the partials
    // Where (round 5, the chained split ring; profiles/r05_plan_ab*.txt, wall
    // ms per iteration of 20- and 100-iteration solves against the T = 8 plan):
    //  - blocks of [2^26, 2^28) cells, where the T = 8 passes are chained
    //    (the 8-GPU rank block 8192 x 16384: 0.106 vs 0.123, in the pipelined
    //    loop 0.122 vs 0.142): every solve of more than 8 iterations;
    //  - a single rank of >= 2^29 cells (the 32768^2 bench grid: 0.676 vs 0.682
    //    at 100 iterations, 20 iterations in 2 passes instead of 3): the same;
    //  - a single rank of 2^28 cells, and decomposed blocks of >= 2^28 (the
    //    two- and four-GPU splits of the bench grid): only where it saves
    //    passes, pass_plan.h short_plan_saves_passes (at 100 iterations the two plans are
    //    within 1-3%; the 4-GPU rank block through the pipelined loop of round
    //    5, 20 iterations: 0.2247-0.2250 vs 0.2317-0.2327 ms per iteration,
    //    profiles/r05_plan_ab_ranks.txt -- round 4's loop measured the opposite).
    const long long cells = (long long)in.ni * in.nj;
    const bool small_chain = cells >= kHrAllCells && cells < kTsteps8Cells &&
                             chain_on(in, variant);
    z.short_all = small_chain || (!in.dist && cells >= 2 * kTsteps8Cells);
    //  - round 6: blocks of >= 2^28 cells too, one rank or decomposed, while
    //    the residual lower bounds are on (MISOR_TUNE_RES_LITE: one FMA per
    //    update fewer on the 10-iteration passes) -- NS config 5, 16384^2 with
    //    100 iterations per solve: 20.63-20.66 ms per step against 21.85-22.57
    //    for the 13 T = 8 passes (profiles/r06_ns_plan_ab.txt); the 4-GPU rank
    //    block (sides L, B) at 100 iterations: 0.2072-0.2081 against
    //    0.2189-0.2224 ms per iteration (profiles/r06_plan_ab_rank100.txt)
    z.short_all_lite = cells >= kTsteps8Cells;
    z.short_plan = variant == kDefaultTbVariant && !in.tsteps_set && in.tb_persistent &&
                   (z.short_all || (!chain_on(in, variant) &&
                                    cells >= (in.dist ? kShortDistCells : kTsteps8Cells)));
    if (z.short_plan) {
        for (int Tp = 1; Tp <= kShortT; ++Tp) {
            SweepParams q = tp;
            q.variant = kShortTbVariant;
            tb_geometry(in, resident, Tp, q);
            if (!tb_rows_fit(q.rows_per_block, tp.pitch)) {
                z.short_plan = false;
                break;
            }
            need = std::max(need, (long long)Tp * tb_parts(q));
        }
    }
    z.partials = need;
    const bool short_chain = z.short_plan && chain_on(in, kShortTbVariant);
    z.chained = chain_on(in, variant) || short_chain;
    // work areas (parts 0 / 1, part 2): head, an initial list of at most
    // one segment per block, the dynamic slots; sized once for every pass
    // length (a launch may still be using them when a plan is built)
    long long most = 1;
    for (int Tp = 1; Tp <= std::max(2, Te); ++Tp) {
        SweepParams q = tp;
        tb_geometry(in, resident, Tp, q);
        most = std::max(most, (long long)q.nblocks);
    }
    for (int Tp = 1; short_chain && Tp <= kShortT; ++Tp) {
        SweepParams q = tp;
        q.variant = kShortTbVariant;
        tb_geometry(in, resident, Tp, q);
        most = std::max(most, (long long)q.nblocks);
    }
    z.max_blocks = most;
    z.work_bytes = kChainHead * (long long)sizeof(int) +
                   (most + kChainSegCap) * (long long)sizeof(unsigned long long);
    return z;
}

// ---------------------------------------------------------------------------
// The segment lists of chained passes
// ---------------------------------------------------------------------------

// one initial segment list: its words in XCD order
struct ChainSegs {
    std::vector<unsigned long long> words;
    int nseg0 = 0, blocks = 0;
    int run[9] = {};  // XCD x takes words [run[x], run[x + 1])
};
// the lists of the main kernel and of the edge kernel (columns at a physical
// left / right side, launched beside it)
struct ChainLists {
    ChainSegs main, edge;
    int reserve = -1;  // the split ring's parts 1 / 2: the slots part 1 leaves to part 2
};

// The initial segment lists of a chained pass (sor_tb.h rb_tbc_kernel) of
// `variant` and Tp iterations, part `part`; tp0: the grid's pass parameters
// (variant: the configured one or the split ring of the short plan; the plan
// follows that variant's geometry: strip width, ring, block height).  Blocks
// in a part: all (0), those whose cone stays clear of the halo (1,
// tb_interior), the rest (2).  Along a column, blocks of steady-able rows
// (tb_steady_row) form runs, each split into segments of about B / G blocks
// (B: blocks of the part, G: workgroups resident at once), so that the initial
// list gives every resident workgroup about one segment; every other block
// (cone at a physical bottom / top side, a last block off the ring) is a
// segment of its own.  The list is column-interleaved (segment s of every
// column, then s + 1 ...): the XCD queues deal contiguous runs of it, so
// neighbouring columns -- whose strips share 4T columns -- march side by side
// on one XCD.
inline ChainLists chain_lists(const TbInput& in, const TbResidency& resident,
                              const SweepParams& tp0, int variant, int Tp, int part) {
    ChainLists pl;
    SweepParams tp = tp0;
    tp.variant = variant;
    tb_geometry(in, resident, Tp, tp);
    const int nbx = tp.nbx, nby = tp.nby;
    auto interior = [&](int bx, int by) { return tb_interior(tp, Tp, bx, by); };
    auto steady = [&](int by) { return tb_steady_row(tp, Tp, by); };
    auto in_part = [&](int bx, int by) { return part == 0 || interior(bx, by) == (part == 1); };
    auto edge_col = [&](int bx) { return tb_edge_col(tp, Tp, bx); };
    // Cost model, in steady-block units: a block of an edge column costs
    // kChainEdgeCost (kSteadyEdge chunks), a block of a row that is not
    // steady-able (a segment of its own) that much plus its 4T warm-up rows.
    // The segments are cut so that each costs about (total / resident
    // workgroups): every workgroup starts one at once and they end together.
    const double E = variant == kHrTbVariant ? (in.dist ? kHrChainEdgeCostDist : kHrChainEdgeCost)
                                             : kChainEdgeCost;
    const int H = tp.rows_per_block;
    // The split ring's plan (round 5): main and edge lists, segments of cost /
    // resident workgroups, and the pipelined pass's part-2 slots sized to its
    // cost share (below): the 8-GPU rank block's pipelined loop 0.130-0.135
    // against 0.145-0.147 ms per iteration with physical left and bottom
    // sides, 0.130-0.131 against 0.136-0.138 with the bottom one only
    // (profiles/r05_reserve_ab.txt).  One list for both kinds of column with
    // exactly one item per workgroup measured 1-3% slower at 32768^2 and on
    // the 8-GPU rank block (profiles/r05_hr_plan_ab.txt: edge-column blocks ran
    // 1.4x longer among the main list's) and was removed.
    const bool sized = variant == kHrTbVariant && part != 0;
    std::vector<unsigned long long> singles;
    double cost = 0;
    long long Bm = 0, Be = 0;
    for (int bx = 0; bx < nbx; ++bx) {
        const bool ecol = edge_col(bx);
        for (int by = 0; by < nby; ++by) {
            if (!in_part(bx, by)) continue;
            if (!steady(by)) {
                singles.push_back(chain_word(bx, by, by + 1));
                cost += E * (H + 4.0 * Tp) / H;
                ++Bm;
            } else {
                cost += ecol ? E : 1.0;
                ++(ecol ? Be : Bm);
            }
        }
    }
    const int G = std::max(8, resident(Tp, tp.variant));
    // a pipelined pass's parts (1: interior blocks, 2: the blocks whose cone
    // reads the halo, launched once the exchange is in): part 2 runs beside
    // part 1 on the slots part 1 leaves free, so those are sized to its share
    // of the pass's cost (at least MISOR_TUNE_TB_RESERVE, which also serves the
    // exchange's kernels) and each part's items to its slots -- part 2's
    // blocks then run as chained runs of the border columns instead of one
    // warmed-up block per slot at the end of the pass
    int Gp = G;
    if (sized) {
        double c12[3] = {0, 0, 0};
        for (int bx = 0; bx < nbx; ++bx) {
            const bool ecol = edge_col(bx);
            for (int by = 0; by < nby; ++by)
                c12[interior(bx, by) ? 1 : 2] +=
                    !steady(by) ? E * (H + 4.0 * Tp) / H : ecol ? E : 1.0;
        }
        const int R = std::min(G / 2, std::max(in.tb_reserve,
                                               (int)llround(G * c12[2] / (c12[1] + c12[2]))));
        pl.reserve = R;
        Gp = std::max(8, part == 1 ? G - R : R);
    }
    double per = std::max(1.0, cost / Gp);  // cost of one segment
    // segments of one steady run of n blocks of cost c1 each
    auto pieces = [&](int n, double c1) {
        return std::min(n, std::max(1, (int)llround(n * c1 / per)));
    };
    auto each_run = [&](auto&& fn) {  // fn(bx, by, n, edge column)
        for (int bx = 0; bx < nbx; ++bx) {
            const bool ecol = edge_col(bx);
            for (int by = 0; by < nby;) {
                if (!in_part(bx, by) || !steady(by)) {
                    ++by;
                    continue;
                }
                int e = by;
                while (e < nby && in_part(bx, e) && steady(e)) ++e;
                fn(bx, by, e - by, ecol);
                by = e;
            }
        }
    };
    std::vector<unsigned long long> edge, inner;  // inner: column-interleaved
    std::vector<std::vector<unsigned long long>> col(nbx);
    each_run([&](int bx, int by, int n, bool ecol) {
        const int k = pieces(n, ecol ? E : 1.0);
        for (int q = 0; q < k; ++q) {
            const unsigned long long w = chain_word(
                bx, by + (int)((long long)n * q / k), by + (int)((long long)n * (q + 1) / k));
            if (ecol) edge.push_back(w);
            else col[bx].push_back(w);
        }
    });
    for (size_t q = 0;; ++q) {
        bool any = false;
        for (int bx = 0; bx < nbx; ++bx)
            if (q < col[bx].size()) {
                inner.push_back(col[bx][q]);
                any = true;
            }
        if (!any) break;
    }
    // XCD runs: the main list -- singles dealt round-robin first, then the
    // inner list in 8 contiguous parts; the edge list round-robin
    auto concat = [](ChainSegs& L, const std::vector<unsigned long long>* xl, long long blocks) {
        for (int x = 0; x < 8; ++x) {
            L.run[x] = (int)L.words.size();
            L.words.insert(L.words.end(), xl[x].begin(), xl[x].end());
        }
        L.run[8] = (int)L.words.size();
        L.nseg0 = (int)L.words.size();
        L.blocks = (int)blocks;
    };
    std::vector<unsigned long long> xm[8], xe[8];
    for (size_t k = 0; k < singles.size(); ++k) xm[k % 8].push_back(singles[k]);
    for (int x = 0; x < 8; ++x)
        for (size_t k = inner.size() * x / 8; k < inner.size() * (x + 1) / 8; ++k)
            xm[x].push_back(inner[k]);
    for (size_t k = 0; k < edge.size(); ++k) xe[k % 8].push_back(edge[k]);
    concat(pl.main, xm, Bm);
    concat(pl.edge, xe, Be);
    return pl;
}

}  // namespace misor
#pragma GCC visibility pop
