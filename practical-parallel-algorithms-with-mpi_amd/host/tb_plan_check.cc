// tb_plan_check.cc -- the launch plans of the temporally blocked pass
// (csrc/tb_plan.h) on the CPU, under AddressSanitizer +
// UndefinedBehaviorSanitizer (make asan -> bin/asan/tb-plan-check;
// tests/test_sanitize_cpu.py).  This arithmetic decides which blocks of a
// pass exist and who runs them: a block missing from a segment list is never
// swept, one listed twice is swept by two workgroups at once.  Here the block
// rows of every geometry are followed row by row and every block of every
// list is marked; argv[1] is the table recorded from tb_geometry and
// chain_plan before they moved here (tests/golden/tb_plan_parent.txt), which
// must come out again line for line.
// Exit 0 and "all checks passed" when every check holds.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "tb_plan.h"

using namespace misor;

static int fails = 0;
static char ctx[256] = "";
#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            if (++fails <= 20)                                                            \
                fprintf(stderr, "check failed %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, ctx); \
        }                                                                                 \
    } while (0)

static long long n_geom = 0, n_lists = 0;

// the library's layout pitch (misor_internal.h layout_pitch: strips of 16 waves)
static long long pitch_of(int ni) { return 160 + (long long)((ni + 2047) / 2048) * 2048; }

// sides: physical left 1, right 2, bottom 4, top 8
static SweepParams params(int ni, int nj, int sides, int variant) {
    SweepParams tp{};
    tp.pitch = pitch_of(ni);
    tp.ni = ni;
    tp.nj = nj;
    tp.ghost_left = sides & 1;
    tp.ghost_right = (sides >> 1) & 1;
    tp.ghost_bottom = (sides >> 2) & 1;
    tp.ghost_top = (sides >> 3) & 1;
    tb_bounds(tp);
    tp.variant = variant;
    return tp;
}

static TbResidency residency(int n) {
    TbResidency r{};
    for (int k = 0; k < kBuiltTbVariants; ++k)
        for (int T = 1; T <= kTbVariants[k].max_t; ++T) r.n[k][T] = n;
    return r;
}

static void set_ctx(const TbInput& in, int sides, int variant, int T, int resident, int part) {
    snprintf(ctx, sizeof ctx,
             "%d x %d dist %d sides %d chain %d persistent %d rows %d variant %d T %d resident "
             "%d part %d",
             in.ni, in.nj, (int)in.dist, sides, in.tb_chain, (int)in.tb_persistent, in.tb_rows_req,
             variant, T, resident, part);
}

// the geometry of one pass length: tp after tb_geometry
static void check_geometry(const TbInput& in, int T, const SweepParams& tp) {
    ++n_geom;
    const int S = tb_ring_slots(T, tp.variant);
    CHECK(tp.nby >= 1 && tp.nby_big >= 0 && tp.nby_big <= tp.nby - 1);
    CHECK(tp.rows_per_block >= 1 && tp.h_small >= 1);
    int next = 1;  // the block rows tile [1, nj + 1)
    for (int by = 0; by < tp.nby; ++by) {
        int j0, j1;
        tb_block_rows(tp, by, j0, j1);
        CHECK(j0 == next && j1 > j0);
        CHECK(j1 - j0 <= tp.rows_per_block);  // (tb_rows_fit's premise)
        if (by < tp.nby_big) CHECK(j1 - j0 == tp.rows_per_block);
        else if (by < tp.nby - 1) CHECK(j1 - j0 == tp.h_small);
        if (tp.chain && by < tp.nby - 1) CHECK((j1 - j0) % S == 0);
        next = j1;
    }
    CHECK(next == in.nj + 1);
    // nbx: the smallest count whose strips cover ni
    const long long cols = (long long)tb_waves(tp.variant) * tb_out_width(T, tp.variant);
    CHECK(tp.nbx >= 1 && tp.nbx * cols >= in.ni && (tp.nbx - 1) * cols < in.ni);
    CHECK(tp.nblocks == tp.nbx * tp.nby);
    CHECK(tb_parts(tp) == (tp.chain ? tp.nblocks * tb_waves(tp.variant) : tp.nblocks));
    CHECK((tp.chain != 0) == chain_on(in, tp.variant));
}

static int word_next(unsigned long long w) { return (int)(w & kChainMask); }
static int word_end(unsigned long long w) { return (int)((w >> kChainBits) & kChainMask); }
static int word_col(unsigned long long w) { return (int)(w >> (2 * kChainBits)); }

// the lists of one part: mark[by * nbx + bx] counts the segments holding the block
static void check_lists(const TbInput& in, int T, const SweepParams& tp, int part, int G,
                        const ChainLists& pl, std::vector<int>& mark) {
    ++n_lists;
    const int nbx = tp.nbx, nby = tp.nby;
    mark.assign((size_t)nbx * nby, 0);
    long long listed[2] = {0, 0};
    const ChainSegs* both[2] = {&pl.main, &pl.edge};
    for (int e = 0; e < 2; ++e) {
        const ChainSegs& L = *both[e];
        CHECK(L.nseg0 == (int)L.words.size());
        CHECK(L.run[0] == 0 && L.run[8] == L.nseg0);
        for (int x = 0; x < 8; ++x) CHECK(L.run[x] <= L.run[x + 1]);
        for (unsigned long long w : L.words) {
            const int n = word_next(w), end = word_end(w), bx = word_col(w);
            CHECK(0 <= n && n < end && end <= nby && 0 <= bx && bx < nbx && bx < (1 << 12));
            if (!(0 <= n && n < end && end <= nby && 0 <= bx && bx < nbx)) continue;
            const bool ecol = tb_edge_col(tp, T, bx);
            for (int by = n; by < end; ++by) {
                ++mark[(size_t)by * nbx + bx];
                const bool steady = tb_steady_row(tp, T, by);
                // a run holds steady rows only; any other block is a segment alone
                if (end - n > 1) CHECK(steady);
                // the edge list: exactly the steady blocks of the edge columns
                CHECK((e == 1) == (ecol && steady));
            }
            listed[e] += end - n;
        }
        CHECK(L.blocks == listed[e]);
    }
    // every block of the part in exactly one segment, no other block in any
    for (int by = 0; by < nby; ++by)
        for (int bx = 0; bx < nbx; ++bx) {
            const bool in_part = part == 0 || tb_interior(tp, T, bx, by) == (part == 1);
            CHECK(mark[(size_t)by * nbx + bx] == (in_part ? 1 : 0));
        }
    if (tp.variant == kHrTbVariant && part != 0) {
        CHECK(pl.reserve >= std::min(in.tb_reserve, G / 2) && pl.reserve <= G / 2);
    } else {
        CHECK(pl.reserve == -1);
    }
}

// every pass length of one configuration: the sizing and the geometries (the
// physical sides change neither), then the segment lists of every part for
// each combination of physical sides in `side_sets` (bit s: check sides = s)
static void check_config(const TbInput& in0, int variant, int resident, unsigned side_sets) {
    const TbResidency res = residency(resident);
    const int G = std::max(8, resident);
    std::vector<int> mark, mark1;
    for (int T = 1; T <= tb_max_t(variant); ++T) {
        TbInput in = in0;
        in.tsteps = T;
        set_ctx(in, -1, variant, T, resident, -1);
        const SweepParams tp0 = params(in.ni, in.nj, 15, variant);

        // effective_tsteps: its halo fits, and T + 1 would not or was not asked for
        const int Te = effective_tsteps(in, variant);
        CHECK(Te >= 1 && Te <= T);
        if (in.dist) {
            const int cap = std::min(std::min(in.imax / in.dims[0], in.jmax / in.dims[1]),
                                     in.max_depth);
            CHECK(Te == 1 || tb_halo_depth(Te, variant) <= cap);
            CHECK(Te == T || tb_halo_depth(Te + 1, variant) > cap);
        } else {
            CHECK(Te == T);
        }

        // the sizing: refused exactly where a pass length's block row is too
        // tall, else the largest of every pass length
        const TbSizing z = tb_sizing(in, res, tp0);
        bool too_tall = false;
        long long need = 1, most = 1;
        for (int Tp = 1; Tp <= std::max(2, Te); ++Tp) {
            SweepParams q = tp0;
            tb_geometry(in, res, Tp, q);
            check_geometry(in, Tp, q);
            if (Tp <= Te) {
                if ((q.rows_per_block + 4LL * kMaxT + 8) * tp0.pitch * 8 >= (1LL << 30))
                    too_tall = true;
                need = std::max(need, (long long)Tp * tb_parts(q));
            }
            most = std::max(most, (long long)q.nblocks);
        }
        CHECK(too_tall == (z.err[0] != '\0'));
        if (too_tall) {
            CHECK(strstr(z.err, "exceeds 1 GiB") != nullptr);
        } else {
            CHECK(z.T == Te);
            CHECK(z.partials >= need && z.max_blocks >= most);
            if (!z.short_plan) CHECK(z.partials == need && z.max_blocks == most);
            CHECK(!z.short_plan ||
                  (variant == kDefaultTbVariant && !in.tsteps_set && in.tb_persistent));
            CHECK(z.chained ==
                  (chain_on(in, variant) || (z.short_plan && chain_on(in, kShortTbVariant))));
            CHECK(z.work_bytes == 4LL * kChainHead + 8LL * (z.max_blocks + kChainSegCap));
        }

        if (!chain_on(in, variant)) continue;
        for (int sides = 0; sides < 16; ++sides) {
            if (!(side_sets >> sides & 1)) continue;
            const SweepParams tps = params(in.ni, in.nj, sides, variant);
            SweepParams tp = tps;
            tb_geometry(in, res, T, tp);
            for (int part = 0; part < 3; ++part) {
                set_ctx(in, sides, variant, T, resident, part);
                const ChainLists pl = chain_lists(in, res, tps, variant, T, part);
                check_lists(in, T, tp, part, G, pl, part == 1 ? mark1 : mark);
                if (part == 2)  // parts 1 and 2: disjoint, together part 0
                    for (size_t q = 0; q < mark.size(); ++q) CHECK(mark[q] + mark1[q] == 1);
            }
        }
    }
}

static TbInput input(int ni, int nj, bool dist, int chain, bool persistent, int rows) {
    TbInput in{};
    in.ni = ni;
    in.nj = nj;
    in.dist = dist;
    // decomposed: a 3 x 3 process grid of such blocks; the deepest halo plan
    // as decomp2.h max_halo_depth gives it
    in.dims[0] = in.dims[1] = dist ? 3 : 1;
    in.imax = ni * in.dims[0];
    in.jmax = nj * in.dims[1];
    in.max_depth = dist ? std::max(2, std::min(2 * kMaxT + 1, std::min(ni, nj))) : 2;
    in.tb_chain = chain;
    in.tb_persistent = persistent;
    in.tb_rows_req = rows;
    in.tb_reserve = kTbReserve;
    in.tsteps_set = false;
    return in;
}

static void sweep() {
    const int sizes[] = {2, 3, 17, 88, 89, 127, 128, 129, 352, 353, 1000, 4096};
    const int tall[2][2] = {{8192, 16384}, {32768, 32768}};
    const int residents[] = {8, 64, 512, 1024};
    const unsigned kAllSides = 0xffffu, kPhysical = 1u << 15;
    std::vector<std::pair<int, int>> shapes;
    for (int ni : sizes)
        for (int nj : sizes) shapes.push_back({ni, nj});
    for (const auto& t : tall) shapes.push_back({t[0], t[1]});
    for (const auto& sh : shapes) {
        const int ni = sh.first, nj = sh.second;
        const bool big = (long long)ni * nj > 4096LL * 4096;
        const int rows_req[] = {0, 1, 7, 32, 100, nj, nj + 5};
        for (const TbVariant& v : kTbVariants)
            for (int rows : rows_req)
                for (int chain = -1; chain <= 1; ++chain)
                    for (int persistent = 0; persistent <= 1; ++persistent) {
                        if (v.id == kHrTbVariant && !persistent) continue;  // configure_tb refuses
                        const TbInput one = input(ni, nj, false, chain, persistent, rows);
                        const TbInput dec = input(ni, nj, true, chain, persistent, rows);
                        // (MISOR_TUNE_TB_CHAIN enters through chain_on alone: forced
                        // to what the automatic rule gives, it is the same case)
                        const TbInput aut = input(ni, nj, false, -1, persistent, rows);
                        if (chain != -1 && chain_on(one, v.id) == chain_on(aut, v.id)) continue;
                        // the resident count enters the lists and the automatic
                        // unchained geometry: every count at the automatic height,
                        // the device's and one other at a height asked for, one
                        // where it does not enter
                        const int other = chain_on(one, v.id) ? residents[(rows + nj) % 4] : 512;
                        for (int resident : residents) {
                            if (rows != 0 && resident != 512 && resident != other) continue;
                            // The lists: a single rank has every side physical, a
                            // decomposed block any combination.  On the tall shapes
                            // (up to millions of blocks) only at the heights the
                            // library picks or 100 rows and the device's count, and
                            // decomposed below.
                            const bool lists =
                                !big || ((rows == 0 || rows == 100) && resident == 512);
                            check_config(one, v.id, resident, lists ? kPhysical : 0);
                            // (every combination of sides at the device's count
                            // and the automatic or a short height; at the rest one
                            // combination, and none physical at the device's count)
                            const bool all = resident == 512 && (rows == 0 || rows == 7);
                            const unsigned some =
                                (resident == 512 ? 1u : 0u) | 1u << ((resident + rows) % 14 + 1);
                            check_config(dec, v.id, resident, big ? 0 : all ? kAllSides : some);
                        }
                    }
    }
    // the tall shapes decomposed, every side combination, at the device's count
    for (const auto& t : tall)
        for (int vid : {kDefaultTbVariant, kHrTbVariant})
            check_config(input(t[0], t[1], true, -1, true, 0), vid, 512, kAllSides);
    // a different MISOR_TUNE_TB_RESERVE: the part-2 slots stay within [., G / 2]
    for (int reserve : {0, 64, 400}) {
        TbInput in = input(1000, 4096, true, -1, true, 0);
        in.tb_reserve = reserve;
        check_config(in, kHrTbVariant, 512, kAllSides);
    }
}

static unsigned long long fnv1a(const std::vector<unsigned long long>& words) {
    unsigned long long h = 14695981039346656037ull;
    for (unsigned long long w : words)
        for (int b = 0; b < 8; ++b) {
            h ^= (w >> (8 * b)) & 0xff;
            h *= 1099511628211ull;
        }
    return h;
}

// the recorded table: every line again from this header
static int check_table(const char* path) {
    std::ifstream f(path);
    if (!f) {
        fprintf(stderr, "cannot read %s\n", path);
        return -1;
    }
    int lines = 0;
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream s(line);
        int ni, nj, dist, imax, jmax, d0, d1, depth, sides, chain, pers, rows, reserve, variant, T,
            resident, part;
        s >> ni >> nj >> dist >> imax >> jmax >> d0 >> d1 >> depth >> sides >> chain >> pers >>
            rows >> reserve >> variant >> T >> resident >> part;
        snprintf(ctx, sizeof ctx, "table line %d", ++lines);
        CHECK(!s.fail());
        if (s.fail()) continue;
        TbInput in{};
        in.ni = ni, in.nj = nj, in.dist = dist != 0, in.imax = imax, in.jmax = jmax;
        in.dims[0] = d0, in.dims[1] = d1, in.max_depth = depth;
        in.tb_chain = chain, in.tb_persistent = pers != 0, in.tb_rows_req = rows;
        in.tb_reserve = reserve, in.tsteps = T, in.tsteps_set = true;
        const TbResidency res = residency(resident);
        const SweepParams tp0 = params(ni, nj, sides, variant);
        SweepParams tp = tp0;
        tb_geometry(in, res, T, tp);
        check_geometry(in, T, tp);
        std::ostringstream o;
        o << tp.nbx << ' ' << tp.nby << ' ' << tp.nby_big << ' ' << tp.h_small << ' '
          << tp.rows_per_block << ' ' << tp.chain;
        if (tp.chain) {
            const ChainLists pl = chain_lists(in, res, tp0, variant, T, part);
            std::vector<int> mark;
            check_lists(in, T, tp, part, std::max(8, resident), pl, mark);
            o << ' ' << pl.reserve;
            for (const ChainSegs* L : {&pl.main, &pl.edge}) {
                o << ' ' << L->nseg0 << ' ' << L->blocks;
                for (int x = 0; x < 9; ++x) o << ' ' << L->run[x];
                char hex[17];
                snprintf(hex, sizeof hex, "%016llx", fnv1a(L->words));
                o << ' ' << hex;
            }
        }
        // the rest of the line, token by token
        std::istringstream got(o.str());
        std::string a, b;
        bool same = true;
        while (s >> a) same = same && (got >> b) && a == b;
        same = same && !(got >> b);
        CHECK(same);
        if (!same && fails <= 20) fprintf(stderr, "  computed: %s\n", o.str().c_str());
    }
    return lines;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s tests/golden/tb_plan_parent.txt\n", argv[0]);
        return 2;
    }
    // the single sweep's blocks
    for (int ni : {2, 129, 1025, 32768})
        for (int nj : {2, 17, 32768})
            for (int waves : {4, 8, 16}) {
                snprintf(ctx, sizeof ctx, "sweep %d x %d, %d waves", ni, nj, waves);
                const int h = pick_rows_per_block(ni, nj, waves);
                int nbx = 0, nby = 0;
                CHECK(h >= 4 && h <= 16);
                CHECK(sweep_partials(ni, nj, h, waves, &nbx, &nby) == nbx * nby);
                CHECK((long long)nbx * waves * kStripCells >= ni &&
                      (long long)(nbx - 1) * waves * kStripCells < ni);
                CHECK(nby * h >= nj && (nby - 1) * h < nj);
            }
    sweep();
    const int lines = check_table(argv[1]);
    snprintf(ctx, sizeof ctx, "table of %d lines", lines);
    CHECK(lines >= 40);
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("%lld geometries, %lld lists, %d table lines: all checks passed\n", n_geom, n_lists,
           lines);
    return 0;
}
