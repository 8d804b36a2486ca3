// misor_internal.h -- device layout, grid state and kernel launchers shared by
// the libmisor translation units.  Not part of the public ABI (include/misor.h).
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <string>

#include "decomp2.h"  // HaloPlan
#include "misor.h"
#include "tb_plan.h"  // kMaxT, kStripCells, SweepParams, the launch plans

namespace misor {

// ---------------------------------------------------------------------------
// HBM layout of every field (p, p', rhs, u, v, f, g)
//
// Reference cell (i,j), i in [0, ni+1], j in [0, nj+1] (ghosts included), lives
// at   base[(j + kYOff) * pitch + (i + kXOff)].
//  - kXOff = 15 puts the first interior column i = 1 on a 128-byte boundary,
//    so every wave's 16-byte-per-lane row segment of 128 cells starts a cache
//    line; the ghost column i = 0 is the last double of the preceding line.
//  - kYOff = 2 * kMaxT + 16 rows below row 0 and as many (+ prefetch run-out)
//    above row nj+1: a block of the temporally blocked sweep streams rows
//    j0-2T-1 .. j1-1+2T (+ rows in flight; the split-ring march up to 14
//    more warm-up rows below, sor_tbh.h) without clamping, and its first
//    strip's columns from 1 - 2T (the tail of the row below, in the
//    allocation: a left halo of depth 2 kMaxT too).
//  - pitch = 160 + round_up(ni, kStripCells * kMaxWavesX): left pad line, the
//    strips, the run-out of the last (overlapping) strip and pad; a multiple
//    of 16 doubles (128 B) that is not a power of two.
// Padding cells are zero and never feed an interior result.
// ---------------------------------------------------------------------------
constexpr int kXOff = 15;
constexpr int kYOff = 2 * kMaxT + 16;
constexpr int kMaxWavesX = 16;             // strips per sweep workgroup (max)
constexpr int kMaxAhead = 3;               // rows a sweep keeps in flight (max)

inline long long layout_pitch(int ni) {
    const int w = kStripCells * kMaxWavesX;
    return 160 + (long long)((ni + w - 1) / w) * w;
}
// rows j = -kYOff .. nj + 2*kMaxT + kMaxAhead + 1 (a temporally blocked block
// streams 2T rows past its last row, plus the rows it keeps in flight)
inline long long layout_rows(int nj) { return (long long)nj + 2 * kYOff + kMaxAhead + 3; }

// sweep kernel variants: strips per workgroup, rows in flight, nt stores
struct SweepVariant {
    int waves, ahead, nt_store, nt_load;
};
constexpr SweepVariant kSweepVariants[] = {
    {4, 1, 0, 0}, {4, 2, 0, 0}, {4, 3, 0, 0}, {4, 1, 1, 0}, {4, 2, 1, 0},
    {8, 1, 0, 0}, {8, 2, 0, 0}, {8, 2, 1, 0}, {8, 1, 1, 0}, {8, 3, 1, 0},
    {16, 1, 1, 0}, {16, 2, 1, 0}, {4, 3, 1, 0}, {8, 2, 1, 1}, {16, 2, 1, 1}};
constexpr int kNumSweepVariants = 15;
constexpr int kDefaultSweepVariant = 7;  // 8 strips, 2 rows ahead, nt stores (tools/tune_sweep.py)
int sweep_waves(int variant);

// workgroups of a persistent pass resident on the device at once: the
// occupancy query behind tb_plan.h TbResidency (sor_tb.hip)
int tb_resident(int T, int variant);

// Solver state that lives on the device between launches.  Written only by
// the finish kernel (one workgroup) and read by the next sweep launch.
struct DevState {
    int it;        // iterations completed
    int done;      // 1 once (res >= eps^2 && it < itermax) is false
    int itermax;   // cap of the current solve call
    int near;      // 1: stopped before iteration it+1, whose res fell within nband of
                   // eps^2 (misor_solve.hip exact_tail recomputes from there)
    int lite_miss; // 1: stopped before iteration it+1, whose residual lower bound (a
                   // lite pass, SweepParams::lite) did not prove the loop goes on
    double res;    // residual of the last iteration
    double epssq;
    double nband = -1.0;  // |res - eps^2| <= nband: near the threshold (< 0: off, the
                          // default of every DevState the host builds)
    double sum[kMaxT];  // sum r^2 of each iteration of the last pass (this rank,
                        // then all-reduced)
};

// zero the head, copy the initial list, empty the dynamic slots
void launch_chain_init(hipStream_t s, int* work, const unsigned long long* tmpl, int nseg0,
                       int cap);

struct NsParams {
    double dx, dy, dt;
    double xlength, ylength;
    double re, gx, gy, gamma;
    int bc_left, bc_right, bc_bottom, bc_top, problem;
};

// kernel launchers (sor_kernels.hip, ns_kernels.hip)
void launch_sweep(hipStream_t s, const SweepParams& prm, const double* src, double* dst,
                  const double* rhs, double* partials, const DevState* st);
// the same sweep (default variant's geometry) storing r^2 of every counted cell into rsq
void launch_sweep_rsq(hipStream_t s, const SweepParams& prm, const double* src, double* dst,
                      const double* rhs, double* partials, const DevState* st, double* rsq);
// T iterations per pass: partials[t * nparts + block]
void launch_finish(hipStream_t s, const double* partials, int nparts, int T, DevState* st,
                   double cells, int decide);
void launch_decide(hipStream_t s, DevState* st, int T, double cells, int lite = 0);
// single-rank loop test in two levels (chunk sums, then the finish kernel over
// kFinishChunks values per stage); scratch holds kMaxT * kFinishChunks doubles
constexpr int kFinishChunks = 32;
// count: a zeroed device int -- the partial-sum launch's last workgroup then
// runs the loop test itself (one launch); nullptr: a second, finish launch.
// decide 0: only the sums into st->sum (decomposed: all-reduce, then decide)
void launch_finish2(hipStream_t s, const double* partials, int nparts, int T, DevState* st,
                    double cells, double* scratch, int* count, int decide, int lite = 0);
// queue: 8 device ints (zeroed by the launch) for a persistent launch whose
// workgroups take blocks from per-XCD queues; nullptr: one workgroup per block
void launch_tb(hipStream_t s, int T, const SweepParams& prm, const double* src, double* dst,
               const double* rhs, double* partials, const DevState* st, int force, int* queue);
// the same for one T (sor_tb_inst.hip, one unit per T)
#define MISOR_DECL_TB(N)                                                                      \
    void launch_tb_t##N(hipStream_t s, const SweepParams& prm, const double* src, double* dst, \
                        const double* rhs, double* partials, const DevState* st, int force,   \
                        int* queue);                                                          \
    int tb_resident_t##N(int variant);
MISOR_DECL_TB(1) MISOR_DECL_TB(2) MISOR_DECL_TB(3) MISOR_DECL_TB(4) MISOR_DECL_TB(5)
MISOR_DECL_TB(6) MISOR_DECL_TB(7) MISOR_DECL_TB(8) MISOR_DECL_TB(9) MISOR_DECL_TB(10)
#undef MISOR_DECL_TB
// lexicographic Gauss-Seidel SOR, whole solve in one workgroup (lex_kernels.hip)
void launch_solve_lex(hipStream_t s, double* p, const double* rhs, int ni, int nj,
                      long long pitch, double idx2, double idy2, double factor, double cells,
                      int xorder, DevState* st);
// what it keeps in LDS: 2 = p and rhs, 1 = p, 0 = nothing (p walked in HBM)
int lex_use_lds(int ni, int nj);
// the same solve as a tiled wavefront over the whole device (lex_tiled.hip):
// tiles of tw x th cells, a persistent grid of at most wgs_cap workgroups
// (<= 0: automatic); wk: its work area, kept by the grid between solves
constexpr int kLexMinTile = 8;
// default tile: 96 x 96 (runner-up 32 x 32; profiles/lex_tiled_ab.txt)
constexpr int kLexTileW = 96, kLexTileH = 96;
// automatic rule: tiled from this many interior cells on.  Measured against
// the one-workgroup kernel (profiles/lex_tiled_ab.txt): 512^2 1.6-1.7x, 1024^2
// 3.0-3.3x, 4096^2 14-16x faster, 256^2 0.8x (slower) -- so from the smallest
// size measured faster, 512^2; below it the one-workgroup kernel stays
constexpr long long kLexTiledCells = 512LL * 512;
struct LexTiledWork {
    void* buf = nullptr;
    size_t bytes = 0;
    int ntx = 0, nty = 0;  // the tile grid its order table lists
};
bool lex_tile_fits(int tw, int th);
hipError_t launch_solve_lex_tiled(hipStream_t s, double* p, const double* rhs, int ni, int nj,
                                  long long pitch, double idx2, double idy2, double factor,
                                  double cells, int xorder, DevState* st, int tw, int th,
                                  int wgs_cap, LexTiledWork& wk);
// whole-solve single-workgroup kernel for grids whose p fits in LDS
int small_solve_fits(int ni, int nj);
void launch_solve_small(hipStream_t s, double* p, const double* rhs, int ni, int nj,
                        long long pitch, double idx2, double idy2, double coef, double cells,
                        DevState* st);
// the same solve for a batch of problems of one shape, one workgroup each
// (sor_kernels.hip rb_solve_batch_kernel): what differs between the members
struct BatchMember {
    double coef;  // omega is per member
    DevState st;  // loop state in, it / res / near out
};
void launch_solve_batch(hipStream_t s, double* p_base, const double* rhs_base,
                        long long member_stride, int nbatch, int ni, int nj, long long pitch,
                        double idx2, double idy2, double cells, BatchMember* members);

// multigrid transfers (mg_kernels.hip) between a fine grid and its coarse grid
// of nic x njc cells (the fine grid has 2 nic x 2 njc): a workgroup covers
// kMgTileW coarse columns x kMgTileH coarse rows, i.e. a fine tile of
// 2 kMgTileW x 2 kMgTileH cells
constexpr int kMgTileW = 256;
constexpr int kMgTileH = 16;
// rc = restriction of rhs - lap p (the residual in registers only)
void launch_mg_residual_restrict(hipStream_t s, const double* p, const double* rhs, double* rc,
                                 int nic, int njc, long long pitch, long long pitch_c,
                                 double idx2, double idy2);
// p += bilinear interpolation of e, then p's ghost copy
void launch_mg_prolong_correct(hipStream_t s, double* p, const double* e, int nic, int njc,
                               long long pitch, long long pitch_c);
// the same on a rank's block of a decomposed level: e + e_off is cell (0, 0) of
// the coarse array as the block sees it, phys the mask of the block's physical
// sides (bit 0 left, 1 right, 2 bottom, 3 top); a side that borders another
// rank reads the coarse halo cell and writes no ghost
void launch_mg_prolong_correct_dist(hipStream_t s, double* p, const double* e, long long e_off,
                                    int phys, int nic, int njc, long long pitch,
                                    long long pitch_c);
// equal bw x bh blocks of a process grid (dims1 ranks along y) and a padded
// whole-domain field: block q of the field packed into buf; blocks 0 ..
// nblocks - 1 of buf (block q at q bw bh) into the field, except block skip
void launch_mg_block_pack(hipStream_t s, const double* field, long long pitch, double* buf, int bw,
                          int bh, int dims1, int q);
void launch_mg_block_scatter(hipStream_t s, double* field, long long pitch, const double* buf,
                             int bw, int bh, int dims1, int nblocks, int skip);

// The tail of a hierarchy -- its trailing levels that each fit the LDS of one
// workgroup (small_solve_fits) -- cycled in ONE launch of one workgroup
// (mg_tail.hip).  One entry per tail level, finest first:
struct MgTailLevel {
    double* p;          // the level's current pressure buffer (levels below the first: e)
    double* rhs;        // its rhs (levels below the first: rc, written by the kernel)
    int ni, nj;
    long long pitch;
    double idx2, idy2, cells;
    double coef_smooth, coef_coarse;  // sor_consts(...).coef for omega_smooth / omega_coarse
};
// ... and the launch's state.  The kernel reads the first group and writes the
// second.  It runs cycles while res >= epssq and fewer than maxcycles are done,
// from cycles0 done with residual res0 (a tail below level 0 runs one cycle:
// cycles0 0, res0 1, epssq 0, maxcycles 1).
struct MgTailState {
    int nu1, nu2, maxcycles, cycles0, itermax_coarse;
    double epssq, res0;
    double epssq_coarse, nband_coarse;  // the coarsest solve's eps^2 and its near band (< 0: none)
    int cycles;       // cycles completed
    int near;         // 1: stopped inside cycle `cycles` + 1, before an iteration of its
                      // coarsest solve whose res fell within nband_coarse of epssq_coarse: the
                      // down half of that cycle is done (every level's p and rhs stored), the
                      // coarsest e is zero; the host finishes the cycle (misor_mg.hip)
    double res;       // the first tail level's residual after the last completed cycle
    double res_part;  // ... and as far as the cycle stopped in got (its pre-smoothing)
};
size_t mg_tail_lds(int ni, int nj);  // of a tail whose first level is ni x nj
hipError_t mg_tail_prepare();        // once per device before the first launch
void launch_mg_tail(hipStream_t s, const MgTailLevel* levels, int count, MgTailState* st,
                    size_t lds);

// 8-neighbour halo exchange of one field (halo.hip) by a plan of decomp2.h
static_assert(kMaxHaloDepth == 2 * kMaxT + 1, "decomp2.h: the deepest halo plan");
void launch_pack(hipStream_t s, const double* field, long long pitch, const HaloPlan& plan,
                 double* sendbuf);
void launch_unpack(hipStream_t s, double* field, long long pitch, const HaloPlan& plan,
                   const double* recvbuf);
// in-process transport: out[k] = combination (sum / max, rank order) of
// gather[q * kMaxT + k] over q < nranks, k < n
void launch_local_combine(hipStream_t s, const double* gather, int nranks, int n, int is_max,
                          double* out);

void launch_fill(hipStream_t s, double* a, long long count, double v);
// the message misor_last_error() returns (thread-local, shared by the 2D and 3D ABI)
void set_last_error(const char* msg);
void launch_poisson_init(hipStream_t s, double* p, double* rhs, const double* sx,
                         const double* sy, const double* rx, int ni, int nj,
                         long long pitch, int problem);

struct NsLaunch {
    hipStream_t s;
    long long pitch;
    int ni, nj;
    NsParams prm;
    // physical-boundary flags (multi-GPU: only edge ranks apply wall BCs)
    int wall_left, wall_right, wall_bottom, wall_top;
    int ioff, joff;          // global index of local cell (0,0)
    int imax_g, jmax_g;      // global interior size
};
void launch_set_bc(const NsLaunch& L, double* u, double* v);
void launch_special_bc(const NsLaunch& L, double* u);
void launch_compute_fg(const NsLaunch& L, const double* u, const double* v, double* f,
                       double* g);
void launch_compute_rhs(const NsLaunch& L, const double* f, const double* g, double* rhs);
// computeFG + computeRHS in one column march (RHS of column 1 / row 1 next to a
// neighbour rank left to launch_rhs_edges after the f, g exchange)
void launch_compute_fg_rhs(const NsLaunch& L, const double* u, const double* v, double* f,
                           double* g, double* rhs);
void launch_rhs_edges(const NsLaunch& L, const double* f, const double* g, double* rhs);
void launch_adapt_uv(const NsLaunch& L, const double* f, const double* g, const double* p,
                     double* u, double* v);
// reductions over ALL (ni+2)(nj+2) cells: partial per block, then a finish
int reduce_blocks(int ni, int nj);
void launch_absmax2(const NsLaunch& L, const double* u, const double* v, double* partials);
// adaptUV + the partials of launch_absmax2 over the fields it leaves
void launch_adapt_absmax(const NsLaunch& L, const double* f, const double* g, const double* p,
                         double* u, double* v, double* partials);
// normalizePressure's sum, exact (order- and decomposition-independent):
// fixed-point terms at 2^(E - kSumFrac), E = exponent of the global max |p|;
// limbs[0..2] = the local sum as three 44-bit integer limbs (doubles, summed
// exactly by an all-reduce); exact_sum_value rounds the total once (host)
constexpr int kSumFrac = 72;
void launch_exact_sum(const NsLaunch& L, const double* p, int E, double* partials,
                      double* limbs);
double exact_sum_value(const double limbs[3], int E);
void launch_finish_reduce(hipStream_t s, const double* partials, int n, int op, int width,
                          double* out);
// p -= avg over the whole local array (normalizePressure)
void launch_sub_mean(const NsLaunch& L, double* p, double avg);
enum { kReduceSum = 0, kReduceMax = 1 };

// ---------------------------------------------------------------------------
// 3D (assignment-6): dense reference layout (imax+2)(jmax+2)(kmax+2), i fastest
// ---------------------------------------------------------------------------
struct G3 {
    int I, J, K;        // interior cells (K: this rank's planes)
    long long sx, sxy;  // strides of j and k: (I+2), (I+2)(J+2)
    int Kg = 0, koff = 0;            // global planes; global k of local plane 0
    int lo_phys = 1, hi_phys = 1;    // local planes 1 / K border the physical boundary
    // Cartesian blocks (misor3_create_cart): I, J are the block's cells too.
    // The defaults are those of a slab / single domain, which spans x and y.
    int ioff = 0, joff = 0;          // global i, j of local cell 0
    int Ig = 0, Jg = 0;              // global cells along x, y (0: I, J)
    int xlo_phys = 1, xhi_phys = 1;  // local columns 1 / I border the physical boundary
    int ylo_phys = 1, yhi_phys = 1;  // local rows 1 / J
    __host__ __device__ long long ix(int i, int j, int k) const {
        return (long long)k * sxy + (long long)j * sx + i;
    }
};
struct Fg3 {  // computeFG's scalars (solver.c:620-629)
    double gamma, ix, iy, iz, iRe, dt, gx, gy, gz;
};
int ns3_partials(const G3& g);
void launch3_rhs(hipStream_t s, const G3& g, const double* f, const double* gg, const double* h,
                 double* rhs, double idx, double idy, double idz, double idt);
// one solve iteration: two colour-pass launches (the ghost copy fused in) and
// the loop test; returns the number of partials per pass
int launch3_rb_iteration(hipStream_t s, const G3& g, double* p, const double* rhs, double idx2,
                         double idy2, double idz2, double factor, double* partials, DevState* st,
                         double cells);
// Cartesian blocks: the same iteration in pieces, because an exchange of p
// goes before each colour pass -- pass 0 / 1 with its partials in
// partials[pass * nb ..] (returns nb), then the block's sum of r^2 of both
// passes into st->sum[0] (all-reduce, launch3_decide)
int launch3_rb_pass(hipStream_t s, const G3& g, double* p, const double* rhs, int pass,
                    double idx2, double idy2, double idz2, double factor, double* partials,
                    const DevState* st);
void launch3_rb_sum(hipStream_t s, const G3& g, const double* partials, DevState* st,
                    double cells);
// a box of cells of a field in the reference layout (halo3.hip): nx x ny x nz
// cells from (x0, y0, z0), strides sx / sxy; packed x fastest
struct Box3 {
    int x0, y0, z0, nx, ny, nz;
    long long sx, sxy;
    long long cells() const { return (long long)nx * ny * nz; }
};
void launch3_box_pack(hipStream_t s, const double* field, const Box3& b, double* buf);
void launch3_box_unpack(hipStream_t s, double* field, const Box3& b, const double* buf);
// launch3_absmax over a box instead of a run of cells
void launch3_absmax_box(hipStream_t s, const double* u, const double* v, const double* w,
                        const Box3& b, double* partials, double* out);
// one solve iteration as ONE sweep launch (red then black, src -> dst) plus
// the loop test; rows in {4, 8, 12}, kc planes per workgroup
int sweep3_blocks(const G3& g, int rows, int kc);
int launch3_sweep(hipStream_t s, const G3& g, const double* src, double* dst, const double* rhs,
                  double idx2, double idy2, double idz2, double factor, int rows, int kc,
                  double* partials, DevState* st, double cells, bool sum_only = false,
                  bool ra2 = false);
void launch3_fg(hipStream_t s, const G3& g, const double* u, const double* v, const double* w,
                double* f, double* gg, double* h, const Fg3& c);
void launch3_adapt(hipStream_t s, const G3& g, const double* f, const double* gg,
                   const double* h, const double* p, double* u, double* v, double* w, double fx,
                   double fy, double fz);
void launch3_wall(hipStream_t s, const G3& g, double* n, double* t1, double* t2, int axis,
                  int gh, int in, int on, int onin, int bc);
void launch3_special(hipStream_t s, const G3& g, double* u, int problem);
int absmax3_blocks();
void launch3_absmax(hipStream_t s, const double* u, const double* v, const double* w,
                    long long n, double* partials, double* out);
void launch3_normalize(hipStream_t s, const G3& g, double* p, double* partials, double* sum,
                       double cells);
// normalizePressure in two halves around a cross-rank all-reduce of *sum
void launch3_interior_sum(hipStream_t s, const G3& g, const double* p, double* partials,
                          double* sum);
void launch3_sub_mean(hipStream_t s, const G3& g, double* p, const double* sum, double cells);
// the loop test of a decomposed solve: st->sum[0] holds the all-reduced sum
// of r^2 of the iteration (written by launch3_sweep with sum_only)
void launch3_decide(hipStream_t s, DevState* st, double cells);
// single rank, the loop test folded into the sweep: the sweep first applies
// the test of the previous sweep (prev_partials; nullptr: none) to st_in,
// workgroup 0 writes the result to st_out, and the launch is a no-op once the
// loop is over; launch3_fold_decide applies the test of a batch's last sweep
void launch3_sweep_folded(hipStream_t s, const G3& g, const double* src, double* dst,
                          const double* rhs, double idx2, double idy2, double idz2,
                          double factor, int rows, int kc, double* partials,
                          const double* prev_partials, const DevState* st_in, DevState* st_out,
                          double cells, bool ra2 = false);
// the whole solve in one cooperative launch, p resident in LDS
// (ns3d_resident.hip): boxes for this grid (0: not possible here), the size of
// its barrier state, the launch (0 ok, 1 refused -> fall back, < 0 error) and
// whether a barrier wait timed out
int resident3_boxes(const G3& g);
size_t resident3_bar_bytes();
int launch3_resident(hipStream_t s, const G3& g, double* p, const double* rhs, double idx2,
                     double idy2, double idz2, double factor, double cells, double* partials,
                     DevState* st, void* bar, double* mbox);
int resident3_aborted(const void* bar, hipStream_t s, int* aborted);
void launch3_fold_decide(hipStream_t s, const G3& g, int rows, int kc,
                         const double* prev_partials, const DevState* st_in, DevState* st_out,
                         double cells);

// 3D multigrid transfers (mg3_kernels.hip) between a fine grid f and its
// coarse grid c (f has 2 c.I x 2 c.J x 2 c.K cells), both single-domain: a
// workgroup covers kMg3TileW coarse columns x kMg3TileH coarse rows and marches
// kMg3TileD coarse planes, i.e. a fine box of twice that each way
constexpr int kMg3TileW = 64;
constexpr int kMg3TileH = 8;
constexpr int kMg3TileD = 8;
// rc = restriction of rhs - lap p (the residual in registers only)
void launch_mg3_residual_restrict(hipStream_t s, const G3& f, const G3& c, const double* p,
                                  const double* rhs, double* rc, double idx2, double idy2,
                                  double idz2);
// p += trilinear interpolation of e, then the ghost copy of p's faces
void launch_mg3_prolong_correct(hipStream_t s, const G3& f, const G3& c, double* p,
                                const double* e);
// the same on a slab of a decomposed grid: c.K coarse planes under the slab's
// f.K = 2 c.K fine planes, local coarse plane 0 at plane koff_c of e (0: e is a
// slab's own array with its exchanged halo; the slab's koff / 2: e is the whole
// domain's array and its neighbouring planes are the real ones); a z side that
// is not physical reads the plane beyond it and gets no ghost plane written
void launch_mg3_prolong_correct_slab(hipStream_t s, const G3& f, const G3& c, double* p,
                                     const double* e, long long koff_c, bool lo_phys,
                                     bool hi_phys);

}  // namespace misor
