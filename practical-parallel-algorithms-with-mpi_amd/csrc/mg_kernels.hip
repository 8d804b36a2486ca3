// mg_kernels.hip -- the two inter-grid transfer kernels of the multigrid
// cycle (misor_mg.hip, DESIGN.md "Geometric multigrid"): cell-centred
// coarsening by two, fine cells (2I-1 .. 2I, 2J-1 .. 2J) under coarse cell
// (I, J), both grids in the padded pitch layout of misor_internal.h.
//
// Both stream HBM once.  A thread owns one coarse column, i.e. the aligned
// pair of fine columns (2I-1, 2I): fine column 1 lies on a 128-byte boundary
// (kXOff), so every pair is one 16-byte access and a wave's 64 pairs are 1 KiB
// of one row.  A workgroup of kMgTileW threads marches kMgTileH coarse rows
// (2 kMgTileH fine rows) upwards.  The x-neighbours of a pair (fine columns
// 2I-2 and 2I+1, coarse columns I-1 and I+1) are the neighbouring lanes' own
// cells: they are loaded again and served by the vector L1, not by HBM.
//
// Compiled with -ffp-contract=off like the sweep kernels: the residual is
// solveRB's expression (assignment-4/src/solver.c:204-210) term for term and
// the composed numpy oracle of tests/test_mg_gpu.py matches bit for bit.

#include "misor_internal.h"
#include "mg_transfer.h"

namespace misor {

namespace {

__device__ __forceinline__ double2 ld2(const double* p) {
    return *reinterpret_cast<const double2*>(p);
}
__device__ __forceinline__ void st2(double* p, double a, double b) {
    *reinterpret_cast<double2*>(p) = make_double2(a, b);
}

// rc(I,J) = 0.25 ((r(2I-1,2J-1) + r(2I,2J-1)) + (r(2I-1,2J) + r(2I,2J))),
// r = rhs - lap p; the expressions are mg_transfer.h's, shared with the
// LDS-resident cycle of mg_tail.hip.  The four residuals live in registers
// only.  Per fine row
// a thread loads its pair of p (16 B), the two x-neighbours (8 B each, L1)
// and its pair of rhs; a fine row of p is loaded once and kept while the
// march needs it (south of, in, north of the row pair), so a workgroup reads
// 2 kMgTileH + 2 rows of p for 2 kMgTileH rows of residuals.
__global__ __launch_bounds__(kMgTileW) void mg_residual_restrict_kernel(
    const double* __restrict__ p, const double* __restrict__ rhs, double* __restrict__ rc,
    int nic, int njc, long long pitch, long long pitch_c, double idx2, double idy2) {
    const int I = blockIdx.x * kMgTileW + threadIdx.x + 1;
    if (I > nic) return;
    const int J0 = blockIdx.y * kMgTileH + 1;
    const int J1 = min(J0 + kMgTileH - 1, njc);
    // cell (2I-1, j) of a fine field: row j starts at (j + kYOff) * pitch
    const long long col = (long long)(2 * I - 1) + kXOff;
    auto row = [&](int j) { return (long long)(j + kYOff) * pitch + col; };

    // rows 2J-2 (south of the pair) and 2J-1 of the first coarse row
    const double2 s0 = ld2(p + row(2 * J0 - 2));
    double2 a = ld2(p + row(2 * J0 - 1));
    double aw = p[row(2 * J0 - 1) - 1], ae = p[row(2 * J0 - 1) + 2];
    double sx = s0.x, sy = s0.y;  // the row below a
    for (int J = J0; J <= J1; ++J) {
        const long long rb = row(2 * J), rn = row(2 * J + 1);
        const double2 b = ld2(p + rb);  // row 2J
        const double bw = p[rb - 1], be = p[rb + 2];
        const double2 n = ld2(p + rn);  // row 2J+1: north of the pair, first row of the next
        const double2 fa = ld2(rhs + row(2 * J - 1));
        const double2 fb = ld2(rhs + rb);
        const double r00 = mg_resid(fa.x, a.x, aw, a.y, sx, b.x, idx2, idy2);
        const double r10 = mg_resid(fa.y, a.y, a.x, ae, sy, b.y, idx2, idy2);
        const double r01 = mg_resid(fb.x, b.x, bw, b.y, a.x, n.x, idx2, idy2);
        const double r11 = mg_resid(fb.y, b.y, b.x, be, a.y, n.y, idx2, idy2);
        rc[(long long)(J + kYOff) * pitch_c + I + kXOff] = mg_restrict4(r00, r10, r01, r11);
        if (J < J1) {
            sx = b.x;
            sy = b.y;
            a = n;
            aw = p[rn - 1];
            ae = p[rn + 2];
        }
    }
}

// p(i,j) += (9 e(I,J) + 3 (e(I+sx,J) + e(I,J+sy)) + e(I+sx,J+sy)) * 0.0625 with
// (I,J) the parent of (i,j), sx = -1 / +1 for odd / even i (sy likewise) and
// neighbour indices clamped to the coarse interior (the Neumann mirror: no
// coarse ghost is read); then solveRB's ghost copy of p, written by the
// threads that own the edge cells.  A thread keeps a 3 x 3 window of e
// (columns I-1 .. I+1 of three coarse rows) and shifts it up the march.
__global__ __launch_bounds__(kMgTileW) void mg_prolong_correct_kernel(
    double* __restrict__ p, const double* __restrict__ e, int nic, int njc, long long pitch,
    long long pitch_c) {
    const int I = blockIdx.x * kMgTileW + threadIdx.x + 1;
    if (I > nic) return;
    const int J0 = blockIdx.y * kMgTileH + 1;
    const int J1 = min(J0 + kMgTileH - 1, njc);
    const int Iw = max(I - 1, 1), Ie = min(I + 1, nic);
    const long long col = (long long)(2 * I - 1) + kXOff;
    auto row = [&](int j) { return (long long)(j + kYOff) * pitch + col; };
    auto crow = [&](int J) { return (long long)(J + kYOff) * pitch_c + kXOff; };
    const int nj = 2 * njc;

    long long c = crow(max(J0 - 1, 1));
    double sw = e[c + Iw], sc = e[c + I], se = e[c + Ie];  // coarse row J-1 (clamped)
    c = crow(J0);
    double mw = e[c + Iw], mc = e[c + I], me = e[c + Ie];  // coarse row J
    for (int J = J0; J <= J1; ++J) {
        c = crow(min(J + 1, njc));
        const double nw = e[c + Iw], nc = e[c + I], ne = e[c + Ie];  // coarse row J+1 (clamped)
        const long long ra = row(2 * J - 1), rb = row(2 * J);
        const double2 a = ld2(p + ra), b = ld2(p + rb);
        // row 2J-1 (sy = -1): columns 2I-1 (sx = -1) and 2I (sx = +1); row 2J (sy = +1)
        const double a0 = a.x + mg_interp(mc, mw, sc, sw);
        const double a1 = a.y + mg_interp(mc, me, sc, se);
        const double b0 = b.x + mg_interp(mc, mw, nc, nw);
        const double b1 = b.y + mg_interp(mc, me, nc, ne);
        st2(p + ra, a0, a1);
        st2(p + rb, b0, b1);
        // the ghost copy (solver.c:218-226): columns 0 and ni + 1, rows 0 and nj + 1
        if (I == 1) {
            p[ra - 1] = a0;
            p[rb - 1] = b0;
        }
        if (I == nic) {  // column ni + 1 = 2I + 1
            p[ra + 2] = a1;
            p[rb + 2] = b1;
        }
        if (J == 1) st2(p + row(0), a0, a1);
        if (J == njc) st2(p + row(nj + 1), b0, b1);
        sw = mw, sc = mc, se = me;
        mw = nw, mc = nc, me = ne;
    }
}

// The same correction on one rank's block of a decomposed level
// (misor_solve_mg_dist): p is the block, e the coarse array seen from the
// block -- e + e_off is its cell (0, 0), which is the coarse block's own array
// (e_off 0, its halo exchanged 1 deep, corners included) or the block's window
// of a whole-domain level.  phys has bit 0 / 1 / 2 / 3 set where the block's
// left / right / bottom / top side is the domain's: there the neighbour index
// is clamped as above and the side's ghost copy of p is written; on a side
// that borders another rank the coarse halo cell is read and no ghost is
// written (the neighbour owns that cell of p).  e_off 0 with phys 15 is
// mg_prolong_correct_kernel, expression for expression.
__global__ __launch_bounds__(kMgTileW) void mg_prolong_correct_dist_kernel(
    double* __restrict__ p, const double* __restrict__ e, long long e_off, int phys, int nic,
    int njc, long long pitch, long long pitch_c) {
    const int I = blockIdx.x * kMgTileW + threadIdx.x + 1;
    if (I > nic) return;
    const int J0 = blockIdx.y * kMgTileH + 1;
    const int J1 = min(J0 + kMgTileH - 1, njc);
    const bool pl = phys & 1, pr = phys & 2, pb = phys & 4, pt = phys & 8;
    const int Iw = (pl && I == 1) ? 1 : I - 1, Ie = (pr && I == nic) ? nic : I + 1;
    const long long col = (long long)(2 * I - 1) + kXOff;
    auto row = [&](int j) { return (long long)(j + kYOff) * pitch + col; };
    auto crow = [&](int J) { return e_off + (long long)(J + kYOff) * pitch_c + kXOff; };
    const int nj = 2 * njc;

    long long c = crow((pb && J0 == 1) ? 1 : J0 - 1);
    double sw = e[c + Iw], sc = e[c + I], se = e[c + Ie];  // coarse row J-1
    c = crow(J0);
    double mw = e[c + Iw], mc = e[c + I], me = e[c + Ie];  // coarse row J
    for (int J = J0; J <= J1; ++J) {
        c = crow((pt && J == njc) ? njc : J + 1);
        const double nw = e[c + Iw], nc = e[c + I], ne = e[c + Ie];  // coarse row J+1
        const long long ra = row(2 * J - 1), rb = row(2 * J);
        const double2 a = ld2(p + ra), b = ld2(p + rb);
        const double a0 = a.x + mg_interp(mc, mw, sc, sw);
        const double a1 = a.y + mg_interp(mc, me, sc, se);
        const double b0 = b.x + mg_interp(mc, mw, nc, nw);
        const double b1 = b.y + mg_interp(mc, me, nc, ne);
        st2(p + ra, a0, a1);
        st2(p + rb, b0, b1);
        if (pl && I == 1) {
            p[ra - 1] = a0;
            p[rb - 1] = b0;
        }
        if (pr && I == nic) {
            p[ra + 2] = a1;
            p[rb + 2] = b1;
        }
        if (pb && J == 1) st2(p + row(0), a0, a1);
        if (pt && J == njc) st2(p + row(nj + 1), b0, b1);
        sw = mw, sc = mc, se = me;
        mw = nw, mc = nc, me = ne;
    }
}

// The hand-over of a decomposed hierarchy to its whole-domain levels
// (misor_comm.hip allgather_blocks): the equal bw x bh blocks of the ranks of
// a process grid with dims1 ranks along y, block q = (q / dims1, q % dims1)
// covering cells (cx bw + 1 .., cy bh + 1 ..) of the padded whole-domain field,
// and buf, which holds blocks packed row by row.  PACK copies block q0 of the
// field to the start of buf; otherwise blocks q0 .. q0 + nq - 1 of buf (block
// q at q bw bh) go to the field, except block skip.  V doubles per access:
// with bw even every row segment starts on a 16-byte boundary in both.
template <int V, bool PACK>
__global__ void mg_block_copy_kernel(double* field, long long pitch, double* buf, int bw, int bh,
                                     int dims1, int q0, int nq, int skip) {
    const int rw = bw / V;  // accesses per block row
    const long long per = (long long)rw * bh;
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= per * nq) return;
    const int q = q0 + (int)(k / per);
    if (!PACK && q == skip) return;
    const long long r = k % per;
    const int j = (int)(r / rw), i = (int)(r % rw) * V;
    double* cell = field + (long long)((q % dims1) * bh + j + 1 + kYOff) * pitch +
                   ((q / dims1) * bw + i + 1 + kXOff);
    double* slot = buf + (PACK ? 0 : (long long)q * bw * bh) + (long long)j * bw + i;
    if (V == 2) {
        if (PACK)
            *reinterpret_cast<double2*>(slot) = *reinterpret_cast<const double2*>(cell);
        else
            *reinterpret_cast<double2*>(cell) = *reinterpret_cast<const double2*>(slot);
    } else {
        if (PACK)
            *slot = *cell;
        else
            *cell = *slot;
    }
}

template <bool PACK>
void launch_block_copy(hipStream_t s, double* field, long long pitch, double* buf, int bw, int bh,
                       int dims1, int q0, int nq, int skip) {
    const int V = (bw & 1) ? 1 : 2;
    const long long n = (long long)(bw / V) * bh * nq;
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (V == 2)
        hipLaunchKernelGGL((mg_block_copy_kernel<2, PACK>), grid, dim3(256), 0, s, field, pitch,
                           buf, bw, bh, dims1, q0, nq, skip);
    else
        hipLaunchKernelGGL((mg_block_copy_kernel<1, PACK>), grid, dim3(256), 0, s, field, pitch,
                           buf, bw, bh, dims1, q0, nq, skip);
}

}  // namespace

void launch_mg_prolong_correct_dist(hipStream_t s, double* p, const double* e, long long e_off,
                                    int phys, int nic, int njc, long long pitch,
                                    long long pitch_c) {
    const dim3 grid((nic + kMgTileW - 1) / kMgTileW, (njc + kMgTileH - 1) / kMgTileH);
    hipLaunchKernelGGL(mg_prolong_correct_dist_kernel, grid, dim3(kMgTileW), 0, s, p, e, e_off,
                       phys, nic, njc, pitch, pitch_c);
}

void launch_mg_block_pack(hipStream_t s, const double* field, long long pitch, double* buf, int bw,
                          int bh, int dims1, int q) {
    launch_block_copy<true>(s, const_cast<double*>(field), pitch, buf, bw, bh, dims1, q, 1, -1);
}

void launch_mg_block_scatter(hipStream_t s, double* field, long long pitch, const double* buf,
                             int bw, int bh, int dims1, int nblocks, int skip) {
    launch_block_copy<false>(s, field, pitch, const_cast<double*>(buf), bw, bh, dims1, 0, nblocks,
                             skip);
}

void launch_mg_residual_restrict(hipStream_t s, const double* p, const double* rhs, double* rc,
                                 int nic, int njc, long long pitch, long long pitch_c,
                                 double idx2, double idy2) {
    const dim3 grid((nic + kMgTileW - 1) / kMgTileW, (njc + kMgTileH - 1) / kMgTileH);
    hipLaunchKernelGGL(mg_residual_restrict_kernel, grid, dim3(kMgTileW), 0, s, p, rhs, rc, nic,
                       njc, pitch, pitch_c, idx2, idy2);
}

void launch_mg_prolong_correct(hipStream_t s, double* p, const double* e, int nic, int njc,
                               long long pitch, long long pitch_c) {
    const dim3 grid((nic + kMgTileW - 1) / kMgTileW, (njc + kMgTileH - 1) / kMgTileH);
    hipLaunchKernelGGL(mg_prolong_correct_kernel, grid, dim3(kMgTileW), 0, s, p, e, nic, njc,
                       pitch, pitch_c);
}

}  // namespace misor
