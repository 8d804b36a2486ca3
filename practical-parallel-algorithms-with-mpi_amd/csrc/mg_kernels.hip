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

}  // namespace

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
