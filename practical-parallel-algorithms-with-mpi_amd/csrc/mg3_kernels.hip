// mg3_kernels.hip -- the two inter-grid transfer kernels of the 3D multigrid
// cycle (misor3_mg.hip, DESIGN.md "Geometric multigrid, 3D"): cell-centred
// coarsening by two, fine cells (2I-1 .. 2I, 2J-1 .. 2J, 2K-1 .. 2K) under
// coarse cell (I, J, K), both grids in the dense reference layout of the 3D
// fields (row stride imax + 2, plane stride (imax + 2)(jmax + 2), no padding).
//
// A thread owns one coarse column and row, i.e. the 2 x 2 fine cells of a
// plane under it; a workgroup of kMg3TileW x kMg3TileH threads covers that
// many coarse columns x rows and marches kMg3TileD coarse planes upwards.  A
// wave is one coarse row: its 64 fine pairs (2I-1, 2I) are 1 KiB of one fine
// row.  Rows are not padded, so a pair is 8-byte aligned only: it moves as
// one 16-byte access of 8-byte alignment (Pair below), which the hardware
// takes for global memory.  All offsets are 64-bit.
//
// Compiled with -ffp-contract=off like the sweep kernels: the residual is the
// 3D solve's expression (assignment-6/src/solver.c:205-222) term for term, and
// the composed numpy oracle of tests/test_mg3_gpu.py matches bit for bit.

#include "misor_internal.h"

namespace misor {

namespace {

constexpr int kThreads = kMg3TileW * kMg3TileH;
// the fine tile of one plane with its one-cell rim
constexpr int kFineW = 2 * kMg3TileW + 2, kFineH = 2 * kMg3TileH + 2;
// the coarse tile of one plane with its one-cell rim
constexpr int kCoarseW = kMg3TileW + 2, kCoarseH = kMg3TileH + 2;

struct __attribute__((aligned(8))) Pair {
    double x, y;
};
__device__ __forceinline__ Pair ldp(const double* p) { return *reinterpret_cast<const Pair*>(p); }
__device__ __forceinline__ void stp(double* p, double a, double b) {
    Pair v;
    v.x = a;
    v.y = b;
    *reinterpret_cast<Pair*>(p) = v;
}

// a thread's 2 x 2 cells of one fine plane: a = row 2J-1, b = row 2J
struct Quad {
    Pair a, b;
};

// the 3D solve's residual of one cell
__device__ __forceinline__ double resid3(double rhs, double c, double w, double e, double s,
                                         double n, double d, double u, double idx2, double idy2,
                                         double idz2) {
    const double tx = (e - 2.0 * c) + w;
    const double ty = (n - 2.0 * c) + s;
    const double tz = (u - 2.0 * c) + d;
    return rhs - ((tx * idx2 + ty * idy2) + tz * idz2);
}

// rc(I,J,K) = 0.125 (sum of the eight residuals under the coarse cell, in the
// order of DESIGN.md), r = rhs - lap p.  The march runs over fine planes k:
// a thread keeps its quad of planes k-1, k, k+1 in registers (each loaded
// once), the quads of plane k and the tile's rim lie in LDS for the in-plane
// neighbours (two buffers, one barrier per plane), and the residuals live in
// registers only.  Per plane a workgroup loads its tile of p and of rhs once;
// what it loads again are the rim cells (the neighbouring tiles' own) and one
// plane below and above its chunk.
__global__ __launch_bounds__(kThreads) void mg3_residual_restrict_kernel(
    const double* __restrict__ p, const double* __restrict__ rhs, double* __restrict__ rc, int nic,
    int njc, int nkc, long long sx, long long sxy, long long sxc, long long sxyc, double idx2,
    double idy2, double idz2) {
    __shared__ double tile[2][kFineH][kFineW];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int I = blockIdx.x * kMg3TileW + tx + 1, J = blockIdx.y * kMg3TileH + ty + 1;
    const bool act = I <= nic && J <= njc;
    const int K0 = blockIdx.z * kMg3TileD + 1;
    const int K1 = min(K0 + kMg3TileD - 1, nkc);
    // the tile's last coarse column / row that exists: its thread loads the rim beyond
    const bool xlo = tx == 0, xhi = I == min((int)(blockIdx.x + 1) * kMg3TileW, nic);
    const bool ylo = ty == 0, yhi = J == min((int)(blockIdx.y + 1) * kMg3TileH, njc);
    const long long col = 2LL * I - 1;
    const long long ra = (2LL * J - 1) * sx + col, rb = ra + sx;  // rows 2J-1, 2J of a plane
    const int lx = 2 * tx + 1, ly = 2 * ty + 1;

    auto load = [&](int k) {
        Quad q;
        const double* pk = p + (long long)k * sxy;
        q.a = ldp(pk + ra);
        q.b = ldp(pk + rb);
        return q;
    };
    // the quad of plane k and the rim cells this thread is in charge of into buffer t
    auto stage = [&](int t, int k, const Quad& q) {
        const double* pk = p + (long long)k * sxy;
        tile[t][ly][lx] = q.a.x;
        tile[t][ly][lx + 1] = q.a.y;
        tile[t][ly + 1][lx] = q.b.x;
        tile[t][ly + 1][lx + 1] = q.b.y;
        if (xlo) {
            tile[t][ly][lx - 1] = pk[ra - 1];
            tile[t][ly + 1][lx - 1] = pk[rb - 1];
        }
        if (xhi) {
            tile[t][ly][lx + 2] = pk[ra + 2];
            tile[t][ly + 1][lx + 2] = pk[rb + 2];
        }
        if (ylo) {
            const Pair s = ldp(pk + ra - sx);
            tile[t][ly - 1][lx] = s.x;
            tile[t][ly - 1][lx + 1] = s.y;
        }
        if (yhi) {
            const Pair n = ldp(pk + rb + sx);
            tile[t][ly + 2][lx] = n.x;
            tile[t][ly + 2][lx + 1] = n.y;
        }
    };

    const int k0 = 2 * K0 - 1, k1 = 2 * K1;
    Quad lo{}, mid{}, hi{};
    if (act) {
        lo = load(k0 - 1);
        mid = load(k0);
        stage(k0 & 1, k0, mid);
    }
    double below = 0.0;  // the four residuals of plane 2K-1
    for (int k = k0; k <= k1; ++k) {
        const int t = k & 1;
        Quad fa{};
        if (act) {
            hi = load(k + 1);
            const double* fk = rhs + (long long)k * sxy;
            fa.a = ldp(fk + ra);
            fa.b = ldp(fk + rb);
        }
        __syncthreads();  // plane k is staged; buffer t ^ 1 (plane k-1) is read no more
        if (act) {
            const double w0 = tile[t][ly][lx - 1], e0 = tile[t][ly][lx + 2];
            const double w1 = tile[t][ly + 1][lx - 1], e1 = tile[t][ly + 1][lx + 2];
            const double s0 = tile[t][ly - 1][lx], s1 = tile[t][ly - 1][lx + 1];
            const double n0 = tile[t][ly + 2][lx], n1 = tile[t][ly + 2][lx + 1];
            const double r00 = resid3(fa.a.x, mid.a.x, w0, mid.a.y, s0, mid.b.x, lo.a.x, hi.a.x,
                                      idx2, idy2, idz2);
            const double r10 = resid3(fa.a.y, mid.a.y, mid.a.x, e0, s1, mid.b.y, lo.a.y, hi.a.y,
                                      idx2, idy2, idz2);
            const double r01 = resid3(fa.b.x, mid.b.x, w1, mid.b.y, mid.a.x, n0, lo.b.x, hi.b.x,
                                      idx2, idy2, idz2);
            const double r11 = resid3(fa.b.y, mid.b.y, mid.b.x, e1, mid.a.y, n1, lo.b.y, hi.b.y,
                                      idx2, idy2, idz2);
            const double sum = (r00 + r10) + (r01 + r11);
            if (k & 1) {
                below = sum;
            } else {
                rc[(long long)(k / 2) * sxyc + (long long)J * sxc + I] = 0.125 * (below + sum);
            }
            lo = mid;
            mid = hi;
            if (k < k1) stage(t ^ 1, k + 1, mid);
        }
    }
}

// p += the trilinear interpolation of e (weights 27, 9, 3, 1 over
// 64, parent (I,J,K) of fine cell (i,j,k), s = -1 / +1 for an odd / even index
// per axis, neighbour indices clamped to the coarse interior -- the Neumann
// mirror, no coarse ghost is read); then the ghost copy of p's faces, written
// by the threads that own the face cells.  A thread keeps a 3 x 3 x 3 window
// of e in registers and shifts it up the march; a coarse plane of the tile
// with its (clamped) rim passes through LDS once, loaded by the whole
// workgroup.
//
// A slab of a decomposed grid (misor3_mg_dist.hip): lo_phys / hi_phys say
// which z sides of the nkc coarse planes are physical.  On a physical side K is
// clamped to the interior and the face ghost plane is written, as on a single
// domain; on a side that faces a rank the coarse halo plane 0 / nkc + 1 is read
// (x and y still clamped: no ghost column or row of it is read) and no ghost
// plane is written.  With both flags set every expression is the single
// domain's.
__device__ __forceinline__ void mg3_prolong_correct_body(
    double* __restrict__ p, const double* __restrict__ e, int nic, int njc, int nkc, long long sx,
    long long sxy, long long sxc, long long sxyc, bool lo_phys, bool hi_phys) {
    __shared__ double tile[kCoarseH][kCoarseW];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int tid = ty * kMg3TileW + tx;
    const int I0 = blockIdx.x * kMg3TileW + 1, J0 = blockIdx.y * kMg3TileH + 1;
    const int I = I0 + tx, J = J0 + ty;
    const bool act = I <= nic && J <= njc;
    const int K0 = blockIdx.z * kMg3TileD + 1;
    const int K1 = min(K0 + kMg3TileD - 1, nkc);
    const long long col = 2LL * I - 1;
    const long long ra = (2LL * J - 1) * sx + col, rb = ra + sx;

    // coarse plane K (clamped on a physical side) of the tile with its clamped
    // rim into w[3][3] (w[y][x]: rows J-1 .. J+1, columns I-1 .. I+1)
    auto fetch = [&](int K, double (&w)[3][3]) {
        const int Kc = (K < 1 && lo_phys) ? 1 : ((K > nkc && hi_phys) ? nkc : K);
        const double* ek = e + (long long)Kc * sxyc;
        __syncthreads();  // the previous plane is read no more
        for (int q = tid; q < kCoarseW * kCoarseH; q += kThreads) {
            const int cx = q % kCoarseW, cy = q / kCoarseW;
            const int Ii = min(max(I0 - 1 + cx, 1), nic), Jj = min(max(J0 - 1 + cy, 1), njc);
            tile[cy][cx] = ek[(long long)Jj * sxc + Ii];
        }
        __syncthreads();
        for (int y = 0; y < 3; ++y)
            for (int x = 0; x < 3; ++x) w[y][x] = tile[ty + y][tx + x];
    };
    // the correction of the fine cell at offsets (x, y) in {0, 1} of the quad in
    // the plane next to coarse plane z (m: plane K, z: plane K + sz)
    auto corr = [&](const double (&m)[3][3], const double (&z)[3][3], int x, int y) {
        const int X = 2 * x, Y = 2 * y;  // I + sx, J + sy in the window
        return (27.0 * m[1][1] + 9.0 * ((m[1][X] + m[Y][1]) + z[1][1]) +
                3.0 * ((m[Y][X] + z[1][X]) + z[Y][1]) + z[Y][X]) *
               0.015625;
    };

    double lo[3][3], mid[3][3], hi[3][3];
    fetch(K0 - 1, lo);
    fetch(K0, mid);
    const int nj = 2 * njc, nk = 2 * nkc;
    for (int K = K0; K <= K1; ++K) {
        Pair a0{}, b0{}, a1{}, b1{};
        double* const pl = p + (2LL * K - 1) * sxy;  // plane 2K-1
        double* const pu = pl + sxy;                 // plane 2K
        if (act) {
            a0 = ldp(pl + ra);
            b0 = ldp(pl + rb);
            a1 = ldp(pu + ra);
            b1 = ldp(pu + rb);
        }
        fetch(K + 1, hi);
        if (act) {
            a0.x += corr(mid, lo, 0, 0);
            a0.y += corr(mid, lo, 1, 0);
            b0.x += corr(mid, lo, 0, 1);
            b0.y += corr(mid, lo, 1, 1);
            a1.x += corr(mid, hi, 0, 0);
            a1.y += corr(mid, hi, 1, 0);
            b1.x += corr(mid, hi, 0, 1);
            b1.y += corr(mid, hi, 1, 1);
            stp(pl + ra, a0.x, a0.y);
            stp(pl + rb, b0.x, b0.y);
            stp(pu + ra, a1.x, a1.y);
            stp(pu + rb, b1.x, b1.y);
            // the ghost copy (solver.c:237-278), faces only
            if (I == 1) {
                pl[ra - 1] = a0.x, pl[rb - 1] = b0.x;
                pu[ra - 1] = a1.x, pu[rb - 1] = b1.x;
            }
            if (I == nic) {  // column ni + 1 = 2I + 1
                pl[ra + 2] = a0.y, pl[rb + 2] = b0.y;
                pu[ra + 2] = a1.y, pu[rb + 2] = b1.y;
            }
            if (J == 1) {
                stp(pl + col, a0.x, a0.y);
                stp(pu + col, a1.x, a1.y);
            }
            if (J == njc) {
                stp(pl + (long long)(nj + 1) * sx + col, b0.x, b0.y);
                stp(pu + (long long)(nj + 1) * sx + col, b1.x, b1.y);
            }
            if (K == 1 && lo_phys) {
                stp(p + ra, a0.x, a0.y);
                stp(p + rb, b0.x, b0.y);
            }
            if (K == nkc && hi_phys) {
                double* const pt = p + (long long)(nk + 1) * sxy;
                stp(pt + ra, a1.x, a1.y);
                stp(pt + rb, b1.x, b1.y);
            }
        }
        for (int y = 0; y < 3; ++y)
            for (int x = 0; x < 3; ++x) {
                lo[y][x] = mid[y][x];
                mid[y][x] = hi[y][x];
            }
    }
}

__global__ __launch_bounds__(kThreads) void mg3_prolong_correct_kernel(
    double* __restrict__ p, const double* __restrict__ e, int nic, int njc, int nkc, long long sx,
    long long sxy, long long sxc, long long sxyc) {
    mg3_prolong_correct_body(p, e, nic, njc, nkc, sx, sxy, sxc, sxyc, true, true);
}

__global__ __launch_bounds__(kThreads) void mg3_prolong_correct_slab_kernel(
    double* __restrict__ p, const double* __restrict__ e, int nic, int njc, int nkc, long long sx,
    long long sxy, long long sxc, long long sxyc, int lo_phys, int hi_phys) {
    mg3_prolong_correct_body(p, e, nic, njc, nkc, sx, sxy, sxc, sxyc, lo_phys != 0, hi_phys != 0);
}

dim3 mg3_grid(int nic, int njc, int nkc) {
    return dim3((nic + kMg3TileW - 1) / kMg3TileW, (njc + kMg3TileH - 1) / kMg3TileH,
                (nkc + kMg3TileD - 1) / kMg3TileD);
}

}  // namespace

void launch_mg3_residual_restrict(hipStream_t s, const G3& f, const G3& c, const double* p,
                                  const double* rhs, double* rc, double idx2, double idy2,
                                  double idz2) {
    hipLaunchKernelGGL(mg3_residual_restrict_kernel, mg3_grid(c.I, c.J, c.K),
                       dim3(kMg3TileW, kMg3TileH), 0, s, p, rhs, rc, c.I, c.J, c.K, f.sx, f.sxy,
                       c.sx, c.sxy, idx2, idy2, idz2);
}

void launch_mg3_prolong_correct(hipStream_t s, const G3& f, const G3& c, double* p,
                                const double* e) {
    hipLaunchKernelGGL(mg3_prolong_correct_kernel, mg3_grid(c.I, c.J, c.K),
                       dim3(kMg3TileW, kMg3TileH), 0, s, p, e, c.I, c.J, c.K, f.sx, f.sxy, c.sx,
                       c.sxy);
}

void launch_mg3_prolong_correct_slab(hipStream_t s, const G3& f, const G3& c, double* p,
                                     const double* e, long long koff_c, bool lo_phys,
                                     bool hi_phys) {
    hipLaunchKernelGGL(mg3_prolong_correct_slab_kernel, mg3_grid(c.I, c.J, c.K),
                       dim3(kMg3TileW, kMg3TileH), 0, s, p, e + koff_c * c.sxy, c.I, c.J, c.K,
                       f.sx, f.sxy, c.sx, c.sxy, lo_phys ? 1 : 0, hi_phys ? 1 : 0);
}

}  // namespace misor
