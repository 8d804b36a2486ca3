#!/usr/bin/env python3
"""The 3D multigrid solve measured, in one process on one build of libmisor.so:

  1. time to res < eps^2 of Grid3.solve_mg (every default) against Grid3.solve
     (omg 1.8, capped at --cap iterations) on rhs = cos(2 pi x) cos(2 pi y)
     cos(2 pi z), p0 = 0, eps 1e-5, on n^3 cells of the unit cube;
  2. solve_mg with timing on: milliseconds per cycle split into level 0's
     smoothing (misor3_get_solve_time), its two transfer kernels
     (misor3_get_mg_info; HIP events on the grid's stream) and the rest (every
     coarser level plus the host side of the cycle); the transfer kernels'
     bytes/s over their minimum of 17 B per fine cell (residual + restriction
     16 B read + 1 B written, prolongation + correction 8 B read + 8 B written +
     1 B of e read) as a fraction of 8 TB/s.

    python tools/mg3_ab.py [--sizes 128,256,384] [--cap 20000] [--out FILE]

Host clock around the synchronising call; the fields are uploaded again before
each call outside the clock.  One warm-up, then 5 repetitions, the two solvers
alternated in part 1; the tables give the median and min .. max.  Exits
non-zero if multigrid is not faster than the SOR solve at 256^3.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "practical-parallel-algorithms-with-mpi_amd"))

OMG, EPS = 1.8, 1e-5
REPS = 5
HBM = 8e12  # bytes/s
MIN_BYTES = 17  # per fine cell, either transfer kernel


def median(v):
    return sorted(v)[len(v) // 2]


def fmt(v):
    return "%9.3f [%9.3f .. %9.3f]" % (median(v), min(v), max(v))


def problem(n):
    import numpy as np

    x = (np.arange(n + 2) - 0.5) / n
    c = np.cos(2.0 * np.pi * x)
    rhs = np.ascontiguousarray(c[:, None, None] * c[None, :, None] * c[None, None, :])
    return np.zeros((n + 2,) * 3), rhs


def params(n, cap):
    return dict(imax=n, jmax=n, kmax=n, xlength=1.0, ylength=1.0, zlength=1.0, re=1000.0,
                gamma=0.9, tau=0.5, omg=OMG, eps=EPS, itermax=cap, gx=0.0, gy=0.0, gz=0.0,
                bcTop=1, bcBottom=1, bcLeft=1, bcRight=1, bcFront=1, bcBack=1, name="dcavity")


def ab(M, n, cap):
    """(cycles, res, ms) of solve_mg and (iterations, res, ms) of solve"""
    p0, rhs = problem(n)
    ta, tb = [], []
    with M.Grid3(params(n, cap)) as g:
        g.upload(M.RHS3, rhs)
        for _ in range(REPS + 1):  # the first is the warm-up
            g.upload(M.P3, p0)
            t0 = time.perf_counter()
            cyc, res_a = g.solve_mg()
            ta.append((time.perf_counter() - t0) * 1e3)
            g.upload(M.P3, p0)
            t0 = time.perf_counter()
            it, res_b = g.solve()
            tb.append((time.perf_counter() - t0) * 1e3)
            assert res_a < EPS * EPS, (n, res_a)
    return (cyc, res_a, ta[1:]), (it, res_b, tb[1:])


def split(M, n, cap):
    """solve_mg with timing on: per repetition the wall ms, level 0's smoothing
    ms and its transfer kernels' ms"""
    p0, rhs = problem(n)
    wall, smooth, restrict, prolong = [], [], [], []
    with M.Grid3(params(n, cap)) as g:
        g.upload(M.RHS3, rhs)
        for _ in range(REPS + 1):
            g.upload(M.P3, p0)
            g.enable_timing(True)  # resets the counters
            t0 = time.perf_counter()
            cyc, res = g.solve_mg()
            wall.append((time.perf_counter() - t0) * 1e3)
            info = g.mg_info()
            assert info["transfers"] == 2 * cyc, info
            smooth.append(g.solve_time()[0])
            restrict.append(info["transfer_ms"][0])
            prolong.append(info["transfer_ms"][1])
        levels = info["levels"]
    return cyc, levels, wall[1:], smooth[1:], restrict[1:], prolong[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,384")
    ap.add_argument("--cap", type=int, default=20000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import pymisor as M

    sizes = [int(x) for x in a.sizes.split(",") if x]
    lines = ["rhs = cos(2 pi x) cos(2 pi y) cos(2 pi z), p0 = 0, eps 1e-5, n^3 cells: ms, median "
             "[min .. max] of %d after one warm-up" % REPS, "",
             "1. time to res < eps^2: (a) Grid3.solve_mg, defaults   (b) Grid3.solve, omg 1.8, "
             "capped at %d iterations, alternated" % a.cap]
    verdict = None
    for n in sizes:
        (cyc, res_a, ta), (it, res_b, tb) = ab(M, n, a.cap)
        done = res_b < EPS * EPS
        lines.append("%4d^3  (a) %3d cycles  res %.2e  %s   (b) %s  res %.2e  %s   (b) / (a) %s%.1fx"
                     % (n, cyc, res_a, fmt(ta),
                        "%6d iterations" % it if done else "not converged in %d" % it, res_b,
                        fmt(tb), "" if done else "> ", median(tb) / median(ta)))
        print(lines[-1], file=sys.stderr, flush=True)
        if n == 256:
            verdict = median(ta) < median(tb)
    lines += ["", "2. Grid3.solve_mg alone, timing on, per cycle: level 0's smoothing (nu1 + nu2 = 4 "
              "iterations), its two transfer kernels (HIP events), rest = wall - those"]
    for n in sizes:
        cyc, levels, wall, smooth, restrict, prolong = split(M, n, a.cap)
        cells = float(n) ** 3
        per = lambda v: median(v) / cyc
        rest = per(wall) - per(smooth) - per(restrict) - per(prolong)
        lines.append("%4d^3  %d levels  %2d cycles  wall %s ms   per cycle %8.3f ms = smoothing "
                     "%7.3f + restrict %7.3f + prolong %7.3f + rest %7.3f"
                     % (n, levels, cyc, fmt(wall), per(wall), per(smooth), per(restrict),
                        per(prolong), rest))
        for name, ms in (("mg3_residual_restrict", restrict), ("mg3_prolong_correct", prolong)):
            rate = MIN_BYTES * cells / (per(ms) * 1e-3)
            lines.append("        %-22s %7.3f ms  %6.2f TB/s over 17 B/cell  %5.2f of 8 TB/s"
                         % (name, per(ms), rate / 1e12, rate / HBM))
        print("\n".join(lines[-3:]), file=sys.stderr, flush=True)
    if verdict is not None:
        lines += ["", "multigrid faster than the SOR solve at 256^3: %s" % ("yes" if verdict else "NO")]
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt)
    return 0 if verdict in (None, True) else 1


if __name__ == "__main__":
    sys.exit(main())
