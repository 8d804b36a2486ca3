#!/usr/bin/env python3
"""The multigrid solve measured, in one process on one build of libmisor.so:

  1. time to res < eps^2 of Grid.solve_mg (every default) against Grid.solve_rb
     (omg 1.9, itermax 10^7) on assignment-4's problem 2, eps 1e-6;
  2. solve_mg alone on large grids: cycles, seconds, and milliseconds per cycle
     split into level 0 (its smoothing passes and its two transfer kernels, by
     HIP events on the grid's stream: misor_enable_timing) and the rest (every
     coarser level plus the host side of the cycle);
  3. the two transfer kernels at level 0 of the largest grid: achieved bytes/s
     over their byte minimum (residual + restriction 16 B read + 2 B written,
     prolongation + correction 8 B read + 8 B written per fine cell) as a
     fraction of 8 TB/s, and their share of a cycle.

  0. (--tail-ab) solve_mg with the fused tail (MISOR_TUNE_MG_TAIL 1: the
     LDS-resident levels cycled in one launch; 100^2 and 128^2 are the whole
     solve in one launch) against level by level (0), alternated on one grid.

    python tools/mg_ab.py [--tail 0|1] [--tail-ab 100,128,512,1024,2048] [--ab 512,1024,2048]
                          [--big 8192,32768] [--out FILE]

--tail sets the knob for parts 1 to 3 (default 1, the library's).

Host clock around the synchronising call; the fields are re-initialised before
each call outside the clock.  One warm-up, then 5 repetitions, the two solvers
alternated in part 1; the tables give the median and min .. max.  Exits
non-zero if multigrid is not faster than solve_rb at 1024^2, or if the fused
tail's median is not below the minimum of the level-by-level runs at 100^2 and
at 1024^2 (where part 0 measured them).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "practical-parallel-algorithms-with-mpi_amd"))

OMG, EPS, ITERMAX = 1.9, 1e-6, 10 ** 7
REPS = 5
HBM = 8e12  # bytes/s
RESTRICT_BYTES, PROLONG_BYTES = 18, 16  # per fine cell


def median(v):
    return sorted(v)[len(v) // 2]


def fmt(v):
    return "%10.3f [%10.3f .. %10.3f]" % (median(v), min(v), max(v))


TAIL = 1  # --tail


def tail_ab(M, n):
    """solve_mg with MISOR_TUNE_MG_TAIL 0 and 1 alternated: per setting (cycles, res,
    times in ms), and the stats of the last fused solve"""
    out = {0: [], 1: []}
    last = {}
    with M.Grid(n, n, 1.0 / n, 1.0 / n, OMG, EPS, ITERMAX) as g:
        for _ in range(REPS + 1):  # the first is the warm-up
            for tail in (0, 1):
                g.set_tuning(M.TUNE_MG_TAIL, tail)
                g.poisson_init(1.0, 1.0, 2)
                t0 = time.perf_counter()
                cyc, res = g.solve_mg()
                out[tail].append((time.perf_counter() - t0) * 1e3)
                assert res < EPS * EPS, (n, tail, res)
                last[tail] = (cyc, res)
        st = g.stats()
    assert last[0] == last[1], (n, last)  # the same cycles and the same bits of res
    return last[1], out[0][1:], out[1][1:], st


def ab(M, n):
    """(cycles, res, times) of solve_mg and (iterations, res, times) of solve_rb, ms"""
    ta, tb = [], []
    with M.Grid(n, n, 1.0 / n, 1.0 / n, OMG, EPS, ITERMAX) as g:
        g.set_tuning(M.TUNE_MG_TAIL, TAIL)
        for _ in range(REPS + 1):  # the first is the warm-up
            g.poisson_init(1.0, 1.0, 2)
            t0 = time.perf_counter()
            cyc, res_a = g.solve_mg()
            ta.append((time.perf_counter() - t0) * 1e3)
            g.poisson_init(1.0, 1.0, 2)
            t0 = time.perf_counter()
            it, res_b = g.solve_rb()
            tb.append((time.perf_counter() - t0) * 1e3)
            assert res_a < EPS * EPS and res_b < EPS * EPS, (n, res_a, res_b)
    return (cyc, res_a, ta[1:]), (it, res_b, tb[1:])


def big(M, n):
    """solve_mg on n x n with timing on: per repetition the wall ms, level 0's
    smoothing ms and its transfer kernels' ms"""
    wall, smooth, restrict, prolong = [], [], [], []
    with M.Grid(n, n, 1.0 / n, 1.0 / n, OMG, EPS, ITERMAX) as g:
        g.set_tuning(M.TUNE_MG_TAIL, TAIL)
        g.enable_timing(True)
        for _ in range(REPS + 1):
            g.poisson_init(1.0, 1.0, 2)
            g.reset_stats()
            t0 = time.perf_counter()
            cyc, res = g.solve_mg()
            wall.append((time.perf_counter() - t0) * 1e3)
            st = g.stats()
            assert st["mg_transfers"] == 2 * cyc, st
            smooth.append(st["sweep_ms"])
            restrict.append(st["mg_transfer_ms"][0])
            prolong.append(st["mg_transfer_ms"][1])
        levels = st["mg_levels"]
    return cyc, res, levels, wall[1:], smooth[1:], restrict[1:], prolong[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", default="512,1024,2048")
    ap.add_argument("--big", default="8192,32768")
    ap.add_argument("--out", default="")
    ap.add_argument("--tail", type=int, choices=(0, 1), default=1)
    ap.add_argument("--tail-ab", default="")
    a = ap.parse_args()
    import pymisor as M

    global TAIL
    TAIL = a.tail
    lines = ["assignment-4 problem 2, eps 1e-6, n x n cells: ms, median [min .. max] of %d after "
             "one warm-up; MISOR_TUNE_MG_TAIL %d in parts 1 to 3" % (REPS, TAIL), ""]
    tail_ok = None
    sizes = [int(x) for x in a.tail_ab.split(",") if x]
    if sizes:
        lines.append("0. Grid.solve_mg, defaults: (0) level by level   (1) the tail fused, "
                     "alternated")
    for n in sizes:
        (cyc, res), t0, t1, st = tail_ab(M, n)
        lines.append("%6d^2  %3d cycles  res %.2e  %d of %d levels fused, %d launches  (0) %s   "
                     "(1) %s   (0) / (1) %6.2fx   (1) median %s min (0)"
                     % (n, cyc, res, st["mg_tail_levels"], st["mg_levels"],
                        st["mg_tail_launches"] // (REPS + 1), fmt(t0), fmt(t1),
                        median(t0) / median(t1), "<" if median(t1) < min(t0) else ">="))
        print(lines[-1], file=sys.stderr, flush=True)
        if n in (100, 1024):
            tail_ok = (tail_ok is not False) and median(t1) < min(t0)
    if sizes:
        lines.append("")
    lines += ["1. time to res < eps^2: (a) Grid.solve_mg, defaults   (b) Grid.solve_rb, omg 1.9, "
             "alternated"]
    verdict = None
    for n in (int(x) for x in a.ab.split(",") if x):
        (cyc, res_a, ta), (it, res_b, tb) = ab(M, n)
        lines.append("%6d^2  (a) %3d cycles      res %.2e  %s   (b) %8d iterations  res %.2e  %s   "
                     "(b) / (a) %8.1fx" % (n, cyc, res_a, fmt(ta), it, res_b, fmt(tb),
                                           median(tb) / median(ta)))
        print(lines[-1], file=sys.stderr, flush=True)
        if n == 1024:
            verdict = median(ta) < median(tb)
    lines += ["", "2. Grid.solve_mg alone, timing on: per cycle, level 0 = its smoothing passes + "
              "its two transfer kernels (HIP events), rest = wall - level 0"]
    last = None
    for n in (int(x) for x in a.big.split(",") if x):
        cyc, res, levels, wall, smooth, restrict, prolong = big(M, n)
        lvl0 = [s + r + p for s, r, p in zip(smooth, restrict, prolong)]
        lines.append("%6d^2  %2d levels  %3d cycles  res %.2e  wall %s ms   per cycle: %9.3f ms = "
                     "level 0 %9.3f + rest %9.3f"
                     % (n, levels, cyc, res, fmt(wall), median(wall) / cyc, median(lvl0) / cyc,
                        (median(wall) - median(lvl0)) / cyc))
        print(lines[-1], file=sys.stderr, flush=True)
        last = (n, cyc, wall, smooth, restrict, prolong)
    if last:
        n, cyc, wall, smooth, restrict, prolong = last
        cells = float(n) * n
        lines += ["", "3. the transfer kernels at level 0 of %d^2: ms per launch, bytes/s over the "
                  "byte minimum, fraction of 8 TB/s, share of a cycle's wall time" % n]
        for name, ms, nbytes in (("mg_residual_restrict", restrict, RESTRICT_BYTES),
                                 ("mg_prolong_correct", prolong, PROLONG_BYTES)):
            per = median(ms) / cyc
            rate = nbytes * cells / (per * 1e-3)
            lines.append("%-22s %8.3f ms  %6.2f TB/s  %5.2f of HBM  %5.1f%% of a cycle"
                         % (name, per, rate / 1e12, rate / HBM,
                            100.0 * median(ms) / median(wall)))
        lines.append("%-22s %8.3f ms per cycle (nu1 + nu2 = 4 iterations)  %5.1f%% of a cycle"
                     % ("level-0 smoothing", median(smooth) / cyc,
                        100.0 * median(smooth) / median(wall)))
    if verdict is not None:
        lines += ["", "multigrid faster than solve_rb at 1024^2: %s" % ("yes" if verdict else "NO")]
    if tail_ok is not None:
        lines += ["", "fused tail's median below the level-by-level minimum at 100^2 and 1024^2: %s"
                  % ("yes" if tail_ok else "NO")]
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt)
    return 0 if verdict in (None, True) and tail_ok in (None, True) else 1


if __name__ == "__main__":
    sys.exit(main())
