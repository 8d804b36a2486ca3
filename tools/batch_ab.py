#!/usr/bin/env python3
"""A/B of the batched solve against the path it replaces, in one process on
one build of libmisor.so:

  (a) Batch.solve_rb with B members: one launch, one workgroup per member;
  (b) a host loop of B Grid.solve_rb calls (the whole-solve LDS kernel, one
      workgroup a launch) on the same data.

    python tools/batch_ab.py [--sizes 100,128] [--batches 1,64,256,1024] [--out FILE]

Every member is poisson.par's problem (assignment-4 initSolver fields, problem
2, eps 1e-6, omg 1.9, itermax 1000000) on n x n cells.  Host clock around the
synchronising call: (a) one Batch.solve_rb; (b) the sum over the B
Grid.solve_rb calls, the grid's fields re-initialised before each call outside
the clock.  One warm-up of both, then 5 repetitions with (a) and (b)
alternated; the table gives the median and the min .. max.  The iteration
counts of (a) and (b) must be equal before a time is printed.  Exits non-zero
if (a) does not beat (b) at B = 256.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "practical-parallel-algorithms-with-mpi_amd"))

OMG, EPS, ITERMAX = 1.9, 1e-6, 1000000  # poisson.par
REPS = 5


def median(v):
    return sorted(v)[len(v) // 2]


def measure(M, n, nb):
    ta, tb = [], []
    with M.Batch(n, n, 1.0 / n, 1.0 / n, nb) as b, \
            M.Grid(n, n, 1.0 / n, 1.0 / n, OMG, EPS, ITERMAX) as g:
        b.set_params(omega=OMG, eps=EPS, itermax=ITERMAX)
        for rep in range(REPS + 1):  # the first is the warm-up
            b.poisson_init(1.0, 1.0, 2)
            t0 = time.perf_counter()
            it_a, _ = b.solve_rb()
            ta.append((time.perf_counter() - t0) * 1e3)
            it_b, t = [], 0.0
            for m in range(nb):
                g.poisson_init(1.0, 1.0, 2)
                t0 = time.perf_counter()
                it, _ = g.solve_rb()
                t += time.perf_counter() - t0
                it_b.append(it)
            tb.append(t * 1e3)
            assert list(it_a) == it_b, (n, nb, sorted(set(it_a)), sorted(set(it_b)))
    return it_b[0], ta[1:], tb[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,128")
    ap.add_argument("--batches", default="1,64,256,1024")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import pymisor as M

    lines = ["B problems of poisson.par (omg 1.9, eps 1e-6) on n x n: ms for all B, median "
             "[min .. max] of %d after one warm-up, (a) and (b) alternated" % REPS,
             "(a) Batch.solve_rb, one launch      (b) host loop of B Grid.solve_rb calls",
             ""]
    verdict = {}
    for n in (int(x) for x in a.sizes.split(",")):
        for nb in (int(x) for x in a.batches.split(",")):
            it, ta, tb = measure(M, n, nb)
            lines.append("%4d^2  %5d iterations  B %5d   (a) %10.3f [%10.3f .. %10.3f]   "
                         "(b) %10.3f [%10.3f .. %10.3f]   (b) / (a) %7.2fx"
                         % (n, it, nb, median(ta), min(ta), max(ta), median(tb), min(tb),
                            max(tb), median(tb) / median(ta)))
            print(lines[-1], file=sys.stderr, flush=True)
            if nb == 256:
                verdict[n] = median(ta) < median(tb)
    lines.append("")
    lines.append("(a) beats (b) at B = 256: %s"
                 % ", ".join("%d^2 %s" % (n, "yes" if ok else "NO") for n, ok in verdict.items()))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt)
    return 0 if all(verdict.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
