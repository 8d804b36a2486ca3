#!/usr/bin/env python3
"""misor_solve_mg_dist measured on in-process ranks that share ONE GPU
(DESIGN.md "Geometric multigrid, decomposed"): assignment-4's problem 2, eps
1e-6, n x n cells on 1 / 2 / 4 ranks, time to res < eps^2 of

  (a) Grid.solve_mg_dist for gather_cells in {0, 1024, 4096, 16384, 65536},
  (b) Grid.solve_rb capped at 1000 iterations on the same ranks (not converged:
      what the decomposed grid could run before), and
  (c) the single-rank Grid.solve_mg, of this build or of --base-lib (another
      libmisor.so, e.g. the parent commit's).

    python tools/mg_dist_ab.py [--n 4096] [--ranks 1,2,4] [--gather 0,1024,4096,16384,65536]
                               [--base-lib PATH] [--limit SECONDS] [--out FILE]

Every row is a process of its own under its own time limit (--limit), so a
step that hangs or fails ends that row only and starts nothing after it.  The
ranks of a row are threads of that process; the clock is the host's around the
collective call on rank 0 between two thread barriers, the fields are
re-initialised outside it.  One warm-up, then 5 repetitions: median [min ..
max] in ms.  Ranks that share a GPU share its HBM and its compute units and
exchange halos by copies inside one device: the table orders the gather_cells
values against each other and says nothing about scaling over xGMI.
"""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "practical-parallel-algorithms-with-mpi_amd"))

OMG, EPS, ITERMAX = 1.9, 1e-6, 10 ** 7
REPS = 5
RB_CAP = 1000


def median(v):
    return sorted(v)[len(v) // 2]


def fmt(v):
    return "%10.3f [%10.3f .. %10.3f]" % (median(v), min(v), max(v))


def child(kind, n, ranks, gather, base_lib):
    """one row: prints a JSON line {times, count, res, levels, ndist}"""
    import pymisor as M

    if base_lib:
        M.LIBPATH = base_lib
        # an older library exports fewer entry points: bind what it has
        M.SIGNATURES = {k: v for k, v in M.SIGNATURES.items()
                        if k not in ("misor_solve_mg_dist", "misor_mg_dist_levels")}
    out = {}
    if ranks == 1 and kind == "mg":
        t = []
        with M.Grid(n, n, 1.0 / n, 1.0 / n, OMG, EPS, ITERMAX) as g:
            for _ in range(REPS + 1):
                g.poisson_init(1.0, 1.0, 2)
                t0 = time.perf_counter()
                cnt, res = g.solve_mg()
                t.append((time.perf_counter() - t0) * 1e3)
            out = dict(times=t[1:], count=cnt, res=res)
        print(json.dumps(out), flush=True)
        return 0
    bar = threading.Barrier(ranks)
    err = []

    def body(r):
        try:
            with M.Grid(n, n, 1.0 / n, 1.0 / n, OMG, EPS, ITERMAX, device=0, nranks=ranks, rank=r,
                        comm_id=b"LOCAL:mgdistab") as g:
                t = []
                for _ in range(REPS + 1):
                    g.poisson_init(1.0, 1.0, 2)
                    g.synchronize()
                    bar.wait()
                    t0 = time.perf_counter()
                    if kind == "dist":
                        cnt, res = g.solve_mg_dist(gather)
                    else:
                        cnt, res = g.solve_rb(RB_CAP)
                    bar.wait()
                    t.append((time.perf_counter() - t0) * 1e3)
                if r == 0:
                    st = g.stats()
                    out.update(times=t[1:], count=cnt, res=res, levels=st["mg_levels"],
                               ndist=st["mg_dist_levels"])
        except BaseException as e:
            err.append((r, repr(e)))
            bar.abort()

    th = [threading.Thread(target=body, args=(r,)) for r in range(ranks)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    if err:
        print(json.dumps(dict(error=repr(err))), flush=True)
        return 1
    print(json.dumps(out), flush=True)
    return 0


def row(a, kind, ranks, gather=-1, base_lib=""):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--n", str(a.n), "--ranks",
           str(ranks), "--gather", str(gather)]
    if base_lib:
        cmd += ["--base-lib", base_lib]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    except subprocess.TimeoutExpired:
        return None, "no result within %d s" % a.limit
    if r.returncode != 0:
        return None, "exit status %d: %s" % (r.returncode, (r.stdout + r.stderr).strip()[-300:])
    return json.loads(r.stdout.strip().split("\n")[-1]), ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--ranks", default="1,2,4")
    ap.add_argument("--gather", default="0,1024,4096,16384,65536")
    ap.add_argument("--base-lib", default="")
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.n, int(a.ranks), int(a.gather), a.base_lib)
    lines = ["assignment-4 problem 2, eps 1e-6, %d^2 cells, in-process ranks on one GPU: ms, median "
             "[min .. max] of %d after one warm-up" % (a.n, REPS), ""]

    def emit(s):
        lines.append(s)
        print(s, file=sys.stderr, flush=True)

    res, why = row(a, "mg", 1, base_lib=a.base_lib)
    emit("(c) single-rank solve_mg (%s)" % (a.base_lib or "this build"))
    if res is None:
        emit("    failed: " + why)
        base = None
    else:
        base = median(res["times"])
        emit("    1 rank   %3d cycles  res %.2e  %s" % (res["count"], res["res"], fmt(res["times"])))
    ok = res is not None
    for ranks in (int(x) for x in a.ranks.split(",") if x):
        if not ok:
            break  # a failed row: nothing more is started on the GPU
        emit("")
        emit("%d rank%s" % (ranks, "" if ranks == 1 else "s"))
        for gc in (int(x) for x in a.gather.split(",") if x):
            res, why = row(a, "dist", ranks, gc)
            if res is None:
                emit("(a) gather_cells %6d  failed: %s" % (gc, why))
                ok = False
                break
            emit("(a) gather_cells %6d  %2d of %2d levels distributed  %3d cycles  res %.2e  %s%s"
                 % (gc, res["ndist"], res["levels"], res["count"], res["res"], fmt(res["times"]),
                    "   / (c) %5.2fx" % (median(res["times"]) / base) if base else ""))
        if not ok:
            break
        res, why = row(a, "rb", ranks)
        if res is None:
            emit("(b) solve_rb, %d iterations  failed: %s" % (RB_CAP, why))
            ok = False
            break
        emit("(b) solve_rb capped at %d     %5d iterations  res %.2e (not converged)  %s"
             % (RB_CAP, res["count"], res["res"], fmt(res["times"])))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
