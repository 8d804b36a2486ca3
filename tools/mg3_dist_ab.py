#!/usr/bin/env python3
"""misor3_solve_mg_dist measured on in-process ranks that share ONE GPU
(DESIGN.md "Geometric multigrid, 3D, decomposed"): the cosine right-hand side
of tools/mg3_ab.py, eps 1e-5, n^3 cells on 1 / 2 / 4 slabs, time to res < eps^2
of

  (a) Grid3.solve_mg_dist for gather_cells in {0, 4096, 32768, 262144, 2097152},
  (b) the slab Grid3.solve capped at 1000 iterations on the same ranks (not
      converged: what a decomposed 3D grid could run before), and
  (c) the single-rank Grid3.solve_mg.

    python tools/mg3_dist_ab.py [--n 256] [--ranks 1,2,4]
                                [--gather 0,4096,32768,262144,2097152]
                                [--limit SECONDS] [--out FILE]

Every row is a process of its own under its own time limit (--limit), so a
step that hangs or fails ends that row only and starts nothing after it.  The
ranks of a row are threads of that process; the clock is the host's around the
collective call on rank 0 between two thread barriers, the fields are
re-initialised outside it.  One warm-up, then 5 repetitions: median [min ..
max] in ms.  Ranks that share a GPU share its HBM and its compute units,
exchange halos by copies inside one device and meet at host barriers: the table
orders the gather_cells values against each other and says nothing about
scaling over xGMI.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

EPS = 1e-5
REPS = 5
RB_CAP = 1000


def median(v):
    return sorted(v)[len(v) // 2]


def fmt(v):
    return "%10.3f [%10.3f .. %10.3f]" % (median(v), min(v), max(v))


def child(kind, n, ranks, gather):
    """one row: prints a JSON line {times, count, res, levels, ndist}"""
    import numpy as np

    import mg3_oracle as O
    import pymisor as M

    p0, rhs = O.cosine_problem(n)
    prm = O.make_prm((n,) * 3, (1.0,) * 3, eps=EPS, omg=1.8, itermax=RB_CAP)
    out = {}
    bar = threading.Barrier(ranks)
    err = []

    def body(r):
        try:
            kw = dict(device=0, nranks=ranks, rank=r, comm_id=b"LOCAL:mg3distab") if ranks > 1 else {}
            with M.Grid3(prm, **kw) as g:
                sl = slice(g.koff, g.koff + g.kloc + 2)
                mine_p, mine_rhs = np.ascontiguousarray(p0[sl]), np.ascontiguousarray(rhs[sl])
                t = []
                for _ in range(REPS + 1):
                    g.upload(M.P3, mine_p)
                    g.upload(M.RHS3, mine_rhs)
                    g.call("synchronize")
                    bar.wait()
                    t0 = time.perf_counter()
                    if kind == "dist":
                        cnt, res = g.solve_mg_dist(gather)
                    elif kind == "mg":
                        cnt, res = g.solve_mg()
                    else:
                        cnt, res = g.solve()
                    g.call("synchronize")
                    bar.wait()
                    t.append((time.perf_counter() - t0) * 1e3)
                if r == 0:
                    info = g.mg_info()
                    out.update(times=t[1:], count=cnt, res=res, levels=info["levels"],
                               ndist=info["dist_levels"])
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


def row(a, kind, ranks, gather=-1):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--n", str(a.n), "--ranks",
           str(ranks), "--gather", str(gather)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    except subprocess.TimeoutExpired:
        return None, "no result within %d s" % a.limit
    if r.returncode != 0:
        return None, "exit status %d: %s" % (r.returncode, (r.stdout + r.stderr).strip()[-300:])
    return json.loads(r.stdout.strip().split("\n")[-1]), ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--ranks", default="1,2,4")
    ap.add_argument("--gather", default="0,4096,32768,262144,2097152")
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.n, int(a.ranks), int(a.gather))
    lines = ["rhs = cos(2 pi x) cos(2 pi y) cos(2 pi z), p0 = 0, eps 1e-5, %d^3 cells, in-process "
             "ranks on one GPU: ms, median [min .. max] of %d after one warm-up" % (a.n, REPS), ""]

    def emit(s):
        lines.append(s)
        print(s, file=sys.stderr, flush=True)

    res, why = row(a, "mg", 1)
    emit("(c) single-rank solve_mg")
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
                emit("(a) gather_cells %8d  failed: %s" % (gc, why))
                ok = False
                break
            emit("(a) gather_cells %8d  %2d of %2d levels distributed  %3d cycles  res %.2e  %s%s"
                 % (gc, res["ndist"], res["levels"], res["count"], res["res"], fmt(res["times"]),
                    "   / (c) %5.2fx" % (median(res["times"]) / base) if base else ""))
        if not ok:
            break
        res, why = row(a, "rb", ranks)
        if res is None:
            emit("(b) solve, %d iterations  failed: %s" % (RB_CAP, why))
            ok = False
            break
        emit("(b) solve capped at %d          %5d iterations  res %.2e (%s)  %s"
             % (RB_CAP, res["count"], res["res"],
                "converged" if res["res"] < EPS * EPS else "not converged", fmt(res["times"])))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
