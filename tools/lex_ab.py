#!/usr/bin/env python3
"""Interleaved A/B of misor_solve_lex: a parent build of libmisor.so (the
one-workgroup kernel at every size) against the in-tree build (one workgroup,
and the tiled wavefront at several tile sizes).

    python tools/lex_ab.py --parent path/to/parent/libmisor.so \
        --sizes 256,512,1024,4096 --tiles 96x96,32x32,64x64,128x64 --rounds 3 --reps 3

Per size n: Poisson init on n x n, eps = 1e-300, itermax = 5, both xorder
values.  Every (library, size) runs in a child process of its own, the two
libraries alternated within each round; a child warms each configuration up
once, then times `reps` solves (host clock around misor_solve_lex, which ends
in a stream synchronise; p re-initialised before each).  Prints per
configuration the median and the min .. max over all rounds x reps (the
spread), and whether p is identical across all configurations of one (size,
xorder).  "parent" = the parent library; "one-wg" = the in-tree library with
MISOR_TUNE_LEX_TILED = 0; "auto" = the in-tree default rule.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "practical-parallel-algorithms-with-mpi_amd"))


def child(a):
    import pymisor as M

    new = not a.lib
    if a.lib:
        M.LIBPATH = os.path.abspath(a.lib)
    n = a.size
    cfgs = [("one-wg", None)] if new else [("parent", None)]
    if new:
        cfgs += [("auto", None)] + [("tiled %s" % t, tuple(int(x) for x in t.split("x")))
                                    for t in a.tiles.split(",") if t]
    out = []
    with M.Grid(n, n, 1.0 / n, 1.0 / n, 1.9, 1e-300, a.itermax) as g:
        for xorder in (0, 1):
            for label, tile in cfgs:
                if new:
                    g.set_tuning(M.TUNE_LEX_TILED, 0 if label == "one-wg" else
                                 -1 if label == "auto" else 1)
                    # (a pair must fit in LDS at every step: through a narrow tile)
                    g.set_tuning(M.TUNE_LEX_TILE_W, 8)
                    g.set_tuning(M.TUNE_LEX_TILE_H, tile[1] if tile else 0)
                    g.set_tuning(M.TUNE_LEX_TILE_W, tile[0] if tile else 0)
                ms = []
                for r in range(a.reps + 1):  # the first is the warm-up
                    g.poisson_init(1.0, 1.0, 2)
                    t0 = time.perf_counter()
                    it, res = g.solve_lex(xorder)
                    ms.append((time.perf_counter() - t0) * 1e3)
                assert it == a.itermax, it
                h = hashlib.sha1(g.download(M.P).tobytes()).hexdigest()[:12]
                is_tiled = g.get_tuning(M.TUNE_LEX_TILED) if new else 0
                out.append(dict(label=label, xorder=xorder, ms=ms[1:], hash=h, res=res,
                                tiled=is_tiled))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--size", type=int, default=0)
    ap.add_argument("--sizes", default="256,512,1024,4096")
    ap.add_argument("--tiles", default="96x96,32x32,64x64,128x64")
    ap.add_argument("--itermax", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent:
        raise SystemExit("--parent: the parent commit's libmisor.so")
    lines = ["misor_solve_lex, Poisson init, eps 1e-300, itermax %d: ms per solve, median "
             "[min .. max] over %d rounds x %d reps, child processes alternated"
             % (a.itermax, a.rounds, a.reps)]
    for n in (int(x) for x in a.sizes.split(",")):
        acc, hashes, auto = {}, {}, {}
        for r in range(a.rounds):
            for lib in (a.parent, ""):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--size", str(n),
                       "--tiles", a.tiles, "--itermax", str(a.itermax), "--reps", str(a.reps)]
                if lib:
                    cmd += ["--lib", lib]
                o = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if o.returncode:
                    print(o.stderr[-2000:], file=sys.stderr)
                    raise SystemExit("child failed: size %d lib %r" % (n, lib))
                for d in json.loads(o.stdout.strip().splitlines()[-1]):
                    acc.setdefault((d["xorder"], d["label"]), []).extend(d["ms"])
                    hashes.setdefault(d["xorder"], set()).add(d["hash"])
                    if d["label"] == "auto":
                        auto[d["xorder"]] = d["tiled"]
            print("size %d round %d done" % (n, r), file=sys.stderr, flush=True)
        lines.append("")
        lines.append("%d x %d   (p identical across configurations: %s; the automatic rule "
                     "runs %s)" % (n, n, all(len(h) == 1 for h in hashes.values()),
                                   "tiled" if auto.get(0) else "one workgroup"))
        for (xo, label), v in sorted(acc.items()):
            v = sorted(v)
            base = sorted(acc[(xo, "parent")])
            lines.append("  xorder %d  %-14s %10.3f  [%10.3f .. %10.3f]   parent / this %6.2fx"
                         % (xo, label, v[len(v) // 2], v[0], v[-1],
                            base[len(base) // 2] / v[len(v) // 2]))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
