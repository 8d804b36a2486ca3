"""bench.py --dump-outputs: a plain run writes what its timed solve left -- p,
the iteration count and the residual, float64 -- and that p is the field the
restatement of solveRB (assignment-4/src/solver.c:179-238) reaches from the
same generated input after the same number of iterations, bit for bit: the
warm-up (--warmup iterations, then a solve of the timed length) and the --steps
timed iterations.  A ragged grid (no multiple of a block or of the pass
length), so the last pass is a short one.  The plain line carries none of
what --full adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_timed_solve(tmp_path):
    n, steps, warmup = 1000, 13, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", str(n),
           "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=150, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["dtype"] == "f64" and line["unit"] == "MLUP/s" and line["higher_is_better"]
    assert not [k for k in line if k.startswith("cpu_baseline")]
    got = {f: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["iterations.npy", "p.npy", "residual.npy"]
    assert all(v.dtype == np.float64 for v in got.values())
    p, rhs = orc.poisson_init(n, n)
    for k in (warmup, steps, steps):  # each solve restarts the iteration count
        it_ref, res_ref = orc.solve_rb(p, rhs, 1.0 / n, 1.0 / n, 1.9, 1e-300, k)
    assert got["iterations.npy"].tolist() == [float(steps)] and it_ref == steps
    assert np.array_equal(got["p.npy"], p), np.argwhere(got["p.npy"] != p)[:5]
    assert abs(got["residual.npy"][0] - res_ref) <= 1e-10 * res_ref
