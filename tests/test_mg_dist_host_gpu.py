"""MISOR_RANKS=4 bin/exe-poisson-mg <file.par>: the host program on a decomposed
domain (misor_solve_mg_dist, host/main_poisson_mg.c) writes the p.dat of the
one-rank run."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "practical-parallel-algorithms-with-mpi_amd", "bin")

PAR = """name poisson
xlength 1.0
ylength 1.0
imax 64
jmax 48
itermax 1000000
eps 0.000001
omg 1.9
"""


def run(tmp, ranks):
    d = tmp / ("r%d" % ranks)
    d.mkdir()
    (d / "poisson.par").write_text(PAR)
    env = dict(os.environ)
    env.pop("MISOR_RANKS", None)
    if ranks > 1:
        env["MISOR_RANKS"] = str(ranks)
    r = subprocess.run([os.path.join(BIN, "exe-poisson-mg"), "poisson.par"], cwd=d, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    # only rank 0 prints the cycle count: one number in front of "Walltime"
    m = re.findall(r"(?m)(?:^|\s)(\d+) Walltime \d+\.\d\ds", r.stdout)
    assert len(m) == 1 and "Cells (x, y): 64, 48" in r.stdout, r.stdout
    assert len(re.findall(r"Walltime", r.stdout)) == 1, r.stdout
    return int(m[0]), (d / "p.dat").read_bytes(), r.stdout


def test_exe_poisson_mg_four_ranks(tmp_path):
    c1, p1, out1 = run(tmp_path, 1)
    c4, p4, out4 = run(tmp_path, 4)
    print("cycles", c1, c4)
    assert 1 <= c1 <= 20 and abs(c4 - c1) <= 1, (c1, c4)
    assert len(p1) > 0 and p4 == p1
    # one cycle count, nothing else, where the one-rank run prints its own
    assert re.sub(r"\d+ Walltime \d+\.\d\ds", "", out4) == re.sub(r"\d+ Walltime \d+\.\d\ds", "",
                                                                   out1)
