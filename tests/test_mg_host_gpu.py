"""bin/exe-poisson-mg <file.par>: exe-poisson with the solve replaced by
multigrid V-cycles (host/main_poisson_mg.c)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "practical-parallel-algorithms-with-mpi_amd", "bin")


def test_exe_poisson_mg(golden, tmp_path):
    shutil.copy(os.path.join(golden, "a4_poisson.par"), tmp_path / "poisson.par")
    r = subprocess.run([os.path.join(BIN, "exe-poisson-mg"), "poisson.par"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = r.stdout
    assert "Parameters:" in out and "Cells (x, y): 100, 100" in out
    # the cycle count where exe-poisson prints its 2388 iterations: 100 -> 50 ->
    # 25 is three levels; the numpy prototype converges in about ten cycles
    m = re.search(r"(?m)(^|\s)(\d+) Walltime \d+\.\d\ds", out)
    assert m, out
    assert 1 <= int(m.group(2)) <= 20, out
    # p.dat in exe-poisson's format: (jmax + 2) rows of (imax + 2) "%f " values
    rows = (tmp_path / "p.dat").read_text().split("\n")
    assert rows[-1] == "" and len(rows) == 103
    assert all(row.endswith(" ") and len(row.split()) == 102 for row in rows[:-1])
    p = np.array([[float(x) for x in row.split()] for row in rows[:-1]])
    # the converged field, up to the constant, of the committed red-black result:
    # "%f" rounds each value of p.dat by at most 0.5e-6, and so its mean; the two
    # solves, both stopped at eps = 1e-6, agree to 2e-8 in the numpy prototype
    z = np.load(os.path.join(golden, "rb_poisson100.npz"))["p"]
    a, b = p[1:-1, 1:-1], z[1:-1, 1:-1]
    assert np.abs((a - a.mean()) - (b - b.mean())).max() < 2e-6
