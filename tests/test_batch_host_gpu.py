"""bin/exe-poisson-scan <file.par> <omg_lo> <omg_hi> <n>: the relaxation-factor
study around poisson.par as one batched solve (host/main_poisson_scan.c)."""
import os
import shutil
import subprocess

import pytest

import orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "practical-parallel-algorithms-with-mpi_amd", "bin", "exe-poisson-scan")


def scan(tmp_path, *args):
    return subprocess.run([EXE, *args], cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_scan_matches_the_oracle_per_omega(golden, tmp_path):
    shutil.copy(os.path.join(golden, "a4_poisson.par"), tmp_path / "poisson.par")
    r = scan(tmp_path, "poisson.par", "1.7", "1.95", "6")
    assert r.returncode == 0, r.stderr
    prm = orc.read_par(os.path.join(golden, "a4_poisson.par"))
    ni, nj = prm["imax"], prm["jmax"]
    lo, hi, n = 1.7, 1.95, 6
    want = []
    for m in range(n):
        omega = lo + m * (hi - lo) / (n - 1)
        p, rhs = orc.poisson_init(ni, nj, prm["xlength"], prm["ylength"], 2)
        it, _ = orc.solve_rb(p, rhs, prm["xlength"] / ni, prm["ylength"] / nj, omega,
                             prm["eps"], prm["itermax"])
        want.append("%f %d\n" % (omega, it))
    assert r.stdout == "".join(want), (r.stdout, want)


def test_scan_single_member_is_omg_lo(golden, tmp_path):
    shutil.copy(os.path.join(golden, "a4_poisson.par"), tmp_path / "poisson.par")
    r = scan(tmp_path, "poisson.par", "1.9", "1.2", "1")
    assert r.returncode == 0, r.stderr
    assert r.stdout == "1.900000 2388\n"


@pytest.mark.parametrize("args", [(), ("poisson.par",), ("poisson.par", "1.7", "1.95"),
                                  ("poisson.par", "1.7", "1.95", "0"),
                                  ("poisson.par", "1.7", "1.95", "six"),
                                  ("poisson.par", "x", "1.95", "6"),
                                  ("poisson.par", "1.7", "1.95", "6", "7")])
def test_bad_arguments_print_usage(golden, tmp_path, args):
    shutil.copy(os.path.join(golden, "a4_poisson.par"), tmp_path / "poisson.par")
    r = scan(tmp_path, *args)
    assert r.returncode != 0
    assert "Usage:" in r.stderr and "<omg_lo> <omg_hi> <n>" in r.stderr
    assert r.stdout == ""


def test_grid_that_does_not_fit_prints_the_library_message(golden, tmp_path):
    txt = open(os.path.join(golden, "a4_poisson.par")).read()
    (tmp_path / "big.par").write_text(txt.replace("imax       100", "imax       200")
                                      .replace("jmax       100", "jmax       200"))
    r = scan(tmp_path, "big.par", "1.7", "1.95", "6")
    assert r.returncode != 0
    assert "LDS-resident problems only" in r.stderr and "misor_create" in r.stderr
