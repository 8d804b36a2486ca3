"""bin/exe-ns3d with MISOR_PSOLVE=mgdist: the step's pressure solve is
misor3_solve_mg_dist with the defaults, on any number of slabs.  The case, the
oracle-measured tolerance noise D = 5.04e-7 and the factor 10 on it are
tests/test_mg3_host_gpu.py's (both solvers stop at eps, so their velocities
differ by tolerance noise)."""
import numpy as np
import pytest

import orc3
from test_mg3_host_gpu import CASE, D_ORACLE, read_vtk_velocity, run_exe
from test_ns3d_host_gpu import write_par

pytestmark = pytest.mark.gpu

LINE = "(misor3_solve_mg_dist)"


def run_in(par, d, **env):
    d.mkdir()
    (d / par.name).write_text(par.read_text())
    return run_exe(par, d, MISOR_VTK_FORMAT="binary", **env)


def test_psolve_mgdist_on_one_and_two_ranks(golden, tmp_path):
    par = write_par(golden, tmp_path, "a6_dcavity.par", **CASE)
    prm = orc3.read_par3(str(par))
    d_sor, d_mg, d_one, d_two = (tmp_path / n for n in ("sor", "mg", "one", "two"))
    r = run_in(par, d_sor)
    assert r.returncode == 0, r.stderr
    r = run_in(par, d_mg, MISOR_PSOLVE="mg")
    assert r.returncode == 0, r.stderr
    r = run_in(par, d_one, MISOR_PSOLVE="mgdist")
    assert r.returncode == 0, r.stderr
    assert "Pressure solver: " in r.stdout and LINE in r.stdout
    # one rank: the call is misor3_solve_mg
    assert (d_one / "dcavity.vtk").read_bytes() == (d_mg / "dcavity.vtk").read_bytes()
    r = run_in(par, d_two, MISOR_PSOLVE="mgdist", MISOR_RANKS="2")
    assert r.returncode == 0, r.stderr
    assert "Pressure solver: " in r.stdout and LINE in r.stdout
    npts = 32 ** 3
    diff = np.abs(read_vtk_velocity(d_two / "dcavity.vtk", prm, npts) -
                  read_vtk_velocity(d_sor / "dcavity.vtk", prm, npts)).max()
    same = (d_two / "dcavity.vtk").read_bytes() == (d_mg / "dcavity.vtk").read_bytes()
    print("mgdist on 2 ranks vs SOR max abs velocity difference", diff, "D", D_ORACLE,
          "| byte for byte the single-rank mg file:", same)
    assert diff <= 10 * D_ORACLE, diff


def test_psolve_mgdist_refused_on_a_cartesian_grid(golden, tmp_path):
    par = write_par(golden, tmp_path, "a6_dcavity.par", **CASE)
    r = run_exe(par, tmp_path, MISOR_PSOLVE="mgdist", MISOR_RANKS="2", MISOR_DIMS="2x1x1")
    assert r.returncode != 0
    assert "Cartesian" in r.stderr and "MISOR_PSOLVE" in r.stderr
    assert "Solution took" not in r.stdout and not (tmp_path / "dcavity.vtk").exists()
