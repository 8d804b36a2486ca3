"""bin/exe-ns3d with MISOR_PSOLVE: unset it is today's program (the .vtk of the
3D oracle's run, byte for byte), with mg the step's pressure solve is
misor3_solve_mg with the defaults.  Both solvers stop at eps, so their
velocities differ by tolerance noise; its scale D is measured on the oracle:
the max abs velocity difference between orc3 runs of the same case at eps and
at eps / 4.  D = 5.04e-7 for the case below (DESIGN.md "Geometric multigrid,
3D"); the mg-vs-SOR difference is held to 10 D, the factor because the two
solvers' stopping measures differ."""
import os
import subprocess

import numpy as np
import pytest

import orc3
from test_ns3d_host_gpu import BIN, vtk_ascii, vtk_header, write_par

pytestmark = pytest.mark.gpu

CASE = dict(imax=32, jmax=32, kmax=32, te=0.1)  # 4 time steps
D_ORACLE = 5.04e-7


def run_exe(par, cwd, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("MISOR_PSOLVE", "MISOR_RANKS")}
    e.update(env)
    return subprocess.run([os.path.join(BIN, "exe-ns3d"), par.name], cwd=cwd, env=e,
                          capture_output=True, text=True, timeout=120)


TAG = b"\nVECTORS velocity double\n"


def vtk_binary(prm, pg, ug, vg, wg):
    """the BINARY file vtkWriter.c writes: big-endian doubles"""
    head = vtk_header(prm, "BINARY").encode() + b"SCALARS pressure double 1\nLOOKUP_TABLE default\n"
    vel = np.stack([ug, vg, wg], axis=1)
    return head + pg.astype(">f8").tobytes() + TAG + vel.astype(">f8").tobytes() + b"\n"


def read_vtk_velocity(path, prm, npts):
    raw = path.read_bytes()
    off = len(vtk_binary(prm, *(np.zeros(npts),) * 4)) - 1 - 24 * npts
    return np.frombuffer(raw, dtype=">f8", count=3 * npts, offset=off)


def test_psolve_unset_and_mg(golden, tmp_path):
    par = write_par(golden, tmp_path, "a6_dcavity.par", **CASE)
    prm = orc3.read_par3(str(par))
    ns = orc3.NS3(prm)
    ns.run()
    d_sor, d_mg = tmp_path / "sor", tmp_path / "mg"
    for d in (d_sor, d_mg):
        d.mkdir()
        (d / par.name).write_text(par.read_text())
    # binary .vtk: the doubles themselves, so the comparison below is not
    # limited by the ASCII file's six decimals
    r_sor = run_exe(par, d_sor, MISOR_VTK_FORMAT="binary")
    assert r_sor.returncode == 0, r_sor.stderr
    assert "Pressure solver" not in r_sor.stdout
    assert (d_sor / "dcavity.vtk").read_bytes() == vtk_binary(prm, *ns.collect())
    r_mg = run_exe(par, d_mg, MISOR_PSOLVE="mg", MISOR_VTK_FORMAT="binary")
    assert r_mg.returncode == 0, r_mg.stderr
    assert "Pressure solver: geometric multigrid V-cycles (misor3_solve_mg)" in r_mg.stdout
    npts = 32 ** 3
    diff = np.abs(read_vtk_velocity(d_mg / "dcavity.vtk", prm, npts) -
                  read_vtk_velocity(d_sor / "dcavity.vtk", prm, npts)).max()
    print("mg vs SOR max abs velocity difference", diff, "D", D_ORACLE)
    assert diff <= 10 * D_ORACLE, diff


def test_psolve_sor_is_the_default(golden, tmp_path):
    par = write_par(golden, tmp_path, "a6_dcavity.par", imax=16, jmax=12, kmax=10, te=0.05)
    prm = orc3.read_par3(str(par))
    ns = orc3.NS3(prm)
    ns.run()
    r = run_exe(par, tmp_path, MISOR_PSOLVE="sor")
    assert r.returncode == 0 and "Pressure solver" not in r.stdout
    assert (tmp_path / "dcavity.vtk").read_text() == vtk_ascii(prm, *ns.collect())


@pytest.mark.parametrize("env,msg", [
    (dict(MISOR_PSOLVE="mg", MISOR_RANKS="2"), "single rank only"),
    (dict(MISOR_PSOLVE="bogus"), "unknown pressure solver"),
])
def test_psolve_errors_start_no_solve(golden, tmp_path, env, msg):
    par = write_par(golden, tmp_path, "a6_dcavity.par", **CASE)
    r = run_exe(par, tmp_path, **env)
    assert r.returncode != 0
    assert msg in r.stderr and "MISOR_PSOLVE" in r.stderr
    assert "Solution took" not in r.stdout and not (tmp_path / "dcavity.vtk").exists()
