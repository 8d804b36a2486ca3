"""bin/exe-ns3d <par> (assignment-6/src/main.c on libmisor's 3D path) end to
end: stdout lines, the per-step iteration log and the <problem>.vtk file,
against the 3D oracle's run of the same .par (oracle/oracle3d.c, pinned to
the reference's own build by tests/test_oracle3d.py).  The run is bit-exact,
so the ASCII VTK file equals, byte for byte, the file vtkWriter.c
(assignment-6/src/vtkWriter.c:44-190) writes from the oracle's collected
arrays."""
import os
import re
import subprocess

import numpy as np
import pytest

import ns_param_sets as PS
import orc3

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "practical-parallel-algorithms-with-mpi_amd", "bin")


def write_par(golden, tmp_path, name, **over):
    txt = open(os.path.join(golden, name)).read()
    for k, v in over.items():
        txt, n = re.subn(r"(?m)^%s\s.*$" % k, "%s %s" % (k, v), txt)
        assert n == 1, k
    path = tmp_path / name.replace("a6_", "")
    path.write_text(txt)
    return path


def vtk_header(prm, fmt):
    I, J, K = prm["imax"], prm["jmax"], prm["kmax"]
    dx, dy, dz = prm["xlength"] / I, prm["ylength"] / J, prm["zlength"] / K
    return ("# vtk DataFile Version 3.0\nPAMPI cfd solver output\n%s\n"
            "DATASET STRUCTURED_POINTS\nDIMENSIONS %d %d %d\nORIGIN %f %f %f\n"
            "SPACING %f %f %f\nPOINT_DATA %d\n"
            % (fmt, I, J, K, dx * 0.5, dy * 0.5, dz * 0.5, dx, dy, dz, I * J * K))


def vtk_ascii(prm, pg, ug, vg, wg):
    return (vtk_header(prm, "ASCII") + "SCALARS pressure double 1\nLOOKUP_TABLE default\n"
            + "".join("%f\n" % x for x in pg) + "VECTORS velocity double\n"
            + "".join("%f %f %f\n" % t for t in zip(ug, vg, wg)))


def run_exe(par, tmp_path, **env):
    e = dict(os.environ, MISOR_ITERLOG=str(tmp_path / "iters.log"), **env)
    return subprocess.run([os.path.join(BIN, "exe-ns3d"), par.name], cwd=tmp_path, env=e,
                          capture_output=True, text=True, timeout=300, check=True).stdout


@pytest.mark.parametrize("name,over", [
    ("a6_dcavity.par", dict(imax=24, jmax=20, kmax=16, te=0.3)),
    ("a6_canal.par", dict(imax=40, jmax=12, kmax=10, te=0.6)),
    # forces on every axis, gamma 0.7, re 50, tau -1: gz from the .par through
    # solver_ns3d.c to misor3_desc, and the fixed-dt branch of the main loop
    # (12 steps of dt 0.005: the run of tests/golden/ns3d_force_short.npz)
    ("a6_dcavity.par", dict(PS.FORCE_RUN_3D, te=0.0575)),
])
def test_exe_ns3d_matches_oracle(golden, tmp_path, name, over):
    par = write_par(golden, tmp_path, name, **over)
    prm = orc3.read_par3(str(par))
    ns = orc3.NS3(prm)
    n, iters, _ = ns.run()
    if "gz" in over:
        assert (prm["gx"], prm["gy"], prm["gz"], prm["tau"]) == (0.5, -1.0, 0.25, -1.0)
        assert n == PS.FORCE_RUN_3D_STEPS
    out = run_exe(par, tmp_path)
    problem = prm["name"]
    assert "Parameters for %s" % problem in out
    assert "Cells (x, y, z): %d, %d, %d" % (prm["imax"], prm["jmax"], prm["kmax"]) in out
    assert re.search(r"Solution took \d+\.\d\ds", out)
    assert "Writing VTK output for %s" % problem in out
    assert "Register scalar pressure" in out and "Register vector velocity" in out
    log = np.loadtxt(tmp_path / "iters.log", ndmin=2)
    assert len(log) == n
    assert np.array_equal(log[:, 3].astype(int), iters)
    got = (tmp_path / (problem + ".vtk")).read_text()
    want = vtk_ascii(prm, *ns.collect())
    assert got == want


def test_exe_ns3d_binary_vtk(golden, tmp_path):
    par = write_par(golden, tmp_path, "a6_dcavity.par", imax=16, jmax=12, kmax=10, te=0.2)
    prm = orc3.read_par3(str(par))
    ns = orc3.NS3(prm)
    ns.run()
    run_exe(par, tmp_path, MISOR_VTK_FORMAT="binary")
    raw = (tmp_path / "dcavity.vtk").read_bytes()
    head = vtk_header(prm, "BINARY").encode() + b"SCALARS pressure double 1\nLOOKUP_TABLE default\n"
    assert raw.startswith(head)
    npts = 16 * 12 * 10
    pg, ug, vg, wg = ns.collect()
    off = len(head)
    p = np.frombuffer(raw, dtype=">f8", count=npts, offset=off)
    assert np.array_equal(p, pg)
    off += 8 * npts
    tag = b"\nVECTORS velocity double\n"
    assert raw[off:off + len(tag)] == tag
    off += len(tag)
    vel = np.frombuffer(raw, dtype=">f8", count=3 * npts, offset=off).reshape(npts, 3)
    assert np.array_equal(vel[:, 0], ug) and np.array_equal(vel[:, 1], vg)
    assert np.array_equal(vel[:, 2], wg)
    assert raw[off + 24 * npts:] == b"\n"


@pytest.mark.parametrize("ranks", [2, 3, 4])
def test_exe_ns3d_decomposed(golden, tmp_path, ranks):
    """MISOR_RANKS=N: N slabs (threads, in-process transport), result collected on
    rank 0 -- the same iteration log and the same .vtk bytes as the oracle's run"""
    par = write_par(golden, tmp_path, "a6_dcavity.par", imax=24, jmax=20, kmax=16, te=0.3)
    prm = orc3.read_par3(str(par))
    ns = orc3.NS3(prm)
    n, iters, _ = ns.run()
    out = run_exe(par, tmp_path, MISOR_RANKS=str(ranks))
    assert out.count("Parameters for dcavity") == 1 and out.count("Solution took") == 1
    log = np.loadtxt(tmp_path / "iters.log", ndmin=2)
    assert len(log) == n and np.array_equal(log[:, 3].astype(int), iters)
    assert (tmp_path / "dcavity.vtk").read_text() == vtk_ascii(prm, *ns.collect())
