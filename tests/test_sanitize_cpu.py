"""Host code under AddressSanitizer + UndefinedBehaviorSanitizer (SURVEY 5:
the reference's failure mode is fail-fast; here memory errors, leaks and UB
in the CPU-side code are caught by a sanitized build).

Six executables, built by `make asan` (gcc / g++ -fsanitize=address,undefined
-fno-sanitize-recover=undefined):
  * bin/asan/host-check (practical-parallel-algorithms-with-mpi_amd/host/
    sanitize_main.c): the .par reader on every .par the tests use, the
    RCCL-id hand-off file (right tag taken, stale tag refused), the legacy
    VTK writer in both formats;
  * bin/asan/pass-plan-check (host/pass_plan_check.cc): the pass-plan
    arithmetic of the red-black solve loop (csrc/pass_plan.h), every plan of
    1..400 iterations in passes of 1..10, and the short plan's rule;
  * bin/asan/decomp3-check (host/decomp3_check.cc): the 3D decompositions
    (csrc/decomp3.h) -- process grids of 1..16 ranks, owned boxes and slab
    gather ranges marked cell by cell, the refused cases, mutual neighbours;
  * bin/asan/decomp2-check (host/decomp2_check.cc): the 2D decomposition and
    its halo plans (csrc/decomp2.h) -- the process grids of 1..64 ranks
    against the recorded MPI_Dims_create table, owned blocks marked cell by
    cell, the 8-neighbour tables, and every send / receive region of every
    rank at every halo depth followed cell by cell to its peer's region;
  * bin/asan/tb-plan-check (host/tb_plan_check.cc): the launch plans of the
    temporally blocked pass (csrc/tb_plan.h) -- over ragged and tall shapes,
    every pass length of every built variant, requested block heights,
    chaining, physical sides and resident counts: the block rows of every
    geometry tile the rows, the segment lists of every part hold each of its
    blocks once, and the table recorded before the arithmetic moved to the
    header (tests/golden/tb_plan_parent.txt) comes out again;
  * oracle/_asan/oracle-check (oracle/sanitize_main.c): every oracle
    function on small ragged grids, with the reference's iteration KATs and
    multi-threaded == scalar bit identity.
GPU code is not sanitized: GPU ASan / xnack+ runs are not available on this
pool, and the library's host-side C++ only runs inside the HIP library.
"""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "practical-parallel-algorithms-with-mpi_amd")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def build(d):
    subprocess.run(["make", "-s", "-C", d, "asan"], check=True, capture_output=True)


def run(cmd, **kw):
    r = subprocess.run(cmd, env=ENV, capture_output=True, text=True, timeout=300, **kw)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    return r.stdout


def test_host_code_sanitized(tmp_path):
    build(PKG)
    pars = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.par")))
    assert len(pars) >= 4
    out = run([os.path.join(PKG, "bin", "asan", "host-check"), str(tmp_path)] + pars)
    assert "all checks passed" in out
    assert (tmp_path / "sanitize_ascii.vtk").stat().st_size > 0


def test_pass_plan_sanitized():
    build(PKG)
    out = run([os.path.join(PKG, "bin", "asan", "pass-plan-check")])
    assert "all checks passed" in out


def test_decomp3_sanitized():
    build(PKG)
    out = run([os.path.join(PKG, "bin", "asan", "decomp3-check")])
    assert "all checks passed" in out


def test_decomp2_sanitized():
    build(PKG)
    out = run([os.path.join(PKG, "bin", "asan", "decomp2-check")])
    assert "all checks passed" in out


def test_tb_plan_sanitized():
    build(PKG)
    out = run([os.path.join(PKG, "bin", "asan", "tb-plan-check"),
               os.path.join(ROOT, "tests", "golden", "tb_plan_parent.txt")])
    assert "all checks passed" in out


def test_oracle_sanitized():
    build(os.path.join(ROOT, "oracle"))
    out = run([os.path.join(ROOT, "oracle", "_asan", "oracle-check")])
    assert "all checks passed" in out
