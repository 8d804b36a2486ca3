"""The lexicographic SOR as a tiled wavefront over the whole device
(lex_tiled.hip; MISOR_TUNE_LEX_TILED / LEX_TILE_W / LEX_TILE_H / LEX_WGS).

Tiles of one tile anti-diagonal run at once in a persistent grid and hand p to
their right and upper neighbours through HBM; iteration k+1 reads halo cells
that another compute unit wrote in iteration k.  Bar: p bit-identical to the
CPU oracle's lexicographic solve and the iteration count equal, for every tile
size, every grid size of the launch and every schedule; res within 1e-12
relative of the oracle's (the summation order differs: one partial per tile,
then tile-index order) and bit-equal across grid sizes of one tile geometry.

Tolerance of res: a sum of n non-negative r^2 terms in any order carries a
relative error below n * 2^-53; the largest case here (600 x 520) gives
3.5e-11 as the worst-case bound and ~sqrt(n) * 2^-53 = 6e-14 as the expected
size, so the 1e-12 of tests/test_lex_gpu.py holds for these sizes as well.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import ns_gpu_driver as D
import orc
import pymisor as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "practical-parallel-algorithms-with-mpi_amd", "bin")


def fmt_pdat(p):  # writeResult, assignment-4/src/solver.c:315-320
    return "\n".join("".join("%f " % x for x in row) for row in p) + "\n"


def tiled(g, tile=(32, 16), wgs=0):
    g.set_tuning(M.TUNE_LEX_TILED, 1)
    g.set_tuning(M.TUNE_LEX_TILE_W, tile[0] if tile else 0)
    g.set_tuning(M.TUNE_LEX_TILE_H, tile[1] if tile else 0)
    g.set_tuning(M.TUNE_LEX_WGS, wgs)
    assert g.get_tuning(M.TUNE_LEX_TILED) == 1


def random_case(ni, nj, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nj + 2, ni + 2)), rng.standard_normal((nj + 2, ni + 2)),
            1.3 / ni, 0.7 / nj)


def solve(p, rhs, dx, dy, k, xorder, tile=(32, 16), wgs=0, eps=1e-300):
    ni, nj = p.shape[1] - 2, p.shape[0] - 2
    with M.Grid(ni, nj, dx, dy, 1.7, eps, k) as g:
        tiled(g, tile, wgs)
        g.upload(M.P, p)
        g.upload(M.RHS, rhs)
        it, res = g.solve_lex(xorder)
        return it, res, g.download(M.P)


# (5,3) one ragged tile, (32,16) one exact tile, (33,17) 2 x 2 tiles with last
# tiles one cell wide / high, (64,16) / (32,48) one tile row / column, (97,50)
# 4 x 4 ragged; (150,141) at the default tile (2 x 2): the HBM-resident size of
# tests/test_lex_gpu.py
@pytest.mark.parametrize("ni,nj,tile", [(5, 3, (32, 16)), (32, 16, (32, 16)), (33, 17, (32, 16)),
                                        (64, 16, (32, 16)), (32, 48, (32, 16)),
                                        (97, 50, (32, 16)), (150, 141, None)])
@pytest.mark.parametrize("xorder", [0, 1])
def test_tiled_random_fields_vs_oracle(ni, nj, tile, xorder):
    p, rhs, dx, dy = random_case(ni, nj, ni * 31 + nj + xorder)
    for k in (1, 2, 5):
        want = p.copy()
        it_ref, res_ref = orc.solve_lex(want, rhs, dx, dy, 1.7, 1e-300, k, xorder=xorder)
        it, res, got = solve(p, rhs, dx, dy, k, xorder, tile)
        print(ni, nj, k, "res", res, "oracle", res_ref, "rel", abs(res - res_ref) / abs(res_ref))
        assert it == it_ref == k
        assert np.array_equal(got, want), (k, np.argwhere(got != want)[:5])
        assert abs(res - res_ref) <= 1e-12 * abs(res_ref)


@pytest.fixture(scope="module")
def case97():
    p, rhs, dx, dy = random_case(97, 50, 97050)
    want = p.copy()
    it_ref, res_ref = orc.solve_lex(want, rhs, dx, dy, 1.7, 1e-300, 5, xorder=0)
    want.setflags(write=False)
    return p, rhs, dx, dy, want, it_ref, res_ref


def test_tiled_independent_of_schedule(case97):
    """a grid of 1 workgroup (the tiles in ticket order), 2, 7 and the
    automatic size: p, it and res the same bits"""
    p, rhs, dx, dy, want, it_ref, _ = case97
    runs = [solve(p, rhs, dx, dy, 5, 0, (32, 16), wgs) for wgs in (1, 2, 7, 0)]
    for it, res, got in runs:
        assert it == it_ref == 5
        assert np.array_equal(got, want)
        assert res == runs[0][1], (res, runs[0][1])


def test_tiled_independent_of_geometry(case97):
    p, rhs, dx, dy, want, it_ref, res_ref = case97
    for tile in ((32, 16), (64, 32), None):
        it, res, got = solve(p, rhs, dx, dy, 5, 0, tile)
        print(tile, "res", res, "oracle", res_ref)
        assert it == it_ref
        assert np.array_equal(got, want)
        assert abs(res - res_ref) <= 1e-12 * abs(res_ref)


def test_tiled_poisson_par_reproduces_committed_pdat(golden):
    """poisson.par through 28 tiles: the loop ends on the residual (2388
    iterations), the committed assignment-4/p.dat byte for byte"""
    z = np.load(os.path.join(golden, "rb_poisson100.npz"))
    with M.Grid(100, 100, 0.01, 0.01, 1.9, 1e-6, 1000000) as g:
        tiled(g)
        g.poisson_init(1.0, 1.0, 2)
        it, res = g.solve_lex(M.LEX_A4)
        p = g.download(M.P)
    assert it == int(z["iterations_lex"]) == 2388
    assert np.array_equal(p, z["p_lex"])
    assert fmt_pdat(p) == open(os.path.join(golden, "a4_p.dat")).read()


@pytest.mark.parametrize("n,iters", [(50, 676), (64, 1061)])
def test_tiled_iteration_counts(n, iters):
    p, rhs = orc.poisson_init(n, n)
    want = p.copy()
    it_ref, _ = orc.solve_lex(want, rhs, 1.0 / n, 1.0 / n, 1.9, 1e-6, 1000000, xorder=0)
    with M.Grid(n, n, 1.0 / n, 1.0 / n, 1.9, 1e-6, 1000000) as g:
        tiled(g)
        g.poisson_init(1.0, 1.0, 2)
        it, _ = g.solve_lex(M.LEX_A4)
        assert it == it_ref == iters
        assert np.array_equal(g.download(M.P), want)


def test_tiled_dispatch():
    with M.Grid(100, 100, 0.01, 0.01, 1.9, 1e-6, 10) as g:
        assert g.get_tuning(M.TUNE_LEX_TILED) == 0  # below the threshold: one workgroup
        g.set_tuning(M.TUNE_LEX_TILED, 1)
        assert g.get_tuning(M.TUNE_LEX_TILED) == 1
        g.set_tuning(M.TUNE_LEX_TILED, -1)
        assert g.get_tuning(M.TUNE_LEX_TILED) == 0
        # tile + halo + rhs beyond LDS; the setting before it stays
        g.set_tuning(M.TUNE_LEX_TILE_W, 64)
        with pytest.raises(M.MisorError):
            g.set_tuning(M.TUNE_LEX_TILE_H, 512)
        with pytest.raises(M.MisorError):
            g.set_tuning(M.TUNE_LEX_TILE_W, 100000)
        assert g.get_tuning(M.TUNE_LEX_TILE_W) == 64
        g.set_tuning(M.TUNE_LEX_TILE_W, 0)
        assert g.get_tuning(M.TUNE_LEX_TILE_W) == g.get_tuning(M.TUNE_LEX_TILE_H)  # default
    # above the measured threshold (512^2 cells), ragged in both directions
    ni, nj = 600, 520
    p, rhs, dx, dy = random_case(ni, nj, 600520)
    want = p.copy()
    it_ref, res_ref = orc.solve_lex(want, rhs, dx, dy, 1.7, 1e-300, 1, xorder=1)
    with M.Grid(ni, nj, dx, dy, 1.7, 1e-300, 1) as g:
        assert g.get_tuning(M.TUNE_LEX_TILED) == 1  # the automatic rule, default tile
        g.upload(M.P, p)
        g.upload(M.RHS, rhs)
        it, res = g.solve_lex(1)
        assert it == it_ref == 1
        assert np.array_equal(g.download(M.P), want)
        assert abs(res - res_ref) <= 1e-12 * abs(res_ref)
        g.set_tuning(M.TUNE_LEX_TILED, 0)
        assert g.get_tuning(M.TUNE_LEX_TILED) == 0


def test_tiled_ns_matches_one_workgroup(golden):
    """the sequential NS on its dcavity.par through the tiled solve (28 tiles)
    against the same run through the one-workgroup kernel: fields and per-step
    iterations equal.  te is cut to a handful of steps (each solve runs into
    itermax = 1000 there; the full 400 steps are tests/test_lex_gpu.py's)"""
    prm = orc.read_par(os.path.join(golden, "seq_dcavity.par"))
    prm["te"] = 0.0008
    out = {}
    for mode in (1, 0):
        g = D.ns_grid(prm)
        if mode:
            tiled(g)
        else:
            g.set_tuning(M.TUNE_LEX_TILED, 0)
        steps, iters, _ = D.run(g, prm, solver="lex")
        out[mode] = (steps, iters, [g.download(f) for f in (M.P, M.U, M.V)])
        g.close()
    assert out[1][0] == out[0][0] >= 3
    assert np.array_equal(out[1][1], out[0][1])
    for a, b in zip(out[1][2], out[0][2]):
        assert np.array_equal(a, b)


def test_exe_poisson_lexicographic_tiled(golden, tmp_path):
    """MISOR_SOLVER=lex on a grid the automatic rule runs tiled: p.dat equals
    the formatted oracle field"""
    ni, nj, k = 600, 520, 3
    txt = open(os.path.join(golden, "a4_poisson.par")).read()
    for key, v in (("imax", ni), ("jmax", nj), ("itermax", k)):
        txt = re.sub(r"(?m)^%s\s+\S+" % key, "%s %d" % (key, v), txt)
    (tmp_path / "poisson.par").write_text(txt)
    env = dict(os.environ, MISOR_SOLVER="lex")
    out = subprocess.run([os.path.join(BIN, "exe-poisson"), "poisson.par"], cwd=tmp_path,
                         env=env, capture_output=True, text=True, timeout=120, check=True).stdout
    assert "Cells (x, y): %d, %d" % (ni, nj) in out
    p, rhs = orc.poisson_init(ni, nj)
    it_ref, _ = orc.solve_lex(p, rhs, 1.0 / ni, 1.0 / nj, 1.9, 1e-6, k, xorder=0)
    assert it_ref == k
    assert (tmp_path / "p.dat").read_text() == fmt_pdat(p)
