"""misor_solve_mg_dist / Grid.solve_mg_dist: the V-cycle of misor_solve_mg on a
decomposed grid (include/misor.h "multigrid", DESIGN.md "Geometric multigrid,
decomposed").

The ranks run as threads of this process over the in-process transport, as in
test_decomposed_gpu.py.  The oracle is test_mg_gpu.py's composed one on the
whole domain; every count is fixed (desc.eps = 0 with maxcycles = n, eps_coarse
= 0 with itermax_coarse = k), so p is compared bit for bit -- on every rank's
whole local window, its exchanged halo included, on the gathered field, and
against the single-rank misor_solve_mg.  res is a sum in another order: the same
bits on every rank, and within the relative 1e-12 used everywhere of the
oracle's."""
import numpy as np
import pytest

import pymisor as M
from test_decomposed_gpu import local_window, run_ranks
from test_mg_gpu import DEFAULTS, TILE_H, TILE_W, data, gpu_solve, levels_rule, oracle_solve
from test_mg_gpu import residual

pytestmark = pytest.mark.gpu

ALL = 10 ** 9  # gather_cells: nothing below level 0 stays distributed


def dist_solve(world, dims, ni, nj, dx, dy, cycles, gather_cells, tail=None, **kw):
    """every rank's (loc, local p, gathered p or None, cycles, res, stats)"""
    p0, rhs = data(ni, nj)
    q = dict(DEFAULTS, **kw)

    def rank_fn(r, cid, dims):
        with M.Grid(ni, nj, dx, dy, 1.9, 0.0, 10, device=0, nranks=world, rank=r, dims=dims,
                    comm_id=cid) as g:
            if tail is not None:
                g.set_tuning(M.TUNE_MG_TAIL, tail)
            g.upload(M.P, local_window(p0, g.loc))
            g.upload(M.RHS, local_window(rhs, g.loc))
            n, res = g.solve_mg_dist(gather_cells, maxcycles=cycles, **q)
            st = g.stats()
            return g.loc, g.download(M.P), g.gather(M.P), n, res, st

    return run_ranks(world, rank_fn, dims)


def check(world, dims, ni, nj, dx, dy, cycles, gather_cells, ndist, tail=None, **kw):
    p0, rhs = data(ni, nj)
    q = dict(DEFAULTS, **kw)
    want, res_ref, nlev = oracle_solve(p0, rhs, dx, dy, cycles, **kw)
    single, _, _, _ = gpu_solve(ni, nj, dx, dy, p0, rhs, cycles, **kw)
    plan = M.mg_dist_levels(world, ni, nj, q["coarse_cells"], gather_cells, dims)
    assert plan == (nlev, ndist), plan
    outs = dist_solve(world, dims, ni, nj, dx, dy, cycles, gather_cells, tail, **kw)
    for r, (loc, p, glob, n, res, st) in enumerate(outs):
        w = local_window(want, loc)
        bad = np.argwhere(p != w)
        assert bad.size == 0, (r, len(bad), bad[:5], np.abs(p - w).max())
        assert n == cycles and st["mg_cycles"] == cycles
        assert (st["mg_levels"], st["mg_dist_levels"]) == plan
        assert res == outs[0][4]  # the same bits on every rank
        print("rank", r, "res", res, "oracle", res_ref)
        assert abs(res - res_ref) <= 1e-12 * abs(res_ref), (res, res_ref)
    glob = outs[0][2]
    assert all(o[2] is None for o in outs[1:])
    assert np.array_equal(glob, want), np.argwhere(glob != want)[:5]
    assert np.array_equal(glob, single)
    return outs


@pytest.mark.parametrize("nu1,nu2", [(2, 2), (1, 0), (0, 1)])
def test_two_distributed_two_gathered_levels(nu1, nu2):
    """16^2 on 2 x 2 ranks: blocks 8^2 and 4^2 distributed, 4^2 and 2^2 gathered;
    every block has a physical corner (clamping) and an inner corner (the corner
    halo of e)"""
    assert levels_rule(16, 16, 1) == [(16, 16), (8, 8), (4, 4), (2, 2)]
    check(4, (0, 0), 16, 16, 1.0 / 16, 1.0 / 16, 2, 0, 2, nu1=nu1, nu2=nu2, coarse_cells=1,
          itermax_coarse=5)


def test_gathered_straight_from_level_0():
    check(4, (0, 0), 16, 16, 1.0 / 16, 1.0 / 16, 2, ALL, 1, coarse_cells=1, itermax_coarse=5)


def test_coarsest_level_distributed():
    """coarse_cells = 64: level 1 (8^2, blocks 4^2) is the coarsest and distributed,
    so the coarsest solve itself is the decomposed one"""
    check(4, (0, 0), 16, 16, 1.0 / 16, 1.0 / 16, 2, 0, 2, coarse_cells=64, itermax_coarse=5)


@pytest.mark.parametrize("dims", [(2, 1), (1, 2)])
def test_two_ranks_either_way(dims):
    check(2, dims, 24, 16, 1.0 / 24, 0.7 / 16, 2, 0, 2, coarse_cells=1, itermax_coarse=5)


def test_eight_ranks():
    """64 x 32 on 4 x 2 ranks: blocks 16^2, 8^2, 4^2 distributed; ranks with two
    and with three neighbouring sides"""
    check(8, (0, 0), 64, 32, 1.0 / 64, 1.0 / 32, 2, 0, 3, coarse_cells=1, itermax_coarse=5)


@pytest.mark.parametrize("gather_cells,ndist", [(0, 2), (ALL, 1)], ids=["dist", "gathered"])
@pytest.mark.parametrize("k", [0, 3])
def test_blocks_beyond_one_transfer_tile(k, gather_cells, ndist):
    """blocks wider and taller than one tile of the transfer kernels and ragged,
    two levels: the coarse blocks span three workgroups each way.  With
    itermax_coarse = 0 the correction is prolong(0)"""
    bi, bj = 2 * TILE_W + 4, 2 * TILE_H + 4
    ni, nj = 2 * bi, 2 * bj
    cc = (ni // 2) * (nj // 2)
    assert len(levels_rule(ni, nj, cc)) == 2
    check(4, (2, 2), ni, nj, 1.0 / ni, 1.0 / nj, 1, gather_cells, ndist, nu1=1, nu2=0,
          itermax_coarse=k, coarse_cells=cc)


def test_one_rank_is_solve_mg():
    ni, nj = 48, 32
    p0, rhs = data(ni, nj)
    q = dict(DEFAULTS, coarse_cells=1, itermax_coarse=5)
    want, n_a, res_a, st_a = gpu_solve(ni, nj, 1.0 / ni, 1.0 / nj, p0, rhs, 2, **q)
    with M.Grid(ni, nj, 1.0 / ni, 1.0 / nj, 1.9, 0.0, 10) as g:
        g.upload(M.P, p0)
        g.upload(M.RHS, rhs)
        n_b, res_b = g.solve_mg_dist(maxcycles=2, **q)
        st_b = g.stats()
        got = g.download(M.P)
    assert (n_b, res_b) == (n_a, res_a) and np.array_equal(got, want)
    assert st_b["mg_dist_levels"] == 0  # nothing is distributed on a grid that is not decomposed
    assert {k: v for k, v in st_a.items() if not k.endswith("_ms")} == \
        {k: v for k, v in st_b.items() if not k.endswith("_ms")}


@pytest.mark.parametrize("gather_cells,ndist,fused", [(ALL, 1, 4), (0, 3, 2)])
def test_fused_tail_inside_the_gathered_cycle(gather_cells, ndist, fused):
    """32^2 on 2 x 2 ranks: the gathered levels (16^2 .. 2^2, or 4^2 and 2^2) all fit
    the LDS of a workgroup, so their cycle is one launch; MISOR_TUNE_MG_TAIL 0
    and 1 give the same bits"""
    assert levels_rule(32, 32, 1) == [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)]
    outs = {}
    for tail in (1, 0):
        outs[tail] = check(4, (0, 0), 32, 32, 1.0 / 32, 1.0 / 32, 2, gather_cells, ndist,
                           tail=tail, coarse_cells=1, itermax_coarse=5)
        assert all(o[5]["mg_tail_levels"] == (fused if tail else 0) for o in outs[tail])
    for a, b in zip(outs[1], outs[0]):
        assert np.array_equal(a[1], b[1]) and a[4] == b[4]


def test_defaults_converge():
    """assignment-4 problem 2 at 256^2, eps 1e-6, every default, 4 ranks: the cycle
    count within one of the single-rank count, res < eps^2 and the full residual
    of the gathered field below eps^2"""
    n, eps = 256, 1e-6
    with M.Grid(n, n, 1.0 / n, 1.0 / n, 1.9, eps, 10 ** 7) as g:
        g.poisson_init(1.0, 1.0, 2)
        cycles1, res1 = g.solve_mg()

    def rank_fn(r, cid, dims):
        with M.Grid(n, n, 1.0 / n, 1.0 / n, 1.9, eps, 10 ** 7, device=0, nranks=4, rank=r,
                    comm_id=cid) as g:
            g.poisson_init(1.0, 1.0, 2)
            rhs = g.gather(M.RHS)
            cycles, res = g.solve_mg_dist()
            return cycles, res, g.gather(M.P), rhs, g.stats()

    outs = run_ranks(4, rank_fn)
    cycles, res, p, rhs, st = outs[0]
    full = np.mean(residual(p, rhs, 1.0 / n, 1.0 / n) ** 2)
    print("cycles", cycles, "single rank", cycles1, "res", res, "single rank", res1,
          "full residual", full, "levels", st["mg_levels"], "distributed", st["mg_dist_levels"])
    assert all((o[0], o[1]) == (cycles, res) for o in outs)
    assert (st["mg_levels"], st["mg_dist_levels"]) == M.mg_dist_levels(4, n, n) == (6, 1)
    assert abs(cycles - cycles1) <= 1, (cycles, cycles1)
    assert res < eps * eps, res
    assert full < eps * eps, full


def test_refusals():
    def odd_blocks(r, cid, dims):
        with M.Grid(18, 16, 1.0 / 18, 1.0 / 16, 1.9, 1e-6, 10, device=0, nranks=2, rank=r,
                    comm_id=cid) as g:
            with pytest.raises(M.MisorError, match="error -5.*odd side"):
                g.solve_mg_dist()
            with pytest.raises(M.MisorError, match="error -1"):  # bad parameters come first
                g.solve_mg_dist(nu1=0, nu2=0)
            for kw in (dict(omega_coarse=0.0), dict(maxcycles=-1), dict(coarse_cells=-1)):
                with pytest.raises(M.MisorError, match="error -1"):
                    g.solve_mg_dist(**kw)
            with pytest.raises(TypeError):
                g.solve_mg_dist(nu3=1)
            return True

    assert run_ranks(2, odd_blocks) == [True, True]

    def rba(r, cid, dims):
        with M.Grid(16, 16, 1.0 / 16, 1.0 / 16, 1.7, 1e-6, 10, variant=M.SOLVE_RBA, device=0,
                    nranks=2, rank=r, comm_id=cid) as g:
            with pytest.raises(M.MisorError, match="error -1.*variant RB"):
                g.solve_mg_dist()
            return True

    assert run_ranks(2, rba) == [True, True]


def test_solve_rb_afterwards_is_a_fresh_grid():
    """a decomposed multigrid solve leaves the grid's own relaxation factor,
    tolerance and plan in force"""
    ni, nj = 192, 160
    p0, rhs = data(ni, nj)

    def rank_fn(mg):
        def fn(r, cid, dims):
            with M.Grid(ni, nj, 1.0 / ni, 1.0 / nj, 1.9, 1e-300, 100, device=0, nranks=4, rank=r,
                        comm_id=cid) as g:
                if mg:
                    g.upload(M.P, local_window(p0, g.loc))
                    g.upload(M.RHS, local_window(rhs, g.loc))
                    n, _ = g.solve_mg_dist(0, maxcycles=1, itermax_coarse=10)
                    assert n == 1
                g.upload(M.P, local_window(p0, g.loc))
                g.upload(M.RHS, local_window(rhs, g.loc))
                it, res = g.solve_rb(5)
                return it, res, g.download(M.P)
        return fn

    for a, b in zip(run_ranks(4, rank_fn(False)), run_ranks(4, rank_fn(True))):
        assert a[0] == b[0] == 5 and a[1] == b[1]
        assert np.array_equal(a[2], b[2])
