"""The fused tail of misor_solve_mg (csrc/mg_tail.hip, DESIGN.md "The fused
tail"): the LDS-resident levels of the hierarchy cycled in one launch, and the
whole solve in one launch where the grid itself fits.

The oracle is test_mg_gpu's composed numpy one.  Counts are fixed (desc.eps = 0,
eps_coarse = 0) unless a test says otherwise, p is compared bit for bit, res to
the relative 1e-12 used everywhere against the oracle (another summation order)
and with == between MISOR_TUNE_MG_TAIL 1 and 0 (the same kernel arithmetic)."""
import numpy as np
import pytest
import torch  # before libmisor.so loads its HIP runtime: test_set_stream_between_fused_solves

import orc
import pymisor as M
from test_mg_gpu import DEFAULTS, data, levels_rule, oracle_cycle, oracle_solve

pytestmark = pytest.mark.gpu


def solve(ni, nj, cycles, tail=1, near=None, eps=0.0, **kw):
    """(p, cycles, res, stats) of one solve_mg on data(ni, nj), dx = 1/ni, dy = 1/nj"""
    p0, rhs = data(ni, nj)
    q = dict(DEFAULTS, **kw)
    with M.Grid(ni, nj, 1.0 / ni, 1.0 / nj, 1.9, eps, 10) as g:
        g.set_tuning(M.TUNE_MG_TAIL, tail)
        assert g.get_tuning(M.TUNE_MG_TAIL) == tail
        if near is not None:
            g.set_tuning(M.TUNE_NEAR_BAND, near)
        g.upload(M.P, p0)
        g.upload(M.RHS, rhs)
        n, res = g.solve_mg(maxcycles=cycles, **q)
        return g.download(M.P), n, res, g.stats()


def check(ni, nj, cycles, **kw):
    """the fused solve against the oracle"""
    p0, rhs = data(ni, nj)
    want, res_ref, nlev = oracle_solve(p0, rhs, 1.0 / ni, 1.0 / nj, cycles, **kw)
    got, n, res, st = solve(ni, nj, cycles, **kw)
    assert n == cycles and st["mg_cycles"] == cycles and st["mg_levels"] == nlev
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5], np.abs(got - want).max())
    print("res", res, "oracle", res_ref)
    assert abs(res - res_ref) <= 1e-12 * abs(res_ref), (res, res_ref)
    return got, res, st


def whole(st):
    """the whole solve was one launch: every level fused, no transfer kernel"""
    assert st["mg_tail_levels"] == st["mg_levels"] >= 2, st
    assert st["mg_tail_launches"] == 1 and st["mg_tail_fallbacks"] == 0, st
    assert st["mg_transfers"] == 0, st


# ------------------------------------------------- 1. whole solve in one launch

@pytest.mark.parametrize("cycles", [1, 3])
def test_whole_solve_smallest(cycles):
    whole(check(4, 4, cycles, coarse_cells=4)[2])


@pytest.mark.parametrize("nu1,nu2", [(2, 2), (1, 0), (0, 1), (3, 1)])
def test_whole_solve_four_levels(nu1, nu2):
    """24x16 .. 3x2: an odd coarse width, pairs with a missing cell"""
    assert levels_rule(24, 16, 1)[-1] == (3, 2)
    whole(check(24, 16, 2, nu1=nu1, nu2=nu2, coarse_cells=1, itermax_coarse=5)[2])


def test_whole_solve_lds_at_its_limit():
    """128^2: 8 pairs per thread, the largest level that fits"""
    assert M.mg_tail(128, 128) == (0, 5)
    whole(check(128, 128, 2, itermax_coarse=7)[2])


@pytest.mark.parametrize("ni,nj", [(126, 4), (4, 126)])
def test_whole_solve_thin(ni, nj):
    """one coarse row / column pair"""
    assert levels_rule(ni, nj, 1) == [(ni, nj), (ni // 2, nj // 2)]
    whole(check(ni, nj, 2, coarse_cells=1, itermax_coarse=5)[2])


def test_coarsest_of_less_than_a_wave():
    """8x8 -> 4x4 -> 2x2: two pairs on the coarsest level, 1022 idle threads"""
    assert levels_rule(8, 8, 1) == [(8, 8), (4, 4), (2, 2)]
    whole(check(8, 8, 2, coarse_cells=1, itermax_coarse=6)[2])


# ---------------------------------------------------- 2. tail below HBM levels

@pytest.mark.parametrize("ni,nj,cycles,kw", [
    (256, 128, 2, dict(itermax_coarse=7)),
    (192, 160, 1, dict(coarse_cells=2000, itermax_coarse=7)),  # 96x80, 48x40 fused
])
def test_tail_below_hbm_levels(ni, nj, cycles, kw):
    assert M.mg_tail(ni, nj, kw.get("coarse_cells", 64))[0] == 1
    _, _, st = check(ni, nj, cycles, **kw)
    assert st["mg_tail_levels"] == st["mg_levels"] - 1 >= 2, st
    assert st["mg_tail_launches"] == cycles and st["mg_tail_fallbacks"] == 0, st


# ------------------------------------------------------------------ 3. the knob

@pytest.mark.parametrize("ni,nj,kw", [
    (24, 16, dict(coarse_cells=1, itermax_coarse=5)),
    (256, 128, dict(itermax_coarse=7)),
])
def test_knob_changes_no_bit(ni, nj, kw):
    p1, n1, r1, s1 = solve(ni, nj, 2, tail=1, **kw)
    p0, n0, r0, s0 = solve(ni, nj, 2, tail=0, **kw)
    assert n0 == n1 == 2 and r0 == r1 and np.array_equal(p0, p1)
    assert s1["mg_tail_launches"] >= 1 and s1["mg_tail_levels"] >= 2
    assert s0["mg_tail_launches"] == 0 and s0["mg_tail_levels"] == 0
    with M.Grid(16, 16, 1.0 / 16, 1.0 / 16, 1.9, 1e-6, 10) as g:
        assert g.get_tuning(M.TUNE_MG_TAIL) == 1  # the default
        with pytest.raises(M.MisorError, match="error -1"):
            g.set_tuning(M.TUNE_MG_TAIL, 2)


# ------------------------------------------------- 4. the loop test in the kernel

def test_loop_runs_in_the_kernel_to_eps():
    """assignment-4 problem 2 at 64^2, eps 1e-6, every default: the kernel runs
    misor_solve_mg's loop and stops where the level-by-level path and the oracle
    stop"""
    n, eps = 64, 1e-6
    out = []
    for tail in (1, 0):
        with M.Grid(n, n, 1.0 / n, 1.0 / n, 1.9, eps, 10 ** 7) as g:
            g.set_tuning(M.TUNE_MG_TAIL, tail)
            g.poisson_init(1.0, 1.0, 2)
            cycles, res = g.solve_mg()
            out.append((cycles, res, g.download(M.P), g.stats()))
    (c1, r1, p1, s1), (c0, r0, p0, _) = out
    p, rhs = orc.poisson_init(n, n, 1.0, 1.0, 2)
    rhs = np.ascontiguousarray(rhs)
    q = dict(DEFAULTS, eps_coarse=0.1 * eps)
    want, res_ref = 0, 1.0
    while res_ref >= eps * eps and want < 100:
        res_ref = oracle_cycle(p, rhs, 1.0 / n, 1.0 / n, levels_rule(n, n, 64), q, res_ref)
        want += 1
    print("cycles", c1, c0, want, "res", r1, r0, res_ref)
    # the oracle on the CPU takes 9 cycles, res 2.31e-13: a factor 4 below eps^2
    assert c1 == c0 == want == 9
    assert r1 == r0 and r1 < eps * eps
    assert np.array_equal(p1, p0)
    assert s1["mg_tail_launches"] == 1 and s1["mg_tail_levels"] == s1["mg_levels"] == 4


# ------------------------------------------------------ 5. near-band hand-back

@pytest.mark.parametrize("ni,nj,kw", [
    (24, 16, dict(coarse_cells=1)),
    (256, 128, dict()),
])
def test_near_band_hands_the_cycle_back(ni, nj, kw):
    """every iteration of the coarsest solve is near its threshold: the kernel
    stops before the first one in each cycle and the host finishes the cycle"""
    kw = dict(kw, eps_coarse=1e-3, itermax_coarse=50)
    p1, n1, r1, s1 = solve(ni, nj, 2, tail=1, near=-30, **kw)
    p0, n0, r0, s0 = solve(ni, nj, 2, tail=0, near=-30, **kw)
    assert n0 == n1 == 2 and r0 == r1 and np.array_equal(p0, p1)
    assert s1["mg_tail_fallbacks"] == 2 and s0["mg_tail_fallbacks"] == 0, (s1, s0)


# ----------------------------------------------------------------- 6. - 8. state

def test_no_cycle_no_launch():
    with M.Grid(64, 64, 1.0 / 64, 1.0 / 64, 1.7, 1e-6, 10) as g:
        assert g.solve_mg(maxcycles=0) == (0, 1.0)
        st = g.stats()
        assert st["mg_tail_launches"] == 0 and st["mg_tail_levels"] == 0


def test_grid_unchanged_by_a_fused_solve():
    """solve_rb after a fused solve gives a fresh grid's bits"""
    ni = nj = 64
    p0, rhs = data(ni, nj)

    def five(g):
        g.upload(M.P, p0)
        g.upload(M.RHS, rhs)
        it, res = g.solve_rb(5)
        return it, res, g.download(M.P)

    with M.Grid(ni, nj, 1.0 / ni, 1.0 / nj, 1.9, 1e-300, 100) as g:
        it_a, res_a, p_a = five(g)
    with M.Grid(ni, nj, 1.0 / ni, 1.0 / nj, 1.9, 1e-300, 100) as g:
        g.upload(M.P, p0)
        g.upload(M.RHS, rhs)
        n, _ = g.solve_mg(maxcycles=1, itermax_coarse=10)
        assert n == 1 and g.stats()["mg_tail_launches"] == 1
        it_b, res_b, p_b = five(g)
    assert it_a == it_b == 5 and res_a == res_b and np.array_equal(p_a, p_b)


def test_set_stream_between_fused_solves():
    ni = nj = 64
    p0, rhs = data(ni, nj)
    q = dict(DEFAULTS, itermax_coarse=7)
    want, res_ref, _ = oracle_solve(p0, rhs, 1.0 / ni, 1.0 / nj, 1, **q)

    def once(g):
        g.upload(M.P, p0)
        g.upload(M.RHS, rhs)
        n, res = g.solve_mg(maxcycles=1, **q)
        assert n == 1
        return g.download(M.P), res

    with M.Grid(ni, nj, 1.0 / ni, 1.0 / nj, 1.9, 0.0, 10) as g:
        p_a, res_a = once(g)          # on the grid's own stream
        s = torch.cuda.Stream()
        g.set_stream(s.cuda_stream)   # its own stream is destroyed here
        p_b, res_b = once(g)
        g.set_stream(None)            # a new own stream
        del s
        torch.cuda.synchronize()
        p_c, res_c = once(g)
        assert g.stats()["mg_tail_ms"] == 0.0
        g.enable_timing(True)
        p_d, res_d = once(g)
        st = g.stats()
        assert st["mg_tail_ms"] > 0.0 and st["mg_tail_launches"] == 4 and st["mg_transfers"] == 0
    assert np.array_equal(p_a, want) and abs(res_a - res_ref) <= 1e-12 * res_ref
    for p, r in ((p_b, res_b), (p_c, res_c), (p_d, res_d)):
        assert np.array_equal(p, p_a) and r == res_a
