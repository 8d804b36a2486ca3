"""misor_solve_mg / Grid.solve_mg: geometric multigrid V-cycles with the
red-black iteration as smoother (include/misor.h "multigrid", DESIGN.md
"Geometric multigrid").

The oracle is composed here: smoothing and the coarsest solve are orc.solve_rb
(the restatement of solveRB, assignment-4/src/solver.c:179-238), the transfers
are restated in numpy below -- residual in solveRB's own expression and
operation order, restriction, zeroing, prolongation and ghost copy.  numpy's
elementwise operations do not contract, so p is compared bit for bit.  Every
count is fixed (desc.eps = 0 with maxcycles = n, eps_coarse = 0 with
itermax_coarse = k), so no loop test can differ in a last bit; res comes from a
sum in another order and is compared to the relative 1e-12 used everywhere."""
import os
import re
import threading

import numpy as np
import pytest

import orc
import pymisor as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile(name):
    """a tile constant of the transfer kernels as built (csrc/misor_internal.h)"""
    txt = open(os.path.join(ROOT, "practical-parallel-algorithms-with-mpi_amd", "csrc",
                            "misor_internal.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, txt).group(1))


# fine cells one workgroup of the transfer kernels covers: kMgTileW coarse
# columns x kMgTileH coarse rows, two fine cells each way per coarse cell.  Read
# from the source, so the ragged shapes below follow the constants.
TILE_W, TILE_H = 2 * _tile("kMgTileW"), 2 * _tile("kMgTileH")

DEFAULTS = dict(nu1=2, nu2=2, omega_smooth=1.0, coarse_cells=64, omega_coarse=1.7,
                eps_coarse=0.0, itermax_coarse=1000)


# ----------------------------------------------------------------- the oracle

def levels_rule(imax, jmax, coarse_cells):
    out = [(imax, jmax)]
    while not (imax % 2 or jmax % 2 or imax < 4 or jmax < 4 or imax * jmax <= coarse_cells):
        imax, jmax = imax // 2, jmax // 2
        out.append((imax, jmax))
    return out


def ghost_copy(p):  # solver.c:218-226; corners are not touched
    p[0, 1:-1] = p[1, 1:-1]
    p[-1, 1:-1] = p[-2, 1:-1]
    p[1:-1, 0] = p[1:-1, 1]
    p[1:-1, -1] = p[1:-1, -2]


def residual(p, rhs, dx, dy):
    """r = rhs - lap p on the interior, solveRB's expression (solver.c:204-210)"""
    dx2, dy2 = dx * dx, dy * dy
    idx2, idy2 = 1.0 / dx2, 1.0 / dy2
    c = p[1:-1, 1:-1]
    return rhs[1:-1, 1:-1] - ((p[1:-1, 2:] - 2.0 * c + p[1:-1, :-2]) * idx2 +
                              (p[2:, 1:-1] - 2.0 * c + p[:-2, 1:-1]) * idy2)


def restrict(r):
    """rc(I,J) = 0.25 ((r(2I-1,2J-1) + r(2I,2J-1)) + (r(2I-1,2J) + r(2I,2J))), with a
    zero ghost layer"""
    rc = np.zeros((r.shape[0] // 2 + 2, r.shape[1] // 2 + 2))
    rc[1:-1, 1:-1] = 0.25 * ((r[0::2, 0::2] + r[0::2, 1::2]) + (r[1::2, 0::2] + r[1::2, 1::2]))
    return rc


def prolong_correct(p, e):
    """p(i,j) += (9 e(I,J) + 3 (e(I+sx,J) + e(I,J+sy)) + e(I+sx,J+sy)) * 0.0625, parent
    (I,J) = ((i+1)/2, (j+1)/2), sx / sy = -1 for odd, +1 for even i / j, neighbour
    indices clamped to the coarse interior; then p's ghost copy"""
    E = np.pad(e[1:-1, 1:-1], 1, mode="edge")  # the clamp
    c = E[1:-1, 1:-1]
    x = {-1: E[1:-1, :-2], 1: E[1:-1, 2:]}
    y = {-1: E[:-2, 1:-1], 1: E[2:, 1:-1]}
    xy = {(-1, -1): E[:-2, :-2], (1, -1): E[:-2, 2:], (-1, 1): E[2:, :-2], (1, 1): E[2:, 2:]}
    f = p[1:-1, 1:-1]
    for sy, j0 in ((-1, 0), (1, 1)):      # fine rows j = 1, 3, .. / 2, 4, ..
        for sx, i0 in ((-1, 0), (1, 1)):
            f[j0::2, i0::2] += (9.0 * c + 3.0 * (x[sx] + y[sy]) + xy[(sx, sy)]) * 0.0625
    ghost_copy(p)


def oracle_cycle(p, rhs, dx, dy, shapes, q, res):
    """one V-cycle in place on p; returns res as misor_solve_mg defines it"""
    if len(shapes) == 1:
        _, r = orc.solve_rb(p, rhs, dx, dy, q["omega_coarse"], q["eps_coarse"],
                            q["itermax_coarse"])
        return r
    if q["nu1"] > 0:
        _, res = orc.solve_rb(p, rhs, dx, dy, q["omega_smooth"], 0.0, q["nu1"])
    rc = restrict(residual(p, rhs, dx, dy))
    e = np.zeros_like(rc)
    oracle_cycle(e, rc, 2.0 * dx, 2.0 * dy, shapes[1:], q, 1.0)
    prolong_correct(p, e)
    if q["nu2"] > 0:
        _, res = orc.solve_rb(p, rhs, dx, dy, q["omega_smooth"], 0.0, q["nu2"])
    return res


def oracle_solve(p0, rhs, dx, dy, cycles, **kw):
    q = dict(DEFAULTS, **kw)
    ni, nj = p0.shape[1] - 2, p0.shape[0] - 2
    shapes = levels_rule(ni, nj, q["coarse_cells"])
    p, res = p0.copy(), 1.0
    rhs = np.ascontiguousarray(rhs)
    for _ in range(cycles):
        res = oracle_cycle(p, rhs, dx, dy, shapes, q, res)
    return p, res, len(shapes)


_data = {}


def data(ni, nj):
    """standard_normal p and rhs, ghosts included; read-only, shared"""
    if (ni, nj) not in _data:
        rng = np.random.default_rng(7919 * ni + nj)
        _data[(ni, nj)] = (rng.standard_normal((nj + 2, ni + 2)),
                           rng.standard_normal((nj + 2, ni + 2)))
        for a in _data[(ni, nj)]:
            a.setflags(write=False)
    return _data[(ni, nj)]


def gpu_solve(ni, nj, dx, dy, p0, rhs, cycles, **kw):
    q = dict(DEFAULTS, **kw)
    with M.Grid(ni, nj, dx, dy, 1.9, 0.0, 10) as g:  # desc.omega, itermax: not used
        g.upload(M.P, p0)
        g.upload(M.RHS, rhs)
        n, res = g.solve_mg(maxcycles=cycles, **q)
        st = g.stats()
        return g.download(M.P), n, res, st


def check(ni, nj, dx, dy, cycles, **kw):
    p0, rhs = data(ni, nj)
    want, res_ref, nlev = oracle_solve(p0, rhs, dx, dy, cycles, **kw)
    got, n, res, st = gpu_solve(ni, nj, dx, dy, p0, rhs, cycles, **kw)
    assert n == cycles and st["mg_cycles"] == cycles and st["mg_levels"] == nlev
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5], np.abs(got - want).max())
    print("res", res, "oracle", res_ref)
    assert abs(res - res_ref) <= 1e-12 * abs(res_ref), (res, res_ref)
    return got


# ------------------------------------------------------------------ the tests

TRANSFER_SHAPES = [
    (4, 4, 0.25, 0.25),                          # the smallest two-level grid, 4x4 -> 2x2
    # the narrowest coarse grids the rule allows, two coarse columns / two coarse
    # rows (a fine side below 4 is not coarsened), three workgroups tall / wide
    (4, 2 * TILE_H + 4, 0.25, 0.25),
    (2 * TILE_W + 4, 4, 0.01, 0.01),
    # ragged in both directions, more than two tiles each way
    (2 * TILE_W + 6, 2 * TILE_H + 2, 1.0 / (2 * TILE_W + 6), 1.0 / (2 * TILE_H + 2)),
    (40, 24, 1.0 / 40, 0.7 / 24),                # imax != jmax, dx != dy
]


@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("ni,nj,dx,dy", TRANSFER_SHAPES)
def test_transfer_kernels_two_levels(ni, nj, dx, dy, k):
    """one pre-smoothing iteration, the transfers, no post-smoothing: with
    itermax_coarse = 0 the correction is prolong(0) (p must be the smoothed
    field, its ghosts copied), with 3 coarse iterations e != 0"""
    cc = (ni // 2) * (nj // 2)  # level 1 is the coarsest
    assert len(levels_rule(ni, nj, cc)) == 2
    got = check(ni, nj, dx, dy, 1, nu1=1, nu2=0, itermax_coarse=k, coarse_cells=cc)
    if k == 0:
        p0, rhs = data(ni, nj)
        sm = p0.copy()
        orc.solve_rb(sm, np.ascontiguousarray(rhs), dx, dy, 1.0, 0.0, 1)
        assert np.array_equal(got, sm)


@pytest.mark.parametrize("nu1,nu2", [(2, 2), (1, 0), (0, 1), (3, 1)])
def test_four_levels_two_cycles(nu1, nu2):
    """24x16 -> 12x8 -> 6x4 -> 3x2 with coarse_cells small, so tiny grids recurse"""
    assert levels_rule(24, 16, 1) == [(24, 16), (12, 8), (6, 4), (3, 2)]
    check(24, 16, 1.0 / 24, 1.0 / 16, 2, nu1=nu1, nu2=nu2, coarse_cells=1, itermax_coarse=5)


def test_levels_across_kernel_families():
    """192x160 (multi-block passes) -> 96x80 (whole-solve LDS kernel) -> 48x40 (the
    coarsest: 1920 cells)"""
    assert levels_rule(192, 160, 2000) == [(192, 160), (96, 80), (48, 40)]
    check(192, 160, 1.0 / 192, 1.0 / 160, 1, coarse_cells=2000, itermax_coarse=7)


def test_one_level_cycle_is_the_coarsest_solve():
    """7x8 cannot be coarsened: a cycle is solveRB with omega_coarse, capped"""
    check(7, 8, 1.0 / 7, 1.0 / 8, 2, itermax_coarse=4)


def test_hierarchy_rebuilt_when_coarse_cells_changes():
    ni, nj = 48, 32
    p0, rhs = data(ni, nj)
    with M.Grid(ni, nj, 1.0 / ni, 1.0 / nj, 1.9, 0.0, 10) as g:
        for cc, nlev in ((1, 5), (400, 2), (1, 5)):
            g.upload(M.P, p0)
            g.upload(M.RHS, rhs)
            q = dict(DEFAULTS, coarse_cells=cc, itermax_coarse=3)
            g.solve_mg(maxcycles=1, **q)
            want, _, n = oracle_solve(p0, rhs, 1.0 / ni, 1.0 / nj, 1, **q)
            assert n == nlev == g.stats()["mg_levels"]
            assert np.array_equal(g.download(M.P), want), cc


def test_omega_restored():
    """a multigrid solve leaves the grid's own relaxation factor, tolerance and
    plan in force: solve_rb afterwards gives the bits of a fresh grid"""
    ni, nj = 192, 160
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
        assert n == 1
        it_b, res_b, p_b = five(g)
    assert it_a == it_b == 5
    assert res_a == res_b  # the same bits
    assert np.array_equal(p_a, p_b)
    want = p0.copy()
    orc.solve_rb(want, np.ascontiguousarray(rhs), 1.0 / ni, 1.0 / nj, 1.9, 1e-300, 5)
    assert np.array_equal(p_a, want)


def test_set_stream_between_solves():
    """the levels run on the grid's stream and move with it: solve, hand the grid
    another stream, solve again -- the same bits -- then back to a stream of its
    own, the foreign stream destroyed, solve once more and destroy the grid"""
    import torch

    ni, nj = 192, 160
    p0, rhs = data(ni, nj)
    q = dict(DEFAULTS, coarse_cells=2000, itermax_coarse=7)
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
        g.enable_timing(True)         # and the timed path on the moved levels
        p_d, res_d = once(g)
        assert g.stats()["mg_transfers"] == 2
    assert np.array_equal(p_a, want) and abs(res_a - res_ref) <= 1e-12 * res_ref
    for p, r in ((p_b, res_b), (p_c, res_c), (p_d, res_d)):
        assert np.array_equal(p, p_a) and r == res_a


def test_defaults_converge():
    """assignment-4 problem 2 at 256^2, eps 1e-6, every default: res < eps^2 within
    20 cycles (the numpy prototype of this definition takes 10), the full
    residual of the result below eps^2, and the field that of the converged
    red-black solve up to its constant"""
    n, eps = 256, 1e-6
    with M.Grid(n, n, 1.0 / n, 1.0 / n, 1.9, eps, 10 ** 7) as g:
        g.poisson_init(1.0, 1.0, 2)
        rhs = g.download(M.RHS)
        cycles, res = g.solve_mg()
        p_mg = g.download(M.P)
        st = g.stats()
        g.poisson_init(1.0, 1.0, 2)
        it_rb, res_rb = g.solve_rb()
        p_rb = g.download(M.P)
    full = np.mean(residual(p_mg, rhs, 1.0 / n, 1.0 / n) ** 2)
    a, b = p_mg[1:-1, 1:-1], p_rb[1:-1, 1:-1]
    diff = np.abs((a - a.mean()) - (b - b.mean())).max()
    print("cycles", cycles, "res", res, "full residual", full, "levels", st["mg_levels"],
          "| solve_rb iterations", it_rb, "res", res_rb, "| max abs difference", diff)
    assert st["mg_levels"] == 6 and st["mg_cycles"] == cycles  # 256 .. 8
    assert res < eps * eps and cycles <= 20, (cycles, res)
    assert res_rb < eps * eps and it_rb == 13921
    # measured 3.98e-14 against eps^2 = 1e-12: a margin of 25, so eps^2 itself
    assert full < eps * eps, full
    # measured once: 1.72e-8 (DESIGN.md "Geometric multigrid"); neither solve is
    # the other's oracle, both stop at eps -- ten times the measured difference
    assert diff <= 1.72e-7, diff


def test_solve_refuses_rba_and_decomposed_grids():
    with M.Grid(16, 16, 1.0 / 16, 1.0 / 16, 1.7, 1e-6, 10, variant=M.SOLVE_RBA) as g:
        with pytest.raises(M.MisorError, match="error -1.*variant RB"):
            g.solve_mg()
    with M.Grid(16, 16, 1.0 / 16, 1.0 / 16, 1.7, 1e-6, 10) as g:
        for kw in (dict(nu1=0, nu2=0), dict(omega_smooth=0.0), dict(maxcycles=-1)):
            with pytest.raises(M.MisorError, match="error -1"):
                g.solve_mg(**kw)
        with pytest.raises(TypeError):
            g.solve_mg(nu3=1)
        q = g.mg_default_params()
        assert (q.nu1, q.nu2, q.omega_smooth, q.coarse_cells) == (2, 2, 1.0, 64)
        assert (q.omega_coarse, q.eps_coarse, q.itermax_coarse, q.maxcycles) == (
            1.7, 0.1 * 1e-6, 1000, 100)
        assert g.solve_mg(maxcycles=0) == (0, 1.0)  # no cycle: solveRB's initial res
    errs = []

    def body(r):
        try:
            with M.Grid(20, 20, 0.05, 0.05, 1.9, 1e-6, 10, device=0, nranks=2, rank=r,
                        comm_id=b"LOCAL:mgreject") as g:
                try:
                    g.solve_mg()
                    errs.append("accepted")
                except M.MisorError as e:
                    if "error -5" not in str(e):
                        errs.append(str(e))
        except BaseException as e:
            errs.append(repr(e))

    th = [threading.Thread(target=body, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
