"""misor3_solve_mg_dist / Grid3.solve_mg_dist: the 3D multigrid V-cycle on a
grid decomposed into slabs (include/misor.h, DESIGN.md "Geometric multigrid,
3D, decomposed"), ranks as host threads over the in-process transport on one
GPU.

The oracle is tests/mg3_oracle.py on the whole domain.  Every count is fixed
(desc.eps = 0 with maxcycles = n, eps_coarse = 0 with itermax_coarse = k), so
no loop test can differ in a last bit, and p is compared with == three ways: on
every rank's whole downloaded slab (planes 0 .. kloc + 1, the halo included), on
rank 0's gather, and against the single-rank Grid3.solve_mg.  res is the same
bits on every rank and within a relative 1e-12 of the oracle's figure (another
summation order), as tests/test_mg3_gpu.py computes it."""
import numpy as np
import pytest

import mg3_oracle as O
import pymisor as M
from test_mg3_gpu import TD, TH, TW, data
from test_ns3d_decomposed_gpu import run_ranks, slab

pytestmark = pytest.mark.gpu

_oracle = {}


def oracle(shape, lengths, cycles, **kw):
    """(p, cycles, res, levels) of the whole domain; computed once, read-only"""
    key = (shape, lengths, cycles, tuple(sorted(kw.items())))
    if key not in _oracle:
        p0, rhs = data(shape)
        out = O.solve(p0, rhs, lengths, eps=0.0, maxcycles=cycles, **kw)
        out[0].setflags(write=False)
        _oracle[key] = out
    return _oracle[key]


def single_rank(shape, lengths, cycles, **kw):
    p0, rhs = data(shape)
    q = dict(O.DEFAULTS, **kw)
    with M.Grid3(O.make_prm(shape, lengths, eps=0.0, omg=1.9, itermax=10)) as g:
        g.upload(M.P3, p0)
        g.upload(M.RHS3, rhs)
        n, res = g.solve_mg(maxcycles=cycles, **q)
        return g.download(M.P3), n, res, g.mg_info()


def dist_solve(world, shape, lengths, cycles, gather_cells, **kw):
    p0, rhs = data(shape)
    q = dict(O.DEFAULTS, **kw)
    prm = O.make_prm(shape, lengths, eps=0.0, omg=1.9, itermax=10)  # omg, itermax: not used

    def rank(r, cid):
        with M.Grid3(prm, device=0, nranks=world, rank=r, comm_id=cid) as g:
            g.upload(M.P3, slab(p0, g.koff, g.kloc))
            g.upload(M.RHS3, slab(rhs, g.koff, g.kloc))
            n, res = g.solve_mg_dist(gather_cells=gather_cells, maxcycles=cycles, **q)
            return n, res, g.download(M.P3), g.gather(M.P3), g.mg_info(), g.koff, g.kloc

    return run_ranks(world, rank)


def check(world, shape, lengths, cycles, gather_cells=0, **kw):
    want, n_ref, res_ref, nlev = oracle(shape, lengths, cycles, **kw)
    out = dist_solve(world, shape, lengths, cycles, gather_cells, **kw)
    cc = dict(O.DEFAULTS, **kw)["coarse_cells"]
    plan = M.mg3_dist_levels(world, *shape, coarse_cells=cc, gather_cells=gather_cells)
    assert plan[0] == nlev
    for r, (n, res, mine, _, info, koff, kloc) in enumerate(out):
        assert n == cycles == n_ref and info["cycles"] == cycles
        assert (info["levels"], info["dist_levels"]) == plan, (r, info, plan)
        ref = slab(want, koff, kloc)
        bad = np.argwhere(mine != ref)  # planes 0 .. kloc + 1: the halo is current
        assert bad.size == 0, (r, len(bad), bad[:5], np.abs(mine - ref).max())
        assert res == out[0][1]  # the same bits on every rank
    got = out[0][3]
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5], np.abs(got - want).max())
    res = out[0][1]
    print("res", res, "oracle", res_ref, "plan", plan)
    assert abs(res - res_ref) <= 1e-12 * abs(res_ref), (res, res_ref)
    p1, n1, _, _ = single_rank(shape, lengths, cycles, **kw)
    assert n1 == cycles and np.array_equal(got, p1)
    return got, plan


SMALL = dict(coarse_cells=1, itermax_coarse=5)
UNIT = (1.0, 1.0, 1.0)


@pytest.mark.parametrize("nu1,nu2", [(2, 2), (1, 0), (0, 1)])
def test_two_distributed_levels_and_one_gathered(nu1, nu2):
    """8 x 8 x 16 on 2 ranks.  (0, 1) needs the exchange of p before the
    restriction, (1, 0) the closing exchange"""
    _, plan = check(2, (8, 8, 16), (1.0, 0.5, 0.75), 2, nu1=nu1, nu2=nu2, **SMALL)
    assert plan == (3, 2)


@pytest.mark.parametrize("gather_cells,ndist", [(0, 3), (10 ** 9, 1)])
def test_coarsest_level_distributed_or_gathered_from_level_0(gather_cells, ndist):
    _, plan = check(2, (8, 8, 32), UNIT, 2, gather_cells=gather_cells, **SMALL)
    assert plan == (3, ndist)


@pytest.mark.parametrize("world,kmax", [(3, 24), (4, 32), (8, 64)])
def test_middle_ranks_face_a_rank_on_both_sides(world, kmax):
    _, plan = check(world, (8, 8, kmax), UNIT, 2, **SMALL)
    assert plan == (3, 2)


# slabs of 36 planes on 2 ranks, longer than two march chunks of the coarse tile,
# ragged in x, y and z against it
RAGGED = (TW + 4, TH + 4, 2 * (2 * TD + 4))  # 132 x 20 x 72 with the 64 x 8 x 8 coarse tile


@pytest.mark.parametrize("gather_cells", [0, 10 ** 9])
@pytest.mark.parametrize("k", [0, 3])
def test_ragged_slabs_two_levels(k, gather_cells):
    """one pre-smoothing iteration, the transfers, no post-smoothing: with
    itermax_coarse = 0 the correction is prolong(0) and p must be the smoothed
    field"""
    shape = RAGGED
    cc = (shape[0] // 2) * (shape[1] // 2) * (shape[2] // 2)
    assert len(O.levels_rule(*shape, cc)) == 2
    got, plan = check(2, shape, (1.0, 0.4, 0.3), 1, gather_cells=gather_cells, nu1=1, nu2=0,
                      itermax_coarse=k, coarse_cells=cc)
    assert plan == (2, 2 if gather_cells == 0 else 1)
    if k == 0:
        p0, rhs = data(shape)
        sm = p0.copy()
        O.solve_orc(sm, rhs, shape, (1.0, 0.4, 0.3), 1.0, 0.0, 1)
        assert np.array_equal(got, sm)


def test_one_rank_is_solve_mg():
    shape, lengths = (32, 16, 24), (1.0, 0.5, 0.75)
    p0, rhs = data(shape)
    q = dict(O.DEFAULTS, coarse_cells=1, itermax_coarse=5)
    out = []
    for fn in ("solve_mg", "solve_mg_dist"):
        with M.Grid3(O.make_prm(shape, lengths, eps=0.0, omg=1.9, itermax=10)) as g:
            g.upload(M.P3, p0)
            g.upload(M.RHS3, rhs)
            n, res = getattr(g, fn)(maxcycles=2, **q)
            info = g.mg_info()
            assert info["dist_levels"] == 0
            out.append((n, res, g.download(M.P3),
                        {k: v for k, v in info.items() if not k.endswith("_ms")}))
    assert out[0][0] == out[1][0] == 2 and out[0][1] == out[1][1]
    assert np.array_equal(out[0][2], out[1][2]) and out[0][3] == out[1][3]


def test_defaults_converge():
    """rhs = cos(2 pi x) cos(2 pi y) cos(2 pi z) at 64^3, p0 = 0, eps 1e-5, every
    default, 4 ranks.  DESIGN.md "Geometric multigrid, 3D": the single-rank solve
    takes 6 cycles and leaves a full residual of 1.24e-11 against eps^2 = 1e-10;
    p is the same bits, res can differ in its last bits"""
    n, eps, world = 64, 1e-5, 4
    p0, rhs = O.cosine_problem(n)
    prm = O.make_prm((n,) * 3, (1.0,) * 3, eps=eps, omg=1.8, itermax=100000)

    def rank(r, cid):
        with M.Grid3(prm, device=0, nranks=world, rank=r, comm_id=cid) as g:
            g.upload(M.P3, slab(p0, g.koff, g.kloc))
            g.upload(M.RHS3, slab(rhs, g.koff, g.kloc))
            cycles, res = g.solve_mg_dist()
            return cycles, res, g.gather(M.P3), g.mg_info()

    out = run_ranks(world, rank)
    cycles, res, p_mg, info = out[0]
    assert all(o[0] == cycles and o[1] == res for o in out)
    full = np.mean(O.residual(p_mg, rhs, (n,) * 3, (1.0,) * 3) ** 2)
    print("cycles", cycles, "res", res, "full residual", full, "info", info)
    assert (info["levels"], info["dist_levels"]) == M.mg3_dist_levels(world, n, n, n)
    assert abs(cycles - 6) <= 1, cycles
    assert res < eps * eps, res
    assert full < eps * eps, full


def test_refusals_leave_no_rank_waiting():
    """odd slabs -> -5 on every rank, bad parameters -> -1 first, a Cartesian grid
    -> -5; every rank refuses from the same arithmetic before any collective, so
    no thread hangs (run_ranks asserts that)"""
    prm = O.make_prm((8, 8, 10), UNIT, eps=1e-6)

    def expect(g, code, **kw):
        with pytest.raises(M.MisorError, match="error %d.*misor3_solve_mg_dist" % code):
            g.solve_mg_dist(**kw)

    def odd(r, cid):
        with M.Grid3(prm, device=0, nranks=2, rank=r, comm_id=cid) as g:
            expect(g, -5, coarse_cells=1)
            expect(g, -1, coarse_cells=1, maxcycles=-1)
            expect(g, -1, nu1=0, nu2=0)
        return True

    assert all(run_ranks(2, odd))
    prm16 = O.make_prm((16, 16, 16), UNIT, eps=1e-6)

    def cart(r, cid):
        with M.Grid3(prm16, device=0, nranks=2, rank=r, comm_id=cid, dims=(1, 1, 2)) as g:
            expect(g, -5)
            expect(g, -1, maxcycles=-1)
        return True

    assert all(run_ranks(2, cart))
    assert M.lib().misor3_solve_mg_dist(None, None, -1, None, None) == -1


def test_solve_afterwards_is_a_fresh_grids():
    """on 2 ranks a fixed-iteration solve() after one solve_mg_dist cycle gives
    the bits and the iteration count of a fresh grid"""
    shape, lengths = (16, 12, 16), UNIT
    p0, rhs = data(shape)
    prm = O.make_prm(shape, lengths, eps=1e-300, omg=1.8, itermax=5)

    def five(g):
        g.upload(M.P3, slab(p0, g.koff, g.kloc))
        g.upload(M.RHS3, slab(rhs, g.koff, g.kloc))
        it, res = g.solve()
        return it, res, g.download(M.P3)

    def fresh(r, cid):
        with M.Grid3(prm, device=0, nranks=2, rank=r, comm_id=cid) as g:
            return five(g)

    def after(r, cid):
        with M.Grid3(prm, device=0, nranks=2, rank=r, comm_id=cid) as g:
            g.upload(M.P3, slab(p0, g.koff, g.kloc))
            g.upload(M.RHS3, slab(rhs, g.koff, g.kloc))
            n, _ = g.solve_mg_dist(gather_cells=0, maxcycles=1, coarse_cells=1, itermax_coarse=10)
            assert n == 1 and g.mg_info()["dist_levels"] == 2
            return five(g)

    a, b = run_ranks(2, fresh), run_ranks(2, after)
    want = p0.copy()
    it_ref, res_ref = O.solve_orc(want, rhs, shape, lengths, 1.8, 1e-300, 5)
    for r in range(2):
        assert a[r][0] == b[r][0] == it_ref == 5
        assert a[r][1] == b[r][1]  # the same bits
        assert abs(a[r][1] - res_ref) <= 1e-12 * res_ref
        assert np.array_equal(a[r][2], b[r][2])
