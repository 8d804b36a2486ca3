"""The NS step functions one at a time on a decomposed grid, on random states
with every boundary type on the physical sides: 3D slabs, the 3D Cartesian
process grid and the 2D decomposition, ranks as host threads joined by
libmisor's in-process transport.

One global random state is given to the single-domain oracle and, block by
block, to the ranks, so a rank's halos hold its neighbours' true values.  Then
setBoundaryConditions, setSpecialBoundaryCondition, computeFG, computeRHS and
adaptUV run in sequence on both, and after each the fields it writes are
compared bit for bit: the gathered global array with every physical ghost (3D),
or every rank's owned cells and physical ghost cells (2D).  The copies of a
neighbour's cells in a rank's halo are not compared.  This is what checks the
per-rank physical-side masks of the boundary kernels (xlo_phys ... / wall_*)
with slip, outflow and periodic sides, the lid and the inflow under them, and
the ghost cells where a physical face meets a rank's halo.

Parameters: set `all` of tests/ns_param_sets.py (forces on every axis, gamma
0.37, another re and box), which the CPU guard shows the oracle to depend on.
"""
import itertools
import zlib

import numpy as np
import pytest

import ns_gpu_driver as D
import ns_param_sets as PS
import orc
import orc3
import pymisor as M
from test_decomposed_gpu import assemble, local_window
from test_decomposed_gpu import run_ranks as run_ranks2
from test_ns3d_cart_gpu import block, run_ranks, slab, world_of
from test_ns3d_gpu import BC_KEYS, BCS, GPU_FIELD

pytestmark = pytest.mark.gpu

DT = 0.0137
BOX3 = (13, 9, 16)
# (oracle name, C ABI name, fields it writes)
STEPS3 = [("set_bc", "set_boundary_conditions", "uvw"),
          ("set_special_bc", "set_special_boundary_condition", "u"),
          ("compute_fg", "compute_fg", "fgh"),
          ("compute_rhs", "compute_rhs", ("rhs",)),
          ("adapt_uvw", "adapt_uvw", "uvw")]
# slabs along k, then process grids: on 2 x 2 x 2 and 3 x 1 x 2 every rank has a
# physical and a rank side on some axis, on 1 x 3 x 1 the middle rank has none
# of the y walls
GRIDS3 = [2, 3, (2, 2, 2), (3, 1, 2), (1, 3, 1)]


def grid3(prm, grid, r, cid):
    if isinstance(grid, int):
        return M.Grid3(prm, nranks=grid, rank=r, comm_id=cid)
    return M.Grid3(prm, nranks=world_of(grid), rank=r, comm_id=cid, dims=grid)


def part3(a, g, grid):
    return slab(a, g.koff, g.kloc) if isinstance(grid, int) else block(a, g)


def oracle3(prm, st, dt):
    ns = orc3.NS3(prm)
    for n in orc3.FIELDS:
        getattr(ns, n)[...] = st[n]
    ns.s.dt = dt
    return ns


@pytest.mark.parametrize("bcs", BCS)
@pytest.mark.parametrize("name", ["a6_dcavity.par", "a6_canal.par"])
@pytest.mark.parametrize("grid", GRIDS3, ids=lambda g: "slab%d" % g if isinstance(g, int)
                         else "cart%dx%dx%d" % g)
def test_step_functions_3d(golden, grid, name, bcs):
    prm = orc3.read_par3(golden + "/" + name)
    prm.update(dict(zip(BC_KEYS, bcs)), imax=BOX3[0], jmax=BOX3[1], kmax=BOX3[2],
               **PS.overrides("all"))
    rng = np.random.default_rng(zlib.crc32(repr((name, bcs)).encode()))
    st = {n: rng.standard_normal((BOX3[2] + 2, BOX3[1] + 2, BOX3[0] + 2)) for n in orc3.FIELDS}
    st["u"] *= 2.0
    ns = oracle3(prm, st, DT)
    want = []
    for fn, _, writes in STEPS3:
        ns.call(fn)
        want.append({n: getattr(ns, n).copy() for n in writes})
    world = grid if isinstance(grid, int) else world_of(grid)

    def rank(r, cid):
        with grid3(prm, grid, r, cid) as g:
            for n in orc3.FIELDS:
                g.upload(GPU_FIELD[n], part3(st[n], g, grid))
            g.set_dt(DT)
            got = []
            for _, fn, writes in STEPS3:
                g.call(fn)
                got.append({n: g.gather(GPU_FIELD[n]) for n in writes})
            got.append({n: g.gather(GPU_FIELD[n]) for n in orc3.FIELDS})
            return got

    got = run_ranks(world, rank)[0]
    for (fn, _, writes), w, g_ in zip(STEPS3, want, got):
        for n in writes:
            bad = np.argwhere(g_[n] != w[n])
            assert len(bad) == 0, "%s: %s differs at %d cells, first (k,j,i) %s" % (
                fn, n, len(bad), bad[:4].tolist())
    for n in orc3.FIELDS:  # and nothing else was touched on the way
        assert np.array_equal(got[-1][n], getattr(ns, n)), n


@pytest.mark.parametrize("grid", [3, (2, 2, 2)], ids=["slab3", "cart2x2x2"])
def test_compute_timestep_3d_last_rank_decides(golden, grid):
    """dz / wmax decides, and the maximum of |w| is a negative value in the last
    owned cell of the last rank"""
    prm = orc3.read_par3(golden + "/a6_canal.par")
    prm.update(imax=BOX3[0], jmax=BOX3[1], kmax=BOX3[2], **PS.overrides("re_len"))
    rng = np.random.default_rng(5)
    st = {n: rng.standard_normal((BOX3[2] + 2, BOX3[1] + 2, BOX3[0] + 2)) for n in orc3.FIELDS}
    st["w"][BOX3[2], BOX3[1], BOX3[0]] = -77.0
    name, val = PS.timestep_winner(prm, [st[n] for n in "uvw"])
    assert name == "dz/wmax"
    ns = oracle3(prm, st, 0.0)
    ns.call("compute_timestep")
    assert ns.s.dt == prm["tau"] * val  # the oracle took this branch
    world = grid if isinstance(grid, int) else world_of(grid)

    def rank(r, cid):
        with grid3(prm, grid, r, cid) as g:
            if r == world - 1:  # the owner of the deciding cell
                assert all(g.off[a] + g.n[a] == BOX3[a] for a in range(3))
            for n in orc3.FIELDS:
                g.upload(GPU_FIELD[n], part3(st[n], g, grid))
            return g.compute_timestep(), g.max_uvw()

    for dt, mx in run_ranks(world, rank):
        assert dt == ns.s.dt
        assert mx == tuple(np.abs(st[n]).max() for n in "uvw")


# ------------------------------------------------------------------------ 2D
FIELDS2 = (("p", M.P), ("rhs", M.RHS), ("u", M.U), ("v", M.V), ("f", M.F), ("g", M.G))
FID2 = dict(FIELDS2)
STEPS2 = [("set_bc", "set_boundary_conditions", "uv"),
          ("set_special_bc", "set_special_boundary_condition", "u"),
          ("compute_fg", "compute_fg", "fg"),
          ("compute_rhs", "compute_rhs", ("rhs",)),
          ("adapt_uv", "adapt_uv", "uv")]
BC2 = list(itertools.product((1, 2, 3), repeat=2))
BOX2 = (131, 77)


def oracle2(prm, st, dt):
    ns = orc.NS(prm)
    for n, _ in FIELDS2:
        getattr(ns, n)[...] = st[n]
    ns.s.dt = dt
    return ns


@pytest.mark.parametrize("lr,bt", [(BC2[k], BC2[(3 * k + 1) % 9]) for k in range(9)])
@pytest.mark.parametrize("name", ["a6_dcavity.par", "a6_canal.par"])
@pytest.mark.parametrize("nranks", [2, 3, 4])
def test_step_functions_2d(golden, nranks, name, lr, bt):
    prm = orc.read_par(golden + "/" + name)
    prm.update(imax=BOX2[0], jmax=BOX2[1], bcLeft=lr[0], bcRight=lr[1], bcBottom=bt[0],
               bcTop=bt[1], **PS.overrides("all", ndim=2))
    rng = np.random.default_rng(zlib.crc32(repr((name, lr, bt)).encode()))
    st = {n: rng.standard_normal((BOX2[1] + 2, BOX2[0] + 2)) for n, _ in FIELDS2}
    ns = oracle2(prm, st, DT)
    want = []
    for fn, _, writes in STEPS2:
        ns.call(fn)
        want.append({n: getattr(ns, n).copy() for n in writes})

    def rank(r, cid, dims):
        g = D.ns_grid(prm, nranks=nranks, rank=r, comm_id=cid)
        with g:
            for n, fid in FIELDS2:
                g.upload(fid, local_window(st[n], g.loc))
            g.set_dt(DT)
            got = []
            for _, fn, writes in STEPS2:
                g.call(fn)
                got.append({n: g.download(FID2[n]) for n in writes})
            got.append({n: g.download(fid) for n, fid in FIELDS2})
            return g.loc, got

    out = run_ranks2(nranks, rank)

    def whole(step, n):  # owned cells and physical ghosts of every rank
        a = assemble([(loc, got[step][n]) for loc, got in out], st[n].shape)
        assert not np.isnan(a).any()
        return a

    for k, (fn, _, writes) in enumerate(STEPS2):
        for n in writes:
            bad = np.argwhere(whole(k, n) != want[k][n])
            assert len(bad) == 0, "%s: %s differs at %d cells, first (j,i) %s" % (
                fn, n, len(bad), bad[:4].tolist())
    for n, _ in FIELDS2:  # and nothing else was touched on the way
        assert np.array_equal(whole(len(STEPS2), n), getattr(ns, n)), n


def test_compute_timestep_2d_last_rank_decides(golden):
    """dy / vmax decides, and the maximum of |v| is a negative value in the last
    owned cell of the last of 4 ranks"""
    prm = orc.read_par(golden + "/a6_canal.par")
    prm.update(imax=BOX2[0], jmax=BOX2[1], **PS.overrides("re_len", ndim=2))
    rng = np.random.default_rng(6)
    st = {n: rng.standard_normal((BOX2[1] + 2, BOX2[0] + 2)) for n, _ in FIELDS2}
    st["v"][BOX2[1], BOX2[0]] = -3000.0
    name, val = PS.timestep_winner(prm, (st["u"], st["v"]), ndim=2)
    assert name == "dy/vmax"
    ns = oracle2(prm, st, 0.0)
    ns.call("compute_timestep")
    assert ns.s.dt == prm["tau"] * val  # the oracle took this branch

    def rank(r, cid, dims):
        with D.ns_grid(prm, nranks=4, rank=r, comm_id=cid) as g:
            if r == 3:  # the owner of the deciding cell
                assert g.loc.ioff + g.loc.ni == BOX2[0] and g.loc.joff + g.loc.nj == BOX2[1]
            for n, fid in FIELDS2:
                g.upload(fid, local_window(st[n], g.loc))
            return g.compute_timestep(ns.s.dtBound, prm["tau"]), g.max_uv()

    for dt, mx in run_ranks2(4, rank):
        assert dt == ns.s.dt
        assert mx == (np.abs(st["u"]).max(), np.abs(st["v"]).max())
