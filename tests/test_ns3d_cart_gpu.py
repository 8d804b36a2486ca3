"""The 3D path on the reference's 3D Cartesian process grid (misor3_create_cart,
assignment-6/src/comm.c:24-101, 476-513): ranks as host threads of one process
joined by libmisor's in-process transport (comm_id "LOCAL:<name>") on the test
box's single MI355X.  Everything but the transport -- block storage with the
1-deep halo, the pack / unpack kernels of the x and y faces, global colours and
physical-side flags in the two colour passes, the all-reduced residual and loop
test, the box gather -- is the code the RCCL path runs.

Bar: the gathered fields are bit-identical to the single-domain 3D oracle
(oracle/oracle3d.c, pinned to assignment-6's own build) with the same iteration
counts, for every process grid.
"""
import os
import threading

import numpy as np
import pytest

import orc3
import pymisor as M

pytestmark = pytest.mark.gpu

_gid = [0]
FIELD = {"p": M.P3, "rhs": M.RHS3, "u": M.U3, "v": M.V3, "w": M.W3, "f": M.F3, "g": M.G3,
         "h": M.H3}


def run_ranks(world, fn):
    _gid[0] += 1
    cid = ("LOCAL:c3d%d" % _gid[0]).encode()
    out = [None] * world
    err = []

    def body(r):
        try:
            out[r] = fn(r, cid)
        except BaseException as e:  # surfaced in the main thread
            err.append((r, repr(e)))

    th = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
        assert not t.is_alive(), "rank thread hung"
    assert not err, err
    return out


def params(golden, name, **over):
    prm = orc3.read_par3(os.path.join(golden, name))
    prm.update(over)
    return prm


def world_of(dims):
    return dims[0] * dims[1] * dims[2]


def fits(box, dims):
    return all(box[a] // dims[a] >= 2 for a in range(3))


def block(a, g):
    """the local array of grid g's block (ghost layer included) out of the global array a"""
    o, n = g.off, g.n
    return np.ascontiguousarray(a[o[2]:o[2] + n[2] + 2, o[1]:o[1] + n[1] + 2,
                                  o[0]:o[0] + n[0] + 2])


def slab(a, koff, kloc):
    return np.ascontiguousarray(a[koff:koff + kloc + 2])


# ----------------------------------------------------------------- exchange
def out_axes(shape):
    """per local cell and axis (x, y, z): -1 in the low ghost layer, +1 in the high one"""
    idx = np.indices(shape)  # (k, j, i)
    return [np.where(idx[2 - a] == 0, -1, np.where(idx[2 - a] == shape[2 - a] - 1, 1, 0))
            for a in range(3)]


@pytest.mark.parametrize("dims", [(2, 2, 2), (3, 1, 2), (1, 3, 1), (2, 1, 1)])
def test_exchange_fills_faces_edges_and_corners(dims):
    """the reference's printExchange idea: every cell carries the code of its
    global (i, j, k); the ghost cells of the global array carry code + 0.25, so a
    physical ghost is told from the owned cell next to it.  Before the exchange
    every ghost cell with a rank side among its out-of-block axes holds a
    per-rank sentinel."""
    box = (13, 9, 16)
    prm = dict(imax=box[0], jmax=box[1], kmax=box[2], xlength=1.0, ylength=1.0, zlength=1.0,
               re=100.0, gamma=0.9, tau=0.5, omg=1.7, eps=1e-3, itermax=10, gx=0.0, gy=0.0,
               gz=0.0, bcTop=1, bcBottom=1, bcLeft=1, bcRight=1, bcFront=1, bcBack=1,
               name="dcavity")
    gshape = (box[2] + 2, box[1] + 2, box[0] + 2)
    k, j, i = np.indices(gshape)
    truth = (i + 100.0 * j + 10000.0 * k)
    ghost = (i == 0) | (i == box[0] + 1) | (j == 0) | (j == box[1] + 1) | (k == 0) | \
            (k == box[2] + 1)
    truth = truth + 0.25 * ghost

    def rank(r, cid):
        with M.Grid3(prm, nranks=world_of(dims), rank=r, comm_id=cid, dims=dims) as g:
            assert g.dims == dims
            want = block(truth, g)
            oa = out_axes(want.shape)
            # out-of-block along an axis on a side that faces another rank
            rs = [((oa[a] == -1) & (g.neighbours[2 * a] >= 0)) |
                  ((oa[a] == 1) & (g.neighbours[2 * a + 1] >= 0)) for a in range(3)]
            halo = rs[0] | rs[1] | rs[2]
            nout = sum((o != 0).astype(int) for o in oa)
            start = want.copy()
            start[halo] = -1000.0 - r
            g.upload(M.U3, start)
            g.exchange(M.U3)
            got = g.download(M.U3)
            faces = halo & (nout == 1)
            assert faces.any()
            assert np.array_equal(got[faces], want[faces]), "faces"
            edges = halo & (nout >= 2)
            assert edges.any()
            assert np.array_equal(got[edges], want[edges]), "edge and corner ghosts"
            assert np.array_equal(got[~halo], start[~halo]), "owned cells or physical ghosts"
            return True

    assert all(run_ranks(world_of(dims), rank))


# -------------------------------------------------------------------- solve
SOLVE_BOXES = [((13, 9, 16), 7), ((130, 37, 29), 4), ((7, 5, 6), 5)]
SOLVE_DIMS = [(2, 2, 2), (1, 2, 2), (2, 1, 1), (1, 1, 3), (3, 2, 1)]
SOLVE_CASES = [(b, it, d) for b, it in SOLVE_BOXES for d in SOLVE_DIMS if fits(b, d)]
SOLVE_CASES.append(((7, 5, 6), 5, (3, 2, 3)))  # 2-cell blocks: every cell next to a halo


@pytest.mark.parametrize("box,itermax,dims", SOLVE_CASES)
def test_solve_fixed_iterations_partition_independent(golden, box, itermax, dims):
    prm = params(golden, "a6_dcavity.par", imax=box[0], jmax=box[1], kmax=box[2],
                 eps=1e-150, itermax=itermax)
    shape = (box[2] + 2, box[1] + 2, box[0] + 2)
    rng = np.random.default_rng(sum(box) + world_of(dims))
    p0, rhs = rng.standard_normal(shape), rng.standard_normal(shape)
    ns = orc3.NS3(prm)
    ns.p[...] = p0
    ns.rhs[...] = rhs
    it_ref, res_ref = ns.solve()
    world = world_of(dims)

    def rank(r, cid):
        with M.Grid3(prm, nranks=world, rank=r, comm_id=cid, dims=dims) as g:
            g.upload(M.P3, block(p0, g))
            g.upload(M.RHS3, block(rhs, g))
            it, res = g.solve()
            return it, res, g.gather(M.P3)

    out = run_ranks(world, rank)
    assert all(o[0] == it_ref == itermax for o in out)
    assert np.array_equal(out[0][2], ns.p)
    for o in out:
        print("res", o[1], "oracle", res_ref, "rel", abs(o[1] - res_ref) / res_ref)
        assert o[1] == pytest.approx(res_ref, rel=1e-12)

    if dims[0] == 1 and dims[1] == 1:  # the slab path cuts the same planes

        def slab_rank(r, cid):
            with M.Grid3(prm, nranks=world, rank=r, comm_id=cid) as g:
                g.upload(M.P3, slab(p0, g.koff, g.kloc))
                g.upload(M.RHS3, slab(rhs, g.koff, g.kloc))
                g.solve()
                return g.gather(M.P3)

        assert np.array_equal(run_ranks(world, slab_rank)[0], out[0][2])


def test_solve_epilogue_counts_on_2x1x1(golden):
    """what the Cartesian schedule does after its loop (test_ns3d_gpu.py's
    test_solve_epilogue_counts_every_schedule_alike, same box and solves): two
    timed 5-iteration solves leave every rank's counters at 10 iterations"""
    prm = params(golden, "a6_dcavity.par", imax=12, jmax=9, kmax=7, eps=0.0, itermax=5)
    rng = np.random.default_rng(28)
    p0, rhs = rng.standard_normal((9, 11, 14)), rng.standard_normal((9, 11, 14))
    ns = orc3.NS3(prm)
    ns.p[...] = p0
    ns.rhs[...] = rhs
    ref = [ns.solve(), ns.solve()]

    def rank(r, cid):
        with M.Grid3(prm, nranks=2, rank=r, comm_id=cid, dims=(2, 1, 1)) as g:
            g.upload(M.P3, block(p0, g))
            g.upload(M.RHS3, block(rhs, g))
            g.enable_timing(True)
            solves = [g.solve(), g.solve()]
            return solves, g.solve_time(), g.gather(M.P3)

    out = run_ranks(2, rank)
    for solves, (ms, its), _ in out:
        print("solves", solves, "oracle", ref, "solve_time", ms, its)
        assert [s[0] for s in solves] == [s[0] for s in ref] == [5, 5]
        assert its == 10 and ms > 0.0
        assert [s[1] for s in solves] == [s[1] for s in out[0][0]]  # the all-reduced residual
        for s, s_ref in zip(solves, ref):
            assert s[1] == pytest.approx(s_ref[1], rel=1e-12)
    assert np.array_equal(out[0][2], ns.p)


@pytest.mark.parametrize("dims", [(2, 2, 2), (1, 2, 2)])
def test_solve_converges_partition_independent(golden, dims):
    """the 33^3 fixture of the slab test (seed 11, eps 1e-4, two consecutive
    solves).  Checked on the CPU with the oracle (its res after m iterations for
    every m up to the count, both solves): seed 11 stops after 169 and 2
    iterations, and the res nearest to eps^2 = 1e-8 on the way is iteration
    168's 1.00168e-8, a relative 1.7e-3 away (second solve: 9.72e-9, 2.8e-2) --
    none lies within relative 1e-9 of it, so the count cannot hinge on the
    order in which r^2 is summed.  The seed is unchanged."""
    prm = params(golden, "a6_dcavity.par", imax=33, jmax=33, kmax=33, eps=1e-4, itermax=5000)
    shape = (35, 35, 35)
    rng = np.random.default_rng(11)
    p0, rhs = rng.standard_normal(shape) * 1e-3, rng.standard_normal(shape) * 1e-3
    ns = orc3.NS3(prm)
    ns.p[...] = p0
    ns.rhs[...] = rhs
    it_ref, _ = ns.solve()
    it2_ref, _ = ns.solve()
    world = world_of(dims)

    def rank(r, cid):
        with M.Grid3(prm, nranks=world, rank=r, comm_id=cid, dims=dims) as g:
            g.upload(M.P3, block(p0, g))
            g.upload(M.RHS3, block(rhs, g))
            it, _ = g.solve()
            it2, _ = g.solve()
            return it, it2, g.gather(M.P3)

    out = run_ranks(world, rank)
    assert 1 < it_ref < 5000
    assert all(o[0] == it_ref and o[1] == it2_ref for o in out)
    assert np.array_equal(out[0][2], ns.p)


# ----------------------------------------------------------------- NS steps
def run_steps(prm, dims, steps):
    world = world_of(dims)

    def rank(r, cid):
        with M.Grid3(prm, nranks=world, rank=r, comm_id=cid, dims=dims) as g:
            for f, v in ((M.U3, prm["u_init"]), (M.V3, prm["v_init"]), (M.W3, prm["w_init"]),
                         (M.P3, prm["p_init"])):
                g.fill(f, v)
            g.set_dt(prm["dt"])
            iters, t = [], 0.0
            for _ in range(steps):
                dt = g.compute_timestep() if prm["tau"] > 0.0 else prm["dt"]
                for fn in ("set_boundary_conditions", "set_special_boundary_condition",
                           "compute_fg", "compute_rhs"):
                    g.call(fn)
                iters.append(g.solve()[0])
                g.call("adapt_uvw")
                t += dt
            fields = {n: g.gather(FIELD[n]) for n in ("p", "u", "v", "w")}
            return iters, t, fields

    return run_ranks(world, rank)


_oracle_runs = {}


def oracle_steps(golden, name, box):
    """8 steps of the single-domain oracle, computed once per problem"""
    if name not in _oracle_runs:
        prm = params(golden, name, imax=box[0], jmax=box[1], kmax=box[2])
        ns = orc3.NS3(prm)
        _, iters, t = ns.run(max_steps=8)
        _oracle_runs[name] = (prm, ns, list(iters), t)
    return _oracle_runs[name]


@pytest.mark.parametrize("dims", [(2, 2, 2), (1, 2, 2), (2, 1, 1), (3, 2, 1)])
@pytest.mark.parametrize("name,box", [("a6_dcavity.par", (24, 20, 16)),
                                      ("a6_canal.par", (40, 12, 12))])
def test_ns_steps_partition_independent(golden, dims, name, box):
    """assignment-6/src/main.c:45-60 on a process grid: every field of every step
    as the single-domain oracle's run, bit for bit -- the lid over the global
    i, k ranges on the top ranks, the inflow on the left ranks only, F / G / H
    from the low neighbour, the edge ghosts computeFG reads"""
    prm, ns, iters_ref, t_ref = oracle_steps(golden, name, box)
    out = run_steps(prm, dims, 8)
    for iters, t, _ in out:
        assert iters == iters_ref and t == t_ref
    for k in ("p", "u", "v", "w"):
        assert np.array_equal(out[0][2][k], getattr(ns, k)), k


def test_reference_fixture_on_2x2x2(golden):
    """the committed 16-step run of the reference itself, on 2 x 2 x 2 ranks"""
    ref = np.load(os.path.join(golden, "ns3d_dcavity_short.npz"))
    d = [int(x) for x in ref["dims"]]
    prm = params(golden, "a6_dcavity.par", imax=d[0], jmax=d[1], kmax=d[2])
    out = run_steps(prm, (2, 2, 2), int(ref["steps"]))
    assert out[0][0] == list(ref["iters"]) and out[0][1] == ref["t"]
    for k in ("p", "u", "v", "w"):
        assert np.array_equal(out[0][2][k], ref[k]), k


def test_normalize_and_timestep(golden):
    """the slab test's setup on 2 x 1 x 2 ranks.  The |w| maximum sits in a
    physical corner ghost of the global array; a larger value is planted in the
    x halo of rank 0's local array only -- a cell of the global array that rank 1
    owns, where it holds the field's value -- and must not enter the maximum."""
    prm = params(golden, "a6_canal.par", imax=20, jmax=10, kmax=12)
    dims = (2, 1, 2)
    shape = (14, 12, 22)
    rng = np.random.default_rng(3)
    st = {n: rng.standard_normal(shape) for n in orc3.FIELDS}
    st["w"][13, 11, 21] = 7.5  # the corner ghost (imax+1, jmax+1, kmax+1)
    ns = orc3.NS3(prm)
    for n in orc3.FIELDS:
        getattr(ns, n)[...] = st[n]
    ns.call("compute_timestep")
    ns.call("normalize_pressure")
    assert np.abs(st["w"]).max() == 7.5

    def rank(r, cid):
        with M.Grid3(prm, nranks=4, rank=r, comm_id=cid, dims=dims) as g:
            for n in orc3.FIELDS:
                a = block(st[n], g)
                if n == "w" and r == 0:
                    assert g.neighbours[1] == 1
                    a[3, 4, g.n[0] + 1] = 99.0  # stale copy of a cell owned by rank 1
                g.upload(FIELD[n], a)
            dt = g.compute_timestep()
            mx = g.max_uvw()
            g.call("normalize_pressure")
            return dt, mx, g.gather(M.P3)

    out = run_ranks(4, rank)
    for dt, mx, _ in out:
        assert dt == ns.s.dt
        assert mx == tuple(np.abs(st[n]).max() for n in ("u", "v", "w"))
    err = np.abs(out[0][2] - ns.p).max()
    print("normalize: max |p - oracle|", err, "bound", 1e-14 * np.abs(ns.p).max())
    assert np.allclose(out[0][2], ns.p, rtol=0, atol=1e-14 * np.abs(ns.p).max())


# ---------------------------------------------------------- knobs and errors
def test_knobs_errors_and_round_trip(golden):
    prm = params(golden, "a6_dcavity.par", imax=9, jmax=8, kmax=8)
    dims = (2, 1, 2)

    def rank(r, cid):
        with M.Grid3(prm, nranks=4, rank=r, comm_id=cid, dims=dims) as g:
            assert g.get_tuning(M.TUNE3_SWEEP) == 0
            assert g.get_tuning(M.TUNE3_RESIDENT) == 0
            with pytest.raises(M.MisorError, match="Cartesian"):
                g.set_tuning(M.TUNE3_SWEEP, 1)
            with pytest.raises(M.MisorError, match="Cartesian"):
                g.set_tuning(M.TUNE3_RESIDENT, 1)
            g.set_tuning(M.TUNE3_SWEEP, 0)
            g.set_tuning(M.TUNE3_ROWS, 4)  # accepted, ignored
            g.set_tuning(M.TUNE3_KCHUNK, 4)
            assert g.get_tuning(M.TUNE3_SWEEP) == 0
            loc = M.decompose3_cart(4, r, 9, 8, 8, dims=dims)
            assert (g.n, g.off, g.coords, g.neighbours) == (
                tuple(loc.n), tuple(loc.off), tuple(loc.coords), tuple(loc.neighbours))
            assert (g.kloc, g.koff) == (g.n[2], g.off[2])
            assert g.shape == (g.n[2] + 2, g.n[1] + 2, g.n[0] + 2)
            a = np.random.default_rng(r).standard_normal(g.shape)
            g.upload(M.F3, a)
            assert np.array_equal(g.download(M.F3), a)
        return True

    assert all(run_ranks(4, rank))


def test_create_rejects_a_process_grid_of_another_size(golden):
    prm = params(golden, "a6_dcavity.par", imax=8, jmax=8, kmax=8)
    with pytest.raises(M.MisorError, match="does not hold 4 ranks"):
        M.Grid3(prm, nranks=4, rank=0, comm_id=b"LOCAL:c3d-bad", dims=(2, 2, 2))
    with pytest.raises(M.MisorError, match="along x"):
        M.Grid3(dict(prm, imax=3), nranks=2, rank=0, comm_id=b"LOCAL:c3d-bad2", dims=(2, 1, 1))


def test_one_rank_cart_is_the_single_domain(golden):
    """misor3_create_cart with nranks <= 1 is misor3_create: the fused sweep stays"""
    prm = params(golden, "a6_dcavity.par", imax=8, jmax=8, kmax=8)
    with M.Grid3(prm, dims=(0, 0, 0)) as g:
        assert g.get_tuning(M.TUNE3_SWEEP) == 1
        assert g.dims == (1, 1, 1) and g.n == (8, 8, 8) and g.neighbours == (-1,) * 6
        g.exchange(M.P3)  # a no-op
