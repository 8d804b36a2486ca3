"""misor_mg_dist_levels: how misor_solve_mg_dist splits a hierarchy into
distributed and gathered levels (csrc/mg_dist_plan.h, include/misor.h), against
a restatement of the rule in Python; host-only arithmetic, no GPU."""
import ctypes as C
import itertools

import pytest

import pymisor as M

EINVAL, ESTATE = -1, -5
DEFAULT_GATHER = 65536


def mpi_dims_create(n):
    best = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return (n // best, best)


def levels_rule(imax, jmax, coarse_cells):
    out = [(imax, jmax)]
    while not (imax % 2 or jmax % 2 or imax < 4 or jmax < 4 or imax * jmax <= coarse_cells):
        imax, jmax = imax // 2, jmax // 2
        out.append((imax, jmax))
    return out


def blocks(shape, dims):
    """the set of block shapes sizeOfRank gives the ranks of a level"""
    return {(shape[0] // dims[0] + (shape[0] % dims[0] > cx),
             shape[1] // dims[1] + (shape[1] % dims[1] > cy))
            for cx in range(dims[0]) for cy in range(dims[1])}


def plan_rule(nranks, dims, imax, jmax, coarse_cells, gather_cells):
    """(nlevels, ndist), or ESTATE: the rule of include/misor.h, level by level
    over every rank's block"""
    if gather_cells < 0:
        gather_cells = DEFAULT_GATHER
    dims = dims if dims[0] > 0 else mpi_dims_create(nranks)
    shapes = levels_rule(imax, jmax, coarse_cells)
    even = lambda s: all(bi % 2 == 0 and bj % 2 == 0 for bi, bj in blocks(s, dims))
    if len(shapes) > 1 and not even(shapes[0]):
        return ESTATE
    ndist = 1
    for l in range(1, len(shapes)):
        if not even(shapes[l - 1]):
            break
        halved = {(bi // 2, bj // 2) for bi, bj in blocks(shapes[l - 1], dims)}
        if any(bi < 4 or bj < 4 for bi, bj in halved):
            break
        if any(bi * bj <= gather_cells for bi, bj in halved):
            break
        if l != len(shapes) - 1 and not even(shapes[l]):
            break
        ndist += 1
    return len(shapes), ndist


def lib_plan(nranks, dims, imax, jmax, coarse_cells, gather_cells):
    n, nd = C.c_int(-7), C.c_int(-7)
    d = (C.c_int * 2)(*dims)
    rc = M.lib().misor_mg_dist_levels(nranks, d, imax, jmax, coarse_cells, gather_cells,
                                      C.byref(n), C.byref(nd))
    if rc:
        assert (n.value, nd.value) == (-7, -7)  # outputs untouched
        return rc
    return n.value, nd.value


SHAPES = [(16, 16), (18, 16), (20, 20), (24, 16), (64, 32), (7, 8), (96, 80), (256, 256),
          (1024, 768), (4096, 4096), (1000, 1000), (48, 36), (32768, 32768), (65536, 32768)]
RANKS = [(1, (0, 0)), (2, (0, 0)), (2, (1, 2)), (3, (0, 0)), (4, (0, 0)), (4, (1, 4)),
         (6, (0, 0)), (8, (0, 0)), (8, (2, 4)), (16, (0, 0))]


def test_sweep_against_the_rule():
    seen = set()
    for (imax, jmax), (nranks, dims), cc, gc in itertools.product(
            SHAPES, RANKS, (0, 1, 64, 2000), (-1, 0, 15, 16, 1024, 10 ** 9)):
        d = dims if dims[0] > 0 else mpi_dims_create(nranks)
        if imax // d[0] < 2 or jmax // d[1] < 2:
            assert lib_plan(nranks, dims, imax, jmax, cc, gc) == EINVAL
            continue
        want = plan_rule(nranks, dims, imax, jmax, cc, gc)
        got = lib_plan(nranks, dims, imax, jmax, cc, gc)
        assert got == want, (imax, jmax, nranks, dims, cc, gc, got, want)
        seen.add(want if want == ESTATE else (want[1] == 1, want[1] == want[0]))
    # refusals, nothing below level 0 distributed, everything distributed, and a split
    assert seen >= {ESTATE, (True, False), (False, True), (False, False)}


def test_named_cases():
    # the weak-scaling box: 8 ranks as 4 x 2, blocks 8192 x 16384; with the default
    # gather_cells the halved blocks stay distributed while they hold more than
    # 65536 cells: 256 x 512 at level 5 does, 128 x 256 = 32768 at level 6 does not
    assert M.mg_dist_levels(8, 32768, 32768) == (13, 6)
    assert M.mg_dist_levels(8, 32768, 32768, gather_cells=0) == (13, 12)  # down to 4 x 8
    assert M.mg_dist_levels(4, 7, 8) == (1, 1)          # a grid of one level, odd blocks and all
    with pytest.raises(M.MisorError, match="error -5.*odd side"):
        M.mg_dist_levels(2, 18, 16)                      # 9-wide blocks
    assert M.mg_dist_levels(2, 20, 20, gather_cells=0) == (3, 1)   # level 1: blocks 5 wide
    assert M.mg_dist_levels(4, 16, 16, coarse_cells=1, gather_cells=0) == (4, 2)
    assert M.mg_dist_levels(4, 16, 16, coarse_cells=1, gather_cells=16) == (4, 1)
    assert M.mg_dist_levels(4, 16, 16, coarse_cells=64, gather_cells=0) == (2, 2)
    assert M.mg_dist_levels(8, 64, 32, coarse_cells=1, gather_cells=0) == (5, 3)
    assert M.mg_dist_levels(1, 16, 16, coarse_cells=1, gather_cells=0) == (4, 3)
    # the default is 65536 cells per halved block
    assert M.mg_dist_levels(4, 2048, 2048) == M.mg_dist_levels(4, 2048, 2048, gather_cells=65536)
    assert M.mg_dist_levels(4, 2048, 2048)[1] == 2  # 512^2 blocks stay, 256^2 = 65536 do not
    assert M.mg_dist_levels(4, 2048, 2048, gather_cells=65535)[1] == 3
    assert M.mg_dist_levels(4, 512, 512, gather_cells=4095)[1] == 3  # 64 x 64 = 4096 > 4095
    assert M.mg_dist_levels(4, 512, 512, gather_cells=4096)[1] == 2


def test_bad_arguments():
    L = M.lib()
    a, b = C.c_int(7), C.c_int(7)
    d = (C.c_int * 2)(0, 0)
    ok = (4, d, 64, 64, 64, -1)
    assert L.misor_mg_dist_levels(*ok, C.byref(a), C.byref(b)) == 0
    a.value = b.value = 7
    assert L.misor_mg_dist_levels(*ok, None, C.byref(b)) == EINVAL
    assert L.misor_mg_dist_levels(*ok, C.byref(a), None) == EINVAL
    bad = (C.c_int * 2)(3, 3)
    for args in ((0, d, 64, 64, 64, -1), (4, d, 1, 64, 64, -1), (4, d, 64, 64, -1, -1),
                 (4, bad, 64, 64, 64, -1), (64, d, 10, 10, 64, -1)):
        assert L.misor_mg_dist_levels(*args, C.byref(a), C.byref(b)) == EINVAL, args[0]
    assert (a.value, b.value) == (7, 7)
    assert L.misor_mg_dist_levels(4, None, 64, 64, 64, -1, C.byref(a), C.byref(b)) == 0


@pytest.mark.parametrize("nranks,dims,imax,jmax,cc,gc", [
    (4, (0, 0), 16, 16, 1, 0), (2, (2, 1), 24, 16, 1, 0), (2, (1, 2), 24, 16, 1, 0),
    (8, (0, 0), 64, 32, 1, 0), (8, (0, 0), 32768, 32768, 64, -1), (6, (0, 0), 96, 64, 1, 0),
    (16, (0, 0), 4096, 4096, 64, 0)])
def test_distributed_levels_are_decompositions_of_the_halved_grid(nranks, dims, imax, jmax, cc,
                                                                  gc):
    """on every distributed level below level 0 the halved block of every rank --
    sides and offset -- is misor_decompose of the halved grid on the same dims"""
    nlev, ndist = M.mg_dist_levels(nranks, imax, jmax, cc, gc, dims)
    assert ndist >= 2
    shapes = M.mg_levels(imax, jmax, cc)
    assert len(shapes) == nlev
    for r in range(nranks):
        up = M.decompose(nranks, r, imax, jmax, dims)
        for l in range(1, ndist):
            lo = M.decompose(nranks, r, shapes[l][0], shapes[l][1], dims)
            assert (2 * lo.ni, 2 * lo.nj, 2 * lo.ioff, 2 * lo.joff) == (up.ni, up.nj, up.ioff,
                                                                       up.joff), (r, l)
            assert tuple(lo.dims) == tuple(up.dims) and tuple(lo.coords) == tuple(up.coords)
            assert list(lo.neighbours) == list(up.neighbours)
            assert lo.ni >= 4 and lo.nj >= 4 and lo.ni * lo.nj > (DEFAULT_GATHER if gc < 0 else gc)
            up = lo


def test_stats_layout_appends_mg_dist_levels():
    S = M.StatsDist
    assert S.mg_dist_levels.offset == C.sizeof(M.StatsTail)
    assert C.sizeof(S) == C.sizeof(M.StatsTail) + 8  # an int and its padding
    assert S.mg_tail_ms.offset == M.StatsTail.mg_tail_ms.offset
