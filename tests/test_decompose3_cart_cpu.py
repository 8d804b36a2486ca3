"""misor3_decompose_cart (host-only): the reference's 3D Cartesian process grid
(assignment-6/src/comm.c:24-101, 476-513) -- MPI_Dims_create's factorisation
with the largest factor on z (the reference indexes its dims KDIM = 0, JDIM =
1, IDIM = 2), MPI_Cart_create's row-major ranks with z slowest, sizeOfRank per
axis."""
import itertools

import pytest

import pymisor as M


def dims_create(n):
    """most balanced factorisation of n into three factors, non-increasing (the
    smallest largest factor, then the smallest second one), largest to z: (x, y, z)"""
    best = None
    for a in range(1, n + 1):
        for b in range(1, a + 1):
            for c in range(1, b + 1):
                if a * b * c == n and (best is None or (a, b, c) < best):
                    best = (a, b, c)
    return best[::-1]


def size_of_rank(rank, size, n):
    return n // size + (1 if n % size > rank else 0)


def test_dims_create_rule_of_the_issue():
    """the values the reference's mpirun -np N gives, spelled out"""
    want = {2: (1, 1, 2), 4: (1, 2, 2), 8: (2, 2, 2), 6: (1, 2, 3), 12: (2, 2, 3)}
    for n, d in want.items():
        assert dims_create(n) == d
        assert tuple(M.decompose3_cart(n, 0, 64, 64, 64).dims) == d


@pytest.mark.parametrize("n", range(1, 17))
def test_automatic_dims(n):
    loc = M.decompose3_cart(n, n - 1, 64, 64, 64)
    assert tuple(loc.dims) == dims_create(n)
    assert loc.dims[0] * loc.dims[1] * loc.dims[2] == n


def test_partly_fixed_dims():
    assert tuple(M.decompose3_cart(8, 0, 64, 64, 64, dims=(4, 0, 0)).dims) == (4, 1, 2)
    assert tuple(M.decompose3_cart(12, 0, 64, 64, 64, dims=(0, 3, 0)).dims) == (2, 3, 2)
    assert tuple(M.decompose3_cart(12, 0, 64, 64, 64, dims=(0, 0, 1)).dims) == (3, 4, 1)
    assert tuple(M.decompose3_cart(6, 5, 64, 64, 64, dims=(3, 2, 1)).dims) == (3, 2, 1)
    assert tuple(M.decompose3_cart(6, 0, 64, 64, 64, dims=(3, 2, 0)).dims) == (3, 2, 1)
    for n, dims in ((8, (3, 0, 0)), (8, (2, 2, 1)), (8, (2, 2, 4)), (6, (4, 0, 0)),
                    (4, (0, -1, 0))):
        with pytest.raises(M.MisorError):
            M.decompose3_cart(n, 0, 64, 64, 64, dims=dims)
    with pytest.raises(M.MisorError):
        M.decompose3_cart(4, 4, 64, 64, 64)


@pytest.mark.parametrize("box,dims", [((13, 9, 16), (2, 2, 2)), ((200, 50, 50), (2, 2, 2)),
                                      ((200, 50, 50), (4, 1, 2)), ((7, 5, 6), (3, 2, 3))])
def test_blocks_tile_the_box(box, dims):
    n = dims[0] * dims[1] * dims[2]
    locs = [M.decompose3_cart(n, r, *box, dims=dims) for r in range(n)]
    owner = {}
    for r, loc in enumerate(locs):
        assert tuple(loc.dims) == dims
        c = tuple(loc.coords)
        # MPI_Cart_create without reorder, z slowest
        assert c == (r % dims[0], (r // dims[0]) % dims[1], r // (dims[0] * dims[1]))
        assert r == (c[2] * dims[1] + c[1]) * dims[0] + c[0]
        for a in range(3):
            assert loc.n[a] == size_of_rank(c[a], dims[a], box[a]) >= 2
            assert loc.off[a] == sum(size_of_rank(q, dims[a], box[a]) for q in range(c[a]))
        cells = itertools.product(*(range(loc.off[a] + 1, loc.off[a] + loc.n[a] + 1)
                                    for a in range(3)))
        for cell in cells:
            assert cell not in owner, (cell, r, owner[cell])
            owner[cell] = r
    assert len(owner) == box[0] * box[1] * box[2]
    # neighbours: left, right, bottom, top, front, back; mutual, -1 at the physical sides
    for r, loc in enumerate(locs):
        c = tuple(loc.coords)
        for s in range(6):
            a, up = s // 2, s % 2
            q = loc.neighbours[s]
            if (c[a] == dims[a] - 1) if up else (c[a] == 0):
                assert q == -1
                continue
            cq = list(c)
            cq[a] += 1 if up else -1
            assert tuple(locs[q].coords) == tuple(cq)
            assert locs[q].neighbours[s ^ 1] == r


def test_too_few_cells_names_the_axis():
    with pytest.raises(M.MisorError, match=r"along x"):
        M.decompose3_cart(2, 0, 3, 50, 50, dims=(2, 1, 1))
    with pytest.raises(M.MisorError, match=r"along z"):
        M.decompose3_cart(4, 0, 50, 50, 7, dims=(1, 1, 4))
    M.decompose3_cart(2, 0, 4, 50, 50, dims=(2, 1, 1))  # 2 cells each: fine
