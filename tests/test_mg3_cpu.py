"""misor3_mg_levels (host-only, no GPU) against a restatement of the level
rule, and the composed oracle of tests/mg3_oracle.py against itself: the numpy
transfers and the seed correction of the smoothing residual are checked at one
small shape against plain Python loops."""
import numpy as np
import pytest

import mg3_oracle as O
import pymisor as M


@pytest.mark.parametrize("shape,cc,want", [
    ((128, 128, 128), 512, [(128,) * 3, (64,) * 3, (32,) * 3, (16,) * 3, (8,) * 3]),
    ((200, 50, 50), 512, [(200, 50, 50), (100, 25, 25)]),   # canal.par: two levels
    ((24, 18, 40), 1, [(24, 18, 40), (12, 9, 20)]),         # an odd side stops it
    ((2, 8, 8), 1, [(2, 8, 8)]),                            # a side of 2: one level
    ((4, 8, 8), 1, [(4, 8, 8), (2, 4, 4)]),                 # a coarse side of 2
    ((32, 16, 24), 1, [(32, 16, 24), (16, 8, 12), (8, 4, 6), (4, 2, 3)]),
    ((7, 8, 6), 512, [(7, 8, 6)]),
    ((16, 16, 16), 4096, [(16, 16, 16)]),                   # at most coarse_cells cells
    ((16, 16, 16), 4095, [(16, 16, 16), (8, 8, 8)]),
])
def test_levels(shape, cc, want):
    assert O.levels_rule(*shape, cc) == want
    assert M.mg3_levels(*shape, coarse_cells=cc) == want


def test_levels_default_coarse_cells():
    assert M.mg3_levels(128, 128, 128)[-1] == (8, 8, 8)
    assert len(M.mg3_levels(128, 128, 128)) == 5


def test_levels_cap_smaller_than_levels():
    import ctypes as C

    L = M.lib()
    n = C.c_int(0)
    buf = (C.c_int * 9)(*([-7] * 9))
    assert L.misor3_mg_levels(128, 128, 128, 512, C.byref(n), buf, 2) == 0
    assert n.value == 5
    assert list(buf) == [128, 128, 128, 64, 64, 64, -7, -7, -7]
    assert L.misor3_mg_levels(128, 128, 128, 512, C.byref(n), None, 0) == 0 and n.value == 5


def test_levels_einval():
    import ctypes as C

    L = M.lib()
    n = C.c_int(0)
    buf = (C.c_int * 3)()
    for args in ((1, 8, 8, 512, C.byref(n), buf, 1), (8, 1, 8, 512, C.byref(n), buf, 1),
                 (8, 8, 1, 512, C.byref(n), buf, 1), (8, 8, 8, -1, C.byref(n), buf, 1),
                 (8, 8, 8, 512, C.byref(n), buf, -1), (8, 8, 8, 512, None, buf, 1),
                 (8, 8, 8, 512, C.byref(n), None, 1)):
        assert L.misor3_mg_levels(*args) == -1, args[:4]
        assert b"misor3_mg_levels" in L.misor_last_error()


# ------------------------------------------- the oracle's own consistency

def py_iteration(p, rhs, d, omega, res):
    """one iteration of orc3_solve in plain Python, the carry res in and out"""
    K, J, I = (s - 2 for s in p.shape)
    dx2, dy2, dz2 = d[0] * d[0], d[1] * d[1], d[2] * d[2]
    idx2, idy2, idz2 = 1.0 / dx2, 1.0 / dy2, 1.0 / dz2
    factor = omega * 0.5 * (dx2 * dy2 * dz2) / (dy2 * dz2 + dx2 * dz2 + dx2 * dy2)
    for ps in range(2):
        for k in range(1, K + 1):
            for j in range(1, J + 1):
                for i in range(1 if (1 + j + k + ps) & 1 else 2, I + 1, 2):
                    c = p[k, j, i]
                    tx = (p[k, j, i + 1] - 2.0 * c) + p[k, j, i - 1]
                    ty = (p[k, j + 1, i] - 2.0 * c) + p[k, j - 1, i]
                    tz = (p[k + 1, j, i] - 2.0 * c) + p[k - 1, j, i]
                    r = rhs[k, j, i] - ((tx * idx2 + ty * idy2) + tz * idz2)
                    p[k, j, i] = c - factor * r
                    res += r * r
    O.ghost_copy(p)
    return res / float(I * J * K)


def test_oracle_consistent_with_plain_loops():
    """6 x 4 x 8: the smoothing of mg3_oracle (orc3_solve and the seed correction)
    against the loop above seeded with 0, and the numpy transfers against
    per-cell loops -- bit for bit for the fields, 1e-12 for res"""
    shape, lengths = (6, 4, 8), (1.0, 0.7, 1.3)
    d = O.spacing(shape, lengths)
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal((10, 6, 8))
    rhs = rng.standard_normal((10, 6, 8))
    for nu in (1, 2, 3):
        a, b, res_b = p0.copy(), p0.copy(), 0.0
        res_a = O.smooth(a, rhs, shape, lengths, 1.0, nu)
        for _ in range(nu):
            res_b = py_iteration(b, rhs, d, 1.0, res_b)
        assert np.array_equal(a, b)
        assert abs(res_a - res_b) <= 1e-12 * res_b, (nu, res_a, res_b)
    # residual and restriction
    r = O.residual(p0, rhs, shape, lengths)
    rc = O.restrict(r)
    idx2, idy2, idz2 = (1.0 / (h * h) for h in d)
    for K in range(1, 5):
        for J in range(1, 3):
            for I in range(1, 4):
                v = []
                for k in (2 * K - 1, 2 * K):
                    for j in (2 * J - 1, 2 * J):
                        for i in (2 * I - 1, 2 * I):
                            c = p0[k, j, i]
                            tx = (p0[k, j, i + 1] - 2.0 * c) + p0[k, j, i - 1]
                            ty = (p0[k, j + 1, i] - 2.0 * c) + p0[k, j - 1, i]
                            tz = (p0[k + 1, j, i] - 2.0 * c) + p0[k - 1, j, i]
                            v.append(rhs[k, j, i] - ((tx * idx2 + ty * idy2) + tz * idz2))
                want = 0.125 * (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])))
                assert rc[K, J, I] == want
    assert not rc[0].any() and not rc[:, 0].any() and not rc[:, :, 0].any()
    # prolongation
    e = rng.standard_normal(rc.shape)
    got = p0.copy()
    O.prolong_correct(got, e)
    want = p0.copy()
    nc = (3, 2, 4)

    def E(I, J, K):
        return e[min(max(K, 1), nc[2]), min(max(J, 1), nc[1]), min(max(I, 1), nc[0])]

    for k in range(1, 9):
        for j in range(1, 5):
            for i in range(1, 7):
                I, J, K = (i + 1) // 2, (j + 1) // 2, (k + 1) // 2
                sx, sy, sz = (-1 if i & 1 else 1), (-1 if j & 1 else 1), (-1 if k & 1 else 1)
                want[k, j, i] += (27.0 * E(I, J, K) +
                                  9.0 * ((E(I + sx, J, K) + E(I, J + sy, K)) + E(I, J, K + sz)) +
                                  3.0 * ((E(I + sx, J + sy, K) + E(I + sx, J, K + sz)) +
                                         E(I, J + sy, K + sz)) +
                                  E(I + sx, J + sy, K + sz)) * 0.015625
    O.ghost_copy(want)
    assert np.array_equal(got, want)
    # edges and corners keep what they held
    assert got[0, 0, 3] == p0[0, 0, 3] and got[0, 0, 0] == p0[0, 0, 0]
