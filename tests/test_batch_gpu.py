"""The batched solve (misor_batch_*, pymisor.Batch): B problems of one shape in
one launch of rb_solve_batch_kernel, one workgroup per member.  Every member
must end with the bits misor_solve_rb gives for it alone on a single grid
(which runs the same device function, rb_solve_small_body), and with the p
and iteration count of the restatement of solveRB / solveRBA
(assignment-4/src/solver.c:179-299)."""
import numpy as np
import pytest

import orc
import pymisor as M

pytestmark = pytest.mark.gpu

# odd ni (the last pair of a row has one cell), single rows / columns of pairs,
# one cell, and 128^2: exactly 8 pairs a thread and the largest LDS
SHAPES = [(3, 2), (2, 7), (1, 1), (33, 17), (128, 128)]
OMEGAS = [1.0, 1.5, 1.7, 1.9, 1.95]
ITERMAX = [0, 1, 2, 7, 4]
VARIANTS = {"rb": M.SOLVE_RB, "rba": M.SOLVE_RBA}
B = len(OMEGAS)

_data, _runs = {}, {}


def data(ni, nj, nb=B, seed=0):
    """(p0, rhs), each (nb, nj+2, ni+2): member m's own standard_normal fields"""
    key = (ni, nj, nb, seed)
    if key not in _data:
        rng = np.random.default_rng(1000003 * ni + 1009 * nj + seed)
        _data[key] = (rng.standard_normal((nb, nj + 2, ni + 2)),
                      rng.standard_normal((nb, nj + 2, ni + 2)))
        for a in _data[key]:
            a.setflags(write=False)
    return _data[key]


def run_batch(ni, nj, variant, p0, rhs, omega, eps, itermax, band=None):
    with M.Batch(ni, nj, 1.0 / ni, 1.0 / nj, len(p0), variant=VARIANTS[variant]) as b:
        if band is not None:
            b.set_tuning(M.TUNE_NEAR_BAND, band)
        b.set_params(omega=omega, eps=eps, itermax=itermax)
        b.upload(M.P, p0)
        b.upload(M.RHS, rhs)
        it, res = b.solve_rb()
        return b.download(M.P), it, res


def run_single(ni, nj, variant, p0, rhs, omega, eps, itermax, band=None):
    """one Grid per member through the whole-solve LDS kernel"""
    ps, its, ress = [], [], []
    for m in range(len(p0)):
        with M.Grid(ni, nj, 1.0 / ni, 1.0 / nj, omega[m], eps[m], itermax[m],
                    variant=VARIANTS[variant]) as g:
            g.set_tuning(M.TUNE_SMALL_SOLVE, 1)
            if band is not None:
                g.set_tuning(M.TUNE_NEAR_BAND, band)
            g.upload(M.P, p0[m])
            g.upload(M.RHS, rhs[m])
            it, res = g.solve_rb()
            ps.append(g.download(M.P))
            its.append(it)
            ress.append(res)
    return np.array(ps), np.array(its), np.array(ress)


def capped_batch(ni, nj, variant):
    key = (ni, nj, variant)
    if key not in _runs:
        p0, rhs = data(ni, nj)
        _runs[key] = run_batch(ni, nj, variant, p0, rhs, OMEGAS, 1e-300, ITERMAX)
    return _runs[key]


@pytest.mark.parametrize("variant", ["rb", "rba"])
@pytest.mark.parametrize("ni,nj", SHAPES)
def test_members_vs_oracle(ni, nj, variant):
    p0, rhs = data(ni, nj)
    got, it, _ = capped_batch(ni, nj, variant)
    assert list(it) == ITERMAX
    for m in range(B):
        want = p0[m].copy()
        it_ref, _ = orc.solve_rb(want, rhs[m].copy(), 1.0 / ni, 1.0 / nj, OMEGAS[m], 1e-300,
                                 ITERMAX[m], variant=variant)
        assert it_ref == ITERMAX[m]
        assert np.array_equal(got[m], want), (m, np.argwhere(got[m] != want)[:5])
    assert np.array_equal(got[0], p0[0])  # itermax = 0: untouched


@pytest.mark.parametrize("variant", ["rb", "rba"])
@pytest.mark.parametrize("ni,nj", SHAPES)
def test_members_vs_single_grid(ni, nj, variant):
    p0, rhs = data(ni, nj)
    if min(ni, nj) < 2:
        # misor_create has no grid with a side of 1 (tests/test_abi.py pins that):
        # nothing to compare this shape with; test_members_vs_oracle covers it
        with pytest.raises(M.MisorError):
            M.Grid(ni, nj, 1.0 / ni, 1.0 / nj, 1.0, 1e-300, 1)
        return
    got, it, res = capped_batch(ni, nj, variant)
    ps, its, ress = run_single(ni, nj, variant, p0, rhs, OMEGAS, [1e-300] * B, ITERMAX)
    assert np.array_equal(it, its)
    assert np.array_equal(got, ps)
    assert all(res[m] == ress[m] for m in range(B)), (res, ress)  # the same bits


def test_mixed_convergence(golden):
    """members that converge at different iterations beside a capped one"""
    ni = nj = 100
    omega = [1.9, 1.7, 1.95, 1.8]
    eps = [1e-6, 1e-6, 1e-6, 1e-300]
    itermax = [1000000, 1000000, 1000000, 50]
    with M.Batch(ni, nj, 1.0 / ni, 1.0 / nj, 4) as b:
        b.set_params(omega=omega, eps=eps, itermax=itermax)
        b.poisson_init(1.0, 1.0, 2)
        it, res = b.solve_rb()
        got = b.download(M.P)
    for m in range(4):
        want, rhs = orc.poisson_init(ni, nj, 1.0, 1.0, 2)
        it_ref, res_ref = orc.solve_rb(want, rhs, 1.0 / ni, 1.0 / nj, omega[m], eps[m],
                                       itermax[m])
        print("member", m, "omega", omega[m], "iterations", it[m], "oracle", it_ref)
        assert it[m] == it_ref, (m, it[m], it_ref)
        assert np.array_equal(got[m], want), m
        assert abs(res[m] - res_ref) <= 1e-12 * res_ref
    assert it[0] == 2388 and it[3] == 50
    assert np.array_equal(got[0], np.load(golden + "/rb_poisson100.npz")["p"])


def test_more_members_than_cus():
    """300 workgroups of ~4 KB LDS: several share a CU and the launch outlasts
    one round of the device's 256 CUs.  Every member is checked against the
    oracle -- none is left out."""
    ni = nj = 20
    nb = 300
    p0, rhs = data(ni, nj, nb, seed=4)
    omega = 1.0 + 0.95 * np.arange(nb) / (nb - 1)
    got, it, _ = run_batch(ni, nj, "rb", p0, rhs, omega, 1e-300, 3)
    assert np.all(it == 3)
    for m in range(nb):
        want = p0[m].copy()
        orc.solve_rb(want, rhs[m].copy(), 1.0 / ni, 1.0 / nj, omega[m], 1e-300, 3)
        assert np.array_equal(got[m], want), m


def test_near_band_forced():
    """a band of 10^30: every member stops before its first iteration and is
    finished by the single grid's path (re-run + exact tail)"""
    ni, nj, nb = 24, 20, 3
    p0, rhs = data(ni, nj, nb, seed=5)
    omega, eps, itermax = [1.2, 1.7, 1.9], [1e-3] * nb, [6] * nb
    got, it, res = run_batch(ni, nj, "rb", p0, rhs, omega, eps, itermax, band=-30)
    ps, its, ress = run_single(ni, nj, "rb", p0, rhs, omega, eps, itermax, band=-30)
    assert list(it) == [6] * nb and np.array_equal(it, its)
    assert np.array_equal(got, ps)
    assert all(res[m] == ress[m] for m in range(nb)), (res, ress)
    for m in range(nb):
        want = p0[m].copy()
        orc.solve_rb(want, rhs[m].copy(), 1.0 / ni, 1.0 / nj, omega[m], eps[m], 6)
        assert np.array_equal(got[m], want), m


def test_single_grid_second_near_solve():
    """the batch finishes its near members on ONE internal grid, one after the
    other: a grid's second near-threshold solve must be as good as its first
    (the re-run up to the near iteration once ran with the exact tail's loop
    state -- 12 iterations' p reported as 6)"""
    ni, nj = 24, 20
    p0, rhs = data(ni, nj, 3, seed=5)
    with M.Grid(ni, nj, 1.0 / ni, 1.0 / nj, 1.7, 1e-3, 6) as g:
        g.set_tuning(M.TUNE_NEAR_BAND, -30)
        for m in range(3):
            g.upload(M.P, p0[m])
            g.upload(M.RHS, rhs[m])
            it, _ = g.solve_rb()
            want = p0[m].copy()
            orc.solve_rb(want, rhs[m].copy(), 1.0 / ni, 1.0 / nj, 1.7, 1e-3, 6)
            assert it == 6
            assert np.array_equal(g.download(M.P), want), m


def test_near_band_default():
    """the default band on converging 32^2 solves: the oracle's counts; and a
    member whose eps^2 lies 1e-12 above the residual of its 20th iteration --
    inside the band, so the hand-off runs -- beside two that stay outside"""
    ni = nj = 32
    omega = [1.5, 1.7, 1.9]
    p_init, rhs_init = orc.poisson_init(ni, nj, 1.0, 1.0, 2)

    def oracle(om, eps, cap=1000000):
        q = p_init.copy()
        return (q,) + orc.solve_rb(q, rhs_init.copy(), 1.0 / ni, 1.0 / nj, om, eps, cap)

    for eps in ([1e-6] * 3, [1e-6, (oracle(1.7, 1e-300, 20)[2] * (1 + 1e-12)) ** 0.5, 1e-6]):
        with M.Batch(ni, nj, 1.0 / ni, 1.0 / nj, 3) as b:
            b.set_params(omega=omega, eps=eps, itermax=1000000)
            b.poisson_init(1.0, 1.0, 2)
            it, res = b.solve_rb()
            got = b.download(M.P)
        p0 = np.broadcast_to(p_init, (3,) + p_init.shape)
        rhs = np.broadcast_to(rhs_init, (3,) + p_init.shape)
        ps, its, ress = run_single(ni, nj, "rb", p0, rhs, omega, eps, [1000000] * 3)
        for m in range(3):
            want, it_ref, _ = oracle(omega[m], eps[m])
            assert it[m] == it_ref == its[m], (m, it[m], it_ref, its[m])
            assert np.array_equal(got[m], want) and np.array_equal(got[m], ps[m]), m
            assert res[m] == ress[m], (m, res[m], ress[m])


def test_upload_download_by_member():
    ni, nj, nb = 9, 6, 4
    p0, rhs = data(ni, nj, nb, seed=6)
    with M.Batch(ni, nj, 1.0 / ni, 1.0 / nj, nb) as b:
        assert not b.download(M.P).any() and not b.download(M.RHS).any()  # zeroed
        b.upload(M.P, p0)  # member = -1: all of them, contiguous
        b.upload(M.RHS, rhs)
        for m in range(nb):
            assert np.array_equal(b.download(M.P, member=m), p0[m])
            assert np.array_equal(b.download(M.RHS, member=m), rhs[m])
        # member = k touches member k of that field alone
        new = np.full((nj + 2, ni + 2), 7.25)
        b.upload(M.P, new, member=2)
        want = p0.copy()
        want[2] = new
        assert np.array_equal(b.download(M.P), want)
        assert np.array_equal(b.download(M.RHS), rhs)
        b.upload(M.RHS, new, member=0)
        assert np.array_equal(b.download(M.RHS, member=0), new)
        assert np.array_equal(b.download(M.RHS)[1:], rhs[1:])
        assert np.array_equal(b.download(M.P), want)
        # itermax 0 (the default): a solve leaves every member as it is
        it, res = b.solve_rb()
        assert not it.any() and np.all(res == 1.0)
        assert np.array_equal(b.download(M.P), want)
