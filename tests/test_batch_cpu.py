"""misor_batch_*'s argument checks (include/misor.h): every one is MISOR_EINVAL
before any device call, so they hold on a host without a GPU -- a batch
touches the device only when data first moves or a solve runs."""
import ctypes as C

import numpy as np
import pytest

import pymisor as M

EINVAL = -1


def create(imax=10, jmax=10, dx=0.1, dy=0.1, nbatch=3, variant=M.SOLVE_RB):
    d = M.BatchDesc()
    d.imax, d.jmax, d.dx, d.dy = imax, jmax, dx, dy
    d.nbatch, d.variant, d.device = nbatch, variant, -1
    h = C.c_void_p()
    return M.lib().misor_batch_create(C.byref(h), C.byref(d)), h


def last_error():
    return M.lib().misor_last_error().decode()


@pytest.mark.parametrize("imax,jmax", [(127, 129),   # 8256 pairs > 8192 (8 a thread)
                                       (129, 127),
                                       (200, 200)])  # p does not fit in LDS
def test_shape_that_does_not_fit_is_refused(imax, jmax):
    rc, h = create(imax=imax, jmax=jmax)
    assert rc == EINVAL and not h
    msg = last_error()
    assert "LDS-resident problems only" in msg and "misor_create" in msg, msg
    with pytest.raises(M.MisorError, match="misor_create"):
        M.Batch(imax, jmax, 0.1, 0.1, 2)


@pytest.mark.parametrize("kw", [dict(nbatch=0), dict(nbatch=-4), dict(imax=0), dict(jmax=0),
                                dict(imax=-3), dict(dx=0.0), dict(dy=-1.0), dict(variant=7)])
def test_create_rejects_bad_descriptors(kw):
    rc, h = create(**kw)
    assert rc == EINVAL and not h, kw
    assert last_error()


def test_create_null_pointers():
    L = M.lib()
    d = M.BatchDesc()
    d.imax = d.jmax = 4
    d.dx = d.dy = 0.25
    d.nbatch = 1
    h = C.c_void_p()
    assert L.misor_batch_create(None, C.byref(d)) == EINVAL
    assert L.misor_batch_create(C.byref(h), None) == EINVAL


def test_null_handle_everywhere():
    L = M.lib()
    a = np.zeros(4)
    one = (C.c_int * 1)(0)
    v = C.c_int(0)
    assert L.misor_batch_set_params(None, None, None, None) == EINVAL
    assert L.misor_batch_upload(None, M.P, 0, M._ptr(a)) == EINVAL
    assert L.misor_batch_download(None, M.P, 0, M._ptr(a)) == EINVAL
    assert L.misor_batch_poisson_init(None, 1.0, 1.0, 2) == EINVAL
    assert L.misor_batch_solve_rb(None, one, M._ptr(a)) == EINVAL
    assert L.misor_batch_set_stream(None, None) == EINVAL
    assert L.misor_batch_set_tuning(None, M.TUNE_NEAR_BAND, 10) == EINVAL
    assert L.misor_batch_get_tuning(None, M.TUNE_NEAR_BAND, C.byref(v)) == EINVAL
    L.misor_batch_destroy(None)  # as free(NULL)


def test_largest_shapes_and_a_single_cell_are_accepted():
    for imax, jmax in [(128, 128), (1, 1), (100, 100), (2, 7)]:
        with M.Batch(imax, jmax, 1.0 / imax, 1.0 / jmax, 5) as b:
            assert b.shape == (jmax + 2, imax + 2) and b.nbatch == 5


def test_transfer_and_tuning_argument_checks():
    L = M.lib()
    with M.Batch(6, 5, 0.1, 0.1, 3) as b:
        one = np.zeros(b.shape)
        for fn in (L.misor_batch_upload, L.misor_batch_download):
            for member in (3, 4, -2, 1 << 20):
                assert fn(b.h, M.P, member, M._ptr(one)) == EINVAL, member
                assert "member" in last_error()
            for field in (M.U, M.V, M.F, M.G, -1, 17):
                assert fn(b.h, field, 0, M._ptr(one)) == EINVAL, field
            assert fn(b.h, M.RHS, 0, None) == EINVAL
        v = C.c_int(-1)
        for key in (M.TUNE_SMALL_SOLVE, M.TUNE_TSTEPS, M.TUNE_LEX_WGS, 0, 99):
            assert L.misor_batch_set_tuning(b.h, key, 1) == EINVAL, key
            assert L.misor_batch_get_tuning(b.h, key, C.byref(v)) == EINVAL, key
        assert L.misor_batch_get_tuning(b.h, M.TUNE_NEAR_BAND, None) == EINVAL
        # the one key a batch has: default as a grid's, set and read back
        assert b.get_tuning(M.TUNE_NEAR_BAND) == 10
        b.set_tuning(M.TUNE_NEAR_BAND, -30)
        assert b.get_tuning(M.TUNE_NEAR_BAND) == -30
        with pytest.raises(M.MisorError):
            b.set_tuning(M.TUNE_SMALL_SOLVE, 0)


def test_set_params_takes_scalars_sequences_and_none():
    with M.Batch(6, 5, 0.1, 0.1, 3) as b:
        b.set_params(omega=1.7)
        b.set_params(eps=[1e-3, 1e-4, 1e-5], itermax=[1, 2, 3])
        b.set_params()
        with pytest.raises(ValueError):
            b.set_params(omega=[1.0, 1.1])  # neither a scalar nor nbatch long
