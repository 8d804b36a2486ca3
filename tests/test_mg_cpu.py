"""The host side of the multigrid solve (include/misor.h "multigrid"): the level
rule of misor_mg_levels against a restatement of it, and the argument checks of
misor_solve_mg / misor_mg_default_params, which all precede the first device
call and so hold on a host without a GPU."""
import ctypes as C

import pytest

import pymisor as M

EINVAL = -1


def levels_rule(imax, jmax, coarse_cells=64):
    """level l+1 = (imax/2, jmax/2); the first level with an odd side, a side
    below 4 or at most coarse_cells cells is the coarsest"""
    out = [(imax, jmax)]
    while not (imax % 2 or jmax % 2 or imax < 4 or jmax < 4 or imax * jmax <= coarse_cells):
        imax, jmax = imax // 2, jmax // 2
        out.append((imax, jmax))
    return out


def test_levels_of_the_flagship_grid():
    lv = M.mg_levels(32768, 32768)
    assert len(lv) == 13 and lv[0] == (32768, 32768) and lv[-1] == (8, 8)
    assert lv == [(32768 >> k, 32768 >> k) for k in range(13)]


@pytest.mark.parametrize("imax,jmax,cc,want", [
    (1000, 1000, 64, [(1000, 1000), (500, 500), (250, 250), (125, 125)]),  # odd: stops
    (100, 100, 16384, [(100, 100)]),                                       # small enough
    (6, 4, 1, [(6, 4), (3, 2)]),                                           # odd / side < 4
    (7, 8, 1, [(7, 8)]),                                                   # cannot coarsen
    (4, 4, 1, [(4, 4), (2, 2)]),                                           # the smallest pair
    (8, 4, 0, [(8, 4), (4, 2)]),                                           # side < 4 stops
    (24, 16, 1, [(24, 16), (12, 8), (6, 4), (3, 2)]),
    (192, 160, 2000, [(192, 160), (96, 80), (48, 40)]),
    (192, 160, 1900, [(192, 160), (96, 80), (48, 40), (24, 20)]),
    (65536, 2, 0, [(65536, 2)]),
])
def test_levels_cases(imax, jmax, cc, want):
    assert M.mg_levels(imax, jmax, cc) == want == levels_rule(imax, jmax, cc)


def test_levels_match_the_rule_on_many_shapes():
    for imax in list(range(2, 70)) + [96, 128, 250, 1024, 4100]:
        for jmax in (2, 3, 4, 6, 8, 12, 40, 64, 100, 512, 4096):
            for cc in (0, 1, 16, 64, 2000):
                lv = M.mg_levels(imax, jmax, cc)
                assert lv == levels_rule(imax, jmax, cc), (imax, jmax, cc)
                assert min(min(s) for s in lv) >= 2  # misor_create's smallest side


def test_levels_cap_and_argument_errors():
    L = M.lib()
    n = C.c_int(0)
    shapes = (C.c_int * 4)(-1, -1, -1, -1)
    # cap 2 of 13 levels: the count is the whole hierarchy's, two shapes are written
    assert L.misor_mg_levels(32768, 32768, 64, C.byref(n), shapes, 2) == 0
    assert n.value == 13 and list(shapes) == [32768, 32768, 16384, 16384]
    assert L.misor_mg_levels(64, 64, 64, C.byref(n), None, 0) == 0 and n.value == 4
    assert L.misor_mg_levels(64, 64, 64, None, None, 0) == EINVAL
    assert L.misor_mg_levels(1, 64, 64, C.byref(n), None, 0) == EINVAL
    assert L.misor_mg_levels(64, 0, 64, C.byref(n), None, 0) == EINVAL
    assert L.misor_mg_levels(64, 64, -1, C.byref(n), None, 0) == EINVAL
    assert L.misor_mg_levels(64, 64, 64, C.byref(n), None, 3) == EINVAL
    assert L.misor_mg_levels(64, 64, 64, C.byref(n), shapes, -1) == EINVAL
    with pytest.raises(M.MisorError):
        M.mg_levels(1, 1)


def params(**kw):
    q = M.MgParams()
    q.nu1, q.nu2, q.omega_smooth, q.coarse_cells = 2, 2, 1.0, 64
    q.omega_coarse, q.eps_coarse, q.itermax_coarse, q.maxcycles = 1.7, 1e-7, 1000, 100
    for k, v in kw.items():
        setattr(q, k, v)
    return q


@pytest.mark.parametrize("kw,word", [
    (dict(nu1=0, nu2=0), "nu1 + nu2"),
    (dict(nu1=-1), "nu1"),
    (dict(nu2=-3, nu1=5), "nu2"),
    (dict(omega_smooth=0.0), "omega"),
    (dict(omega_smooth=-1.0), "omega"),
    (dict(omega_smooth=float("nan")), "omega"),
    (dict(omega_coarse=0.0), "omega"),
    (dict(coarse_cells=-1), "coarse_cells"),
    (dict(itermax_coarse=-1), "itermax_coarse"),
    (dict(maxcycles=-1), "maxcycles"),
])
def test_solve_rejects_bad_parameters_before_any_device_call(kw, word):
    """the parameter checks come first of all: they are reached, and name the
    parameter, without a grid (which only a GPU host can create)"""
    L = M.lib()
    assert L.misor_solve_mg(None, C.byref(params(**kw)), None, None) == EINVAL
    msg = L.misor_last_error().decode()
    assert "misor_solve_mg" in msg and word in msg, msg


def test_null_grid():
    L = M.lib()
    n, r = C.c_int(7), C.c_double(7.0)
    for prm in (None, C.byref(params())):
        assert L.misor_solve_mg(None, prm, C.byref(n), C.byref(r)) == EINVAL
        assert "null grid" in L.misor_last_error().decode()
    assert n.value == 7 and r.value == 7.0  # outputs untouched
    q = M.MgParams()
    assert L.misor_mg_default_params(None, C.byref(q)) == EINVAL
    assert L.misor_mg_default_params(None, None) == EINVAL


def test_stats_layout_keeps_the_existing_offsets():
    """the multigrid counters are appended: lite_misses stays where it was"""
    assert M.Stats.lite_misses.offset + 8 == M.Stats.mg_cycles.offset
    assert [f[0] for f in M.Stats._fields_][-4:] == ["mg_cycles", "mg_levels", "mg_transfer_ms",
                                                     "mg_transfers"]
