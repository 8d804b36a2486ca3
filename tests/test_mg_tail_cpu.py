"""misor_mg_tail (include/misor.h "multigrid"): the tail of a hierarchy -- its
trailing levels that each fit the LDS of one workgroup, which misor_solve_mg
cycles in one launch -- against a restatement of the rule.  Host-only, like
misor_mg_levels; and the layout of the counters appended to misor_stats."""
import ctypes as C

import pytest

import pymisor as M

EINVAL = -1


def fits(ni, nj):
    """small_solve_fits (csrc/sor_kernels.hip): p with its ghosts and 256 bytes in
    160 KB of LDS, at most 8 cell pairs for each of 1024 threads"""
    return (ni + 2) * (nj + 2) * 8 + 256 <= 160 * 1024 and nj * ((ni + 1) // 2) <= 8 * 1024


def tail_rule(imax, jmax, cc):
    lv = M.mg_levels(imax, jmax, cc)
    first = next((l for l in range(len(lv)) if all(fits(*s) for s in lv[l:])), len(lv))
    return first, len(lv) - first


@pytest.mark.parametrize("imax,jmax,cc,want", [
    (4, 4, 4, (0, 2)),            # 4^2, 2^2
    (128, 128, 64, (0, 5)),       # the largest square that fits: 128 .. 8
    (130, 128, 64, (1, 1)),       # 8320 pairs miss the limit; 65 x 64 is odd: the coarsest
    (256, 128, 64, (1, 5)),       # 128 x 64 .. 8 x 4
    (192, 160, 2000, (1, 2)),     # 96 x 80, 48 x 40
    (2048, 2048, 64, (4, 5)),     # 128^2 is level 4 of 9
    (100, 100, 16384, (0, 1)),    # nothing is coarsened, the grid fits
    (1000, 1000, 10 ** 7, (1, 0)),  # nothing is coarsened, nothing fits
    (1000, 1000, 64, (3, 1)),     # 125^2, odd, is the coarsest and fits
    (24, 16, 1, (0, 4)),
])
def test_tail_cases(imax, jmax, cc, want):
    assert M.mg_tail(imax, jmax, cc) == want == tail_rule(imax, jmax, cc)


def test_tail_matches_the_rule_on_many_shapes():
    for imax in (2, 5, 8, 100, 126, 128, 130, 200, 254, 256, 258, 512, 4100, 16384):
        for jmax in (2, 4, 50, 64, 80, 126, 128, 130, 256, 1024):
            for cc in (0, 64, 2000):
                assert M.mg_tail(imax, jmax, cc) == tail_rule(imax, jmax, cc), (imax, jmax, cc)


def test_tail_argument_errors():
    L = M.lib()
    a, b = C.c_int(7), C.c_int(7)
    assert L.misor_mg_tail(64, 64, 64, C.byref(a), C.byref(b)) == 0
    assert (a.value, b.value) == (0, 4)
    a.value = b.value = 7
    for args in ((1, 64, 64), (64, 0, 64), (64, 64, -1)):  # misor_mg_levels' cases
        assert L.misor_mg_tail(*args, C.byref(a), C.byref(b)) == EINVAL, args
    assert L.misor_mg_tail(64, 64, 64, None, C.byref(b)) == EINVAL
    assert L.misor_mg_tail(64, 64, 64, C.byref(a), None) == EINVAL
    assert (a.value, b.value) == (7, 7)  # outputs untouched
    with pytest.raises(M.MisorError):
        M.mg_tail(1, 1)


def test_stats_layout_appends_the_tail_counters():
    """the tail's counters follow mg_transfers, which stays where it was"""
    S = M.StatsTail
    assert S.mg_transfers.offset == M.Stats.mg_transfers.offset
    assert S.mg_tail_levels.offset == M.Stats.mg_transfers.offset + 8 == C.sizeof(M.Stats)
    assert S.mg_tail_launches.offset == S.mg_tail_levels.offset + 8
    assert S.mg_tail_fallbacks.offset == S.mg_tail_launches.offset + 8
    assert S.mg_tail_ms.offset == S.mg_tail_fallbacks.offset + 8
    assert C.sizeof(S) == S.mg_tail_ms.offset + 8
    assert M.TUNE_MG_TAIL == 21
