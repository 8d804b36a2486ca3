"""The parameter sets of tests/ns_param_sets.py against the CPU oracle alone:
every set changes F, G (and H) at every interior cell, every force component
changes its own array and no other, at both dt values and at every shape the
GPU parity tests use them -- so those tests cannot pass on a set that the
checker ignores.  Also pins the table itself to what the tests rely on."""
import os

import numpy as np
import pytest

import ns_param_sets as PS
import orc
import orc3


def state3(shape, seed):
    rng = np.random.default_rng(seed)
    return {n: rng.standard_normal(shape) for n in orc3.FIELDS}


def state2(shape, seed):
    rng = np.random.default_rng(seed)
    return {n: rng.standard_normal(shape) for n in orc.NS.FIELDS}


def test_table_is_what_the_tests_rely_on():
    assert PS.SET_IDS == ["force", "gamma0", "gamma1", "gamma_mid", "re_len", "all"]
    f = PS.SETS["force"]
    assert f["gx"] > 0 > f["gy"] and f["gz"] > 0
    assert len(set(abs(v) for v in PS.SETS["all"].values())) == len(PS.SETS["all"])  # distinct
    for v in set(abs(v) for s in PS.SETS.values() for v in s.values()):
        if v not in (0.0, 1.0):  # gamma's two end points are exact on purpose
            assert v.as_integer_ratio()[1] >= 2 ** 40, "%r is exact in binary" % v
    assert PS.SETS["all"] == dict(gx=0.7, gy=-9.81, gz=3.3, re=7.3, xlength=2.7, ylength=0.9,
                                  zlength=1.3, gamma=0.37)
    assert PS.DTS == (1e-5, 0.5)


@pytest.mark.parametrize("dt", PS.DTS)
@pytest.mark.parametrize("set_id", PS.SET_IDS)
@pytest.mark.parametrize("name,dims", [("a6_dcavity.par", (13, 9, 7)),
                                       ("a6_canal.par", (70, 33, 6))])
def test_sets_move_the_3d_oracle(golden, name, dims, set_id, dt):
    base = orc3.read_par3(os.path.join(golden, name))
    base.update(imax=dims[0], jmax=dims[1], kmax=dims[2])
    st = state3((dims[2] + 2, dims[1] + 2, dims[0] + 2), 5)
    PS.assert_sensitive(base, set_id, st, dt, ndim=3)


@pytest.mark.parametrize("dt", PS.DTS)
@pytest.mark.parametrize("set_id", PS.SET_IDS)
@pytest.mark.parametrize("ni,nj", [(37, 23), (126, 65), (300, 70)])
def test_sets_move_the_2d_oracle(golden, ni, nj, set_id, dt):
    base = orc.read_par(os.path.join(golden, "a6_canal.par"))
    base.update(imax=ni, jmax=nj)
    PS.assert_sensitive(base, set_id, state2((nj + 2, ni + 2), 6), dt, ndim=2)


def test_guard_rejects_an_ignored_set(golden):
    """the guard itself: a set that only repeats the defaults must fail it"""
    base = orc3.read_par3(os.path.join(golden, "a6_dcavity.par"))
    base.update(imax=6, jmax=5, kmax=4)
    st = state3((6, 7, 8), 1)
    PS.SETS["_noop"] = dict(gamma=base["gamma"])
    try:
        with pytest.raises(AssertionError, match="as the default does"):
            PS.assert_sensitive(base, "_noop", st, 0.5)
    finally:
        del PS.SETS["_noop"]
