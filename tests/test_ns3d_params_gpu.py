"""The 3D NS step kernels (ns3d_kernels.hip through misor3d_api.hip) off the
two shipped .par files' physical parameters: the sets of
tests/ns_param_sets.py (gx, gy, gz all non-zero and distinct, gy negative,
gamma 0 / 1 / 0.37, another re and box) with dt 1e-5 and 0.5, every candidate
of computeTimestep as the minimum, and a whole run with forces on the
fixed-dt branch of the main loop.  Bit for bit against the 3D oracle, which
tests/test_oracle3d.py pins to the reference at the same parameters; the
oracle is first shown to depend on each set (ns_param_sets.assert_sensitive)."""
import os

import numpy as np
import pytest

import ns_param_sets as PS
import orc3
from test_ns3d_cart_gpu import run_steps
from test_ns3d_gpu import GPU_FIELD, assert_fields_equal, pair, params, random_state, run_gpu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dt", PS.DTS)
@pytest.mark.parametrize("set_id", PS.SET_IDS)
@pytest.mark.parametrize("name,dims", [("a6_dcavity.par", (13, 9, 7)),
                                       ("a6_canal.par", (70, 33, 6))])
def test_fg_rhs_adapt_param_sets_bitwise(golden, name, dims, set_id, dt):
    """dx, dy and dz differ at both shapes, for the shipped boxes and for re_len's"""
    base = params(golden, name, imax=dims[0], jmax=dims[1], kmax=dims[2])
    prm = dict(base, **PS.overrides(set_id))
    d = [prm[a + "length"] / prm[n] for a, n in zip("xyz", ("imax", "jmax", "kmax"))]
    assert len(set(d)) == 3, d
    st = random_state((dims[2] + 2, dims[1] + 2, dims[0] + 2), sum(dims))
    PS.assert_sensitive(base, set_id, st, dt)
    ns, g = pair(prm, st, dt)
    with g:
        for fn in ("compute_fg", "compute_rhs", "adapt_uvw"):
            ns.call(fn)
            g.call(fn)
            assert_fields_equal(ns, g, fn)


def plant(a, where, value):
    """put `value` (the array's largest magnitude by far) at a named place"""
    nk, nj, ni = (n - 2 for n in a.shape)
    idx = {"interior": (nk // 2, nj // 2, ni // 3),
           "ghost": (nk // 2, 0, ni // 2),  # a physical ghost cell
           "last": (nk + 1, nj + 1, ni + 1)}[where]  # the array's last element
    a[idx] = value


# which candidate decides, where the deciding maximum sits, its sign
TIMESTEP_CASES = [("dtBound", "interior", 1.0), ("dx/umax", "ghost", 1.0),
                  ("dy/vmax", "last", 1.0), ("dz/wmax", "interior", -1.0),
                  ("dy/vmax", "ghost", -1.0)]


@pytest.mark.parametrize("decides,where,sign", TIMESTEP_CASES)
def test_compute_timestep_every_candidate(golden, decides, where, sign):
    """set re_len at 13 x 9 x 7: dx = 0.208, dy = 0.1, dz = 0.186 and dtBound =
    0.0240 all differ and none is the shipped files' round value"""
    prm = params(golden, "a6_dcavity.par", imax=13, jmax=9, kmax=7, **PS.overrides("re_len"))
    rng = np.random.default_rng(43)
    st = {n: rng.standard_normal((9, 11, 15)) for n in orc3.FIELDS}
    if decides == "dtBound":
        for n in "uvw":
            st[n] *= 0.1
    else:
        plant(st[{"dx/umax": "u", "dy/vmax": "v", "dz/wmax": "w"}[decides]], where, sign * 90.0)
    name, val = PS.timestep_winner(prm, [st[n] for n in "uvw"])
    assert name == decides
    ns, g = pair(prm, st, 0.0)
    with g:
        ns.call("compute_timestep")
        assert ns.s.dt == prm["tau"] * val  # the oracle took this branch
        assert g.compute_timestep() == ns.s.dt
        mx = g.max_uvw()
        for q, n in enumerate("uvw"):
            assert mx[q] == np.abs(st[n]).max() == \
                orc3.lib().orc3_max_element(ns.s, getattr(ns.s, n))


def force_prm(golden):
    z = np.load(os.path.join(golden, "ns3d_force_short.npz"))
    prm = params(golden, "a6_dcavity.par", **PS.FORCE_RUN_3D)
    assert tuple(int(x) for x in z["dims"]) == (prm["imax"], prm["jmax"], prm["kmax"])
    assert int(z["steps"]) == PS.FORCE_RUN_3D_STEPS and prm["tau"] < 0
    return z, prm


@pytest.mark.parametrize("tune", [(1, 8, 0), (0, 8, 0), (1, 8, 0, 1, 0, 1)])
def test_force_run_matches_reference_fixture(golden, tune):
    """12 steps of the cavity at 16 x 12 x 10 with gx 0.5, gy -1.0, gz 0.25,
    gamma 0.7, re 50, tau -1 and dt 0.005 (the reference's own run,
    tests/golden/ns3d_force_short.npz): per-step iterations, t and fields, bit
    for bit, on the fused sweep, the two colour passes and the resident solve"""
    z, prm = force_prm(golden)
    g, iters, t = run_gpu(prm, int(z["steps"]), tune)
    with g:
        assert np.array_equal(iters, z["iters"])
        assert t == z["t"]
        for n in ("p", "u", "v", "w"):
            assert np.array_equal(g.download(GPU_FIELD[n]), z[n]), n


def test_force_run_on_2x2x2(golden):
    z, prm = force_prm(golden)
    out = run_steps(prm, (2, 2, 2), int(z["steps"]))
    for iters, t, _ in out:
        assert iters == list(z["iters"]) and t == z["t"]
    for n in ("p", "u", "v", "w"):
        assert np.array_equal(out[0][2][n], z[n]), n
