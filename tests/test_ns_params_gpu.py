"""The 2D NS step kernels (ns_kernels.hip through misor_ns.hip) off the two
shipped .par files' physical parameters: the sets of tests/ns_param_sets.py
(non-zero gx and gy of opposite sign, gamma 0 / 1 / 0.37, another re and box)
with dt 1e-5 and 0.5, every candidate of computeTimestep as the minimum, and
a whole run with forces.  Bit for bit against the CPU oracle, which
tests/test_oracle.py pins to the reference at the same parameters; the oracle
is first shown to depend on each set (ns_param_sets.assert_sensitive)."""
import os

import numpy as np
import pytest

import ns_param_sets as PS
import orc
import pymisor as M
from test_ns_gpu import assert_fields, check_run, load_both, par, random_state

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("dt", PS.DTS)
@pytest.mark.parametrize("set_id", PS.SET_IDS)
@pytest.mark.parametrize("ni,nj", [(37, 23), (126, 65), (300, 70)])
def test_fg_rhs_adapt_param_sets_bitwise(golden, ni, nj, set_id, dt, fuse):
    """37 x 23: one workgroup; 126 x 65: the second 64-row band of fg_rhs_kernel
    starts from a recomputed G(i, 64) (gy enters its prologue) and the waves'
    column ranges end on ni; 300 x 70: two workgroups along x, the recomputed
    F(i-1, j) (gx) crosses their edge.  fuse = 0: fg_kernel and the separate
    computeRHS."""
    base = par(golden, "a6_canal.par", imax=ni, jmax=nj)
    st = random_state(base, ni + nj)
    PS.assert_sensitive(base, set_id, st, dt, ndim=2)
    prm = dict(base, **PS.overrides(set_id, ndim=2))
    ns, g = load_both(prm, st, dt)
    g.set_tuning(M.TUNE_NS_FUSE, fuse)
    ns.call("compute_fg")
    g.call("compute_fg")
    assert_fields(ns, g, ("f", "g", "u", "v"))
    ns.call("compute_rhs")
    g.call("compute_rhs")
    assert_fields(ns, g, ("rhs", "f", "g"))
    ns.call("adapt_uv")
    g.call("adapt_uv")
    assert_fields(ns, g, ("u", "v", "p"))
    # computeTimestep right after adaptUV takes the maxima adaptUV left behind
    ns.call("compute_timestep")
    assert g.compute_timestep(ns.s.dtBound, prm["tau"]) == ns.s.dt
    g.close()


def plant(a, where, value):
    """put `value` (the array's largest magnitude by far) at a named place"""
    nj, ni = a.shape[0] - 2, a.shape[1] - 2
    idx = {"interior": (nj // 2, ni // 3), "ghost": (nj // 2, ni + 1),  # a physical ghost cell
           "last": (nj + 1, ni + 1)}[where]  # the array's last element
    a[idx] = value


# which candidate decides, the scale of (u, v), where the deciding maximum sits, its sign
TIMESTEP_CASES = [("dtBound", (1e-3, 1e-3), "interior", 1.0),
                  ("dx/umax", (1.0, 1.0), "ghost", 1.0),
                  ("dx/umax", (1.0, 1.0), "interior", -1.0),
                  ("dy/vmax", (1.0, 1.0), "last", 1.0),
                  ("dy/vmax", (1.0, 1.0), "ghost", -1.0)]


@pytest.mark.parametrize("decides,scale,where,sign", TIMESTEP_CASES)
def test_compute_timestep_every_candidate(golden, decides, scale, where, sign):
    """set re_len: dx = 2.7/70, dy = 0.9/45 and dtBound = 1.15e-3 all differ and
    none is the shipped files' round value"""
    prm = par(golden, "a6_dcavity.par", imax=70, jmax=45, **PS.overrides("re_len", ndim=2))
    st = random_state(prm, 41)
    st["u"] *= scale[0]
    st["v"] *= scale[1]
    if decides != "dtBound":
        plant(st["u" if decides == "dx/umax" else "v"], where, sign * 400.0)
    name, val = PS.timestep_winner(prm, (st["u"], st["v"]), ndim=2)
    assert name == decides
    ns, g = load_both(prm, st, 0.02)
    ns.call("compute_timestep")
    assert ns.s.dt == prm["tau"] * val  # the oracle took this branch
    dt = g.compute_timestep(ns.s.dtBound, prm["tau"])
    assert dt == ns.s.dt
    umax, vmax = g.max_uv()
    assert umax == np.abs(st["u"]).max() == orc.lib().orc_ns_max_element(ns.s, orc._ptr(ns.u))
    assert vmax == np.abs(st["v"]).max() == orc.lib().orc_ns_max_element(ns.s, orc._ptr(ns.v))
    g.close()


@pytest.mark.parametrize("nranks", [1, 4])
def test_force_run_matches_reference_fixture(golden, nranks):
    """40 steps of the cavity at 48 x 32 with gx 0.5, gy -1.0, gamma 0.7, re 50
    (the reference's own run, tests/golden/ns_force_short.npz): per-step
    iterations, t and fields, on one rank and on 2 x 2"""
    z = np.load(os.path.join(golden, "ns_force_short.npz"))
    assert int(z["steps"]) == PS.FORCE_RUN_2D_STEPS
    check_run(golden, "ns_force_short.npz", "a6_dcavity.par", nranks, over=PS.FORCE_RUN_2D)
