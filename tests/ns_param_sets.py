"""Physical parameter sets off the two shipped .par files' values, shared by
the reference pins (test_oracle.py, test_oracle3d.py), the CPU sensitivity
guard (test_ns_param_sets_cpu.py) and the GPU parity tests
(test_ns_params_gpu.py, test_ns3d_params_gpu.py, test_ns_steps_decomposed_gpu.py).

TEST INFRASTRUCTURE.  Every value is inexact in binary and the magnitudes are
pairwise distinct; all three forces are non-zero and gy carries the opposite
sign, so a swapped, negated or dropped term changes the bits of F, G or H.
"""
import numpy as np

import orc
import orc3

FORCE = dict(gx=0.7, gy=-9.81, gz=3.3)
RE_LEN = dict(re=7.3, xlength=2.7, ylength=0.9, zlength=1.3)
SETS = {
    "force": dict(FORCE),
    "gamma0": dict(gamma=0.0),
    "gamma1": dict(gamma=1.0),
    "gamma_mid": dict(gamma=0.37),
    "re_len": dict(RE_LEN),
    "all": dict(FORCE, **RE_LEN, gamma=0.37),
}
SET_IDS = list(SETS)
DTS = (1e-5, 0.5)  # each set runs with both, instead of the single 0.0137
KEYS_3D_ONLY = ("gz", "zlength")

# the whole runs with forces, off-default gamma and re (make_golden.py's
# ns_force_short.npz and ns3d_force_short.npz, both on a6_dcavity.par)
FORCE_RUN = dict(gx=0.5, gy=-1.0, gz=0.25, gamma=0.7, re=50.0)
FORCE_RUN_3D = dict(FORCE_RUN, imax=16, jmax=12, kmax=10, tau=-1.0, dt=0.005)
FORCE_RUN_3D_STEPS = 12
FORCE_RUN_2D = dict({k: v for k, v in FORCE_RUN.items() if k != "gz"}, imax=48, jmax=32)
FORCE_RUN_2D_STEPS = 40


def overrides(set_id, ndim=3):
    """the set's overrides; the 2D solver has no gz and no zlength"""
    o = dict(SETS[set_id])
    if ndim == 2:
        for k in KEYS_3D_ONLY:
            o.pop(k, None)
    return o


def write_par(golden, tmp_path, name, **over):
    """the shipped .par `name` with overrides, as a file (the reference and the
    host programs read files); a key the file lacks is appended"""
    import os
    import re
    txt = open(os.path.join(golden, name)).read()
    for k, v in over.items():
        txt, n = re.subn(r"(?m)^%s\s.*$" % k, "%s %r" % (k, v), txt)
        if n == 0:
            txt += "\n%s %r\n" % (k, v)
    path = tmp_path / name.replace("a6_", "")
    path.write_text(txt)
    return str(path)


# ------------------------------------------------------------ sensitivity guard
def _fg3(prm, st, dt):
    ns = orc3.NS3(prm)
    for n in orc3.FIELDS:
        getattr(ns, n)[...] = st[n]
    ns.s.dt = dt
    ns.call("compute_fg")
    # the cells no wall override fixes: F(imax,j,k) = U, G(i,jmax,k) = V, H(i,j,kmax) = W
    return {"f": ns.f[1:-1, 1:-1, 1:-2].copy(), "g": ns.g[1:-1, 1:-2, 1:-1].copy(),
            "h": ns.h[1:-2, 1:-1, 1:-1].copy()}


def _fg2(prm, st, dt):
    ns = orc.NS(prm)
    for n in orc.NS.FIELDS:
        getattr(ns, n)[...] = st[n]
    ns.s.dt = dt
    ns.call("compute_fg")
    return {"f": ns.f[1:-1, 1:-2].copy(), "g": ns.g[1:-2, 1:-1].copy()}


def assert_sensitive(base, set_id, st, dt, ndim=3):
    """A condition on the CPU oracle alone: with the set's overrides its F, G
    (and H) differ from the result of the unmodified parameters `base` at every
    interior cell, and for the sets with forces each of F, G, H differs from
    the result with that one force component zeroed -- a set the oracle ignores
    cannot pass a parity test."""
    fg = _fg3 if ndim == 3 else _fg2
    over = overrides(set_id, ndim)
    want = fg(dict(base, **over), st, dt)
    plain = fg(base, st, dt)
    for n in want:
        same = np.count_nonzero(want[n] == plain[n])
        assert same == 0, "set %s leaves %d cells of %s as the default does" % (set_id, same, n)
    for n, key in (("f", "gx"), ("g", "gy"), ("h", "gz")):
        if key in over and n in want:
            zeroed = fg(dict(base, **dict(over, **{key: 0.0})), st, dt)
            same = np.count_nonzero(want[n] == zeroed[n])
            assert same == 0, "set %s: %s ignores %s at %d cells" % (set_id, n, key, same)
            for m in want:  # and the component enters no other array
                if m != n:
                    assert np.array_equal(want[m], zeroed[m]), (set_id, key, m)


# ------------------------------------------------- which timestep bound decides
def timestep_candidates(prm, vel, ndim=3):
    """computeTimestep's candidates by the reference's formula
    (assignment-6/src/solver.c:340-362, assignment-5/sequential/src/solver.c:219-234),
    from the numpy arrays: [("dtBound", .), ("dx/umax", .), ...] in its order"""
    names = ("x", "y", "z")[:ndim]
    d = [prm[n + "length"] / prm[m] for n, m in zip(names, ("imax", "jmax", "kmax"))]
    inv = 1.0 / (d[0] * d[0]) + 1.0 / (d[1] * d[1])
    if ndim == 3:
        inv = inv + 1.0 / (d[2] * d[2])
    out = [("dtBound", 0.5 * prm["re"] * 1.0 / inv)]
    for h, n, a in zip(d, ("dx/umax", "dy/vmax", "dz/wmax"), vel):
        out.append((n, h / np.abs(a).max()))
    return out


def timestep_winner(prm, vel, ndim=3):
    """(name, value) of the strict minimum among the candidates"""
    c = timestep_candidates(prm, vel, ndim)
    best = min(c, key=lambda t: t[1])
    assert sum(1 for t in c if t[1] == best[1]) == 1, c
    return best
