"""Pin the CPU oracle (oracle/oracle.c) before trusting it.

1. Against the reference's own committed fixtures (assignment-4/p.dat,
   init.dat) -- always.
2. Against vectors generated from the reference compiled in this container
   (tests/golden/*.npz, rb_kat.json; see tests/golden/make_golden.py) -- always.
3. Against the reference itself (oracle/_ref/libref.so) on fresh random
   inputs -- when _ref was built (build container; it also travels to the GPU
   box as an in-tree .so).
"""
import json
import os

import numpy as np
import pytest

import ns_param_sets as PS
import orc

A6_DCAVITY = "a6_dcavity.par"
A6_CANAL = "a6_canal.par"


def fmt_rows(p):
    return "\n".join("".join("%f " % x for x in row) for row in p) + "\n"


def test_lexicographic_matches_committed_pdat(golden):
    """assignment-4/p.dat is the reference's own output of poisson.par"""
    p, rhs = orc.poisson_init(100, 100, 1.0, 1.0, 2)
    it, _ = orc.solve_lex(p, rhs, 0.01, 0.01, 1.9, 1e-6, 1000000, xorder=0)
    assert it == 2388
    assert fmt_rows(p) == open(os.path.join(golden, "a4_p.dat")).read()


def test_init_matches_committed_initdat(golden):
    """init.dat agrees to its 6 printed decimals; it shows -0.000000 where our
    (glibc) sin gives +1.2e-16 at x = pi multiples, so compare numerically."""
    p, _ = orc.poisson_init(100, 100, 1.0, 1.0, 2)
    ref = np.array([[float(x) for x in line.split()]
                    for line in open(os.path.join(golden, "a4_init.dat"))])
    assert ref.shape == p.shape
    assert np.abs(np.round(p, 6) - ref).max() <= 1e-6


def test_rb_iteration_kats(golden):
    kat = json.load(open(os.path.join(golden, "rb_kat.json")))
    for key, want in kat["iterations"].items():
        ni, nj = (map(int, key.split("x")) if "x" in key else (int(key), int(key)))
        p, rhs = orc.poisson_init(ni, nj)
        it, res = orc.solve_rb(p, rhs, 1.0 / ni, 1.0 / nj, kat["omega"], kat["eps"], 10 ** 7)
        assert it == want, key
        assert res < kat["eps"] ** 2


def test_rb_poisson100_fixture(golden):
    z = np.load(os.path.join(golden, "rb_poisson100.npz"))
    p, rhs = orc.poisson_init(100, 100)
    it, _ = orc.solve_rb(p, rhs, 0.01, 0.01, 1.9, 1e-6, 1000000)
    assert it == int(z["iterations"])
    assert np.array_equal(p, z["p"])
    p, rhs = orc.poisson_init(100, 100)
    it, _ = orc.solve_lex(p, rhs, 0.01, 0.01, 1.9, 1e-6, 1000000, xorder=0)
    assert it == int(z["iterations_lex"])
    assert np.array_equal(p, z["p_lex"])


def test_rb_sweep_fixtures(golden):
    z = np.load(os.path.join(golden, "rb_sweeps.npz"))
    for key in z.files:
        if not key.startswith("geom_"):
            continue
        ni, nj, xl, yl = z[key]
        ni, nj = int(ni), int(nj)
        for k in (1, 2, 7):
            p, rhs = orc.poisson_init(ni, nj, xl, yl, 2)
            it, _ = orc.solve_rb(p, rhs, xl / ni, yl / nj, 1.9, 1e-300, k)
            assert it == k
            assert np.array_equal(p, z["p_%dx%d_k%d" % (ni, nj, k)]), key


@pytest.mark.parametrize("name,par", [("ns_canal_rb_short.npz", A6_CANAL),
                                      ("ns_dcavity_rb_short.npz", A6_DCAVITY)])
def test_rb_ns_fixtures(golden, name, par):
    z = np.load(os.path.join(golden, name))
    prm = orc.read_par(os.path.join(golden, par))
    prm["te"] = float(z["te"])
    ns = orc.NS(prm)
    n, iters, t = ns.run(solver=1)
    assert n == int(z["steps"])
    assert np.array_equal(iters, z["iters"])
    for f in ("p", "u", "v"):
        assert np.array_equal(getattr(ns, f), z[f]), f
    assert t == float(z["t"])


# ------------------------------------------------------------ vs the reference

needs_ref = pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built")


@needs_ref
@pytest.mark.parametrize("which", ["rb", "rba", "lex"])
def test_solvers_vs_reference_random(which):
    rng = np.random.default_rng(11)
    for (ni, nj) in ((5, 4), (31, 17), (64, 90)):
        init = rng.standard_normal((nj + 2, ni + 2))
        it_ref, p_ref, rhs = orc.ref_a4(ni, nj, which, itermax=37, eps=1e-300, omg=1.7,
                                        xlength=1.3, ylength=0.9, init_p=init)
        p = init.copy()
        dx, dy = 1.3 / ni, 0.9 / nj
        if which == "lex":
            it, _ = orc.solve_lex(p, rhs, dx, dy, 1.7, 1e-300, 37, xorder=0)
        else:
            it, _ = orc.solve_rb(p, rhs, dx, dy, 1.7, 1e-300, 37, variant=which)
        assert it == it_ref == 37
        assert np.array_equal(p, p_ref)


@needs_ref
@pytest.mark.parametrize("par,steps", [(A6_DCAVITY, 25), (A6_CANAL, 12)])
def test_ns_vs_reference(golden, par, steps):
    path = os.path.join(golden, par)
    for solver in (0, 1):
        n, iters, p, u, v, t = orc.ref_ns(path, max_steps=steps, solver=solver)
        ns = orc.NS(orc.read_par(path))
        n2, iters2, t2 = ns.run(solver=solver, max_steps=steps)
        assert n == n2 == steps and t == t2
        if solver == 1:
            assert np.array_equal(iters, iters2)
        for f, ref in (("p", p), ("u", u), ("v", v)):
            assert np.array_equal(getattr(ns, f), ref), (solver, f)


@needs_ref
def test_ns_step_functions_vs_reference_bc_variants(golden, tmp_path):
    """every boundary flag on every wall, via edited copies of canal.par"""
    base = open(os.path.join(golden, A6_CANAL)).read()
    for combo in ((2, 2, 2, 2), (1, 3, 2, 1), (3, 1, 1, 3), (2, 1, 3, 2)):
        txt = base
        for key, val in zip(("bcLeft", "bcRight", "bcBottom", "bcTop"), combo):
            lines = [("%s    %d\t\t#" % (key, val)) if ln.startswith(key) else ln
                     for ln in txt.split("\n")]
            txt = "\n".join(lines)
        txt = txt.replace("imax          200", "imax          40").replace(
            "jmax          50", "jmax          20")
        f = tmp_path / ("c%d%d%d%d.par" % combo)
        f.write_text(txt)
        n, iters, p, u, v, t = orc.ref_ns(str(f), max_steps=6, solver=1)
        prm = orc.read_par(str(f))
        assert (prm["bcLeft"], prm["bcRight"], prm["bcBottom"], prm["bcTop"]) == combo
        ns = orc.NS(prm)
        ns.run(solver=1, max_steps=6)
        for fld, ref in (("p", p), ("u", u), ("v", v)):
            assert np.array_equal(getattr(ns, fld), ref), (combo, fld)


@needs_ref
@pytest.mark.parametrize("tau,dt,steps", [(-1.0, PS.DTS[0], 6), (-1.0, PS.DTS[1], 2),
                                          (0.5, 0.02, 6)])
@pytest.mark.parametrize("set_id", PS.SET_IDS)
@pytest.mark.parametrize("name", [A6_DCAVITY, A6_CANAL])
def test_ns_step_functions_vs_reference_param_sets(golden, tmp_path, name, set_id, tau, dt, steps):
    """the step functions off the shipped files' physical parameters
    (tests/ns_param_sets.py: non-zero gx and gy, gamma 0 / 1 / 0.37, another re
    and box), with both fixed dt values and with the adaptive dt: the 2D
    reference is driven as whole steps, so a few steps at 40 x 20, bit for bit"""
    over = dict(PS.overrides(set_id, ndim=2), imax=40, jmax=20, bcLeft=2, bcRight=3, bcBottom=1,
                bcTop=2, tau=tau, dt=dt)
    path = PS.write_par(golden, tmp_path, name, **over)
    prm = orc.read_par(path)
    for k, v in over.items():
        assert prm[k] == v, k  # the override reached the file the reference reads
    n, iters, p, u, v, t = orc.ref_ns(path, max_steps=steps, solver=1)
    ns = orc.NS(prm)
    n2, iters2, t2 = ns.run(solver=1, max_steps=steps)
    assert n == n2 == steps and t == t2
    assert np.array_equal(iters, iters2)
    for fld, ref in (("p", p), ("u", u), ("v", v)):
        assert np.isfinite(ref).all(), fld
        assert np.array_equal(getattr(ns, fld), ref), (set_id, fld)


@needs_ref
def test_ns_force_run_vs_reference(golden, tmp_path):
    """the run of tests/golden/ns_force_short.npz (forces, gamma 0.7, re 50 on
    the cavity at 48 x 32, adaptive dt): oracle, reference and fixture agree"""
    path = PS.write_par(golden, tmp_path, A6_DCAVITY, **PS.FORCE_RUN_2D)
    steps = PS.FORCE_RUN_2D_STEPS
    n, iters, p, u, v, t = orc.ref_ns(path, max_steps=steps, solver=1)
    ns = orc.NS(orc.read_par(path))
    n2, iters2, t2 = ns.run(solver=1, max_steps=steps)
    assert n == n2 == steps and t == t2
    z = np.load(os.path.join(golden, "ns_force_short.npz"))
    assert np.array_equal(iters, iters2) and np.array_equal(iters, z["iters"])
    assert t == float(z["t"])
    for fld, ref in (("p", p), ("u", u), ("v", v)):
        assert np.array_equal(getattr(ns, fld), ref), fld
        assert np.array_equal(z[fld], ref), fld


def test_lex_ns_oracle_vs_reference_fixture(golden):
    """the oracle's lexicographic NS against the reference build's own run
    (assignment-5/sequential with its shipped solve, te=0.05): bit-exact"""
    z = np.load(os.path.join(golden, "ns_seq_dcavity_lex_short.npz"))
    prm = orc.read_par(os.path.join(golden, "seq_dcavity.par"))
    prm["te"] = float(z["te"])
    ns = orc.NS(prm)
    steps, iters, t = ns.run(solver=0)
    assert steps == int(z["steps"])
    for k in ("p", "u", "v"):
        assert np.array_equal(getattr(ns, k), z[k]), k
    # the per-step iteration counts the GPU test checks against (the shipped
    # solve() reports none: they are this run's, tests/golden/make_golden.py)
    assert np.array_equal(iters, z["iters_oracle"])


@pytest.mark.parametrize("ni,nj,threads", [(37, 23, 3), (64, 64, 8), (100, 100, 4), (9, 5, 8)])
def test_multicore_solve_rb_matches_single_thread(ni, nj, threads):
    """the bench's multi-core CPU baseline (oracle_mt.c) is the same solveRB:
    p bit for bit, same iteration count; residual to rounding"""
    p1, rhs = orc.poisson_init(ni, nj, 1.0, 1.0, 2)
    p2 = p1.copy()
    it1, r1 = orc.solve_rb(p1, rhs, 1.0 / ni, 1.0 / nj, 1.9, 1e-300, 25)
    it2, r2 = orc.solve_rb_mt(p2, rhs, 1.0 / ni, 1.0 / nj, 1.9, 1e-300, 25, threads)
    assert it1 == it2 == 25
    assert np.array_equal(p1, p2)
    assert r2 == pytest.approx(r1, rel=1e-12)
    # to convergence: the poisson.par iteration count
    if (ni, nj) == (100, 100):
        p3, _ = orc.poisson_init(ni, nj, 1.0, 1.0, 2)
        it3, _ = orc.solve_rb_mt(p3, rhs, 0.01, 0.01, 1.9, 1e-6, 1000000, threads)
        assert it3 == 2388


def test_ns_run_threaded_solve_matches(golden):
    """orc_ns_run's solver 2 (solveRB on 16 threads, used for the 16384^2
    config-5 check) gives the fields and per-step iterations of solver 1"""
    prm = orc.read_par(os.path.join(golden, "a6_dcavity.par"))
    prm.update(imax=301, jmax=203, itermax=40)
    a, b = orc.NS(prm), orc.NS(prm)
    sa, ia, _ = a.run(solver=1, max_steps=6)
    sb, ib, _ = b.run(solver=2, max_steps=6)
    assert sa == sb == 6 and list(ia) == list(ib)
    for k in ("p", "u", "v"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
