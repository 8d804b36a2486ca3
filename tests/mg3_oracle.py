"""The composed CPU oracle of misor3_solve_mg (DESIGN.md "Geometric multigrid,
3D"), shared by tests/test_mg3_cpu.py and tests/test_mg3_gpu.py.

TEST INFRASTRUCTURE ONLY.  Smoothing and the coarsest solve are orc3_solve
(oracle/oracle3d.c) reached through orc3.NS3 with p and rhs set; the transfers
are restated in numpy -- residual in the solve's own expression and operation
order, restriction, zeroing, prolongation and ghost copy.  numpy's elementwise
operations do not contract, so p is compared bit for bit.  Arrays have shape
(kmax+2, jmax+2, imax+2), A(i,j,k) = a[k, j, i]."""
import os

import numpy as np

import orc3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAR = os.path.join(ROOT, "tests", "golden", "a6_dcavity.par")

DEFAULTS = dict(nu1=2, nu2=2, omega_smooth=1.0, coarse_cells=512, omega_coarse=1.7,
                eps_coarse=0.0, itermax_coarse=1000)


def levels_rule(imax, jmax, kmax, coarse_cells):
    n = (imax, jmax, kmax)
    out = [n]
    while not (any(s % 2 or s < 4 for s in n) or n[0] * n[1] * n[2] <= coarse_cells):
        n = tuple(s // 2 for s in n)
        out.append(n)
    return out


def make_prm(shape, lengths, eps=0.0, omg=1.7, itermax=10):
    """a parameter dict for orc3.NS3 / pymisor.Grid3: a6_dcavity.par's values
    with the sizes, lengths and solve parameters replaced"""
    prm = orc3.read_par3(PAR)
    prm.update(imax=shape[0], jmax=shape[1], kmax=shape[2], xlength=lengths[0],
               ylength=lengths[1], zlength=lengths[2], eps=eps, omg=omg, itermax=itermax)
    return prm


def solve_orc(p, rhs, shape, lengths, omega, eps, itermax):
    """orc3_solve in place on p (carry seeded with 1.0): (iterations, res)"""
    ns = orc3.NS3(make_prm(shape, lengths, eps=eps, omg=omega, itermax=itermax))
    ns.p[...] = p
    ns.rhs[...] = rhs
    it, res = ns.solve()
    p[...] = ns.p
    return it, res


def smooth(p, rhs, shape, lengths, omega, nu):
    """nu iterations, no early exit, the carry seeded with 0.0: orc3_solve
    seeds it with 1.0, which adds exactly N^-nu to what it reports"""
    it, res = solve_orc(p, rhs, shape, lengths, omega, 0.0, nu)
    assert it == nu
    n = float(shape[0] * shape[1] * shape[2])
    return res - n ** -nu


def ghost_copy(p):
    """solver.c:237-278: faces only, edges and corners are not touched"""
    p[0, 1:-1, 1:-1] = p[1, 1:-1, 1:-1]
    p[-1, 1:-1, 1:-1] = p[-2, 1:-1, 1:-1]
    p[1:-1, 0, 1:-1] = p[1:-1, 1, 1:-1]
    p[1:-1, -1, 1:-1] = p[1:-1, -2, 1:-1]
    p[1:-1, 1:-1, 0] = p[1:-1, 1:-1, 1]
    p[1:-1, 1:-1, -1] = p[1:-1, 1:-1, -2]


def spacing(shape, lengths):
    return tuple(lengths[a] / shape[a] for a in range(3))


def residual(p, rhs, shape, lengths):
    """r = rhs - ((tx idx2 + ty idy2) + tz idz2) on the interior"""
    dx, dy, dz = spacing(shape, lengths)
    idx2, idy2, idz2 = 1.0 / (dx * dx), 1.0 / (dy * dy), 1.0 / (dz * dz)
    c = p[1:-1, 1:-1, 1:-1]
    tx = (p[1:-1, 1:-1, 2:] - 2.0 * c) + p[1:-1, 1:-1, :-2]
    ty = (p[1:-1, 2:, 1:-1] - 2.0 * c) + p[1:-1, :-2, 1:-1]
    tz = (p[2:, 1:-1, 1:-1] - 2.0 * c) + p[:-2, 1:-1, 1:-1]
    return rhs[1:-1, 1:-1, 1:-1] - ((tx * idx2 + ty * idy2) + tz * idz2)


def restrict(r):
    """rc = 0.125 (((r000 + r100) + (r010 + r110)) + ((r001 + r101) + (r011 + r111))),
    rXYZ the fine cell at offsets X, Y, Z; with a zero ghost layer"""
    rc = np.zeros(tuple(s // 2 + 2 for s in r.shape))

    def plane(z):
        return ((r[z::2, 0::2, 0::2] + r[z::2, 0::2, 1::2]) +
                (r[z::2, 1::2, 0::2] + r[z::2, 1::2, 1::2]))

    rc[1:-1, 1:-1, 1:-1] = 0.125 * (plane(0) + plane(1))
    return rc


def prolong_correct(p, e):
    """p += (27 c + 9 ((ex + ey) + ez) + 3 ((exy + exz) + eyz) + exyz) * 0.015625
    with the parent's neighbours on the fine cell's side, clamped to the coarse
    interior; then p's ghost copy"""
    E = np.pad(e[1:-1, 1:-1, 1:-1], 1, mode="edge")  # the clamp
    m = slice(1, -1)
    sl = {-1: slice(None, -2), 1: slice(2, None)}
    c = E[m, m, m]
    f = p[1:-1, 1:-1, 1:-1]
    for sz, k0 in ((-1, 0), (1, 1)):
        for sy, j0 in ((-1, 0), (1, 1)):
            for sx, i0 in ((-1, 0), (1, 1)):
                X, Y, Z = sl[sx], sl[sy], sl[sz]
                f[k0::2, j0::2, i0::2] += (27.0 * c +
                                           9.0 * ((E[m, m, X] + E[m, Y, m]) + E[Z, m, m]) +
                                           3.0 * ((E[m, Y, X] + E[Z, m, X]) + E[Z, Y, m]) +
                                           E[Z, Y, X]) * 0.015625
    ghost_copy(p)


def cycle(p, rhs, lengths, shapes, q, res):
    """one V-cycle in place on p; returns res as misor3_solve_mg defines it"""
    shape = shapes[0]
    if len(shapes) == 1:
        _, r = solve_orc(p, rhs, shape, lengths, q["omega_coarse"], q["eps_coarse"],
                         q["itermax_coarse"])
        return r
    if q["nu1"] > 0:
        res = smooth(p, rhs, shape, lengths, q["omega_smooth"], q["nu1"])
    rc = restrict(residual(p, rhs, shape, lengths))
    e = np.zeros_like(rc)
    cycle(e, rc, lengths, shapes[1:], q, 1.0)
    prolong_correct(p, e)
    if q["nu2"] > 0:
        res = smooth(p, rhs, shape, lengths, q["omega_smooth"], q["nu2"])
    return res


def solve(p0, rhs, lengths, eps=0.0, maxcycles=100, **kw):
    """misor3_solve_mg restated: (p, cycles, res, levels)"""
    q = dict(DEFAULTS, **kw)
    shape = (p0.shape[2] - 2, p0.shape[1] - 2, p0.shape[0] - 2)
    shapes = levels_rule(*shape, q["coarse_cells"])
    p, res, n = p0.copy(), 1.0, 0
    rhs = np.ascontiguousarray(rhs)
    while res >= eps * eps and n < maxcycles:
        res = cycle(p, rhs, lengths, shapes, q, res)
        n += 1
    return p, n, res, len(shapes)


def cosine_problem(n):
    """rhs = cos(2 pi x) cos(2 pi y) cos(2 pi z) at the cell centres of the unit
    cube with n^3 cells (compatible with Neumann), p0 = 0"""
    x = (np.arange(n + 2) - 0.5) / n
    c = np.cos(2.0 * np.pi * x)
    rhs = c[:, None, None] * c[None, :, None] * c[None, None, :]
    return np.zeros((n + 2,) * 3), np.ascontiguousarray(rhs)
