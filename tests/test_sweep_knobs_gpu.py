"""The single-iteration sweep (sor_kernels.hip rb_sweep_kernel) under every
launch-geometry knob, and the knobs' other readers, against the restatement of
solveRB (assignment-4/src/solver.c:179-238).

misor.h promises results that are "bit-identical for every setting".  Here:

  MISOR_TUNE_SWEEP_VARIANT   all 15 instantiations (4 / 8 / 16 strips per
                             workgroup, 1..3 rows in flight, nt stores / loads)
  MISOR_TUNE_ROWS_PER_BLOCK  1, heights that do not divide nj, heights above nj
  MISOR_TUNE_XCD_REMAP       block counts that are no multiple of 8 (the q / rr
                             arithmetic of rb_sweep_kernel and of sor_tb.h
                             for_each_block's one-workgroup-per-block branch)
  SweepParams::part          the interior / boundary split of an overlapped
                             decomposed sweep, for every strip count
  MISOR_TUNE_TB_PERSISTENT   0: solves with one workgroup per block
  exact_tail                 its own (default-variant) geometry under another
                             configured sweep variant
  the knobs changed between two solves of one grid

Bars (the suite's): p over the whole array, ghosts and corners included, bit
for bit; the iteration count equal; res within a relative 1e-12 (only the
order in which r^2 is summed differs).  Fields: standard_normal p and 10 x rhs,
ghosts included, dx != dy, a fixed iteration count (eps = 1e-300) unless stated.
"""
import functools

import numpy as np
import pytest

import orc
import pymisor as M
from test_decomposed_gpu import assemble, local_window, run_ranks

pytestmark = pytest.mark.gpu

# misor_internal.h kSweepVariants: (strips per workgroup, rows in flight, nt stores, nt loads)
SWEEP_VARIANTS = [(4, 1, 0, 0), (4, 2, 0, 0), (4, 3, 0, 0), (4, 1, 1, 0), (4, 2, 1, 0),
                  (8, 1, 0, 0), (8, 2, 0, 0), (8, 2, 1, 0), (8, 1, 1, 0), (8, 3, 1, 0),
                  (16, 1, 1, 0), (16, 2, 1, 0), (4, 3, 1, 0), (8, 2, 1, 1), (16, 2, 1, 1)]
DEFAULT_VARIANT = 7
STRIP = 128  # tb_plan.h kStripCells
OMEGA = 1.7


def waves_of(variant):
    return SWEEP_VARIANTS[variant][0]


def auto_rows(ni, nj, waves):
    """tb_plan.h pick_rows_per_block"""
    nbx = -(-(-(-ni // STRIP)) // waves)
    want_nby = -(-2048 // nbx)
    return min(16, max(4, -(-nj // want_nby)))


def sweep_blocks(ni, nj, variant, rows):
    """tb_plan.h sweep_partials: (nbx, nby) of the launch; rows <= 0: automatic"""
    w = waves_of(variant)
    h = rows if rows > 0 else auto_rows(ni, nj, w)
    return -(-(-(-ni // STRIP)) // w), -(-nj // h)


@functools.lru_cache(maxsize=None)
def case(ni, nj, k, seed=0):
    """fields and the oracle's (p, it, res) after k iterations; shared by the
    tests of a shape, never written to"""
    rng = np.random.default_rng(ni + 7 * nj + seed)
    p = rng.standard_normal((nj + 2, ni + 2))
    rhs = rng.standard_normal((nj + 2, ni + 2)) * 10
    dx, dy = 1.1 / ni, 0.9 / nj
    want = p.copy()
    it, res = orc.solve_rb(want, rhs, dx, dy, OMEGA, 1e-300, k)
    assert it == k
    for a in (p, rhs, want):
        a.setflags(write=False)
    return p, rhs, dx, dy, want, it, res


def set_sweep(g, variant, rows, remap):
    """the three knobs of the single sweep, and T = 1 on the multi-block path"""
    g.set_tuning(M.TUNE_SMALL_SOLVE, 0)
    g.set_tuning(M.TUNE_TSTEPS, 1)
    g.set_tuning(M.TUNE_SWEEP_VARIANT, variant)
    g.set_tuning(M.TUNE_ROWS_PER_BLOCK, rows)
    g.set_tuning(M.TUNE_XCD_REMAP, remap)
    ni, nj = g.loc.ni, g.loc.nj
    assert g.get_tuning(M.TUNE_SWEEP_VARIANT) == variant
    assert g.get_tuning(M.TUNE_XCD_REMAP) == remap
    assert g.get_tuning(M.TUNE_ROWS_PER_BLOCK) == (
        rows if rows > 0 else auto_rows(ni, nj, waves_of(variant)))


def ran_single_sweep(st):
    """the sweep kernel, not a T = 1 pass of a temporally blocked one"""
    return st["iters_per_pass"] == 1 and st["tb_variant"] == -1


def sweep_solve(ni, nj, k, variant, rows, remap):
    p, rhs, dx, dy, _, _, _ = case(ni, nj, k)
    with M.Grid(ni, nj, dx, dy, OMEGA, 1e-300, k) as g:
        set_sweep(g, variant, rows, remap)
        g.upload(M.P, p)
        g.upload(M.RHS, rhs)
        it, res = g.solve_rb()
        assert ran_single_sweep(g.stats()), g.stats()
        return it, res, g.download(M.P)


def check(got, want, it, it_ref, res, res_ref, what):
    assert it == it_ref, what
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5])
    assert abs(res - res_ref) <= 1e-12 * res_ref, (what, res, res_ref)


# ---------------------------------------------------------------------------
# 1. every variant x shape x remap, one rank
# ---------------------------------------------------------------------------

# the column edges of the 128-column strip and of the 512 / 1024 / 2048-column
# workgroup; k = 3: the result ends in the other ping-pong buffer
SHAPES = [
    (37, 2),     # less than one strip, two rows
    (128, 5),    # the right ghost column is the next strip's first pair
    (129, 3),    # ia == ni + 1: ghost-right store from the left lane's value
    (130, 3),    # ib == ni + 1: ghost-right store from the lane's own value
    (1024, 9),   # c0 + 128 == ni + 1 at a workgroup edge for 4 and 8 strips
    (1025, 4),   # one column into a second workgroup
    (2050, 37),  # two workgroups wide at 16 strips
]
WIDE, WIDE_ROWS = (2050, 37), 7


def test_wide_shape_block_counts():
    """(2050, 37) at 7 rows a block: 30, 18 and 12 blocks for 4, 8 and 16
    strips -- at least 9 and no multiple of 8, so the remap's rr is not 0"""
    counts = {}
    for v in range(len(SWEEP_VARIANTS)):
        nbx, nby = sweep_blocks(*WIDE, v, WIDE_ROWS)
        assert nbx * nby >= 9 and (nbx * nby) % 8 != 0, (v, nbx, nby)
        counts[waves_of(v)] = nbx * nby
    assert counts == {4: 30, 8: 18, 16: 12}


@pytest.mark.parametrize("variant", range(len(SWEEP_VARIANTS)))
@pytest.mark.parametrize("ni,nj", SHAPES)
def test_every_variant_vs_oracle(ni, nj, variant):
    k = 3
    _, _, _, _, want, it_ref, res_ref = case(ni, nj, k)
    rows = WIDE_ROWS if (ni, nj) == WIDE else 0
    for remap in (0, 1):
        it, res, got = sweep_solve(ni, nj, k, variant, rows, remap)
        check(got, want, it, it_ref, res, res_ref, (variant, remap))


# ---------------------------------------------------------------------------
# 2. rows per block
# ---------------------------------------------------------------------------

ROWS_SHAPE = (300, 45)


def test_rows_shape_block_counts():
    """(300, 45) is one workgroup wide: the rows values give 45, 23, 7, 1, 1 and
    (automatic: 4 rows) 12 blocks -- rr = 5, 7, 7, 1, 1, 4 under the remap"""
    for v in (2, 7, 14):
        assert [sweep_blocks(*ROWS_SHAPE, v, r) for r in (1, 2, 7, 45, 54, 0)] == \
            [(1, 45), (1, 23), (1, 7), (1, 1), (1, 1), (1, 12)]
        assert auto_rows(*ROWS_SHAPE, waves_of(v)) == 4


# one variant per strip count; 2 also has 3 rows in flight
@pytest.mark.parametrize("rows", [1, 2, 7, 45, 54, 0])
@pytest.mark.parametrize("variant", [2, 7, 14])
def test_rows_per_block_vs_oracle(variant, rows):
    ni, nj = ROWS_SHAPE
    k = 3
    _, _, _, _, want, it_ref, res_ref = case(ni, nj, k)
    ress = []
    for remap in (0, 1):
        it, res, got = sweep_solve(ni, nj, k, variant, rows, remap)
        check(got, want, it, it_ref, res, res_ref, (variant, rows, remap))
        ress.append(res)
    # the partials are indexed by logical block: one sum order, remapped or not
    assert ress[0] == ress[1], ress


@pytest.mark.parametrize("back", [0, -3])
def test_rows_zero_or_negative_is_automatic(back):
    ni, nj = ROWS_SHAPE
    k = 3
    p, rhs, dx, dy, want, it_ref, res_ref = case(ni, nj, k)
    with M.Grid(ni, nj, dx, dy, OMEGA, 1e-300, k) as g:
        set_sweep(g, 14, 7, 1)
        g.set_tuning(M.TUNE_ROWS_PER_BLOCK, back)
        assert g.get_tuning(M.TUNE_ROWS_PER_BLOCK) == auto_rows(ni, nj, 16) == 4
        g.upload(M.P, p)
        g.upload(M.RHS, rhs)
        it, res = g.solve_rb()
        assert ran_single_sweep(g.stats())
        check(g.download(M.P), want, it, it_ref, res, res_ref, back)


# ---------------------------------------------------------------------------
# 3. decomposed, T = 1: the interior / boundary split (SweepParams::part)
# ---------------------------------------------------------------------------

def block_classes(loc, variant, rows):
    """rb_sweep_kernel's `interior` of every block of one rank's launch, with
    tb_plan.h sweep_interior_bounds: (interior blocks, boundary blocks)"""
    ni, nj, nb = loc.ni, loc.nj, list(loc.neighbours)
    w = waves_of(variant)
    h = rows if rows > 0 else auto_rows(ni, nj, w)
    nbx, nby = sweep_blocks(ni, nj, variant, rows)
    big = 10 ** 9
    int_lo_i = 3 if nb[0] >= 0 else -big
    int_hi_i = ni - 2 if nb[1] >= 0 else 2 * big
    int_lo_j = 3 if nb[2] >= 0 else -big
    int_hi_j = nj - 2 if nb[3] >= 0 else 2 * big
    n_int = 0
    for by in range(nby):
        for bx in range(nbx):
            c0b = 1 + bx * w * STRIP
            j0b = 1 + by * h
            j1b = min(j0b + h, nj + 1)
            n_int += (c0b - 2 >= int_lo_i and c0b + w * STRIP + 1 <= int_hi_i and
                      j0b - 2 >= int_lo_j and j1b + 1 <= int_hi_j)
    return n_int, nbx * nby - n_int


# 2 x 2 ranks of 2101 / 2100 x 21 / 20 cells: each has one neighbour side and
# one physical side each way, and at 16 strips two block columns (2048 + the
# rest), one of which is interior; 3 x 1 ranks of 4200 x 20: the middle rank
# has no physical left or right side and three block columns at 16 strips
DIST = {(2, 2): (4201, 41), (3, 1): (12600, 20)}


# automatic rows are 4 on every one of these blocks (pick_rows_per_block's floor:
# asserted below), so 0 and 4 launch one geometry through two settings; 6 divides
# neither 20 nor 21: a short last block row (j1b = nj + 1) in the `interior` rule
DIST_ROWS = [0, 4, 6]


@pytest.mark.parametrize("variant", [0, 7, 10])  # 4, 8, 16 strips
@pytest.mark.parametrize("rows", DIST_ROWS)
@pytest.mark.parametrize("dims", sorted(DIST))
def test_decomposed_shapes_split_both_ways(dims, rows, variant):
    """every rank's overlapped launch has interior and boundary blocks"""
    ni, nj = DIST[dims]
    world = dims[0] * dims[1]
    for r in range(world):
        loc = M.decompose(world, r, ni, nj, dims=dims)
        assert auto_rows(loc.ni, loc.nj, waves_of(variant)) == 4
        assert loc.nj % 6 != 0
        n_int, n_bnd = block_classes(loc, variant, rows)
        assert n_int >= 1 and n_bnd >= 1, (r, n_int, n_bnd)
    if dims == (3, 1):
        mid = M.decompose(3, 1, ni, nj, dims=dims)
        assert list(mid.neighbours)[0] >= 0 and list(mid.neighbours)[1] >= 0


def decomposed_sweep(dims, variant, rows, overlap):
    ni, nj = DIST[dims]
    world, k = dims[0] * dims[1], 3
    p, rhs, dx, dy, want, it_ref, res_ref = case(ni, nj, k)

    def rank_fn(r, cid, dims):
        with M.Grid(ni, nj, dx, dy, OMEGA, 1e-300, k, device=0, nranks=world, rank=r,
                    dims=dims, comm_id=cid) as g:
            g.set_tuning(M.TUNE_OVERLAP, overlap)
            set_sweep(g, variant, rows, 1)
            g.upload(M.P, local_window(p, g.loc))
            g.upload(M.RHS, local_window(rhs, g.loc))
            it, res = g.solve_rb()
            return g.loc, g.download(M.P), it, res, g.stats()

    outs = run_ranks(world, rank_fn, dims)
    for (_, _, it, res, st) in outs:
        assert ran_single_sweep(st), st
        assert it == it_ref
        assert abs(res - res_ref) <= 1e-12 * res_ref
    got = assemble([(o[0], o[1]) for o in outs], p.shape)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


@pytest.mark.parametrize("variant", [0, 7, 10])
@pytest.mark.parametrize("rows", DIST_ROWS)
@pytest.mark.parametrize("overlap", [1, 0], ids=["overlap", "serial"])
def test_decomposed_sweep_variants(overlap, rows, variant):
    decomposed_sweep((2, 2), variant, rows, overlap)


@pytest.mark.parametrize("variant", [0, 7, 10])
@pytest.mark.parametrize("rows", [4, 6])
def test_decomposed_sweep_rank_without_physical_sides(rows, variant):
    decomposed_sweep((3, 1), variant, rows, 1)


# ---------------------------------------------------------------------------
# 4. MISOR_TUNE_TB_PERSISTENT = 0: one workgroup per block
# ---------------------------------------------------------------------------

TB_SHAPE = (600, 300)
TB_WAVES = {0: 4, 2: 2}  # tb_plan.h kTbVariants


def tb_blocks(ni, nj, T, variant, rows):
    """tb_plan.h tb_geometry with an explicit block height, unchained"""
    ow = STRIP - 4 * T
    nbx = -(-(-(-ni // ow)) // TB_WAVES[variant])
    return nbx * -(-nj // min(rows, nj))


def tb_rows_for(T, variant):
    """block heights in ring lengths S = 2T + 2 (sor_tb.h ring_slots, 2 rows in
    flight): 3 S, as test_pow2_spacing_unchained_vs_oracle.  That gives 34, 18,
    12 blocks for variant 0 and 51, 27, 24 for variant 2 at T = 2, 5, 8: where
    the count is a multiple of 8 (variant 2, T = 8), 2 S as well (36 blocks)"""
    S = 2 * T + 2
    rows = [3 * S]
    if tb_blocks(*TB_SHAPE, T, variant, 3 * S) % 8 == 0:
        rows.append(2 * S)
    return rows


def test_unqueued_block_counts():
    for variant, want in ((0, [34, 18, 12]), (2, [51, 27, 24])):
        assert [tb_blocks(*TB_SHAPE, T, variant, 3 * (2 * T + 2)) for T in (2, 5, 8)] == want
    for variant in (0, 2):
        for T in (2, 5, 8):
            assert tb_blocks(*TB_SHAPE, T, variant, tb_rows_for(T, variant)[-1]) % 8 != 0


@pytest.mark.parametrize("T", [2, 5, 8])
@pytest.mark.parametrize("variant", [0, 2])
def test_unqueued_passes_vs_oracle(variant, T):
    ni, nj = TB_SHAPE
    for k in (T, 2 * T + 1):
        p, rhs, dx, dy, want, it_ref, res_ref = case(ni, nj, k)
        for rows in tb_rows_for(T, variant):
            for remap in (0, 1):
                with M.Grid(ni, nj, dx, dy, OMEGA, 1e-300, k) as g:
                    g.set_tuning(M.TUNE_SMALL_SOLVE, 0)
                    g.set_tuning(M.TUNE_TB_PERSISTENT, 0)
                    g.set_tuning(M.TUNE_TB_VARIANT, variant)
                    g.set_tuning(M.TUNE_TSTEPS, T)
                    g.set_tuning(M.TUNE_TB_ROWS, rows)
                    g.set_tuning(M.TUNE_XCD_REMAP, remap)
                    assert g.get_tuning(M.TUNE_TB_PERSISTENT) == 0
                    assert g.get_tuning(M.TUNE_TB_ROWS) == rows
                    g.upload(M.P, p)
                    g.upload(M.RHS, rhs)
                    it, res = g.solve_rb()
                    st = g.stats()
                    assert (st["tb_variant"], st["chained"], st["iters_per_pass"]) == \
                        (variant, 0, T), st
                    check(g.download(M.P), want, it, it_ref, res, res_ref, (k, rows, remap))


# ---------------------------------------------------------------------------
# 5. the exact tail under a non-default sweep variant
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tail_case():
    """eps between the residual of iteration k* (20 <= k* < 40) and the smallest
    one before it: solveRB stops at k*.  The random fields times 2^-40 (exact:
    the same solve scaled), so that every residual is below the 1.0 solveRB's
    loop starts from and the loop runs at all"""
    ni, nj = 300, 190
    p, rhs, dx, dy = case(ni, nj, 1)[:4]
    p, rhs = p * 2.0 ** -40, rhs * 2.0 ** -40
    q, res = p.copy(), {}
    for k in range(1, 40):
        res[k] = orc.solve_rb(q, rhs, dx, dy, OMEGA, 1e-300, 1)[1]
    ks = next(k for k in range(20, 40)
              if res[k] < min(res[j] for j in range(1, k)) * (1 - 1e-6))
    eps = ((res[ks] + min(res[j] for j in range(1, ks))) / 2) ** 0.5
    want = p.copy()
    it_ref, res_ref = orc.solve_rb(want, rhs, dx, dy, OMEGA, eps, 100000)
    assert it_ref == ks
    want.setflags(write=False)
    return ni, nj, p, rhs, dx, dy, eps, want, it_ref, res_ref


def test_exact_tail_under_other_sweep_variant():
    """NEAR_BAND = -30: every iteration goes through exact_tail, whose sweep is
    the default variant's (8 strips, automatic rows: 48 blocks here) whatever
    is configured -- here variant 0 at 190 rows, a launch of one block.  p and
    the count as the oracle's; it and res the same bits as at the default
    variant: only the exact sum is independent of the geometry (the batched
    passes' res differs in its last bits between 1 and 48 blocks), so the equal
    bits are what shows that the exact path ran.

    Not covered: the regrowth of the partials in that branch (misor_solve.hip
    `sp.nblocks > g->partials_cap`).  misor_create configures the default
    variant's automatic geometry first (set_geometry -> configure_sweep), which
    sizes the partials for exactly the launch the tail rebuilds, and
    ensure_partials never shrinks: the condition is false on every grid
    misor_create makes.  The line is dead code, left for a later change."""
    ni, nj, p, rhs, dx, dy, eps, want, it_ref, res_ref = tail_case()
    assert sweep_blocks(ni, nj, 0, 190) == (1, 1)
    assert sweep_blocks(ni, nj, DEFAULT_VARIANT, 0) == (1, 48)
    out = {}
    for variant, rows in ((0, 190), (DEFAULT_VARIANT, 0)):
        with M.Grid(ni, nj, dx, dy, OMEGA, eps, 100000) as g:
            g.set_tuning(M.TUNE_NEAR_BAND, -30)
            set_sweep(g, variant, rows, 1)
            g.upload(M.P, p)
            g.upload(M.RHS, rhs)
            it, res = g.solve_rb()
            st = g.stats()
            assert ran_single_sweep(st), st
            check(g.download(M.P), want, it, it_ref, res, res_ref, variant)
            out[variant] = (it, res)
    assert out[0] == out[DEFAULT_VARIANT], out


# ---------------------------------------------------------------------------
# 6. knobs changed between solves of one grid
# ---------------------------------------------------------------------------

def test_knobs_changed_between_solves():
    """one grid: a solve at the defaults (chained passes of the automatic T),
    then other sweep knobs (configure_sweep also writes the blocked passes'
    xcd_remap and keeps their chain plans), then back; then the same with T = 1,
    where the single sweep itself runs on the grid the blocked passes used, and
    T automatic again.  The same p goes up before every solve."""
    ni, nj, k = 1000, 150, 19
    p, rhs, dx, dy, want, it_ref, res_ref = case(ni, nj, k)
    with M.Grid(ni, nj, dx, dy, OMEGA, 1e-300, k) as g:
        g.set_tuning(M.TUNE_SMALL_SOLVE, 0)
        g.upload(M.RHS, rhs)

        def again(what, single):
            g.upload(M.P, p)
            it, res = g.solve_rb()
            st = g.stats()
            assert ran_single_sweep(st) if single else st["iters_per_pass"] > 1, (what, st)
            check(g.download(M.P), want, it, it_ref, res, res_ref, what)

        again("defaults", False)
        g.set_tuning(M.TUNE_XCD_REMAP, 0)
        g.set_tuning(M.TUNE_SWEEP_VARIANT, 14)
        g.set_tuning(M.TUNE_ROWS_PER_BLOCK, 7)
        again("remap 0, variant 14, rows 7", False)
        g.set_tuning(M.TUNE_XCD_REMAP, 1)
        g.set_tuning(M.TUNE_SWEEP_VARIANT, 7)
        again("remap 1, variant 7", False)
        # the single sweep on the same grid, its knobs changed between solves
        g.set_tuning(M.TUNE_TSTEPS, 1)
        again("T = 1, variant 7, rows 7", True)
        g.set_tuning(M.TUNE_XCD_REMAP, 0)
        g.set_tuning(M.TUNE_SWEEP_VARIANT, 14)
        g.set_tuning(M.TUNE_ROWS_PER_BLOCK, 1)
        assert sweep_blocks(ni, nj, 14, 1) == (1, 150)
        again("T = 1, remap 0, variant 14, rows 1", True)
        g.set_tuning(M.TUNE_SWEEP_VARIANT, 0)
        g.set_tuning(M.TUNE_ROWS_PER_BLOCK, 0)
        g.set_tuning(M.TUNE_XCD_REMAP, 1)
        again("T = 1, remap 1, variant 0, automatic rows", True)
        g.set_tuning(M.TUNE_TSTEPS, 0)
        again("T automatic again", False)


# ---------------------------------------------------------------------------
# 7. errors (misor_create needs a device, so not beside the ABI tests)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [-1, len(SWEEP_VARIANTS)])
def test_bad_sweep_variant_is_refused(bad):
    ni, nj = ROWS_SHAPE
    k = 3
    p, rhs, dx, dy, want, it_ref, res_ref = case(ni, nj, k)
    with M.Grid(ni, nj, dx, dy, OMEGA, 1e-300, k) as g:
        set_sweep(g, 2, 7, 0)
        # MISOR_EINVAL (-1) from configure_sweep, not just any failure
        with pytest.raises(M.MisorError, match=r"error -1: bad variant"):
            g.set_tuning(M.TUNE_SWEEP_VARIANT, bad)
        assert g.get_tuning(M.TUNE_SWEEP_VARIANT) == 2
        assert g.get_tuning(M.TUNE_ROWS_PER_BLOCK) == 7
        assert g.get_tuning(M.TUNE_XCD_REMAP) == 0
        g.upload(M.P, p)
        g.upload(M.RHS, rhs)
        it, res = g.solve_rb()
        check(g.download(M.P), want, it, it_ref, res, res_ref, bad)
