"""Cross-list steals of the chained split-ring pass (TB variant 13), forced
and observed (MISOR_TUNE_EDGE_STEAL; misor_solve.hip's whole-pass fork,
sor_tbh.h rb_tbhc_kernel's alt loop, sor_tb.h chain_acquire(..., alt_n0)).

In a whole pass the edge kernel's workgroups, their own list done, take runs
of 4 or more unclaimed blocks from the main kernel's list.  EDGE_STEAL = 2
launches the main kernel in stream order behind the edge kernel, so the edge
workgroups find every main segment whole and split each until its owner keeps
fewer than 4 blocks: of a segment of n >= 4 blocks they run at least
n - 3 >= n / 4.  The chain trace (MISOR_CHAIN_TRACE=1) marks a block run by
the edge kernel with bit 33 of its third word.  Residual partials go to fixed
slots, so who ran a block changes no bit: p is the restatement's
(assignment-4/src/solver.c:179-238, orc.solve_rb_mt) bit for bit, ghosts
included, and res is bit-equal among EDGE_STEAL 0, 1 and 2.

Shapes.  Blocks are one ring length tall (MISOR_TUNE_TB_ROWS = S: 6, 12, 18
rows at T = 2, 5, 10) and 4 strips of 128 - 4T columns wide; 4 block columns,
the first and the last of them edge columns (a strip at a physical left /
right side), the two between them the main list's.  tb_plan.h chain_lists
cuts a column's steady run into segments of cost / G blocks, G the resident
workgroups: cost = 1 per main block, 2.5 per edge-column block, 2.5 (S + 4T) /
S per block whose cone reaches the bottom / top side (those are segments of
one block in the main list, whichever column).  The compiled kernels hold 135,
191 and 256 VGPRs at T = 2, 5, 10, so 3, 2, 2 workgroups a CU: G = 768, 512,
512 on 256 CUs.  nj below gives cost / G = 10.1, 10.0, 10.1 (plan_cost), so
the main segments are 10 blocks long (8 or more up to G = 970, 643, 648; 4 or
more -- what the assertion needs -- up to twice that):

    T   ni    nj     block rows  cells   cost
    2   1920  6601   1101        12.7 M  7756
    5   1728  8707   726         15.0 M  5141
    10  1408  13057  726         18.4 M  5183
    10  1231  13057  the same, ragged: ni odd, the last column 2 strips, 175 columns

Observed on an MI355X with EDGE_STEAL = 2 (stolen blocks / steady blocks of
the main columns, the same for both spacings and RES_LITE settings): T = 2
1542 / 2196 = 0.702, T = 5 1014 / 1446 = 0.701, T = 10 1018 / 1444 = 0.705 on
both T = 10 shapes; with EDGE_STEAL = 0 none.  The launches had 544 + 224,
360 + 152 and 356 + 156 workgroups (edge + main kernel): G = 768, 512, 512.
"""
import functools

import numpy as np
import pytest

import orc
import pymisor as M
from test_tb_variants_gpu import hr_slots

pytestmark = pytest.mark.gpu

W = 4  # strips per workgroup
SHAPES = {2: (1920, 6601), 5: (1728, 8707), 10: (1408, 13057)}
RAGGED = (10, 1231, 13057)


def ring(T):
    return hr_slots(T, sk=1 if T >= 2 else 0)


def geometry(ni, nj, T):
    """block columns and rows of a pass of T iterations with blocks of one ring
    length; per column: an edge column? (tb_plan.h tb_edge_col);
    per block row: steady-able? (sor_tbh.h hr_chain_rows_ok, one rank)"""
    S, OW = ring(T), 128 - 4 * T
    nbx = -(-(-(-ni // OW)) // W)
    nby = -(-nj // S)

    def edge_col(bx):
        for w in range(W):
            c_out = 1 + (bx * W + w) * OW
            if c_out > ni:
                break
            c_ld = c_out - 2 * T
            if not (c_ld >= 1 and c_ld + 127 <= ni and (c_out + OW - 1 <= ni or ni % 2 == 0)):
                return True
        return False

    def steady(by):
        j0 = 1 + by * S
        j1 = nj + 1 if by == nby - 1 else j0 + S
        return j0 - 2 * T >= 1 and j1 - 1 + 2 * T <= nj and (j1 - j0) % S == 0

    return (nbx, nby, np.array([edge_col(bx) for bx in range(nbx)]),
            np.array([steady(by) for by in range(nby)]))


def plan_cost(ni, nj, T):
    """chain_plan's cost of a whole pass, in steady main blocks"""
    nbx, nby, ecol, steady = geometry(ni, nj, T)
    S = ring(T)
    single = 2.5 * (S + 4.0 * T) / S
    ns = int(steady.sum())
    return ns * (2.5 * ecol.sum() + (~ecol).sum()) + (nby - ns) * nbx * single


def test_shapes_give_long_segments():
    """the docstring's arithmetic: cost / G >= 10 at the G the compiled
    kernels' registers give, two main columns between two edge columns, a
    ragged last block row"""
    for (T, ni, nj), G in zip([(T, *SHAPES[T]) for T in (2, 5, 10)] + [RAGGED],
                              (768, 512, 512, 512)):
        nbx, nby, ecol, steady = geometry(ni, nj, T)
        assert ecol.tolist() == [True, False, False, True]
        assert plan_cost(ni, nj, T) / G >= 10.0, (T, ni, plan_cost(ni, nj, T))
        assert nj % ring(T) != 0
    assert RAGGED[1] % 2 == 1 and RAGGED[1] % (W * (128 - 4 * RAGGED[0])) != 0


# (one case at a time: the fields are 100-150 MB each; the parameters are
# ordered so that the cases sharing one follow each other)
@functools.lru_cache(maxsize=1)
def case(T, ni, nj, pow2):
    """random normal fields (test_tb_variants_gpu.fields) and the
    restatement's p and res after T and 2T + 1 iterations"""
    rng = np.random.default_rng(ni + 7 * nj + T + (1 if pow2 else 0))
    p = rng.standard_normal((nj + 2, ni + 2))
    rhs = rng.standard_normal((nj + 2, ni + 2)) * 10
    dx, dy = (2.0 ** -12, 2.0 ** -12) if pow2 else (1.1 / ni, 0.9 / nj)
    want, q = {}, p.copy()
    it, res = orc.solve_rb_mt(q, rhs, dx, dy, 1.7, 1e-300, T, 16)
    assert it == T
    want[T] = (q.copy(), res)
    # (the next T + 1 iterations from there: the state after 2T + 1)
    it, res = orc.solve_rb_mt(q, rhs, dx, dy, 1.7, 1e-300, T + 1, 16)
    assert it == T + 1
    want[2 * T + 1] = (q, res)
    for a in (p, rhs, want[T][0], q):
        a.setflags(write=False)
    return p, rhs, dx, dy, want


def check_steals(T, lite, ni, nj, pow2, monkeypatch):
    monkeypatch.setenv("MISOR_CHAIN_TRACE", "1")  # read when the passes are configured
    p, rhs, dx, dy, want = case(T, ni, nj, pow2)
    nbx, nby, ecol, steady = geometry(ni, nj, T)
    col = np.arange(nbx * nby) % nbx  # block L = by * nbx + bx
    in_main_col = ~ecol[col]
    is_steady = steady[np.arange(nbx * nby) // nbx]
    with M.Grid(ni, nj, dx, dy, 1.7, 1e-300, 2 * T + 1) as g:
        g.set_tuning(M.TUNE_SMALL_SOLVE, 0)
        g.set_tuning(M.TUNE_TB_VARIANT, 13)
        g.set_tuning(M.TUNE_TSTEPS, T)
        g.set_tuning(M.TUNE_TB_ROWS, ring(T))
        g.set_tuning(M.TUNE_RES_LITE, lite)
        assert g.get_tuning(M.TUNE_EDGE_STEAL) == 1  # the default
        g.upload(M.RHS, rhs)
        for k in (T, 2 * T + 1):
            p_ref, res_ref = want[k]
            runs = {}
            for steal in (2, 0, 1):
                g.set_tuning(M.TUNE_EDGE_STEAL, steal)
                assert g.get_tuning(M.TUNE_EDGE_STEAL) == steal
                g.upload(M.P, p)
                it, res = g.solve_rb(itermax=k)
                got = g.download(M.P)
                st = g.stats()
                assert (st["tb_variant"], st["chained"], st["iters_per_pass"]) == (13, 1, T)
                assert it == k
                assert np.array_equal(got, p_ref), (k, steal, np.argwhere(got != p_ref)[:5])
                assert abs(res - res_ref) <= 1e-12 * res_ref, (k, steal, res, res_ref)
                runs[steal] = res
                if k != T or steal == 1:
                    continue
                # the one pass of the k = T solve: who ran each block
                tr = g.chain_trace()
                assert tr is not None and tr.shape == (nbx * nby, 3)
                assert (tr[:, 1] != 0).all(), "a block without an end time"
                by_edge = ((tr[:, 2] >> np.uint64(33)) & np.uint64(1)).astype(bool)
                stolen = by_edge & in_main_col
                share = stolen.sum() / (in_main_col & is_steady).sum()
                print("T %d lite %d %dx%d pow2 %d steal %d: %d blocks, main columns %d steady; "
                      "edge kernel ran %d, %d of them stolen (share %.3f); workgroups: edge "
                      "%d, main %d" % (T, lite, ni, nj, pow2, steal, len(tr),
                                       (in_main_col & is_steady).sum(), by_edge.sum(),
                                       stolen.sum(), share,
                                       (tr[by_edge, 2] & np.uint64(0xffffffff)).max() + 1,
                                       (tr[~by_edge, 2] & np.uint64(0xffffffff)).max() + 1))
                # the edge list is the steady blocks of the edge columns; a block
                # whose cone reaches the bottom / top side is a segment of one
                # block in the main list: never stolen (steals take 4 or more)
                assert by_edge[~in_main_col & is_steady].all()
                assert not by_edge[~is_steady].any()
                if steal == 0:
                    assert not stolen.any()
                else:
                    assert stolen.any(), "the forced order stole nothing"
                    assert 4 * stolen.sum() >= (in_main_col & is_steady).sum(), share
            assert runs[0] == runs[1] == runs[2], (k, runs)


@pytest.mark.parametrize("T,lite", [(2, 1), (5, 1), (10, 1), (10, 0)])
@pytest.mark.parametrize("pow2", [False, True])
def test_forced_steals(T, lite, pow2, monkeypatch):
    """general spacing and dx = dy = 2^-12; T = 10 with the residual lower
    bounds on (the LITE steady chunks run on stolen runs in the k = T pass)
    and off"""
    check_steals(T, lite, *SHAPES[T], pow2, monkeypatch)


@pytest.mark.parametrize("lite", [1, 0])
def test_forced_steals_ragged_last_column(lite, monkeypatch):
    """ni odd and no multiple of the column width: the last column has two
    strips, the second ragged"""
    check_steals(RAGGED[0], lite, RAGGED[1], RAGGED[2], False, monkeypatch)


def test_bad_edge_steal_refused():
    with M.Grid(300, 190, 1.0 / 300, 1.0 / 190, 1.7, 1e-300, 10) as g:
        for bad in (-1, 3):
            with pytest.raises(M.MisorError):
                g.set_tuning(M.TUNE_EDGE_STEAL, bad)
            assert g.get_tuning(M.TUNE_EDGE_STEAL) == 1
