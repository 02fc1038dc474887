"""CPU: the panels and the reference of tests/sweep_ref.py can tell a wrong sweep from a right one.

tests/test_gpu_sweep.py holds tpg_sweep_kernel / run_sweep (csrc/pca.hip) to sweep_exact() bit for bit on the exact panels and
to sweep_bound() on the general ones.  Here, without a GPU: the exactness claim itself (three orders of float64 addition give
sweep_exact() in every bit, on every panel of the GPU grid); every fault model of sweep_ref.FAULTS moves at least one element of
every exact panel it applies to, and leaves sweep_bound() on the general panels; the pairs a fault does not apply to are the
ones listed in NOT_APPLICABLE, with the reason; the shapes reach the split counts they were chosen for.
"""
import numpy as np
import pytest

from tests import sweep_ref as sr

CASES = [("colscale",) + c for c in sr.T_CASES] + [("valid",) + c for c in sr.T_CASES] + [("rowscale",) + c for c in sr.L_CASES]
SHAPES = [(mode, n, m) for mode in ("colscale", "valid") for (n, m) in sr.T_SHAPES] + [("rowscale", n, m) for (n, m) in sr.L_SHAPES]


def _S(mode, n, m):
    return (sr.L_SHAPES if mode == "rowscale" else sr.T_SHAPES)[(n, m)]


_exact = {}


def _want(mode, n, m, K):
    """sweep_exact at KMAX columns once per (mode, shape); a case reads its first K columns (a column's sum does not depend on K)"""
    if (mode, n, m) not in _exact:
        _exact[(mode, n, m)] = sr.sweep_exact(mode, *sr.panel("exact", n, m).args(mode, sr.KMAX))
    out, rss = _exact[(mode, n, m)]
    return out[:, :K], rss


def test_shapes_reach_their_split_counts():
    for mode, n, m in SHAPES:
        assert sr.splits(mode, n, m, 256) == _S(mode, n, m), (mode, n, m)
    lens = lambda nb, S: [b1 - b0 for b0, b1 in sr.split_bounds(nb, S)]
    assert sr.dims("colscale", 130, 767)[1] == 6 and lens(6, 4) == [1, 2, 1, 2]
    assert sr.dims("colscale", 130, 769)[1] == 7 and lens(7, 4) == [1, 2, 2, 2]
    assert sr.dims("rowscale", 643, 300)[1] == 6 and sr.dims("colscale", 130, 12805)[1] == 101
    assert len(set(lens(101, 64))) == 2  # S = 64: ranges of one and of two blocks
    # the crossing: every K with a shape of S > 1 and a ragged shape, every shape with K = 4 and K = 21
    for shapes, cases in ((sr.T_SHAPES, sr.T_CASES), (sr.L_SHAPES, sr.L_CASES)):
        for K in sr.KS:
            mine = [(n, m) for n, m, k in cases if k == K]
            assert any(shapes[s] > 1 for s in mine) and any(s[0] % 32 and s[1] % 128 for s in mine), K
        for s in shapes:
            assert {4, 21} <= {k for n, m, k in cases if (n, m) == s}
    assert [sr.passes(K) for K in (1, 4, 5, 21, 41, 64)] == [[(0, 1)], [(0, 4)], [(0, 5)], [(0, 20), (20, 1)], [(0, 20), (20, 20), (40, 1)],
                                                            [(0, 20), (20, 20), (40, 20), (60, 4)]]


@pytest.mark.parametrize("n,m", list(sr.T_SHAPES) + list(sr.L_SHAPES))
def test_exact_panels_are_on_the_grid_and_carry_their_edges(n, m):
    p = sr.panel("exact", n, m)
    G = p.G
    assert set(np.unique(4 * p.center).tolist()) <= set(range(9)) and set(p.scale.tolist()) <= set(sr.SCALES)
    assert np.array_equal(p.V, np.round(p.V)) and np.array_equal(p.U, np.round(p.U)) and max(np.abs(p.V).max(), np.abs(p.U).max()) <= 2 ** 20
    assert np.all(np.frexp(p.d)[0] == 0.5)
    for T in (p.V, p.U):
        assert len({T[:, k].tobytes() for k in range(sr.KMAX)}) == sr.KMAX and np.all(T[-1] != 0)
    k = np.arange(sr.KMAX)
    for back in (20, 40, 60):
        assert np.all(p.d[k[back:]] != p.d[k[back:] - back])
    if n < 3 or m < 3:
        assert (n, m) == (1, 1) and G[0, 0] != 3
        return
    miss = G == 3
    assert miss[n // 2].all() and miss[:, m // 3].all()
    for a, size, step in [(ax, sz, st) for ax, sz in ((0, n), (1, m)) for st in (32, 128)]:
        for b in range(step, size, step):
            lo, hi = np.take(miss, b - 1, axis=a), np.take(miss, b, axis=a)
            assert lo.any() and hi.any() and not lo.all() or b - 1 in (n // 2, m // 3) or b in (n // 2, m // 3), (a, b)
    assert miss[n - 1].any() and not miss[n - 1].all() and miss[:, m - 1].any() and not miss[:, m - 1].all()
    assert not miss[n - 1, m - 1]


@pytest.mark.parametrize("mode,n,m", SHAPES)
def test_three_orders_of_float64_addition_equal_the_integer_reference(mode, n, m):
    """the exactness claim of sweep_ref's docstring: no addition rounds, so the order cannot matter"""
    args = sr.panel("exact", n, m).args(mode, sr.KMAX)
    want, want_rss = _want(mode, n, m, sr.KMAX)
    orders = [("forward", 1), ("reversed", 1), ("split", _S(mode, n, m))]
    if _S(mode, n, m) == 1 and sr.dims(mode, n, m)[1] > 1:
        orders.append(("split", 2))
    for order, S in orders:
        got, rss = sr.sweep_model(mode, *args, order=order, S=S)
        assert np.array_equal(got, want), (order, S)
        assert (rss is None) == (want_rss is None) and (rss is None or np.array_equal(rss, want_rss)), (order, S)


# fault, where it does not apply (a predicate of mode, rows of the sweep, K, S, panel), the reason the fault model gives
NOT_APPLICABLE = {
    "last_column_dropped": [],
    "last_block_dropped": [],
    "split_off_by_one_block": [(lambda mode, nrows, K, S, p: S == 1, "one range: there is no boundary between ranges")],
    "pass_reads_tab_of_pass_0": [(lambda mode, nrows, K, S, p: K <= 20, "K <= 20: one pass")],
    "rss_from_last_pass": [(lambda mode, nrows, K, S, p: True, "z does not depend on the pass: every pass would give the same rss")],
    "rss_added_in_every_pass": [(lambda mode, nrows, K, S, p: mode != "colscale", "no rss is returned in this mode"),
                                (lambda mode, nrows, K, S, p: K <= 20, "K <= 20: one pass")],
    "missing_counted_as_3": [(lambda mode, nrows, K, S, p: not (p.G == 3).any(), "no missing genotype in the panel")],
    "center_scale_of_neighbour": [(lambda mode, nrows, K, S, p: mode == "valid", "no center or scale in this mode"),
                                  (lambda mode, nrows, K, S, p: p.m < 2, "one locus: no neighbour")],
    "padded_rows_one_up": [(lambda mode, nrows, K, S, p: nrows % 32 == 0, "the rows fill their last 32-tile: no padded row")],
    "col_div_of_pass_0": [(lambda mode, nrows, K, S, p: mode != "rowscale", "no col_div in this mode"),
                          (lambda mode, nrows, K, S, p: K <= 20, "K <= 20: one pass")],
}
# How many of the 76 exact cases (30 T cases in two modes, 16 L cases) each fault does not apply to: the table above, counted
# by hand from the grid.  S = 1: three T shapes and two L shapes at K = 4 and 21 (3 * 2 * 2 + 2 * 2).  K <= 20: 9 + 6 T cases
# in two modes, 5 + 3 L cases.  rss: the 46 cases outside "colscale" and its 15 of K <= 20.  No missing genotype: (1, 1), two K,
# two modes.  Neighbour: the 30 "valid" cases and (1, 1) under "colscale".  No padded row: (32, 128), two K, two modes (no L
# shape has a multiple of 32 loci).  col_div: the 60 T cases and the 8 L cases of K <= 20.
N_NOT_APPLICABLE = {"last_column_dropped": 0, "last_block_dropped": 0, "split_off_by_one_block": 16, "pass_reads_tab_of_pass_0": 38,
                    "rss_from_last_pass": 76, "rss_added_in_every_pass": 61, "missing_counted_as_3": 4,
                    "center_scale_of_neighbour": 32, "padded_rows_one_up": 4, "col_div_of_pass_0": 68}


def _expected_reason(fault, mode, nrows, K, S, p):
    for pred, reason in NOT_APPLICABLE[fault.__name__]:
        if pred(mode, nrows, K, S, p):
            return reason
    return None


def _differs(got, want):
    out, rss = got
    return (not np.array_equal(out, want[0])) or (rss is not None and not np.array_equal(rss, want[1]))


def test_fault_list_is_the_table():
    assert [f.__name__ for f in sr.FAULTS] == list(NOT_APPLICABLE)


@pytest.mark.parametrize("fault", sr.FAULTS, ids=[f.__name__ for f in sr.FAULTS])
def test_every_fault_moves_an_element_of_every_exact_panel_it_applies_to(fault):
    skipped = 0
    for mode, n, m, K in CASES:
        p = sr.panel("exact", n, m)
        S = _S(mode, n, m)
        reason = _expected_reason(fault, mode, sr.dims(mode, n, m)[2], K, S, p)
        if reason is not None:
            with pytest.raises(sr.NotApplicable) as e:
                fault(mode, *p.args(mode, K), S)
            assert str(e.value) == reason, (mode, n, m, K)
            skipped += 1
            continue
        got = fault(mode, *p.args(mode, K), S)  # (NotApplicable here = a pair the table does not list: an error)
        assert _differs(got, _want(mode, n, m, K)), (fault.__name__, mode, n, m, K, "the fault changes no element")
    assert skipped == N_NOT_APPLICABLE[fault.__name__], (fault.__name__, skipped)


_general = {}


def _general_case(mode):
    if mode not in _general:
        n, m = sr.GENERAL[mode]
        args = sr.panel("general", n, m).args(mode, 21)
        _general[mode] = (args, sr.sweep_fraction(mode, *args), sr.sweep_bound(mode, *args), sr.splits(mode, n, m, 256))
    return _general[mode]


def _excess(got, ref, bound):
    """largest |got - ref| / bound over out and rss: above 1 = some element has left the bound (sr.excess: a bound of 0, the
    row typed nowhere, allows no error at all)"""
    return sr.excess(got, ref, bound)


@pytest.mark.parametrize("mode", sr.MODES)
def test_float64_sums_stay_inside_the_derived_bound(mode):
    args, ref, bound, S = _general_case(mode)
    assert S == 2 and np.count_nonzero(bound[0] == 0) <= bound[0].shape[1]  # (one row typed nowhere at the most)
    for order, s in (("forward", 1), ("reversed", 1), ("split", S)):
        assert _excess(sr.sweep_model(mode, *args, order=order, S=s), ref, bound) <= 1.0, order


@pytest.mark.parametrize("fault", sr.FAULTS, ids=[f.__name__ for f in sr.FAULTS])
@pytest.mark.parametrize("mode", sr.MODES)
def test_every_fault_leaves_the_bound_on_the_general_panels(mode, fault):
    args, ref, bound, S = _general_case(mode)
    n, m = sr.GENERAL[mode]
    reason = _expected_reason(fault, mode, sr.dims(mode, n, m)[2], 21, S, sr.panel("general", n, m))
    if reason is not None:
        with pytest.raises(sr.NotApplicable) as e:
            fault(mode, *args, S)
        assert str(e.value) == reason
        return
    # out of the bound, and not by a hair: the bound is ~ 1e-14 of an element's majorant, a lost term 1e-3 of it or more
    assert _excess(fault(mode, *args, S), ref, bound) > 1e6, (fault.__name__, mode)
