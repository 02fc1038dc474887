"""CPU: the references, panels and fault models of tests/loadings_ref.py can tell a wrong loadings kernel from a right one.

tests/test_gpu_loadings_exact.py holds tpg_pca_loadings (csrc/pca.hip: the digit, column-sum, MFMA and finalize kernels) to
exact_loadings() with np.array_equal on the exact panels and to bound() on the general ones.  Here, without a GPU:

  - the exactness claim, in integers, on every exact case of the GPU grid: 2 S - 2 c Wsum fits 53 bits, so no operation of
    the finalize expression rounds, fused or not, and exact_loadings() IS that integer times a power of two;
  - the derived bound holds for the unfused and for the fused evaluation (one rounding of the exact difference, in rationals) of
    the general panels;
  - the restated launch plan gives G'W again in both layouts, and says what the issue's shape lists were chosen for;
  - every fault model moves at least one cell of every named exact panel it applies to; the pairs it does not apply to are the
    ones NOT_APPLICABLE lists, with the reason, and counted;
  - the faults that move a result by less than 2^-30 of its size pass the 1e-9 assertion of tests/test_gpu_loadings.py.
"""
from fractions import Fraction

import numpy as np
import pytest

from tests import loadings_ref as lr

_cache = {}


def _panel(case):
    layout, n, m, k, kind = case
    key = (n, m, k, kind)
    if key not in _cache:
        _cache[key] = lr.exact_panel(n, m, k, kind)
    return _cache[key]


def test_grid_reaches_the_depths_it_was_chosen_for():
    assert [lr.chunks(n) for n in lr.N_ROWS] == [1, 1, 1, 2, 3, 4, 4, 5, 6, 8, 9, 9]
    assert [lr.chunks(n) for n in lr.N_LM] == [1, 1, 2, 3, 3, 4, 5, 8, 9]
    assert all(n % 8 == 0 for n in lr.N_LM) and all(n % 8 == 0 for n in lr.N_EDGE["locus_major"])
    assert [[lr.chunks(n) for n in lr.N_EDGE[l]] for l in ("rows", "locus_major")] == [[1, 3, 5], [1, 3, 5]]
    # launches: 1, 2, 3, 4, 4 + 1, 4 + 2, 4 + 3, 4 + 4 + 1, 4 + 4 + 4 column tiles, and straddling components from k = 6 on
    assert [[w for _, w in lr.launches(k)[1]] for k in lr.KS] == [[1], [1], [2], [3], [3], [4], [4, 1], [4, 2], [4, 3], [4, 4, 1],
                                                                  [4, 4, 4]]
    # loci: (tiles, workgroups, idle waves).  m <= 128: waves 0 and 1 own the four tiles (of which 3, 2, 2 or 0 are padding
    # alone), waves 2 and 3 are idle; 129 .. 256: one full workgroup; 257 .. 289: a second one, half idle
    assert [(lr.grid(m)[0], lr.grid(m)[1], len(lr.grid(m)[2])) for m in lr.M_EDGES] == \
        [(4, 1, 2), (4, 1, 2), (4, 1, 2), (4, 1, 2), (8, 1, 0), (8, 1, 0), (12, 2, 2), (12, 2, 2)]


@pytest.mark.parametrize("lm", [False, True])
def test_pipeline_hands_every_group_its_own_chunk_and_fragments(lm):
    """the slots and LDS buffers, tracked as the kernel assigns them, at every depth up to 13 (three times the unroll and one)"""
    for Q in range(1, 14):
        used = lr.pipeline(Q, lm)
        assert [u for _, u in used] == list(range(Q))
        if lm:
            assert [base + dq for (base, dq), _ in used] == list(range(Q))
            for (base, dq), _ in used:  # the lane trade: lane (r, h) ends with piece (chunk q, locus r, h) in every dword
                chunk, locus, h = lr.lm_lane_map(Q, base, dq)
                i = np.arange(64)
                assert (chunk == base + dq).all() and (locus == (i & 31)).all() and (h == (i >> 5)).all()
        else:
            assert [g for g, _ in used] == list(range(Q))


@pytest.mark.parametrize("case", lr.EXACT_CASES, ids=lr.case_id)
def test_exact_tier_rounds_nowhere(case):
    p = _panel(case)
    S, Wsum, FU = lr.quantised_sums(p.G, p.U)
    c2 = (2 * p.center).astype(np.int64)
    assert np.array_equal(c2 / 2.0, p.center)
    N2 = 2 * S - c2[:, None] * Wsum[None, :]  # = 2 (gu - c usum) 2^FU
    lim = 2 ** 53
    # gu, usum, c usum (Wsum times 0, 1/2, 1 or 2) and the difference are integers below 2^53 times a power of two: doubles
    assert np.abs(S).max() < lim and np.abs(Wsum).max() < lim and np.abs(N2).max() < lim
    es, ed = np.frexp(p.scale)[1] - 1, np.frexp(p.d)[1] - 1
    assert np.array_equal(np.ldexp(1.0, es), p.scale) and np.array_equal(np.ldexp(1.0, ed), p.d)
    sh = (-FU - 1 - es[:, None] - ed[None, :]).astype(np.int32)
    want = np.ldexp(N2.astype(np.float64), sh)  # the exact value, if it neither overflows nor goes subnormal
    nz = want != 0
    assert np.isfinite(want).all() and (np.abs(want[nz]) > 2.0 ** -960).all() and np.array_equal(nz, N2 != 0)
    ref = lr.exact_loadings(*p.args())
    assert np.array_equal(ref, want)
    # a few cells in rationals from the start, and the fused route on them
    for j, kk in {(0, 0), (p.m - 1, p.k - 1), (p.m // 2, p.k // 3)}:
        exact = (Fraction(int(S[j, kk])) - Fraction(p.center[j]) * int(Wsum[kk])) * Fraction(2) ** (-FU) \
            / (Fraction(p.scale[j]) * Fraction(p.d[kk]))
        assert Fraction(ref[j, kk]) == exact
    if p.m * p.k <= 200:
        assert np.array_equal(lr.finalize(S, Wsum, FU, p.center, p.scale, p.d, fused=True), ref)


@pytest.mark.parametrize("case", lr.EXACT_CASES, ids=lr.case_id)
def test_restated_launch_plan_gives_the_integer_sums(case):
    p = _panel(case)
    S, _, FU = lr.quantised_sums(p.G, p.U)
    assert np.array_equal(lr.model_sums(p.G, lr.fixed(p.U, FU), case[0] == "locus_major"), S)


def test_single_entry_panel_names_every_byte_position():
    """m = 256: each individual of the first and of the last chunk owns one locus, and S there is g times its W"""
    for n in (520, 641):
        G, rows = lr.single_entry_genotypes(n, 256)
        Q = lr.chunks(n)
        assert set(rows[0::2]) == set(range(128)) and set(rows[1::2]) == set(range(128 * (Q - 1), n))
        assert (G.sum(axis=0) == G[rows, np.arange(256)]).all() and set(G[rows, np.arange(256)]) == {1, 2}


def test_prescribed_digits_are_what_they_say():
    n, k = 264, 3
    dg = {name: lr.digits(lr.fixed(U, lr.exponent(U)[1])) for name, U in ((nm, f(n, k)) for nm, f in lr.PRESCRIBED.items())}
    assert (dg["digits_min_max"][:5] == -64).all(axis=0).any() and (dg["digits_min_max"][:5] == 63).all(axis=0).any()
    assert (int(dg["digits_min_max"][5].min()), int(dg["digits_min_max"][5].max())) == (-31, 32)  # (2^40 - 1 is 32 | 0 ... | -1)
    W = lr.fixed(lr.w_carries(n, k), 40)
    assert (W == 64 * lr.LOW5).any() and (W == -65 * lr.LOW5).any()
    assert [int(d) for d in lr.digits(np.array([64 * lr.LOW5]))[:, 0]] == [-64, -63, -63, -63, -63, 1]   # the carry runs through
    assert [int(d) for d in lr.digits(np.array([-65 * lr.LOW5]))[:, 0]] == [63, 62, 62, 62, 62, -1]      # and the borrow
    assert lr.exponent(lr.PRESCRIBED["tiny"](n, k))[1] == 40 + 664 and lr.exponent(lr.PRESCRIBED["huge"](n, k))[1] == 40 - 665
    assert np.abs(lr.fixed(lr.w_pm_full(n, k), 40)).max() == 2 ** 40 - 1
    sp = lr.fixed(lr.spike_U(n, k), lr.exponent(lr.spike_U(n, k))[1])
    assert np.abs(sp[:, 2]).max() < 2 ** 38  # beside the spike the other columns live in the low digits


# ---------------------------------------------------------------------------------------------------------------------
# the general tier
GENERAL = [(1152, 24, 6), (641, 17, 5), (8, 9, 2)]


@pytest.mark.parametrize("n,m,k", GENERAL)
def test_derived_bound_holds_unfused_and_fused(n, m, k):
    """|v - N / D| <= 2^-53 (|c usum| + 4 |N|) / |D|: see the derivation in tests/loadings_ref.py.  Unfused is numpy's own FP64;
    fused rounds the exact gu - c usum once"""
    p = lr.general_panel(n, m, k)
    S, Wsum, FU = lr.quantised_sums(p.G, p.U)
    N, D, P = lr.rational_loadings(*p.args())
    for fused in (False, True):
        got = lr.finalize(S, Wsum, FU, p.center, p.scale, p.d, fused=fused)
        worst = lr.error_over_bound(got, N, D, P)
        assert worst <= 1.0, (fused, worst)
    # one unit in the lowest digit of one individual with g = 1 is 2^-FU off in N: outside the bound wherever c usum is small
    S1 = S.copy()
    S1[0, 0] += 1
    assert lr.error_over_bound(lr.finalize(S1, Wsum, FU, p.center, p.scale, p.d), N, D, P) > 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the fault models
FAULT_PANELS = [("rows", 641, 289, 22, "carries"), ("locus_major", 520, 289, 22, "carries"), ("locus_major", 264, 45, 6, "gauss"),
                ("rows", 129, 33, 1, "full"), ("locus_major", 128, 32, 5, "digits_min_max"), ("rows", 513, 129, 27, "gauss"),
                ("locus_major", 136, 130, 3, "gauss")]

# fault -> the reasons it gives on FAULT_PANELS, in order (None: it applies and must move a cell)
_ROWS = "rows layout: no pairs"
NOT_APPLICABLE = {
    "digit_unsigned": [None] * 7,
    # (a drawn u has its lowest digit at an edge once in 128 entries: the prescribed panels are there for these two)
    "carry_dropped_63_64": [None, None, None, "no lowest digit at the edge in the piece", None, None,
                            "no lowest digit at the edge in the piece"],
    "carry_dropped_m64_m65": [None, None, "no lowest digit at the edge in the piece", "no lowest digit at the edge in the piece", None,
                              None, "no lowest digit at the edge in the piece"],
    "digits_reversed": [None] * 7,
    "usum_unrounded": ["u lies on the fixed-point grid", "u lies on the fixed-point grid", None, "u lies on the fixed-point grid",
                       "u lies on the fixed-point grid", None, None],
    "ct0_lost": [None, None, "CT <= 4: one launch", "CT <= 4: one launch", "CT <= 4: one launch", None, "CT <= 4: one launch"],
    "straddle_read_from_one_tile": [None, None, None, "k <= 5: no component straddles two tiles",
                                    "k <= 5: no component straddles two tiles", None, "k <= 5: no component straddles two tiles"],
    "last_fragments_from_Qm2": [None, None, None, None, "Q = 1: one group", None, None],
    "slot_not_refilled": [None, None, "Q <= 4: no slot is used twice", "Q <= 4: no slot is used twice",
                          "Q <= 4: no slot is used twice", None, "Q <= 4: no slot is used twice"],
    "lm_clamped_chunk_added": [_ROWS, None, None, _ROWS, None, _ROWS, "Q even: no clamped half pair"],
    "lm_pair_swapped": [_ROWS, None, None, _ROWS, "Q = 1: the pair is one chunk twice", _ROWS, None],
    "lm_trade_first_dword_only": ["rows layout: no lane trade", None, None, "rows layout: no lane trade", None,
                                  "rows layout: no lane trade", None],
    "idle_wave_stored": [None, None, None, None, "one tile of loci: the idle waves' copy of tile 0 lands on padding alone",
                         "no idle wave: the tiles fill their workgroups", "no idle wave: the tiles fill their workgroups"],
}


def test_fault_list_is_the_table():
    assert [f.__name__ for f in lr.FAULTS] == list(NOT_APPLICABLE)
    assert sum(r is not None for rs in NOT_APPLICABLE.values() for r in rs) == N_NOT_APPLICABLE


# counted by hand from the table, fault by fault: 0 + 2 + 3 + 0 + 4 + 4 + 3 + 1 + 4 + 4 + 4 + 3 + 3 of the 13 * 7 pairs
N_NOT_APPLICABLE = 35


@pytest.mark.parametrize("fault", lr.FAULTS, ids=[f.__name__ for f in lr.FAULTS])
def test_every_fault_moves_a_cell_of_every_exact_panel_it_applies_to(fault):
    for case, reason in zip(FAULT_PANELS, NOT_APPLICABLE[fault.__name__]):
        p = _panel(case)
        lm = case[0] == "locus_major"
        if reason is not None:
            with pytest.raises(lr.NotApplicable) as e:
                fault(p, lm)
            assert str(e.value) == reason, case
            continue
        got = lr.faulty_loadings(fault, p, lm)  # (NotApplicable here = a pair the table does not list: an error)
        assert not np.array_equal(got, lr.exact_loadings(*p.args())), (fault.__name__, case, "the fault changes no cell")


# the slips the issue names as invisible today: one lane's piece, lowest digit
SMALL_TODAY = {"digit_unsigned", "carry_dropped_63_64", "carry_dropped_m64_m65"}


def test_small_faults_pass_the_tolerance_of_today():
    """tests/test_gpu_loadings.py asserts max |got - want| <= 1e-9 max |want| against FP64 Z'U / d at n = 130 and 136.  On such a
    panel every fault that moves the result by less than 2^-30 of its size passes that assertion -- and the faults of SMALL_TODAY
    are among them; each of them is outside the derived bound of the general tier"""
    p = lr.general_panel(136, 130, 22, seed=4)
    want = ((p.G.astype(float) - p.center) / p.scale).T @ p.U / p.d
    S, Wsum, FU = lr.quantised_sums(p.G, p.U)
    good = lr.finalize(S, Wsum, FU, p.center, p.scale, p.d)
    N, D, P = lr.rational_loadings(*p.args())
    assert np.abs(good - want).max() <= 1e-9 * np.abs(want).max()
    small = set()
    for fault in lr.FAULTS:
        for lm in (False, True):
            try:
                got = lr.faulty_loadings(fault, p, lm)
            except lr.NotApplicable:
                continue
            moved = np.abs(got - good).max()
            assert moved > 0, fault.__name__
            if moved < 2.0 ** -30 * np.abs(good).max():
                small.add(fault.__name__)
                assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), fault.__name__  # today: passes
                assert lr.error_over_bound(got, N, D, P) > 1.0, fault.__name__                 # the general tier: fails
    assert small >= SMALL_TODAY, small
