"""CPU-only: the host side of include/tpg.h "Mantel tests" -- tpg_mantel_perms against its restatement, the finishers
tpg_mantel_from_sums and tpg_mantel_partial against their float64 restatements and their Fraction routes, the ordered cross sum of
tests/mantel_ref.py against its exact route and against wrong sums (the reference has teeth), great_circle_dist on known arcs, and
csrc/host/host_mantel.h as a stand-alone program under the host sanitizers."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import mantel_ref as mr

R_VALUES = (0, 1, 2, 7, 2 ** 31 - 1)
STRATA = np.array([0, 2, 1, 1, 0, 2, 2, 1, 0, 0, 2, 1, 1, 1, 0, 2, 2, 0, 1, 3, 0, 2, 1], dtype=np.int32)  # stratum 3 holds one


def _tpg():
    import tidypopgen_amd as t

    return t


# ---- a. the permutation rule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stratified", [False, True])
@pytest.mark.parametrize("seed", [11, 2 ** 40 + 9])
def test_perms_equal_the_restatement(stratified, seed):
    tpg = _tpg()
    n = len(STRATA)
    st, k = (STRATA, 4) if stratified else (None, 0)
    rows = {}
    for r in R_VALUES:
        got = tpg.mantel_perms(n, seed, r, 1, st, k)
        assert got.shape == (1, n) and got.dtype == np.int32
        assert np.array_equal(got, mr.perms(n, seed, r, 1, st)), r
        assert sorted(got[0]) == list(range(n))  # a bijection
        if stratified:  # nobody leaves a stratum
            assert np.array_equal(STRATA[got[0]], STRATA)
        rows[r] = tuple(got[0])
    assert rows[0] == tuple(range(n))  # r = 0 is the identity
    assert len(set(rows.values())) == len(rows)
    assert tuple(tpg.mantel_perms(n, seed + 1, 1, 1, st, k)[0]) != rows[1]
    # one call for a batch: the rows do not depend on (r0, R)
    batch = tpg.mantel_perms(n, seed, 0, 9, st, k)
    assert np.array_equal(batch, mr.perms(n, seed, 0, 9, st))
    for r in (0, 1, 2, 7):
        assert tuple(batch[r]) == rows[r]
    assert np.array_equal(tpg.mantel_perms(n, seed, 5, 4, st, k), batch[5:9])
    assert np.array_equal(tpg.mantel_perms(n, seed, 2 ** 31 - 2, 2, st, k)[1], rows[2 ** 31 - 1])
    if stratified:  # ... and a stratified list differs from an unstratified one
        assert not np.array_equal(batch[1:], tpg.mantel_perms(n, seed, 1, 8))
    assert tpg.mantel_perms(n, seed, 3, 0, st, k).shape == (0, n)


def test_a_long_list_dealt_to_threads_equals_its_rows_one_by_one():
    tpg = _tpg()
    n, R = 2048, 64  # enough keys to sort for the library to deal the rows to several threads
    st = (np.arange(n) % 3).astype(np.int32)
    for strata, k in ((None, 0), (st, 3)):
        batch = tpg.mantel_perms(n, 77, 0, R, strata, k)
        for r in range(R):
            assert np.array_equal(tpg.mantel_perms(n, 77, r, 1, strata, k)[0], batch[r]), r
        assert np.array_equal(batch[[0, 1, 63]], np.concatenate([mr.perms(n, 77, 0, 2, strata), mr.perms(n, 77, 63, 1, strata)]))


def test_perms_refuse_bad_arguments():
    tpg = _tpg()
    n = len(STRATA)
    bad_hi, bad_lo = STRATA.copy(), STRATA.copy()
    bad_hi[3], bad_lo[5] = 4, -1
    for kw in (dict(r0=-1), dict(r0=2 ** 31), dict(r0=2 ** 31 - 1, R=2), dict(R=-1), dict(strata=bad_hi), dict(strata=bad_lo),
               dict(strata=STRATA, nstrata=0), dict(n=0, strata=None), dict(n=16385, strata=None)):
        a = dict(n=n, seed=5, r0=1, R=1, strata=STRATA, nstrata=4)
        a.update(kw)
        with pytest.raises(tpg._lib.TpgError) as e:
            tpg.mantel_perms(a["n"], a["seed"], a["r0"], a["R"], a["strata"], a["nstrata"])
        assert e.value.code == 1, kw
    assert tpg.mantel_perms(16384, 5, 1, 1).shape == (1, 16384)


# ---- b. the finishers ------------------------------------------------------------------------------------------------------------
def test_from_sums_and_partial_equal_the_restatement_bit_for_bit():
    tpg = _tpg()
    rng = np.random.default_rng(3)
    for _ in range(200):
        N = int(rng.integers(2, 10 ** 6))
        a, b = rng.normal(size=40) * 7 + rng.normal() * 30, rng.normal(size=40) * 3 + rng.normal() * 100
        args = (N, a.sum(), (a * a).sum(), b.sum(), (b * b).sum(), (a * b).sum())
        assert mr.same_values(tpg.mantel_from_sums(*args), mr.from_sums(*args))
        rs = rng.uniform(-1, 1, size=3)
        assert mr.same_values(tpg.mantel_partial(*rs), mr.partial(*rs))


def test_the_finishers_agree_with_the_fraction_route_on_integer_inputs():
    tpg = _tpg()
    rng = np.random.default_rng(4)
    for _ in range(50):
        k = int(rng.integers(5, 60))
        a, b = rng.integers(-50, 51, size=k), rng.integers(-50, 51, size=k)
        args = (k, int(a.sum()), int((a * a).sum()), int(b.sum()), int((b * b).sum()), int((a * b).sum()))
        cov, vv = mr.from_sums_exact(*args)
        if vv <= 0:
            continue
        want = math.copysign(math.sqrt(cov * cov / vv), cov)
        assert abs(tpg.mantel_from_sums(*args) - want) <= 1e-12
        assert abs(tpg.mantel_from_sums(*args) - np.corrcoef(a, b)[0, 1]) <= 1e-12  # ... which is Pearson's r
        rs = [Fraction(int(x), 64) for x in rng.integers(-60, 61, size=3)]
        num, under = mr.partial_exact(*rs)
        got = tpg.mantel_partial(*[float(x) for x in rs])
        assert abs(got - float(num) / math.sqrt(under)) <= 1e-12


def test_the_finishers_give_nan_at_every_degenerate_case():
    tpg = _tpg()
    f = tpg.mantel_from_sums
    assert np.isnan(f(0, 0.0, 0.0, 0.0, 0.0, 0.0)) and np.isnan(f(-3, 1.0, 2.0, 1.0, 2.0, 1.0))  # N < 1
    assert np.isnan(f(4, 8.0, 16.0, 1.0, 9.0, 3.0))  # a constant: its variance term is zero
    assert np.isnan(f(4, 1.0, 9.0, 8.0, 16.0, 3.0))  # b constant
    assert np.isnan(f(4, 8.0, 15.0, 1.0, 9.0, 3.0))  # a negative variance term
    assert np.isnan(f(4, np.nan, 9.0, 1.0, 9.0, 3.0)) and np.isnan(f(4, 1.0, 9.0, 1.0, 9.0, np.nan))
    assert f(4, 0.0, 4.0, 0.0, 4.0, 4.0) == 1.0 and f(4, 0.0, 4.0, 0.0, 4.0, -4.0) == -1.0
    p = tpg.mantel_partial
    assert np.isnan(p(0.3, 1.0, 0.2)) and np.isnan(p(0.3, 0.2, -1.0)) and np.isnan(p(0.3, 1.5, 0.2)) and np.isnan(p(0.3, np.nan, 0.2))
    assert np.isnan(p(np.nan, 0.1, 0.2)) and p(0.5, 0.0, 0.0) == 0.5
    for args in ((0, 0.0, 0.0, 0.0, 0.0, 0.0), (4, 8.0, 16.0, 1.0, 9.0, 3.0), (4, 8.0, 15.0, 1.0, 9.0, 3.0)):
        assert np.isnan(mr.from_sums(*args))


# ---- c. the ordered sum: its bound, and its teeth ----------------------------------------------------------------------------------
def test_the_ordered_sum_lies_within_its_bound_of_the_exact_sum():
    L = mr.lanes()
    assert L in (256, 512, 1024)
    n = 67
    P = mr.perm_rows(5, n, 3)
    for kind in ("int", "real"):
        A, B = mr.matrix(kind, n, 32), mr.matrix(kind, n, 33)
        for small_L in (L, 16):  # (n < L: one stride; L = 16: five strides, the last one ragged)
            got = mr.ordered_sums(A, [B], P, small_L)
            for r in range(3):
                (s, ab, k), raw = mr.exact_sums(A, B, P[r])
                if kind == "int":
                    assert Fraction(float(got[r, 0])) == s == raw == mr.int_sums(A, B, P[r])
                else:
                    assert abs(Fraction(float(got[r, 0])) - s) <= Fraction(k, 2 ** 52) * ab, (r, small_L)


def test_the_reference_has_teeth():
    L = mr.lanes()
    n = 2 * L + 3  # a panel of the GPU test: three strides, the last one ragged
    P = mr.perm_rows(7 * n, n, 4)
    for kind in ("real", "int"):
        A, B = mr.matrix(kind, n, 1000 + n), mr.matrix(kind, n, 2000 + n)
        right = mr.ordered_sums(A, [B], P, L)
        for fault in mr.FAULTS:
            # On the integer panel every order gives the exact integer (|a b| <= 2^20, n^2 terms: far below 2^53), as the header
            # says, and a fused product rounds nothing: the four order faults and the fusion cannot show there.  The index faults
            # must, and do, because the matrices are not symmetric.
            if kind == "int" and fault in ("tree_ascending", "contiguous_partials", "fused_product", "columns_descending"):
                continue
            rows = P[2:3] if fault == "fused_product" else P  # (an exact emulation in Fractions: one random permutation)
            wrong = mr.ordered_sums(A, [B], rows, L, fault=fault)
            want = right[2:3] if fault == "fused_product" else right
            if fault == "inverse_perm":  # the identity and the reversal are their own inverses: the random rows must differ
                assert mr.same_values(wrong[:2], want[:2]) and not (wrong[2:] == want[2:]).any(), kind
            elif fault == "rows_only":  # (the identity permutes nothing)
                assert mr.same_values(wrong[:1], want[:1]) and not (wrong[1:] == want[1:]).any(), kind
            elif fault in ("swap_ij", "with_diagonal", "skip_ragged_stride"):  # an index fault changes every row
                assert not (wrong == want).any(), (kind, fault)
            else:  # an order fault changes last bits: of the panel's sums, not of each one
                assert not mr.same_values(wrong, want), (kind, fault)
        if kind == "real":  # another L: other bits
            assert not mr.same_values(mr.ordered_sums(A, [B], P, L // 2), right)
    # NaN: on a diagonal nothing changes; off the diagonal of B the sum is NaN
    A, B = mr.matrix("real", 40, 1), mr.matrix("real", 40, 2)
    P = mr.perm_rows(3, 40, 3)
    right = mr.ordered_sums(A, [B], P, L)
    A2, B2 = A.copy(), B.copy()
    A2[5, 5] = B2[9, 9] = np.nan
    assert mr.same_bits(mr.ordered_sums(A2, [B2], P, L), right)
    B2[3, 4] = np.nan
    assert np.isnan(mr.ordered_sums(A2, [B, B2], P, L)[:, 1]).all() and mr.same_bits(mr.ordered_sums(A2, [B, B2], P, L)[:, 0], right[:, 0])


def test_the_scratch_is_bounded_independently_of_R():
    tpg = _tpg()
    a, b = tpg.mantel_scratch_bytes(5000, 10 ** 4, 2), tpg.mantel_scratch_bytes(5000, 10 ** 9, 2)
    assert 0 < a == b < 1 << 28
    assert 0 < tpg.mantel_scratch_bytes(5000, 1, 2) < a
    assert 0 < tpg.mantel_scratch_bytes(16384, 10 ** 9, 4) < 1 << 28
    for bad in ((0, 1, 1), (16385, 1, 1), (10, -1, 1), (10, 1, 0), (10, 1, 5)):
        assert tpg.mantel_scratch_bytes(*bad) == -1, bad


# ---- d. great-circle distances -----------------------------------------------------------------------------------------------------
def test_great_circle_dist_on_known_arcs():
    tpg = _tpg()
    R = 6371.0088
    lon, lat = [0.0, 90.0, 0.0, 0.0, 13.4, -70.7], [0.0, 0.0, 90.0, -90.0, 52.5, -33.4]
    d = tpg.great_circle_dist(lon, lat)
    assert d.shape == (6, 6) and np.array_equal(d, d.T) and (np.diag(d) == 0).all() and (d[~np.eye(6, dtype=bool)] > 0).all()
    assert abs(d[0, 1] - math.pi * R / 2) <= 1e-12 * math.pi * R / 2  # a quarter of the equator
    assert abs(d[2, 3] - math.pi * R) <= 1e-12 * math.pi * R  # pole to pole
    assert abs(d[0, 2] - math.pi * R / 2) <= 1e-12 * math.pi * R
    assert abs(tpg.great_circle_dist(lon, lat, radius_km=1.0)[2, 3] - math.pi) <= 1e-12 * math.pi
    # the spherical law of cosines agrees where it is well conditioned (Berlin - Santiago de Chile)
    la, lb, dl = math.radians(52.5), math.radians(-33.4), math.radians(13.4 + 70.7)
    want = R * math.acos(math.sin(la) * math.sin(lb) + math.cos(la) * math.cos(lb) * math.cos(dl))
    assert abs(d[4, 5] - want) <= 1e-9 * want


def test_midranks_equal_the_restatement():
    tpg = _tpg()
    rng = np.random.default_rng(6)
    M = rng.integers(0, 9, size=(13, 13)).astype(float)  # many ties
    M = M + M.T
    got = tpg.offdiag_midranks(M)
    assert np.array_equal(got, mr.midranks(M)) and np.array_equal(got, got.T) and (np.diag(got) == 0).all()
    off = got[np.tril_indices(13, -1)]
    assert off.sum() == 78 * 79 / 2  # mid-ranks keep the sum of 1 .. 78
    with pytest.raises(ValueError):
        tpg.offdiag_midranks(rng.normal(size=(5, 5)))


# ---- e. the host pieces under the sanitizers ---------------------------------------------------------------------------------------
def test_the_sanitized_host_program(tmp_path):
    exe = mr.build_host_program(str(tmp_path / "mantel_san"))
    tpg = _tpg()
    rng = np.random.default_rng(8)
    n = len(STRATA)
    queries, want = [], []
    for has in (0, 1):
        for r0, R in ((0, 3), (7, 2), (2 ** 31 - 1, 1), (4, 0)):
            queries.append([1, n, 4, 2 ** 40 + 9, r0, R, has, *(STRATA if has else [])])
            want.append([0, *mr.perms(n, 2 ** 40 + 9, r0, R, STRATA if has else None).ravel()])
    queries.append([1, 2048, 0, 9, 0, 64, 0])  # a list long enough for the threads
    want.append([0, *np.concatenate([tpg.mantel_perms(2048, 9, r, 1)[0] for r in range(64)])])
    bad_st = STRATA.copy()
    bad_st[2] = 4
    for bad in ([1, n, 4, 5, -1, 1, 0], [1, n, 4, 5, 2 ** 31, 1, 0], [1, n, 4, 5, 2 ** 31 - 1, 2, 0], [1, n, 4, 5, 1, -1, 0], [1, 0, 4, 5, 1, 1, 0],
                [1, 16385, 4, 5, 1, 1, 0], [1, n, 4, 5, 1, 2, 1, *bad_st], [1, n, 0, 5, 1, 2, 1, *STRATA]):
        queries.append(bad)
        want.append([1])
    fin = []
    for _ in range(10):
        a, b = rng.normal(size=30) + 5, rng.normal(size=30) * 2 - 1
        fin.append((30, a.sum(), (a * a).sum(), b.sum(), (b * b).sum(), (a * b).sum()))
    fin += [(0, 0.0, 0.0, 0.0, 0.0, 0.0), (4, 8.0, 16.0, 1.0, 9.0, 3.0), (4, 8.0, 15.0, 1.0, 9.0, 3.0)]
    for args in fin:
        queries.append([2, args[0], *[mr.bits(x) for x in args[1:]]])
        want.append([mr.bits(mr.from_sums(*args))])
    for rs in [tuple(rng.uniform(-1, 1, size=3)) for _ in range(10)] + [(0.3, 1.0, 0.2), (0.3, 0.2, 1.5)]:
        queries.append([3, *[mr.bits(x) for x in rs]])
        want.append([mr.bits(mr.partial(*rs))])
    for nn, R in ((1, 1), (7, 3), (40, 2)):
        P = mr.perm_rows(nn, nn, R) if nn > 1 else np.zeros((1, 1), dtype=np.int32)
        queries.append([4, nn, 2, R, *P.ravel()])
        want.append([0, *np.stack([np.argsort(p) for p in P]).ravel()])
    queries.append([4, 5, 1, 0])  # R = 0 is fine
    want.append([0])
    for bad in ([4, 4, 1, 1, 0, 1, 1, 3], [4, 4, 1, 1, 0, 1, 2, 4], [4, 4, 1, 1, 0, -1, 2, 3], [4, 4, 0, 1, 0, 1, 2, 3], [4, 4, 5, 1, 0, 1, 2, 3],
                [4, 4, 1, -1], [4, 0, 1, 0], [4, 16385, 1, 0]):
        queries.append(bad)
        want.append([1])
    for args in ((5000, 10 ** 9, 2), (16384, 40, 4), (1, 0, 1), (0, 1, 1), (10, 1, 5)):
        queries.append([5, *args])
        want.append([tpg.mantel_scratch_bytes(*args)])
    got = mr.run_host_program(exe, tmp_path / "q.txt", queries)
    for q, g, w in zip(queries, got, want):
        if q[0] in (2, 3):  # doubles: NaN payloads aside
            assert mr.same_values(mr.from_bits(g[0]), mr.from_bits(w[0])), q
        else:
            assert g == [int(x) for x in w], q[:8]
