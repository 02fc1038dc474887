"""CPU-only: the host side of include/tpg.h "Fst under relabelings" -- tpg_fst_perm_labels against its restatement, the p-value on
hand-made vectors, the ordered sum of tests/fstperm_ref.py against its exact route and against wrong orders (the reference has
teeth), and csrc/host/host_fstperm.h as a stand-alone program under the host sanitizers."""
from fractions import Fraction

import numpy as np
import pytest

from tests import fstperm_ref as fr


def _tpg():
    import tidypopgen_amd as t

    return t


def _gid(seed, n, G):
    return np.random.default_rng(seed).integers(0, G, size=n).astype(np.int32)


CASES = [(0, 37, 4, 1, 3, 11), (0, 130, 6, 5, 0, 2 ** 40 + 9), (1, 37, 4, 0, 0, 11), (1, 130, 7, 0, 0, 0)]


@pytest.mark.parametrize("scheme,n,G,a,b,seed", CASES)
def test_perm_labels_equal_the_restatement(scheme, n, G, a, b, seed):
    tpg = _tpg()
    gid = _gid(n + G, n, G)
    ident = np.where(gid == a, 0, np.where(gid == b, 1, -1)) if scheme == 0 else gid
    rows = {}
    for r in (0, 1, 2, 7, 2 ** 31 - 1):
        got = tpg.fst_perm_labels(n, gid, G, scheme, a, b, seed, r)
        assert np.array_equal(got, fr.perm_labels(n, gid, G, scheme, a, b, seed, r)), r
        # the group sizes are preserved, and whoever is outside stays outside
        assert np.array_equal(np.bincount(got[got >= 0], minlength=G), np.bincount(ident[ident >= 0], minlength=G))
        assert np.array_equal(got < 0, ident < 0)
        rows[r] = got
    assert np.array_equal(rows[0], ident)  # r = 0 is the identity
    assert len({tuple(v) for v in rows.values()}) == len(rows)  # distinct r: distinct rows
    other = tpg.fst_perm_labels(n, gid, G, scheme, a, b, seed + 1, 1)
    assert not np.array_equal(other, rows[1])  # another seed: another row
    assert np.array_equal(tpg.fst_perm_labels(n, gid, G, "pairwise" if scheme == 0 else "global", a, b, seed, 7), rows[7])


def test_perm_labels_refuse_bad_arguments():
    tpg = _tpg()
    gid = _gid(1, 20, 3)
    for kw in (dict(scheme=2), dict(a=1, b=1), dict(a=3), dict(b=-1), dict(r=-1), dict(r=2 ** 31)):
        args = dict(scheme=0, a=0, b=1, r=1)
        args.update(kw)
        with pytest.raises(tpg._lib.TpgError) as e:
            tpg.fst_perm_labels(20, gid, 3, args["scheme"], args["a"], args["b"], 5, args["r"])
        assert e.value.code == 1, kw
    bad = gid.copy()
    bad[4] = 3
    with pytest.raises(tpg._lib.TpgError):
        tpg.fst_perm_labels(20, bad, 3, 1, 0, 0, 5, 1)


def test_pvalue_on_hand_made_vectors():
    tpg = _tpg()
    nan, inf = float("nan"), float("inf")
    obs = np.array([0.5, 0.5, 0.5, nan, inf, 0.1])
    perm = np.array([[0.1, 0.5, nan, 0.1, 0.1, 0.1],
                     [0.6, 0.5, nan, 0.2, 0.2, nan],
                     [0.5, 0.4, nan, 0.3, inf, -inf],
                     [0.2, nan, nan, 0.4, 0.4, 0.1]])
    p, nv = tpg.fst_perm_pvalue(obs, perm)
    # column 0: 0.6 and the tie 0.5 count -> 3 / 5; column 1: two ties of three finite -> 3 / 4; column 2: no finite value -> 1 / 1;
    # columns 3, 4: the observed value is not finite -> NaN; column 5: the ties 0.1, 0.1 of two finite (-inf, NaN are not) -> 3 / 3
    assert np.array_equal(nv, [4, 3, 0, 4, 3, 2])
    assert np.array_equal(p[[0, 1, 2, 5]], [3 / 5, 3 / 4, 1.0, 1.0])
    assert np.isnan(p[3]) and np.isnan(p[4])
    for k in range(6):
        pk, nk = fr.pvalue(obs[k], perm[:, k])
        assert nk == nv[k] and (pk == p[k] or (np.isnan(pk) and np.isnan(p[k])))


@pytest.fixture(scope="module")
def crafted():
    """130 x 1037 with a tenth missing, three groups with some individuals outside; terms by the oracle for all three methods"""
    U, S = fr.unit_span()
    codes = fr.panel(21, 130, 2 * S + U + 5)
    lab = fr.label_rows(22, 130, 3, 2)[1]
    codes[lab == 0, 77] = fr.MISSING  # a locus no pair with group 0 keeps
    return {meth: fr.terms(codes, lab, 3, meth) for meth in ("Hudson", "WC84", "Nei87")}, U, S


def test_the_ordered_sum_lies_within_its_bound_of_the_exact_sum(crafted):
    tabs, U, S = crafted
    for meth, (num, den) in tabs.items():
        m = num.shape[0]
        sn, sd, nk = fr.ordered_sums(num, den, U, S)
        en, an, ed, ad = fr.exact_sums(num, den)
        assert list(nk) == [m - 1, m - 1, m]  # the planted locus is dropped by the two pairs of group 0, by nobody else
        for k in range(num.shape[1]):
            assert abs(Fraction(float(sn[k])) - en[k]) <= Fraction(m, 2 ** 52) * an[k], (meth, k)
            assert abs(Fraction(float(sd[k])) - ed[k]) <= Fraction(m, 2 ** 52) * ad[k], (meth, k)


def test_the_reference_has_teeth(crafted):
    tabs, U, S = crafted
    num, den = tabs["Hudson"]
    sn, sd, nk = fr.ordered_sums(num, den, U, S)
    # another unit size, another span: other bits (1037 terms of mixed magnitude: some pair's rounding differs)
    for u2, s2 in ((U * 2 if U < 32 else U // 2, S), (U, S * 2), (1, S)):
        wn, wd, _ = fr.ordered_sums(num, den, u2, s2)
        assert not (np.array_equal(wn, sn) and np.array_equal(wd, sd)), (u2, s2)
    # a table of terms in which one locus has a numerator and no denominator (no diploid panel gives one: the three methods'
    # num and den are NaN together; the rule is stated for both all the same): deciding on num alone adds that numerator
    den2 = den.copy()
    den2[5, :] = np.nan
    a = fr.ordered_sums(num, den2, U, S)
    b = fr.ordered_sums(num, den2, U, S, keep_on_num_alone=True)
    assert np.array_equal(a[2], nk - 1) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], b[0])


def test_the_scratch_is_bounded_independently_of_R():
    lib = _tpg()._lib.lib
    U, S = fr.unit_span()
    assert 32 % U == 0 and S % 128 == 0
    # host only: the bound has no R in it; at 5 000 x 10^6 it stays below 1 GiB for the pairwise scheme and for ten groups
    assert 0 < lib.tpg_fst_relabel_scratch_bytes(5000, 10 ** 6, 2, 1) < 1 << 30
    assert 0 < lib.tpg_fst_relabel_scratch_bytes(5000, 10 ** 6, 10, 45) < 1 << 30
    for bad in ((0, 10, 2, 1), (1 << 24, 10, 2, 1), (10, -1, 2, 1), (10, 10, 1, 1), (10, 10, 65, 1), (10, 10, 2, 0)):
        assert lib.tpg_fst_relabel_scratch_bytes(*bad) == -1, bad


def test_the_sanitized_host_program(tmp_path):
    exe = fr.build_host_program(str(tmp_path / "fstperm_san"))
    rng = np.random.default_rng(8)
    queries, want = [], []
    # the label generator, both schemes, and its refusals
    for scheme, n, G, a, b, seed in CASES:
        gid = _gid(n, n, G)
        for r in (0, 1, 9):
            queries.append([1, n, G, scheme, a, b, seed, r, *gid])
            want.append([0, *fr.perm_labels(n, gid, G, scheme, a, b, seed, r)])
    gid = _gid(3, 9, 3)
    gid[0] = 2  # (out of range when the query says two groups)
    for bad in ([1, 9, 3, 0, 1, 1, 5, 1, *gid], [1, 9, 3, 2, 0, 1, 5, 1, *gid], [1, 9, 3, 1, 0, 0, 5, -1, *gid],
                [1, 9, 2, 1, 0, 0, 5, 1, *gid], [1, 0, 2, 1, 0, 0, 5, 1]):
        queries.append(bad)
        want.append([1] if bad[1] else [0])
    # the class packing: slots that do not fill a tile (3, 5, 33), that do (2, 32), one relabeling per tile (64)
    for G, rows in ((2, 33), (3, 22), (5, 13), (32, 3), (33, 2), (64, 2)):
        n = 17
        lab = rng.integers(-1, G, size=(rows, n))
        slots = 64 // G
        cs = np.zeros(-(-rows // slots) * 64, dtype=np.int64)
        for b in range(rows):
            for l in lab[b][lab[b] >= 0]:
                cs[(b // slots) * 64 + (b % slots) * G + l] += 1
        queries.append([2, n, G, rows, *lab.ravel()])
        want.append([*cs, *lab.ravel()])
    # the argument checks: fine, then every refusal of "Limits and errors"
    n, lab = 6, [0, 1, -1, 2, 1, 0]
    ok = [3, n, 3, 1, 2, 1, 2, 3, 1, *lab]
    queries.append(ok)
    want.append([0])
    queries.append([3, n, 3, 0, 1, 1, 2])  # R = 0 is fine
    want.append([0])
    for bad in ([3, n, 3, 1, 1, 1, 2, 0, 1, -2, 2, 1, 0], [3, n, 3, 1, 1, 1, 2, 0, 1, 3, 2, 1, 0], [3, n, 3, 1, 1, 0, 2, *lab],
                [3, n, 3, 1, 1, 1, 4, *lab], [3, n, 3, 1, 1, 2, 2, *lab], [3, n, 3, 1, 0, *lab], [3, n, 3, -1, 1, 1, 2],
                [3, n, 65, 1, 1, 1, 2, *lab], [3, n, 1, 1, 1, 1, 2, *lab]):
        queries.append(bad)
        want.append([1])
    got = fr.run_host_program(exe, tmp_path / "q.txt", queries)
    for q, g, w in zip(queries, got, want):
        assert g == [int(x) for x in w], q[:8]
