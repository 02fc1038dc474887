"""CPU-only: the restatement tests/sfs_ref.py has teeth, and the host side of include/tpg.h "site frequency spectra" -- the
projection row of csrc/host/host_sfs.h through tpg_sfs_project_row and through the sanitized stand-alone program, the split
rule, the scratch formula, folding and the summary statistics -- against it."""
import ctypes as C
from fractions import Fraction
from math import comb

import numpy as np
import pytest

from tests import sfs_ref as sr

SIZES = (1, 4, 5, 2)
_STATE = {}


def _tpg():
    import tidypopgen_amd as tpg

    return tpg


def _small():
    """a small panel with missing data and every table of the exact route, in Fractions proper"""
    if "small" not in _STATE:
        codes, gid, planted = sr.panel(11, SIZES, 90, miss=0.15, plant_v=(2, 4, 6, 2))
        G = len(SIZES)
        x, v = sr.group_tables(codes, gid, G)
        _STATE["small"] = dict(codes=codes, gid=gid, planted=planted, x=x, v=v, G=G)
    return _STATE["small"]


def _fraction_tables(x, v, n, t):
    """sfs and jsfs of the whole panel as sums of Fractions, straight from the definition"""
    m, G = x.shape
    o = sr.offsets(n)
    W = int(o[-1])
    rows = [[Fraction(0)] * W for _ in range(m)]
    for j in range(m):
        for g in range(G):
            if t[j, g]:
                rows[j][o[g]:o[g + 1]] = sr.exact_row(int(x[j, g]), int(v[j, g]), int(n[g]))
    sfs = [sum((rows[j][c] for j in range(m)), Fraction(0)) for c in range(W)]
    J = [[sum((rows[j][a] * rows[j][c] for j in range(m)), Fraction(0)) for c in range(W)] for a in range(W)]
    return sfs, J


def test_the_exact_row_is_the_share_of_subsets_for_every_small_case():
    for v in range(1, 9):
        for n in range(1, v + 1):
            for x in range(v + 1):
                assert sr.exact_row(x, v, n) == sr.brute_row(x, v, n), (x, v, n)


def test_projecting_the_spectrum_equals_projecting_the_loci():
    rng = np.random.default_rng(3)
    n = 12
    xs = rng.integers(0, n + 1, size=40)
    full = [Fraction(int((xs == k).sum())) for k in range(n + 1)]
    for n_to in (1, 2, 5, 11):
        direct = [sum((sr.exact_row(int(x), n, n_to)[k] for x in xs), Fraction(0)) for k in range(n_to + 1)]
        assert sr.project_spectrum(full, n_to) == direct
        assert sum(direct) == len(xs)


@pytest.mark.parametrize("proj", [(0, 0, 0, 0), (1, 5, 6, 3), (2, 4, 6, 2)])
def test_sums_margins_and_the_integer_route(proj):
    cs = _small()
    G, x, v = cs["G"], cs["x"], cs["v"]
    n = sr.proj_sizes(cs["gid"], G, proj)
    t = sr.usable(v, n)
    sfs, J = _fraction_tables(x, v, n, t)
    o = sr.offsets(n)
    m = len(x)
    n1, n2 = sr.n_used(t, [0], [m])
    # the integer route is the same rational numbers
    Hint, D = sr.weights_int(x, v, n, t)
    ex = sr.blocks_exact(Hint, D, [0], [m])
    W = int(o[-1])
    assert all(Fraction(int(ex["sfs_num"][c, 0]), int(D[c])) == sfs[c] for c in range(W))
    assert all(Fraction(int(ex["jsfs_num"][a, c, 0]), int(ex["jsfs_den"][a, c])) == J[a][c] for a in range(W) for c in range(W))
    for g in range(G):
        assert sum(sfs[o[g]:o[g + 1]]) == n1[g, 0]
    for g1 in range(G):
        for g2 in range(G):
            blk = [row[o[g2]:o[g2 + 1]] for row in J[o[g1]:o[g1 + 1]]]
            assert sum(sum(r) for r in blk) == n2[g1, g2, 0]
            # the margin over g2 is the spectrum of g1 over the loci usable in both
            both = t[:, g1] & t[:, g2]
            want = [sum((sr.exact_row(int(x[j, g1]), int(v[j, g1]), int(n[g1]))[k] for j in np.flatnonzero(both)), Fraction(0))
                    for k in range(int(n[g1]) + 1)]
            assert [sum(r) for r in blk] == want
    # flip of every locus mirrors every spectrum
    xf = sr.counted(x, v, np.ones(m, dtype=np.uint8))
    sfs_f, J_f = _fraction_tables(xf, v, n, t)
    for g in range(G):
        assert sfs_f[o[g]:o[g + 1]] == sfs[o[g]:o[g + 1]][::-1]
    a, b = 1, 2
    assert [r[o[b]:o[b + 1]] for r in J_f[o[a]:o[a + 1]]] == [r[o[b]:o[b + 1]][::-1] for r in J[o[a]:o[a + 1]][::-1]]
    assert n1.min() > 0 and (n2[0] > 0).all()
    if not any(proj):  # full size: every weight is 0 or 1 and the float route is the integer histogram
        fl = sr.blocks_float(sr.weights_float(x, v, n, t), [0], [m])
        assert np.array_equal(fl["sfs"][:, 0], np.array([float(s) for s in sfs]))
        assert np.array_equal(fl["jsfs"][:, :, 0], np.array([[float(c) for c in r] for r in J]))


def _sweep(seed=5, count=400, vmax=400):
    rng = np.random.default_rng(seed)
    q = [(0, 1, 1), (1, 1, 1), (0, 7, 3), (7, 7, 3), (3, 399, 399), (200, 399, 1)]
    for _ in range(count):
        v = int(rng.integers(1, vmax))
        q.append((int(rng.integers(0, v + 1)), v, int(rng.integers(1, v + 1))))
    return q


def _check_rows(rows, queries):
    worst = 0.0
    for h, (x, v, n) in zip(rows, queries):
        ex = sr.exact_row(x, v, n)
        assert len(h) == n + 1
        # the cap on skipped entries is zero: no exact entry of the sweep is below the range that has a relative bound
        assert all(e == 0 or e >= sr.TINY_ENTRY for e in ex)
        bound = Fraction(sr.entry_roundings(n), 2 ** 53)
        for k in range(n + 1):
            if ex[k] == 0:
                assert h[k] == 0.0 and not np.signbit(h[k]), (x, v, n, k)
            else:
                rel = abs(Fraction(float(h[k])) - ex[k]) / ex[k]
                assert rel <= bound, (x, v, n, k, float(rel / bound))
                worst = max(worst, float(rel / bound))
        if v == n:
            assert h[x] == 1.0 and np.count_nonzero(h) == 1
    return worst


def _check_large(h, x, v, n):
    assert np.isfinite(h).all() and (h >= 0).all()
    total = sum((Fraction(float(a)) for a in h), Fraction(0))
    # every entry within E(n) of the exact one, relatively, or (below 2^-1000) under 2^-999 absolutely; the exact ones sum to 1
    assert abs(total - 1) <= Fraction(sr.entry_roundings(n), 2 ** 53) + (n + 1) * Fraction(1, 2 ** 999)
    kmin, kmax = max(0, n - (v - x)), min(n, x)
    assert not h[:kmin].any() and not h[kmax + 1:].any()
    k0 = int(np.argmax(h))
    want = Fraction(comb(x, k0) * comb(v - x, n - k0), comb(v, n))
    assert abs(Fraction(float(h[k0])) - want) <= Fraction(sr.entry_roundings(n), 2 ** 53) * want


LARGE = [(4000, 10000, 6000), (1, 10000, 9999), (9999, 10000, 5000), (5000, 10000, 10000), (0, 10000, 777)]


def test_tpg_sfs_project_row_against_the_exact_route():
    tpg = _tpg()
    queries = _sweep()
    worst = _check_rows([tpg.sfs_project_row(*q) for q in queries], queries)
    print(f"worst relative error / ((9 n + 4) 2^-53) over {len(queries)} rows: {worst:.4f}")
    for x, v, n in LARGE:
        _check_large(tpg.sfs_project_row(x, v, n), x, v, n)
    lib = tpg._lib.lib
    h = np.zeros(4)
    for bad in ((-1, 4, 2), (5, 4, 2), (1, 4, 0), (1, 4, 5), (0, 0, 0), (1, 1 << 31, 2)):
        assert lib.tpg_sfs_project_row(*bad, C.c_void_p(h.ctypes.data)) == 1  # TPG_EINVAL
    assert lib.tpg_sfs_project_row(1, 4, 2, None) == 1
    assert not h.any()


def test_the_sanitized_host_program_gives_the_same_rows(tmp_path):
    tpg = _tpg()
    exe = sr.build_host_program(str(tmp_path / "sfs_san"))
    queries = _sweep(seed=6, count=150) + LARGE
    rows = sr.run_host_program(exe, tmp_path / "q.txt", queries)
    _check_rows(rows[:-len(LARGE)], queries[:-len(LARGE)])
    for h, q in zip(rows, queries):  # the library (hipcc's host compiler) and g++ run the same pinned order
        assert np.array_equal(h.view(np.uint64), tpg.sfs_project_row(*q).view(np.uint64)), q


def test_the_split_rule_and_the_scratch_formula():
    tpg = _tpg()
    seg = tpg.sfs_segments
    assert [seg(L, 5) for L in (0, 1, 1024, 1025, 2048, 2049)] == [1, 1, 1, 2, 2, 3]
    assert seg(63 * 1024, 5) == 63 and seg(63 * 1024 + 1, 5) == 64 and seg(10 ** 9, 5) == 64  # one tile: the cap is 64
    assert seg(10 ** 6, 603) == 18 and seg(10 ** 6, 1071) == 6  # 55 and 153 tiles for about 1024 workgroups
    assert seg(10 ** 6, 4096) == 1 and seg(5, 1) == -1 and seg(-1, 5) == -1 and seg(5, 4097) == -1
    assert tpg.SFS_CHUNK_LOCI == 64 and tpg.SFS_MAX_WIDTH == 4096
    sb = tpg.sfs_scratch_bytes
    assert sb(1000, 6, 172, 1) > 0 and sb(1000, 6, 11, 1) == -1 and sb(1000, 6, 4097, 1) == -1 and sb(-1, 6, 172, 1) == -1
    # bounded whatever m and nb are: the staged operand, the partial tiles, the tables
    for W in (2, 172, 603, 1071, 4096):
        big = sb(10 ** 9, 1, W, 16777215)
        assert big == sb(10 ** 8, 1, W, 1000000) and big < 200 << 20, (W, big)
    assert sb(1000, 6, 172, 1, joint=False) < sb(1000, 6, 172, 1)


def test_folding_and_statistics_against_their_restatement():
    tpg = _tpg()
    rng = np.random.default_rng(9)
    for n in (2, 3, 8, 13):
        s = rng.integers(0, 50, size=n + 1).astype(np.float64) / 4
        want = sr.fold1([Fraction(float(a)) for a in s])
        got = tpg.sfs_fold(s)
        assert [Fraction(float(a)) for a in got] == want and sum(want) == sum(Fraction(float(a)) for a in s)
        st, ex = tpg.sfs_stats(s), sr.stats([Fraction(float(a)) for a in s])
        assert Fraction(st["S"]) == ex["S"]  # quarters: every partial sum is exact
        for k in ("theta_pi", "theta_h"):
            assert abs(Fraction(st[k]) - ex[k]) <= Fraction(n + 4, 2 ** 53) * abs(ex[k])
        assert abs(st["fay_wu_h"] - float(ex["fay_wu_h"])) <= (2 * n + 10) * 2.0 ** -53 * float(ex["theta_pi"] + ex["theta_h"])
        assert abs(st["theta_w"] - float(ex["S"] / ex["a1"])) <= (n + 4) * 2.0 ** -53 * float(ex["S"] / ex["a1"])
    for n1, n2 in ((2, 2), (3, 4), (4, 6), (5, 5)):
        J = rng.integers(0, 40, size=(n1 + 1, n2 + 1)).astype(np.float64) / 2
        want = sr.fold2([[Fraction(float(c)) for c in r] for r in J])
        got = tpg.jsfs_fold(J)
        assert [[Fraction(float(c)) for c in r] for r in got] == want
        assert sum(sum(r) for r in want) == Fraction(float(J.sum()))
        assert not got[np.add.outer(np.arange(n1 + 1), np.arange(n2 + 1)) * 2 > n1 + n2].any()
    # Tajima's D of a spectrum against the Tajima section's own host entry point
    s = np.array([10.0, 7.0, 3.0, 2.0, 1.0, 0.0, 4.0])
    st = tpg.sfs_stats(s)
    assert st["tajimas_d"] == tpg.tajimas_d_from_sums(6, int(st["S"]), st["theta_pi"])
    with pytest.raises(ValueError):
        tpg.sfs_stats([1.0, 2.0])
    with pytest.raises(ValueError):
        tpg.sfs_fold([1.0])
