"""CPU: include/tpg.h "LD statistics" restated in numpy (tests/ldstat_ref.py) against an exact route in Fractions and against
numpy's correlation; the identities that tie the per-locus sums to the bins; the comparison the GPU tests make has teeth; the
statistic behaves on panels with and without LD; and the routines the kernel's epilogue calls (csrc/host/host_ldstat.h) as a
stand-alone program under the host sanitizers against the restatement."""
import shutil

import numpy as np
import pytest

from tests import ld_ref
from tests import ldstat_ref as sr
from tests.knn_impute_ref import window


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    return sr.build_host_program(str(tmp_path_factory.mktemp("ldstat") / "ldstat_san"), sanitize=True)


def _small_panels():
    """(G, hi): small panels with LD, monomorphic loci among them, whole-panel and narrow windows, two chromosomes"""
    out = []
    for seed, n, m, rho in ((1, 7, 30, 0.5), (2, 40, 60, 0.8), (3, 65, 45, 0.0), (4, 130, 40, 0.9), (5, 3, 25, 0.5), (6, 2, 20, 0.5)):
        G = np.array(ld_ref.ld_panel(seed, n, m, rho))
        G[:, 0] = 0
        G[:, m // 2] = 2
        out.append((G, window(m, m)))
        out.append((G, window(m, 7, chrom_ends=[m // 3, m])))
    return out


def test_q_of_the_float_route_is_q_of_the_exact_route():
    pairs = skipped = 0
    for G, hi in _small_panels():
        for (j, ks, r2), (je, kse, ex) in zip(sr.rows(G, hi), sr.exact_rows(G, hi)):
            assert j == je and list(ks) == kse
            q = sr.q_of(r2[~np.isnan(r2)])
            assert [e is None for e in ex] == list(np.isnan(r2))  # the same pairs are valid
            at = 0
            for e in ex:
                if e is None:
                    continue
                want, off_half = sr.exact_q(e)
                pairs += 1
                if off_half < 2.0 ** -20:  # the float route may round r2 2^30 + 0.5 across the integer
                    skipped += 1
                else:
                    assert int(q[at]) == want, (j, at, float(e))
                at += 1
    print(f"{pairs} pairs, {skipped} within 2^-20 of a half-integer")
    assert pairs > 3000 and skipped * 1000 <= pairs


def test_r2_is_the_squared_correlation():
    G = np.array(ld_ref.ld_panel(7, 400, 120, 0.7))
    G[:, 5] = 1
    hi = window(120, 120)
    corr = np.corrcoef(G[:, np.r_[0:5, 6:120]].astype(np.float64), rowvar=False) ** 2
    keep = np.r_[0:5, 6:120]
    worst = 0.0
    for j, ks, r2 in sr.rows(G, hi):
        if j == 5:
            assert np.isnan(r2).all()
            continue
        assert np.isnan(r2[ks == 5]).all() and not np.isnan(r2[ks != 5]).any()
        a = np.searchsorted(keep, j)
        b = np.searchsorted(keep, ks[ks != 5])
        worst = max(worst, float(np.abs(r2[ks != 5] - corr[a, b]).max(initial=0.0)))
    print(f"largest |r2 - corrcoef^2| = {worst:.3g}")
    assert worst <= 1e-10


def test_bins_and_scores_add_up():
    rng = np.random.default_rng(11)
    beyond = set()
    for G, hi in _small_panels():
        m = G.shape[1]
        pos = np.cumsum(rng.integers(0, 4, size=m))  # ties among them
        for bin_size, nbins in ((1, 4096), (3, 5), (1000, 1)):
            s = sr.stats(G, hi, pos, bin_size, nbins)
            rep = s["report"]
            assert int(s["bin_pairs"].sum()) + rep["pairs_beyond"] == int(s["n_partners"].sum()) // 2 == rep["pairs_valid"]
            assert int(s["n_partners"].sum()) % 2 == 0 and rep["pairs_valid"] <= rep["pairs"]
            if rep["pairs_beyond"] == 0:
                assert int(s["bin_sum_q"].sum()) * 2 == int(s["score_q"].sum())
            else:
                assert int(s["bin_sum_q"].sum()) * 2 <= int(s["score_q"].sum())
            beyond.add(rep["pairs_beyond"] > 0)
        t = sr.stats(G, hi)  # without bins: the same scores
        assert np.array_equal(t["score_q"], s["score_q"]) and np.array_equal(t["n_partners"], s["n_partners"])
        assert "bin_pairs" not in t
    assert beyond == {False, True}


def test_region_matrix_and_band_agree():
    G, _ = _small_panels()[2]
    m = G.shape[1]
    R = sr.region_r2(G, 3, m - 2)
    assert np.array_equal(np.isnan(R), np.isnan(R.T)) and np.allclose(np.nan_to_num(R), np.nan_to_num(R.T), rtol=0, atol=0)
    band = sr.band_r2(G, window(m, m), 3, m - 2)
    for j in range(3, m - 2):
        assert sr.same_bits(R[j - 3, j - 3 + 1:], band[j - 3, :m - 3 - j])  # (the band runs on to the loci behind the region)
    mono = m // 2 - 3
    assert np.isnan(R[mono]).all() and np.isnan(R[:, mono]).all()
    ok = np.delete(np.arange(R.shape[0]), mono)
    assert (np.diag(R)[ok] == 1.0).all()


def test_the_comparison_has_teeth():
    G, hi = _small_panels()[2]
    m = G.shape[1]
    band = sr.band_r2(G, hi, 0, m)
    assert sr.same_bits(band, band.copy())
    j, b = np.argwhere(~np.isnan(band) & (band > 0))[7]
    for other in (np.nextafter(band[j, b], 2.0), np.nextafter(band[j, b], -1.0), np.nan):  # one ulp either way; a pair made invalid
        off = band.copy()
        off[j, b] = other
        assert not sr.same_bits(band, off)
    pos = np.arange(m) * 2
    s = sr.stats(G, hi, pos, 2, 64)
    assert sr.equal_stats(s, sr.stats(G, hi, pos, 2, 64))
    for jj in (1, m - 2):  # one pair dropped at the edge of a window: the last neighbour of a locus
        cut = hi.copy()
        cut[:jj + 1] = np.minimum(cut[:jj + 1], max(hi[jj] - 1, jj))
        assert (hi - cut).sum() >= 1
        t = sr.stats(G, cut, pos, 2, 64)
        assert not sr.equal_stats(s, t)
        assert not np.array_equal(s["n_partners"], t["n_partners"]) and not np.array_equal(s["bin_pairs"], t["bin_pairs"])
    t = sr.stats(G, hi, pos, 2, 64)
    t["score_q"] = t["score_q"].copy()
    t["score_q"][4] += np.uint64(1)  # one q off by the last bit
    assert not sr.equal_stats(s, t)


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_the_decay_curve_decays_and_the_adjustment_removes_the_bias(seed):
    """ld_panel(seed, 400, 1500, rho).  At rho = 0.9 the mean r2 at lags 1 .. 8 falls strictly, from above 0.75 to below 0.25
    (observed 0.809 .. 0.185 to 0.811 .. 0.190).  At rho = 0 and a window of 50 the mean r2 per partner is 1 / (n - 1) up to
    2e-4 (observed within 1.4e-5), and its adjusted form 0 up to 1e-4 (observed at most 1.4e-5)."""
    n, m = 400, 1500
    G = ld_ref.ld_panel(seed, n, m, 0.9)
    d = sr.decay(G, window(m, 8), None, 1, 9)
    lag = d["mean_r2"][1:9]
    print(f"seed {seed}, rho 0.9: mean r2 at lags 1 .. 8 = {np.round(lag, 4)}")
    assert d["n_pairs"][0] == 0 and np.isnan(d["mean_r2"][0]) and d["pairs_beyond"] == 0
    assert (np.diff(lag) < 0).all() and lag[0] > 0.75 and lag[7] < 0.25
    G = ld_ref.ld_panel(seed, n, m, 0.0)
    s = sr.stats(G, window(m, 50))
    S, c = float(s["score_q"].sum()) / sr.Q_ONE, float(s["n_partners"].sum())
    raw = S / c
    adj = raw - (1.0 - raw) / (n - 2)
    print(f"seed {seed}, rho 0: mean r2 per partner {raw:.6f} (1 / (n - 1) = {1 / (n - 1):.6f}), adjusted {adj:.2e}")
    assert abs(adj) < 1e-4
    assert abs(raw - 1.0 / (n - 1)) < 2e-4
    score = sr.ld_score(G, window(m, 50))
    assert abs(float(np.nanmean(score)) - 1.0) < 0.02  # the adjusted score of independent loci is its self term


def test_r2_and_q_of_the_host_routines_under_sanitizers(exe, tmp_path):
    lines, want = [], []
    for G, hi in _small_panels():
        n, sx, d = ld_ref.sums(G)
        g = G.astype(np.int64)
        for j, ks, r2 in sr.rows(G, hi):
            ok = ~np.isnan(r2)
            sxy = g[:, j] @ g[:, ks[ok]]
            for k, s, r in zip(ks[ok], sxy, r2[ok]):
                lines.append(f"R {n} {s} {sx[j]} {sx[k]} {d[j]} {d[k]}")
                want.append([int(np.float64(r).view(np.uint64)), int(sr.q_of(r))])
    # the ends of the range: the largest n the band takes (r2 = 1 of a locus with itself, and a small r2), and r2 = 0
    big = (1 << 22) - 1
    a = np.zeros(big, dtype=np.int64)
    a[:big // 2] = 2
    b = np.arange(big, dtype=np.int64) % 3
    ends = [(a, a), (a, b), (b, b), (np.array([0, 0, 2, 2]), np.array([0, 2, 0, 2]))]
    for x, y in ends:
        n = len(x)
        sxj, sxk, sxy = int(x.sum()), int(y.sum()), int(x @ y)
        dj, dk = n * int((x * x).sum()) - sxj * sxj, n * int((y * y).sum()) - sxk * sxk
        dn = np.float64(n * sxy - sxj * sxk)
        r = (dn * dn) / (np.float64(dj) * np.float64(dk))
        lines.append(f"R {n} {sxy} {sxj} {sxk} {dj} {dk}")
        want.append([int(np.float64(r).view(np.uint64)), int(sr.q_of(r))])
    got = sr.run_host_program(exe, tmp_path / "r.txt", lines)
    assert got == want
    assert max(w[1] for w in want) == sr.Q_ONE and min(w[1] for w in want) == 0


def test_bin_of_the_host_routine_under_sanitizers(exe, tmp_path):
    rng = np.random.default_rng(5)
    cases = []
    for bs in (1, 2, 3, 1000, (1 << 32) - 1, 1 << 32, (1 << 40) + 7, (1 << 62) - 1, (1 << 63) - 1):
        for nbins in (1, 2, 511, 512, 513, 4095, 4096):
            for q in (0, 1, nbins - 1, nbins, nbins + 1, 8191, 8192, 1 << 20):
                for r in (0, 1, bs - 1):
                    dist = q * bs + r
                    if dist < (1 << 63) - 1:
                        cases.append((dist, bs, nbins))
    for _ in range(3000):
        bs = int(rng.integers(1, 1 << int(rng.integers(1, 63))))
        dist = int(rng.integers(0, 1 << int(rng.integers(1, 63))))
        cases.append((dist, bs, int(rng.integers(1, 4097))))
    got = sr.run_host_program(exe, tmp_path / "b.txt", [f"B {d} {b} {nb}" for d, b, nb in cases])
    want = [[min(d // b, nb)] for d, b, nb in cases]
    assert got == want
    assert {w[0] for w in want} >= {0, 1, 511, 512, 4095, 4096}
