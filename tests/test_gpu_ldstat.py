"""LD statistics on the GPU (include/tpg.h "LD statistics"): tpg_ld_stats and tpg_ld_band_r2 against the numpy restatement
tests/ldstat_ref.py -- every integer to equality, r2 bit for bit -- and the host layer on top of them (loci_ld_score, ld_decay,
ld_region_r2)."""
import ctypes as C

import numpy as np
import pytest

from tests import knn_impute_ref as kr
from tests import ld_ref
from tests import ldstat_ref as sr

pytestmark = pytest.mark.gpu

NS = (2, 3, 63, 64, 65, 130)  # one group of individuals, a group edge, the padding individuals of the last group
MS = (1, 2, 31, 32, 33, 65, 545, 1100)
WIDTHS = (0, 1, 31, 32, 33, 511, 512, 513, 1050)  # no pair; one tile; a super-chunk of 16 tiles, its edge; more than two
EINVAL, EUNSUPPORTED, ENUMERIC = 1, 3, 4


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


def _panel(seed, n, m, rho=0.7, mono=True):
    """genotypes with LD; monomorphic loci at 0, 31, 32 and m - 1 (three different constants)"""
    G = np.array(ld_ref.ld_panel(seed, n, m, rho))
    if mono:
        for j, c in ((0, 0), (31, 1), (32, 2), (m - 1, 0)):
            if 0 <= j < m:
                G[:, j] = c
    return np.asfortranarray(G)


def _view(tpg, G):
    return tpg.View(tpg.FBM.from_numpy(np.asfortranarray(G), code256=tpg.CODE_012))


def _windows(m):
    """(name, hi): every width, the whole panel, and three chromosomes cut off the tile edges, one of them a single locus"""
    out = [(f"w{w}", kr.window(m, w)) for w in WIDTHS if w == 0 or w < m + 32]
    out.append(("whole", kr.window(m, m)))
    if m >= 3:
        a = max(1, min(m - 2, 37 if m > 40 else m // 2))
        out.append(("chrom", kr.window(m, m, chrom_ends=[a, a + 1, m])))
    return out


def _got(tpg, v, hi, pos=None, bin_size=1, nbins=0, scores=True):
    return tpg.ld_stats(v, hi, pos, bin_size, nbins, scores=scores)


@pytest.mark.parametrize("n", NS)
def test_stats_and_band_equal_the_restatement(tpg, n):
    rng = np.random.default_rng(300 + n)
    valid = 0
    for m in MS:
        G = _panel(10 * n + m, n, m)
        v = _view(tpg, G)
        for name, hi in _windows(m):
            use_pos = rng.random() < 0.5
            pos = np.cumsum(rng.integers(0, 3, size=m)) if use_pos else None
            bin_size, nbins = (int(rng.integers(1, 4)), int(rng.integers(1, 700))) if name != "w0" else (1, 1)
            want = sr.stats(G, hi, pos, bin_size, nbins)
            got = _got(tpg, v, hi, pos, bin_size, nbins)
            assert sr.equal_stats(got, want), (m, name, use_pos, bin_size, nbins)
            valid += want["report"]["pairs_valid"]
            j0 = int(rng.integers(0, m))
            j1 = int(rng.integers(j0 + 1, m + 1))
            for a, b in ((0, m), (j0, j1)):
                assert sr.same_bits(tpg.ld_band_r2(v, hi, a, b), sr.band_r2(G, hi, a, b)), (m, name, a, b)
        v.free()
    assert valid > 0 or n < 3


def test_a_panel_that_is_monomorphic_everywhere(tpg):
    G = np.asfortranarray(np.tile(np.array([0, 1, 2, 1] * 17, dtype=np.uint8), (70, 1)))  # 70 x 68, every column a constant
    m = G.shape[1]
    v = _view(tpg, G)
    hi = kr.window(m, 40)
    got = _got(tpg, v, hi, None, 1, 64)
    assert sr.equal_stats(got, sr.stats(G, hi, None, 1, 64))
    assert got["report"]["pairs_valid"] == 0 and got["report"]["pairs"] > 0 and not got["score_q"].any() and not got["bin_pairs"].any()
    assert np.isnan(tpg.ld_band_r2(v, hi, 0, m)).all()
    X = tpg.FBM.from_numpy(G, code256=tpg.CODE_012)
    assert np.isnan(tpg.loci_ld_score(X, size=40, use_positions=False)).all()
    assert np.isnan(tpg.ld_region_r2(X, 2, 40)).all()


# (pos recipe, bin_size, nbins): ties; every pair in one bin; one bin and pairs beyond it; bins behind the 512 the workgroups keep
# on chip; distances and a bin_size of 2^32 and more
BIN_CASES = [("ties", 1, 4096), ("ties", 1, 1), ("ties", 1 << 40, 1), ("ties", 7, 3), ("index", 1, 4096), ("index", 1, 100),
             ("index", 3, 512), ("wide", 1, 4096), ("wide", 5, 4096), ("wide", 4000, 2), ("huge", 1 << 40, 4096), ("huge", (1 << 33) + 1, 9),
             ("huge", 1, 4096)]


def _bin_positions(m):
    rng = np.random.default_rng(41)
    return {"ties": np.cumsum(rng.integers(0, 3, size=m)), "index": None, "wide": np.cumsum(rng.integers(0, 40, size=m)),
            "huge": np.cumsum(rng.integers(0, 1 << 34, size=m)) - (1 << 40)}


@pytest.mark.parametrize("recipe,bin_size,nbins", BIN_CASES)
def test_bins(tpg, recipe, bin_size, nbins):
    n, m = 65, 545
    G = _panel(41, n, m)
    v = _view(tpg, G)
    pos = _bin_positions(m)[recipe]
    for hi in (kr.window(m, 300), kr.window(m, m, chrom_ends=[37, 38, m])):
        want = sr.stats(G, hi, pos, bin_size, nbins)
        got = _got(tpg, v, hi, pos, bin_size, nbins)
        assert sr.equal_stats(got, want)
        rep = got["report"]
        assert int(got["bin_pairs"].sum()) + rep["pairs_beyond"] == rep["pairs_valid"] == int(got["n_partners"].sum()) // 2


def test_bins_were_exercised_on_both_sides_of_every_edge():
    """the cases above, on the restatement alone: pairs beyond the last bin and none; bins behind bin 511 in use; a tie"""
    n, m = 65, 545
    G = _panel(41, n, m)
    pos = _bin_positions(m)
    hi = kr.window(m, 300)
    s = sr.stats(G, hi, pos["ties"], 1, 4096)
    assert s["bin_pairs"][0] > 0 and s["report"]["pairs_beyond"] == 0
    assert sr.stats(G, hi, pos["ties"], 7, 3)["report"]["pairs_beyond"] > 0
    s = sr.stats(G, hi, pos["wide"], 1, 4096)
    assert s["bin_pairs"][512:].sum() > 0 and s["report"]["pairs_beyond"] > 0
    s = sr.stats(G, hi, pos["huge"], (1 << 33) + 1, 9)
    assert (s["bin_pairs"] > 0).sum() > 1 and s["bin_sum_dist"].max() >= 1 << 32


def test_positions_that_decrease(tpg):
    n, m = 20, 100
    G = _panel(5, n, m)
    v = _view(tpg, G)
    hi = kr.window(m, 10, chrom_ends=[40, m])
    pos = np.r_[np.arange(40) * 3 + 500, np.arange(60) * 2]  # falls at the border of the two chromosomes only
    got = _got(tpg, v, hi, pos, 2, 50)
    assert sr.equal_stats(got, sr.stats(G, hi, pos, 2, 50))
    bad = pos.copy()
    bad[17] = bad[16] - 1
    with pytest.raises(tpg._lib.TpgError) as e:
        _got(tpg, v, hi, bad, 2, 50)
    assert e.value.code == EINVAL
    with pytest.raises(tpg._lib.TpgError) as e:  # the same positions under one window over the border
        _got(tpg, v, kr.window(m, 10), pos, 2, 50)
    assert e.value.code == EINVAL
    assert sr.equal_stats(_got(tpg, v, kr.window(m, 10), pos, 2, 0), sr.stats(G, kr.window(m, 10)))  # without bins nobody reads pos


def _raw_call(tpg, v, hi, pos, bin_size, nbins, sq, npart, bp, bq, bd, rep=None):
    """the C entry point itself; an argument is a numpy array, None, or device memory (the c_void_p of Context.dev_alloc)"""
    a = lambda x: x if isinstance(x, C.c_void_p) else tpg.api._ptr(x)
    return tpg._lib.lib.tpg_ld_stats(v.ctx.h, v.h, a(hi), a(pos), bin_size, nbins, a(sq), a(npart), a(bp), a(bq), a(bd),
                                     None if rep is None else C.byref(rep))


def test_each_group_alone_and_host_or_device_memory(tpg):
    n, m, nbins = 64, 545, 600
    rng = np.random.default_rng(9)
    G = _panel(9, n, m)
    v = _view(tpg, G)
    ctx, lib = v.ctx, tpg._lib.lib
    hi = kr.window(m, 513)
    pos = np.cumsum(rng.integers(0, 3, size=m)).astype(np.int64)
    want = sr.stats(G, hi, pos, 2, nbins)
    full = _got(tpg, v, hi, pos, 2, nbins)
    assert sr.equal_stats(full, want)
    assert sr.equal_stats(_got(tpg, v, hi, pos, 2, nbins), full)  # the same call twice: the same bits
    only_scores = _got(tpg, v, hi, pos, 2, 0)
    only_bins = _got(tpg, v, hi, pos, 2, nbins, scores=False)
    assert "bin_pairs" not in only_scores and "score_q" not in only_bins
    for k in ("score_q", "n_partners"):
        assert np.array_equal(only_scores[k], want[k])
    for k in ("bin_pairs", "bin_sum_q", "bin_sum_dist"):
        assert np.array_equal(only_bins[k], want[k])
    assert only_bins["report"] == want["report"] and only_scores["report"] == dict(want["report"], pairs_beyond=0)
    rep = tpg._lib.LdStatReport()  # neither group: the report alone
    assert _raw_call(tpg, v, hi, None, 0, 0, None, None, None, None, None, rep) == 0
    assert (rep.pairs, rep.pairs_valid, rep.band_tiles) == tuple(want["report"][k] for k in ("pairs", "pairs_valid", "band_tiles"))
    # hi, pos and every output in device memory
    bufs = []

    def dev(x):
        p = ctx.dev_alloc(max(16, x.nbytes))
        bufs.append(p)
        tpg._lib.check(lib.tpg_dev_from_host(ctx.h, p, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes)))
        return p

    def back(p, like):
        out = np.zeros_like(like)
        tpg._lib.check(lib.tpg_dev_to_host(ctx.h, C.c_void_p(out.ctypes.data), p, C.c_size_t(out.nbytes)))
        return out

    d_hi, d_pos = dev(hi), dev(pos)
    keys = ("score_q", "n_partners", "bin_pairs", "bin_sum_q", "bin_sum_dist")
    d_out = [dev(np.full_like(want[k], 77)) for k in keys]
    assert _raw_call(tpg, v, d_hi, d_pos, 2, nbins, *d_out) == 0
    for k, p in zip(keys, d_out):
        assert np.array_equal(back(p, want[k]), want[k]), k
    # mixed: the window on the device, the positions on the host, outputs alternating
    h_out = [np.full_like(want[k], 77) for k in keys]
    mixed = [d_out[i] if i % 2 else h_out[i] for i in range(5)]
    assert _raw_call(tpg, v, d_hi, pos, 2, nbins, *mixed) == 0
    for i, k in enumerate(keys):
        assert np.array_equal(back(d_out[i], want[k]) if i % 2 else h_out[i], want[k]), k
    d_r2 = dev(np.zeros((m, 513)))
    tpg._lib.check(lib.tpg_ld_band_r2(ctx.h, v.h, d_hi, 0, m, d_r2, 513))
    assert sr.same_bits(back(d_r2, np.zeros((m, 513))), sr.band_r2(G, hi, 0, m, 513))
    for p in bufs:
        ctx.dev_free(p)


def test_a_sub_view_equals_the_copied_sub_panel(tpg):
    rng = np.random.default_rng(12)
    big = _panel(12, 140, 300, mono=False)
    X = tpg.FBM.from_numpy(big, code256=tpg.CODE_012)
    rows = np.arange(140, 0, -2, dtype=np.int32)  # reversed
    cols = np.r_[np.arange(2, 120, 3), np.arange(121, 300)].astype(np.int32)
    sub = np.asfortranarray(big[rows - 1][:, cols - 1])
    m = len(cols)
    hi = kr.window(m, 60)
    pos = np.cumsum(rng.integers(1, 5, size=m))
    want = sr.stats(sub, hi, pos, 4, 80)
    for v in (tpg.View(X, rows, cols), _view(tpg, sub)):
        assert sr.equal_stats(_got(tpg, v, hi, pos, 4, 80), want)
        assert sr.same_bits(tpg.ld_band_r2(v, hi, 10, 200), sr.band_r2(sub, hi, 10, 200))
    sel = tpg.View(X).select_loci(cols - 1)
    assert sr.equal_stats(_got(tpg, sel, hi, pos, 4, 80), sr.stats(np.asfortranarray(big[:, cols - 1]), hi, pos, 4, 80))


def test_errors_leave_the_outputs_untouched(tpg):
    n, m = 30, 70
    G = _panel(3, n, m)
    hi = kr.window(m, 20)
    v = _view(tpg, G)
    holes = G.copy()
    holes[4, 50] = 3
    v_holes = tpg.View(tpg.FBM.from_numpy(holes, code256=tpg.CODE_012))
    bad_hi, short_hi = hi.copy(), hi.copy()
    bad_hi[10] = bad_hi[9] - 1  # decreases
    short_hi[5] = 4  # below its own locus
    cases = [(v_holes, hi, 1, 8, ENUMERIC), (v, bad_hi, 1, 8, EINVAL), (v, short_hi, 1, 8, EINVAL), (v, hi, 1, 0, EINVAL),
             (v, hi, 1, 4097, EINVAL), (v, hi, 0, 8, EINVAL)]
    for vv, h, bin_size, nbins, code in cases:
        outs = [np.full(m, 77, dtype=np.uint64), np.full(m, 77, dtype=np.int32), np.full(4097, 77, dtype=np.int64),
                np.full(4097, 77, dtype=np.uint64), np.full(4097, 77, dtype=np.int64)]
        rep = tpg._lib.LdStatReport(77, 77, 77, 77)
        assert _raw_call(tpg, vv, h, None, bin_size, nbins, *outs, rep) == code, (bin_size, nbins, code)
        assert all((o == 77).all() for o in outs) and rep.pairs == 77 and rep.band_tiles == 77
        r2 = np.full((m, 20), 77.0)
        if vv is v_holes or h is not hi:
            assert tpg._lib.lib.tpg_ld_band_r2(vv.ctx.h, vv.h, tpg.api._ptr(h), 0, m, tpg.api._ptr(r2), 20) == code
            assert (r2 == 77.0).all()
    # half a group is an error too
    sq = np.full(m, 77, dtype=np.uint64)
    assert _raw_call(tpg, v, hi, None, 1, 0, sq, None, None, None, None) == EINVAL and (sq == 77).all()
    r2 = np.full((m, 20), 77.0)
    band = tpg._lib.lib.tpg_ld_band_r2
    for j0, j1, stride in ((0, m, 19), (5, 5, 20), (-1, 4, 20), (0, m + 1, 20), (0, m, (1 << 26) // m + 1)):
        assert band(v.ctx.h, v.h, tpg.api._ptr(hi), j0, j1, tpg.api._ptr(r2), stride) == EINVAL, (j0, j1, stride)
    assert (r2 == 77.0).all()
    # sizes the definition refuses, both seen on the host before anything runs: 2^33 pairs or more, 2^22 individuals or more
    wide = _view(tpg, np.zeros((2, 131073), dtype=np.uint8))
    sq, npart = np.full(wide.m, 77, dtype=np.uint64), np.full(wide.m, 77, dtype=np.int32)
    whole = kr.window(wide.m, wide.m)
    assert int((whole - np.arange(wide.m)).sum()) == (1 << 33) + (1 << 16)
    assert _raw_call(tpg, wide, whole, None, 1, 0, sq, npart, None, None, None) == EUNSUPPORTED
    tall = _view(tpg, np.zeros((1 << 22, 2), dtype=np.uint8))
    assert _raw_call(tpg, tall, kr.window(2, 1), None, 1, 0, sq[:2], npart[:2], None, None, None) == EUNSUPPORTED
    r2 = np.full((2, 1), 77.0)
    assert band(tall.ctx.h, tall.h, tpg.api._ptr(kr.window(2, 1)), 0, 2, tpg.api._ptr(r2), 1) == EUNSUPPORTED
    assert (sq == 77).all() and (npart == 77).all() and (r2 == 77.0).all()
    with pytest.raises(ValueError):
        tpg.loci_ld_score(tpg.FBM.from_numpy(np.asfortranarray(G[:2]), code256=tpg.CODE_012), size=5, use_positions=False)  # n < 3


@pytest.mark.parametrize("n", (3, 64, 130))
def test_band_r2_is_the_r2_of_the_top_neighbours(tpg, n):
    m = 200
    G = _panel(50 + n, n, m)
    v = _view(tpg, G)
    for hi in (kr.window(m, 33), kr.window(m, m, chrom_ends=[70, 71, m])):
        width = int((hi - np.arange(m)).max())
        band = tpg.ld_band_r2(v, hi, 0, m)
        assert band.shape == (m, max(1, width))
        nbr, r2 = tpg.ld_top_neighbours(v, hi, 32, 0.0)
        seen = 0
        for j in range(m):
            for k, r in zip(nbr[j], r2[j]):
                if k > j:  # a forward neighbour: the pair (j, k) of the band
                    assert np.float64(r).view(np.uint64) == band[j, k - j - 1].view(np.uint64), (j, k)
                    seen += 1
                elif k >= 0:
                    assert np.float64(r).view(np.uint64) == band[k, j - k - 1].view(np.uint64), (j, k)
        assert seen > m or n == 3
        inside = np.arange(band.shape[1])[None, :] < (hi - np.arange(m))[:, None]
        assert np.isnan(band[~inside]).all()  # outside the window
        _, _, d = ld_ref.sums(G)
        for j in np.flatnonzero(d == 0):  # a monomorphic locus: its row, and its entry in the rows in front of it
            assert np.isnan(band[j]).all()
            for i in range(max(0, j - width), j):
                if hi[i] >= j:
                    assert np.isnan(band[i, j - i - 1])
        assert not np.isnan(band[inside & (d > 0)[:, None]]).all()


def test_mid_size_panel_through_the_host_layer(tpg):
    n, m = 300, 8192
    G = _panel(77, n, m, rho=0.9)
    X = tpg.FBM.from_numpy(G, code256=tpg.CODE_012)
    chrom = np.r_[np.full(3000, 1), np.full(37, 2), np.full(m - 3037, 3)]
    pos = np.r_[np.arange(3000) * 7, np.arange(37) * 5, np.cumsum(np.random.default_rng(1).integers(0, 9, size=m - 3037))]
    # windows of 600 loci
    hi = ld_ref.window_hi(chrom, None, 600, use_positions=False)
    s = sr.stats(G, hi)
    for adjusted, include_self in ((True, True), (False, False)):
        got = tpg.loci_ld_score(X, size=600, chromosome=chrom, use_positions=False, adjusted=adjusted, include_self=include_self)
        want = sr.ld_score(G, hi, adjusted, include_self, s=s)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == 4
        assert np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])  # the same integers through the same expression
    # windows of 2 000 positions, one curve per chromosome
    hi = ld_ref.window_hi(chrom, pos, 2.0, use_positions=True)
    got = tpg.ld_decay(X, size=2.0, chromosome=chrom, position=pos, bin_size=25, n_bins=60, by_chromosome=True, adjusted=True)
    assert list(got["chromosome"]) == [1, 2, 3]
    for c, (a, b) in enumerate(((0, 3000), (3000, 3037), (3037, m))):
        want = sr.decay(G[:, a:b], hi[a:b] - a, pos[a:b], 25, 60, adjusted=True)
        for k, w in want.items():
            g = got[k][c]
            assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.nan_to_num(g), np.nan_to_num(w)), (c, k)
    assert got["pairs_beyond"].sum() > 0 and (got["n_pairs"] > 0).any(axis=1).all()
    whole = tpg.ld_decay(X, size=2.0, chromosome=chrom, position=pos, bin_size=25, n_bins=60)
    assert np.array_equal(whole["n_pairs"], got["n_pairs"].sum(axis=0)) and whole["pairs_beyond"] == got["pairs_beyond"].sum()
    R = tpg.ld_region_r2(X, 2990, 3100)
    assert sr.same_bits(R, sr.region_r2(G, 2990, 3100))
