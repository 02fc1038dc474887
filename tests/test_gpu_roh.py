"""GPU: runs of homozygosity (include/tpg.h "Runs of homozygosity") against the numpy restatement tests/roh_ref.py.  Everything
is an integer, so every comparison is equality: the in-run bits of the status stage with their padding, the runs with nOpp /
nMiss, the per-individual summary and the per-locus counts."""
import ctypes as C

import numpy as np
import pytest

from tests import roh_ref as rr

pytestmark = pytest.mark.gpu

NS = (1, 31, 32, 33, 65, 500)
MS = (1, 14, 127, 128, 129, 1000, 4097)
WS = (1, 2, 15, 64, 128, 129, 512)
GRID = [(n, m, WS[(a + b) % len(WS)]) for a, n in enumerate(NS) for b, m in enumerate(MS)]
assert {w for _, _, w in GRID} == set(WS) and (1, 4097, 512) in GRID


def _view(tpg, G, ind_row=None, ind_col=None):
    X = tpg.FBM.from_numpy(np.asfortranarray(G), code256=tpg.CODE_012)
    return tpg.View(X, ind_row, ind_col)


def _check_detect(tpg, v, G, chrom, pos, **kw):
    want = rr.roh_vec(G, chrom, pos, **kw)
    r = tpg.Roh(v, chrom, pos, **kw)
    got = r.fetch()
    assert r.count == len(want["indiv"])
    assert rr.same_runs(got, want)
    n_runs, total = r.indiv_summary()
    w_runs, w_total = rr.indiv_summary(want, G.shape[0], pos)
    assert np.array_equal(n_runs, w_runs) and np.array_equal(total, w_total)
    lc = r.locus_counts()
    assert lc.dtype == np.int32 and np.array_equal(lc, rr.locus_counts(want, G.shape[1]))
    r.free()
    return want


@pytest.mark.parametrize("n,m,W", GRID)
def test_grid_status_and_runs(n, m, W):
    import tidypopgen_amd as tpg

    G = rr.roh_panel(100 + n, n, m, W)
    chrom, pos = rr.roh_loci(100 + n, m, W=W)
    v = _view(tpg, G)
    for kw in (dict(window_size=W), dict(window_size=W, threshold=0.3, max_opp_window=2, max_miss_window=0)):
        want = rr.status_vec(G, chrom, pos, rr.params(**kw))
        bits = tpg.roh_snp_status(v, chrom, pos, return_bits=True, **kw)
        assert np.array_equal(bits, rr.pack_bits(want))  # padding bits of the last word included
        assert np.array_equal(tpg.roh_snp_status(v, chrom, pos, **kw), want)
    _check_detect(tpg, v, G, chrom, pos, window_size=W)
    _check_detect(tpg, v, G, chrom, pos, window_size=W, **rr.UNFILTERED)


@pytest.mark.parametrize("seed,n,m,W", [p for p in rr.FILTER_PANELS if p[3] in (15, 128) and p[2] >= 1000])
def test_every_filter_and_runs_of_heterozygosity(seed, n, m, W):
    import tidypopgen_amd as tpg

    G = rr.roh_panel(seed, n, m, W)
    chrom, pos = rr.roh_loci(seed, m, W=W)
    v = _view(tpg, G)
    base = _check_detect(tpg, v, G, chrom, pos, window_size=W, **rr.UNFILTERED)
    for name, over, _ in rr.FILTERS:
        kw = dict(rr.UNFILTERED, window_size=W, **over)
        if kw["min_snp"] == "W+5":
            kw["min_snp"] = W + 5
        got = _check_detect(tpg, v, G, chrom, pos, **kw)
        assert rr.run_set(got) != rr.run_set(base), name  # (tests/test_roh_host.py asserts the same of the reference alone)
    het = _check_detect(tpg, v, G, chrom, pos, window_size=W, heterozygosity=True, max_opp_window=(2 * W) // 3, **rr.UNFILTERED)
    assert len(het["indiv"]) > 0
    bits = tpg.roh_snp_status(v, chrom, pos, return_bits=True, window_size=W, heterozygosity=True, max_opp_window=(2 * W) // 3)
    assert np.array_equal(bits, rr.pack_bits(rr.status_vec(G, chrom, pos, rr.params(window_size=W, heterozygosity=True,
                                                                                     max_opp_window=(2 * W) // 3))))


def test_a_wider_stride_leaves_the_extra_words_zero():
    import tidypopgen_amd as tpg

    n, m, W = 33, 129, 15
    G = rr.roh_panel(7, n, m, W)
    chrom, pos = rr.roh_loci(7, m, W=W)
    v = _view(tpg, G)
    want = rr.status_vec(G, chrom, pos, rr.params(window_size=W))
    bits = tpg.roh_snp_status(v, chrom, pos, stride_words=9, return_bits=True, window_size=W)
    assert bits.shape == (n, 9) and np.array_equal(bits, rr.pack_bits(want, 9)) and not bits[:, 5:].any()
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.roh_snp_status(v, chrom, pos, stride_words=4, return_bits=True, window_size=W)
    assert e.value.code == 1


@pytest.mark.parametrize("which", ["2C+1", "3C-1"])
@pytest.mark.parametrize("W", [15, 129])
def test_chunk_seams(which, W):
    import tidypopgen_amd as tpg

    Cc = tpg.ROH_CHUNK_LOCI
    m = 2 * Cc + 1 if which == "2C+1" else 3 * Cc - 1
    n = 33
    G = rr.roh_panel(11, n, m, W)
    chrom, pos = rr.roh_loci(11, m, W=W)
    G[0] = 0          # homozygous everywhere: one run per unbroken stretch, across every seam
    G[1] = 1          # heterozygous everywhere: no run
    G[2] = 3          # all missing
    G[3] = 1
    G[3, Cc - 3 * W:Cc] = 2      # a run that ends exactly on a seam (its last locus is the last of chunk 0)
    G[4] = 1
    G[4, Cc:Cc + 3 * W] = 0      # a run that starts exactly on a seam
    G[5] = 1
    if m >= 2 * Cc + 3 * W:
        G[5, 2 * Cc:2 * Cc + 3 * W] = 0  # the same on the second seam
    G[32] = np.where(np.arange(m) % (2 * W) == 0, 1, 0)  # one heterozygote per window's reach: runs across the seams
    pos = 1000 + 100 * np.arange(m, dtype=np.int64)      # (no gap next to the seams: the planted runs stand whole)
    cb = Cc + 5 * W                                      # the second chromosome begins here
    chrom = np.where(np.arange(m) < cb, 1, 2).astype(np.int32)
    v = _view(tpg, G)
    thr = 1.0 / (2 * W)  # need = 1 whatever the cover: one OK window puts its loci into a run, so the ends are exact
    for kw in (dict(window_size=W, threshold=thr), dict(window_size=W, threshold=thr, **rr.UNFILTERED)):
        want = rr.status_vec(G, chrom, pos, rr.params(**kw))
        assert np.array_equal(tpg.roh_snp_status(v, chrom, pos, return_bits=True, **kw), rr.pack_bits(want))
        runs = _check_detect(tpg, v, G, chrom, pos, **kw)
        by = {i: [(a, b) for j, a, b in sorted(rr.run_set(runs)) if j == i] for i in range(6)}
        assert by[0] == [(0, cb - 1), (cb, m - 1)] and by[1] == [] and by[2] == []
        assert by[3] == [(Cc - 3 * W - 1, Cc)] and by[4] == [(Cc - 1, Cc + 3 * W)]  # (one heterozygote joins at either end)
    # with clean windows only, the two planted runs begin and end on the seam itself
    kw = dict(window_size=W, threshold=thr, max_opp_window=0, **rr.UNFILTERED)
    _check_detect(tpg, v, G, chrom, pos, window_size=W)  # and the default threshold, against the reference alone
    runs = _check_detect(tpg, v, G, chrom, pos, **kw)
    got = sorted(rr.run_set(runs))
    assert (3, Cc - 3 * W, Cc - 1) in got and (4, Cc, Cc + 3 * W - 1) in got
    assert ((5, 2 * Cc, 2 * Cc + 3 * W - 1) in got) == (m >= 2 * Cc + 3 * W)


def test_a_view_without_T_gives_the_same_runs():
    import tidypopgen_amd as tpg

    n, m, W = 65, 1000, 15
    G = rr.roh_panel(13, n, m, W)
    chrom, pos = rr.roh_loci(13, m, W=W)
    X = tpg.FBM.from_numpy(np.asfortranarray(G), code256=tpg.CODE_012)
    va, vb = tpg.View.pair(X, None, None, code256_a=tpg.CODE_012, code256_b=tpg.CODE_012)
    v = tpg.View(X)
    want = rr.pack_bits(rr.status_vec(G, chrom, pos, rr.params(window_size=W)))
    for view in (v, va, vb):
        assert np.array_equal(tpg.roh_snp_status(view, chrom, pos, return_bits=True, window_size=W), want)
        _check_detect(tpg, view, G, chrom, pos, window_size=W)


def test_row_and_column_subsets_and_the_table():
    import tidypopgen_amd as tpg

    n, m, W = 70, 1200, 15
    G = rr.roh_panel(17, n, m, W)
    rng = np.random.default_rng(17)
    rows = np.sort(rng.permutation(n)[:45]) + 1
    cols = np.sort(rng.permutation(m)[:1000]) + 1
    chrom, pos = rr.roh_loci(17, len(cols), W=W)
    sub = G[np.ix_(rows - 1, cols - 1)]
    X = tpg.FBM.from_numpy(np.asfortranarray(G), code256=tpg.CODE_012)
    _check_detect(tpg, tpg.View(X, rows, cols), sub, chrom, pos, window_size=W)
    want = rr.roh_vec(sub, chrom, pos, window_size=W)
    ids = np.array([f"id{r}" for r in rows])
    labels = np.array(["chr%d" % c for c in chrom])
    out, rep = tpg.windows_indiv_roh(X, rows, cols, chromosome=labels, position=pos, ids=ids, return_report=True)
    assert list(out) == ["group", "id", "chrom", "nSNP", "from", "to", "lengthBps", "first_locus", "last_locus", "n_opp", "n_miss"]
    assert np.array_equal(out["id"], ids[want["indiv"]]) and np.array_equal(out["group"], out["id"])
    assert np.array_equal(out["chrom"], labels[want["first"]])
    assert np.array_equal(out["first_locus"], want["first"]) and np.array_equal(out["last_locus"], want["last"])
    assert np.array_equal(out["nSNP"], want["last"] - want["first"] + 1)
    assert np.array_equal(out["from"], pos[want["first"]]) and np.array_equal(out["to"], pos[want["last"]])
    assert np.array_equal(out["lengthBps"], pos[want["last"]] - pos[want["first"]])
    assert np.array_equal(out["n_opp"], want["n_opp"]) and np.array_equal(out["n_miss"], want["n_miss"])
    w_runs, w_total = rr.indiv_summary(want, len(rows), pos)
    assert np.array_equal(rep["n_runs"], w_runs) and np.array_equal(rep["sum_length_bps"], w_total)
    assert np.array_equal(rep["locus_counts"], rr.locus_counts(want, len(cols)))
    plain = tpg.windows_indiv_roh(X, rows, cols, chromosome=labels, position=pos, groups=np.arange(len(rows)) % 3)
    assert np.array_equal(plain["id"], want["indiv"]) and np.array_equal(plain["group"], want["indiv"] % 3)


def test_edge_cases():
    import tidypopgen_amd as tpg
    from tidypopgen_amd import _lib

    n, m = 5, 40
    G = np.zeros((n, m), dtype=np.uint8)
    chrom, pos = np.ones(m, dtype=np.int32), 1000 * np.arange(m, dtype=np.int64)
    v = _view(tpg, G)
    r = tpg.Roh(v, chrom, pos, window_size=41)  # m < W: no window, no run
    assert r.count == 0 and not r.indiv_summary()[0].any() and not r.locus_counts().any()
    assert not tpg.roh_snp_status(v, chrom, pos, window_size=41).any()
    r = tpg.Roh(v, chrom, pos, window_size=40)
    assert r.count == n and np.array_equal(r.fetch()["last"], np.full(n, m - 1))

    def detect(P, ch, ps):
        h = C.c_void_p()
        rc = _lib.lib.tpg_roh_detect(v.ctx.h, v.h, ch.ctypes.data, ps.ctypes.data, C.byref(P), C.byref(h))
        if h:
            _lib.lib.tpg_roh_free(h)
        return rc

    ok = tpg.api._roh_params(window_size=15)
    assert detect(ok, chrom, pos) == 0
    wide = tpg.api._roh_params(window_size=15)
    wide.window_size = 513
    assert detect(wide, chrom, pos) == 1  # TPG_EINVAL
    back = pos.copy()
    back[20] = back[19] - 1
    assert detect(ok, chrom, back) == 1 and "not ordered" in _lib.lib.tpg_last_error().decode()
    two = chrom.copy()
    two[20:] = 2  # the same positions on a new chromosome are in order
    assert detect(ok, two, back) == 0
    with pytest.raises(ValueError, match="not ordered"):
        tpg.roh_snp_status(v, chrom, back)
