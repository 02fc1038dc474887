"""GPU: autoSVD (include/tpg.h "autoSVD") against the numpy restatement tests/autosvd_ref.py.

What is compared how.
  select_loci: the sub-view against the view packed from the store with the same columns -- its codes, its per-locus counts,
    the pairwise counts (they need the T layout) and the PCA -- bit for bit; from an imputed view against imputing, then slicing.
  rollmean: bit for bit the reference loop fed the library's weights (the weights themselves are held to the reference within
    1e-13 in tests/test_autosvd_host.py: the host's exp and erfc may differ from Python's by an ulp).
  tukey_mc_up: q1, q3, med and the medcouple bit for bit against brute force over all ratios; coef and thr within 1e-12 relative
    (qnorm_upper goes through erfc, exp on the host).  One exponential sample of 200 001 values (N = 1e10 > 2^32 ratios) against
    the reference's vectorised bisection.
  The driver on the planted panel (generator seed 1: the reference's smallest |S2 - thr| / thr is 1.5e-2): the reference's
    conditions first, then the same kept set, iterations and long-range LD regions; the SVD bit for bit gt_pca_partialSVD on the
    kept loci; the one call bit for bit the staged calls.  The reference takes its loadings from numpy's SVD and the library
    from its own PCA; on this panel the two fences differ by 2.7e-4 relative in q1 (measured), inside the margin.  Steps 3 - 5
    themselves are held tighter: the reference fed the DEVICE's loadings must give the device's report within 1e-8 relative.
    Reasoning: the OGK distance agrees with the reference to 1e-12 .. 1e-11 on the same input (tests/test_gpu_pcadapt.py: 6.2e-13
    at eigengaps of 0.03); the square root halves a relative error, the rolling mean is a convex combination and the quartiles
    and the median are selections (no amplification); the medcouple divides differences from the median, which for the middle
    ratios are of the order of the interquartile range, a tenth of the values here: a factor of a few tens; the fence is linear
    in the quartiles and has d thr / d mc <= 4 (thr - q3).  1e-8 leaves two orders of room.  Measured: 3.8e-12 in q1 / q3 / med,
    1.3e-10 in mc, 7.9e-12 in thr (last pass); 4.1e-13, 2.6e-11, 1.6e-12 (first pass)."""
import ctypes as C

import numpy as np
import pytest

from tests import autosvd_ref as ar

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _svd(v, k):
    """tpg_pca_partial_svd on a view -> dict(d, u, v, center, scale, square_frobenius)"""
    from tidypopgen_amd.api import _ptr, check, lib

    d, u, vl = np.zeros(k), np.zeros((v.n, k), order="F"), np.zeros((v.m, k), order="F")
    center, scale, fro = np.zeros(v.m), np.zeros(v.m), C.c_double()
    check(lib.tpg_pca_partial_svd(v.ctx.h, v.h, k, _ptr(d), _ptr(u), _ptr(vl), _ptr(center), _ptr(scale), C.byref(fro)))
    return dict(d=d, u=u, v=vl, center=center, scale=scale, square_frobenius=fro.value)


def _pairwise_counts(v):
    import tidypopgen_amd as tpg

    pw = tpg.Pairwise(v.ctx, v.n)
    pw.accumulate(v)
    return pw.counts()


# ---- select_loci ------------------------------------------------------------------------------------------------------------
def _idx_variants(m, rng):
    tiles = np.unique(np.r_[np.arange(0, m, 32), np.minimum(np.arange(31, m + 31, 32), m - 1)])
    return {"all": np.arange(m), "every_other": np.arange(0, m, 2), "reversed": np.arange(m)[::-1].copy(),
            "tile_edges": tiles, "duplicate": np.r_[tiles, tiles[-1], rng.integers(0, m, 3), 0]}


@pytest.mark.parametrize("n", [1, 33, 129, 257])
@pytest.mark.parametrize("m", [1, 31, 33, 130, 1500])
def test_select_loci_is_the_view_packed_from_the_store(n, m):
    import tidypopgen_amd as tpg

    rng = np.random.default_rng(1000 * n + m)
    G = rng.integers(0, 4, size=(n, m)).astype(np.uint8)  # 3 = missing
    X = tpg.FBM.from_numpy(np.asfortranarray(G), code256=tpg.CODE_012)
    v = tpg.View(X)
    for name, idx in _idx_variants(m, rng).items():
        sub, want = v.select_loci(idx), tpg.View(X, None, idx + 1)
        assert (sub.n, sub.m) == (n, len(idx))
        assert np.array_equal(sub.unpack(), G[:, idx]), name
        assert np.array_equal(tpg.loci_counts(sub), tpg.loci_counts(want)), name
        a, b = _pairwise_counts(sub), _pairwise_counts(want)
        for key in a:
            assert np.array_equal(a[key], b[key]), (name, key)
    # from an imputed view: imputing, then slicing
    imp = v.impute("mode")
    idx = _idx_variants(m, rng)["duplicate"]
    assert np.array_equal(imp.select_loci(idx).unpack(), imp.unpack()[:, idx])
    for bad in ([m], [-1], [0, m + 5], []):
        with pytest.raises(tpg._lib.TpgError) as e:
            v.select_loci(np.array(bad, dtype=np.int64))
        assert e.value.code == 1, bad  # TPG_EINVAL


@pytest.mark.parametrize("n,m", [(33, 130), (129, 1500), (257, 33)])
def test_pca_of_a_selected_view_is_the_pca_of_the_packed_view(n, m):
    import tidypopgen_amd as tpg

    rng = np.random.default_rng(7 * n + m)
    G = rng.binomial(2, rng.uniform(0.2, 0.8, m), size=(n, m)).astype(np.uint8)
    X = tpg.FBM.from_numpy(np.asfortranarray(G), code256=tpg.CODE_012)
    v = tpg.View(X)
    for name, idx in _idx_variants(m, rng).items():
        if len(idx) < 8:
            continue
        sub, want = v.select_loci(idx), tpg.View(X, None, idx + 1)
        ca, cb = tpg.pca_center_scale(sub), tpg.pca_center_scale(want)
        assert _same_bits(ca[0], cb[0]) and _same_bits(ca[1], cb[1]), name
        assert _same_bits(tpg.pca_gram(sub, *ca), tpg.pca_gram(want, *cb)), name
        a, b = _svd(sub, 3), _svd(want, 3)
        for key in a:
            assert _same_bits(a[key], b[key]), (name, key)


# ---- rollmean ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1, 4, 5, 50])
def test_rollmean_is_the_reference_loop(radius):
    import tidypopgen_amd as tpg

    ln, m = 2 * radius + 1, 3000
    seg = np.array([0, ln, 2 * ln + 1, m])
    chrom = np.repeat([3, 1, 2], np.diff(seg))  # (labels need not ascend)
    rng = np.random.default_rng(radius)
    x = rng.exponential(size=m)
    w = tpg.rollmean_weights(radius)
    assert len(w) == ln
    got = tpg.rollmean(x, chrom, radius)
    assert _same_bits(got, ar.rollmean_fast(x, seg, radius, w=w))
    if radius <= 5:
        assert _same_bits(got[:3 * ln], ar.rollmean(x, seg, radius, w=w)[:3 * ln])  # the plain loops on the short segments
    assert _same_bits(tpg.rollmean(x[:ln], None, radius), ar.rollmean_fast(x[:ln], np.array([0, ln]), radius, w=w))
    if radius:
        short = np.repeat([1, 2], [ln - 1, ln + 3])
        with pytest.raises(tpg._lib.TpgError, match="roll_size exceeds the number of variants on at least one chromosome") as e:
            tpg.rollmean(x[:len(short)], short, radius)
        assert e.value.code == 1


def test_rollmean_refuses_a_radius_beyond_its_table():
    import tidypopgen_amd as tpg

    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.rollmean(np.zeros(4000), None, 1025)
    assert e.value.code == 1


# ---- medcouple / tukey_mc_up ------------------------------------------------------------------------------------------------
COUNTS = (1, 2, 3, 4, 5, 64, 65, 1023, 1025, 2049)


def _content(kind, c, rng):
    if kind == "normal":
        return rng.standard_normal(c)
    if kind == "exponential":
        return rng.exponential(size=c)
    if kind == "small_integers":  # heavy ties, also at the median
        return rng.integers(0, 4, c).astype(np.float64)
    if kind == "all_equal":
        return np.full(c, 2.5)
    if kind == "subnormals":
        return rng.permutation(np.r_[rng.integers(-40, 40, c - c // 2) * 5e-324, rng.standard_normal(c // 2) * 1e-310])
    if kind == "huge":
        return rng.choice([1e300, -1e300, 1.0, -1.0, 0.5], size=c) * rng.uniform(0.5, 1.0, c)
    if kind == "signed_zeros":
        return rng.choice([0.0, -0.0, 1.0, -1.0, -0.0], size=c)
    if kind == "non_finite":  # NaN and the infinities never enter a count or a rank
        x = rng.exponential(size=c)
        bad = rng.random(c) < 0.3
        x[bad] = rng.choice([np.nan, np.inf, -np.inf], size=int(bad.sum()))
        return x
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["normal", "exponential", "small_integers", "all_equal", "subnormals", "huge", "signed_zeros",
                                  "non_finite"])
def test_tukey_fence_is_the_brute_force_over_all_ratios(kind):
    import tidypopgen_amd as tpg

    rng = np.random.default_rng(len(kind))
    for c in COUNTS:
        x = _content(kind, c, rng)
        got, want = tpg.tukey_mc_up(x, 0.05), ar.tukey_mc_up(x, 0.05)
        assert got["n_finite"] == want["n_finite"], (kind, c)
        for key in ("q1", "q3", "med", "mc"):
            assert _same_bits(got[key], want[key]), (kind, c, key, got[key], want[key])
        for key in ("coef", "thr"):
            assert (np.isnan(got[key]) and np.isnan(want[key])) or abs(got[key] - want[key]) <= 1e-12 * abs(want[key]), (kind, c, key)
        assert _same_bits(tpg.medcouple(x), want["mc"]), (kind, c)


def test_no_finite_value_gives_nan():
    import tidypopgen_amd as tpg

    for x in (np.array([]), np.array([np.nan, np.inf, -np.inf])):
        r = tpg.tukey_mc_up(x, 0.05)
        assert r["n_finite"] == 0 and all(np.isnan(r[key]) for key in ("q1", "q3", "med", "mc", "coef", "thr"))
        assert np.isnan(tpg.medcouple(x))


def test_medcouple_counts_in_64_bits():
    import tidypopgen_amd as tpg

    x = np.random.default_rng(9).exponential(size=200001)  # N = 100 001 x 100 001 > 2^32
    assert _same_bits(tpg.medcouple(x), ar.medcouple_bisect(x))


# ---- the driver on the planted panel ----------------------------------------------------------------------------------------
ARGS = dict(k=ar.PANEL_K, thr_r2=ar.PANEL_THR, use_positions=False, size=ar.PANEL_WINDOW, roll_size=ar.PANEL_ROLL,
            chromosome=ar.CHROM, position=ar.POSITION)


@pytest.fixture(scope="module")
def planted():
    import tidypopgen_amd as tpg

    G, hi, ref = ar.planted_reference()
    ar.check_planted_reference(G, ref)  # the conditions on the reference alone come first
    X = tpg.FBM.from_numpy(np.asfortranarray(G.astype(np.uint8)), code256=tpg.CODE_012)
    return dict(G=G, hi=hi, ref=ref, X=X, got=tpg.gt_pca_autoSVD(X, **ARGS))


def test_driver_keeps_what_the_reference_keeps(planted):
    ref, got = planted["ref"], planted["got"]
    assert np.array_equal(got["loci"], ref["kept"] + 1)
    assert not np.isin(ar.LOW_MAC + 1, got["loci"]).any()
    assert got["n_iter"] == ref["n_iter"] == 2 and got["converged"] is True and got["method"] == "autoSVD"
    assert len(got["history"]) == len(ref["history"])
    for a, b in zip(got["history"], ref["history"]):
        assert (a["n_kept"], a["n_outliers"]) == (b["n_kept"], b["n_outliers"])
        assert np.array_equal(a["pos0"], b["pos0"]) and np.array_equal(a["idx0"], b["idx0"])
    want = [(int(ar.CHROM[a]), int(ar.POSITION[a]), int(ar.POSITION[b])) for h in ref["history"] for a, b in h["runs"]]
    assert len(want) == 1 and got["lrldr"] == want


def test_driver_returns_the_svd_of_the_kept_loci(planted):
    import tidypopgen_amd as tpg

    got = planted["got"]
    want = tpg.gt_pca_partialSVD(planted["X"], None, got["loci"], k=ar.PANEL_K)
    for key in ("d", "u", "v", "center", "scale"):
        assert _same_bits(got[key], want[key]), key
    assert got["square_frobenius"] == want["square_frobenius"]


def test_one_call_is_the_staged_calls(planted):
    import tidypopgen_amd as tpg

    X, got, hi = planted["X"], planted["got"], planted["hi"]
    v = tpg.View(X, code256=tpg.CODE_IMPUTE_PRED)
    counts = tpg.loci_counts(v).astype(np.int64)
    sx = counts[:, 1] + 2 * counts[:, 2]
    exclude = np.minimum(sx, 2 * v.n - sx) < 10
    idx = np.flatnonzero(tpg.ld_clump(v, hi, ar.PANEL_THR, exclude=exclude))
    history = []
    while True:
        svd = _svd(v.select_loci(idx), ar.PANEL_K)
        S = np.sqrt(tpg.robust_dist_ogk(svd["v"])["dist"])
        S2 = tpg.rollmean(S, ar.CHROM[idx], ar.PANEL_ROLL)
        rep = tpg.tukey_mc_up(S2, 0.05)
        out = S2 > rep["thr"]
        history.append((len(idx), np.flatnonzero(out), idx[out], rep))
        if not out.any():
            break
        idx = idx[~out]
    assert np.array_equal(got["loci"], idx + 1) and len(history) == len(got["history"])
    for (nk, pos, oidx, rep), h in zip(history, got["history"]):
        assert nk == h["n_kept"] and np.array_equal(pos, h["pos0"]) and np.array_equal(oidx, h["idx0"])
        assert rep["n_finite"] == h["report"]["n_finite"]
        for key in ("q1", "q3", "med", "mc", "coef", "thr"):
            assert _same_bits(rep[key], h["report"][key]), key
    for key in ("d", "u", "v", "center", "scale"):
        assert _same_bits(got[key], svd[key]), key


def test_steps_3_to_5_on_the_device_loadings_are_the_reference(planted):
    import tidypopgen_amd as tpg

    X, got = planted["X"], planted["got"]
    kept = got["loci"] - 1  # the last iteration: its loadings are the ones returned
    r = ar.detect(got["v"], ar.CHROM[kept], ar.PANEL_ROLL, 0.05)
    rep = got["history"][-1]["report"]
    assert rep["n_finite"] == r["report"]["n_finite"] == len(kept) and not r["out"].any()
    for key in ("q1", "q3", "med", "mc", "coef", "thr"):
        err = abs(rep[key] - r["report"][key]) / abs(r["report"][key])
        print(key, rep[key], r["report"][key], err)
        assert err <= 1e-8, key
    # and of the first iteration, whose outliers are the block
    first = np.sort(np.r_[kept, got["history"][0]["idx0"]])
    V = _svd(tpg.View(X, None, first + 1, code256=tpg.CODE_IMPUTE_PRED), ar.PANEL_K)["v"]
    r = ar.detect(V, ar.CHROM[first], ar.PANEL_ROLL, 0.05)
    assert np.array_equal(np.flatnonzero(r["out"]), got["history"][0]["pos0"])
    for key in ("q1", "q3", "med", "mc", "coef", "thr"):
        err = abs(got["history"][0]["report"][key] - r["report"][key]) / abs(r["report"][key])
        print(key, err)
        assert err <= 1e-8, key


def test_max_iter_zero_is_the_svd_of_the_clumped_set(planted):
    import tidypopgen_amd as tpg

    X, ref = planted["X"], planted["ref"]
    got = tpg.gt_pca_autoSVD(X, max_iter=0, **ARGS)
    clumped = np.sort(np.r_[ref["kept"], ref["history"][0]["idx0"]])
    assert got["converged"] is False and got["n_iter"] == 1 and got["history"] == [] and got["lrldr"] == []
    assert np.array_equal(got["loci"], clumped + 1)
    want = tpg.gt_pca_partialSVD(X, None, clumped + 1, k=ar.PANEL_K)
    for key in ("d", "u", "v", "center", "scale"):
        assert _same_bits(got[key], want[key]), key


def test_without_clumping_only_the_mac_filter_removes_loci(planted):
    import tidypopgen_amd as tpg

    got = tpg.gt_pca_autoSVD(planted["X"], **dict(ARGS, thr_r2=None))
    ref = ar.autosvd_ref(planted["G"], ar.CHROM, None, k=ar.PANEL_K, roll_size=ar.PANEL_ROLL)
    margin = min(float(np.min(np.abs(h["S2"] - h["report"]["thr"]) / h["report"]["thr"])) for h in ref["history"])
    assert margin >= 1e-4 and ref["history"][0]["n_kept"] == ar.M_PANEL - len(ar.LOW_MAC), margin
    assert got["history"][0]["n_kept"] == ar.M_PANEL - len(ar.LOW_MAC)
    assert np.array_equal(got["loci"], ref["kept"] + 1) and (got["n_iter"], got["converged"]) == (ref["n_iter"], ref["converged"])
    everything = tpg.gt_pca_autoSVD(planted["X"], **dict(ARGS, thr_r2=None, min_mac=0, max_iter=0))
    assert np.array_equal(everything["loci"], np.arange(1, ar.M_PANEL + 1))


def test_missing_genotypes_and_unordered_chromosomes_are_refused(planted):
    import tidypopgen_amd as tpg

    G = planted["G"].astype(np.uint8)
    G[17, 1234] = 3
    X = tpg.FBM.from_numpy(np.asfortranarray(G), code256=tpg.CODE_012)
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.gt_pca_autoSVD(X, **ARGS)
    assert e.value.code == 4  # TPG_ENUMERIC
    got = tpg.gt_pca_autoSVD(X, impute="mode", **ARGS)
    assert got["converged"] and not np.isin(ar.LOW_MAC + 1, got["loci"]).any()
    chrom = ar.CHROM.copy()
    chrom[-5:] = 1  # chromosome 1 comes back after 3
    for thr in (ar.PANEL_THR, None):
        with pytest.raises(tpg._lib.TpgError) as e:
            tpg.gt_pca_autoSVD(planted["X"], **dict(ARGS, chromosome=chrom, thr_r2=thr))
        assert e.value.code == 1  # TPG_EINVAL
    with pytest.raises(tpg._lib.TpgError, match="roll_size exceeds") as e:
        tpg.gt_pca_autoSVD(planted["X"], **dict(ARGS, roll_size=400))
    assert e.value.code == 1
