"""GPU: the pcadapt scan (include/tpg.h "pcadapt") against the numpy restatement tests/pcadapt_ref.py.

What is compared how.
  Medians and MADs (tpg_col_median_mad): bit for bit numpy.median of the finite entries (read as x + 0.0), over every row count
    around the workgroup's tile T = TPG_SELECT_TILE and every content class that steers the radix select.
  z-scores: every cell within the bound of the header, evaluated from the extended route (sums by math.fsum, the rest at 50
    digits); the NaN rows and n_valid equal.  beta and tot do not leave the device: they are held through z, whose bound carries
    the term of beta, and through the NaN rows (tot == 0 exactly for a monomorphic locus).
  OGK: with the device's own eigenvectors (`basis`) handed to the reference every other operation is stated, so dist, center and
    cov must agree to 4 K ulps per cell (observed: 0); each E is orthonormal and diagonalises the reference's R to 64 K eps.
    Against the reference with numpy's eigh the tolerance is 16 x the largest relative difference in dist between the
    reference's float route and its 50-digit route on the same Z, measured in the test.  Measured on the panel's z-scores
    (K = 2, eigengaps 0.014 / 0.011): 2.3e-15, bound used 3.6e-14, device against float 3.4e-15; hand-made K = 2: 4.4e-15,
    bound 7.0e-14, device 1.9e-15; hand-made K = 5 (eigengaps 0.058 / 0.034): 5.9e-13, bound 9.5e-12, device 6.2e-13.
  log10 p: |d| <= 1e-12 (1 + |log10 p|) against logq_ref; odd K far in the tail against mpmath.
  End to end (the planted panel, the reference fed the device's u): z within the per-cell bound; dist within tol = 16 x the
    largest relative difference between the reference's float pipeline and its 50-digit pipeline (z-scores and OGK) on that
    panel; gc_lambda within tol + 4 eps (a median of values each within tol moves by at most tol; one division); stat within
    2 tol + 4 eps; log10 p within stat * (2 tol + 4 eps) / (2 ln 10) + the 1e-12 contract (for K = 2 log Q = -x / 2, and for
    every K >= 2 the hazard of the chi-square is at most 1/2).  Measured: float against 50 digits 1.0e-14, tol 1.7e-13; device
    against float 1.4e-14 in dist, 3.4e-16 in gc_lambda, 1.4e-14 in stat, log10 p at 1 % of its bound."""
import math

import numpy as np
import pytest

from tests import pcadapt_ref as pr

pytestmark = pytest.mark.gpu

LOGQ_K, ODD_FAR, logq_points = pr.LOGQ_K, pr.ODD_FAR, pr.logq_points

LN10 = math.log(10.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _view(G, seed):
    """the panel as rows / columns of a larger store -> (X, v, rows, cols)"""
    import tidypopgen_amd as tpg

    n, m = G.shape
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.permutation(n + 3)[:n])
    cols = np.sort(rng.permutation(m + 5)[:m])
    big = rng.integers(0, 4, size=(n + 3, m + 5)).astype(np.uint8)
    big[np.ix_(rows, cols)] = G
    X = tpg.FBM.from_numpy(np.asfortranarray(big), code256=tpg.CODE_012)
    return X, tpg.View(X, rows + 1, cols + 1), rows + 1, cols + 1


# ---- tpg_col_median_mad -----------------------------------------------------------------------------------------------------
def _tile():
    from tidypopgen_amd import api

    return api.SELECT_TILE


def _content(kind, rows, rng):
    if kind == "equal":
        return np.full(rows, 3.25)
    if kind == "halves":  # the two middle values of an even count sit on both sides of zero
        x = np.concatenate([-rng.uniform(0.5, 2.0, rows // 2), rng.uniform(0.5, 2.0, rows - rows // 2)])
        return rng.permutation(x)
    if kind == "close":  # all keys share their high bytes
        return rng.permutation(1 + np.arange(rows) * 2.0 ** -40)
    if kind == "zeros":
        return rng.choice([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], size=rows)
    if kind == "subnormal":
        return rng.integers(-2000, 2000, size=rows) * 5e-324
    if kind == "huge":
        return rng.choice([1e300, -1e300], size=rows)
    if kind == "ties":
        return np.round(rng.standard_normal(rows))
    if kind == "nan":
        x = rng.standard_normal(rows)
        x[rng.random(rows) < 0.3] = np.nan
        x[rng.random(rows) < 0.05] = np.inf
        x[rng.random(rows) < 0.05] = -np.inf
        return x
    raise AssertionError(kind)


def _np_med_mad(x):
    f = x[np.isfinite(x)] + 0.0
    if len(f) == 0:
        return np.nan, np.nan, 0
    c0 = np.median(f)
    return c0, np.median(np.abs(f - c0)), len(f)


@pytest.mark.parametrize("kind", ["equal", "halves", "close", "zeros", "subnormal", "huge", "ties", "nan"])
def test_col_median_mad_is_numpys_median_bit_for_bit(kind):
    from tidypopgen_amd import api

    T = _tile()
    assert T >= 258
    rng = np.random.default_rng(sum(map(ord, kind)))
    for rows in (1, 2, 3, 4, 255, 256, 257, T, T + 1, 2 * T + 1):
        for ncols in (1, 2, 21):
            A = np.full((rows + 3, ncols), 7.0, order="F")  # ld > rows: the rows below are never read
            for k in range(ncols):
                A[:rows, k] = _content(kind, rows, rng)
            if kind == "nan" and ncols > 1:
                A[:rows, 1] = np.nan  # a column with no finite entry
            med, mad, cnt = api.col_median_mad(A[:rows, :], return_counts=True)
            want = [_np_med_mad(A[:rows, k]) for k in range(ncols)]
            assert _same_bits(med, [w[0] for w in want]), (kind, rows, ncols, med, want)
            assert _same_bits(mad, [w[1] for w in want]), (kind, rows, ncols, mad, want)
            assert cnt.tolist() == [w[2] for w in want]
            if kind == "equal":
                assert (mad == 0).all()


def test_col_median_mad_refuses_bad_shapes():
    import tidypopgen_amd as tpg
    from tidypopgen_amd import _lib, api

    ctx = tpg.default_context()
    x, out = np.zeros(4), np.zeros(1)
    for rows, ncols, ld in ((0, 1, 4), (4, 0, 4), (4, 1, 3)):
        assert _lib.lib.tpg_col_median_mad(ctx.h, api._ptr(x), rows, ncols, ld, api._ptr(out), api._ptr(out), None) == 1


# ---- tpg_pcadapt_zscores ----------------------------------------------------------------------------------------------------
def _genotypes(n, m, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, m)
    G = rng.binomial(2, p, size=(n, m)).astype(np.int64)
    if m >= 31:
        G[:, 3], G[:, 17] = 0, 2  # monomorphic: invalid
    return G


def _orthonormal(n, K, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, K)))
    return np.asfortranarray(q)


ZCASES = [(n, m, K) for n in (7, 33, 96) for m in (1, 31, 129, 1500) for K in (1, 4, 5, 21) if n - K - 1 >= 1]


@pytest.mark.parametrize("n,m,K", ZCASES)
def test_zscores_within_the_per_cell_bound(n, m, K):
    pytest.importorskip("mpmath")
    from tidypopgen_amd import api

    G = _genotypes(n, m, 100 * n + m + K)
    U = _orthonormal(n, K, n + K)
    _, v, _, _ = _view(G, n + m)
    z, nv = api.pcadapt_zscores(v, U, return_n_valid=True)
    b = pr.zscore_bounds(n, K, pr.zscores_ext(G, U))
    valid = ~np.isnan(b["z"]).any(axis=1)
    assert z.shape == (m, K) and nv == int(valid.sum())
    assert np.array_equal(np.isnan(z), np.repeat(~valid[:, None], K, axis=1))
    if m >= 31:
        assert not valid[3] and not valid[17]
    err = np.abs(z[valid] - b["z"][valid])
    assert (err <= b["dz"][valid]).all(), (err / b["dz"][valid]).max()
    # and the float route of the restatement, which carries the same bound against the exact value
    zr = pr.zscores_ref(G, U)["z"]
    assert (np.abs(z[valid] - zr[valid]) <= 2 * b["dz"][valid]).all()


def test_zscores_error_paths():
    import tidypopgen_amd as tpg
    from tidypopgen_amd import api

    n, m = 33, 40
    G = _genotypes(n, m, 9)
    U = _orthonormal(n, 4, 2)
    _, v, _, _ = _view(G, 3)
    Gm = G.copy()
    Gm[5, 11] = 3
    _, vm, _, _ = _view(Gm, 3)
    with pytest.raises(tpg._lib.TpgError) as e:
        api.pcadapt_zscores(vm, U)
    assert e.value.code == 4  # TPG_ENUMERIC
    Us = U.copy()
    Us[:, 2] *= 1.001
    for bad in (Us, np.zeros((n, 0)), _orthonormal(n, 4, 2)[:, :0], np.zeros((n, 65)), _orthonormal(n, n - 1, 1)):
        with pytest.raises(tpg._lib.TpgError) as e:
            api.pcadapt_zscores(v, np.asfortranarray(bad))
        assert e.value.code == 1, bad.shape  # TPG_EINVAL
    assert np.isfinite(api.pcadapt_zscores(v, U)).any()  # the view still serves


# ---- tpg_robust_dist_ogk ----------------------------------------------------------------------------------------------------
def _handmade(K, mv, seed, n_nan=5):
    """mv valid rows of correlated columns with distinct scales, n_nan invalid rows in between"""
    rng = np.random.default_rng(seed)
    mix = np.eye(K) + 0.35 * np.triu(np.ones((K, K)), 1) / np.arange(1, K + 1)
    Z = (rng.standard_normal((mv, K)) * (1.0 + 0.5 * np.arange(K))) @ mix
    Z[rng.integers(0, mv, size=max(1, mv // 50))] *= 6.0  # some outliers
    full = np.empty((mv + n_nan, K))
    bad = np.sort(rng.permutation(mv + n_nan)[:n_nan])
    ok = np.setdiff1d(np.arange(mv + n_nan), bad)
    full[ok] = Z
    full[bad] = rng.standard_normal((n_nan, K))
    for i, r in enumerate(bad):  # a NaN or an infinity somewhere in the row
        full[r, i % K] = [np.nan, np.inf, -np.inf][i % 3]
    return np.asfortranarray(full)


_PANEL = {}


def _panel():
    """the 96 x 1500 panel of the definition-level test, its view, the PCA of its polymorphic loci and the device's z-scores"""
    import tidypopgen_amd as tpg
    from tidypopgen_amd import api

    if not _PANEL:
        G = pr.panel(0)
        X, v, rows, cols = _view(G, 77)
        poly = np.array([j for j in range(G.shape[1]) if j not in pr.MONO])
        pca = tpg.gt_pca_partialSVD(X, rows, cols[poly], k=2, code256=tpg.CODE_012)
        z = api.pcadapt_zscores(v, pca["u"])
        _PANEL.update(G=G, X=X, v=v, rows=rows, cols=cols, pca=pca, z=z)
    return _PANEL


def _check_ogk_with_its_basis(Z, K):
    from tidypopgen_amd import api

    got = api.robust_dist_ogk(Z, return_basis=True)
    ref = pr.ogk_ref(Z, basis=got["basis"])
    eps = 2.0 ** -52
    for t in range(2):
        E, R = got["basis"][t], ref["R"][t]
        assert np.abs(E.T @ E - np.eye(K)).max() <= 64 * K * eps
        D = E.T @ R @ E
        assert np.abs(D - np.diag(np.diag(D))).max() <= 64 * K * eps * np.linalg.norm(R, 2)
    assert got["n_valid"] == ref["n_valid"]
    for name in ("dist", "center", "cov"):
        d = pr.ulp_diff(got[name], ref[name])
        assert d.max() <= 4 * K, (name, d.max())
    return got, ref


@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("mv", ["K+2", 300, 4097])
def test_ogk_reproduced_from_its_own_basis(K, mv):
    mv = K + 2 if mv == "K+2" else mv
    Z = _handmade(K, mv, 10 * K + mv % 7, n_nan=0 if mv == K + 2 else 5)
    got, _ = _check_ogk_with_its_basis(Z, K)
    assert np.array_equal(np.isnan(got["dist"]), ~np.isfinite(Z).all(axis=1))


def test_ogk_on_the_device_zscores_reproduced_from_its_own_basis():
    _check_ogk_with_its_basis(_panel()["z"], 2)


@pytest.mark.parametrize("which", ["panel", "hand2", "hand5"])
def test_ogk_against_numpys_eigh(which):
    pytest.importorskip("mpmath")
    from tidypopgen_amd import api

    Z = {"panel": lambda: _panel()["z"], "hand2": lambda: _handmade(2, 300, 41), "hand5": lambda: _handmade(5, 300, 42)}[which]()
    ref = pr.ogk_ref(Z)
    assert min(ref["gaps"]) >= 1e-2, ref["gaps"]  # the condition under which two eigen solvers may be compared
    ext = pr.ogk_ext(Z)
    ok = np.isfinite(ref["dist"])
    measured = float((np.abs(ref["dist"][ok] - ext[ok]) / ext[ok]).max())
    tol = 16 * measured
    got = api.robust_dist_ogk(Z)
    rel = float((np.abs(got["dist"][ok] - ref["dist"][ok]) / ref["dist"][ok]).max())
    print(f"ogk vs eigh [{which}]: float-vs-50-digit {measured:.3g}, bound {tol:.3g}, device-vs-float {rel:.3g}")
    assert rel <= tol, (rel, tol)
    assert np.isnan(got["dist"][~ok]).all()


def test_ogk_refuses_degenerate_input():
    import tidypopgen_amd as tpg
    from tidypopgen_amd import api

    Z = _handmade(3, 300, 7)
    Zc = Z.copy()
    Zc[:, 1] = 2.5  # a constant column: sigma = 0
    with pytest.raises(tpg._lib.TpgError) as e:
        api.robust_dist_ogk(Zc)
    assert e.value.code == 4
    with pytest.raises(ValueError):
        pr.ogk_ref(Zc)
    Zs = _handmade(3, 4, 8, n_nan=3)  # M' = K + 1
    with pytest.raises(tpg._lib.TpgError) as e:
        api.robust_dist_ogk(Zs)
    assert e.value.code == 4


# ---- tpg_pchisq_log10_upper -------------------------------------------------------------------------------------------------
def test_pchisq_log10_upper_holds_its_contract():
    from tidypopgen_amd import api

    for K in LOGQ_K:
        xs = np.array(logq_points(K))
        got = api.pchisq_log10_upper(xs, K)
        want = np.array([pr.logq_ref(K, float(x)) for x in xs]) / LN10
        assert (np.abs(got - want) <= 1e-12 * (1 + np.abs(want))).all(), (K, got, want)
    got = api.pchisq_log10_upper(np.array([np.nan, -1.0, np.inf, 0.0]), 3)
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == -np.inf and got[3] == 0.0


def test_pchisq_log10_upper_far_in_the_tail():
    pytest.importorskip("mpmath")
    from tidypopgen_amd import api

    for K in LOGQ_K:
        xs = np.array(ODD_FAR)
        got = api.pchisq_log10_upper(xs, K)
        want = np.array([pr.logq_mp(K, float(x)) for x in xs]) / LN10
        assert np.isfinite(got).all() and (np.abs(got - want) <= 1e-12 * (1 + np.abs(want))).all(), (K, got, want)


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_scan_end_to_end_on_the_planted_panel():
    import tidypopgen_amd as tpg
    from tidypopgen_amd import api

    c = _panel()
    G, v, u = c["G"], c["v"], c["pca"]["u"]
    before = v.unpack().copy()
    # the staged calls, each against the reference fed the device's u
    z, nv = api.pcadapt_zscores(v, u, return_n_valid=True)
    assert nv == 1497 and np.isnan(z[sorted(pr.MONO)]).all()
    o = api.robust_dist_ogk(z)
    lam = np.median(o["dist"][np.isfinite(o["dist"])]) / api.qchisq_median(2)
    stat = o["dist"] / lam
    lp = api.pchisq_log10_upper(stat, 2)
    ok = np.isfinite(stat)
    want_lp = np.array([pr.logq_ref(2, float(x)) for x in stat[ok]]) / LN10
    assert (np.abs(lp[ok] - want_lp) <= 1e-12 * (1 + np.abs(want_lp))).all() and np.isnan(lp[~ok]).all()
    assert 0.9 <= lam <= 1.1
    # ... and the reference fed the device's u: z within its per-cell bound, dist / gc_lambda / stat / log10 p within the bounds
    # the file header derives from the reference's own float-versus-50-digit difference on this panel
    pytest.importorskip("mpmath")
    ref = pr.pcadapt_ref(G, u)
    x50 = pr.pcadapt_ext(G, u)
    b = pr.zscore_bounds(G.shape[0], 2, x50["ext"])
    valid = ~np.isnan(b["z"]).any(axis=1)
    assert np.array_equal(valid, ok) and np.array_equal(valid, ref["zs"]["valid"])
    assert (np.abs(z[valid] - b["z"][valid]) <= b["dz"][valid]).all()
    assert (np.abs(z[valid] - ref["z"][valid]) <= 2 * b["dz"][valid]).all()
    eps = 2.0 ** -52
    measured = float((np.abs(ref["dist"][ok] - x50["dist"][ok]) / x50["dist"][ok]).max())
    tol = 16 * measured
    rel_dist = float((np.abs(o["dist"][ok] - ref["dist"][ok]) / ref["dist"][ok]).max())
    rel_lam = abs(lam - ref["gc_lambda"]) / ref["gc_lambda"]
    rel_stat = float((np.abs(stat[ok] - ref["stat"][ok]) / ref["stat"][ok]).max())
    ref_lp = np.array([pr.logq_ref(2, float(x)) for x in ref["stat"][ok]]) / LN10
    lp_bound = ref["stat"][ok] * (2 * tol + 4 * eps) / (2 * LN10) + 1e-12 * (1 + np.abs(ref_lp))
    print(f"end to end: float-vs-50-digit {measured:.3g}, tol {tol:.3g}; device-vs-float dist {rel_dist:.3g}, gc_lambda {rel_lam:.3g}, "
          f"stat {rel_stat:.3g}, log10 p worst fraction of its bound {float((np.abs(lp[ok] - ref_lp) / lp_bound).max()):.3g}")
    assert rel_dist <= tol and np.isnan(o["dist"][~ok]).all() and np.isnan(ref["dist"][~ok]).all()
    assert rel_lam <= tol + 4 * eps
    assert rel_stat <= 2 * tol + 4 * eps
    assert (np.abs(lp[ok] - ref_lp) <= lp_bound).all()
    # the whole scan in one call: bit for bit the staged calls
    one = api.pcadapt(v, u, return_zscores=True)
    assert _same_bits(one["zscores"], z) and _same_bits(one["dist"], o["dist"]) and _same_bits(one["stat"], stat)
    assert _same_bits(one["log10_p"], lp) and _bits(one["gc_lambda"]) == _bits(lam) and one["n_valid"] == nv
    # the public entry: the 15 largest scores are the planted loci
    r = tpg.gt_pcadapt(c["X"], c["pca"], 2, c["rows"], c["cols"])
    assert _same_bits(r["score"], stat) and _same_bits(r["log10_p"], lp) and r["gc_lambda"] == lam and r["n_valid"] == nv
    top = np.argsort(-np.nan_to_num(r["score"], nan=-1.0))[:15]
    assert sorted(top.tolist()) == pr.PLANTED.tolist()
    assert np.allclose(r["p"][ok], 10.0 ** lp[ok], rtol=1e-15, atol=0)
    assert np.array_equal(v.unpack(), before)  # the view is unchanged
    # k as the reference demands it
    for bad in ([1, 2], 3, 0, 1.5):
        with pytest.raises(ValueError):
            tpg.gt_pcadapt(c["X"], c["pca"], bad, c["rows"], c["cols"])


def test_scan_with_missing_genotypes_needs_imputation():
    import tidypopgen_amd as tpg

    G = pr.panel(0)
    poly = np.array([j for j in range(G.shape[1]) if j not in pr.MONO])
    Gm = G[:, poly].copy()
    rng = np.random.default_rng(12)
    Gm[rng.random(Gm.shape) < 0.02] = 3
    X, _, rows, cols = _view(Gm, 78)
    pca = tpg.gt_pca_partialSVD(X, rows, cols, k=2, code256=tpg.CODE_012, impute="mode")
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.gt_pcadapt(X, pca, 2, rows, cols)
    assert e.value.code == 4
    r = tpg.gt_pcadapt(X, pca, 2, rows, cols, impute="mode", return_zscores=True)
    assert r["zscores"].shape == (Gm.shape[1], 2) and np.isfinite(r["score"]).sum() == r["n_valid"] > 0
    assert r["gc_lambda"] > 0 and (r["log10_p"][np.isfinite(r["score"])] <= 0).all()
