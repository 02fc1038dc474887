"""GPU: the FP64 sweeps of csrc/pca.hip (tpg_sweep_kernel<KC, MODE>, run_sweep, tpg_sweep_reduce_kernel) bit for bit.

On the exact panels of tests/sweep_ref.py every partial sum is a double, so the device must return sweep_exact() in every bit
whatever the order it adds in: np.array_equal, no tolerance (the argument is in sweep_ref's docstring, shown on the host and
armed against sweep_ref's fault models by tests/test_sweep_host.py).  The general panels are held to the derived sweep_bound().

Launch arms through K: 1 and 4 (KC = 4, first and last), 5 and 20 (KC = 20, one pass), 21 = 20 + 1, 40 = 20 + 20,
41 = 20 + 20 + 1, 64 = three passes and one of kc = 4.  Shapes and their split counts S, derived for 256 CUs (4 * 256 = 1024 row
blocks fill the chip; S doubles while ceil(nrowtiles / 4) S < 1024, 2 S <= nblocks and S < 64):
  T layout (COLSCALE, VALID), nrowtiles = 4 ceil(n / 128), nblocks = ceil(m / 128):
    (1, 1) (31, 127) (32, 128): one block, S = 1;  (33, 129) (129, 130): two blocks, S = 2;  (130, 769): seven blocks (768 is
    six), S = 4 cut 1 / 2 / 2 / 2;  (130, 767): the six blocks cut 1 / 2 / 1 / 2;  (260, 1153): ten blocks, S = 8;  (130, 12805):
    101 blocks, S = 64, ranges of one and of two blocks.
  L layout (ROWSCALE), nrowtiles = 4 ceil(m / 128), nblocks = ceil(n / 128):
    (5, 40) (128, 129): S = 1;  (130, 257) (136, 289): S = 2;  (643, 300): six blocks, S = 4 cut 1 / 2 / 1 / 2.
The binding does not expose the context's CU count, so S is not asserted here (tests/test_sweep_host.py checks the table against
the restated rule); on another CU count every test still holds the kernel to the same reference, through other splits.
Every shape runs K = 4 and K = 21; every K runs on a shape with S > 1 and on a ragged one (sweep_ref.T_CASES / L_CASES).

Entry points: tpg.fbm256_prod_and_rowSumsSq (COLSCALE: XV and rss), tpg_fbm256_valid_prod through ctypes as predict_gt_pca calls
it (VALID), tpg.pca_loadings on views WITH missing genotypes (ROWSCALE with col_div: the fallback of the MFMA digit route, for
View(X) and for the locus-major member of View.pair), predict_gt_pca(project_method = "least_squares") end to end.
The RAW mode runs only with K = 1, behind tpg_pca_gram with a general center:
test_pca_gram_weight_classes_general_center_and_scale (tests/test_gpu_parity.py) covers it.
"""
import ctypes as C

import numpy as np
import pytest

from tests import sweep_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


_stores, _exact = {}, {}


def _store(tpg, kind, n, m, miss=sr.MISS):
    """(panel, FBM of its codes as bytes: 3 reads as missing through CODE_012 and through CODE_IMPUTE_PRED), once per module"""
    key = (kind, n, m, miss)
    if key not in _stores:
        p = sr.panel(kind, n, m, miss)
        _stores[key] = (p, tpg.FBM.from_numpy(np.asfortranarray(p.G)))
    return _stores[key]


def _want(mode, n, m, K, miss=sr.MISS):
    """sweep_exact at KMAX columns once per (mode, shape): a column's sum does not depend on K"""
    key = (mode, n, m, miss)
    if key not in _exact:
        _exact[key] = sr.sweep_exact(mode, *sr.panel("exact", n, m, miss).args(mode, sr.KMAX))
    out, rss = _exact[key]
    return out[:, :K], rss


def _valid_prod(v, tab):
    from tidypopgen_amd.api import _ptr, check, lib

    tab = np.asfortranarray(tab, dtype=float)
    out = np.zeros((v.n, tab.shape[1]), order="F")
    check(lib.tpg_fbm256_valid_prod(v.ctx.h, v.h, _ptr(tab), tab.shape[1], _ptr(out)))
    return out


def _where(got, want):
    """the first differing element, for the message: (row, column = k, got, want)"""
    bad = np.argwhere(got != want)
    return None if len(bad) == 0 else (tuple(bad[0]), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]), len(bad))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,K", sr.T_CASES)
def test_colscale_bit_for_bit(tpg, n, m, K):
    p, X = _store(tpg, "exact", n, m)
    _, center, scale, V, _ = p.args("colscale", K)
    XV, rss = tpg.fbm256_prod_and_rowSumsSq(X, None, None, center, scale, V, code256=tpg.CODE_012)
    want, want_rss = _want("colscale", n, m, K)
    assert np.array_equal(XV, want), _where(XV, want)
    assert np.array_equal(rss, want_rss), _where(rss, want_rss)


@pytest.mark.parametrize("K", [4, 21])
def test_colscale_subset_of_a_larger_store(tpg, K):
    """a row subset and a scattered column subset (1-based, out of order) of the (260, 1153) store: 131 x 770, S = 4"""
    p, X = _store(tpg, "exact", 260, 1153)
    rng = np.random.default_rng(3)
    nowhere_row, nowhere_col = 260 // 2, 1153 // 3
    rows = np.concatenate([[nowhere_row], np.sort(rng.choice(np.delete(np.arange(260), nowhere_row), 130, replace=False))])
    cols = rng.choice(np.delete(np.arange(1153), nowhere_col), 770, replace=False)
    cols[-2] = nowhere_col  # the column typed nowhere, next to the last column of the view
    V = np.asfortranarray(p.V[-770:, :K])  # (the table belongs to the view's columns: its last row is the odd one out)
    XV, rss = tpg.fbm256_prod_and_rowSumsSq(X, rows + 1, cols + 1, p.center[cols], p.scale[cols], V, code256=tpg.CODE_012)
    want, want_rss = sr.sweep_exact("colscale", p.G[np.ix_(rows, cols)], p.center[cols], p.scale[cols], V)
    assert np.all(want[0] == 0) and want_rss[0] == 0 and np.abs(want[1:]).max(axis=1).min() > 0
    assert np.array_equal(XV, want), _where(XV, want)
    assert np.array_equal(rss, want_rss), _where(rss, want_rss)


@pytest.mark.parametrize("n,m,K", sr.T_CASES)
def test_valid_bit_for_bit(tpg, n, m, K):
    p, X = _store(tpg, "exact", n, m)
    got = _valid_prod(tpg.View(X, code256=tpg.CODE_012), p.V[:, :K])
    want, _ = _want("valid", n, m, K)
    assert np.array_equal(got, want), _where(got, want)


def test_valid_rows_typed_nowhere_and_everywhere(tpg):
    """a row typed nowhere gives zeros in every column; a row typed everywhere the plain column sums of Tab (41 columns: three
    passes; (130, 769): S = 4)"""
    n, m, K = 130, 769, 41
    p = sr.panel("exact", n, m)
    G = p.G.copy()
    G[1] = np.where(G[1] == 3, 1, G[1])
    assert (G[n // 2] == 3).all() and not (G[1] == 3).any()
    got = _valid_prod(tpg.View(tpg.FBM.from_numpy(np.asfortranarray(G)), code256=tpg.CODE_012), p.V[:, :K])
    want, _ = sr.sweep_exact("valid", G, None, None, np.asfortranarray(p.V[:, :K]))
    assert np.array_equal(got, want), _where(got, want)
    assert np.all(got[n // 2] == 0) and np.array_equal(got[1], p.V[:, :K].sum(axis=0))


# ---------------------------------------------------------------------------------------------------------------------
def _loadings_views(tpg, n, m, miss=sr.MISS):
    p, X = _store(tpg, "exact", n, m, miss)
    views = [("rows", tpg.View(X))]
    if n % 8 == 0:  # the fast pack kernel writes the pair's second member locus-major
        views.append(("locus_major", tpg.View.pair(X)[1]))
    return p, views


@pytest.mark.parametrize("n,m,K", sr.L_CASES)
def test_pca_loadings_missing_genotypes_bit_for_bit(tpg, n, m, K):
    """tpg.pca_loadings on a view with missing genotypes: the FP64 ROWSCALE sweep with col_div = d.  `center` is a multiple of 1/4
    drawn at random, not the column mean: the arm accepts any center."""
    p, views = _loadings_views(tpg, n, m)
    G, center, scale, U, d = p.args("rowscale", K)
    assert (G == 3).any() and not np.array_equal(center, np.where(G == 3, 0, G).sum(0) / n)
    want, _ = _want("rowscale", n, m, K)
    got = {}
    for name, v in views:
        got[name] = tpg.pca_loadings(v, center, scale, U, d)
        assert np.array_equal(got[name], want), (name, _where(got[name], want))
    if (n, m) == (136, 289):
        assert np.array_equal(got["rows"], got["locus_major"])  # the two layouts, bit for bit


@pytest.mark.parametrize("K", [4, 21])
def test_pca_loadings_seam_between_the_two_routes(tpg, K):
    """the same call on a panel with NO missing genotype goes the MFMA digit route: within the suite's 1e-9-of-max bound of the
    exact value (test_gpu_loadings.py); one genotype set to missing sends it back to the sweep, bit for bit."""
    n, m = 136, 289
    p, views = _loadings_views(tpg, n, m, miss=0.0)
    G, center, scale, U, d = p.args("rowscale", K)
    assert not (G == 3).any() and len(views) == 2
    want, _ = _want("rowscale", n, m, K, miss=0.0)
    for name, v in views:
        got = tpg.pca_loadings(v, center, scale, U, d)
        err = float(np.abs(got - want).max() / np.abs(want).max())
        assert err <= 1e-9, (name, K, err)
    G1 = G.copy()
    G1[int(np.argmax(np.abs(G[:, m - 1] - center[m - 1]))), m - 1] = 3  # (a genotype whose z is not 0: the sums change)
    X1 = tpg.FBM.from_numpy(np.asfortranarray(G1))
    want1, _ = sr.sweep_exact("rowscale", G1, center, scale, U, d)
    assert not np.array_equal(want1, want)
    for v in (tpg.View(X1), tpg.View.pair(X1)[1]):
        got = tpg.pca_loadings(v, center, scale, U, d)
        assert np.array_equal(got, want1), _where(got, want1)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sr.MODES)
def test_general_values_inside_the_derived_bound(tpg, mode):
    """real center / scale, Gaussian Tab, d from linspace; ragged, S = 2, K = 21: |device - rational reference| <=
    (N + 8) 2^-53 sum |z t|, elementwise (sweep_ref.sweep_bound: derived from the arithmetic, nothing measured)"""
    n, m = sr.GENERAL[mode]
    p, X = _store(tpg, "general", n, m)
    G, center, scale, Tab, d = args = p.args(mode, 21)
    if mode == "colscale":
        got = tpg.fbm256_prod_and_rowSumsSq(X, None, None, center, scale, Tab, code256=tpg.CODE_012)
    elif mode == "valid":
        got = (_valid_prod(tpg.View(X, code256=tpg.CODE_012), Tab), None)
    else:
        got = (tpg.pca_loadings(tpg.View(X), center, scale, Tab, d), None)
    worst = sr.excess(got, sr.sweep_fraction(mode, *args), sr.sweep_bound(mode, *args))
    print(f"sweep general {mode}: worst |err| / bound = {worst:.3g}")
    assert worst <= 1.0, (mode, worst)


# ---------------------------------------------------------------------------------------------------------------------
def test_predict_least_squares_device_sums_are_exact(tpg, monkeypatch):
    """predict_gt_pca(project_method = "least_squares") on an exact panel: the right-hand sides (COLSCALE sweep) and the masked
    normal equations (VALID sweep over the pairwise products of the loadings) the device hands back equal the integer sums; the
    solve after them is host numpy and held to numpy."""
    from tidypopgen_amd import api

    n, m = 130, 769
    p = sr.panel("exact", n, m)
    lsq = (2, 5, 7)
    rng = np.random.default_rng(11)
    v = np.asfortranarray(rng.integers(-512, 513, (m, 8)).astype(np.float64))  # products of two columns stay below 2^20
    pca = {"v": v, "center": p.center, "scale": p.scale}
    seen = {}
    real_prod = api._prod_and_rss

    def prod(*a, **k):
        seen["rhs"] = real_prod(*a, **k)[0]
        return seen["rhs"], None

    class Lib:
        def __getattr__(self, name):
            return getattr(api._lib.lib, name)

        def tpg_fbm256_valid_prod(self, ctx, view, tab, K, out):
            rc = api._lib.lib.tpg_fbm256_valid_prod(ctx, view, tab, K, out)
            seen["masked"] = np.ctypeslib.as_array((C.c_double * (n * K)).from_address(out.value)).reshape((n, K), order="F").copy()
            return rc

    monkeypatch.setattr(api, "_prod_and_rss", prod)
    monkeypatch.setattr(api, "lib", Lib())
    G = p.G.copy()
    G[n // 2, ::2] = 1  # (a row typed nowhere has no normal equations to solve)
    Xs = tpg.FBM.from_numpy(np.asfortranarray(G))
    got = tpg.predict_gt_pca(pca, Xs, project_method="least_squares", lsq_pcs=lsq, code256=tpg.CODE_012)
    Vs = np.asfortranarray(v[:, [a - 1 for a in lsq]])
    pairs = [(a, b) for a in range(3) for b in range(a, 3)]
    tab = np.asfortranarray(np.stack([Vs[:, a] * Vs[:, b] for a, b in pairs], axis=1))
    rhs, _ = sr.sweep_exact("colscale", G, p.center, p.scale, Vs)
    masked, _ = sr.sweep_exact("valid", G, None, None, tab)
    assert np.array_equal(seen["rhs"], rhs), _where(seen["rhs"], rhs)
    assert np.array_equal(seen["masked"], masked), _where(seen["masked"], masked)
    want = np.zeros((n, 3))
    for i in range(n):
        A = np.zeros((3, 3))
        for (a, b), val in zip(pairs, masked[i]):
            A[a, b] = A[b, a] = val
        want[i] = np.linalg.solve(A, rhs[i])
    assert np.allclose(got, want, rtol=1e-12, atol=0)
