"""GPU: PCA by operator products (csrc/pcaop.hip; include/tpg.h "PCA by operator products").

The two halves W = Z'Q and Y = Z W on int8 MFMA against the exact route of tests/pcaop_ref.py within its DERIVED bounds,
their composition against numpy's FP64, and the Gram-free truncated SVD (tpg_pca_random_svd_op,
gt_pca_randomSVD(route="operator")) against numpy's SVD and the Gram route.  Shapes: partial row tiles, one and two
128-wide chunks of the contraction (so fewer chunks than the split would like), chunk edges; block widths 1, 5, 6, 22, 64 =
6, 30, 36, 132, 384 int8 columns (inside one column tile, two tiles, a 4 + 1 launch split, three full launches).
tests/test_pcaop_host.py shows on the same inputs that the bounds hold for the model and fail for a model with one digit
fewer or with one exponent for the whole block."""
import ctypes as C

import numpy as np
import pytest

from tests import pcaop_ref as ref

pytestmark = pytest.mark.gpu

EINVAL, ENUMERIC = 1, 4
FLOOR = 1e-8


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


_PANELS = {}


def _panel(tpg, shape, seed=None, npop=3):
    """(G, FBM, columns, view, center, scale) of a panel without missing values, monomorphic loci dropped"""
    key = (shape, seed, npop)
    if key not in _PANELS:
        from oracle import oracle as orc

        n, m = shape
        seed = 31 + n if seed is None else seed
        fbm = orc.synth_fbm(seed, n, m, npop=npop, miss=0.0)
        keep = np.where((fbm.sum(axis=0) > 0) & (fbm.sum(axis=0) < 2 * n))[0]
        G = fbm[:, keep].astype(np.int64)  # (what ref.panel returns)
        cols = (keep + 1).astype(np.int32)
        X = tpg.FBM.from_numpy(fbm)
        v = tpg.View(X, None, cols, code256=tpg.CODE_IMPUTE_PRED)
        center, scale = tpg.pca_center_scale(v)
        assert np.array_equal(center, ref.center_scale(G)[0])
        G.setflags(write=False)
        _PANELS[key] = (G, X, cols, v, center, scale)
    return _PANELS[key]


def _check_halves(tpg, shape, b, kind):
    G, _, _, v, center, scale = _panel(tpg, shape)
    n, m = G.shape
    Q = ref.operand(kind, n, b, 7)
    W = tpg.pca_zt_prod(v, center, scale, Q)
    assert W.shape == (m, b)
    ezt = np.abs(W - ref.exact_zt(G, center, scale, Q))
    bzt = ref.bound_zt(G, center, scale, Q)
    print(f"zt {shape} b={b} {kind}: worst error / bound {np.max(ezt / np.where(bzt > 0, bzt, 1)):.3f}")
    assert np.all(ezt <= bzt)
    assert np.array_equal(W, ref.model_zt(G, center, scale, Q))  # the model restates the device step by step: the same bits
    Win = ref.operand(kind, m, b, 8)
    Y = tpg.pca_z_prod(v, center, scale, Win)
    assert Y.shape == (n, b)
    ez = np.abs(Y - ref.exact_z(G, center, scale, Win))
    bz = ref.bound_z(G, center, scale, Win)
    print(f"z  {shape} b={b} {kind}: worst error / bound {np.max(ez / np.where(bz > 0, bz, 1)):.3f}")
    assert np.all(ez <= bz)
    assert np.array_equal(Y, ref.model_z(G, center, scale, Win))
    return Q, W, Win, Y


@pytest.mark.parametrize("b", ref.BS)
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_halves_against_the_exact_route(tpg, shape, b):
    _check_halves(tpg, shape, b, "normal")


@pytest.mark.parametrize("shape", ((33, 130), (200, 1000)))
def test_two_magnitudes_keep_their_own_exponents(tpg, shape):
    # columns of magnitude 1 and 1e-7 in one block: the bound of a weak column is 1e-7 times its neighbour's, and a
    # common exponent misses it by 2^23 (tests/test_pcaop_host.py)
    for b in (2, 6):
        _check_halves(tpg, shape, b, "two_mag")


@pytest.mark.parametrize("shape", ((33, 130), (200, 1000)))
def test_a_zero_column_gives_exact_zeros(tpg, shape):
    for b in (1, 6):
        G, _, _, v, center, scale = _panel(tpg, shape)
        n, m = G.shape
        if b == 1:
            assert np.all(tpg.pca_zt_prod(v, center, scale, np.zeros((n, 1))) == 0)
            assert np.all(tpg.pca_z_prod(v, center, scale, np.zeros((m, 1))) == 0)
            continue
        _, W, _, Y = _check_halves(tpg, shape, b, "zero_col")
        assert np.all(W[:, b // 2] == 0) and np.all(Y[:, b // 2] == 0)
        assert np.all(np.isfinite(W)) and np.all(np.isfinite(Y))


@pytest.mark.parametrize("shape", ((33, 130), (200, 1000)))
def test_a_negative_only_column(tpg, shape):
    Q, _, Win, _ = _check_halves(tpg, shape, 6, "neg_col")
    assert np.all(Q[:, 0] < 0) and np.all(Win[:, 0] < 0)


def test_a_column_that_is_not_finite_is_nan_and_alone(tpg):
    G, _, _, v, center, scale = _panel(tpg, (129, 257))
    n, m = G.shape
    Q = ref.operand("normal", n, 3, 7)
    good = tpg.pca_zt_prod(v, center, scale, Q)
    Q[5, 1] = np.nan
    W = tpg.pca_zt_prod(v, center, scale, Q)
    assert np.all(np.isnan(W[:, 1])) and np.array_equal(W[:, [0, 2]], good[:, [0, 2]])
    Win = ref.operand("normal", m, 3, 8)
    good = tpg.pca_z_prod(v, center, scale, Win)
    Win[9, 2] = np.inf
    Y = tpg.pca_z_prod(v, center, scale, Win)
    assert np.all(np.isnan(Y[:, 2])) and np.array_equal(Y[:, :2], good[:, :2])


@pytest.mark.parametrize("shape,b", [((33, 130), 5), ((129, 257), 22), ((200, 1000), 64)])
def test_composition_against_numpy(tpg, shape, b):
    G, _, _, v, center, scale = _panel(tpg, shape)
    Q = ref.operand("normal", G.shape[0], b, 11)
    W = tpg.pca_zt_prod(v, center, scale, Q)
    Y = tpg.pca_z_prod(v, center, scale, W)
    Z = ref.scaled(G, center, scale)
    err = np.abs(Y - Z @ (Z.T @ Q))
    bound = ref.bound_apply(G, center, scale, Q, W)
    print(f"composition {shape} b={b}: worst error / bound {np.max(err / bound):.3f}, relative error in norm "
          f"{np.linalg.norm(err) / np.linalg.norm(Z @ (Z.T @ Q)):.3e}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("shape,b", [((129, 257), 22), ((200, 1000), 64)])
def test_a_half_twice_gives_the_same_bits(tpg, shape, b):
    G, _, _, v, center, scale = _panel(tpg, shape)
    n, m = G.shape
    Q, Win = ref.operand("normal", n, b, 7), ref.operand("normal", m, b, 8)
    assert tpg.pca_zt_prod(v, center, scale, Q).tobytes() == tpg.pca_zt_prod(v, center, scale, Q).tobytes()
    assert tpg.pca_z_prod(v, center, scale, Win).tobytes() == tpg.pca_z_prod(v, center, scale, Win).tobytes()


def test_a_locus_major_view_gives_the_same_bits(tpg):
    # the second view of View.pair holds the LM layout alone when n is a multiple of 8: the operator builds L and T from it
    from oracle import oracle as orc

    n, m = 136, 289
    G, _ = ref.panel(5, n, m)
    X = tpg.FBM.from_numpy(orc.fbm_from_genotypes(G.astype(float)))
    v_rows, v_lm = tpg.View(X), tpg.View.pair(X)[1]
    center, scale = tpg.pca_center_scale(v_rows)
    Q, Win = ref.operand("normal", n, 6, 7), ref.operand("normal", G.shape[1], 6, 8)
    assert np.array_equal(tpg.pca_zt_prod(v_rows, center, scale, Q), tpg.pca_zt_prod(v_lm, center, scale, Q))
    assert np.array_equal(tpg.pca_z_prod(v_rows, center, scale, Win), tpg.pca_z_prod(v_lm, center, scale, Win))
    assert np.all(np.abs(tpg.pca_zt_prod(v_lm, center, scale, Q) - ref.exact_zt(G, center, scale, Q))
                  <= ref.bound_zt(G, center, scale, Q))


# ---------------------------------------------------------------------------------------------------------------------
# the SVD
@pytest.fixture(scope="module")
def svd_panel(tpg):
    """the panel of test_gt_pca_randomSVD_tolerance (300 x 4 000, six populations), numpy's SVD of it, the Gram route"""
    n, m, k = 300, 4000, 8
    G, X, cols, v, center, scale = _panel(tpg, (n, m), seed=77, npop=6)
    Z = ref.scaled(G, center, scale)
    Un, sn, _ = np.linalg.svd(Z, full_matrices=False)
    gram = tpg.gt_pca_partialSVD(X, None, cols, k=k)
    return dict(G=G, X=X, cols=cols, v=v, center=center, scale=scale, Z=Z, lam=sn ** 2, Un=Un, gram=gram, k=k)


@pytest.mark.parametrize("tol", (1e-4, FLOOR))
def test_svd_by_operator_products(tpg, svd_panel, tol):
    p = svd_panel
    G, Z, lam, k = p["G"], p["Z"], p["lam"], p["k"]
    r = tpg.gt_pca_randomSVD(p["X"], None, p["cols"], k=k, tol=tol, route="operator")
    assert r["method"] == "randomSVD" and r["route"] == "operator" and r["n_apply"] >= 2
    d, u = r["d"], r["u"]
    d1sq = d[0] ** 2
    E = np.array([ref.op_error_norm(G, p["center"], p["scale"], u[:, j]) for j in range(k)])  # the operator's error for u_j
    res = np.linalg.norm(Z @ (Z.T @ u) - u * d ** 2, axis=0)
    print(f"tol {tol:g}: n_apply {r['n_apply']}, residual / (tol d_1^2) {np.max(res / (tol * d1sq)):.3e}, E / d_1^2 {E.max() / d1sq:.3e}")
    assert np.all(res <= 1.001 * tol * d1sq + E)
    assert np.all(np.abs(d ** 2 - lam[:k]) <= tol * d1sq + E)
    assert np.abs(u.T @ u - np.eye(k)).max() <= 1e-9
    want_v = Z.T @ u / d
    assert np.abs(r["v"] - want_v).max() <= 1e-9 * np.abs(want_v).max()  # the bound of tests/test_gpu_loadings.py
    g = p["gram"]
    assert r["square_frobenius"] == g["square_frobenius"]
    assert np.array_equal(r["center"], g["center"]) and np.array_equal(r["scale"], g["scale"])
    # six populations: five structured directions, then the bulk
    gap = lam[4] - lam[5]
    sine_bound = (tol * d1sq + E.max()) / gap
    if tol == 1e-4:
        assert sine_bound < 1e-2
    cosines = np.linalg.svd(g["u"][:, :5].T @ u[:, :5], compute_uv=False)
    # sin of the largest principal angle, from the part of one basis outside the other (accurate for small angles)
    sine = np.linalg.norm(u[:, :5] - g["u"][:, :5] @ (g["u"][:, :5].T @ u[:, :5]), 2)
    print(f"tol {tol:g}: sine of the leading subspaces {sine:.3e} (bound {sine_bound:.3e}), smallest cosine {cosines.min():.12f}")
    assert sine <= sine_bound


def test_svd_operator_is_a_function_of_the_view(tpg, svd_panel):
    p = svd_panel
    a = tpg.gt_pca_randomSVD(p["X"], None, p["cols"], k=3, tol=1e-4, route="operator")
    b = tpg.gt_pca_randomSVD(p["X"], None, p["cols"], k=3, tol=1e-4, route="operator")
    assert a["n_apply"] == b["n_apply"]
    for key in ("d", "u", "v"):
        assert a[key].tobytes() == b[key].tobytes()


def test_tall_panel(tpg):
    n, m, k, tol = 40000, 384, 4, 1e-4
    G, X, cols, v, center, scale = _panel(tpg, (n, m), seed=5, npop=5)
    r = tpg.gt_pca_randomSVD(X, None, cols, k=k, tol=tol, route="operator")
    assert r["route"] == "operator"
    Z = ref.scaled(G, center, scale)
    lam = np.linalg.svd(Z, compute_uv=False)[:k] ** 2
    d1sq = r["d"][0] ** 2
    E = max(ref.op_error_norm(G, center, scale, r["u"][:, j]) for j in range(k))
    print(f"tall: n_apply {r['n_apply']}, |d^2 - lambda| / d_1^2 {np.max(np.abs(r['d'] ** 2 - lam)) / d1sq:.3e}, E / d_1^2 {E / d1sq:.3e}")
    assert np.all(np.abs(r["d"] ** 2 - lam) <= tol * d1sq + E)
    assert np.abs(r["u"].T @ r["u"] - np.eye(k)).max() <= 1e-9
    assert tpg.pca_op_scratch_bytes(n, m, k) < 8 * n * n / 50


def test_scratch_is_linear():
    import tidypopgen_amd as t

    pad = 64 << 20  # tile padding and the fixed small blocks
    for n, m, k in ((40000, 384, 4), (5000, 1000000, 20), (100000, 100000, 10), (3000, 3000, 52), (1 << 20, 1 << 17, 8)):
        base = t.pca_op_scratch_bytes(n, m, k)
        assert base > 0
        assert t.pca_op_scratch_bytes(2 * n, m, k) <= 2 * base + pad, (n, m, k)
        assert t.pca_op_scratch_bytes(n, 2 * m, k) <= 2 * base + pad, (n, m, k)
    assert t.pca_op_scratch_bytes(1000, 1000, 53) == 0 and t.pca_op_scratch_bytes(0, 10, 1) == 0


# ---------------------------------------------------------------------------------------------------------------------
# errors and routes
def _svd_op_rc(tpg, v, k, tol):
    lib = tpg._lib.lib
    d, u, vl = np.zeros(k), np.zeros((v.n, k), order="F"), np.zeros((v.m, k), order="F")
    center, scale = np.zeros(v.m), np.zeros(v.m)
    napp = C.c_int()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return lib.tpg_pca_random_svd_op(v.ctx.h, v.h, k, tol, ptr(d), ptr(u), ptr(vl), ptr(center), ptr(scale), None, C.byref(napp))


def test_errors(tpg, svd_panel):
    p = svd_panel
    v, lib = p["v"], tpg._lib.lib
    assert _svd_op_rc(tpg, v, 53, 1e-4) == EINVAL and b"Gram route" in lib.tpg_last_error()
    for tol in (FLOOR / 10, 0.0, 1.0):
        assert _svd_op_rc(tpg, v, 4, tol) == EINVAL, tol
    assert _svd_op_rc(tpg, v, 4, FLOOR) == 0
    center, scale = p["center"], p["scale"]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for b in (0, 65):
        Q, W = np.zeros((v.n, max(b, 1)), order="F"), np.zeros((v.m, max(b, 1)), order="F")
        assert lib.tpg_pca_zt_prod(v.ctx.h, v.h, ptr(center), ptr(scale), ptr(Q), b, ptr(W)) == EINVAL
        assert lib.tpg_pca_z_prod(v.ctx.h, v.h, ptr(center), ptr(scale), ptr(W), b, ptr(Q)) == EINVAL
    with pytest.raises(ValueError):
        tpg.gt_pca_randomSVD(p["X"], None, p["cols"], k=4, route="bogus")
    with pytest.raises(ValueError):
        tpg.pca_zt_prod(v, center, scale, np.zeros((v.n + 1, 2)))


def test_a_missing_genotype_is_refused(tpg):
    from oracle import oracle as orc

    G, _ = ref.panel(31 + 129, 129, 257)
    g = G.astype(float)
    g[17, 40] = np.nan
    X = tpg.FBM.from_numpy(orc.fbm_from_genotypes(g))
    v = tpg.View(X)
    center, scale = ref.center_scale(G)
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.pca_zt_prod(v, center, scale, np.ones((v.n, 2)))
    assert e.value.code == ENUMERIC
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.pca_z_prod(v, center, scale, np.ones((v.m, 2)))
    assert e.value.code == ENUMERIC
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.gt_pca_randomSVD(X, k=3, route="operator", code256=tpg.CODE_012)
    assert e.value.code == ENUMERIC
    scale0 = scale.copy()
    scale0[3] = 0.0
    v_ok = tpg.View(tpg.FBM.from_numpy(orc.fbm_from_genotypes(G.astype(float))))
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.pca_z_prod(v_ok, center, scale0, np.ones((v_ok.m, 2)))
    assert e.value.code == ENUMERIC


def test_routes(tpg, svd_panel):
    p = svd_panel
    today = tpg.gt_pca_randomSVD(p["X"], None, p["cols"], k=p["k"], tol=1e-6)
    gram = tpg.gt_pca_randomSVD(p["X"], None, p["cols"], k=p["k"], tol=1e-6, route="gram")
    assert today["route"] == gram["route"] == "gram" and "n_apply" not in gram
    for key in ("d", "u", "v", "center", "scale"):
        assert today[key].tobytes() == gram[key].tobytes(), key
    assert today["square_frobenius"] == gram["square_frobenius"]
    auto = tpg.gt_pca_randomSVD(p["X"], None, p["cols"], k=p["k"], tol=1e-6, route="auto")
    assert auto["route"] == "gram"
    for key in ("d", "u", "v"):
        assert auto[key].tobytes() == gram[key].tobytes(), key
