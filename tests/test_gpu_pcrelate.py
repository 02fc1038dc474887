"""GPU: pcrelate_coef, pcrelate_isaf, pcrelate_gram, pcrelate and gt_pcrelate (include/tpg.h "PC-Relate") against the numpy
restatement and the extended-precision route of tests/pcrelate_ref.py.

What is compared how.  The basis is the restatement's bit for bit.  mean is exact, c is held to its elementwise bound against the
long-double sums.  Given the DEVICE's mean and c, mu and valid are bit for bit the pinned loop's.  Cnt is exact; Num and Den are
held cell by cell to (m + 4) eps sum |R R| and (m + 8) eps sum S S against the long-double Grams of the very mu the device used
(times REF_SLACK for the reference's own error).  The whole call is bit for bit the staged calls, twice; kin and f carry the
NaN pattern of the exact route and lie within the propagated bound."""
import numpy as np
import pytest

from tests import pcrelate_ref as pr

pytestmark = pytest.mark.gpu

EINVAL = 1
B = 1024  # csrc/pcrelate.hip: the operand block for these n (tpg_pcrelate_block_loci; checked below)

# (n, m, K, miss): n = 1 + L, then across the 16-row fragment (15, 16, 17), the wave's 32 rows (33) and the workgroup's 64-row
# tile (70, 130: two and three tiles, diagonal and off-diagonal workgroups); m across the 128-locus T block and the operand
# block B (B - 1, B, B + 1, 2 B + 5: three blocks, the last of 5 loci); K = 0, 1, 2, 10, 32
GRID = [(2, 1, 0, 0.0), (3, 3, 1, 0.0), (4, 127, 2, 0.1), (12, 128, 10, 0.0), (34, 129, 32, 0.1), (15, B - 1, 2, 0.1),
        (16, B, 1, 0.0), (17, B + 1, 10, 0.1), (33, 2 * B + 5, 0, 0.1), (70, 129, 32, 0.0), (130, 2 * B + 5, 2, 0.1),
        (70, B + 1, 10, 0.0), (130, 127, 1, 0.0), (16, 3, 0, 0.1), (17, 1, 2, 0.0), (33, 128, 10, 0.1), (15, 2 * B + 5, 1, 0.0),
        (130, B - 1, 32, 0.1), (70, B, 0, 0.1), (34, B + 1, 32, 0.0)]


def _view(tpg, codes, ind_row=None, ind_col=None):
    return tpg.View(tpg.FBM.from_numpy(codes), ind_row, ind_col, code256=None)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_case(tpg, codes, V, K, thr=0.01):
    n, m = codes.shape
    v = _view(tpg, codes)
    Q = tpg.pcrelate_basis(V, n)
    assert np.array_equal(_bits(Q), _bits(pr.basis(V, n)))
    # step 1
    cf = tpg.pcrelate_coef(v, Q)
    mean_x, c_x, c_bound = pr.coef_exact(codes, Q)
    assert np.array_equal(_bits(cf["mean"]), _bits(mean_x))
    dc = np.abs(cf["c"].astype(pr.LD) - c_x).astype(np.float64)
    assert not dc[c_bound == 0].any()
    rc = float((dc[c_bound > 0] / c_bound[c_bound > 0]).max()) if (c_bound > 0).any() else 0.0
    # step 2, from the device's own mean and c
    isaf = tpg.pcrelate_isaf(v, cf["mean"], cf["c"], Q, maf_bound=thr)
    mu = pr.mu_pinned(cf["mean"], cf["c"], Q)
    assert np.array_equal(_bits(isaf["mu"]), _bits(mu))
    assert np.array_equal(isaf["valid"], pr.operands(codes, mu, thr)[0])
    # step 3
    g = tpg.pcrelate_gram(v, cf["mean"], cf["c"], Q, maf_bound=thr)
    ex = pr.gram_exact(codes, mu, thr)
    assert np.array_equal(g["cnt"], ex["cnt"].astype(np.float64))
    ratios = {}
    for name in ("num", "den"):
        d = np.abs(g[name].astype(pr.LD) - ex[name]).astype(np.float64)
        bound = ex["b" + name]
        assert not d[bound == 0].any(), name  # no jointly valid locus (padding included): an exact zero
        ratios[name] = float((d[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        assert np.array_equal(g[name], g[name].T), name  # the mirror
    print(f"n {n} m {m} K {K}: largest ratio to the bound c {rc:.3e} num {ratios['num']:.3e} den {ratios['den']:.3e}")
    assert rc <= pr.REF_SLACK and ratios["num"] <= pr.REF_SLACK and ratios["den"] <= pr.REF_SLACK
    # the whole call: bit for bit the staged calls, and the same bits on a second call
    kin_s, f_s, ns_s = pr.epilogue(g["num"], g["den"], g["cnt"])
    for _ in range(2):
        w = tpg.pcrelate(v, V, maf_bound=thr)
        assert np.array_equal(_bits(w["kin"]), _bits(kin_s))
        assert np.array_equal(_bits(w["inbreeding"]), _bits(f_s))
        assert np.array_equal(w["n_snp"], ns_s)
    g2 = tpg.pcrelate_gram(v, cf["mean"], cf["c"], Q, maf_bound=thr)
    assert all(np.array_equal(_bits(g[k]), _bits(g2[k])) for k in ("num", "den", "cnt"))
    # step 4 against the exact route
    kin_x, f_x, _ = pr.epilogue(ex["num"].astype(np.float64), ex["den"].astype(np.float64), ex["cnt"])
    assert np.array_equal(np.isnan(w["kin"]), np.isnan(kin_x)) and np.array_equal(np.isnan(w["inbreeding"]), np.isnan(f_x))
    assert np.array_equal(np.isnan(kin_x), ex["cnt"] == 0)
    ok = ~np.isnan(kin_x)
    kb = pr.kin_bound(ex)
    with np.errstate(invalid="ignore"):
        kin_ld = (ex["num"] / (4 * ex["den"]))
    assert (np.abs(w["kin"].astype(pr.LD) - kin_ld).astype(np.float64)[ok] <= pr.REF_SLACK * kb[ok]).all()
    fb = 2.0 * np.diag(kb) + 2 * pr.EPS * (np.abs(f_x) + 1.0)
    okf = ~np.isnan(f_x)
    f_ld = (2 * np.diag(kin_ld) - 1)
    assert (np.abs(w["inbreeding"].astype(pr.LD) - f_ld).astype(np.float64)[okf] <= pr.REF_SLACK * fb[okf]).all()
    return dict(valid=isaf["valid"], kin=w["kin"], f=w["inbreeding"])


def test_block_and_scratch_sizes():
    import tidypopgen_amd as tpg

    assert all(tpg.pcrelate_block_loci(n) == B for n in sorted({g[0] for g in GRID}))
    # bounded independently of m: 16 bytes per padded row and locus of ONE block
    assert tpg.pcrelate_scratch_bytes(130, 2 * B + 5, 2) == 16 * 192 * B == tpg.pcrelate_scratch_bytes(130, 10 ** 9, 32)
    assert tpg.pcrelate_scratch_bytes(17, 129, 2) == 16 * 64 * 256
    big = tpg.pcrelate_block_loci(100000)
    assert big % 128 == 0 and 128 <= big < B and tpg.pcrelate_scratch_bytes(100000, 10 ** 9, 10) <= 256 << 20


@pytest.mark.parametrize("n,m,K,miss", GRID)
def test_pcrelate_grid(n, m, K, miss):
    import tidypopgen_amd as tpg

    codes, V = pr.panel(1000 * K + 7 * n + m, n, m, miss, K)
    r = _check_case(tpg, codes, V, K)
    if m >= 2:
        assert not r["valid"][:, :2].any()  # the locus wholly missing and the monomorphic one: invalid for everyone
    if n >= 4:
        assert np.isnan(r["kin"][1]).all() and np.isnan(r["kin"][:, 1]).all() and np.isnan(r["f"][1])  # wholly missing


def test_a_locus_whose_mu_straddles_the_bound():
    import tidypopgen_amd as tpg

    codes, V = pr.panel(99, 130, 300, 0.0, 2)
    codes[:, 2] = 0
    codes[np.argsort(V[:, 0])[-20:], 2] = 1  # a rare allele at one end of the cline
    r = _check_case(tpg, codes, V, 2)
    typed = codes[:, 2] != 3
    assert r["valid"][typed, 2].any() and not r["valid"][typed, 2].all()


def test_sub_view_equals_the_copied_sub_panel():
    import tidypopgen_amd as tpg

    codes, _ = pr.panel(5, 90, 700, 0.1, 2)
    rows, cols = np.arange(3, 90, 2), np.r_[np.arange(1, 400, 3), np.arange(500, 700)]
    sub = np.ascontiguousarray(codes[np.ix_(rows, cols)])
    V = pr.numpy_scores(sub, 2)
    a = tpg.pcrelate(_view(tpg, codes, rows + 1, cols + 1), V)  # the indices of a view are 1-based, as the reference's
    b = tpg.pcrelate(_view(tpg, sub), V)
    for k in ("kin", "inbreeding"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(a["n_snp"], b["n_snp"])
    X = tpg.FBM.from_numpy(codes)
    pca = dict(u=V / np.linalg.norm(V, axis=0), d=np.linalg.norm(V, axis=0))
    c = tpg.gt_pcrelate(X, pca, ind_row=rows + 1, ind_col=cols + 1)
    assert np.allclose(c["kin"], a["kin"], rtol=1e-9, atol=1e-12, equal_nan=True)  # u d re-multiplied: not the same bits of V


def test_refusals_leave_the_outputs_untouched():
    import ctypes as C

    import tidypopgen_amd as tpg
    from tidypopgen_amd import _lib

    codes, V = pr.panel(3, 20, 200, 0.05, 2)
    v = _view(tpg, codes)
    Q = tpg.pcrelate_basis(V)
    cf = tpg.pcrelate_coef(v, Q)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    kin, f, ns = np.full((20, 20), 7.0, order="F"), np.full(20, 7.0), np.full((20, 20), 7, dtype=np.int64, order="F")
    dup = np.asfortranarray(np.column_stack([V[:, 0], 2.0 * V[:, 0]]))
    const = np.asfortranarray(np.column_stack([V[:, 0], np.full(20, 3.0)]))
    bad = [(V, 2, 0.0), (V, 2, 0.5), (V, 2, float("nan")), (dup, 2, 0.01), (const, 2, 0.01), (V, 33, 0.01), (V, -1, 0.01)]
    for Vb, K, thr in bad:
        assert _lib.lib.tpg_pcrelate(v.ctx.h, v.h, ptr(Vb), K, thr, ptr(kin), ptr(f), ptr(ns)) == EINVAL, (K, thr)
    wide = np.asfortranarray(np.random.default_rng(0).standard_normal((20, 19)))  # n < L + 1
    assert _lib.lib.tpg_pcrelate(v.ctx.h, v.h, ptr(wide), 19, 0.01, ptr(kin), ptr(f), ptr(ns)) == EINVAL
    num, den, cnt = (np.full((20, 20), 7.0, order="F") for _ in range(3))
    for L, thr in ((0, 0.01), (34, 0.01), (3, 0.5), (3, -0.1)):
        assert _lib.lib.tpg_pcrelate_gram(v.ctx.h, v.h, ptr(cf["mean"]), ptr(cf["c"]), ptr(Q), L, thr, ptr(num), ptr(den),
                                          ptr(cnt)) == EINVAL
    cnan = cf["c"].copy(order="F")
    cnan[5, 1] = np.nan
    assert _lib.lib.tpg_pcrelate_gram(v.ctx.h, v.h, ptr(cf["mean"]), ptr(cnan), ptr(Q), 3, 0.01, ptr(num), ptr(den), ptr(cnt)) == 4
    mu, valid = np.full((20, 200), 7.0, order="F"), np.full((20, 200), 7, dtype=np.uint8, order="F")
    assert _lib.lib.tpg_pcrelate_isaf(v.ctx.h, v.h, ptr(cf["mean"]), ptr(cf["c"]), ptr(Q), 3, 0.7, ptr(mu), ptr(valid)) == EINVAL
    for a in (kin, f, ns, num, den, cnt, mu, valid):
        assert (a == 7).all()
    with pytest.raises(_lib.TpgError):
        tpg.pcrelate_basis(dup)
    # above the cell cap (2^26) the dense mu is refused
    cap = int(_lib.lib.tpg_pcrelate_isaf_max_cells())
    assert cap == 1 << 26
    nb = 8200  # 8200^2 = 2^26 + 131 136
    vb = tpg.View(tpg.FBM.synth(1, nb, nb, npop=2, miss=0.0), code256=None)
    mean, c1, Q1 = np.ones(nb), np.zeros((nb, 1), order="F"), np.full((nb, 1), 1.0 / np.sqrt(nb), order="F")
    mu, valid = np.empty((nb, nb), order="F"), np.empty((nb, nb), dtype=np.uint8, order="F")
    assert _lib.lib.tpg_pcrelate_isaf(vb.ctx.h, vb.h, ptr(mean), ptr(c1), ptr(Q1), 1, 0.01, ptr(mu), ptr(valid)) == EINVAL
    assert "cells" in _lib.lib.tpg_last_error().decode()


def test_pedigree_panel_end_to_end():
    import tidypopgen_amd as tpg

    codes, anc, pairs = pr.pedigree_panel()
    X = tpg.FBM.from_numpy(codes)
    pca = tpg.gt_pca_partialSVD(X, k=2, code256=None, impute="mode")
    r = tpg.gt_pcrelate(X, pca, k=2)
    kin = r["kin"]
    assert kin.shape == (150, 150) and not np.isnan(kin).any() and np.array_equal(kin, kin.T)
    model = pr.pcrelate(codes, np.asfortranarray(pca["u"] * pca["d"][None, :]))
    assert np.array_equal(r["n_snp"], model["n_snp"])
    assert np.allclose(kin, model["kin"], rtol=0, atol=1e-10) and np.allclose(r["inbreeding"], model["inbreeding"], rtol=0, atol=1e-10)
    # every first-degree pair is found, and the filter leaves no related pair behind
    for ix in (pairs["po"], pairs["fs"]):
        assert (kin[ix[:, 0], ix[:, 1]] > 0.0884).all()
    passed, removed, keep = tpg.filter_high_relatedness(kin, 0.0884)
    sub = kin[np.ix_(keep, keep)]
    assert (sub[~np.eye(len(sub), dtype=bool)] <= 0.0884).all()
    rel = np.r_[pairs["po"], pairs["fs"]]
    assert not (keep[rel[:, 0]] & keep[rel[:, 1]]).any() and len(removed) >= pr.PED_FAMILIES * 2
    # the hook: mean and c from the unrelated founders through the staged calls, the Grams over everybody
    F = pairs["founders"]
    V = pr.numpy_scores(codes, 2, F)
    want = pr.pcrelate_trained(codes, V, F)
    cf = tpg.pcrelate_coef(_view(tpg, codes, F + 1), want["Qt"])
    g = tpg.pcrelate_gram(_view(tpg, codes), cf["mean"], cf["c"], want["Q"])
    kin_t = pr.epilogue(g["num"], g["den"], g["cnt"])[0]
    assert np.allclose(kin_t, want["kin"], rtol=0, atol=1e-10)
    d = pr.pedigree_deviations(kin_t, anc, pairs)
    print("trained K = 2 on the device:", d)
    assert d["po"] < 0.03 and d["fs"] < 0.03 and d["cross"] < 0.03  # the records of tests/test_pcrelate_host.py, rounded up
