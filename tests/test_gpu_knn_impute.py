"""LD-kNN imputation on the GPU (include/tpg.h "LD-kNN imputation"): tpg_ld_top_neighbours, tpg_view_impute_knn,
tpg_fbm_impute_knn and tpg_view_impute_errors against the numpy restatement tests/knn_impute_ref.py -- everything to equality,
r2 bit for bit."""
import itertools
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import fixtures as fx
from tests import impute_ref as ir
from tests import knn_impute_ref as kr

pytestmark = pytest.mark.gpu

NS = (2, 5, 63, 64, 65, 129, 300)
MS = (1, 31, 32, 33, 97, 300)
WIDTHS = (0, 1, 31, 32, 33, 100)  # bands that end on, before and after a 32-locus tile and a 16-tile super-chunk
LS = (1, 10, 32)
MIN_R2 = (0.0, 0.2)


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


def _raw_store(rng, n, m, rates=(0.0, 0.02, 0.5, 1.0)):
    """CODE_012 bytes with a missing rate per locus drawn from `rates` (mixed), and allele frequencies from 0 to 1 (the recipe
    of tests/test_gpu_impute.py)"""
    p = rng.random(m)
    p[::11] = 0.0
    p[5::11] = 1.0
    g = rng.binomial(2, p[None, :], size=(n, m)).astype(np.uint8)
    rate = rng.choice(list(rates), size=m)
    g[rng.random((n, m)) < rate[None, :]] = 3
    return np.asfortranarray(g)


def _duplicate_columns(g):
    """copies of a column at distances 2 and 4: r2 ties that the distance and then the index decide"""
    m = g.shape[1]
    for c in range(3, m - 6, 13):
        g[:, c + 2] = g[:, c]
        g[:, c + 4] = g[:, c]
    return g


def _windows(m, width):
    """one chromosome; two chromosomes whose border falls inside a 32-locus tile"""
    out = [kr.window(m, width)]
    if m >= 4:
        out.append(kr.window(m, width, chrom_ends=[m // 2 + 3, m]))
    return out


def _rotation(*lists):
    """every combination of the parameter lists, over and over"""
    return itertools.cycle(itertools.product(*lists))


@pytest.mark.parametrize("n", NS)
def test_top_neighbours_equal_r2_bit_for_bit(tpg, n):
    rng = np.random.default_rng(100 + n)
    rot = _rotation(LS, MIN_R2, (0, tpg.KNN_SMALL_CHUNKS))
    ties = 0
    for m in MS:
        filled = _duplicate_columns(ir.impute_codes(_raw_store(rng, n, m), "mode"))  # monomorphic and all-missing loci mixed in
        v = tpg.View(tpg.FBM.from_numpy(np.asfortranarray(filled)), code256=None)
        for width in WIDTHS:
            for hi in _windows(m, width):
                l, min_r2, flags = next(rot)
                nbr, r2 = tpg.ld_top_neighbours(v, hi, l, min_r2, _flags=flags)
                want_nbr, want_r2 = kr.top_neighbours(filled, hi, l, min_r2)
                assert np.array_equal(nbr, want_nbr), (m, width, l, min_r2, flags)
                assert np.array_equal(r2.view(np.uint64), want_r2.view(np.uint64)), (m, width, l, min_r2, flags)
                ties += int(((want_r2[:, 1:] == want_r2[:, :-1]) & (want_nbr[:, 1:] >= 0)).sum())
    assert ties > 0 or n < 5  # the duplicated columns did give ties


def _knn_case(rng, n, m):
    raw = _duplicate_columns(_raw_store(rng, n, m, rates=(0.0, 0.05, 0.5, 1.0)))
    if n >= 5:
        raw[1, :] = 3  # an individual missing everywhere
    if m >= 8:
        raw[:, 6] = 3  # a locus where only one individual is typed
        raw[n // 2, 6] = 1
    return np.asfortranarray(raw)


@pytest.mark.parametrize("n", (1,) + NS)
def test_view_impute_knn_equals_the_restatement(tpg, n):
    rng = np.random.default_rng(200 + n)
    rot = _rotation(LS, (1, 8, n + 5), MIN_R2, (0, tpg.KNN_SMALL_CHUNKS, tpg.KNN_PROFILES_GLOBAL))
    seen = dict(left=0, none=0, imputed=0)
    for m in MS:
        raw = _knn_case(rng, n, m)
        for code in (None, tpg.CODE_012):
            v = tpg.View(tpg.FBM.from_numpy(raw), code256=code)
            for width in WIDTHS[code is not None::2]:  # the widths are dealt to the two code tables
                for hi in _windows(m, width):
                    l, k, min_r2, flags = next(rot)
                    got = v.impute_knn(hi, l, k, min_r2, _flags=flags)
                    want, rep, _, _ = kr.impute(raw, hi, l, k, min_r2)
                    assert np.array_equal(got.unpack(), want), (m, width, l, k, min_r2, flags)
                    assert got.impute_report == rep, (m, width, l, k, min_r2, flags)
                    for f in seen:
                        seen[f] += rep[{"left": "entries_left", "none": "loci_without_neighbours", "imputed": "imputed"}[f]]
                    got.free()
    assert seen["left"] > 0 and seen["none"] > 0 and (seen["imputed"] > 0 or n == 1)


def test_subsets_and_bed_store(tpg):
    rng = np.random.default_rng(7)
    raw = _knn_case(rng, 140, 200)
    X = tpg.FBM.from_numpy(raw)
    rows = np.arange(140, 0, -2, dtype=np.int32)  # reversed
    cols = np.r_[np.arange(2, 120, 3), np.arange(121, 200)].astype(np.int32)
    sub = raw[rows - 1][:, cols - 1]
    hi = kr.window(len(cols), 40)
    got = tpg.View(X, rows, cols, code256=None).impute_knn(hi, 10, 8)
    want, rep, _, _ = kr.impute(sub, hi, 10, 8)
    assert np.array_equal(got.unpack(), want) and got.impute_report == rep
    n, m = 176, 79
    path = os.path.join(fx.GOLDEN, "lobster/lobster.bed")
    geno = orc.read_bed(path, n, m)
    codes = np.where(geno < 3, geno, 3).astype(np.uint8)
    assert (codes == 3).any()
    B = tpg.FBM.open_bed(path, n, m)
    hi = kr.window(m, 30)
    got = tpg.View(B, code256=tpg.CODE_012).impute_knn(hi, 10, 8, 0.05)
    want, rep, _, _ = kr.impute(codes, hi, 10, 8, 0.05)
    assert np.array_equal(got.unpack(), want) and got.impute_report == rep
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.gt_impute_knn(B, size=30)
    assert e.value.code == 3 and "tpg_view_impute_knn" in str(e.value)


def test_profiles_in_lds_and_in_global_scratch_give_the_same_bytes(tpg):
    """n <= 11 520 keeps the profiles in LDS, more reads them from global scratch; TPG_KNN_PROFILES_GLOBAL forces the second
    path at a size that runs in a moment (1 300 individuals: 11 blocks of 128, more than one pass of the 256 threads over the
    dwords of a locus)"""
    rng = np.random.default_rng(8)
    _, raw = kr.panel(rng, 1300, 70, miss=0.03)
    raw[:, 11] = 3
    raw = np.asfortranarray(raw)
    v = tpg.View(tpg.FBM.from_numpy(raw), code256=None)
    hi = kr.window(70, 25)
    a = v.impute_knn(hi, 10, 8)
    b = v.impute_knn(hi, 10, 8, _flags=tpg.KNN_PROFILES_GLOBAL)
    want, rep, _, _ = kr.impute(raw, hi, 10, 8)
    assert np.array_equal(a.unpack(), want) and np.array_equal(b.unpack(), want)
    assert a.impute_report == rep and b.impute_report == rep


@pytest.mark.parametrize("n", (11520, 11521))
def test_either_side_of_the_lds_limit(tpg, n):
    """11 520 individuals are the most whose profiles one workgroup keeps in LDS (162 432 of the 163 840 bytes); one more and the
    call takes the global scratch by itself"""
    rng = np.random.default_rng(n)
    _, raw = kr.panel(rng, n, 12, founders=6, miss=0.01)
    raw = np.asfortranarray(raw)
    hi = kr.window(12, 5)
    got = tpg.View(tpg.FBM.from_numpy(raw), code256=None).impute_knn(hi, 4, 8)
    want, rep, _, _ = kr.impute(raw, hi, 4, 8)
    assert np.array_equal(got.unpack(), want) and got.impute_report == rep and rep["imputed"] > 1000


@pytest.mark.parametrize("nrow", (5, 16, 17, 65, 1000))
def test_gt_impute_knn_store_bytes(tpg, nrow):
    rng = np.random.default_rng(300 + nrow)
    m = 45 if nrow >= 1000 else 131  # nrow * j is no multiple of 16 for most columns
    raw = _knn_case(rng, nrow, m)
    hi = kr.window(m, 20)
    X = tpg.FBM.from_numpy(raw)
    assert tpg.gt_impute_knn(X, l=10, k=8, size=20) is X
    want, rep = kr.store_bytes(raw, hi, 10, 8)
    got = X.to_numpy()
    assert np.array_equal(got[raw != 3], raw[raw != 3]), "a typed byte changed"
    assert np.array_equal(got, want), int((got != want).sum())
    assert X.impute_report == rep
    assert np.array_equal(X.code256, tpg.CODE_IMPUTE_PRED, equal_nan=True)
    # a second call on the imputed store is refused and changes nothing
    with pytest.raises(tpg._lib.TpgError, match="already imputed") as e:
        tpg.gt_impute_knn(X, l=10, k=8, size=20)
    assert e.value.code == 3
    assert np.array_equal(X.to_numpy(), want)


def test_refusals_and_the_pca_of_an_imputed_store(tpg):
    rng = np.random.default_rng(9)
    raw = _raw_store(rng, 60, 90)
    for byte in (4, 200):
        bad = raw.copy()
        bad[17, 50] = byte
        X = tpg.FBM.from_numpy(bad)
        with pytest.raises(tpg._lib.TpgError, match="already imputed") as e:
            tpg.gt_impute_knn(X, size=10)
        assert e.value.code == 3
        assert np.array_equal(X.to_numpy(), bad)
    X = tpg.FBM.from_numpy(raw)
    v = tpg.View(X, code256=None)
    hi = kr.window(90, 10)
    lib = tpg._lib.lib
    import ctypes as C

    out = C.c_void_p()
    for l, k, r in ((0, 8, 0.0), (33, 8, 0.0), (10, 0, 0.0), (10, 8, -0.1), (10, 8, float("nan"))):
        assert lib.tpg_view_impute_knn(v.ctx.h, v.h, hi.ctypes.data, l, k, r, 0, C.byref(out), None, None) == 1, (l, k, r)
        assert lib.tpg_fbm_impute_knn(X.ctx.h, X.h, hi.ctypes.data, l, k, r, 0, None, None) == 1, (l, k, r)
    assert lib.tpg_view_impute_knn(v.ctx.h, v.h, hi[::-1].copy().ctypes.data, 10, 8, 0.0, 0, C.byref(out), None, None) == 1
    assert out.value is None and np.array_equal(X.to_numpy(), raw)
    assert tpg.knn_impute_scratch_bytes(5000, 1000000, 100, 10) > 0
    # the imputed store runs through the PCA (no locus of this panel is typed nowhere), where the raw one is refused
    truth, praw = kr.panel(np.random.default_rng(10), 120, 400)
    praw = praw[:, [len(set(c[c != 3])) >= 2 for c in praw.T]]  # (a monomorphic locus has a zero scale: the PCA refuses that too)
    assert praw.shape[1] > 300
    P = tpg.FBM.from_numpy(np.asfortranarray(praw))
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.gt_pca_partialSVD(P, k=3)
    assert e.value.code == 4
    tpg.gt_impute_knn(P, size=50)
    assert P.impute_report["entries_left"] == 0
    pca = tpg.gt_pca_partialSVD(P, k=3)
    assert np.isfinite(pca["d"]).all() and pca["u"].shape == (120, 3)


def test_knn_impute_errors_counts(tpg):
    rng = np.random.default_rng(11)
    _, raw = kr.panel(rng, 150, 257, switch=0.05)
    raw = np.asfortranarray(raw)
    v = tpg.View(tpg.FBM.from_numpy(raw), code256=None)
    hi = kr.window(257, 50)
    got = tpg.knn_impute_errors(v, hi, 10, 8, 0.0, fraction=0.05, seed=3)
    train = v.holdout_fraction(0.05, 3)
    tcodes = train.unpack()
    filled, _, _, _ = kr.impute(tcodes, hi, 10, 8)
    per, tot = kr.errors(raw, tcodes, filled)
    assert np.array_equal(got["per_locus"], per.T)
    assert (got["held"], got["wrong"]) == (int(tot[0]), int(tot[1])) and got["held"] == train.n_held > 0
    # the totals against the three unpacked views, compared on the host
    f = train.impute_knn(hi, 10, 8)
    held = (raw != 3) & (tcodes == 3)
    assert got["wrong"] == int((f.unpack() != raw)[held].sum()) and 0 < got["wrong"] < got["held"]
    # gt_impute_knn attaches the same table when asked for it
    X = tpg.FBM.from_numpy(raw)
    tpg.gt_impute_knn(X, size=50, append_error=True, error_fraction=0.05, seed=3)
    assert np.array_equal(X.impute_errors["per_locus"], per.T)


def test_mosaic_panel_equals_the_restatement_and_twice_the_same(tpg):
    """the device fill equals the restatement, so it inherits the accuracy tests/test_knn_impute_host.py shows on the host"""
    _, raw = kr.panel(np.random.default_rng(11), 200, 300)
    raw = np.asfortranarray(raw)
    v = tpg.View(tpg.FBM.from_numpy(raw), code256=None)
    hi = kr.window(300, 50)
    a, b = v.impute_knn(hi, 10, 8), v.impute_knn(hi, 10, 8)
    want, rep, _, _ = kr.impute(raw, hi, 10, 8)
    assert np.array_equal(a.unpack(), want) and a.impute_report == rep
    assert np.array_equal(a.unpack(), b.unpack()) and a.impute_report == b.impute_report
    X, Y = tpg.FBM.from_numpy(raw), tpg.FBM.from_numpy(raw)
    tpg.gt_impute_knn(X, size=50)
    tpg.gt_impute_knn(Y, size=50)
    assert np.array_equal(X.to_numpy(), Y.to_numpy()) and np.array_equal(X.to_numpy(), kr.store_bytes(raw, hi, 10, 8)[0])
