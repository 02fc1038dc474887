"""GPU: Hardy-Weinberg exact tests (csrc/hwe.hip) through the C ABI and tidypopgen_amd.api against the exact-arithmetic
reference of tests/hwe_ref.py, applied to genotype counts taken with numpy from the same bytes.

Tolerance (hwe_ref.close): relative 8 max(n, 8) 2^-53 with n the typed individuals of that test, absolute 1e-300 where the
exact p is below that.  A case is compared only if no other heterozygote count is almost, but not exactly, as likely as
the observed one (hwe_ref.comparable: nearest >= 2^-30); the share left out is asserted: 0 for the exhaustive set, at most
0.1 % of a synthetic panel."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import fixtures as fx
from tests import hwe_ref as hr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


_cache = {}


def _exact(a, h, b):
    key = (min(a, b), h, max(a, b))
    if key not in _cache:
        _cache[key] = hr.exact(*key)
    return _cache[key]


def _check(got, tables, midp, max_left_out):
    """got[k] against the exact value of tables[k] = (hom1, het, hom2); returns the number of cases left out"""
    got = np.asarray(got, dtype=np.float64).ravel()
    assert got.shape[0] == len(tables)
    left_out = 0
    for k, (a, h, b) in enumerate(tables):
        r = _exact(int(a), int(h), int(b))
        if not hr.comparable(r):
            left_out += 1
            continue
        want = r.p_mid if midp else r.p
        assert hr.close(float(got[k]), want, int(a) + int(h) + int(b)), (int(a), int(h), int(b), midp, float(got[k]), float(want))
    assert left_out <= max_left_out, (left_out, len(tables))
    return left_out


def test_every_table_of_up_to_40_individuals(tpg):
    tabs = hr.all_tables(40)
    counts = np.ascontiguousarray(np.array(tabs, dtype=np.int32))  # count x 3 row-major = 3 x count column-major
    ctx = tpg.default_context()
    lib = tpg._lib.lib
    for midp in (0, 1):
        out = np.full(len(tabs), -1.0)
        tpg._lib.check(lib.tpg_hwe_exact_counts(ctx.h, counts.ctypes.data, C.c_int64(len(tabs)), C.c_int(midp), out.ctypes.data))
        assert _check(out, tabs, midp, 0) == 0
        # device pointers on both sides: the same bits
        d_in, d_out = ctx.dev_alloc(counts.nbytes), ctx.dev_alloc(out.nbytes)
        tpg._lib.check(lib.tpg_dev_from_host(ctx.h, d_in, C.c_void_p(counts.ctypes.data), C.c_size_t(counts.nbytes)))
        tpg._lib.check(lib.tpg_hwe_exact_counts(ctx.h, d_in, C.c_int64(len(tabs)), C.c_int(midp), d_out))
        dev = np.zeros(len(tabs))
        tpg._lib.check(lib.tpg_dev_to_host(ctx.h, C.c_void_p(dev.ctypes.data), d_out, C.c_size_t(dev.nbytes)))
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)
        assert np.array_equal(dev, out)
        # the literal mirrors
        assert np.array_equal(tpg.hwe_on_matrix(counts.T, midp), out)
    assert tpg.SNPHWE2_R(4, 0, 2, 1) == tpg.hwe_on_matrix(np.array([[0], [4], [2]]), True)[0]
    assert hr.close(tpg.SNPHWE2_R(4, 0, 2, 1), hr.exact(0, 4, 2).p_mid, 6)


@pytest.mark.parametrize("mid_p,name", [(False, "families_hwe.hwe"), (True, "families_hwe_midp.hwe")])
def test_families_against_plink(tpg, mid_p, name):
    rows = hr.read_plink_hwe(os.path.join(fx.GOLDEN, "related", name))
    fam = tpg.FBM.open_bed(os.path.join(fx.GOLDEN, "related/families.bed"), 12, 961)
    p = tpg.loci_hwe(fam, None, np.arange(1, 11), mid_p=mid_p)
    assert p.shape == (10,)
    for k, (snp, tab, want) in enumerate(rows):
        assert abs(p[k] - want) <= 5e-5, (snp, tab, p[k], want)
    # the same genotypes as an FBM of bytes, all loci: the PLINK rows are the first ten
    X = tpg.FBM.from_numpy(fx.families_fbm())
    assert np.array_equal(tpg.loci_hwe(X, mid_p=mid_p)[:10], p)


def _tables(codes, gid=None, G=1):
    """(m * G) tables in the order of a column-major m x G result, from codes (n x m; 0, 1, 2, 3 = missing)"""
    gid = np.zeros(codes.shape[0], dtype=np.int64) if gid is None else np.asarray(gid)
    out = []
    for g in range(G):
        sub = codes[gid == g]
        c = np.stack([(sub == k).sum(axis=0) for k in range(3)], axis=1)
        out.extend(tuple(int(v) for v in row) for row in c)
    return out


# n, m, G: m scaled so that the exact reference of the whole module stays under a minute
PANELS = [(2, 300, 1), (65, 400, 3), (65, 150, 51), (1000, 300, 1), (1000, 120, 3), (1000, 40, 51), (5000, 60, 1), (5000, 24, 3),
          (5000, 8, 51)]


@pytest.mark.parametrize("n,m,G", PANELS)
def test_synthetic_panels(tpg, n, m, G):
    seed = 1000 * G + n
    fbm = orc.synth_fbm(seed, n, m, npop=max(G, 2), miss=0.03)
    fbm[:, m // 2] = 3  # a locus nobody is typed at
    X = tpg.FBM.from_numpy(fbm)
    codes = np.where(fbm < 3, fbm, 3)
    rng = np.random.default_rng(seed)
    gid = rng.integers(0, G, size=n).astype(np.int32)
    if G > 1:
        gid[gid == G - 1] = 0  # an empty group
    for mid_p in (True, False):
        v = tpg.View(X)
        p = tpg.gt_grouped_hwe(v, gid, G, mid_p=mid_p)
        assert p.shape == (m, G)
        tabs = _tables(codes, gid, G)
        _check(p.ravel(order="F"), tabs, mid_p, len(tabs) // 1000)
        assert np.all(p[m // 2] == (0.5 if mid_p else 1.0))
        if G > 1:
            assert np.all(p[:, G - 1] == (0.5 if mid_p else 1.0))
        q = tpg.loci_hwe(X, mid_p=mid_p)
        tabs1 = _tables(codes)
        _check(q, tabs1, mid_p, len(tabs1) // 1000)
        # one device function behind all three: bit for bit
        assert np.array_equal(tpg.gt_grouped_hwe(v, np.zeros(n, dtype=np.int32), 1, mid_p=mid_p)[:, 0], q)
        assert np.array_equal(tpg.hwe_on_matrix(tpg.loci_counts(v).T, mid_p), q)
    # row / column subsets and permutations
    if n > 2:
        rows = rng.permutation(n)[: max(2, (2 * n) // 3)] + 1
        cols = rng.permutation(m)[: max(1, m // 2)] + 1
        sub = codes[np.ix_(rows - 1, cols - 1)]
        q = tpg.loci_hwe(X, rows, cols)
        tabs = _tables(sub)
        _check(q, tabs, True, len(tabs) // 1000)
        v = tpg.View(X, rows, cols)
        p = tpg.gt_grouped_hwe(v, gid[rows - 1], G)
        tabs = _tables(sub, gid[rows - 1], G)
        _check(p.ravel(order="F"), tabs, True, len(tabs) // 1000)


def test_imputed_store_through_code_impute_pred(tpg):
    n, m = 301, 200
    raw = orc.synth_fbm(77, n, m, npop=3, miss=0.1)
    X = tpg.FBM.from_numpy(raw)
    before = tpg.loci_hwe(X)
    tpg.gt_impute_simple(X, "mode")  # bytes 4..6 now read as genotypes: nobody is missing any more
    filled = X.to_numpy()
    codes = np.where(filled >= 4, filled - 4, filled)
    assert (codes < 3).all()
    after = tpg.loci_hwe(X)
    tabs = _tables(codes)
    _check(after, tabs, True, len(tabs) // 1000)
    assert not np.array_equal(before, after)
    v = tpg.View(X, code256=tpg.CODE_012)  # the raw reading of the same store: the imputed bytes are missing again
    assert np.array_equal(tpg.gt_grouped_hwe(v, np.zeros(n, dtype=np.int32), 1)[:, 0], before)


def test_forty_thousand_individuals(tpg):
    """int64 products (2 n het overflows int32), p < 1e-300 on both sides of the expectation, and an ordinary table"""
    tabs = [(7000, 26000, 7000), (13000, 14000, 13000), (10000, 20000, 10000), (9000, 22000, 9000), (39000, 900, 100)]
    for midp in (0, 1):
        got = tpg.hwe_on_matrix(np.array(tabs).T, midp)
        _check(got, tabs, midp, 0)
        assert 0.0 <= got[0] <= 1e-300 and 0.0 <= got[1] <= 1e-300
    # the same through a genotype store: one locus of 40 000 individuals per table
    n = 40000
    g = np.zeros((n, len(tabs)), dtype=np.uint8, order="F")
    for j, (a, h, b) in enumerate(tabs):
        g[a:a + h, j] = 1
        g[a + h:, j] = 2
    X = tpg.FBM.from_numpy(g)
    for midp in (False, True):
        assert np.array_equal(tpg.loci_hwe(X, mid_p=midp), tpg.hwe_on_matrix(np.array(tabs).T, midp))


def test_errors(tpg):
    lib = tpg._lib.lib
    ctx = tpg.default_context()
    X = tpg.FBM.from_numpy(orc.synth_fbm(3, 20, 30, npop=2))
    v = tpg.View(X)
    out = np.zeros(30 * 2)
    gid = np.zeros(20, dtype=np.int32)
    counts = np.array([[1, 2, 3], [4, -1, 6]], dtype=np.int32)
    assert lib.tpg_hwe_exact_counts(ctx.h, None, C.c_int64(2), C.c_int(0), out.ctypes.data) == 1
    assert lib.tpg_hwe_exact_counts(ctx.h, counts.ctypes.data, C.c_int64(2), C.c_int(0), None) == 1
    assert lib.tpg_hwe_exact_counts(ctx.h, counts.ctypes.data, C.c_int64(-1), C.c_int(0), out.ctypes.data) == 1
    assert lib.tpg_hwe_exact_counts(ctx.h, counts.ctypes.data, C.c_int64(2), C.c_int(2), out.ctypes.data) == 1
    assert lib.tpg_hwe_exact_counts(ctx.h, counts.ctypes.data, C.c_int64(2), C.c_int(0), out.ctypes.data) == 1
    assert "negative" in lib.tpg_last_error().decode()
    assert lib.tpg_hwe_exact_counts(ctx.h, counts.ctypes.data, C.c_int64(1), C.c_int(0), out.ctypes.data) == 0
    assert lib.tpg_hwe_exact_counts(ctx.h, None, C.c_int64(0), C.c_int(0), None) == 0
    assert lib.tpg_loci_hwe(ctx.h, None, C.c_int(0), out.ctypes.data) == 1
    assert lib.tpg_loci_hwe(ctx.h, v.h, C.c_int(0), None) == 1
    assert lib.tpg_loci_hwe(ctx.h, v.h, C.c_int(3), out.ctypes.data) == 1
    assert lib.tpg_gt_grouped_hwe(ctx.h, v.h, None, C.c_int(1), C.c_int(0), out.ctypes.data) == 1
    assert lib.tpg_gt_grouped_hwe(ctx.h, v.h, gid.ctypes.data, C.c_int(1), C.c_int(0), None) == 1
    assert lib.tpg_gt_grouped_hwe(ctx.h, v.h, gid.ctypes.data, C.c_int(0), C.c_int(0), out.ctypes.data) == 1
    for bad in (-1, 2):
        gid[7] = bad
        assert lib.tpg_gt_grouped_hwe(ctx.h, v.h, gid.ctypes.data, C.c_int(2), C.c_int(0), out.ctypes.data) == 1
        assert "groupIds[7]" in lib.tpg_last_error().decode()
    with pytest.raises(tpg._lib.TpgError):
        tpg.hwe_on_matrix(counts.T, True)
    with pytest.raises(ValueError, match="Not implemented for a single individual"):
        tpg.loci_hwe(X, np.array([3]), None)
    with pytest.raises(ValueError, match="Not implemented for a single individual"):
        tpg.loci_hwe(tpg.FBM.from_numpy(np.zeros((1, 4), dtype=np.uint8)))
