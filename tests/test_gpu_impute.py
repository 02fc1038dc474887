"""Simple imputation on the GPU (include/tpg.h "simple imputation"): tpg_fbm_impute_simple on a byte store, tpg_view_impute on a
packed view, and impute= on the PCA routes, against the integer-only numpy restatement tests/impute_ref.py -- bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import fixtures as fx
from tests import impute_ref as ir

pytestmark = pytest.mark.gpu

NROWS = (1, 5, 15, 16, 17, 63, 64, 65, 1000, 5003)
SEEDS = (0, 0xDEADBEEFCAFE1234)


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


def _raw_store(rng, n, m):
    """CODE_012 bytes with a missing rate of 0, 2 %, 50 % or 100 % per locus (mixed), and allele frequencies from 0 to 1"""
    p = rng.random(m)
    p[::11] = 0.0
    p[5::11] = 1.0
    g = rng.binomial(2, p[None, :], size=(n, m)).astype(np.uint8)
    rate = rng.choice([0.0, 0.02, 0.5, 1.0], size=m)
    g[rng.random((n, m)) < rate[None, :]] = 3
    return np.asfortranarray(g)


def _aligned(a, b):
    return b * np.sign((a * b).sum(axis=0))


@pytest.mark.parametrize("nrow", NROWS)
def test_store_bytes_bit_for_bit(tpg, nrow):
    rng = np.random.default_rng(1000 + nrow)
    m = 301 if nrow >= 1000 else 400
    raw = _raw_store(rng, nrow, m)
    for method in ir.METHODS:
        for seed in SEEDS:
            X = tpg.FBM.from_numpy(raw)
            rep = X.impute_simple(method, seed)
            got = X.to_numpy()
            want = ir.store_bytes(raw, method, seed)
            assert np.array_equal(got[raw != 3], raw[raw != 3]), (method, seed, "a typed byte changed")
            assert np.array_equal(got, want), (method, seed, int((got != want).sum()))
            assert rep == ir.report(raw), (method, seed)
            X.free()


@pytest.mark.parametrize("wpl", ["1", "4", "16"])
def test_store_every_launch_shape_gives_the_same_bytes(tpg, wpl, monkeypatch):
    """a wave per locus, 4 waves, 16 waves (TPG_IMPUTE_WPL): 9 000 rows do not fit one wave's registers, so the forced
    one-wave shape also runs the read-twice form of the kernel"""
    monkeypatch.setenv("TPG_IMPUTE_WPL", wpl)
    rng = np.random.default_rng(7)
    for nrow in (777, 9001):
        raw = _raw_store(rng, nrow, 64)
        X = tpg.FBM.from_numpy(raw)
        X.impute_simple("random", 3)
        assert np.array_equal(X.to_numpy(), ir.store_bytes(raw, "random", 3)), nrow
        X.free()


def test_refusals_leave_the_store_unchanged(tpg):
    rng = np.random.default_rng(5)
    raw = _raw_store(rng, 333, 500)
    raw[:, 250] = rng.integers(0, 4, 333)
    bad = raw.copy()
    bad[17, 250] = 4  # one imputed byte in a column that has missing entries left
    bad[3, 499] = 200
    X = tpg.FBM.from_numpy(bad)
    for method in ir.METHODS:
        with pytest.raises(tpg._lib.TpgError) as e:
            X.impute_simple(method, 1)
        assert e.value.code == 3 and "object x is already imputed" in str(e.value)
        assert np.array_equal(X.to_numpy(), bad), method
    # unknown method: TPG_EINVAL from the C ABI (the Python wrapper refuses the name before that)
    rc = tpg._lib.lib.tpg_fbm_impute_simple(X.ctx.h, X.h, C.c_int(7), C.c_uint64(0), None)
    assert rc == 1
    rc = tpg._lib.lib.tpg_fbm_impute_simple(X.ctx.h, X.h, C.c_int(0), C.c_uint64(0), None)
    assert rc == 1
    assert np.array_equal(X.to_numpy(), bad)
    with pytest.raises(ValueError):
        X.impute_simple("mean2")
    # a second call on an imputed store is the reference's "already imputed" error
    Y = tpg.FBM.from_numpy(raw)
    tpg.gt_impute_simple(Y, "mode")
    assert np.array_equal(Y.code256, tpg.CODE_IMPUTE_PRED, equal_nan=True)
    after = Y.to_numpy()
    with pytest.raises(tpg._lib.TpgError, match="already imputed"):
        tpg.gt_impute_simple(Y, "mode")
    assert np.array_equal(Y.to_numpy(), after)
    # .bed-form store: no byte to hold 4 + v
    B = tpg.FBM.open_bed(os.path.join(fx.GOLDEN, "lobster/lobster.bed"), 176, 79)
    with pytest.raises(tpg._lib.TpgError) as e:
        B.impute_simple("mode")
    assert e.value.code == 3 and "tpg_view_impute" in str(e.value)


@pytest.mark.parametrize("n,m", [(130, 700), (1, 40), (257, 129), (5003, 300)])
def test_view_equals_store(tpg, n, m):
    rng = np.random.default_rng(n * 7 + m)
    raw = _raw_store(rng, n, m)
    for method in ir.METHODS:
        for code in (None, tpg.CODE_012):
            X = tpg.FBM.from_numpy(raw)
            v = tpg.View(X, code256=code).impute(method, 11)
            got = v.unpack()
            assert v.impute_report == ir.report(raw)
            X.impute_simple(method, 11)
            via_store = tpg.View(X, code256=tpg.CODE_IMPUTE_PRED).unpack()
            assert np.array_equal(got, via_store), method
            assert np.array_equal(got, ir.impute_codes(raw, method, 11)), method
            # the imputed view serves the per-locus sweeps like any other view
            lc = tpg.loci_counts(v)
            want = ir.impute_codes(raw, method, 11)
            assert np.array_equal(lc, np.stack([(want == g).sum(axis=0) for g in range(4)], axis=1))


def test_view_of_bed_stores_and_row_subsets(tpg):
    for name, n, m in (("related/families", 12, 961), ("lobster/lobster", 176, 79)):
        path = os.path.join(fx.GOLDEN, name + ".bed")
        geno = orc.read_bed(path, n, m)
        codes = np.where(geno < 3, geno, 3).astype(np.uint8)
        X = tpg.FBM.open_bed(path, n, m)
        for method in ir.METHODS:
            assert np.array_equal(tpg.View(X, code256=tpg.CODE_012).impute(method, 2).unpack(), ir.impute_codes(codes, method, 2)), (name, method)
        # the fill comes from the kept rows, and `random` is keyed by the kept position
        rows = np.arange(n, 0, -2, dtype=np.int32)
        cols = np.arange(2, m, 3, dtype=np.int32)
        sub = codes[rows - 1][:, cols - 1]
        for method in ir.METHODS:
            got = tpg.View(X, rows, cols, code256=tpg.CODE_012).impute(method, 2).unpack()
            assert np.array_equal(got, ir.impute_codes(sub, method, 2)), (name, method)
    # lobster has missing genotypes: the check above is not vacuous
    assert (codes == 3).any()


def _pca_panel(n, m, seed=21):
    raw = orc.synth_fbm(seed, n, m, npop=5, miss=0.02, imputed_bytes=False)
    assert raw.max() == 3 and (raw == 3).mean() > 0.01
    return np.asfortranarray(raw)


def test_pca_end_to_end(tpg):
    n, m, k = 300, 4000, 4
    raw = _pca_panel(n, m)
    X = tpg.FBM.from_numpy(raw)
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.gt_pca_partialSVD(X, k=k)
    assert e.value.code == 4  # TPG_ENUMERIC, as today
    ibs0, king0 = tpg.snp_ibs(X), tpg.snp_king(X)
    for method in ("mode", "random"):
        got = tpg.gt_pca_partialSVD(X, k=k, impute=method, impute_seed=9)
        assert np.array_equal(X.to_numpy(), raw)  # impute= works on the view: the store is as it was
        H = tpg.FBM.from_numpy(ir.store_bytes(raw, method, 9))  # imputed on the host
        want = tpg.gt_pca_partialSVD(H, k=k)
        assert np.array_equal(got["center"], want["center"]) and np.array_equal(got["scale"], want["scale"])
        print(method, "d rel", np.abs(got["d"] / want["d"] - 1).max(), "u", np.abs(_aligned(want["u"], got["u"]) - want["u"]).max(),
              "v", np.abs(_aligned(want["v"], got["v"]) - want["v"]).max())
        assert np.allclose(got["d"], want["d"], rtol=1e-8, atol=0)
        assert np.abs(_aligned(want["u"], got["u"]) - want["u"]).max() <= 1e-6
        assert np.abs(_aligned(want["v"], got["v"]) - want["v"]).max() <= 1e-6
        r = tpg.gt_pca_randomSVD(X, k=k, impute=method, impute_seed=9)
        assert np.array_equal(r["center"], want["center"]) and np.allclose(r["d"], want["d"], rtol=1e-3)
    # in place: the PCA of the imputed store is the same one, and the raw-byte analyses do not see the fills
    tpg.gt_impute_simple(X, "mode")
    again = tpg.gt_pca_partialSVD(X, k=k)
    want = tpg.gt_pca_partialSVD(tpg.FBM.from_numpy(ir.store_bytes(raw, "mode")), k=k)
    assert np.array_equal(again["center"], want["center"]) and np.allclose(again["d"], want["d"], rtol=1e-8, atol=0)
    assert np.array_equal(tpg.snp_ibs(X), ibs0, equal_nan=True)
    assert np.array_equal(tpg.snp_king(X), king0, equal_nan=True)


def _compare_pca(s, p, o, tol_d, tol_u):
    """center / scale identical to the resident run of the imputed view; d, u, v within the streamed bounds of
    tests/test_gpu_stream.py:_compare (1e-10 / 1e-8 under a budget, 1e-8 / 1e-6 without) of the resident run AND of the
    FP64 oracle on the host-imputed bytes"""
    assert np.array_equal(s["center"], p["center"]) and np.array_equal(s["scale"], p["scale"])
    assert s["square_frobenius"] == pytest.approx(p["square_frobenius"], rel=1e-12)
    for name, ref in (("resident", p), ("oracle", o)):
        fig = (np.abs(s["d"] / ref["d"] - 1).max(), np.abs(_aligned(ref["u"], s["u"]) - ref["u"]).max(),
               np.abs(_aligned(ref["v"], s["v"]) - ref["v"]).max())
        print("vs", name, "d %.3g u %.3g v %.3g" % fig)
        assert np.allclose(s["d"], ref["d"], rtol=tol_d, atol=0), name
        assert fig[1] <= tol_u and fig[2] <= tol_u, name


def _bed_payload(fbm):
    n, m = fbm.shape
    enc = np.array([3, 2, 0, 1], dtype=np.uint8)[fbm]  # FBM byte 0,1,2,3 -> bed code 11,10,00,01
    pad = np.zeros((4 * ((n + 3) // 4), m), dtype=np.uint8)
    pad[:n] = enc
    return (pad[0::4] | (pad[1::4] << 2) | (pad[2::4] << 4) | (pad[3::4] << 6)).T.copy()  # (m, bytes per SNP)


@pytest.mark.parametrize("source", ["bytes", "bed"])
@pytest.mark.parametrize("budget", [0, 700 << 10])
def test_streamed_pca_with_impute(tpg, source, budget):
    """`random` keyed by position in the selection: whatever the block plan (8 blocks without a budget, blocks of a few hundred
    loci under one), the streamed PCA is the resident PCA of the imputed view"""
    n, m, k = 260, 5001, 3
    raw = _pca_panel(n, m, seed=33)
    X = tpg.FBM.from_numpy(raw)
    p = tpg.gt_pca_partialSVD(X, k=k, impute="random", impute_seed=4)
    o = orc.gt_pca_partialSVD(ir.store_bytes(raw, "random", 4), None, None, k=k)
    if source == "bytes":
        st = tpg.Stream.from_numpy(raw, budget_bytes=budget)
    else:
        payload = _bed_payload(raw)
        st = tpg.Stream.from_bed_payload(payload, n, m, budget_bytes=budget)
    with pytest.raises(tpg._lib.TpgError) as e:
        st.run(k=k, code256_pca=tpg.CODE_012)
    assert e.value.code == 4  # unimputed: TPG_ENUMERIC
    s = st.run(k=k, impute="random", impute_seed=4, pairwise=("king",), loci_counts=True)
    if source == "bytes":
        assert s["report"]["blocks"] >= 8
    assert np.array_equal(s["king"], tpg.snp_king(X), equal_nan=True)  # the other outputs go on reading the raw store
    assert np.array_equal(s["loci_counts"][:, 3], (raw == 3).sum(axis=0))
    _compare_pca(s, p, o, 1e-10 if budget else 1e-8, 1e-8 if budget else 1e-6)
    # rows and columns selected: positions in the selection key the draw
    rows = np.arange(n, 0, -3, dtype=np.int32)
    cols = np.arange(5, m - 7, dtype=np.int32)
    s2 = st.run(rows, cols, k=k, impute="random", impute_seed=4)
    p2 = tpg.gt_pca_partialSVD(X, rows, cols, k=k, impute="random", impute_seed=4)
    assert np.array_equal(s2["center"], p2["center"]) and np.array_equal(s2["scale"], p2["scale"])
    assert np.allclose(s2["d"], p2["d"], rtol=1e-7, atol=0)
    st.close()


def test_stream_job_struct_sizes(tpg):
    n, m, k = 200, 1500, 2
    raw = _pca_panel(n, m, seed=3)
    st = tpg.Stream.from_numpy(raw, budget_bytes=0)
    lib, L = tpg._lib.lib, tpg._lib

    def job_for(size, garbage):
        buf = (C.c_uint8 * (C.sizeof(L.StreamJob) + 64))()
        C.memset(buf, 0xA5 if garbage else 0, len(buf))
        C.memset(buf, 0, L.STREAM_JOB_SIZE_V1)
        job = L.StreamJob.from_buffer(buf)
        out = dict(d=np.zeros(k), u=np.empty((n, k), order="F"), v=np.empty((m, k), order="F"), center=np.empty(m), scale=np.empty(m))
        code = np.ascontiguousarray(tpg.CODE_012)
        job.struct_size, job.k, job.code256_pca = size, k, code.ctypes.data
        for name, a in out.items():
            setattr(job, name, a.ctypes.data)
        return buf, job, out, code

    # the previous size with garbage behind it: runs, unimputed (the PCA meets the missing genotypes: TPG_ENUMERIC)
    buf, job, out, code = job_for(L.STREAM_JOB_SIZE_V1, True)
    assert job.impute_method != 0  # the garbage would ask for something if it were read
    assert lib.tpg_stream_run(st.ctx.h, st.h, C.byref(job), None) == 4
    # ... and on a store without missing genotypes it simply succeeds
    full = tpg.Stream.from_numpy(np.asfortranarray(ir.store_bytes(raw, "mode")), budget_bytes=0)
    buf2, job2, out2, code2 = job_for(L.STREAM_JOB_SIZE_V1, True)
    cip = np.ascontiguousarray(tpg.CODE_IMPUTE_PRED)
    job2.code256_pca = cip.ctypes.data
    assert lib.tpg_stream_run(full.ctx.h, full.h, C.byref(job2), None) == 0
    want = full.run(k=k)
    assert np.array_equal(out2["center"], want["center"]) and np.allclose(out2["d"], want["d"], rtol=1e-12)
    # this library's size: the fields are read
    buf3, job3, out3, code3 = job_for(C.sizeof(L.StreamJob), False)
    job3.impute_method, job3.impute_seed = 1, 0
    assert lib.tpg_stream_run(st.ctx.h, st.h, C.byref(job3), None) == 0
    assert np.array_equal(out3["center"], want["center"])
    job3.impute_method = 9
    assert lib.tpg_stream_run(st.ctx.h, st.h, C.byref(job3), None) == 1
    # with impute_method the PCA reads the raw store: CODE_IMPUTE_PRED as its table is a contradiction
    job3.impute_method, job3.code256_pca = 1, cip.ctypes.data
    assert lib.tpg_stream_run(st.ctx.h, st.h, C.byref(job3), None) == 1
    # any other size is refused
    for size in (C.sizeof(L.StreamJob) - 8, L.STREAM_JOB_SIZE_V1 - 8, C.sizeof(L.StreamJob) + 8, 0):
        b, j, o_, c_ = job_for(size, False)
        assert lib.tpg_stream_run(st.ctx.h, st.h, C.byref(j), None) == 1, size
    # several devices: the fields are not ignored -- refused
    mg = tpg.Multi(1)
    with pytest.raises(tpg._lib.TpgError) as e:
        st.run(k=k, impute="mode", multi=mg)
    assert e.value.code == 3
    mg.close()
    st.close()
    full.close()


def test_random_is_what_it_says(tpg):
    n, p = 20000, 0.3
    rng = np.random.default_rng(99)
    col = rng.binomial(2, p, size=n).astype(np.uint8)
    miss = np.zeros(n, dtype=bool)
    miss[rng.permutation(n)[: n // 2]] = True
    raw = np.asfortranarray(np.where(miss, 3, col).astype(np.uint8)[:, None])

    def run(seed):
        X = tpg.FBM.from_numpy(raw)
        X.impute_simple("random", seed)
        return X.to_numpy()[:, 0]

    a, b, c = run(12345), run(12345), run(54321)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert set(np.unique(a[miss])) <= {4, 5, 6} and np.array_equal(a[~miss], raw[~miss, 0])
    typed = raw[~miss, 0].astype(np.int64)
    p_hat = typed.sum() / (2 * typed.size)  # the frequency the draw uses: s / (2 t)
    mean = (a[miss].astype(np.int64) - 4).mean()
    se = np.sqrt(2 * p * (1 - p) / (n // 2))
    print("mean imputed", mean, "2 p_hat", 2 * p_hat, "2 p", 2 * p, "se", se)
    assert abs(mean - 2 * p) <= 5 * se
