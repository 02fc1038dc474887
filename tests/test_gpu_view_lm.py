"""GPU: the locus-major layout LM of a view (csrc/common.h, csrc/devfrag.h: tpg_lm_piece).

The fast pack kernel writes the second (imputed) member of View.pair as LM instead of L: the class Gram's gather and the
loadings kernel of the PCA read it as it is, and every other consumer gets L rebuilt from it (tpg_view_need_L).  LM is a
permutation of L's 16-byte pieces, so everything below is compared BIT FOR BIT with a view of the same store packed on its own
(L, and LM only as a per-call scratch copy); only the streamed run, which adds its blocks in another order, is held to the
bounds tests/test_gpu_stream.py uses for streamed against resident.

Shapes: twice Q = ceil(n / 128) = 1, 1, 2, 3, 4, 5, 6 (the transposition works on groups of four chunks, the loadings on pairs: a
lone chunk, an odd last pair, a partial last group, a whole group, a group and one), n never a multiple of 32, m never a
multiple of 32 (padding loci in the last tile; 128 is one whole locus group).  Bytes as the benchmark synthesises them: 2 %
missing kept as imputed bytes.  big_SVD stops on a locus without variance, so a monomorphic locus gets one 0 and one 2 in its
first two rows; a single individual has no PCA at all, and there both routes must refuse alike."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

# a byte store takes the fast pack kernel -- the one that writes LM -- when its columns are 8-byte aligned (n a multiple of 8);
# any other n takes the generic kernel, which gives the pair's second member L as before
SHAPES_FAST = [(8, 33), (40, 95), (136, 128), (296, 1000), (408, 161), (520, 257), (648, 4099)]
SHAPES = [(1, 33), (37, 95), (130, 128), (300, 1000), (401, 161), (513, 257), (643, 4099)] + SHAPES_FAST


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


def _bytes(n, m, imputed_bytes=True):
    """the bench's bytes at this shape, every locus polymorphic through CODE_IMPUTE_PRED (n >= 2)"""
    fbm = orc.synth_fbm(7 + n, n, m, npop=min(n, 5), miss=0.02, imputed_bytes=imputed_bytes)
    if n >= 2:
        # bytes 4 + g read as g through CODE_IMPUTE_PRED; a .bed store's second table reads "missing" as dosage 0
        dos = np.where(fbm >= 4, fbm - 4, fbm) if imputed_bytes else np.where(fbm == 3, 0, fbm)
        alt = dos.astype(np.int64).sum(axis=0)
        mono = (alt == 0) | (alt == 2 * n)
        fbm[0, mono], fbm[1, mono] = 0, 2
    return fbm


def _svd(v, k):
    """tpg_pca_partial_svd on a view"""
    from tidypopgen_amd.api import _ptr, check, lib

    d, u, vl = np.zeros(k), np.zeros((v.n, k), order="F"), np.zeros((v.m, k), order="F")
    center, scale, fro = np.zeros(v.m), np.zeros(v.m), C.c_double()
    check(lib.tpg_pca_partial_svd(v.ctx.h, v.h, k, _ptr(d), _ptr(u), _ptr(vl), _ptr(center), _ptr(scale), C.byref(fro)))
    return dict(d=d, u=u, v=vl, center=center, scale=scale, square_frobenius=np.array([fro.value]))


def _svd_or_code(tpg, v, k):
    try:
        return _svd(v, k)
    except tpg._lib.TpgError as e:
        return e.code


def _same_pca(tpg, pair_view, single_view, k):
    a, b = _svd_or_code(tpg, pair_view, k), _svd_or_code(tpg, single_view, k)
    if isinstance(b, int) or isinstance(a, int):
        assert a == b, (a, b)  # refused alike (a single individual: no variance anywhere)
        return False
    for key in ("d", "u", "v", "center", "scale", "square_frobenius"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    return True


def _subsets(n, m):
    rng = np.random.default_rng(n * 31 + m)
    rows = (np.sort(rng.permutation(n)[: n - 5]) + 1).astype(np.int32)
    cols = (np.sort(rng.permutation(m)[: m - 37]) + 1).astype(np.int32)
    return rows, cols


@pytest.mark.parametrize("gram", ["model", "classes"])
@pytest.mark.parametrize("n,m", SHAPES)
def test_pca_through_the_pair_equals_pca_through_a_single_view(tpg, monkeypatch, n, m, gram):
    """d, u, v, center, scale and the Frobenius term, whichever Gram kernel the cost model picks (where it declines the class
    path the digit kernel reads T, made from L, made from LM) and with the class path forced (the gather reads LM)."""
    if gram == "classes":
        monkeypatch.setenv("TPG_GRAM_CLASSES", "1")
    X = tpg.FBM.from_numpy(_bytes(n, m))
    k = min(n, 3)
    vb = tpg.View.pair(X)[1]
    sb = tpg.View(X, code256=tpg.CODE_IMPUTE_PRED)
    ran = _same_pca(tpg, vb, sb, k)
    assert ran == (n >= 2)
    if ran:  # the same view once more: whatever the first call left on it (L beside LM on the digit route) changes nothing
        assert _same_pca(tpg, vb, sb, k)


@pytest.mark.parametrize("gram", ["model", "classes"])
def test_pca_pair_with_subsets(tpg, monkeypatch, gram):
    """colInd alone keeps the fast pack kernel (LM through a column gather); rowInd takes the generic kernel, which writes L"""
    if gram == "classes":
        monkeypatch.setenv("TPG_GRAM_CLASSES", "1")
    n, m = 296, 1000
    fbm = _bytes(n, m)
    X = tpg.FBM.from_numpy(fbm)
    rows, cols = _subsets(n, m)
    for r, c in ((None, cols), (rows, cols), (rows, None)):
        sel = fbm[np.ix_(np.arange(n) if r is None else r - 1, np.arange(m) if c is None else c - 1)]
        alt = np.where(sel >= 4, sel - 4, sel).astype(np.int64).sum(axis=0)
        keep = (alt > 0) & (alt < 2 * sel.shape[0])
        cc = (np.arange(1, m + 1, dtype=np.int32) if c is None else c)[keep]
        vb, sb = tpg.View.pair(X, r, cc)[1], tpg.View(X, r, cc, code256=tpg.CODE_IMPUTE_PRED)
        assert _same_pca(tpg, vb, sb, 4)
        assert np.array_equal(vb.unpack(), sb.unpack())


def _bed_file(fbm, path):
    """an FBM (bytes 0 / 1 / 2 / 3 = missing) as a PLINK .bed file; the unused bit pairs of a SNP's last byte are garbage"""
    n, m = fbm.shape
    enc = np.array([3, 2, 0, 1], dtype=np.uint8)[fbm]  # FBM byte 0,1,2,3 -> bed code 11,10,00,01
    pad = np.vstack([enc, np.full(((-n) % 4, m), 2, dtype=np.uint8)])
    bed = (pad[0::4] | (pad[1::4] << 2) | (pad[2::4] << 4) | (pad[3::4] << 6)).T.copy()  # (m, bytes per SNP)
    with open(path, "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]) + bed.tobytes())


@pytest.mark.parametrize("n,m", [(37, 95), (513, 257)])
def test_pca_pair_from_a_bed_store(tpg, tmp_path, n, m):
    """the .bed front end of the fast pack kernel writes LM too: n not a multiple of 4 or 16, the last byte of a SNP partly
    padding; a .bed store has no imputed bytes, so the second table reads a missing genotype as dosage 0"""
    fbm = _bytes(n, m, imputed_bytes=False)
    path = str(tmp_path / "x.bed")
    _bed_file(fbm, path)
    Xb, Xf = tpg.FBM.open_bed(path, n, m), tpg.FBM.from_numpy(fbm)
    code_imp = np.array([0, 1, 2, 0] + [np.nan] * 252)
    vb = tpg.View.pair(Xb, None, None, tpg.CODE_012, code_imp)[1]
    sb = tpg.View(Xb, code256=code_imp)
    sf = tpg.View(Xf, code256=code_imp)
    assert _same_pca(tpg, vb, sb, 3)
    assert _same_pca(tpg, vb, sf, 3)
    assert np.array_equal(vb.unpack(), sf.unpack())
    assert np.array_equal(tpg.loci_counts(vb), tpg.loci_counts(sf))


@pytest.mark.parametrize("n,m", SHAPES)
def test_the_derived_L_is_the_packed_L(tpg, n, m):
    """consumers that read L (or T, which is made from L) on the LM-only member of a pair against the single view: the codes
    themselves, per-locus and per-group counts, per-individual counts, imputation, and the pairwise {V, D} sums"""
    fbm = _bytes(n, m)
    X = tpg.FBM.from_numpy(fbm)
    gid = (np.arange(n) % 3).astype(np.int32)
    G = int(gid.max()) + 1

    def fresh():  # every consumer meets a view that holds LM and nothing else
        return tpg.View.pair(X)[1]

    sb = tpg.View(X, code256=tpg.CODE_IMPUTE_PRED)
    codes = sb.unpack()
    assert np.array_equal(codes, np.where(fbm >= 4, fbm - 4, fbm))
    assert np.array_equal(fresh().unpack(), codes)  # (T against L on the device, then T: both from LM)
    assert np.array_equal(tpg.loci_counts(fresh()), tpg.loci_counts(sb))
    assert np.array_equal(tpg.grouped_alt_freq_dip_pseudo_cpp(fresh(), gid, G, np.full(n, 2.0), True),
                          tpg.grouped_alt_freq_dip_pseudo_cpp(sb, gid, G, np.full(n, 2.0), True))
    assert np.array_equal(tpg.indiv_counts(fresh()), tpg.indiv_counts(sb))
    # imputation wants missing genotypes: a pair of two RAW views, the second of which is the locus-major one
    rb, rs = tpg.View.pair(X, None, None, tpg.CODE_012, tpg.CODE_012)[1], tpg.View(X, code256=tpg.CODE_012)
    for method in ("mode", "random"):
        ib, isg = rb.impute(method, seed=5), rs.impute(method, seed=5)
        assert ib.impute_report == isg.impute_report
        assert np.array_equal(ib.unpack(), isg.unpack()), method
        rb = tpg.View.pair(X, None, None, tpg.CODE_012, tpg.CODE_012)[1]
    # tpg_view_need_T (from L, from LM), the FP4 operands from T, then the {V, D} kernel
    rb = tpg.View.pair(X, None, None, tpg.CODE_012, tpg.CODE_012)[1]
    pb, ps = tpg.Pairwise(X.ctx, n), tpg.Pairwise(X.ctx, n)
    pb.accumulate(rb, products=tpg.PW_V | tpg.PW_D)
    ps.accumulate(rs, products=tpg.PW_V | tpg.PW_D)
    cb, cs = pb.counts(("as_num", "as_den")), ps.counts(("as_num", "as_den"))
    for key in cs:
        assert np.array_equal(cb[key], cs[key]), key


def _aligned(a, b):
    """columns of b with the signs of a"""
    return b * np.sign((a * b).sum(axis=0))


def test_streamed_pca_in_two_blocks_agrees_with_the_resident_one(tpg, monkeypatch):
    """Stream.run packs every block as a pair, so its PCA views are locus-major: two blocks of 512 loci of the 296 x 1000
    panel against the resident PCA, at the bounds tests/test_gpu_stream.py (_compare) holds streamed against resident to."""
    n, m, k = 296, 1000, 4
    fbm = _bytes(n, m)
    X = tpg.FBM.from_numpy(fbm)
    p = tpg.gt_pca_partialSVD(X, None, None, k=k)
    monkeypatch.setenv("TPG_STREAM_BLOCKS", "2")
    st = tpg.Stream.from_numpy(fbm)
    s = st.run(k=k)
    assert s["report"]["blocks"] == 2
    assert np.array_equal(s["center"], p["center"]) and np.array_equal(s["scale"], p["scale"])
    assert s["square_frobenius"] == pytest.approx(p["square_frobenius"], rel=1e-12)
    assert np.allclose(s["d"], p["d"], rtol=1e-7, atol=0)
    assert np.abs(_aligned(p["u"], s["u"]) - p["u"]).max() <= 1e-6
    st.close()
