"""GPU: blocked f2 (include/tpg.h "f2 blocks") against the restatement tests/f2_ref.py.

What is compared how.  cnt, ap_cnt and n_kept are integers: equality in every cell.  f2 and ap against the exact (Fraction)
route in EVERY cell within (4 L + 16) 2^-52 absolute, L the block's length (f2_ref.bound has the derivation; the bound is not
measured).  NaN exactly where the exact route has no value; the diagonal of f2 is +0.0 with its sign bit.  The one large case
(200 000 loci) is held against the float route at the same bound."""
import ctypes as C

import numpy as np
import pytest

from tests import f2_ref as fr
from tests import fixtures as fx

pytestmark = pytest.mark.gpu

NS = (13, 65, 200)
GS = (1, 3, 16, 17, 51, 64, 65)  # MFMA tile edges and the 64-group tile edge; 65: a second tile with one live row
M = 1000
_CASES = {}


def _tpg():
    import tidypopgen_amd as tpg

    return tpg


def _case(n, G, m=M, seed=None, hap=True):
    """one panel, its store on the device and its integer tables; made once per shape"""
    key = (n, G, m, seed, hap)
    if key not in _CASES:
        tpg = _tpg()
        codes, gid, pl, planted = fr.panel(1000 * n + G if seed is None else seed, n, m, G, hap=hap)
        X = tpg.FBM.from_numpy(np.asfortranarray(codes), code256=tpg.CODE_012)
        alt2, c = fr.group_tables(codes, gid, G, pl)
        _CASES[key] = dict(codes=codes, gid=gid, pl=pl, planted=planted, X=X, v=tpg.View(X), alt2=alt2, c=c, G=G, m=m)
    return _CASES[key]


def _blocks(m, planted):
    """every block of the issue: lengths 0, 1, 3, 4, 5 (the MFMA's k = 4), chunk - 1, chunk, chunk + 1, 2 chunk + 1, blocks whose
    loci are all filtered (the locus nobody is typed at; the monomorphic stretch for f2), two overlapping blocks, the whole view"""
    K = _tpg().F2_CHUNK_LOCI
    assert K > 1
    lo, hi, at = [], [], 7
    for L in (0, 1, 3, 4, 5, K - 1, K, K + 1, 2 * K + 1):
        lo.append(at)
        hi.append(at + L)
        at += L + 2
    lo += [planted["untyped"], planted["mono"][0], m // 2 - 40, m // 2 - 3, 0, m, 0]
    hi += [planted["untyped"] + 1, planted["mono"][1], m // 2 + 30, m // 2 + 90, m, m, 0]
    return np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)


def _run(cs, lo, hi, v=None, gid="case", pl="case", **kw):
    tpg = _tpg()
    gid = cs["gid"] if isinstance(gid, str) else gid
    pl = cs["pl"] if isinstance(pl, str) else pl
    return tpg.f2_blocks(cs["v"] if v is None else v, gid, cs["G"], lo, hi, ploidy=pl, **kw)


def _api_kw(pr):
    return dict(maxmiss=pr["maxmiss"], minmaf=pr["minmaf"], maxmaf=pr["maxmaf"], minac2=pr["minac2"], poly_only=pr["poly_only"],
                apply_corr=pr["apply_corr"], keep=pr["keep"])


def _assert_equal_exact(got, ex, lo, hi, tag=""):
    G = got["f2"].shape[0]
    assert np.array_equal(got["counts"], ex["cnt"]), tag
    assert np.array_equal(got["ap_counts"], ex["ap_cnt"]), tag
    assert np.array_equal(got["block_lengths"], ex["n_kept"]), tag
    w_f2, w_ap = fr.max_excess(got["f2"], ex["f2"], lo, hi), fr.max_excess(got["ap"], ex["ap"], lo, hi)
    print(f"{tag} worst |got - exact| / bound: f2 {w_f2:.4f} ap {w_ap:.4f}")
    assert w_f2 <= 1.0 and w_ap <= 1.0, (tag, w_f2, w_ap)
    d = got["f2"][np.arange(G), np.arange(G), :]
    live = got["counts"][np.arange(G), np.arange(G), :] > 0
    assert np.all(d[live] == 0.0) and not np.signbit(d[live]).any() and np.isnan(d[~live]).all(), tag
    assert not np.signbit(got["f2"][np.isnan(got["f2"])]).any(), tag
    for k in ("f2", "ap"):  # symmetric bit for bit
        assert np.array_equal(got[k].view(np.uint64), np.transpose(got[k], (1, 0, 2)).copy(order="F").view(np.uint64)), (tag, k)


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("n", NS)
def test_every_cell_against_the_exact_route(n, G):
    cs = _case(n, G)
    lo, hi = _blocks(cs["m"], cs["planted"])
    pr = fr.params(maxmiss=1.0)  # the panel has a group nobody belongs to: the default maxmiss = 0 would drop every locus
    ex = fr.blocks_exact(cs["alt2"], cs["c"], lo, hi, pr)
    got = _run(cs, lo, hi, **_api_kw(pr))
    _assert_equal_exact(got, ex, lo, hi, f"n={n} G={G}")
    # the planted things are there and do what they should
    assert (cs["c"] % 2 == 1).any() and (cs["c"] == 1).any()  # pseudohaploids: odd c, and c = 1
    b_unt, b_mono = 9, 10
    assert ex["n_kept"][b_unt] == 0 and (got["counts"][:, :, b_unt] == 0).all() and np.isnan(got["f2"][:, :, b_unt]).all()
    assert ex["n_kept"][b_mono] > 0 and (got["counts"][:, :, b_mono] == 0).all() and np.isnan(got["f2"][:, :, b_mono]).all()
    assert (got["ap_counts"][:, :, b_mono] > 0).any()  # poly_only = "f2": ap keeps the monomorphic loci
    if G >= 3 and n >= G + 1:
        assert np.isnan(got["f2"][G - 1, :, :]).all() and (got["counts"][:, G - 1, :] == 0).all()  # the empty group
        assert np.isfinite(got["f2"][G - 2, 0, 13])  # the singleton group: max(1, c - 1)
    assert (got["counts"][:, :, 0] == 0).all() and np.isnan(got["ap"][:, :, 0]).all()  # an empty block


FILTERS = [dict(), dict(maxmiss=0.06), dict(maxmiss=1.0, minmaf=0.11, maxmaf=0.37), dict(maxmiss=1.0, minac2=1),
           dict(maxmiss=1.0, keep="random"), dict(maxmiss=1.0, poly_only=0), dict(maxmiss=1.0, poly_only=fr.POLY_AP),
           dict(maxmiss=1.0, poly_only=fr.POLY_F2 | fr.POLY_AP), dict(maxmiss=1.0, apply_corr=0)]


@pytest.mark.parametrize("G", [2, 17])
@pytest.mark.parametrize("flt", FILTERS, ids=lambda f: ",".join(f"{k}={v}" for k, v in f.items()) or "defaults")
def test_each_filter_alone(flt, G):
    """G = 2 has no empty group (the defaults and minac2 keep loci there), G = 17 has one, a singleton and a pseudohaploid"""
    cs = _case(65, G, m=1200, seed=77 + G)
    lo, hi = _blocks(cs["m"], cs["planted"])
    flt = dict(flt)
    if flt.get("keep") == "random":
        flt["keep"] = (np.random.default_rng(5).random(cs["m"]) < 0.6).astype(np.uint8)
    pr = fr.params(**flt)
    ex = fr.blocks_exact(cs["alt2"], cs["c"], lo, hi, pr)
    got = _run(cs, lo, hi, **_api_kw(pr))
    _assert_equal_exact(got, ex, lo, hi, f"G={G} {sorted(flt)}")
    base = fr.blocks_exact(cs["alt2"], cs["c"], lo, hi, fr.params(maxmiss=1.0))
    whole = 13  # the block [0, m)
    if flt and flt != dict(maxmiss=1.0):  # the filter bites: something differs from the unfiltered run
        differs = (not np.array_equal(ex["cnt"], base["cnt"]) or not np.array_equal(ex["ap_cnt"], base["ap_cnt"])
                   or ex["f2"][0, 1, whole] != base["f2"][0, 1, whole])
        assert differs, flt
    if G == 2:
        assert ex["n_kept"][whole] > 0, flt  # and it does not drop everything


def test_ploidy_vector_and_all_diploid_differ_and_both_match():
    cs = _case(65, 17, m=1200, seed=94)
    lo, hi = _blocks(cs["m"], cs["planted"])
    pr = fr.params(maxmiss=1.0)
    assert cs["pl"] is not None and (cs["pl"] == 1.0).sum() == 1
    dip_alt2, dip_c = fr.group_tables(cs["codes"], cs["gid"], 17, None)
    got_h = _run(cs, lo, hi, **_api_kw(pr))
    got_d = _run(cs, lo, hi, pl=None, **_api_kw(pr))
    _assert_equal_exact(got_h, fr.blocks_exact(cs["alt2"], cs["c"], lo, hi, pr), lo, hi, "pseudohaploid")
    _assert_equal_exact(got_d, fr.blocks_exact(dip_alt2, dip_c, lo, hi, pr), lo, hi, "all diploid")
    assert not np.array_equal(got_h["f2"], got_d["f2"], equal_nan=True)
    got_2 = _run(cs, lo, hi, pl=np.full(65, 2.0), **_api_kw(pr))  # a ploidy vector of twos is the NULL case
    assert all(np.array_equal(got_2[k], got_d[k], equal_nan=True) for k in got_d)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def test_a_cell_depends_on_its_block_alone():
    cs = _case(65, 65)
    lo, hi = _blocks(cs["m"], cs["planted"])
    kw = _api_kw(fr.params(maxmiss=1.0))
    a = _run(cs, lo, hi, **kw)
    again = _run(cs, lo, hi, **kw)
    perm = np.random.default_rng(1).permutation(len(lo))
    shuffled = _run(cs, np.r_[lo[perm], lo], np.r_[hi[perm], hi], **kw)  # another place in a longer list
    for k in ("f2", "counts", "ap", "ap_counts"):
        assert np.array_equal(_bits(a[k]), _bits(again[k])), k
        assert np.array_equal(_bits(a[k][:, :, perm]), _bits(shuffled[k][:, :, :len(lo)])), k
        assert np.array_equal(_bits(a[k]), _bits(shuffled[k][:, :, len(lo):])), k
    for b in (8, 12, 13):  # alone
        one = _run(cs, lo[b:b + 1], hi[b:b + 1], **kw)
        for k in ("f2", "counts", "ap", "ap_counts"):
            assert np.array_equal(_bits(one[k][:, :, 0]), _bits(a[k][:, :, b])), (k, b)
        assert one["block_lengths"][0] == a["block_lengths"][b]


def test_device_outputs_and_inputs_equal_host_ones():
    tpg = _tpg()
    cs = _case(65, 17)
    lo, hi = _blocks(cs["m"], cs["planted"])
    keep = (np.random.default_rng(8).random(cs["m"]) < 0.7).astype(np.uint8)
    kw = _api_kw(fr.params(maxmiss=1.0, keep=keep))
    host = _run(cs, lo, hi, **kw)
    dev = _run(cs, lo, hi, on_device=True, **kw)
    ctx = cs["v"].ctx
    try:
        for k in ("f2", "counts", "ap", "ap_counts"):
            back = np.zeros_like(host[k])
            tpg._lib.check(tpg._lib.lib.tpg_dev_to_host(ctx.h, C.c_void_p(back.ctypes.data), dev[k], C.c_size_t(back.nbytes)))
            assert np.array_equal(_bits(back), _bits(host[k])), k
    finally:
        for k in ("f2", "counts", "ap", "ap_counts"):
            ctx.dev_free(dev[k])
    assert np.array_equal(dev["block_lengths"], host["block_lengths"])
    no_ap = _run(cs, lo, hi, afprod=False, **kw)  # outputs may be NULL
    assert set(no_ap) == {"f2", "counts", "block_lengths"} and np.array_equal(_bits(no_ap["f2"]), _bits(host["f2"]))
    lib = tpg._lib.lib
    pr = tpg._lib.F2Params()
    tpg._lib.check(lib.tpg_f2_params_default(C.byref(pr)))
    pr.maxmiss = 1.0
    pr.keep = keep.ctypes.data
    only_ap = np.zeros_like(host["ap"])
    gid = np.ascontiguousarray(cs["gid"], dtype=np.int32)
    tpg._lib.check(lib.tpg_f2_blocks(ctx.h, cs["v"].h, C.c_void_p(gid.ctypes.data), 17, C.c_void_p(cs["pl"].ctypes.data), C.byref(pr),
                                     C.c_void_p(lo.ctypes.data), C.c_void_p(hi.ctypes.data), C.c_int64(len(lo)), None, None,
                                     C.c_void_p(only_ap.ctypes.data), None, None))
    assert np.array_equal(_bits(only_ap), _bits(host["ap"]))


def test_subsets_and_a_permutation_of_the_individuals():
    tpg = _tpg()
    cs = _case(65, 17)
    rng = np.random.default_rng(3)
    rows, cols = np.sort(rng.permutation(65)[:41]), np.sort(rng.permutation(cs["m"])[:613])
    v = tpg.View(cs["X"], rows + 1, cols + 1)
    lo, hi = np.array([0, 100, 0], dtype=np.int64), np.array([613, 133, 17], dtype=np.int64)
    pr = fr.params(maxmiss=1.0)
    alt2, c = fr.group_tables(cs["codes"][np.ix_(rows, cols)], cs["gid"][rows], 17, cs["pl"][rows])
    got = _run(cs, lo, hi, v=v, gid=cs["gid"][rows], pl=cs["pl"][rows], **_api_kw(pr))
    _assert_equal_exact(got, fr.blocks_exact(alt2, c, lo, hi, pr), lo, hi, "subset")
    perm = rng.permutation(65)
    lo, hi = _blocks(cs["m"], cs["planted"])
    a = _run(cs, lo, hi, **_api_kw(pr))
    b = _run(cs, lo, hi, v=tpg.View(cs["X"], perm + 1), gid=cs["gid"][perm], pl=cs["pl"][perm], **_api_kw(pr))
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_argument_errors():
    tpg = _tpg()
    cs = _case(13, 3)
    m = cs["m"]
    ok = dict(maxmiss=1.0)
    for lo, hi in (([5], [4]), ([0], [m + 1]), ([-1], [3]), ([0, m + 1], [3, m + 1])):
        with pytest.raises(tpg._lib.TpgError) as e:
            _run(cs, np.array(lo, dtype=np.int64), np.array(hi, dtype=np.int64), **ok)
        assert e.value.code == 1
    lo, hi = np.array([0], dtype=np.int64), np.array([m], dtype=np.int64)
    with pytest.raises(ValueError, match="minac2"):
        _run(cs, lo, hi, minac2=2, **ok)
    lib = tpg._lib.lib
    pr = tpg._lib.F2Params()
    tpg._lib.check(lib.tpg_f2_params_default(C.byref(pr)))
    assert (pr.maxmiss, pr.minmaf, pr.maxmaf, pr.minac2, pr.poly_only, pr.apply_corr, pr.keep) == (0.0, 0.0, 0.5, 0, 1, 1, None)
    gid = np.ascontiguousarray(cs["gid"], dtype=np.int32)
    out = np.zeros((3, 3, 1), order="F")

    def call(G, params):
        return lib.tpg_f2_blocks(cs["v"].ctx.h, cs["v"].h, C.c_void_p(gid.ctypes.data), G, None, params, C.c_void_p(lo.ctypes.data),
                                 C.c_void_p(hi.ctypes.data), C.c_int64(1), C.c_void_p(out.ctypes.data), None, None, None, None)

    pr.minac2 = 2
    assert call(3, C.byref(pr)) == 1  # TPG_EINVAL
    pr.minac2 = 0
    max_groups = 4096  # TPG_F2_MAX_GROUPS
    assert call(max_groups + 1, C.byref(pr)) == 1 and call(0, C.byref(pr)) == 1
    pr.poly_only = 4
    assert call(3, C.byref(pr)) == 1
    assert call(3, None) == 0  # params = NULL: the defaults
    want = _run(cs, lo, hi, pl=None)
    assert np.array_equal(_bits(out), _bits(want["f2"]))
    empty = _run(cs, lo[:0], hi[:0], **ok)  # nb = 0: nothing written
    assert empty["f2"].shape == (3, 3, 0) and len(empty["block_lengths"]) == 0
    with pytest.raises(tpg._lib.TpgError):
        _run(cs, lo, hi, gid=np.full(13, 3, dtype=np.int32), **ok)
    with pytest.raises(tpg._lib.TpgError):
        _run(cs, lo, hi, pl=np.full(13, 3.0), **ok)


def test_200000_loci_against_the_float_route():
    """the largest offsets of the suite: 200 000 loci, 51 groups with a pseudohaploid (a count table of 3 x 200 000 x 128 words),
    ~150 blocks of ~1 300 loci from f2_block_ranges on a synthetic map; against the float route at the bound of the others"""
    tpg = _tpg()
    n, G, m = 65, 51, 200_000
    cs = _case(n, G, m=m, seed=2024)
    rng = np.random.default_rng(12)
    chrom = np.sort(rng.integers(1, 23, size=m))
    dist = np.concatenate([np.sort(rng.uniform(0, 0.34, size=int((chrom == k).sum()))) for k in range(1, 23)])
    lo, hi = tpg.f2_block_ranges(chrom, dist, 0.05)
    assert 120 <= len(lo) <= 180 and lo[0] == 0 and hi[-1] == m and np.array_equal(lo[1:], hi[:-1])
    pr = fr.params(maxmiss=1.0)
    got = _run(cs, lo, hi, **_api_kw(pr))
    want = fr.blocks_float(cs["alt2"], cs["c"], lo, hi, pr)
    assert np.array_equal(got["counts"], want["cnt"]) and np.array_equal(got["ap_counts"], want["ap_cnt"])
    assert np.array_equal(got["block_lengths"], want["n_kept"]) and got["block_lengths"].sum() > 0.9 * m
    bd = fr.bound(lo, hi)[None, None, :]
    for k in ("f2", "ap"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        err = np.nanmax(np.abs(got[k] - want[k]) / bd)
        print(f"200000 loci, {len(lo)} blocks: worst |{k} - float route| / bound = {err:.4f}")
        assert err <= 1.0, (k, err)


def test_gt_extract_f2_on_the_lobster_panel_and_f4_on_top():
    tpg = _tpg()
    codes = np.asarray(fx.lobster_fbm())
    n, m = codes.shape
    assert (n, m) == (176, 79)
    G = 6
    gid = (np.arange(n) * G // n).astype(np.int32)
    chrom = np.repeat([1, 2, 3], [30, 30, 19])
    dist = np.concatenate([np.arange(30) * 0.011, np.arange(30) * 0.02, np.arange(19) * 0.004])
    X = tpg.FBM.from_numpy(np.asfortranarray(codes), code256=tpg.CODE_012)
    got = tpg.gt_extract_f2(X, None, None, gid, G, chrom, genetic_dist=dist, blgsize=0.05, maxmiss=0.2)
    lo, hi = fr.block_ranges(chrom, dist, 0.05)
    assert np.array_equal(got["lo"], lo) and np.array_equal(got["hi"], hi) and len(lo) >= 8
    alt2, c = fr.group_tables(codes, gid, G)
    pr = fr.params(maxmiss=0.2)
    _assert_equal_exact(got, fr.blocks_exact(alt2, c, lo, hi, pr), lo, hi, "lobster")
    assert got["block_lengths"].sum() > 40
    with pytest.raises(TypeError, match="unsupported"):
        tpg.gt_extract_f2(X, None, None, gid, G, chrom, genetic_dist=dist, fst=True)
    with pytest.raises(ValueError):
        tpg.gt_extract_f2(X, None, None, gid, G, chrom, genetic_dist=dist, minac2=2)
    quads = np.array([[0, 1, 2, 3], [0, 5, 2, 4], [2, 0, 2, 1]])
    r4 = tpg.f4_from_f2_blocks(got["f2"], got["block_lengths"], quads)
    for q in range(3):
        est, se, g = fr.f4_jackknife(got["f2"], got["block_lengths"], quads[q])
        assert r4["est"][q] == est and r4["se"][q] == se and r4["n_blocks"][q] == g and g >= 2
        assert np.isfinite(r4["z"][q])
    r3 = tpg.f3_from_f2_blocks(got["f2"], got["block_lengths"], [[2, 0, 1]])
    assert r3["est"][0] == r4["est"][2] and r3["se"][0] == r4["se"][2]
