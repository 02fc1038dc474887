"""GPU: the argument checks every grouped entry point shares (the class plan of csrc/loci.hip: make_class_plan,
tpg_check_group_ids, tpg_require_diploid), the range check of the windowed ones (tpg_check_ranges) and the owner of the cached
per-class counts (tpg_view::gc_buf), all through the C ABI.

Shapes: n = 130 individuals cross the 128-individual block (Q = 2), m = 33 loci cross a 32-locus tile, G = 3 groups, and
G = 33 where the padded class count goes from 32 to 64."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

N, M, G = 130, 33, 3
OK, EINVAL, EUNSUPPORTED = 0, 1, 3
HUDSON, WC84 = 0, 2


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


@pytest.fixture(scope="module")
def fbm():
    return orc.synth_fbm(23, N, M, npop=G, miss=0.05)


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _gid(g=G):
    return (np.arange(N) % g).astype(np.int32)


def _pairs(tpg, g):
    """2 x P, 1-based, column-major as the C ABI reads it"""
    return np.asfortranarray(tpg.combn2(g), dtype=np.int32)


LO = np.array([0, 5, 32, 10], dtype=np.int64)   # the whole range, an empty window, the last locus alone, an inner one
HI = np.array([33, 5, 33, 20], dtype=np.int64)


def _entries(tpg, v):
    """name -> call(gid, ngroups, ploidy, method) -> return code; outputs sized for G groups"""
    lib, ctx = tpg._lib.lib, v.ctx
    mg = np.zeros((M, 2 * G), order="F")
    o = [np.zeros((M, G), order="F") for _ in range(4)]
    i3 = np.zeros((3, M, G), dtype=np.int32)
    g10, ov = np.zeros((M, 10), order="F"), np.zeros(10)
    pairs = _pairs(tpg, G)
    P = pairs.shape[1]
    tot = np.zeros(P)
    dg, w = np.zeros(G), np.zeros((len(LO), G), order="F")
    f2 = np.zeros((G, G, len(LO)), order="F")
    A = np.asfortranarray(np.random.default_rng(1).random((N, N)))
    mean = np.zeros((G, G), order="F")
    return {
        "grouped_alt_freq": lambda gid, g, pl, method: lib.tpg_grouped_alt_freq_dip_pseudo(
            ctx.h, v.h, _p(gid), C.c_int(g), _p(pl), C.c_int(0), _p(mg)),
        "grouped_missingness": lambda gid, g, pl, method: lib.tpg_grouped_missingness(ctx.h, v.h, _p(gid), C.c_int(g), _p(o[0])),
        "grouped_summaries": lambda gid, g, pl, method: lib.tpg_grouped_summaries_dip_pseudo(
            ctx.h, v.h, _p(gid), C.c_int(g), _p(pl), _p(o[0]), _p(o[1]), _p(o[2]), _p(o[3])),
        "grouped_pi": lambda gid, g, pl, method: lib.tpg_gt_grouped_pi_diploid(ctx.h, v.h, _p(gid), C.c_int(g), _p(o[0]), _p(o[1])),
        "grouped_genotype_counts": lambda gid, g, pl, method: lib.tpg_grouped_genotype_counts(ctx.h, v.h, _p(gid), C.c_int(g), _p(i3)),
        "pop_global_stats": lambda gid, g, pl, method: lib.tpg_pop_global_stats(ctx.h, v.h, _p(gid), C.c_int(g), _p(pl), _p(g10), _p(ov)),
        "pop_basic_stats": lambda gid, g, pl, method: lib.tpg_pop_basic_stats(
            ctx.h, v.h, _p(gid), C.c_int(g), _p(pl), C.c_int(1), _p(o[0]), _p(dg)),
        "gt_grouped_hwe": lambda gid, g, pl, method: lib.tpg_gt_grouped_hwe(ctx.h, v.h, _p(gid), g, 1, _p(o[0])),
        "pairwise_pop_fst": lambda gid, g, pl, method: lib.tpg_pairwise_pop_fst(
            ctx.h, v.h, _p(gid), C.c_int(g), _p(pl), C.c_int(method), _p(pairs), C.c_int(P), C.c_int(0), C.c_int(0), _p(tot), None, None),
        "pop_tajimas_d": lambda gid, g, pl, method: lib.tpg_pop_tajimas_d(ctx.h, v.h, _p(gid), g, _p(pl), _p(dg), None, None),
        "windows_pop_tajimas_d": lambda gid, g, pl, method: lib.tpg_windows_pop_tajimas_d(
            ctx.h, v.h, _p(gid), g, _p(pl), _p(LO), _p(HI), None, len(LO), 1, _p(w), None, None, None),
        "f2_blocks": lambda gid, g, pl, method: lib.tpg_f2_blocks(
            ctx.h, v.h, _p(gid), g, _p(pl), None, _p(LO), _p(HI), len(LO), _p(f2), None, None, None, None),
        "block_means": lambda gid, g, pl, method: lib.tpg_block_means(
            ctx.h, _p(A), C.c_int64(N), _p(gid), C.c_int(g), C.c_int(1), _p(mean), None),
    }


# The return code of every entry point for: a group id equal to G at index 5; ngroups = 0; one ploidy of 3.0; one ploidy of
# 1.0 (None: the entry point takes no ploidy).  Read off the source before the checks were shared.
CODES = {
    #                           bad id   ngroups 0  ploidy 3      ploidy 1
    "grouped_alt_freq":        (EINVAL,  EINVAL,    EUNSUPPORTED, OK),
    "grouped_missingness":     (EINVAL,  EINVAL,    None,         None),
    "grouped_summaries":       (EINVAL,  EINVAL,    EUNSUPPORTED, OK),
    "grouped_pi":              (EINVAL,  EINVAL,    None,         None),
    "grouped_genotype_counts": (EINVAL,  EINVAL,    None,         None),
    "pop_global_stats":        (EINVAL,  EINVAL,    EINVAL,       EINVAL),
    "pop_basic_stats":         (EINVAL,  EINVAL,    EINVAL,       EINVAL),
    "gt_grouped_hwe":          (EINVAL,  EINVAL,    None,         None),
    "pairwise_pop_fst":        (EINVAL,  EINVAL,    EUNSUPPORTED, OK),   # method = Hudson
    "pop_tajimas_d":           (EINVAL,  EINVAL,    EINVAL,       EINVAL),
    "windows_pop_tajimas_d":   (EINVAL,  EINVAL,    EINVAL,       EINVAL),
    "f2_blocks":               (EINVAL,  EINVAL,    EUNSUPPORTED, OK),
    "block_means":             (EINVAL,  EINVAL,    None,         None),
}


def test_the_same_return_codes_from_one_class_plan(tpg, fbm):
    lib = tpg._lib.lib
    v = tpg.View(tpg.FBM.from_numpy(fbm))
    calls = _entries(tpg, v)
    assert sorted(calls) == sorted(CODES)
    good, bad = _gid(), _gid()
    bad[5] = G
    two = np.full(N, 2.0)
    for name, (c_bad, c_zero, c_three, c_one) in CODES.items():
        call = calls[name]
        assert call(good, G, two if c_three is not None else None, HUDSON) == OK, (name, lib.tpg_last_error())
        assert call(bad, G, None, HUDSON) == c_bad, name
        assert "groupIds[5]" in lib.tpg_last_error().decode(), (name, lib.tpg_last_error())
        assert call(good, 0, None, HUDSON) == c_zero, name
        if c_three is None:
            continue
        for value, want in ((3.0, c_three), (1.0, c_one)):
            pl = two.copy()
            pl[2] = value
            assert call(good, G, pl, HUDSON) == want, (name, value, lib.tpg_last_error())
    pl = two.copy()
    pl[2] = 1.0
    assert calls["pairwise_pop_fst"](good, G, pl, WC84) == EINVAL  # R/pairwise_pop_fst.R:110-115
    assert "only method = Hudson" in lib.tpg_last_error().decode()
    v.free()


def _windowed(tpg, v, x):
    """name -> (word in the message, call(lo, hi) -> (return code, outputs)); lo / hi host arrays or device pointers"""
    lib, ctx = tpg._lib.lib, v.ctx
    nw, gid = len(LO), _gid()

    def ptr(a):
        return a if isinstance(a, C.c_void_p) else _p(a)

    def window_stats(lo, hi):
        stat, nl = np.zeros((nw, 2), order="F"), np.zeros((nw, 2), dtype=np.int32, order="F")
        rc = lib.tpg_window_stats(ctx.h, _p(x), C.c_int64(M), C.c_int(2), ptr(lo), ptr(hi), None, C.c_int64(nw), C.c_int(0),
                                  C.c_int(1), _p(stat), _p(nl))
        return rc, (stat, nl)

    def tajima(lo, hi):
        d, seg = np.zeros((nw, G), order="F"), np.zeros((nw, G), dtype=np.int64, order="F")
        k, nl = np.zeros((nw, G), order="F"), np.zeros((nw, G), dtype=np.int32, order="F")
        rc = lib.tpg_windows_pop_tajimas_d(ctx.h, v.h, _p(gid), G, None, ptr(lo), ptr(hi), None, nw, 1, _p(d), _p(seg), _p(k), _p(nl))
        return rc, (d, seg, k, nl)

    def f2_blocks(lo, hi):
        f2, cnt = np.zeros((G, G, nw), order="F"), np.zeros((G, G, nw), dtype=np.int32, order="F")
        kept = np.zeros(nw, dtype=np.int64)
        rc = lib.tpg_f2_blocks(ctx.h, v.h, _p(gid), G, None, None, ptr(lo), ptr(hi), nw, _p(f2), _p(cnt), None, None, _p(kept))
        return rc, (f2, cnt, kept)

    return {"window_stats": ("window", window_stats), "windows_pop_tajimas_d": ("window", tajima), "f2_blocks": ("block", f2_blocks)}


def test_ranges_in_host_and_in_device_memory(tpg, fbm):
    lib = tpg._lib.lib
    v = tpg.View(tpg.FBM.from_numpy(fbm))
    ctx = v.ctx
    x = np.asfortranarray(np.random.default_rng(2).random((M, 2)))
    x[7, 0] = np.nan

    def on_device(a):
        d = ctx.dev_alloc(a.nbytes)
        tpg._lib.check(lib.tpg_dev_from_host(ctx.h, d, _p(a), C.c_size_t(a.nbytes)))
        return d

    def swapped(i):  # lo > hi at i
        lo, hi = LO.copy(), HI.copy()
        lo[i], hi[i] = 20, 10
        return lo, hi

    def past_m(i):  # hi > m at i
        lo, hi = LO.copy(), HI.copy()
        hi[i] = M + 1
        return lo, hi

    def negative(i):  # lo < 0 at i
        lo, hi = LO.copy(), HI.copy()
        lo[i] = -1
        return lo, hi

    held = []
    try:
        for name, (word, call) in _windowed(tpg, v, x).items():
            rc, host = call(LO, HI)
            assert rc == OK, (name, lib.tpg_last_error())
            d_lo, d_hi = on_device(LO), on_device(HI)
            held += [d_lo, d_hi]
            rc, dev = call(d_lo, d_hi)
            assert rc == OK, (name, lib.tpg_last_error())
            for a, b in zip(host, dev):
                assert a.tobytes() == b.tobytes(), name
            for make, i in ((swapped, 1), (past_m, 2), (negative, 0)):
                lo, hi = make(i)
                d_lo, d_hi = on_device(lo), on_device(hi)
                held += [d_lo, d_hi]
                for args in ((lo, hi), (d_lo, d_hi)):
                    assert call(*args)[0] == EINVAL, (name, make.__name__)
                    assert f"{word} {i} " in lib.tpg_last_error().decode(), (name, make.__name__, lib.tpg_last_error())
    finally:
        for d in held:
            ctx.dev_free(d)
        v.free()


def _sequence(tpg, v):
    """grouped alt freq (G = 3), Fst on the same ids (the cached counts), grouped summaries with G = 33 (Cpad 32 -> 64: the
    cache is replaced), grouped alt freq with the G = 3 ids again"""
    lib = tpg._lib.lib
    pairs = _pairs(tpg, G)
    tot = np.zeros(pairs.shape[1])
    out = [tpg.grouped_alt_freq_dip_pseudo_cpp(v, _gid(), G)]
    gid = _gid()
    tpg._lib.check(lib.tpg_pairwise_pop_fst(v.ctx.h, v.h, _p(gid), C.c_int(G), None, C.c_int(HUDSON), _p(pairs),
                                            C.c_int(pairs.shape[1]), C.c_int(0), C.c_int(0), _p(tot), None, None))
    out.append(tot)
    with np.errstate(invalid="ignore", divide="ignore"):
        out.append(tpg.grouped_summaries_dip_pseudo_cpp(v, _gid(33), 33))
    out.append(tpg.grouped_alt_freq_dip_pseudo_cpp(v, _gid(), G))
    return out


def test_the_cached_counts_under_their_new_owner(tpg, fbm):
    lib = tpg._lib.lib
    X = tpg.FBM.from_numpy(fbm)
    v = tpg.View(X)
    got = _sequence(tpg, v)
    v.free()
    # every step alone on a view of its own
    pairs = _pairs(tpg, G)
    tot, gid = np.zeros(pairs.shape[1]), _gid()
    fresh = []
    for step in range(4):
        w = tpg.View(X)
        if step in (0, 3):
            fresh.append(tpg.grouped_alt_freq_dip_pseudo_cpp(w, _gid(), G))
        elif step == 1:
            tpg._lib.check(lib.tpg_pairwise_pop_fst(w.ctx.h, w.h, _p(gid), C.c_int(G), None, C.c_int(HUDSON), _p(pairs),
                                                    C.c_int(pairs.shape[1]), C.c_int(0), C.c_int(0), _p(tot), None, None))
            fresh.append(tot)
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                fresh.append(tpg.grouped_summaries_dip_pseudo_cpp(w, _gid(33), 33))
        w.free()
    two = np.full(N, 2.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        want_freq = orc.grouped_alt_freq_dip_pseudo_cpp(fbm, None, None, _gid(), G, two)
        want_fst = orc.pairwise_pop_fst(fbm, None, None, _gid(), G, method="Hudson")["fst_tot"]
        want_sum = orc.grouped_summaries_dip_pseudo_cpp(fbm, None, None, _gid(33), 33, two)
    for k in (0, 3):  # tests/test_gpu_parity.py: the grouped frequencies and summaries equal the oracle's bit for bit
        assert got[k].tobytes() == fresh[k].tobytes()
        assert np.array_equal(got[k], want_freq, equal_nan=True)
    assert got[1].tobytes() == fresh[1].tobytes()
    assert np.allclose(got[1], want_fst, rtol=1e-12, atol=0, equal_nan=True)  # (test_fst_vs_oracle)
    for k in want_sum:
        assert got[2][k].tobytes() == fresh[2][k].tobytes(), k
        assert np.array_equal(got[2][k], want_sum[k], equal_nan=True), k


def test_the_cached_counts_go_back_with_their_view(tpg, fbm):
    """The sequence above four times in a context of its own (an empty pool), each on a fresh view that is freed: the device
    memory in use, read through the HIP runtime the library runs on as tests/test_gpu_stream.py reads it, is no more after
    the fourth run than after the first -- a block that left the pool with a view and did not come back would have to be
    allocated again.  (No other process allocates on this GPU meanwhile.)"""
    hip = C.CDLL("libamdhip64.so.7")

    def used():
        fr, tot = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
        return tot.value - fr.value

    ctx = tpg.Context(0)
    X = tpg.FBM.from_numpy(fbm, ctx=ctx)
    after = []
    for _ in range(4):
        v = tpg.View(X)
        _sequence(tpg, v)
        v.free()
        ctx.sync()
        after.append(used())
    print("device bytes in use after each run:", after)
    X.free()
    ctx.close()
    assert after[3] <= after[0], after
