"""GPU: IBD segments (include/tpg.h "IBD segments") against the numpy restatement tests/ibdseg_ref.py.  Everything is an
integer, so every comparison is equality: the segments with n_typed / n_err, their count, the per-pair counts and sums of
lengths.  The panels carry the seam cases (tests/test_ibdseg_host.py asserts that of the reference alone): a bad locus on the
last bit of a word and of a chunk, breaks on a word and on a chunk border, a segment across three chunks."""
import ctypes as C

import numpy as np
import pytest

from tests import ibdseg_ref as ir

pytestmark = pytest.mark.gpu

SENT32, SENT64 = -77, -7777


def _view(tpg, G, ind_row=None, ind_col=None):
    X = tpg.FBM.from_numpy(np.asfortranarray(G), code256=tpg.CODE_012)
    return tpg.View(X, ind_row, ind_col)


def _raw(tpg, v, chrom, pos, cap, arrays=True, kind=1, min_snp=20, min_length=0, max_gap=10**6, bridge_min_snp=8, max_err=-1):
    """tpg_ibd_segments as it is, into arrays full of a sentinel -> (rc, count, the six arrays or None, n_seg, sum_length)"""
    from tidypopgen_amd import _lib
    from tidypopgen_amd.api import _ptr

    n = v.n
    seg = None
    if arrays:
        seg = [np.full(max(cap, 1), SENT32 if k in (0, 1, 4, 5) else SENT64, dtype=np.int32 if k in (0, 1, 4, 5) else np.int64)
               for k in range(6)]
    n_seg, total = np.full((n, n), SENT32, dtype=np.int32), np.full((n, n), SENT64, dtype=np.int64)
    count = C.c_int64(SENT64)
    ptrs = [_ptr(a) for a in seg] if arrays else [None] * 6
    rc = _lib.lib.tpg_ibd_segments(v.ctx.h, v.h, _ptr(chrom), _ptr(pos), kind, min_snp, min_length, max_gap, bridge_min_snp, max_err,
                                   cap, *ptrs, C.byref(count), _ptr(n_seg), _ptr(total))
    return rc, count.value, seg, n_seg, total


def _untouched(res):
    _, count, seg, n_seg, total = res
    return count == SENT64 and np.all(n_seg == SENT32) and np.all(total == SENT64) and all(
        np.all(a == (SENT32 if a.dtype == np.int32 else SENT64)) for a in seg)


def _check(tpg, v, G, chrom, pos, **kw):
    want = ir.segments_vec(G, chrom, pos, **kw)
    got = tpg.ibd_segments(v, chrom, pos, **kw)
    assert len(got["first"]) == len(want["first"])
    assert ir.same_segments(got, want)
    assert got["ind_a"].dtype == np.int32 and got["first"].dtype == np.int64 and got["n_typed"].dtype == np.int32
    assert np.array_equal(got["length"], np.asarray(pos)[want["last"]] - np.asarray(pos)[want["first"]])
    w_seg, w_total = ir.summary(want, G.shape[0], pos)
    assert got["n_seg"].dtype == np.int32 and np.array_equal(got["n_seg"], w_seg)
    assert got["sum_length"].dtype == np.int64 and np.array_equal(got["sum_length"], w_total)
    return want, got


@pytest.mark.parametrize("n,m", ir.GRID)
def test_grid(n, m):
    import tidypopgen_amd as tpg

    assert tpg.IBD_CHUNK_LOCI == ir.CHUNK
    G, chrom, pos = ir.grid_case(n, m)
    v = _view(tpg, G)
    for kind, bridge in ir.CONFIGS:
        kw = dict(ir.GRID_PARAMS, kind=kind, bridge_min_snp=bridge)
        want, got = _check(tpg, v, G, chrom, pos, **kw)
        again = tpg.ibd_segments(v, chrom, pos, **kw)  # two calls, the same bits
        assert all(np.array_equal(got[k], again[k]) for k in got)
        c = len(want["first"])
        w_seg, w_total = ir.summary(want, n, pos)
        res = _raw(tpg, v, chrom, pos, 0, arrays=False, kind=kind, bridge_min_snp=bridge)  # the counting call
        assert res[0] == 0 and res[1] == c and np.array_equal(res[3], w_seg) and np.array_equal(res[4], w_total)
        if c >= 1:  # too short: the count and the per-pair outputs are complete, the arrays untouched
            res = _raw(tpg, v, chrom, pos, max(c - 1, 1) if c > 1 else 0, arrays=True, kind=kind, bridge_min_snp=bridge)
            assert res[0] == 0 and res[1] == c and np.array_equal(res[3], w_seg) and np.array_equal(res[4], w_total)
            assert all(np.all(a == (SENT32 if a.dtype == np.int32 else SENT64)) for a in res[2])
        if bridge and m >= 128 and n >= 2:
            assert c > 0
    for kind, min_snp, bridge in ir.LONG_CONFIGS:
        _check(tpg, v, G, chrom, pos, **dict(ir.GRID_PARAMS, kind=kind, min_snp=min_snp, bridge_min_snp=bridge))
    if m >= 2 * ir.CHUNK and n >= 2:  # the segment across three chunks is among what the device reported
        s = tpg.ibd_segments(v, chrom, pos, **dict(ir.GRID_PARAMS, kind=2, bridge_min_snp=ir.GRID_BRIDGE))
        assert any(a == 0 and b == 1 and f < ir.CHUNK and l >= 2 * ir.CHUNK and e >= 1
                   for a, b, f, l, e in zip(s["ind_a"], s["ind_b"], s["first"], s["last"], s["n_err"]))


def test_the_wrapper_calls_again_when_the_arrays_are_short():
    import tidypopgen_amd as tpg

    G, chrom, pos = ir.grid_case(33, 1000)
    v = _view(tpg, G)
    kw = dict(ir.GRID_PARAMS, kind=1, bridge_min_snp=ir.GRID_BRIDGE)
    want = ir.segments_vec(G, chrom, pos, **kw)
    assert len(want["first"]) > 3
    for cap in (1, 3, len(want["first"]), 0):
        got = tpg.ibd_segments(v, chrom, pos, cap=cap, **kw)
        assert ir.same_segments(got, want)
    plain = tpg.ibd_segments(v, chrom, pos, summary=False, **kw)
    assert ir.same_segments(plain, want) and "n_seg" not in plain
    # the default has room for a segment per pair: one counting walk, where arrays that are too short cost two
    ctx = v.ctx
    ctx.prof_enable(True)
    try:
        for cap, walks in ((None, 1), (1, 2)):
            ctx.sync(); ctx.prof_reset()
            tpg.ibd_segments(v, chrom, pos, cap=cap, **kw)
            ctx.sync()
            assert ctx.prof_dump()["ibd_count_1"][0] == walks
    finally:
        ctx.prof_enable(False)


def test_every_parameter_reaches_the_device():
    import tidypopgen_amd as tpg
    from tests.test_ibdseg_host import TEETH

    G, chrom, pos = ir.grid_case(33, 1000)
    v = _view(tpg, G)
    for kind in (1, 2):
        base = dict(ir.GRID_PARAMS, kind=kind, bridge_min_snp=ir.GRID_BRIDGE)
        for _, over in TEETH:
            _check(tpg, v, G, chrom, pos, **dict(base, **over))
    _check(tpg, v, G, chrom, pos, kind=1)  # the defaults
    _check(tpg, v, G, chrom, pos, kind=2, min_snp=1, bridge_min_snp=1, max_gap=0)
    _check(tpg, v, G, chrom, pos, kind=2, min_snp=30, bridge_min_snp=2**40, max_err=2**40, min_length=2**40)


def test_a_sub_view_equals_the_copied_sub_panel():
    import tidypopgen_amd as tpg

    n, m = 70, 1300
    G = ir.ibd_panel(17, n, m)
    rng = np.random.default_rng(17)
    rows = np.sort(rng.permutation(n)[:45]) + 1
    cols = np.sort(rng.permutation(m)[:1100]) + 1
    chrom, pos = ir.ibd_loci(17, len(cols))
    sub = G[np.ix_(rows - 1, cols - 1)]
    X = tpg.FBM.from_numpy(np.asfortranarray(G), code256=tpg.CODE_012)
    for kind in (1, 2):
        kw = dict(ir.GRID_PARAMS, kind=kind, bridge_min_snp=ir.GRID_BRIDGE)
        want, _ = _check(tpg, tpg.View(X, rows, cols), sub, chrom, pos, **kw)
        assert len(want["first"]) > 0
        got = tpg.ibd_segments(X, chrom, pos, ind_row=rows, ind_col=cols, **kw)
        assert ir.same_segments(got, want)
        assert ir.same_segments(tpg.ibd_segments(_view(tpg, sub), chrom, pos, **kw), want)


def test_errors_leave_the_outputs_untouched():
    import tidypopgen_amd as tpg
    from tidypopgen_amd import _lib

    G, chrom, pos = ir.grid_case(3, 129)
    v = _view(tpg, G)
    assert _raw(tpg, v, chrom, pos, 64)[0] == 0
    for bad in (dict(min_snp=0), dict(min_length=-1), dict(max_gap=-1), dict(bridge_min_snp=-1), dict(kind=0), dict(kind=3)):
        res = _raw(tpg, v, chrom, pos, 64, **bad)
        assert res[0] == 1 and _untouched(res), bad  # TPG_EINVAL
    back = pos.copy()
    back[20] = back[19] - 1
    res = _raw(tpg, v, chrom, back, 64)
    assert res[0] == 1 and "not ordered" in _lib.lib.tpg_last_error().decode() and _untouched(res)
    two = chrom.copy()
    two[20:] += 7  # the same positions on a new chromosome are in order
    assert _raw(tpg, v, two, back, 64)[0] == 0
    with pytest.raises(ValueError, match="not ordered"):
        tpg.ibd_segments(v, chrom, back)
    out = C.c_int64(SENT64)
    assert _lib.lib.tpg_ibd_genome_length(chrom.ctypes.data, back.ctypes.data, len(back), 10**6, C.byref(out)) == 1
    assert out.value == SENT64
    assert tpg.ibd_genome_length(chrom, pos, 10**6) == ir.genome_length(chrom, pos, 10**6)
    assert tpg.ibd_genome_length(two, back, 1500) == ir.genome_length(two, back, 1500)


def test_one_individual_and_a_wholly_missing_one():
    import tidypopgen_amd as tpg

    G, chrom, pos = ir.grid_case(3, 129)
    got = tpg.ibd_segments(_view(tpg, G[:1]), chrom, pos, min_snp=1)
    assert len(got["first"]) == 0 and got["n_seg"].shape == (1, 1) and not got["n_seg"].any() and not got["sum_length"].any()
    G[1] = 3
    G[2] = G[0]
    for kind in (1, 2):
        got = tpg.ibd_segments(_view(tpg, G), chrom, pos, kind=kind, min_snp=1, bridge_min_snp=0)
        assert set(zip(got["ind_a"].tolist(), got["ind_b"].tolist())) == {(0, 2)}  # the duplicate: a segment per break-free region
        assert got["sum_length"][0, 2] == ir.genome_length(chrom, pos, 10**6)
        assert ir.same_segments(got, ir.segments_vec(G, chrom, pos, kind=kind, min_snp=1, bridge_min_snp=0))


def test_outputs_in_device_memory():
    import tidypopgen_amd as tpg
    from tidypopgen_amd import _lib
    from tidypopgen_amd.api import _ptr

    G, chrom, pos = ir.grid_case(33, 129)
    v = _view(tpg, G)
    kw = dict(ir.GRID_PARAMS, kind=1, bridge_min_snp=ir.GRID_BRIDGE)
    want = ir.segments_vec(G, chrom, pos, **kw)
    c, n = len(want["first"]), 33
    assert c > 0
    ctx = v.ctx
    host = [np.zeros(c, dtype=np.int32), np.zeros(c, dtype=np.int32), np.zeros(c, dtype=np.int64), np.zeros(c, dtype=np.int64),
            np.zeros(c, dtype=np.int32), np.zeros(c, dtype=np.int32), np.zeros(1, dtype=np.int64), np.zeros((n, n), dtype=np.int32),
            np.zeros((n, n), dtype=np.int64)]
    dev = [ctx.dev_alloc(a.nbytes) for a in host]
    d_chrom, d_pos = ctx.dev_alloc(chrom.nbytes), ctx.dev_alloc(pos.nbytes)
    try:
        for d, a in ((d_chrom, chrom), (d_pos, pos)):
            _lib.check(_lib.lib.tpg_dev_from_host(ctx.h, d, _ptr(a), C.c_size_t(a.nbytes)))
        _lib.check(_lib.lib.tpg_ibd_segments(ctx.h, v.h, d_chrom, d_pos, 1, 20, 0, 10**6, ir.GRID_BRIDGE, -1, c, *dev))
        for d, a in zip(dev, host):
            _lib.check(_lib.lib.tpg_dev_to_host(ctx.h, _ptr(a), d, C.c_size_t(a.nbytes)))
    finally:
        for d in dev + [d_chrom, d_pos]:
            ctx.dev_free(d)
    assert host[6][0] == c
    assert ir.same_segments(dict(zip(ir.KEYS, host[:6])), want)
    w_seg, w_total = ir.summary(want, n, pos)
    assert np.array_equal(host[7], w_seg) and np.array_equal(host[8], w_total)


def test_pairwise_ibd_on_the_pedigree_and_the_relatedness_filter():
    import tidypopgen_amd as tpg

    G, chrom, pos, A = ir.pedigree(1)
    n = G.shape[0]
    X = tpg.FBM.from_numpy(np.asfortranarray(G), code256=tpg.CODE_012)
    r = tpg.pairwise_ibd(X, chrom, pos, **ir.PED_PARAMS)
    segs = {kind: ir.segments_vec(G, chrom, pos, kind=kind, **ir.PED_PARAMS) for kind in (1, 2)}
    assert ir.same_segments(r["segments1"], segs[1]) and ir.same_segments(r["segments2"], segs[2])
    Lg = ir.genome_length(chrom, pos, ir.PED_PARAMS["max_gap"])
    L1, L2 = ir.summary(segs[1], n, pos)[1], ir.summary(segs[2], n, pos)[1]
    assert r["genome_length"] == Lg
    assert np.array_equal(r["ibd1_prop"], (L1 - L2) / Lg) and np.array_equal(r["ibd2_prop"], L2 / Lg)
    assert np.array_equal(r["kin"], (L1 + L2) / (4.0 * Lg))
    for child, parents in enumerate(ir.PED_CHILDREN, start=ir.PED_N_FOUNDERS):
        for par in parents:
            assert r["ibd1_prop"][par, child] == 1.0 and r["ibd2_prop"][par, child] == 0.0
    for bad in (dict(kind=2), dict(summary=False)):
        with pytest.raises(ValueError):
            tpg.pairwise_ibd(X, chrom, pos, **bad)
    with pytest.raises(ValueError, match="span no length"):
        tpg.pairwise_ibd(X, chrom, np.zeros_like(pos), **ir.PED_PARAMS)
    passed, removed, keep = tpg.filter_high_relatedness(r["kin"], 0.0884)
    kept = np.flatnonzero(keep)
    assert 0 < len(removed) < n
    for a in kept:
        for b in kept:
            if a < b:
                assert not ir.true_ibd(A, a, b).any(), (a, b)
