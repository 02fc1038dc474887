"""LD clumping on the GPU (include/tpg.h "LD clumping"): tpg_ld_band_links and tpg_ld_clump against the numpy restatement
tests/ld_ref.py, everything by equality."""
import ctypes as C

import numpy as np
import pytest

from tests import fixtures as fx
from tests import impute_ref as ir
from tests import ld_ref as lr

pytestmark = pytest.mark.gpu

THR = 0.2
NS = (1, 63, 64, 65, 127, 129, 500)
MS = (1, 31, 33, 1000, 4097)
WINDOWS = (0, 1, 31, 32, 33, 10 ** 6)  # in loci; the last one is wider than every m


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


def _view(tpg, G):
    X = tpg.FBM.from_numpy(np.asfortranarray(G, dtype=np.uint8), code256=tpg.CODE_012)
    return tpg.View(X)


def _hi(m, win):
    return lr.window_hi(np.zeros(m, dtype=np.int64), None, win, use_positions=False)


def _window_of(n, m):
    """one window per (n, m), every value of WINDOWS being used across the grid"""
    return WINDOWS[(NS.index(n) + MS.index(m)) % len(WINDOWS)]


_ref_cache = {}


def _ref(n, m, win):
    key = (n, m, win)
    if key not in _ref_cache:
        G = lr.ld_panel(100 * n + m, n, m, 0.9)
        hi = _hi(m, win)
        bits = lr.band_bits(G, hi, THR)
        _ref_cache[key] = (G, hi, bits, lr.bits_to_adjacency(bits))
    return _ref_cache[key]


def _check_clump(tpg, v, G, hi, adj, S=None, exclude=None):
    key = lr.priority_key(G, S)
    want = lr.greedy(adj, key, exclude)
    _, rounds, left = lr.parallel_rounds(adj, key, exclude, max_rounds=lr.MAX_ROUNDS)
    keep, rep = tpg.ld_clump(v, hi, THR, S=S, exclude=exclude, return_report=True)
    assert np.array_equal(keep, want), int((keep != want).sum())
    assert rep["links"] == sum(len(a) for a in adj) // 2
    assert rep["kept"] == int(want.sum())
    assert rep["rounds"] == rounds and rep["finish_loci"] == left
    return rep


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_band_and_clump_around_every_tile_edge(tpg, n, m):
    win = _window_of(n, m)
    G, hi, bits, adj = _ref(n, m, win)
    v = _view(tpg, G)
    got, links = tpg.ld_band_links(v, hi, THR, return_links=True)
    assert got.shape == bits.shape and np.array_equal(got, bits), int((got != bits).sum())  # the zero padding bits included
    assert links == sum(len(a) for a in adj) // 2
    rng = np.random.default_rng(n + m)
    _check_clump(tpg, v, G, hi, adj)
    _check_clump(tpg, v, G, hi, adj, S=rng.integers(0, 4, m).astype(np.float64))  # many ties
    _check_clump(tpg, v, G, hi, adj, S=np.arange(m, dtype=np.float64))            # priority rises along the genome


@pytest.mark.parametrize("win", WINDOWS)
def test_every_window_width(tpg, win):
    n, m = 129, 1000
    G, hi, bits, adj = _ref(n, m, win)
    v = _view(tpg, G)
    # a wider stride than needed: the unused words are zero
    stride = bits.shape[1] + 3
    out = np.full((m, stride), 0xFFFFFFFF, dtype=np.uint32)
    from tidypopgen_amd import _lib

    _lib.check(_lib.lib.tpg_ld_band_links(v.ctx.h, v.h, C.c_void_p(hi.ctypes.data), C.c_double(THR), C.c_void_p(out.ctypes.data),
                                          C.c_int64(stride), None))
    assert np.array_equal(out[:, :bits.shape[1]], bits) and not out[:, bits.shape[1]:].any()
    _check_clump(tpg, v, G, hi, adj)
    if win == 0:
        assert not bits.any() and tpg.ld_clump(v, hi, THR).all()


def test_long_priority_chain_takes_the_finish_path(tpg):
    G, hi, bits, adj = _ref(500, 4097, 33)
    v = _view(tpg, G)
    rep = _check_clump(tpg, v, G, hi, adj, S=np.arange(4097, dtype=np.float64))
    assert rep["rounds"] == lr.MAX_ROUNDS and rep["finish_loci"] > 0
    rep = _check_clump(tpg, v, G, hi, adj, S=-np.arange(4097, dtype=np.float64))
    assert rep["rounds"] == lr.MAX_ROUNDS and rep["finish_loci"] > 0
    rep = _check_clump(tpg, v, G, hi, adj)  # the default key settles in a few rounds
    assert rep["finish_loci"] == 0


def test_window_from_positions_with_several_chromosomes(tpg):
    n, m = 200, 3000
    rng = np.random.default_rng(8)
    G = lr.ld_panel(8, n, m, 0.9)
    chrom = np.sort(rng.integers(1, 6, m))
    pos = np.concatenate([np.sort(rng.integers(1, 400_000, int((chrom == c).sum()))) for c in np.unique(chrom)])
    size = 20.0  # kb: about 30 loci a side, varying per locus
    hi = lr.window_hi(chrom, pos, size, True)
    assert len(np.unique(hi - np.arange(m))) > 10
    v = _view(tpg, G)
    bits = lr.band_bits(G, hi, THR)
    assert np.array_equal(tpg.ld_band_links(v, hi, THR), bits)
    adj = lr.bits_to_adjacency(bits)
    _check_clump(tpg, v, G, hi, adj)
    # the public entry point, flags included
    X = tpg.FBM.from_numpy(G, code256=tpg.CODE_012)
    want = lr.greedy(adj, lr.priority_key(G))
    got = tpg.loci_ld_clump(X, thr_r2=THR, size=size, chromosome=chrom, position=pos)
    assert got.dtype == bool and np.array_equal(got, want)
    assert np.array_equal(tpg.loci_ld_clump(X, thr_r2=THR, size=size, chromosome=chrom, position=pos, return_id=True),
                          np.flatnonzero(want) + 1)
    ex1 = np.flatnonzero(want)[::3] + 1  # exclude every third kept locus (1-based)
    exb = np.zeros(m, dtype=bool)
    exb[ex1 - 1] = True
    want_ex = lr.greedy(adj, lr.priority_key(G), exb)
    got_ex = tpg.loci_ld_clump(X, thr_r2=THR, size=size, chromosome=chrom, position=pos, exclude=ex1)
    assert np.array_equal(got_ex, want_ex) and not got_ex[exb].any() and not np.array_equal(want_ex, want)
    _check_clump(tpg, v, G, hi, adj, exclude=exb.astype(np.uint8))
    # the default size is 100 / thr_r2 kb; without positions it counts loci
    hi500 = lr.window_hi(chrom, None, 100 / THR, False)
    w500 = lr.greedy(lr.bits_to_adjacency(lr.band_bits(G, hi500, THR)), lr.priority_key(G))
    assert np.array_equal(tpg.loci_ld_clump(X, thr_r2=THR, chromosome=chrom, use_positions=False), w500)
    with pytest.raises(ValueError, match="not ordered"):
        tpg.loci_ld_clump(X, thr_r2=THR, chromosome=np.r_[chrom[1:], chrom[0]], use_positions=False)


@pytest.mark.parametrize("name", ["families", "lobster"])
def test_golden_bed_panels_after_mode_imputation(tpg, name):
    raw = fx.families_fbm() if name == "families" else fx.lobster_fbm()
    G = ir.impute_codes(raw, "mode")
    typed = (G != 3).all(axis=0)
    assert typed.all()
    n, m = G.shape
    hi = _hi(m, 40)
    bits = lr.band_bits(G, hi, THR)
    adj = lr.bits_to_adjacency(bits)
    v = _view(tpg, G)
    assert np.array_equal(tpg.ld_band_links(v, hi, THR), bits)
    _check_clump(tpg, v, G, hi, adj)
    # the same through impute= on the raw store
    X = tpg.FBM.from_numpy(np.asfortranarray(raw), code256=tpg.CODE_012)
    got = tpg.loci_ld_clump(X, thr_r2=THR, size=40, use_positions=False, impute="mode")
    assert np.array_equal(got, lr.greedy(adj, lr.priority_key(G)))
    from tidypopgen_amd._lib import TpgError

    with pytest.raises(TpgError) as e:
        tpg.loci_ld_clump(X, thr_r2=THR, size=40, use_positions=False)
    assert e.value.code == 4


def test_refusals(tpg):
    from tidypopgen_amd import _lib

    n, m = 65, 200
    G = lr.ld_panel(5, n, m, 0.9)
    hi = _hi(m, 20)
    bad = G.copy()
    bad[7, 100] = 3
    vb = _view(tpg, bad)
    keep = np.full(m, 7, dtype=np.uint8)
    bits = np.full((m, 1), 0xABCDEF01, dtype=np.uint32)
    rc = _lib.lib.tpg_ld_clump(vb.ctx.h, vb.h, C.c_void_p(hi.ctypes.data), C.c_double(THR), None, None, C.c_void_p(keep.ctypes.data), None)
    assert rc == 4 and (keep == 7).all()  # TPG_ENUMERIC, keep untouched
    rc = _lib.lib.tpg_ld_band_links(vb.ctx.h, vb.h, C.c_void_p(hi.ctypes.data), C.c_double(THR), C.c_void_p(bits.ctypes.data), C.c_int64(1), None)
    assert rc == 4 and (bits == 0xABCDEF01).all()
    v = _view(tpg, G)

    def clump_rc(h, S=None):
        h = np.ascontiguousarray(h, dtype=np.int64)
        s = None if S is None else np.ascontiguousarray(S, dtype=np.float64)
        rc = _lib.lib.tpg_ld_clump(v.ctx.h, v.h, C.c_void_p(h.ctypes.data), C.c_double(THR),
                                   None if s is None else C.c_void_p(s.ctypes.data), None, C.c_void_p(keep.ctypes.data), None)
        return rc

    S = np.arange(m, dtype=np.float64)
    S[50] = np.nan
    assert clump_rc(hi, S) == 1 and (keep == 7).all()  # TPG_EINVAL
    dec = hi.copy()
    dec[30] = dec[29] - 1
    assert clump_rc(dec) == 1
    low = hi.copy()
    low[0:3] = [0, 0, 1]  # hi[2] < 2
    assert clump_rc(low) == 1
    far = hi.copy()
    far[-1] = m
    assert clump_rc(far) == 1 and (keep == 7).all()
    short = np.zeros((m, 0), dtype=np.uint32)
    rc = _lib.lib.tpg_ld_band_links(v.ctx.h, v.h, C.c_void_p(hi.ctypes.data), C.c_double(THR), C.c_void_p(bits.ctypes.data), C.c_int64(short.shape[1]), None)
    assert rc == 1  # stride_words too small for the window
    assert clump_rc(hi) == 0 and set(np.unique(keep)) <= {0, 1}


def test_invariance_to_how_the_view_was_made_and_to_device_pointers(tpg):
    from tidypopgen_amd import _lib

    rng = np.random.default_rng(9)
    N, M = 300, 2500
    big = lr.ld_panel(9, N, M, 0.9)
    rows = np.sort(rng.permutation(N)[:129]) + 1
    cols = np.arange(101, 2101)  # contiguous: LD structure survives
    sub = np.asfortranarray(big[np.ix_(rows - 1, cols - 1)])
    m = len(cols)
    hi = _hi(m, 60)
    bits = lr.band_bits(sub, hi, THR)
    adj = lr.bits_to_adjacency(bits)
    want = lr.greedy(adj, lr.priority_key(sub))
    X = tpg.FBM.from_numpy(big, code256=tpg.CODE_012)
    v1 = tpg.View(X, rows, cols)
    v2 = _view(tpg, sub)
    for v in (v1, v2):
        assert np.array_equal(tpg.ld_band_links(v, hi, THR), bits)
        assert np.array_equal(tpg.ld_clump(v, hi, THR), want)
    got = tpg.loci_ld_clump(X, rows, cols, thr_r2=THR, size=60, use_positions=False)
    assert np.array_equal(got, want)
    # device pointers on both sides: hi, S, exclude in, keep and bits out
    ctx = v2.ctx
    S = rng.integers(0, 3, m).astype(np.float64)
    ex = (rng.random(m) < 0.05).astype(np.uint8)
    want_s = lr.greedy(adj, S, ex)
    bufs = []

    def dev(a):
        p = ctx.dev_alloc(max(16, a.nbytes))
        bufs.append(p)
        _lib.check(_lib.lib.tpg_dev_from_host(ctx.h, p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes)))
        return p

    d_hi, d_S, d_ex = dev(hi), dev(S), dev(ex)
    d_keep, d_bits = dev(np.zeros(m, dtype=np.uint8)), dev(np.zeros_like(bits))
    rep = _lib.LdReport()
    _lib.check(_lib.lib.tpg_ld_clump(ctx.h, v2.h, d_hi, C.c_double(THR), d_S, d_ex, d_keep, C.byref(rep)))
    keep = np.zeros(m, dtype=np.uint8)
    _lib.check(_lib.lib.tpg_dev_to_host(ctx.h, C.c_void_p(keep.ctypes.data), d_keep, C.c_size_t(m)))
    assert np.array_equal(keep.astype(bool), want_s) and rep.kept == int(want_s.sum())
    assert np.array_equal(tpg.ld_clump(v2, hi, THR, S=S, exclude=ex), want_s)
    _lib.check(_lib.lib.tpg_ld_band_links(ctx.h, v2.h, d_hi, C.c_double(THR), d_bits, C.c_int64(bits.shape[1]), None))
    back = np.zeros_like(bits)
    _lib.check(_lib.lib.tpg_dev_to_host(ctx.h, C.c_void_p(back.ctypes.data), d_bits, C.c_size_t(bits.nbytes)))
    assert np.array_equal(back, bits)
    for p in bufs:
        ctx.dev_free(p)


def _device_panel(tpg, n, m, rho, seed):
    """the generator of tests/ld_ref.py at a size where its per-locus Python loop is too slow: the same recurrence, run
    in blocks of loci with numpy on whole blocks (a different random stream: the panel is its own input)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, size=m)
    G = np.empty((n, m), dtype=np.uint8, order="F")
    prev = (rng.random(2 * n) < p[0]).astype(np.uint8)
    B = 2000
    for j0 in range(0, m, B):
        j1 = min(m, j0 + B)
        own = (rng.random((2 * n, j1 - j0)) < p[None, j0:j1]).astype(np.uint8)
        copy = rng.random((2 * n, j1 - j0)) < rho
        hap = np.empty((2 * n, j1 - j0), dtype=np.uint8)
        for j in range(j1 - j0):
            prev = np.where(copy[:, j], prev, own[:, j]) if (j0 + j) > 0 else prev
            hap[:, j] = prev
        G[:, j0:j1] = hap[:n] + hap[n:]
    return G


def test_scale_5000_by_200000_window_500(tpg):
    n, m, win = 5000, 200_000, 500
    G = _device_panel(tpg, n, m, 0.97, 21)
    hi = _hi(m, win)
    v = _view(tpg, G)
    bits, links = tpg.ld_band_links(v, hi, THR, return_links=True)
    rng = np.random.default_rng(22)
    rows = np.sort(rng.choice(m, 2000, replace=False))
    want = lr.band_bits(G, hi, THR, stride=bits.shape[1], rows=rows)
    assert np.array_equal(bits[rows], want[rows])
    assert links == int(np.unpackbits(bits.view(np.uint8)).sum())
    # the full keep vector against a host greedy run on the downloaded band
    keep, rep = tpg.ld_clump(v, hi, THR, return_report=True)
    adj = lr.bits_to_adjacency(bits)
    host = lr.greedy(adj, lr.priority_key(G))
    assert np.array_equal(keep, host)
    assert rep["links"] == links and rep["kept"] == int(host.sum()) and 0 < rep["kept"] < m


def test_largest_sample_size_is_exact_and_the_next_one_is_refused(tpg):
    """n = 2^22 - 1 leaves one padding individual in the last group and sums Sxy up to 4 n = 2^24 - 4: loci that are all 2
    (monomorphic: linked to nothing) or all 2 but for a few individuals need every one of those sums exact"""
    from tidypopgen_amd import _lib

    n, m = 2 ** 22 - 1, 34
    rng = np.random.default_rng(31)
    G = np.full((n, m), 2, dtype=np.uint8, order="F")
    who = rng.permutation(n)[:64]
    for j in range(2, 12):  # all 2 but for 1 .. 10 individuals, shared between neighbouring loci: r^2 on both sides of thr
        G[who[:j - 1], j] = rng.integers(0, 2, j - 1)
    for j in range(12, m):  # ordinary loci in LD
        own = rng.binomial(2, 0.5, n).astype(np.uint8)
        G[:, j] = np.where(rng.random(n) < 0.6, G[:, j - 1], own) if j > 12 else own
    hi = _hi(m, 8)
    bits = lr.band_bits(G, hi, THR)
    assert not bits[0].any() and not bits[1].any() and bits[2:12].any() and bits[12:].any()
    v = _view(tpg, G)
    got, links = tpg.ld_band_links(v, hi, THR, return_links=True)
    assert np.array_equal(got, bits)
    adj = lr.bits_to_adjacency(bits)
    keep = tpg.ld_clump(v, hi, THR)
    assert np.array_equal(keep, lr.greedy(adj, lr.priority_key(G))) and keep[0] and keep[1]
    del v, G
    big = _view(tpg, np.ones((2 ** 22, 2), dtype=np.uint8))
    h2 = np.array([1, 1], dtype=np.int64)
    out = np.full(2, 7, dtype=np.uint8)
    rc = _lib.lib.tpg_ld_clump(big.ctx.h, big.h, C.c_void_p(h2.ctypes.data), C.c_double(THR), None, None, C.c_void_p(out.ctypes.data), None)
    assert rc == 3 and (out == 7).all()  # TPG_EUNSUPPORTED
