"""GPU: Tajima's D (include/tpg.h "Tajima's D") against the numpy restatement tests/tajima_ref.py.

What is compared how.  seg and n_loci are integers: equality.  The NaN / Inf pattern of k_hat and D: equality.  pi is the same
double on both sides (integers below 2^48 and one correctly rounded division), so k_hat differs from the float route only by
the order of a sum of L non-negative terms: |dk| <= L 2^-52 k_hat.  D divides k_hat - S / a1 by sqrt(vd), with a1 computed
twice: |dD| <= 2^-50 (L k_hat + S / a1) / sqrt(vd) + 2^-48 |D|.  Those hold for every cell.  The numerator formed from the
device's k_hat is held against the exact (Fraction) route within 2^-50 (L k_hat + S / a1) on a SAMPLE of the cells with a finite
k_hat: the windows that contain a planted locus only just (size 1 at the pi = 1 locus), the window [0, m), the windows across
the chunk border, and an even stride through the rest up to EXACT_CELLS per case (Fraction arithmetic on every one of the
150 000 cells of the largest case would take minutes).  seg and k_hat do not depend on min_loci, so that check runs at
min_loci = 1."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests import tajima_ref as tr

pytestmark = pytest.mark.gpu

NS = (13, 65)
GS = (1, 3, 33)
EXACT_CELLS = 1500  # strided cells per case held against the Fraction route, beside the planted ones (all, where there are fewer)


def _chunk():
    from tidypopgen_amd import api

    return api.TAJIMA_CHUNK_LOCI


def _ms():
    return (1, 63, 64, 65, 300, _chunk() + 1)


def _embed(codes, seed):
    """the panel as rows / columns of a larger store: -> bytes, ind_row, ind_col (1-based)"""
    n, m = codes.shape
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.permutation(n + 3)[:n])
    cols = np.sort(rng.permutation(m + 5)[:m])
    big = rng.integers(0, 4, size=(n + 3, m + 5)).astype(np.uint8)
    big[np.ix_(rows, cols)] = codes
    return big, rows + 1, cols + 1


def _window_lists(tpg, m, chunk):
    """every list of the issue, end to end: -> lo, hi, pad_na"""
    one = np.ones(m, dtype=np.int64)
    two = np.r_[np.ones(m // 2, dtype=np.int64), np.full(m - m // 2, 2)]
    rng = np.random.default_rng(m)
    bp = np.cumsum(rng.choice([1, 3, 40, 700], size=m, p=[0.5, 0.3, 0.15, 0.05]))  # gaps wider than a window: empty windows
    parts = [tpg.window_index_ranges(one, None, 1, 1),
             tpg.window_index_ranges(two, None, 3, 2),
             tpg.window_index_ranges(one, None, 64, 1),
             tpg.window_index_ranges(one, None, 65, 1),
             tpg.window_index_ranges(one, bp, 100, 100, size_unit="bp"),
             tpg.window_index_ranges(two, None, 3, 2, complete=True),
             tpg.window_index_ranges(one, bp, 250, 100, size_unit="bp", complete=True)]
    lo = np.concatenate([p["lo"] for p in parts] + [[0, m // 2, m]])  # the whole view and two empty windows
    hi = np.concatenate([p["hi"] for p in parts] + [[m, m // 2, m]])
    pad = np.concatenate([p["pad_na"] for p in parts] + [[0, 0, 0]]).astype(np.uint8)
    if m > chunk:  # a window straddling the chunk border
        lo, hi, pad = np.r_[lo, chunk - 5, chunk - 70], np.r_[hi, chunk + 1, chunk + 1], np.r_[pad, 0, 0].astype(np.uint8)
    assert pad.any() and (lo == hi).any()
    return lo.astype(np.int64), hi.astype(np.int64), pad


def _check(got, want, sizes, L, codes=None, gid=None, lo=None, hi=None):
    """got / want: dict(tajimas_d, seg, k_hat[, n_loci]) of equal shapes (cells x G); L: loci summed per cell"""
    G = len(sizes)
    seg, k, d = np.asarray(got["seg"]).reshape(-1, G), np.asarray(got["k_hat"]).reshape(-1, G), np.asarray(got["tajimas_d"]).reshape(-1, G)
    wseg, wk, wd = want["seg"].reshape(-1, G), want["k_hat"].reshape(-1, G), want["tajimas_d"].reshape(-1, G)
    L = np.broadcast_to(np.asarray(L, dtype=np.float64).reshape(-1, 1), k.shape)
    assert np.array_equal(seg, wseg)
    if "n_loci" in want:
        assert np.array_equal(np.asarray(got["n_loci"]).reshape(-1, G), want["n_loci"].reshape(-1, G))
    for a, b in ((k, wk), (d, wd)):
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
        assert np.array_equal(np.isneginf(a), np.isneginf(b))
    fk = np.isfinite(wk)
    assert np.all(np.abs(k[fk] - wk[fk]) <= L[fk] * 2.0 ** -52 * wk[fk])
    for g in range(G):
        if sizes[g] == 0:
            continue
        n_all = 2 * int(sizes[g])
        a1 = tr.consts(n_all)[0]
        f = np.isfinite(wd[:, g])
        with np.errstate(invalid="ignore", divide="ignore"):
            bound = 2.0 ** -50 * (L[:, g] * wk[:, g] + wseg[:, g] / a1) / np.sqrt(tr.var_d(n_all, wseg[:, g])) + 2.0 ** -48 * np.abs(wd[:, g])
        assert np.all(np.abs(d[f, g] - wd[f, g]) <= bound[f]), (g, np.max(np.abs(d[f, g] - wd[f, g]) / bound[f]))
    if codes is None:
        return
    # the numerator from the device's k_hat against the exact route
    x, v = tr.group_counts(codes, gid, G)
    cells = [(w, g) for g in range(G) if sizes[g] > 0 for w in range(k.shape[0]) if np.isfinite(k[w, g])]
    m = codes.shape[1]
    if lo is None:
        planted = []
    else:  # the pi = 1 locus alone, the whole view, the windows across the chunk border
        chunk = _chunk()
        planted = [(w, g) for w, g in cells
                   if (lo[w], hi[w]) in ((m // 2, m // 2 + 1), (0, m)) or (lo[w] < chunk < hi[w] and hi[w] - lo[w] <= 70)]
    for w, g in planted + cells[::max(1, -(-len(cells) // EXACT_CELLS))]:
        n_all = 2 * int(sizes[g])
        a, b = (0, codes.shape[1]) if lo is None else (lo[w], hi[w])
        eseg, ek = tr.sums_exact(x[a:b, g], v[a:b, g])
        assert eseg == seg[w, g] and ek is not None
        num = Fraction(float(k[w, g])) - Fraction(eseg) / Fraction(tr.consts(n_all)[0])
        a1x = tr.a1_exact(n_all)
        assert abs(num - (ek - Fraction(eseg) / a1x)) <= Fraction(1, 2 ** 50) * ((b - a) * ek + Fraction(eseg) / a1x)


@pytest.fixture(scope="module")
def cases():
    """panel, store and reference of a shape, made once and left unchanged"""
    import tidypopgen_amd as tpg

    made = {}

    def get(n, G, m):
        if (n, G, m) not in made:
            codes, gid = tr.panel(7 * n + G, n, m, G)
            big, rows, cols = _embed(codes, m)
            X = tpg.FBM.from_numpy(np.asfortranarray(big), code256=tpg.CODE_012)
            lo, hi, pad = _window_lists(tpg, m, _chunk())
            made[(n, G, m)] = dict(codes=codes, gid=gid, X=X, rows=rows, cols=cols, lo=lo, hi=hi, pad=pad,
                                   sizes=tr.group_sizes(n, gid, G), ref={})
        return made[(n, G, m)]

    def ref(c, G, min_loci):
        if min_loci not in c["ref"]:
            c["ref"][min_loci] = tr.windows_ref(c["codes"], c["gid"], G, c["lo"], c["hi"], c["pad"], min_loci)
        return c["ref"][min_loci]

    get.ref = ref
    return get


@pytest.mark.parametrize("m_index", range(6))
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("n", NS)
def test_windows_against_the_reference(cases, n, G, m_index):
    import tidypopgen_amd as tpg

    m = _ms()[m_index]
    c = cases(n, G, m)
    v = tpg.View(c["X"], c["rows"], c["cols"])
    assert (v.n, v.m) == (n, m)
    for min_loci in (1, 3):
        want = cases.ref(c, G, min_loci)
        got = tpg.tajima_windows(v, c["gid"], G, c["lo"], c["hi"], c["pad"], min_loci)
        for key in ("tajimas_d", "seg", "k_hat", "n_loci"):
            assert got[key].shape == (len(c["lo"]), G)
        pad = c["pad"].astype(bool)
        assert (got["n_loci"][pad] == -1).all() and (got["seg"][pad] == 0).all() and np.isnan(got["k_hat"][pad]).all()
        assert np.isnan(got["tajimas_d"][got["n_loci"] < min_loci]).all()
        exact = dict(codes=c["codes"], gid=c["gid"], lo=c["lo"], hi=c["hi"]) if min_loci == 1 else {}
        _check(got, want, c["sizes"], c["hi"] - c["lo"], **exact)
        # D from the additive pieces on the host reproduces the device's D
        for g in range(G):
            if c["sizes"][g] == 0:
                assert np.isnan(got["tajimas_d"][:, g]).all() and np.isnan(got["k_hat"][:, g]).all()
                continue
            ok = got["n_loci"][:, g] >= min_loci
            host = np.array([tpg.tajimas_d_from_sums(2 * int(c["sizes"][g]), s, k)
                             for s, k in zip(got["seg"][ok, g], got["k_hat"][ok, g])])
            assert tr.max_ulp(got["tajimas_d"][ok, g], host) <= 4
    if m >= 64 and n == 65:  # the cases are not vacuous
        d = cases.ref(c, G, 1)["tajimas_d"]
        assert np.isfinite(d).any() and np.isnan(d).any()


def _bits(r):
    return {k: np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32) for k, a in r.items()}


@pytest.mark.parametrize("n,G,m_index", [(65, 3, 4), (13, 33, 5)])
def test_determinism_of_the_window_results(cases, n, G, m_index):
    import tidypopgen_amd as tpg
    from tidypopgen_amd import _lib

    m = _ms()[m_index]
    c = cases(n, G, m)
    v = tpg.View(c["X"], c["rows"], c["cols"])
    lo, hi, pad = c["lo"], c["hi"], c["pad"]
    nw = len(lo)
    base = _bits(tpg.tajima_windows(v, c["gid"], G, lo, hi, pad, 1))
    again = _bits(tpg.tajima_windows(v, c["gid"], G, lo, hi, pad, 1))
    assert all(np.array_equal(base[k], again[k]) for k in base)
    perm = np.random.default_rng(3).permutation(nw)
    shuffled = _bits(tpg.tajima_windows(v, c["gid"], G, lo[perm], hi[perm], pad[perm], 1))
    assert all(np.array_equal(base[k][perm], shuffled[k]) for k in base)
    sub = np.arange(5, nw, 7)  # some of the windows inside another list
    longer = _bits(tpg.tajima_windows(v, c["gid"], G, np.r_[0, lo[sub], 0], np.r_[m, hi[sub], 0], np.r_[0, pad[sub], 1].astype(np.uint8), 1))
    assert all(np.array_equal(base[k][sub], longer[k][1:-1]) for k in base)
    # inputs and outputs in device memory
    ctx = v.ctx
    gid = None if c["gid"] is None else np.ascontiguousarray(c["gid"], dtype=np.int32)
    host_out = dict(tajimas_d=np.zeros((nw, G), order="F"), seg=np.zeros((nw, G), dtype=np.int64, order="F"),
                    k_hat=np.zeros((nw, G), order="F"), n_loci=np.zeros((nw, G), dtype=np.int32, order="F"))
    dev = {}
    try:
        for name, a in (("lo", lo), ("hi", hi), ("pad", pad)):
            dev[name] = ctx.dev_alloc(a.nbytes)
            _lib.check(_lib.lib.tpg_dev_from_host(ctx.h, dev[name], C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes)))
        for name, a in host_out.items():
            dev[name] = ctx.dev_alloc(a.nbytes)
        _lib.check(_lib.lib.tpg_windows_pop_tajimas_d(
            ctx.h, v.h, None if gid is None else C.c_void_p(gid.ctypes.data), C.c_int(G), None, dev["lo"], dev["hi"], dev["pad"],
            C.c_int64(nw), C.c_int(1), dev["tajimas_d"], dev["seg"], dev["k_hat"], dev["n_loci"]))
        for name, a in host_out.items():
            _lib.check(_lib.lib.tpg_dev_to_host(ctx.h, C.c_void_p(a.ctypes.data), dev[name], C.c_size_t(a.nbytes)))
    finally:
        for p in dev.values():
            ctx.dev_free(p)
    on_device = _bits(host_out)
    assert all(np.array_equal(base[k], on_device[k]) for k in base)
    # the optional outputs may be left out
    d_only = np.zeros((nw, G), order="F")
    _lib.check(_lib.lib.tpg_windows_pop_tajimas_d(
        ctx.h, v.h, None if gid is None else C.c_void_p(gid.ctypes.data), C.c_int(G), None, C.c_void_p(lo.ctypes.data),
        C.c_void_p(hi.ctypes.data), None, C.c_int64(nw), C.c_int(1), C.c_void_p(d_only.ctypes.data), None, None, None))
    unpadded = _bits(tpg.tajima_windows(v, c["gid"], G, lo, hi, None, 1))
    assert np.array_equal(d_only.view(np.uint64), unpadded["tajimas_d"])


def test_public_window_function_and_its_argument_errors(cases):
    import tidypopgen_amd as tpg

    n, G, m = 65, 3, 300
    c = cases(n, G, m)
    chrom = np.r_[np.ones(m // 2, dtype=np.int64), np.full(m - m // 2, 2)]
    for complete in (False, True):
        out = tpg.windows_pop_tajimas_d(c["X"], c["rows"], c["cols"], c["gid"], G, chrom, window_size=7, step_size=2, min_loci=2,
                                        complete=complete, return_sums=True)
        wr = tpg.window_index_ranges(chrom, None, 7, 2, complete=complete)
        want = tr.windows_ref(c["codes"], c["gid"], G, wr["lo"], wr["hi"], wr["pad_na"], 2)
        assert np.array_equal(out["chromosome"], wr["chromosome"]) and np.array_equal(out["start"], wr["start"])
        assert np.array_equal(out["end"], wr["end"])
        nl = want["n_loci"].astype(float)
        nl[want["n_loci"] < 0] = np.nan
        assert np.array_equal(out["n_loci"], nl, equal_nan=True) and np.isnan(out["n_loci"]).any() == complete
        _check(dict(tajimas_d=out["tajimas_d"], seg=out["seg"], k_hat=out["k_hat"]),
               {k: want[k] for k in ("tajimas_d", "seg", "k_hat")}, c["sizes"], wr["hi"] - wr["lo"])
    one = tpg.windows_pop_tajimas_d(c["X"], c["rows"], c["cols"], None, 0, chrom, window_size=10, step_size=10)
    assert one["tajimas_d"].shape[1] == 1 and set(one) == {"chromosome", "start", "end", "n_loci", "tajimas_d"}
    kw = dict(window_size=3, step_size=2)
    with pytest.raises(ValueError, match="same number of rows"):
        tpg.windows_pop_tajimas_d(c["X"], c["rows"], c["cols"], c["gid"], G, chrom[:-1], **kw)
    with pytest.raises(ValueError, match="min_loci must be positive"):
        tpg.windows_pop_tajimas_d(c["X"], c["rows"], c["cols"], c["gid"], G, chrom, min_loci=0, **kw)
    with pytest.raises(ValueError, match="min_loci must be less than window_size"):
        tpg.windows_pop_tajimas_d(c["X"], c["rows"], c["cols"], c["gid"], G, chrom, min_loci=4, **kw)
    with pytest.raises(ValueError, match="window_size must be positive"):
        tpg.windows_pop_tajimas_d(c["X"], c["rows"], c["cols"], c["gid"], G, chrom, window_size=0, step_size=2)
    with pytest.raises(ValueError, match="step_size must be positive"):
        tpg.windows_pop_tajimas_d(c["X"], c["rows"], c["cols"], c["gid"], G, chrom, window_size=3, step_size=0)
    v = tpg.View(c["X"], c["rows"], c["cols"])
    for lo, hi, ml in (([5], [4], 1), ([0], [m + 1], 1), ([-1], [3], 1), ([0], [3], 0)):
        with pytest.raises(tpg._lib.TpgError) as e:
            tpg.tajima_windows(v, c["gid"], G, lo, hi, None, ml)
        assert e.value.code == 1  # TPG_EINVAL
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.tajima_windows(v, c["gid"], G, [0], [3], None, 1, ploidy=np.r_[np.full(n - 1, 2.0), 1.0])
    assert e.value.code == 1
    # more windows than one launch takes are refused as an argument error, before anything is read or launched
    one = np.zeros(1, dtype=np.int64)
    d1 = np.zeros(G)
    rc = tpg._lib.lib.tpg_windows_pop_tajimas_d(v.ctx.h, v.h, None, C.c_int(1), None, C.c_void_p(one.ctypes.data),
                                                C.c_void_p(one.ctypes.data), None, C.c_int64(2 ** 24), C.c_int(1),
                                                C.c_void_p(d1.ctypes.data), None, None, None)
    assert rc == 1
    empty = tpg.tajima_windows(v, c["gid"], G, [], [], None, 1)  # nw == 0
    assert empty["tajimas_d"].shape == (0, G)


@pytest.mark.parametrize("m_index", (0, 3, 4, 5))
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("n", NS)
def test_whole_view_against_the_reference(cases, n, G, m_index):
    import tidypopgen_amd as tpg

    m = _ms()[m_index]
    c = cases(n, G, m)
    keep = np.setdiff1d(np.arange(m), [m // 3]) if m > 2 else np.arange(m)  # without the locus that makes group 0 NaN
    for loci in (np.arange(m), keep):
        codes = c["codes"][:, loci]
        want = tr.pop_ref(codes, c["gid"], G)
        got = tpg.pop_tajimas_d(c["X"], c["rows"], c["cols"][loci], c["gid"], G, return_sums=True)
        plain = tpg.pop_tajimas_d(c["X"], c["rows"], c["cols"][loci], c["gid"], G)
        if c["gid"] is None:
            assert isinstance(plain, float) and isinstance(got["tajimas_d"], float)
            got = {k: np.array([a]) for k, a in got.items()}
            plain = np.array([plain])
        assert plain.shape == (G,) and np.array_equal(plain.view(np.uint64), got["tajimas_d"].view(np.uint64))
        _check(got, want, c["sizes"], len(loci), codes=codes, gid=c["gid"])
    if m >= 65 and G == 3:
        assert np.isfinite(want["tajimas_d"][:2]).all() and not np.isfinite(want["tajimas_d"][2])


def test_whole_view_at_200000_loci():
    import tidypopgen_amd as tpg

    n, G, m = 40, 3, 200000
    codes, gid = tr.panel(11, n, m, G)
    X = tpg.FBM.from_numpy(np.asfortranarray(codes), code256=tpg.CODE_012)
    sizes = tr.group_sizes(n, gid, G)
    keep = np.setdiff1d(np.arange(m), [m // 3])
    want = tr.pop_ref(codes[:, keep], gid, G)
    assert np.isfinite(want["tajimas_d"][:2]).all() and want["seg"][0] > 100000
    got = tpg.pop_tajimas_d(X, None, keep + 1, gid, G, return_sums=True)
    _check(got, want, sizes, len(keep), codes=codes[:, keep], gid=gid)
    again = tpg.pop_tajimas_d(X, None, keep + 1, gid, G, return_sums=True)
    assert all(np.array_equal(got[k].view(np.uint64), again[k].view(np.uint64)) for k in got)
    whole = tpg.pop_tajimas_d(X, None, None, gid, G, return_sums=True)  # the all-missing locus of group 0 is back
    _check(whole, tr.pop_ref(codes, gid, G), sizes, m)
    assert np.isnan(whole["tajimas_d"][0]) and np.isnan(whole["k_hat"][0])
    # everybody in one group, and the host finish from the sums
    ung = tpg.pop_tajimas_d(X, None, keep + 1, return_sums=True)
    w1 = tr.pop_ref(codes[:, keep], None, 1)
    _check({k: np.array([a]) for k, a in ung.items()}, w1, np.array([n]), len(keep), codes=codes[:, keep], gid=None)
    assert tr.max_ulp([tpg.tajimas_d_from_sums(2 * n, ung["seg"], ung["k_hat"])], [ung["tajimas_d"]]) <= 4


def test_single_individual_and_ploidy():
    import tidypopgen_amd as tpg

    codes, gid = tr.panel(2, 13, 65, 3)
    X = tpg.FBM.from_numpy(np.asfortranarray(codes), code256=tpg.CODE_012)
    assert np.isnan(tpg.pop_tajimas_d(X, [4]))  # R/pop_tajimas_d.R:91-95: NA
    with pytest.raises(tpg._lib.TpgError) as e:  # ... but a non-diploid individual is refused there too
        tpg.pop_tajimas_d(X, [4], ploidy=[1.0])
    assert e.value.code == 1
    r = tpg.pop_tajimas_d(X, [4], return_sums=True)
    assert np.isnan(r["tajimas_d"]) and np.isnan(r["k_hat"])
    assert np.isfinite(tpg.pop_tajimas_d(X, [4, 5, 6, 7], np.arange(1, 20)))
    assert np.array_equal(tpg.pop_tajimas_d(X, None, None, gid, 3, ploidy=np.full(13, 2.0)), tpg.pop_tajimas_d(X, None, None, gid, 3),
                          equal_nan=True)
    pl = np.full(13, 2.0)
    pl[3] = 1.0
    for call in (lambda: tpg.pop_tajimas_d(X, None, None, gid, 3, ploidy=pl), lambda: tpg.pop_tajimas_d(X, ploidy=pl)):
        with pytest.raises(tpg._lib.TpgError) as e:
            call()
        assert e.value.code == 1  # TPG_EINVAL
    with pytest.raises(tpg._lib.TpgError):
        tpg.pop_tajimas_d(X, None, None, np.r_[gid[:-1], 3], 3)  # a group id out of range
