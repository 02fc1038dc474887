"""GPU: the fused window scan (include/tpg.h "windowed pairwise Fst") against the numpy restatement tests/winfst_ref.py, fed the
by-locus numerators and denominators tpg_pairwise_pop_fst(return_num_dem = 1) writes for the same view.

What is compared how.  n_num and n_den are integers: equality.  The NaN / +-Inf patterns of mean_num, mean_den and fst:
equality.  fst is one IEEE division of the two returned means: bitwise.  A window sum of L non-NaN doubles x_j: the device adds
them in the order the header states, the float route one after the other; each is within L 2^-52 sum|x_j| of the exact sum, so
EVERY cell has |mean n - float sum| <= 2 L 2^-52 sum|x_j| + 2^-51 |sum| (the last term: the division by n and the
multiplication back, on either side).  Against the exact route (math.fsum of the same doubles) the bound is the header's,
|mean n - exact| <= L 2^-52 sum|x_j| + 2^-52 |exact|, on every cell where a case has at most EXACT_CELLS of them and otherwise
on the border / planted windows plus an even stride of EXACT_CELLS cells."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from tests import tajima_ref as tr
from tests import winfst_ref as wr

pytestmark = pytest.mark.gpu

NS = (13, 65)
GS = (2, 3, 9, 33)  # P = 1, 3, 36, 528 (528: eight pairs per thread, more than one pass of 256)
METHODS = ("Hudson", "WC84", "Nei87")
EXACT_CELLS = 1500
EINVAL = 1


def _chunk():
    from tidypopgen_amd import api

    return api.WINFST_CHUNK_LOCI


def _ms():
    c = _chunk()
    return (1, c - 1, c, c + 1, 2 * c + 3, 300)


def _embed(codes, seed):
    """the panel as rows / columns of a larger store: -> bytes, ind_row, ind_col (1-based)"""
    n, m = codes.shape
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.permutation(n + 3)[:n])
    cols = np.sort(rng.permutation(m + 5)[:m])
    big = rng.integers(0, 4, size=(n + 3, m + 5)).astype(np.uint8)
    big[np.ix_(rows, cols)] = codes
    return big, rows + 1, cols + 1


def _border_windows(m, c):
    """windows that start or end exactly on a chunk border, straddle one, or hold whole chunks with a ragged head and tail"""
    w = []
    if m > c:
        w += [(c - 5, c + 1), (max(0, c - 70), c + 1)]          # straddle the first border
    if m >= c + 7:
        w += [(c, c + 7), (c - 7, c), (0, c)]                   # start on it, end on it, exactly the first chunk
    if m >= 2 * c + 3:
        w += [(c, 2 * c), (3, 2 * c + 2), (0, 2 * c + 3)]       # one whole chunk; ragged head, one chunk, ragged tail; two chunks + tail
    if m >= 4 * c + 10:
        w += [(5, 4 * c + 9), (c - 1, 3 * c + 1)]               # ragged head, >= 2 whole chunks, ragged tail
    return w


def _window_lists(tpg, m, c):
    """every list of the issue, end to end: -> lo, hi, pad_na, the border windows among them"""
    one = np.ones(m, dtype=np.int64)
    two = np.r_[np.ones(m // 2, dtype=np.int64), np.full(m - m // 2, 2)]
    rng = np.random.default_rng(m)
    bp = np.cumsum(rng.choice([1, 3, 40, 700], size=m, p=[0.5, 0.3, 0.15, 0.05]))  # gaps wider than a window: empty windows
    parts = [tpg.window_index_ranges(one, None, 1, 1),
             tpg.window_index_ranges(two, None, 3, 2),
             tpg.window_index_ranges(one, None, c, 1),
             tpg.window_index_ranges(one, None, c + 1, 1),
             tpg.window_index_ranges(one, bp, 100, 100, size_unit="bp"),
             tpg.window_index_ranges(two, None, 3, 2, complete=True),
             tpg.window_index_ranges(one, bp, 250, 100, size_unit="bp", complete=True)]
    border = _border_windows(m, c)
    extra = [(0, m), (m // 2, m // 2), (m, m)] + border  # the whole view and two empty windows
    lo = np.concatenate([p["lo"] for p in parts] + [[a for a, _ in extra]])
    hi = np.concatenate([p["hi"] for p in parts] + [[b for _, b in extra]])
    pad = np.concatenate([p["pad_na"] for p in parts] + [np.zeros(len(extra))]).astype(np.uint8)
    assert pad.any() and (lo == hi).any()
    assert bool(border) == (m > c)
    if m >= 4 * c + 10:
        assert any(-(-a // c) + 2 <= b // c and a % c and b % c for a, b in border)
    return lo.astype(np.int64), hi.astype(np.int64), pad, set(border)


def _ploidy(n, gid, G):
    """mixed ploidy for Hudson: the members of the last non-empty group (a group of one, tests/tajima_ref.py: panel) are
    pseudohaploid, so that group has ONE typed allele wherever it is typed: p q / (n - 1) is 0 / 0 there, den is finite"""
    k = G if G <= n else max(2, n // 3)
    pl = np.full(n, 2.0)
    pl[gid == k - 1] = 1.0
    return pl


@pytest.fixture(scope="module")
def cases():
    """panel, store, window list, by-locus terms and reference of a shape, made once and left unchanged"""
    import tidypopgen_amd as tpg

    made = {}

    def get(n, G, m):
        if (n, G, m) not in made:
            codes, gid = tr.panel(7 * n + G, n, m, G)
            big, rows, cols = _embed(codes, m)
            X = tpg.FBM.from_numpy(np.asfortranarray(big), code256=tpg.CODE_012)
            lo, hi, pad, border = _window_lists(tpg, m, _chunk())
            made[(n, G, m)] = dict(codes=codes, gid=gid, X=X, rows=rows, cols=cols, lo=lo, hi=hi, pad=pad, border=border,
                                   hap=_ploidy(n, gid, G), terms={}, ref={})
        return made[(n, G, m)]

    def terms(c, G, method):
        """by-locus num / den of the same view from the by-locus path (Hudson: with the mixed ploidy)"""
        if method not in c["terms"]:
            pl = c["hap"] if method == "Hudson" else None
            r = tpg.pairwise_pop_fst(c["X"], c["rows"], c["cols"], c["gid"], G, pl, method, return_num_dem=True)
            c["terms"][method] = (r["Fst_by_locus_num"], r["Fst_by_locus_den"], pl)
        return c["terms"][method]

    def ref(c, G, method, min_loci):
        if (method, min_loci) not in c["ref"]:
            num, den, _ = terms(c, G, method)
            c["ref"][(method, min_loci)] = wr.windows_ref(num, den, c["lo"], c["hi"], c["pad"], min_loci)
        return c["ref"][(method, min_loci)]

    get.terms, get.ref = terms, ref
    return get


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _ratio_is_exact(fst, mean_num, mean_den):
    """fst is ONE IEEE division of the two returned means: the same bits as the host's division, a NaN for a NaN (the sign and
    payload of an invalid operation's NaN are the processor's own)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        q = mean_num / mean_den
    return np.array_equal(np.isnan(fst), np.isnan(q)) and np.array_equal(_bits(fst)[~np.isnan(q)], _bits(q)[~np.isnan(q)])


def _same_kind(a, b):
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
            and np.array_equal(np.isneginf(a), np.isneginf(b)))


def _check(got, want, num, den, lo, hi, special):
    """got: dict of windows_fst(return_parts=True); want: windows_ref at the same min_loci"""
    assert np.array_equal(got["n_num"], want["n_num"]) and np.array_equal(got["n_den"], want["n_den"])
    for key in ("mean_num", "mean_den", "fst"):
        assert _same_kind(got[key], want[key]), key
    assert _ratio_is_exact(got["fst"], got["mean_num"], got["mean_den"])
    worst = 0.0
    for mean, cnt, ab, x in (("mean_num", "n_num", "abs_num", num), ("mean_den", "n_den", "abs_den", den)):
        n = want[cnt].astype(np.float64)
        f = np.isfinite(want[mean]) & np.isfinite(want[ab])
        s_got, s_ref = got[mean] * n, want[mean] * n
        bound = 2 * n * 2.0 ** -52 * want[ab] + 2.0 ** -51 * np.abs(s_ref)  # (2^-51: the reference's mean is rounded as well)
        assert np.all(np.abs(s_got[f] - s_ref[f]) <= bound[f]), mean
        # the exact route
        cells = np.argwhere(f)
        if len(cells) > EXACT_CELLS:
            sp = [tuple(c) for c in cells if (lo[c[0]], hi[c[0]]) in special][:4 * EXACT_CELLS]
            cells = sp + [tuple(c) for c in cells[::-(-len(cells) // EXACT_CELLS)]]
        for w, p in cells:
            ex = wr.sum_exact(x[lo[w]:hi[w], p])
            err = abs(got[mean][w, p] * n[w, p] - ex)
            tol = n[w, p] * 2.0 ** -52 * want[ab][w, p] + 2.0 ** -52 * abs(ex)
            assert err <= tol, (mean, w, p, err, tol)
            worst = max(worst, err / tol if tol > 0 else 0.0)
    return worst


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("n", NS)
def test_windows_against_the_reference(cases, n, G, method):
    import tidypopgen_amd as tpg

    seen = set()
    worst = 0.0
    for m in _ms():
        c = cases(n, G, m)
        num, den, pl = cases.terms(c, G, method)
        v = tpg.View(c["X"], c["rows"], c["cols"])
        special = c["border"] | {(0, m), (m // 2, m // 2 + 1), (m // 3, m // 3 + 1)}
        base = None
        for min_loci in (1, 2, 5):
            got = tpg.windows_fst(v, c["gid"], G, c["lo"], c["hi"], c["pad"], min_loci, pl, method, return_parts=True)
            want = cases.ref(c, G, method, min_loci)
            if min_loci == 1:
                worst = max(worst, _check(got, want, num, den, c["lo"], c["hi"], special))
                base = got
            else:  # min_loci changes only which cells are NaN
                assert np.array_equal(got["n_num"], base["n_num"]) and np.array_equal(got["n_den"], base["n_den"])
                for key, cnt in (("mean_num", "n_num"), ("mean_den", "n_den")):
                    short = (base[cnt] < min_loci)
                    assert np.isnan(got[key][short]).all()
                    assert got[key][~short].tobytes() == base[key][~short].tobytes()
                assert _same_kind(got["fst"], want["fst"])
                assert _ratio_is_exact(got["fst"], got["mean_num"], got["mean_den"])
        v.free()
        # what the case is there for
        if (base["n_num"] != base["n_den"]).any():
            seen.add("n_num != n_den")
        if (base["n_num"] == -1).any():
            seen.add("pad")
        if ((base["n_num"] == 0) & (c["lo"] == c["hi"])[:, None]).any():
            seen.add("empty")
        if c["border"]:
            seen.add("border")
        if m > 2:
            j = m // 3  # group 0 wholly missing: every pair with population 1 has no term there
            w = np.where((c["lo"] == j) & (c["hi"] == j + 1) & (c["pad"] == 0))[0][0]
            pairs = tpg.combn2(G)
            assert (base["n_den"][w, pairs[0] == 1] == 0).all() and np.isnan(base["fst"][w, pairs[0] == 1]).all()
            seen.add("group missing")
            a = m // 4  # the monomorphic stretch
            w = np.where((c["lo"] == a) & (c["hi"] == a + 1) & (c["pad"] == 0))[0][0]
            assert np.all((base["mean_den"][w] == 0) | np.isnan(base["mean_den"][w]))
            seen.add("monomorphic")
    print(f"n={n} G={G} {method}: worst error / bound against the exact route {worst:.3f}")
    assert {"pad", "empty", "border", "group missing", "monomorphic"} <= seen
    if method == "Hudson":
        assert "n_num != n_den" in seen  # the pseudohaploid group of one typed allele


def _call(tpg, v, gid, G, pl, method, pairs_c, lo, hi, pad, nw, min_loci, outs):
    """the C entry point itself; an argument is a numpy array, None, or device memory (the c_void_p of Context.dev_alloc)"""
    from tidypopgen_amd.api import FST_METHODS, _ptr

    def p(x):
        return x if isinstance(x, C.c_void_p) else _ptr(x)

    return tpg._lib.lib.tpg_windows_pairwise_pop_fst(v.ctx.h, v.h, p(gid), G, p(pl), FST_METHODS[method], p(pairs_c), len(pairs_c),
                                                     p(lo), p(hi), p(pad), nw, min_loci, *[p(o) for o in outs])


@pytest.mark.parametrize("n,G,m,method", [(65, 9, 300, "Hudson"), (13, 33, 131, "WC84")])
def test_bits_do_not_depend_on_the_call(cases, n, G, m, method):
    import tidypopgen_amd as tpg

    c = cases(n, G, m)
    _, _, pl = cases.terms(c, G, method)
    v = tpg.View(c["X"], c["rows"], c["cols"])
    lo, hi, pad = c["lo"], c["hi"], c["pad"]
    nw = len(lo)
    keys = ("fst", "mean_num", "mean_den", "n_num", "n_den")
    a = tpg.windows_fst(v, c["gid"], G, lo, hi, pad, 2, pl, method, return_parts=True)
    b = tpg.windows_fst(v, c["gid"], G, lo, hi, pad, 2, pl, method, return_parts=True)
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k
    # a permuted list, and a list with other windows appended
    perm = np.random.default_rng(1).permutation(nw)
    p = tpg.windows_fst(v, c["gid"], G, lo[perm], hi[perm], pad[perm], 2, pl, method, return_parts=True)
    more = tpg.windows_fst(v, c["gid"], G, np.r_[lo, 0, 1, m // 2], np.r_[hi, m, m - 1, m], np.r_[pad, 0, 0, 1], 2, pl, method,
                           return_parts=True)
    for k in keys:
        assert np.array_equal(_bits(p[k]), _bits(a[k][perm])), k
        assert np.array_equal(_bits(more[k][:nw]), _bits(a[k])), k
    # the optional outputs NULL
    only = tpg.windows_fst(v, c["gid"], G, lo, hi, pad, 2, pl, method)
    assert list(only) == ["fst"] and only["fst"].tobytes() == a["fst"].tobytes()
    # windows and outputs in device memory
    ctx, lib = v.ctx, tpg._lib.lib
    P = a["fst"].shape[1]
    pairs_c = np.ascontiguousarray(tpg.combn2(G).T)
    host_in = (lo, hi, pad)
    d_in = [ctx.dev_alloc(x.nbytes) for x in host_in]
    sizes = (8, 8, 8, 4, 4)
    d_out = [ctx.dev_alloc(s * nw * P) for s in sizes]
    try:
        for d, x in zip(d_in, host_in):
            assert lib.tpg_dev_from_host(ctx.h, d, x.ctypes.data, x.nbytes) == 0
        gid = np.ascontiguousarray(c["gid"], dtype=np.int32)
        assert _call(tpg, v, gid, G, pl, method, pairs_c, d_in[0], d_in[1], d_in[2], nw, 2, d_out) == 0
        for k, d in zip(keys, d_out):
            back = np.zeros_like(a[k])
            assert lib.tpg_dev_to_host(ctx.h, back.ctypes.data, d, back.nbytes) == 0
            assert back.tobytes() == a[k].tobytes(), k
    finally:
        for d in d_in + d_out:
            ctx.dev_free(d)
    v.free()


def test_errors_leave_the_outputs_untouched(cases):
    import tidypopgen_amd as tpg

    n, G, m = 13, 3, 300
    c = cases(n, G, m)
    v = tpg.View(c["X"], c["rows"], c["cols"])
    gid = np.ascontiguousarray(c["gid"], dtype=np.int32)
    pairs = np.ascontiguousarray(tpg.combn2(G).T)
    lo, hi, pad = np.array([0, 10], dtype=np.int64), np.array([5, 20], dtype=np.int64), np.zeros(2, dtype=np.uint8)

    def run(method="Hudson", pl=None, pairs_c=pairs, lo=lo, hi=hi, nw=2, min_loci=1):
        outs = [np.full((2, len(pairs_c)), 7.0, order="F"), np.full((2, len(pairs_c)), 7.0, order="F"),
                np.full((2, len(pairs_c)), 7.0, order="F"), np.full((2, len(pairs_c)), 7, dtype=np.int32, order="F"),
                np.full((2, len(pairs_c)), 7, dtype=np.int32, order="F")]
        rc = _call(tpg, v, gid, G, pl, method, pairs_c, lo, hi, pad, nw, min_loci, outs)
        return rc, all((o == 7).all() for o in outs)

    assert run() == (0, False)
    bad_pair0, bad_pair1 = pairs.copy(), pairs.copy()
    bad_pair0[1, 0], bad_pair1[2, 1] = 0, G + 1
    for kw in (dict(hi=np.array([5, m + 1], dtype=np.int64)), dict(lo=np.array([6, 10], dtype=np.int64)), dict(min_loci=0),
               dict(pairs_c=bad_pair0), dict(pairs_c=bad_pair1), dict(method="WC84", pl=c["hap"]), dict(method="Nei87", pl=c["hap"]),
               dict(nw=-1), dict(nw=(1 << 24))):
        assert run(**kw) == (EINVAL, True), kw
    rc, untouched = run(method="WC84", pl=c["hap"])
    assert rc == EINVAL and "only method = Hudson is valid when the data include pseudohaploids" in tpg._lib.lib.tpg_last_error().decode()
    assert run(nw=0) == (0, True)  # TPG_OK, nothing written
    outs = [np.zeros((2, 3), order="F")] + [None] * 4
    assert _call(tpg, v, gid, G, None, "Hudson", pairs[:0], lo, hi, pad, 2, 1, outs) == EINVAL  # P = 0
    with pytest.raises(ValueError):
        tpg.windows_fst(v, gid, G, lo, hi[:1])
    with pytest.raises(ValueError):
        tpg.windows_fst(v, gid, G, lo, hi, method="nope")
    v.free()


@pytest.mark.parametrize("n,m,G", [(10, 8, 3), (300, 2500, 6)])
def test_routes(n, m, G):
    """route = "fused" against route = "staged" and against the oracle, at the tolerances test_windows_pairwise_pop_fst of
    tests/test_gpu_parity.py holds the staged route to"""
    import tidypopgen_amd as tpg

    fbm = orc.synth_fbm(91, n, m, npop=G, miss=0.1)
    gid = (np.arange(n) % G).astype(np.int32)
    X = tpg.FBM.from_numpy(fbm)
    chrom = np.array(["chr1"] * (m // 3) + ["chr2"] * (m - m // 3))
    rng = np.random.default_rng(5)
    pos = np.concatenate([np.sort(rng.integers(1, 50 * m, m // 3)), np.sort(rng.integers(1, 50 * m, m - m // 3))])
    for kw in (dict(window_size=3, step_size=2, size_unit="snp", min_loci=2),
               dict(window_size=40, step_size=40, size_unit="snp", min_loci=1, complete=True),
               dict(window_size=5000, step_size=2500, size_unit="bp", min_loci=2)):
        t = tpg.windows_pairwise_pop_fst(X, None, None, gid, G, chrom, pos, route="fused", **kw)
        s = tpg.windows_pairwise_pop_fst(X, None, None, gid, G, chrom, pos, route="staged", **kw)
        d = tpg.windows_pairwise_pop_fst(X, None, None, gid, G, chrom, pos, **kw)
        assert d["fst"].tobytes() == s["fst"].tobytes()  # staged is the default
        with np.errstate(invalid="ignore", divide="ignore"):
            o = orc.windows_pairwise_pop_fst(fbm, None, None, gid, G, chrom, pos, **kw)
        for other in (s, o):
            assert np.array_equal(t["start"], other["start"]) and np.array_equal(t["end"], other["end"])
            assert list(t["chromosome"]) == list(other["chromosome"])
            assert np.array_equal(np.isnan(t["fst"]), np.isnan(other["fst"]))
            assert np.allclose(t["fst"], other["fst"], rtol=1e-11, atol=1e-14, equal_nan=True)
    t = tpg.windows_pairwise_pop_fst(X, None, None, gid, G, chrom, pos, window_size=3, step_size=2, size_unit="snp", min_loci=2,
                                     route="fused")
    r = tpg.window_index_ranges(chrom, pos, 3, 2, "snp")
    for w in (0, len(r["lo"]) - 1):
        loci = np.arange(r["lo"][w] + 1, r["hi"][w] + 1, dtype=np.int32)
        if len(loci) < 2:
            continue
        alone = tpg.pairwise_pop_fst(X, None, loci, gid, G, method="Hudson")["fst_tot"]
        assert np.allclose(t["fst"][w], alone, rtol=1e-11, atol=1e-14, equal_nan=True)
    with pytest.raises(ValueError):
        tpg.windows_pairwise_pop_fst(X, None, None, gid, G, chrom, pos, window_size=3, step_size=2, route="neither")


@pytest.mark.parametrize("n,m,G", [(10, 8, 4), (300, 2500, 5)])
def test_windows_nwise_pop_pbs(n, m, G):
    import tidypopgen_amd as tpg

    fbm = orc.synth_fbm(17, n, m, npop=G, miss=0.1)
    gid = (np.arange(n) % G).astype(np.int32)
    X = tpg.FBM.from_numpy(fbm)
    chrom = np.array(["chr1"] * (m // 3) + ["chr2"] * (m - m // 3))
    kw = dict(window_size=3, step_size=2, min_loci=2) if m < 100 else dict(window_size=100, step_size=40, min_loci=2, complete=True)
    r = tpg.windows_nwise_pop_pbs(X, None, None, gid, G, chrom, return_fst=True, **kw)
    wr_ = tpg.window_index_ranges(chrom, None, kw["window_size"], kw["step_size"], "snp", kw.get("complete", False))
    nw, P = len(wr_["lo"]), G * (G - 1) // 2
    trips, tcols = tpg.api._pbs_triplets(G)
    T = len(trips)
    assert T == G * (G - 1) * (G - 2) // 6 and r["pbs"].shape == (nw, 6 * T) and r["fst"].shape == (nw, P)
    assert np.array_equal(r["start"], wr_["start"]) and np.array_equal(r["end"], wr_["end"]) and list(r["chromosome"]) == list(wr_["chromosome"])
    # names in nwise_pop_pbs order
    assert r["names"] == tpg.nwise_pop_pbs(X, None, None, gid, G)["names"] and len(r["names"]) == 6 * T
    assert r["names"][:6] == ["pbs_1.2.3", "pbs_2.1.3", "pbs_3.1.2", "pbsn1_1.2.3", "pbsn1_2.1.3", "pbsn1_3.1.2"]
    # the window Fst is the fused route's, bit for bit
    f = tpg.windows_pairwise_pop_fst(X, None, None, gid, G, chrom, route="fused", **kw)["fst"]
    assert r["fst"].tobytes() == f.tobytes()
    assert np.isfinite(f).any()
    for t in range(T):
        want = wr.pbs_one_triplet(f[:, tcols[t, 0]], f[:, tcols[t, 1]], f[:, tcols[t, 2]])
        for q in range(6):
            got = r["pbs"][:, 6 * t + q]
            assert np.array_equal(np.isnan(got), np.isnan(want[q]))
            assert np.allclose(got, want[q], rtol=1e-12, atol=1e-14, equal_nan=True)
    assert np.isfinite(r["pbs"]).any()
    # triplets = restricts the columns, bit for bit
    sel = tpg.windows_nwise_pop_pbs(X, None, None, gid, G, chrom, triplets=[(1, 2, 4)], **kw)
    k = trips.index((1, 2, 4))
    assert "fst" not in sel and sel["pbs"].tobytes() == np.asfortranarray(r["pbs"][:, 6 * k:6 * k + 6]).tobytes()
    assert sel["names"] == r["names"][6 * k:6 * k + 6]
    with pytest.raises(ValueError, match="At least 3 populations are required to compute PBS."):
        tpg.windows_nwise_pop_pbs(X, None, None, gid % 2, 2, chrom, **kw)
    with pytest.raises(ValueError, match="should be one of"):
        tpg.windows_nwise_pop_pbs(X, None, None, gid, G, chrom, fst_method="Weir", **kw)
    for bad in ([(1, 2)], [(2, 1, 3)], [(1, 2, G + 1)], [(0, 1, 2)], [(1, 1, 2)], [(1.5, 2, 3)], []):
        with pytest.raises(ValueError):
            tpg.windows_nwise_pop_pbs(X, None, None, gid, G, chrom, triplets=bad, **kw)
    with pytest.raises(ValueError, match="min_loci must be less than window_size."):
        tpg.windows_nwise_pop_pbs(X, None, None, gid, G, chrom, window_size=3, step_size=2, min_loci=4)


def _used(hip):
    fr, tot = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
    return tot.value - fr.value


@pytest.mark.parametrize("shape", ["issue", "large"])
def test_scratch_is_what_the_header_says(shape):
    """In a context of its own (an empty pool, which keeps every block it ever handed out), with the count table cached and
    windows and outputs in device memory, the device memory in use grows over one call by the call's scratch: the pool rounds a
    block up to 256 bytes (1 MiB from 1 MiB on) and the runtime below it hands out memory in pieces of up to 2 MiB, which is the
    granularity allowed for.  The runtime keeps no statistics of single allocations, so "no allocation of 8 m P bytes" is held
    against the peak: at m = 2 c + 3, G = 33 those 553 KB are below that granularity, so the same is asserted at m = 20 000
    (84 MB against 4 MB of scratch) as well.  (No other process allocates on this GPU meanwhile.)"""
    import tidypopgen_amd as tpg

    hip = C.CDLL("libamdhip64.so.7")
    c = _chunk()
    n, G, m = (13, 33, 2 * c + 3) if shape == "issue" else (65, 33, 20000)
    gran = 2 << 20
    codes, gid = tr.panel(3, n, m, G)
    ctx = tpg.Context(0)
    X = tpg.FBM.from_numpy(np.asfortranarray(codes), code256=tpg.CODE_012, ctx=ctx)
    v = tpg.View(X)
    gid = np.ascontiguousarray(gid, dtype=np.int32)
    pairs_c = np.ascontiguousarray(tpg.combn2(G).T)
    P = len(pairs_c)
    lo = np.arange(0, m - 40, 37, dtype=np.int64)
    hi = np.minimum(lo + 3 * c + 5, m).astype(np.int64)
    nw = len(lo)
    lib = tpg._lib.lib
    d_lo, d_hi, d_fst = ctx.dev_alloc(lo.nbytes), ctx.dev_alloc(hi.nbytes), ctx.dev_alloc(8 * nw * P)
    try:
        assert lib.tpg_dev_from_host(ctx.h, d_lo, lo.ctypes.data, lo.nbytes) == 0
        assert lib.tpg_dev_from_host(ctx.h, d_hi, hi.ctypes.data, hi.nbytes) == 0
        tpg.grouped_genotype_counts(v, gid, G)  # the count table of this grouping is cached on the view from here on
        ctx.sync()
        before = _used(hip)
        assert _call(tpg, v, gid, G, None, "Hudson", pairs_c, d_lo, d_hi, None, nw, 1, [d_fst, None, None, None, None]) == 0
        ctx.sync()
        growth = _used(hip) - before
        want = lib.tpg_windows_fst_scratch_bytes(m, G, P, nw)
        print(f"{shape}: m={m} P={P} nw={nw}: growth {growth} B, tpg_windows_fst_scratch_bytes {want} B, 8 m P = {8 * m * P} B")
        assert want == (m // c) * P * 24 + 8 * P and want <= m * P + (64 << 20)
        assert growth <= want + gran
        if shape == "large":
            assert growth >= want - gran and growth < 8 * m * P // 4
        back = np.zeros((nw, P), order="F")
        assert lib.tpg_dev_to_host(ctx.h, back.ctypes.data, d_fst, back.nbytes) == 0
        assert back.tobytes() == tpg.windows_fst(v, gid, G, lo, hi)["fst"].tobytes()
    finally:
        for d in (d_lo, d_hi, d_fst):
            ctx.dev_free(d)
        v.free()
        X.free()
        ctx.close()
