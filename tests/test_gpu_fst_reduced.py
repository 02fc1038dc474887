"""GPU: the totals-only Fst kernels of csrc/fst.hip after their reduction (DESIGN.md 3 "Fst totals").

WC84: tpg_fst_wc84_tile_kernel<true> sums the reduced pair (per-population c = n p (1 - p), one table entry {alpha, r}) and
forms a locus again by the full pair's statements wherever some pair of the wave is singular (nt <= 2) or has an empty
population; panels with a group of fewer than three individuals get the full pair, tpg_fst_wc84_tile_kernel<false>.  The tile
kernels need more than 256 pairs, at most 64 populations and groups of at most 127 individuals.
Hudson: tpg_fst_hudson_gemm_kernel issues C C' and one column of sums per row population for every chunk of 16 loci, and the
masked products A B', C B' only for a chunk in which some population is masked, over the loci where one is; the final kernel
adds the two parts.

References, never the totals path itself: the oracle's totals, and the library's own BY-LOCUS route (statement for statement the
reference's, untouched by the reduction) summed on the host in float64 with a locus dropped where its numerator or denominator
is NaN, as the reduce drops it.  Tolerance: the contract of tests/test_gpu_parity.py::test_fst_vs_oracle for totals.

Loci: 37 (three chunks of 16, the last of 5: one chunk per workgroup) and 2 * 16 * 4 * (compute units) + 5 (the grid is 4
workgroups per compute unit: every workgroup takes a second chunk, the last one a short one)."""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-11, atol=1e-15, equal_nan=True)


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


@pytest.fixture(scope="module")
def m_long(tpg):
    # the compute units of the device the context runs on, from the HIP runtime the library has loaded (dlopen by soname)
    import ctypes as C

    hip, cus = C.CDLL("libamdhip64.so.7"), C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(cus), 63, 0) == 0 and cus.value > 0  # hipDeviceAttributeMultiprocessorCount
    return 2 * 16 * 4 * cus.value + 5


def _loci(which, m_long):
    return 37 if which == "short" else m_long


def _groups(sizes):
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)


def _uneven(G, lo, hi, seed):
    return _groups(np.random.default_rng(seed).integers(lo, hi + 1, G))


def _by_locus_totals(tpg, X, gid, G, method, pairs):
    """sums over the loci of the library's by-locus numerators and denominators, a block of pairs at a time"""
    P = pairs.shape[1]
    sn, sd = np.zeros(P), np.zeros(P)
    for k0 in range(0, P, 512):
        sub = np.ascontiguousarray(pairs[:, k0:k0 + 512])
        nd = tpg.pairwise_pop_fst(X, None, None, gid, G, method=method, return_num_dem=True, pairwise_combn=sub)
        num, den = nd["Fst_by_locus_num"], nd["Fst_by_locus_den"]
        keep = ~(np.isnan(num) | np.isnan(den))
        sn[k0:k0 + 512] = np.where(keep, num, 0.0).sum(axis=0)
        sd[k0:k0 + 512] = np.where(keep, den, 0.0).sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return sn / sd


def _check(tpg, fbm, gid, G, method, pairs=None):
    """the totals-only call against both references; returns (totals, oracle totals)"""
    X = tpg.FBM.from_numpy(fbm)
    with np.errstate(invalid="ignore", divide="ignore"):
        if pairs is None:
            o_tot = orc.pairwise_pop_fst(fbm, None, None, gid, G, method=method)["fst_tot"]
        else:
            pf = orc.grouped_summaries_dip_pseudo_cpp(fbm, None, None, gid, G, np.full(fbm.shape[0], 2.0))
            if method == "WC84":
                o_tot = orc.pairwise_fst_wc84_loop(pairs, pf["n"], pf["freq_alt"], pf["het_obs"])["fst_tot"]
            else:
                o_tot = orc.pairwise_fst_hudson_loop(pairs, pf["n"], pf["freq_alt"], pf["freq_ref"])["fst_tot"]
    allp = tpg.combn2(G) if pairs is None else pairs
    b_tot = _by_locus_totals(tpg, X, gid, G, method, allp)
    got = tpg.pairwise_pop_fst(X, None, None, gid, G, method=method, pairwise_combn=pairs)["fst_tot"]
    X.free()
    print(f"{method} G={G} m={fbm.shape[1]} P={allp.shape[1]}: largest |difference| / (atol + rtol |reference|) "
          f"{_frac(got, o_tot):.3g} (oracle) {_frac(got, b_tot):.3g} (by-locus sums), {int(np.isnan(o_tot).sum())} NaN totals")
    assert np.allclose(got, o_tot, **TOL)
    assert np.allclose(got, b_tot, **TOL)
    return got, o_tot


def _frac(a, b):
    """the largest difference as a fraction of what TOL allows (printed, not asserted)"""
    fin = np.isfinite(a) & np.isfinite(b)
    return float(np.max(np.abs(a[fin] - b[fin]) / (TOL["atol"] + TOL["rtol"] * np.abs(b[fin])))) if fin.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# WC84 totals, tile kernels


@pytest.mark.parametrize("which", ["short", "long"])
def test_wc84_reduced_uneven_groups(tpg, m_long, which):
    """24 populations (276 pairs, the fewest that take the tile kernel with whole populations) of 3 ... 12 individuals"""
    G = 24
    gid = _uneven(G, 3, 12, 5)
    fbm = orc.synth_fbm(101, len(gid), _loci(which, m_long), npop=G, miss=0.05)
    assert np.bincount(gid).min() == 3 and np.bincount(gid).max() == 12 and 130 <= len(gid) <= 200
    _check(tpg, fbm, gid, G, "WC84")


@pytest.mark.parametrize("which", ["short", "long"])
def test_wc84_reduced_51_populations(tpg, m_long, which):
    G, n = 51, 255
    fbm = orc.synth_fbm(102, n, _loci(which, m_long), npop=G, miss=0.05)
    _check(tpg, fbm, (np.arange(n) % G).astype(np.int32), G, "WC84")


SINGULAR_SEED, SINGULAR_M = 3, 533


def _singular_panel():
    """24 populations of 3 ... 5 individuals, 70 ... 90 % of the genotypes of a locus missing: at most loci some pair has
    nt <= 2 or an empty population"""
    G = 24
    gid = _uneven(G, 3, 5, SINGULAR_SEED)
    rng = np.random.default_rng(SINGULAR_SEED)
    fbm = orc.synth_fbm(200 + SINGULAR_SEED, len(gid), SINGULAR_M, npop=G, miss=0.0)
    miss = rng.uniform(0.7, 0.9, SINGULAR_M)
    fbm[rng.random(fbm.shape) < miss[None, :]] = 3
    return fbm, gid, G


def test_wc84_reduced_singular_loci(tpg):
    """The rare path: the wave forms the locus by the full pair's statements; what those give at nt <= 2 (NaN or +-inf)
    decides which loci the sums keep, so totals and their NaN pattern are the references'."""
    fbm, gid, G = _singular_panel()
    with np.errstate(invalid="ignore", divide="ignore"):
        o = orc.pairwise_pop_fst(fbm, None, None, gid, G, method="WC84", return_num_dem=True)
    num, den = np.asarray(o["Fst_by_locus_num"]), np.asarray(o["Fst_by_locus_den"])
    bad = ~(np.isfinite(num) & np.isfinite(den))
    assert bad.mean() >= 0.01
    got, o_tot = _check(tpg, fbm, gid, G, "WC84")
    assert np.isfinite(o_tot).sum() >= o_tot.size / 2
    assert np.array_equal(np.isnan(got), np.isnan(o_tot)) and np.array_equal(np.isinf(got), np.isinf(o_tot))


def test_wc84_reduced_partial_pair_list(tpg):
    """300 pairs of 40 populations in no order, a third of them as (g2, g1) with g2 > g1; tiles with one listed pair"""
    G, m = 40, 37
    gid = _uneven(G, 3, 8, 9)
    fbm = orc.synth_fbm(103, len(gid), m, npop=G, miss=0.05)
    rng = np.random.default_rng(9)
    allp = tpg.combn2(G)
    pairs = allp[:, rng.permutation(allp.shape[1])[:300]].copy()
    flip = rng.random(300) < 0.33
    pairs[:, flip] = pairs[::-1, flip]
    pairs = np.ascontiguousarray(pairs)
    assert (pairs[0] > pairs[1]).sum() > 50
    # the tiles of csrc/host/host_fsttiles.h: 3 first populations x 2 second populations
    tiles = {}
    for a, b in (pairs - 1).T:
        tiles[(a // 3, b // 2)] = tiles.get((a // 3, b // 2), 0) + 1
    assert min(tiles.values()) == 1
    _check(tpg, fbm, gid, G, "WC84", pairs=pairs)


def test_wc84_tiny_group_takes_full_pair(tpg):
    """A group of one and a group of two among 26 (325 pairs): every wave would be singular at every locus, the host
    launches the full pair's kernel."""
    G = 26
    gid = _groups([4] * 11 + [1] + [5] * 6 + [2] + [3] * 7)
    fbm = orc.synth_fbm(104, len(gid), 293, npop=G, miss=0.05)
    _check(tpg, fbm, gid, G, "WC84")


@pytest.mark.parametrize("method,G", [("WC84", 24), ("Hudson", 51), ("Hudson", 70)])
def test_totals_repeatable(tpg, method, G):
    """the partial sums are added in a fixed order: two calls, the same bits"""
    if method == "WC84":
        fbm, gid, G = _singular_panel()
    else:
        fbm, gid = _masked_panel(G, 1301)
    X = tpg.FBM.from_numpy(fbm)
    a = tpg.pairwise_pop_fst(X, None, None, gid, G, method=method, sums=True)
    b = tpg.pairwise_pop_fst(X, None, None, gid, G, method=method, sums=True)
    X.free()
    assert np.array_equal(a["sum_num"], b["sum_num"], equal_nan=True)
    assert np.array_equal(a["sum_den"], b["sum_den"], equal_nan=True)
    assert np.array_equal(a["fst_tot"], b["fst_tot"], equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------------
# Hudson totals


@pytest.mark.parametrize("which", ["short", "long"])
@pytest.mark.parametrize("G", [5, 51, 70])
def test_hudson_products(tpg, m_long, G, which):
    """5: one partial tile; 51: the benchmark's; 70: 2 x 2 tiles of 64 populations, the off-diagonal ones included"""
    n = 5 * G
    fbm = orc.synth_fbm(110 + G, n, _loci(which, m_long), npop=min(G, 51), miss=0.02)
    _check(tpg, fbm, (np.arange(n) % G).astype(np.int32), G, "Hudson")


def _masked_panel(G, m):
    """five individuals per population, 2 % missing; no population is empty in the first 64 loci (m > 64), about 10 % of the
    others have a population with no typed individual or one, and one population has none at EVERY locus of one chunk"""
    n = 5 * G
    fbm = orc.synth_fbm(120 + G, n, m, npop=min(G, 51), miss=0.02)
    gid = (np.arange(n) % G).astype(np.int32)
    rng = np.random.default_rng(G + m)
    first = 64 if m > 64 else 16
    for j in np.flatnonzero(rng.random(m) < 0.10):
        if j < first:
            continue
        rows = np.flatnonzero(gid == rng.integers(G))
        fbm[rows[rng.integers(2):], j] = 3  # none typed, or the first one only
    c0 = 16 if m <= 64 else 16 * 7
    fbm[np.ix_(np.flatnonzero(gid == G - 2), np.arange(c0, c0 + 16))] = 3
    with np.errstate(invalid="ignore", divide="ignore"):
        typed = orc.grouped_summaries_dip_pseudo_cpp(fbm, None, None, gid, G, np.full(n, 2.0))["n"]
    assert np.all(typed[:first] > 0) and np.any(typed[first:] == 0)
    return fbm, gid


@pytest.mark.parametrize("which", ["short", "long"])
@pytest.mark.parametrize("G", [51, 70])
def test_hudson_products_masked(tpg, m_long, G, which):
    """chunks with and without mask products in one launch"""
    fbm, gid = _masked_panel(G, _loci(which, m_long))
    _check(tpg, fbm, gid, G, "Hudson")


def test_hudson_loop_entry_with_nan_frequency(tpg):
    """pairwise_fst_hudson_loop on the caller's matrices (the generic staging of the same kernel): a NaN frequency masks its
    population at that locus"""
    n, m, G = 60, 37, 5
    fbm = orc.synth_fbm(130, n, m, npop=G, miss=0.05)
    gid = (np.arange(n) % G).astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        pf = orc.grouped_summaries_dip_pseudo_cpp(fbm, None, None, gid, G, np.full(n, 2.0))
    fa, fr = pf["freq_alt"].copy(), pf["freq_ref"].copy()
    for j, g in ((3, 1), (20, 4), (36, 0)):
        fa[j, g] = np.nan
        fr[j, g] = np.nan
    pairs = tpg.combn2(G)
    with np.errstate(invalid="ignore", divide="ignore"):
        o_tot = orc.pairwise_fst_hudson_loop(pairs, pf["n"], fa, fr)["fst_tot"]
    nd = tpg.pairwise_fst_hudson_loop(pairs, pf["n"], fa, fr, by_locus=True, return_num_dem=True)
    num, den = nd["Fst_by_locus_num"], nd["Fst_by_locus_den"]
    keep = ~(np.isnan(num) | np.isnan(den))
    assert (~keep).sum() >= 3 * (G - 1)
    b_tot = np.where(keep, num, 0.0).sum(axis=0) / np.where(keep, den, 0.0).sum(axis=0)
    got = tpg.pairwise_fst_hudson_loop(pairs, pf["n"], fa, fr)["fst_tot"]
    assert np.allclose(got, o_tot, **TOL)
    assert np.allclose(got, b_tot, **TOL)
