"""Host side of LD clumping: the numpy restatement tests/ld_ref.py against itself (greedy = fixed point = parallel rounds), its
link decision against np.corrcoef, the window construction against a double loop, and the R shim's registration.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import ld_ref as lr
from tests import rmock

# (seed, n, m, rho, window in loci), thr_r2 = 0.2: panels with both links and survivors.  The seeds are chosen so that no
# pair of neighbours has an r^2 within 1e-9 of the threshold (test_link_decision_...: a condition on the inputs).  With 64
# individuals the sums are small integers and exact ties are common: seeds 1 and 3 of the last shape hold a pair with
# 5 num^2 = d_j d_k, r^2 = 1/5 exactly, which the definition (0.2 as a double lies above 1/5) does not link and a rounded
# np.corrcoef does.
PANELS = [(1, 200, 3000, 0.9, 50), (1, 500, 4000, 0.97, 200), (2, 64, 2000, 0.8, 30)]
THR = 0.2


def _setup(seed, n, m, rho, win):
    G = lr.ld_panel(seed, n, m, rho)
    hi = lr.window_hi(np.zeros(m, dtype=np.int64), None, win, use_positions=False)
    return G, hi


@pytest.mark.parametrize("seed,n,m,rho,win", PANELS)
def test_greedy_is_the_fixed_point_and_the_parallel_rounds_reach_it(seed, n, m, rho, win):
    G, hi = _setup(seed, n, m, rho, win)
    bits = lr.band_bits(G, hi, THR)
    adj = lr.bits_to_adjacency(bits)
    links = sum(len(a) for a in adj) // 2
    rng = np.random.default_rng(seed)
    ex = rng.random(m) < 0.1
    for key, exclude in ((lr.priority_key(G), None), (rng.integers(0, 5, m).astype(np.float64), None), (lr.priority_key(G), ex)):
        keep = lr.greedy(adj, key, exclude)
        assert lr.fixed_point_holds(adj, key, keep, exclude)
        par, rounds, left = lr.parallel_rounds(adj, key, exclude)
        assert left == 0 and np.array_equal(par, keep)
        assert rounds >= 1
        if exclude is not None:
            assert not keep[exclude].any()
        # the panels exercise both links and survivors
        assert 0 < keep.sum() < m and 0 < links < int((hi - np.arange(m)).sum())
    # flipping one kept locus breaks the characterisation: it is a test of something
    key = lr.priority_key(G)
    keep = lr.greedy(adj, key)
    keep[np.flatnonzero(keep)[0]] = False
    assert not lr.fixed_point_holds(adj, key, keep)


@pytest.mark.parametrize("seed,n,m,rho,win", PANELS)
def test_link_decision_is_r2_above_the_threshold(seed, n, m, rho, win):
    G, hi = _setup(seed, n, m, rho, win)
    x = G.astype(np.float64)
    got = lr.link_rows(G, hi, THR)  # every row: every pair of neighbours
    closest, pairs = np.inf, 0
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(m):
            if hi[j] == j:
                assert len(got[j]) == 0
                continue
            r2 = np.corrcoef(x[:, j:hi[j] + 1], rowvar=False)[0, 1:] ** 2  # NaN at a monomorphic locus: linked to nothing
            assert r2.shape == got[j].shape
            pairs += len(r2)
            if not np.isnan(r2).all():
                closest = min(closest, float(np.nanmin(np.abs(r2 - THR))))
            assert np.array_equal(got[j], r2 > THR), j
    assert pairs == int((hi - np.arange(m)).sum())
    # a condition on the inputs, not a tolerance: no pair of the committed seeds lies within 1e-9 of the threshold
    assert closest > 1e-9


def test_window_from_positions_against_a_double_loop():
    rng = np.random.default_rng(3)
    m = 700
    chrom = np.sort(rng.integers(1, 5, m))
    pos = np.empty(m)
    for c in np.unique(chrom):
        k = int((chrom == c).sum())
        pos[chrom == c] = np.sort(rng.integers(1, 3_000_000, k))
    pos[10] = pos[11]  # equal positions are neighbours
    for size in (0.0, 1.5, 40.0, 1e6):
        hi = lr.window_hi(chrom, pos, size, use_positions=True)
        hi_idx = lr.window_hi(chrom, None, size, use_positions=False)
        for j in range(m):
            want = want_idx = j
            for k in range(j + 1, m):
                if chrom[k] == chrom[j] and abs(pos[k] - pos[j]) <= size * 1000:
                    want = k
                if chrom[k] == chrom[j] and k - j <= size:
                    want_idx = k
            assert hi[j] == want and hi_idx[j] == want_idx, (size, j)
        assert np.all(np.diff(hi) >= 0) and np.all(hi >= np.arange(m))


def test_api_window_is_the_reference_window_and_refuses_unordered_loci():
    import tidypopgen_amd.api as api  # needs the built library to import, no device

    rng = np.random.default_rng(4)
    m = 400
    chrom = np.sort(rng.integers(1, 4, m))
    pos = np.concatenate([np.sort(rng.integers(1, 2_000_000, int((chrom == c).sum()))) for c in np.unique(chrom)])
    for size in (0.0, 25.0, 500.0):
        assert np.array_equal(api.ld_window_hi(chrom, pos, size, True), lr.window_hi(chrom, pos, size, True))
        assert np.array_equal(api.ld_window_hi(chrom, None, size, False), lr.window_hi(chrom, None, size, False))
    assert np.array_equal(api.ld_window_hi(None, None, 7, False, m=20), np.minimum(np.arange(20) + 7, 19))
    with pytest.raises(ValueError, match="not ordered"):
        api.ld_window_hi(chrom, pos[::-1].copy(), 10.0, True)
    with pytest.raises(ValueError, match="not ordered"):
        api.ld_window_hi(np.array([1, 1, 2, 2, 1]), None, 3, False)


def test_shim_registers_the_ld_entry_once_with_arity_7(tmp_path):
    for extra in ((), ("-DTPG_RSHIM_STANDALONE",)):
        r = rmock.compile_only(extra)
        assert r.returncode == 0, r.stderr[-4000:]
    lib = rmock.build(tmp_path)  # links against libtpg_hip.so; loading it needs no GPU
    tab = (rmock.Entry * 4).in_dll(lib, "tpg_rshim_entries_ld")
    got = {}
    for e in tab:
        if not e.name:
            break
        got[e.name.decode()] = (e.fun, e.numArgs)
    assert {k: v[1] for k, v in got.items()} == {"_tidypopgen_tpg_ld_clump": 7}
    assert got["_tidypopgen_tpg_ld_clump"][0] == C.cast(lib._tidypopgen_tpg_ld_clump, C.c_void_p).value
    main = rmock.entries(lib)
    assert not set(got) & set(main) and len(main) == 21  # the main table is as it was: 14 reference rows + 7 additions
