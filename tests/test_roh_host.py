"""Host side of runs of homozygosity: the numpy restatement tests/roh_ref.py against itself (loop = cumulative sums), the
conditions that keep the filter tests from being vacuous on the committed seeds, the reference's own toy, the R shim's
registration and the argument checks of the Python layer.  No GPU."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from tests import rmock
from tests import roh_ref as rr

TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roh_toy")
TOY_PARAMS = dict(window_size=4, min_snp=2, min_density=1 / 500, max_gap=5000, min_length_bps=1000, threshold=0.05)


def _panel(seed, n, m, W):
    return (rr.roh_panel(seed, n, m, W),) + rr.roh_loci(seed, m, W=W)


@pytest.mark.parametrize("seed,n,m,W", rr.FILTER_PANELS)
def test_loop_equals_cumulative_sums(seed, n, m, W):
    G, chrom, pos = _panel(seed, n, m, W)
    if n * m > 100000:  # the literal loop on a slice of the individuals
        G = G[:6]
    for kw in ({}, rr.UNFILTERED, dict(rr.UNFILTERED, heterozygosity=True, max_opp_window=(2 * W) // 3)):
        p = rr.params(window_size=W, **kw)
        a, b = rr.status_loop(G, chrom, pos, p), rr.status_vec(G, chrom, pos, p)
        assert np.array_equal(a, b)
        assert rr.same_runs(rr.runs_loop(G, a, chrom, pos, p), rr.runs_vec(G, b, chrom, pos, p))


@pytest.mark.parametrize("seed,n,m,W", rr.FILTER_PANELS)
def test_every_filter_bites_on_the_committed_seeds(seed, n, m, W):
    """Every filter of the list changes the set of runs.  One case cannot: at W = 2, threshold 0.5 gives the same need table
    as 0.05 (max(1, ceil(threshold c)) = 1 for c = 1, 2), whatever the panel, so there the runs are asserted equal."""
    G, chrom, pos = _panel(seed, n, m, W)
    base = rr.roh_vec(G, chrom, pos, window_size=W, **rr.UNFILTERED)
    assert len(base["indiv"]) > 0
    for name, over, must_leave_runs in rr.FILTERS:
        p = dict(rr.UNFILTERED, window_size=W, **over)
        r = rr.roh_vec(G, chrom, pos, **p)
        if "threshold" in over and np.array_equal(rr.need_table(W, over["threshold"]), rr.need_table(W, 0.05)):
            # W = 2: need = [1, 1] at 0.05 and at 0.5 alike (max(1, ceil(threshold c)) for c = 1, 2), so the runs cannot differ
            assert rr.same_runs(r, base), name
        else:
            assert rr.run_set(r) != rr.run_set(base), name
        if must_leave_runs:
            assert len(r["indiv"]) > 0, name
    het = rr.roh_vec(G, chrom, pos, window_size=W, heterozygosity=True, max_opp_window=(2 * W) // 3, **rr.UNFILTERED)
    assert len(het["indiv"]) > 0 and rr.run_set(het) != rr.run_set(base)


@pytest.mark.parametrize("W", [128, 512])
def test_wide_windows_have_runs(W):
    G, chrom, pos = _panel(6, 33, 4097, W)
    assert len(rr.roh_vec(G, chrom, pos, window_size=W)["indiv"]) > 0


def _toy():
    G = np.loadtxt(os.path.join(TOY, "genotypes.txt"), dtype=np.int64).astype(np.uint8)
    loci = np.loadtxt(os.path.join(TOY, "loci.txt"), dtype=np.int64)
    want = np.loadtxt(os.path.join(TOY, "expected_runs.txt"), dtype=np.int64).reshape(-1, 5)
    return G, loci[:, 0].astype(np.int32), loci[:, 1], want


def _rows(r):
    return np.stack([np.asarray(r[k], dtype=np.int64) for k in ("indiv", "first", "last", "n_opp", "n_miss")], axis=1)


def test_the_reference_toy_and_its_two_invariances():
    G, chrom, pos, want = _toy()
    for f in (rr.roh_loop, rr.roh_vec):
        full = _rows(f(G, chrom, pos, **TOY_PARAMS))
        assert np.array_equal(full, want)  # a: no run; b: loci 0..3 with one heterozygote; c: loci 0..3 with none
        assert np.array_equal(_rows(f(G[:, :6], chrom[:6], pos[:6], **TOY_PARAMS)), want)  # the last locus dropped
        sub = _rows(f(G[[1, 2]], chrom, pos, **TOY_PARAMS))  # a subset of the individuals: the rows of the full result
        sub[:, 0] = np.array([1, 2])[sub[:, 0]]
        assert np.array_equal(sub, full[np.isin(full[:, 0], [1, 2])])


def test_shim_registers_the_roh_entry_once_with_arity_6(tmp_path):
    for extra in ((), ("-DTPG_RSHIM_STANDALONE",)):
        r = rmock.compile_only(extra)
        assert r.returncode == 0, r.stderr[-4000:]
    lib = rmock.build(tmp_path)  # links against libtpg_hip.so; loading it needs no GPU
    tab = (rmock.Entry * 4).in_dll(lib, "tpg_rshim_entries_roh")
    got = {}
    for e in tab:
        if not e.name:
            break
        got[e.name.decode()] = (e.fun, e.numArgs)
    assert {k: v[1] for k, v in got.items()} == {"_tidypopgen_tpg_indiv_roh": 6}
    assert got["_tidypopgen_tpg_indiv_roh"][0] == C.cast(lib._tidypopgen_tpg_indiv_roh, C.c_void_p).value
    main = rmock.entries(lib)
    assert not set(got) & set(main) and len(main) == 21  # the main table is as it was


def test_python_layer_refuses_unordered_positions_and_bad_windows():
    from tidypopgen_amd import api

    X = types.SimpleNamespace(ncol=5)  # (refused before the store is touched)
    chrom, pos = np.array([1, 1, 1, 2, 2]), np.array([10, 30, 20, 5, 6])
    with pytest.raises(ValueError, match="not ordered"):
        api.windows_indiv_roh(X, chromosome=chrom, position=pos)
    for W in (0, 513, -3):
        with pytest.raises(ValueError, match="window_size"):
            api.windows_indiv_roh(X, chromosome=chrom, position=np.sort(pos), window_size=W)
    assert api.ROH_CHUNK_LOCI > 0 and api.ROH_CHUNK_LOCI % 128 == 0
