"""Host side of the fused window scan (include/tpg.h "windowed pairwise Fst"): the numpy restatement tests/winfst_ref.py tied
to the pinned oracle, the declarations in the header and the binding, the R shim's registration, and the scratch bound.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests import rmock
from tests import winfst_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = {"tpg_winfst_chunk_loci": 0, "tpg_windows_fst_scratch_bytes": 4, "tpg_windows_pairwise_pop_fst": 18}
# the reference's three window settings (tests/test_gpu_parity.py: test_windows_pairwise_pop_fst)
SETTINGS = (dict(window_size=3, step_size=2, size_unit="snp", min_loci=2),
            dict(window_size=40, step_size=40, size_unit="snp", min_loci=1, complete=True),
            dict(window_size=5000, step_size=2500, size_unit="bp", min_loci=2))


@pytest.mark.parametrize("n,m,G", [(10, 8, 3), (120, 700, 4)])
def test_float_route_reproduces_the_oracle(n, m, G):
    """windows_ref fed the oracle's by-locus Hudson numerators and denominators against the oracle's own
    windows_pairwise_pop_fst.  The oracle sums a window with numpy's sum, which adds up to 8 values one after the other: with
    windows of 3 loci both sides do the same operations and the match is bitwise.  Longer windows are summed in another order
    there; two sums of the same L doubles in any two orders differ by at most 2 L 2^-53 sum|x| (each is within L 2^-53 sum|x| of
    the exact sum), which moves the mean by that over n and the ratio of the two means by the relative sum of both, plus one
    ulp for the division itself (1.01: the second-order terms of that first-order bound)."""
    from tidypopgen_amd import api

    fbm = orc.synth_fbm(91, n, m, npop=G, miss=0.1)
    gid = (np.arange(n) % G).astype(np.int32)
    chrom = np.array(["chr1"] * (m // 3) + ["chr2"] * (m - m // 3))
    rng = np.random.default_rng(5)
    pos = np.concatenate([np.sort(rng.integers(1, 50 * m, m // 3)), np.sort(rng.integers(1, 50 * m, m - m // 3))])
    with np.errstate(invalid="ignore", divide="ignore"):
        nd = orc.pairwise_pop_fst(fbm, None, None, gid, G, method="Hudson", return_num_dem=True)
    num, den = nd["Fst_by_locus_num"], nd["Fst_by_locus_den"]
    bitwise = 0
    for kw in SETTINGS:
        with np.errstate(invalid="ignore", divide="ignore"):
            o = orc.windows_pairwise_pop_fst(fbm, None, None, gid, G, chrom, pos, **kw)
        r = api.window_index_ranges(chrom, pos, kw["window_size"], kw["step_size"], kw["size_unit"], kw.get("complete", False))
        assert np.array_equal(r["start"], o["start"]) and np.array_equal(r["end"], o["end"])
        got = wr.windows_ref(num, den, r["lo"], r["hi"], r["pad_na"], kw["min_loci"])
        assert got["fst"].shape == o["fst"].shape
        assert np.array_equal(np.isnan(got["fst"]), np.isnan(o["fst"]))
        L = (r["hi"] - r["lo"]).astype(np.float64)[:, None]
        if L.max() <= 8:
            assert got["fst"].tobytes() == o["fst"].tobytes()
            bitwise += 1
            continue
        f = np.isfinite(o["fst"])
        sn, sd = np.abs(got["mean_num"] * got["n_num"]), np.abs(got["mean_den"] * got["n_den"])
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = 2 * L * 2.0 ** -53 * (got["abs_num"] / sn + got["abs_den"] / sd) + 2.0 ** -52
        d = np.abs(got["fst"] - o["fst"])
        assert np.all(d[f] <= 1.01 * rel[f] * np.abs(o["fst"][f])), np.nanmax(d[f] / (rel[f] * np.abs(o["fst"][f])))
    assert bitwise >= 1  # the windows of 3 loci (on the small panel every window is that short)


def test_exact_routes_agree_and_bound_the_float_route():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(200, 3)) * 10.0 ** rng.integers(-8, 8, size=(200, 3))
    x[rng.random(x.shape) < 0.1] = np.nan
    lo, hi = np.array([0, 5, 70, 199, 50]), np.array([200, 6, 140, 200, 50])
    s, n, a = wr.window_sums(x, lo, hi)
    for w in range(len(lo)):
        for c in range(3):
            col = x[lo[w]:hi[w], c]
            ex, fr = wr.sum_exact(col), wr.sum_fraction(col)
            assert abs(fr - wr.Fraction(ex)) <= abs(fr) * wr.Fraction(1, 2 ** 53)
            assert n[w, c] == np.sum(~np.isnan(col))
            assert abs(s[w, c] - ex) <= n[w, c] * 2.0 ** -52 * a[w, c]
    assert wr.sum_exact([np.inf, 1.0, np.nan]) == np.inf and np.isnan(wr.sum_exact([np.inf, -np.inf]))
    p = wr.pbs_one_triplet(np.array([0.2]), np.array([0.3]), np.array([0.1]))
    t12, t13, t23 = -np.log(0.8), -np.log(0.7), -np.log(0.9)
    assert p[0][0] == (t12 + t13 - t23) / 2 and p[3][0] == p[0][0] / (1 + p[0][0] + p[1][0] + p[2][0])


def test_header_and_binding_declare_the_functions():
    from tidypopgen_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "tpg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for f, arity in FUNCTIONS.items():
        mt = re.search(r"\b(?:int|int64_t) " + f + r"\s*\(([^)]*)\)\s*;", code)
        assert mt, f
        params = [p for p in mt.group(1).split(",") if p.strip() != "void"]
        assert len(params) == arity, (f, params)
        assert f in _lib.SYMBOLS and hasattr(_lib.lib, f) and len(getattr(_lib.lib, f).argtypes) == arity
    assert _lib.lib.tpg_winfst_chunk_loci.restype is C.c_int64 and _lib.lib.tpg_windows_fst_scratch_bytes.restype is C.c_int64
    assert "windowed pairwise Fst" in hdr
    import tidypopgen_amd as tpg

    for f in ("windows_fst", "windows_nwise_pop_pbs", "windows_pairwise_pop_fst"):
        assert callable(getattr(tpg, f))
    import inspect

    assert inspect.signature(tpg.windows_pairwise_pop_fst).parameters["route"].default == "staged"


def _table(lib, symbol):
    """a NULL-terminated registration table of the shim, whatever its length: {name: (function pointer, arity)}"""
    row = C.cast(C.addressof(rmock.Entry.in_dll(lib, symbol)), C.POINTER(rmock.Entry))
    out, k = {}, 0
    while row[k].name:
        out[row[k].name.decode()] = (row[k].fun, row[k].numArgs)
        k += 1
    return out


def test_shim_registers_the_two_entries_once(tmp_path):
    lib = rmock.build(tmp_path)  # links against libtpg_hip.so; loading it needs no GPU
    got = _table(lib, "tpg_rshim_entries_winfst")
    assert {k: v[1] for k, v in got.items()} == {"_tidypopgen_tpg_windows_pairwise_pop_fst": 10,
                                                  "_tidypopgen_tpg_windows_nwise_pop_pbs": 10}
    for name, (fun, _) in got.items():
        assert fun == C.cast(getattr(lib, name), C.c_void_p).value
    src = open(os.path.join(ROOT, "shim", "tpg_rshim.c")).read()
    tables = set(re.findall(r"const R_CallMethodDef (tpg_rshim_entries\w*)\[\]", src)) - {"tpg_rshim_entries_winfst"}
    assert {"tpg_rshim_entries", "tpg_rshim_entries_tajima"} <= tables
    for tab in tables:  # no name shared with any other table
        assert not set(got) & set(_table(lib, tab)), tab
    # merged into the package's one .Call table, and wrapped and exported on the R side
    init = src[src.index("void R_init_tpgshim"):]
    assert init.count("tpg_rshim_entries_winfst") == 3  # its size (twice in the sizeof quotient) and its rows
    ns = open(os.path.join(ROOT, "shim", "tpgshim", "NAMESPACE")).read()
    rsrc = open(os.path.join(ROOT, "shim", "tpgshim", "R", "tpgshim.R")).read()
    for fn in ("tpg_windows_pairwise_pop_fst", "tpg_windows_nwise_pop_pbs"):
        assert f"export({fn})" in ns and re.search(rf"^{fn} <- function", rsrc, re.M) and f"`_tidypopgen_{fn}`" in rsrc


def test_scratch_bound():
    from tidypopgen_amd import _lib, api

    c = _lib.lib.tpg_winfst_chunk_loci()
    assert c >= 32 and c & (c - 1) == 0 and api.WINFST_CHUNK_LOCI == c
    sb = _lib.lib.tpg_windows_fst_scratch_bytes
    assert 0 < sb(10 ** 6, 51, 1275, 10 ** 4) <= 10 ** 6 * 1275 + (64 << 20)
    prev = -1
    for m in (0, 1, c - 1, c, c + 1, 2 * c + 3, 300, 10 ** 4, 10 ** 6, 10 ** 6 + 1, 1 << 33):
        b = sb(m, 51, 1275, 100)
        assert b >= prev and b <= m * 1275 + (64 << 20)
        prev = b
    assert sb(10 ** 6, 51, 1275, 1) == sb(10 ** 6, 51, 1275, 10 ** 6)  # the part that grows with m does not depend on nw
    assert sb(-1, 51, 1275, 1) < 0 and sb(10, 51, 0, 1) < 0
    assert api.windows_fst_scratch_bytes(300, 9, 36, 5) == sb(300, 9, 36, 5)
