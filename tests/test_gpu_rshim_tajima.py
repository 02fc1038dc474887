"""GPU: the R entry points of Tajima's D, `.Call("_tidypopgen_tpg_pop_tajimas_d", BM, rowInd, colInd, groupIds, ngroups)` and
`.Call("_tidypopgen_tpg_windows_pop_tajimas_d", BM, rowInd, colInd, groupIds, ngroups, lo, hi, pad_na, min_loci)` of
shim/tpg_rshim.c (tpg_rshim_entries_tajima[]), through the strict R mock: equal to the Python route bit for bit, NA_real_ /
NA_integer_ where the reference assigns NA and a plain NaN where the arithmetic gives one, protect stack balanced, backing
file untouched."""
import numpy as np
import pytest

from tests import rmock
from tests import tajima_ref as tr

pytestmark = pytest.mark.gpu

CODE_012 = np.r_[0.0, 1.0, 2.0, np.full(253, np.nan)]


def _tajima_entries(lib):
    tab = (rmock.Entry * 4).in_dll(lib, "tpg_rshim_entries_tajima")
    out = {}
    for e in tab:
        if not e.name:
            break
        out[e.name.decode()] = (e.fun, e.numArgs)
    return out


@pytest.fixture(scope="module")
def r(tmp_path_factory):
    lib = rmock.build(tmp_path_factory.mktemp("rshim_tajima"))
    lib.rmock_gctorture(1)
    lib.rmock_strict(1)
    s = rmock.Session(lib)
    s.ent = {**s.ent, **_tajima_entries(lib)}
    yield s
    lib.rmock_gctorture(0)
    lib.rmock_strict(0)
    lib.R_unload_tpgshim(None)
    lib.rmock_reset()


def test_table_rows_and_arities(r):
    ent = _tajima_entries(r.lib)
    assert {k: v[1] for k, v in ent.items()} == {"_tidypopgen_tpg_pop_tajimas_d": 5, "_tidypopgen_tpg_windows_pop_tajimas_d": 9}
    assert not set(ent) & set(rmock.entries(r.lib))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n,m,G", [(13, 300, 3), (65, 1100, 33), (20, 90, 1)])
def test_entries_equal_the_python_route(r, tmp_path, n, m, G):
    import tidypopgen_amd as tpg

    codes, gid = tr.panel(40 + n, n + 2, m + 4, G)
    path = tmp_path / "geno.bk"
    path.write_bytes(codes.tobytes(order="F"))
    BM = r.fbm(path, n + 2, m + 4, CODE_012)
    rows, cols = np.arange(2, n + 2), np.arange(3, m + 3)  # 1-based subsets
    g_sub = None if gid is None else gid[rows - 1]
    X = tpg.FBM.from_numpy(np.asfortranarray(codes), code256=tpg.CODE_012)
    depth = r.depth()
    gid_sexp = r.lib.rmock_nil() if g_sub is None else r.index(g_sub, double=True)  # .group_ids(x) - 1 is a double vector

    # whole view
    out = r.call("tpg_pop_tajimas_d", BM, r.int(rows), r.index(cols, double=True), gid_sexp, r.int([G]))
    assert r.lib.TYPEOF(out) == 14 and r.lib.XLENGTH(out) == G
    py = np.atleast_1d(tpg.pop_tajimas_d(X, rows, cols, g_sub, G))
    assert np.array_equal(_bits(r.as_numpy(out)), _bits(py))

    # windows: 7 SNPs step 2 with pad windows at the end, and 64 SNPs step 1
    wa = tpg.window_index_ranges(np.ones(m), None, 7, 2, complete=True)
    wb = tpg.window_index_ranges(np.ones(m), None, 64, 1)
    lo, hi = np.r_[wa["lo"], wb["lo"], m], np.r_[wa["hi"], wb["hi"], m]
    pad = np.r_[wa["pad_na"], wb["pad_na"], 0].astype(np.int32)
    nw = len(lo)
    v = tpg.View(X, rows, cols)
    for min_loci in (1, 3):
        want = tpg.tajima_windows(v, g_sub, G, lo, hi, pad, min_loci)
        na = (want["n_loci"] < 0) | (want["n_loci"] < min_loci)
        for as_double in (True, False):  # lo / hi as R holds them: double or integer
            lo_s, hi_s = (r.real(lo), r.real(hi)) if as_double else (r.int(lo), r.int(hi))
            out = r.call("tpg_windows_pop_tajimas_d", BM, r.int(rows), r.int(cols), gid_sexp, r.real([float(G)]), lo_s, hi_s,
                         r.int(pad), r.int([min_loci]))
            assert r.lib.TYPEOF(out) == 19 and r.names(out) == ["stat", "n_loci"]
            s_sexp, n_sexp = r.lib.VECTOR_ELT(out, 0), r.lib.VECTOR_ELT(out, 1)
            assert r.lib.TYPEOF(s_sexp) == 14 and r.lib.TYPEOF(n_sexp) == 13 and r.dim(s_sexp) == (nw, G) == r.dim(n_sexp)
            stat, nl = r.as_numpy(s_sexp, (nw, G)), r.as_numpy(n_sexp, (nw, G))
            # NA_real_ exactly where the reference assigns NA; elsewhere the device's bits, a plain NaN included
            assert np.array_equal(rmock.is_na(stat.ravel()).reshape(nw, G), na)
            assert np.array_equal(_bits(stat[~na]), _bits(want["tajimas_d"][~na]))
            assert np.array_equal(nl == -2147483648, want["n_loci"] < 0) and np.array_equal(nl[nl != -2147483648], want["n_loci"][want["n_loci"] >= 0])
        assert (want["n_loci"] < 0).any() and na.any()
        assert np.isnan(want["tajimas_d"][~na]).any() and np.isfinite(want["tajimas_d"][~na]).any()
    # pad_na = NULL: no window is padded
    out = r.call("tpg_windows_pop_tajimas_d", BM, r.int(rows), r.int(cols), gid_sexp, r.int([G]), r.real(lo), r.real(hi),
                 r.lib.rmock_nil(), r.int([1]))
    want = tpg.tajima_windows(v, g_sub, G, lo, hi, None, 1)
    assert np.array_equal(r.list_elt(out, 1, (nw, G)), want["n_loci"])
    assert r.depth() == depth
    assert np.array_equal(np.frombuffer(path.read_bytes(), dtype=np.uint8), codes.ravel(order="F"))


def test_bad_arguments_are_r_errors(r, tmp_path):
    n, m, G = 13, 60, 3
    codes, gid = tr.panel(9, n, m, G)
    path = tmp_path / "g.bk"
    path.write_bytes(codes.tobytes(order="F"))
    BM = r.fbm(path, n, m, CODE_012)
    rows, cols = r.int(np.arange(1, n + 1)), r.int(np.arange(1, m + 1))
    g, ng, one = r.int(gid), r.int([G]), r.int([1])
    lo, hi = r.real([0.0, 3.0]), r.real([3.0, 6.0])
    nil = r.lib.rmock_nil()
    depth = r.depth()
    with pytest.raises(RuntimeError, match="differ in length"):
        r.call("tpg_pop_tajimas_d", BM, rows, cols, r.int(gid[:-1]), ng)
    with pytest.raises(RuntimeError, match="ngroups must be 1"):
        r.call("tpg_pop_tajimas_d", BM, rows, cols, nil, ng)
    with pytest.raises(RuntimeError, match="positive integer"):
        r.call("tpg_pop_tajimas_d", BM, rows, cols, g, r.int([0]))
    with pytest.raises(RuntimeError, match="out of"):
        r.call("tpg_pop_tajimas_d", BM, rows, cols, r.int(np.r_[gid[:-1], G]), ng)
    with pytest.raises(RuntimeError, match="min_loci must be positive"):
        r.call("tpg_windows_pop_tajimas_d", BM, rows, cols, g, ng, lo, hi, nil, r.int([0]))
    with pytest.raises(RuntimeError, match="differ in length"):
        r.call("tpg_windows_pop_tajimas_d", BM, rows, cols, g, ng, lo, r.real([3.0]), nil, one)
    with pytest.raises(RuntimeError, match="differ in length"):
        r.call("tpg_windows_pop_tajimas_d", BM, rows, cols, g, ng, lo, hi, r.int([0]), one)
    for bad_lo, bad_hi in (([4.0, 0.0], [3.0, 2.0]), ([0.0, 0.0], [m + 1.0, 3.0]), ([-1.0, 0.0], [3.0, 3.0]),
                           ([0.5, 0.0], [3.0, 3.0]), ([rmock.na_real(), 0.0], [3.0, 3.0])):
        with pytest.raises(RuntimeError, match="window 1 is NA, not whole numbers or outside"):
            r.call("tpg_windows_pop_tajimas_d", BM, rows, cols, g, ng, r.real(bad_lo), r.real(bad_hi), nil, one)
    with pytest.raises(RuntimeError, match="must be integer or double"):
        r.call("tpg_windows_pop_tajimas_d", BM, rows, cols, g, ng, r.lib.rmock_str(b"a"), hi, nil, one)
    assert r.depth() == depth
