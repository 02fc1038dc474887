"""GPU: the R entry point of the f2 blocks, `.Call("_tidypopgen_tpg_f2_blocks", BM, rowInd, colInd, groupIds, ngroups, ploidy, lo,
hi, params)` of shim/tpg_rshim.c (tpg_rshim_entries_f2[]), through the strict R mock: against the exact route of
tests/f2_ref.py in every cell and equal to the Python route bit for bit, the arrays G x G x nb with their dim attribute, protect
stack balanced, backing file untouched."""
import numpy as np
import pytest

from tests import f2_ref as fr
from tests import rmock

pytestmark = pytest.mark.gpu

CODE_012 = np.r_[0.0, 1.0, 2.0, np.full(253, np.nan)]
NAMES = ["f2", "counts", "ap", "ap_counts", "block_lengths"]


def _f2_entries(lib):
    tab = (rmock.Entry * 2).in_dll(lib, "tpg_rshim_entries_f2")
    return {e.name.decode(): (e.fun, e.numArgs) for e in tab if e.name}


@pytest.fixture(scope="module")
def r(tmp_path_factory):
    lib = rmock.build(tmp_path_factory.mktemp("rshim_f2"))
    lib.rmock_gctorture(1)
    lib.rmock_strict(1)
    s = rmock.Session(lib)
    s.ent = {**s.ent, **_f2_entries(lib)}
    yield s
    lib.rmock_gctorture(0)
    lib.rmock_strict(0)
    lib.R_unload_tpgshim(None)
    lib.rmock_reset()


def test_table_row_and_arity(r):
    ent = _f2_entries(r.lib)
    assert {k: v[1] for k, v in ent.items()} == {"_tidypopgen_tpg_f2_blocks": 9}
    assert not set(ent) & set(rmock.entries(r.lib))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _params(pr, m):
    six = [pr["maxmiss"], pr["minmaf"], pr["maxmaf"], float(pr["minac2"]), float(pr["poly_only"]), float(pr["apply_corr"])]
    return np.r_[six, np.asarray(pr["keep"], dtype=np.float64)] if pr["keep"] is not None else np.asarray(six)


@pytest.mark.parametrize("n,m,G", [(13, 300, 3), (65, 700, 17), (40, 200, 65), (20, 90, 1)])
def test_entry_equals_the_exact_route_and_the_python_route(r, tmp_path, n, m, G):
    import tidypopgen_amd as tpg

    codes, gid, pl, planted = fr.panel(60 + n, n + 2, m + 4, G)
    path = tmp_path / "geno.bk"
    path.write_bytes(codes.tobytes(order="F"))
    BM = r.fbm(path, n + 2, m + 4, CODE_012)
    rows, cols = np.arange(2, n + 2), np.arange(3, m + 3)  # 1-based subsets
    g_sub = None if gid is None else gid[rows - 1]
    p_sub = None if pl is None else pl[rows - 1]
    sub = codes[np.ix_(rows - 1, cols - 1)]
    alt2, c = fr.group_tables(sub, g_sub, G, p_sub)
    K = tpg.F2_CHUNK_LOCI
    lo = np.array([0, 0, 5, 20, 40, 30, m], dtype=np.int64)
    hi = np.array([m, 0, 6, 20 + K + 1, 40 + 2 * K + 1, 60, m], dtype=np.int64)
    nb = len(lo)
    X = tpg.FBM.from_numpy(np.asfortranarray(codes), code256=tpg.CODE_012)
    v = tpg.View(X, rows, cols)
    depth = r.depth()
    nil = r.lib.rmock_nil()
    gid_sexp = nil if g_sub is None else r.index(g_sub, double=True)  # .group_ids(x) - 1 is a double vector
    keep = (np.arange(m) % 5 != 2)
    for pr in (fr.params(maxmiss=1.0), fr.params(maxmiss=1.0, poly_only=3, apply_corr=0, keep=keep), fr.params(maxmiss=0.41, minmaf=0.06)):
        ex = fr.blocks_exact(alt2, c, lo, hi, pr)
        py = tpg.f2_blocks(v, g_sub, G, lo, hi, ploidy=p_sub, maxmiss=pr["maxmiss"], minmaf=pr["minmaf"], maxmaf=pr["maxmaf"],
                           minac2=pr["minac2"], poly_only=pr["poly_only"], apply_corr=pr["apply_corr"], keep=pr["keep"])
        for as_double in (True, False):  # lo / hi as R holds them: double or integer
            lo_s, hi_s = (r.real(lo), r.real(hi)) if as_double else (r.int(lo), r.int(hi))
            out = r.call("tpg_f2_blocks", BM, r.int(rows), r.index(cols, double=True), gid_sexp, r.real([float(G)]),
                         nil if p_sub is None else r.real(p_sub), lo_s, hi_s, r.real(_params(pr, m)))
            assert r.lib.TYPEOF(out) == 19 and r.names(out) == NAMES
            got = {}
            for k, name in enumerate(NAMES[:4]):
                e = r.lib.VECTOR_ELT(out, k)
                assert r.lib.TYPEOF(e) == (14 if k % 2 == 0 else 13) and r.dim(e) == (G, G, nb), name
                got[name] = r.as_numpy(e, (G, G, nb))
            bl = r.lib.VECTOR_ELT(out, 4)
            assert r.lib.TYPEOF(bl) == 14 and r.lib.XLENGTH(bl) == nb
            got["block_lengths"] = r.as_numpy(bl)
            assert np.array_equal(got["counts"], ex["cnt"]) and np.array_equal(got["ap_counts"], ex["ap_cnt"])
            assert np.array_equal(got["block_lengths"], ex["n_kept"].astype(np.float64))
            assert fr.max_excess(got["f2"], ex["f2"], lo, hi) <= 1.0 and fr.max_excess(got["ap"], ex["ap"], lo, hi) <= 1.0
            assert not rmock.is_na(got["f2"].ravel()).any()  # a pair without a locus is NaN, not NA_real_
            for name in NAMES[:4]:
                assert np.array_equal(_bits(got[name]), _bits(py[name])), name
        # not vacuous: NaN cells and values (one group has no polymorphic locus, so f2 is NaN throughout there: ap has the values)
        assert np.isnan(py["f2"]).any() and np.isfinite(py["f2"] if G > 1 else py["ap"]).any() == (G > 1 or not pr["poly_only"] & 2)
    assert r.depth() == depth
    assert np.array_equal(np.frombuffer(path.read_bytes(), dtype=np.uint8), codes.ravel(order="F"))


def test_bad_arguments_are_r_errors(r, tmp_path):
    n, m, G = 13, 60, 3
    codes, gid, pl, _ = fr.panel(9, n, m, G)
    path = tmp_path / "g.bk"
    path.write_bytes(codes.tobytes(order="F"))
    BM = r.fbm(path, n, m, CODE_012)
    rows, cols = r.int(np.arange(1, n + 1)), r.int(np.arange(1, m + 1))
    g, ng = r.int(gid), r.int([G])
    lo, hi = r.real([0.0, 3.0]), r.real([3.0, 6.0])
    nil = r.lib.rmock_nil()
    ok = r.real([1.0, 0.0, 0.5, 0.0, 1.0, 1.0])
    depth = r.depth()

    def call(*a):
        return r.call("tpg_f2_blocks", BM, rows, cols, *a)

    with pytest.raises(RuntimeError, match="differ in length"):
        call(r.int(gid[:-1]), ng, nil, lo, hi, ok)
    with pytest.raises(RuntimeError, match="ngroups must be 1"):
        call(nil, ng, nil, lo, hi, ok)
    with pytest.raises(RuntimeError, match="positive integer"):
        call(g, r.int([0]), nil, lo, hi, ok)
    with pytest.raises(RuntimeError, match="out of"):
        call(r.int(np.r_[gid[:-1], G]), ng, nil, lo, hi, ok)
    with pytest.raises(RuntimeError, match="ploidy and rowInd differ"):
        call(g, ng, r.real(np.full(n - 1, 2.0)), lo, hi, ok)
    with pytest.raises(RuntimeError, match="differ in length"):
        call(g, ng, nil, lo, r.real([3.0]), ok)
    with pytest.raises(RuntimeError, match="6 numbers"):
        call(g, ng, nil, lo, hi, r.real([1.0, 0.0, 0.5]))
    with pytest.raises(RuntimeError, match="minac2"):
        call(g, ng, nil, lo, hi, r.real([1.0, 0.0, 0.5, 2.0, 1.0, 1.0]))
    with pytest.raises(RuntimeError, match="poly_only"):
        call(g, ng, nil, lo, hi, r.real([1.0, 0.0, 0.5, 0.0, 4.0, 1.0]))
    with pytest.raises(RuntimeError, match="NA in params"):
        call(g, ng, nil, lo, hi, r.real([rmock.na_real(), 0.0, 0.5, 0.0, 1.0, 1.0]))
    for bad_lo, bad_hi in (([4.0, 0.0], [3.0, 2.0]), ([0.0, 0.0], [m + 1.0, 3.0]), ([-1.0, 0.0], [3.0, 3.0]),
                           ([0.5, 0.0], [3.0, 3.0]), ([rmock.na_real(), 0.0], [3.0, 3.0])):
        with pytest.raises(RuntimeError, match="block 1 is NA, not whole numbers or outside"):
            call(g, ng, nil, r.real(bad_lo), r.real(bad_hi), ok)
    with pytest.raises(RuntimeError, match="must be integer or double"):
        call(g, ng, nil, r.lib.rmock_str(b"a"), hi, ok)
    assert r.depth() == depth
