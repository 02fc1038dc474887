"""GPU: the R entry point of runs of homozygosity, `.Call("_tidypopgen_tpg_indiv_roh", BM, rowInd, colInd, chrom, pos, params)`
of shim/tpg_rshim.c (tpg_rshim_entries_roh[]), through the strict R mock: a list of integer and double columns equal to the
Python route and to the numpy restatement with 1-based indices, protect stack balanced, backing file untouched."""
import numpy as np
import pytest

from tests import rmock
from tests import roh_ref as rr

pytestmark = pytest.mark.gpu

CODE_012 = np.r_[0.0, 1.0, 2.0, np.full(253, np.nan)]
NAMES = ["indiv", "nSNP", "from", "to", "lengthBps", "first", "last"]


def _roh_entries(lib):
    tab = (rmock.Entry * 4).in_dll(lib, "tpg_rshim_entries_roh")
    out = {}
    for e in tab:
        if not e.name:
            break
        out[e.name.decode()] = (e.fun, e.numArgs)
    return out


@pytest.fixture(scope="module")
def r(tmp_path_factory):
    lib = rmock.build(tmp_path_factory.mktemp("rshim_roh"))
    lib.rmock_gctorture(1)
    lib.rmock_strict(1)
    s = rmock.Session(lib)
    s.ent = {**s.ent, **_roh_entries(lib)}
    yield s
    lib.rmock_gctorture(0)
    lib.rmock_strict(0)
    lib.R_unload_tpgshim(None)
    lib.rmock_reset()


def _params(**kw):
    p = rr.params(**kw)
    na = rmock.na_real()
    return np.array([p["window_size"], p["threshold"], p["min_snp"], float(p["heterozygosity"]), p["max_opp_window"],
                     p["max_miss_window"], p["max_gap"], p["min_length_bps"], p["min_density"],
                     na if p["max_opp_run"] is None else p["max_opp_run"], na if p["max_miss_run"] is None else p["max_miss_run"]],
                    dtype=np.float64)


def test_table_row_and_arity(r):
    ent = _roh_entries(r.lib)
    assert {k: v[1] for k, v in ent.items()} == {"_tidypopgen_tpg_indiv_roh": 6}
    assert not set(ent) & set(rmock.entries(r.lib))


@pytest.mark.parametrize("n,m,W", [(12, 200, 4), (65, 1000, 15), (40, 4097, 50)])
def test_list_equals_the_python_route(r, tmp_path, n, m, W):
    import tidypopgen_amd as tpg

    G = rr.roh_panel(20 + W, n, m, W)
    path = tmp_path / "geno.bk"
    path.write_bytes(G.tobytes(order="F"))
    BM = r.fbm(path, n, m, CODE_012)
    rng = np.random.default_rng(n)
    rows = np.sort(rng.permutation(n)[: max(2, (3 * n) // 4)]) + 1
    cols = np.arange(3, m - 2)
    chrom, pos = rr.roh_loci(20 + W, len(cols), W=W)
    sub = G[np.ix_(rows - 1, cols - 1)]
    X = tpg.FBM.from_numpy(np.asfortranarray(G), code256=tpg.CODE_012)
    depth = r.depth()
    for kw in (dict(window_size=W), dict(window_size=W, max_opp_run=0, **rr.UNFILTERED),
               dict(window_size=W, heterozygosity=True, max_opp_window=(2 * W) // 3, max_miss_run=1, **rr.UNFILTERED)):
        want = rr.roh_vec(sub, chrom, pos, **kw)
        py = tpg.windows_indiv_roh(X, rows, cols, chromosome=chrom, position=pos, **kw)
        for pos_sexp in (r.real(pos.astype(np.float64)), r.int(pos)):  # positions as R holds them: double or integer
            out = r.call("tpg_indiv_roh", BM, r.int(rows), r.index(cols, double=True), r.int(chrom), pos_sexp, r.real(_params(**kw)))
            assert r.lib.TYPEOF(out) == 19 and r.names(out) == NAMES  # VECSXP
            types = [r.lib.TYPEOF(r.lib.VECTOR_ELT(out, k)) for k in range(7)]
            assert types == [13, 13, 14, 14, 14, 13, 13]  # INTSXP / REALSXP
            got = {k: r.list_elt(out, i) for i, k in enumerate(NAMES)}
            assert np.array_equal(got["indiv"], want["indiv"] + 1)
            assert np.array_equal(got["first"], want["first"] + 1) and np.array_equal(got["last"], want["last"] + 1)
            assert np.array_equal(got["first"], py["first_locus"] + 1) and np.array_equal(got["last"], py["last_locus"] + 1)
            assert np.array_equal(got["nSNP"], py["nSNP"]) and np.array_equal(got["from"], py["from"])
            assert np.array_equal(got["to"], py["to"]) and np.array_equal(got["lengthBps"], py["lengthBps"])
    assert len(want["indiv"]) > 0
    assert r.depth() == depth
    assert np.array_equal(np.frombuffer(path.read_bytes(), dtype=np.uint8), G.ravel(order="F"))


def test_bad_arguments_are_r_errors(r, tmp_path):
    n, m = 20, 60
    G = rr.roh_panel(3, n, m, 15)
    path = tmp_path / "g.bk"
    path.write_bytes(G.tobytes(order="F"))
    BM = r.fbm(path, n, m, CODE_012)
    rows, cols = np.arange(1, n + 1), np.arange(1, m + 1)
    chrom, pos = rr.roh_loci(3, m, W=15)
    fpos = pos.astype(np.float64)
    depth = r.depth()
    ok = r.real(_params())
    with pytest.raises(RuntimeError, match="differ in length"):
        r.call("tpg_indiv_roh", BM, r.int(rows), r.int(cols), r.int(chrom[:-1]), r.real(fpos), ok)
    with pytest.raises(RuntimeError, match="differ in length"):
        r.call("tpg_indiv_roh", BM, r.int(rows), r.int(cols), r.int(chrom), r.real(fpos[:-1]), ok)
    with pytest.raises(RuntimeError, match="11 numbers"):
        r.call("tpg_indiv_roh", BM, r.int(rows), r.int(cols), r.int(chrom), r.real(fpos), r.real(_params()[:10]))
    with pytest.raises(RuntimeError, match="NA in params"):
        r.call("tpg_indiv_roh", BM, r.int(rows), r.int(cols), r.int(chrom), r.real(fpos), r.real(np.r_[rmock.na_real(), _params()[1:]]))
    with pytest.raises(RuntimeError, match="NA in chrom or pos"):
        r.call("tpg_indiv_roh", BM, r.int(rows), r.int(cols), r.int(chrom), r.real(np.r_[fpos[:5], rmock.na_real(), fpos[6:]]), ok)
    with pytest.raises(RuntimeError, match="window_size"):
        r.call("tpg_indiv_roh", BM, r.int(rows), r.int(cols), r.int(chrom), r.real(fpos), r.real(_params(window_size=513)))
    text = r.lib.rmock_str(b"chr1")  # a wrong type: a character vector where numbers are expected
    for args in ((text, r.real(fpos), ok), (r.int(chrom), text, ok), (r.int(chrom), r.real(fpos), text)):
        with pytest.raises(RuntimeError, match="must be integer or double"):
            r.call("tpg_indiv_roh", BM, r.int(rows), r.int(cols), *args)
    with pytest.raises(RuntimeError, match="whole number"):
        r.call("tpg_indiv_roh", BM, r.int(rows), r.int(cols), r.int(chrom), r.real(fpos), r.real(np.r_[15.5, _params()[1:]]))
    with pytest.raises(RuntimeError, match="whole number"):
        r.call("tpg_indiv_roh", BM, r.int(rows), r.int(cols), r.int(chrom), r.real(fpos), r.real(np.r_[_params()[:2], 1e12, _params()[3:]]))
    back = fpos.copy()
    back[1] = back[0] - 1
    ch1 = np.ones(m, dtype=np.int32)
    with pytest.raises(RuntimeError, match="not ordered"):
        r.call("tpg_indiv_roh", BM, r.int(rows), r.int(cols), r.int(ch1), r.real(back), ok)
    assert r.depth() == depth
