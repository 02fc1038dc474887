"""GPU: the R entry point of autoSVD, `.Call("_tidypopgen_tpg_pca_auto_svd", BM, rowInd, colInd, chrom, pos, hi, params)` of
shim/tpg_rshim.c (tpg_rshim_entries_autosvd[]), through the strict R mock: the same list and attributes as the Python call on
the planted panel, bit for bit; protect stack balanced, backing file untouched, bad arguments R errors."""
import os
import re

import numpy as np
import pytest

from tests import autosvd_ref as ar
from tests import rmock

pytestmark = pytest.mark.gpu

CODE_012 = np.r_[0.0, 1.0, 2.0, np.full(253, np.nan)]
PARAMS = [ar.PANEL_K, ar.PANEL_THR, ar.PANEL_ROLL, 20, 0.05, 10, 5]


def _autosvd_entries(lib):
    tab = (rmock.Entry * 2).in_dll(lib, "tpg_rshim_entries_autosvd")
    out = {}
    for e in tab:
        if not e.name:
            break
        out[e.name.decode()] = (e.fun, e.numArgs)
    return out


@pytest.fixture(scope="module")
def r(tmp_path_factory):
    lib = rmock.build(tmp_path_factory.mktemp("rshim_autosvd"))
    lib.Rf_install.restype, lib.Rf_install.argtypes = rmock.C.c_void_p, [rmock.C.c_char_p]
    lib.rmock_gctorture(1)
    lib.rmock_strict(1)
    s = rmock.Session(lib)
    s.ent = {**s.ent, **_autosvd_entries(lib)}
    yield s
    lib.rmock_gctorture(0)
    lib.rmock_strict(0)
    lib.R_unload_tpgshim(None)
    lib.rmock_reset()


def test_table_rows_and_arity(r):
    ent = _autosvd_entries(r.lib)
    assert {k: v[1] for k, v in ent.items()} == {"_tidypopgen_tpg_pca_auto_svd": 7}
    assert not set(ent) & set(rmock.entries(r.lib))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "shim", "tpg_rshim.c")).read()
    tabs = set(re.findall(r"const R_CallMethodDef (tpg_rshim_entries\w*)\[\]", src))
    assert "tpg_rshim_entries_autosvd" in tabs
    for tab in tabs:  # every table is registered by the stand-alone package
        assert f"e = {tab};" in src, tab
    assert "#pragma weak tpg_pca_auto_svd" in src and "TPG_NEEDS(tpg_pca_auto_svd)" in src
    ns = open(os.path.join(root, "shim", "tpgshim", "NAMESPACE")).read()
    rsrc = open(os.path.join(root, "shim", "tpgshim", "R", "tpgshim.R")).read()
    assert "export(gt_pca_autoSVD_gpu)" in ns and "`_tidypopgen_tpg_pca_auto_svd`" in rsrc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _attr(r, sexp, name):
    return r.lib.Rf_getAttrib(sexp, r.lib.Rf_install(name.encode()))


def test_entry_equals_the_python_route(r, tmp_path):
    import tidypopgen_amd as tpg
    from tidypopgen_amd import api

    G = ar.planted_panel(ar.PANEL_SEED).astype(np.uint8)
    n, m = G.shape
    path = tmp_path / "geno.bk"
    path.write_bytes(G.tobytes(order="F"))
    BM = r.fbm(path, n, m, CODE_012)
    X = tpg.FBM.from_numpy(np.asfortranarray(G), code256=tpg.CODE_012)
    want = tpg.gt_pca_autoSVD(X, k=ar.PANEL_K, thr_r2=ar.PANEL_THR, use_positions=False, size=ar.PANEL_WINDOW,
                              roll_size=ar.PANEL_ROLL, chromosome=ar.CHROM, position=ar.POSITION)
    assert want["converged"] and len(want["lrldr"]) == 1
    hi = api.ld_window_hi(ar.CHROM, None, ar.PANEL_WINDOW, use_positions=False)
    rows, cols = np.arange(1, n + 1), np.arange(1, m + 1)
    depth = r.depth()
    for ri, ci, hs in ((r.int(rows), r.int(cols), r.real(hi)), (r.index(rows, double=True), r.index(cols, double=True), r.int(hi))):
        out = r.call("tpg_pca_auto_svd", BM, ri, ci, r.int(ar.CHROM), r.real(ar.POSITION), hs, r.real(PARAMS))
        assert r.lib.TYPEOF(out) == 19 and r.names(out) == ["d", "u", "v", "center", "scale", "n_iter", "converged"]
        mk = len(want["loci"])
        for i, (name, shape) in enumerate((("d", (ar.PANEL_K,)), ("u", (n, ar.PANEL_K)), ("v", (mk, ar.PANEL_K)), ("center", (mk,)),
                                           ("scale", (mk,)))):
            s = r.lib.VECTOR_ELT(out, i)
            assert r.lib.TYPEOF(s) == 14
            got = r.as_numpy(s, shape if len(shape) == 2 else None)
            assert got.shape == shape and np.array_equal(_bits(got), _bits(want[name])), name
            assert r.dim(s) == (shape if len(shape) == 2 else None)
        assert r.as_numpy(r.lib.VECTOR_ELT(out, 5)).tolist() == [want["n_iter"]]
        assert r.lib.TYPEOF(r.lib.VECTOR_ELT(out, 6)) == 10 and r.as_numpy(r.lib.VECTOR_ELT(out, 6)).tolist() == [1]
        sub = _attr(r, out, "subset")
        assert r.lib.TYPEOF(sub) == 13 and np.array_equal(r.as_numpy(sub), want["loci"])
        lr = _attr(r, out, "lrldr")
        assert r.lib.TYPEOF(lr) == 19 and r.names(lr) == ["Chr", "Start", "Stop"]
        got = list(zip(*(r.as_numpy(r.lib.VECTOR_ELT(lr, i)).tolist() for i in range(3))))
        assert got == [(c, float(a), float(b)) for c, a, b in want["lrldr"]]
    # without positions there is no lrldr; without a window nothing is clumped
    out = r.call("tpg_pca_auto_svd", BM, r.int(rows), r.int(cols), r.int(ar.CHROM), r.lib.rmock_nil(), r.lib.rmock_nil(), r.real(PARAMS))
    noclump = tpg.gt_pca_autoSVD(X, k=ar.PANEL_K, thr_r2=None, roll_size=ar.PANEL_ROLL, chromosome=ar.CHROM)
    assert np.array_equal(r.as_numpy(_attr(r, out, "subset")), noclump["loci"])
    assert r.lib.XLENGTH(r.lib.VECTOR_ELT(_attr(r, out, "lrldr"), 0)) == 0
    assert np.array_equal(_bits(r.as_numpy(r.lib.VECTOR_ELT(out, 0))), _bits(noclump["d"]))
    assert r.depth() == depth
    assert np.array_equal(np.frombuffer(path.read_bytes(), dtype=np.uint8), G.ravel(order="F"))


def test_bad_arguments_are_r_errors(r, tmp_path):
    G = ar.planted_panel(ar.PANEL_SEED).astype(np.uint8)
    n, m = G.shape
    path = tmp_path / "g.bk"
    path.write_bytes(G.tobytes(order="F"))
    BM = r.fbm(path, n, m, CODE_012)
    rows, cols, nil = r.int(np.arange(1, n + 1)), r.int(np.arange(1, m + 1)), r.lib.rmock_nil()
    depth = r.depth()
    with pytest.raises(RuntimeError, match="differ in length"):
        r.call("tpg_pca_auto_svd", BM, rows, cols, r.int(ar.CHROM[:-1]), nil, nil, r.real(PARAMS))
    with pytest.raises(RuntimeError, match="params must be 7 numbers"):
        r.call("tpg_pca_auto_svd", BM, rows, cols, r.int(ar.CHROM), nil, nil, r.real(PARAMS[:6]))
    with pytest.raises(RuntimeError, match="roll_size"):
        r.call("tpg_pca_auto_svd", BM, rows, cols, r.int(ar.CHROM), nil, nil, r.real(PARAMS[:2] + [-1] + PARAMS[3:]))
    with pytest.raises(RuntimeError, match="roll_size exceeds the number of variants"):
        r.call("tpg_pca_auto_svd", BM, rows, cols, r.int(ar.CHROM), nil, nil, r.real(PARAMS[:2] + [400] + PARAMS[3:]))
    chrom = ar.CHROM.copy()
    chrom[-5:] = 1
    with pytest.raises(RuntimeError, match="more than one run"):
        r.call("tpg_pca_auto_svd", BM, rows, cols, r.int(chrom), nil, nil, r.real(PARAMS))
    Gm = G.copy()
    Gm[4, 9] = 3
    path2 = tmp_path / "g2.bk"
    path2.write_bytes(Gm.tobytes(order="F"))
    with pytest.raises(RuntimeError, match="missing values"):
        r.call("tpg_pca_auto_svd", r.fbm(path2, n, m, CODE_012), rows, cols, r.int(ar.CHROM), nil, nil, r.real(PARAMS))
    assert r.depth() == depth
