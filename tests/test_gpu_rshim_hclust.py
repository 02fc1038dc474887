"""GPU: the R entry point of the Ward clusters on PCA scores, `.Call("_tidypopgen_tpg_cluster_pca_ward", scores, k, power)` of
shim/tpg_rshim.c (tpg_rshim_entries_hclust[]), through the strict R mock: equal to the Python route (gt_cluster_pca_ward) bit for
bit, list names, types and dims as INTEGRATION.md states them, argument-type refusals, protect stack balanced."""
import os
import re

import numpy as np
import pytest

from tests import rmock

pytestmark = pytest.mark.gpu

NAMES = ["groups", "WSS", "merge", "height"]


def _hclust_entries(lib):
    tab = (rmock.Entry * 2).in_dll(lib, "tpg_rshim_entries_hclust")
    out = {}
    for e in tab:
        if not e.name:
            break
        out[e.name.decode()] = (e.fun, e.numArgs)
    return out


@pytest.fixture(scope="module")
def r(tmp_path_factory):
    lib = rmock.build(tmp_path_factory.mktemp("rshim_hclust"))
    lib.rmock_gctorture(1)
    lib.rmock_strict(1)
    s = rmock.Session(lib)
    s.ent = {**s.ent, **_hclust_entries(lib)}
    yield s
    lib.rmock_gctorture(0)
    lib.rmock_strict(0)
    lib.R_unload_tpgshim(None)
    lib.rmock_reset()


def test_table_rows_and_arity(r):
    ent = _hclust_entries(r.lib)
    assert {k: v[1] for k, v in ent.items()} == {"_tidypopgen_tpg_cluster_pca_ward": 3}
    assert not set(ent) & set(rmock.entries(r.lib))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "shim", "tpg_rshim.c")).read()
    tables = set(re.findall(r"const R_CallMethodDef (tpg_rshim_entries\w*)\[\]", src))
    assert "tpg_rshim_entries_hclust" in tables and "tpg_rshim_entries_cluster" in tables
    for tab in tables - {"tpg_rshim_entries_hclust"}:
        row = rmock.C.cast(rmock.C.addressof(rmock.Entry.in_dll(r.lib, tab)), rmock.C.POINTER(rmock.Entry))
        k = 0
        while row[k].name:
            assert row[k].name.decode() not in ent, tab
            k += 1
    for sym in ("tpg_hclust_ward", "tpg_hclust_cut", "tpg_hclust_r_merge", "tpg_cluster_wss"):
        assert f"#pragma weak {sym}\n" in src and f"TPG_NEEDS({sym})" in src
    assert "for (const R_CallMethodDef* e = tpg_rshim_entries_hclust; e->name; e++) all[k++] = *e;" in src
    assert "sizeof(tpg_rshim_entries_hclust) / sizeof(tpg_rshim_entries_hclust[0])" in src
    ns = open(os.path.join(root, "shim", "tpgshim", "NAMESPACE")).read()
    rsrc = open(os.path.join(root, "shim", "tpgshim", "R", "tpgshim.R")).read()
    assert "export(gt_cluster_pca_ward_gpu)" in ns and "`_tidypopgen_tpg_cluster_pca_ward`" in rsrc


def _scores(seed, n, d, g=3):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.normal(size=(g, d))[np.arange(n) % g] * 6.0 + rng.normal(size=(n, d)))


@pytest.mark.parametrize("n,d,ks", [(65, 3, [1, 2, 3, 4]), (301, 17, [3, 7, 65, 301])])
def test_entry_equals_the_python_route(r, n, d, ks):
    import tidypopgen_amd as tpg

    X = _scores(n + d, n, d)
    depth = r.depth()
    for criterion, power in (("reference", r.int([2])), ("ward", r.real([1.0]))):  # power as R holds it: integer or double
        for k_sexp in (r.int(ks), r.real([float(k) for k in ks])):
            out = r.call("tpg_cluster_pca_ward", r.matrix(X), k_sexp, power)
            assert r.lib.TYPEOF(out) == 19 and r.names(out) == NAMES
            g, w, mg, h = (r.lib.VECTOR_ELT(out, i) for i in range(4))
            assert [r.lib.TYPEOF(x) for x in (g, w, mg, h)] == [13, 14, 13, 14]
            assert r.dim(g) == (n, len(ks)) and r.dim(mg) == (n - 1, 2)
            assert r.lib.XLENGTH(w) == len(ks) and r.lib.XLENGTH(h) == n - 1
            # the Python route, k by k and all k at once: the tree does not depend on k
            pca = dict(u=X, d=np.ones(d))
            for pos, k in enumerate(ks):
                cl = tpg.gt_cluster_pca_ward(pca, k_clusters=k, criterion=criterion)["clusters"]
                assert np.array_equal(r.as_numpy(g, (n, len(ks)))[:, pos], cl["groups"][k])
                assert r.as_numpy(w)[pos:pos + 1].view(np.uint64)[0] == np.array([cl["WSS"][0]]).view(np.uint64)[0]
            assert np.array_equal(r.as_numpy(mg, (n - 1, 2)), cl["merge"])
            assert np.array_equal(r.as_numpy(h).view(np.uint64), cl["height"].view(np.uint64))
    assert r.depth() == depth


def test_bad_arguments_are_r_errors(r):
    X = _scores(1, 20, 2)
    sc, k, pw = r.matrix(X), r.int([2, 3]), r.int([2])
    depth = r.depth()
    with pytest.raises(RuntimeError, match="scores must be a numeric matrix"):
        r.call("tpg_cluster_pca_ward", r.real(X.ravel()), k, pw)  # no dim attribute
    with pytest.raises(RuntimeError, match="scores must be a numeric matrix"):
        r.call("tpg_cluster_pca_ward", r.lib.rmock_str(b"x"), k, pw)
    with pytest.raises(RuntimeError, match="k must be a vector of whole numbers"):
        r.call("tpg_cluster_pca_ward", sc, r.lib.rmock_str(b"2"), pw)
    for bad in ([0], [21], [2.5]):
        with pytest.raises(RuntimeError, match="every k must be a whole number"):
            r.call("tpg_cluster_pca_ward", sc, r.real(bad), pw)
    for bad in (r.int([3]), r.real([0.0]), r.int([1, 2]), r.lib.rmock_str(b"2")):
        with pytest.raises(RuntimeError, match="power must be 1 or 2"):
            r.call("tpg_cluster_pca_ward", sc, k, bad)
    with pytest.raises(RuntimeError, match="k = 1025 is above 1024"):  # (refused before the tree of 1030 points is built)
        r.call("tpg_cluster_pca_ward", r.matrix(np.zeros((1030, 1))), r.int([2, 1025]), pw)
    with pytest.raises(RuntimeError, match="k holds more than 65535 values"):
        r.call("tpg_cluster_pca_ward", sc, r.int([2] * 65536), pw)
    Xn = X.copy()
    Xn[3, 1] = np.nan
    with pytest.raises(RuntimeError, match="not finite"):
        r.call("tpg_cluster_pca_ward", r.matrix(Xn), k, pw)
    wide = np.zeros((4, 65))
    with pytest.raises(RuntimeError, match="d = 65"):
        r.call("tpg_cluster_pca_ward", r.matrix(wide), r.int([2]), pw)
    assert r.depth() == depth
