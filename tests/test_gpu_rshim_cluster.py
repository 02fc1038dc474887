"""GPU: the R entry point of the clusters on PCA scores, `.Call("_tidypopgen_tpg_cluster_pca", scores, k, n_start, n_iter, seed)`
of shim/tpg_rshim.c (tpg_rshim_entries_cluster[]), through the strict R mock: equal to the Python route (gt_cluster_pca) bit for
bit, list names, types and lengths as INTEGRATION.md states them, argument-type refusals, protect stack balanced."""
import os
import re

import numpy as np
import pytest

from tests import rmock

pytestmark = pytest.mark.gpu

NAMES = ["groups", "WSS", "n_iter", "converged", "n_empty"]


def _cluster_entries(lib):
    tab = (rmock.Entry * 2).in_dll(lib, "tpg_rshim_entries_cluster")
    out = {}
    for e in tab:
        if not e.name:
            break
        out[e.name.decode()] = (e.fun, e.numArgs)
    return out


@pytest.fixture(scope="module")
def r(tmp_path_factory):
    lib = rmock.build(tmp_path_factory.mktemp("rshim_cluster"))
    lib.rmock_gctorture(1)
    lib.rmock_strict(1)
    s = rmock.Session(lib)
    s.ent = {**s.ent, **_cluster_entries(lib)}
    yield s
    lib.rmock_gctorture(0)
    lib.rmock_strict(0)
    lib.R_unload_tpgshim(None)
    lib.rmock_reset()


def test_table_rows_and_arity(r):
    ent = _cluster_entries(r.lib)
    assert {k: v[1] for k, v in ent.items()} == {"_tidypopgen_tpg_cluster_pca": 5}
    assert not set(ent) & set(rmock.entries(r.lib))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "shim", "tpg_rshim.c")).read()
    for tab in set(re.findall(r"const R_CallMethodDef (tpg_rshim_entries\w*)\[\]", src)) - {"tpg_rshim_entries_cluster"}:
        row = rmock.C.cast(rmock.C.addressof(rmock.Entry.in_dll(r.lib, tab)), rmock.C.POINTER(rmock.Entry))
        k = 0
        while row[k].name:
            assert row[k].name.decode() not in ent, tab
            k += 1
    assert "#pragma weak tpg_kmeans_batch" in src and "TPG_NEEDS(tpg_kmeans_batch)" in src
    assert "for (const R_CallMethodDef* e = tpg_rshim_entries_cluster; e->name; e++) all[k++] = *e;" in src
    ns = open(os.path.join(root, "shim", "tpgshim", "NAMESPACE")).read()
    rsrc = open(os.path.join(root, "shim", "tpgshim", "R", "tpgshim.R")).read()
    assert "export(gt_cluster_pca_gpu)" in ns and "`_tidypopgen_tpg_cluster_pca`" in rsrc


def _scores(seed, n, d, g=3):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.normal(size=(g, d))[np.arange(n) % g] * 6.0 + rng.normal(size=(n, d)))


@pytest.mark.parametrize("n,d,ks,n_start", [(65, 3, [1, 2, 3, 4], 3), (301, 17, [3, 7, 65], 2)])
def test_entry_equals_the_python_route(r, n, d, ks, n_start):
    import tidypopgen_amd as tpg

    X = _scores(n + d, n, d)
    depth = r.depth()
    for k_sexp in (r.int(ks), r.real([float(k) for k in ks])):  # k as R holds it: integer or double
        out = r.call("tpg_cluster_pca", r.matrix(X), k_sexp, r.int([n_start]), r.real([1e5]), r.real([77.0]))
        assert r.lib.TYPEOF(out) == 19 and r.names(out) == NAMES
        g, w, it, cv, em = (r.lib.VECTOR_ELT(out, i) for i in range(5))
        assert [r.lib.TYPEOF(x) for x in (g, w, it, cv, em)] == [13, 14, 13, 10, 13]
        assert r.dim(g) == (n, len(ks)) and all(r.lib.XLENGTH(x) == len(ks) for x in (w, it, cv, em))
        # the Python route, k by k (every k of it starts from the same run seeds whatever else is in the batch)
        for pos, k in enumerate(ks):
            pca = dict(u=X, d=np.ones(d))
            cl = tpg.gt_cluster_pca(pca, k_clusters=k, n_start=n_start, seed=77)["clusters"]
            assert np.array_equal(r.as_numpy(g, (n, len(ks)))[:, pos], cl["groups"][k])
            assert r.as_numpy(w)[pos:pos + 1].view(np.uint64)[0] == np.array([cl["WSS"][0]]).view(np.uint64)[0]
            assert int(r.as_numpy(it)[pos]) == cl["n_iter"][0] and bool(r.as_numpy(cv)[pos]) == cl["converged"][0]
            assert int(r.as_numpy(em)[pos]) == cl["n_empty"][0]
    assert r.depth() == depth


def test_bad_arguments_are_r_errors(r):
    X = _scores(1, 20, 2)
    sc, k, ns, ni, seed = r.matrix(X), r.int([2, 3]), r.int([2]), r.int([100]), r.real([1.0])
    depth = r.depth()
    with pytest.raises(RuntimeError, match="scores must be a numeric matrix"):
        r.call("tpg_cluster_pca", r.real(X.ravel()), k, ns, ni, seed)  # no dim attribute
    with pytest.raises(RuntimeError, match="scores must be a numeric matrix"):
        r.call("tpg_cluster_pca", r.lib.rmock_str(b"x"), k, ns, ni, seed)
    with pytest.raises(RuntimeError, match="k must be a vector of whole numbers"):
        r.call("tpg_cluster_pca", sc, r.lib.rmock_str(b"2"), ns, ni, seed)
    for bad in ([0], [21], [2.5]):
        with pytest.raises(RuntimeError, match="every k must be a whole number"):
            r.call("tpg_cluster_pca", sc, r.real(bad), ns, ni, seed)
    with pytest.raises(RuntimeError, match="n_start must be a positive integer"):
        r.call("tpg_cluster_pca", sc, k, r.int([0]), ni, seed)
    with pytest.raises(RuntimeError, match="n_iter must be a positive integer"):
        r.call("tpg_cluster_pca", sc, k, ns, r.int([0]), seed)
    with pytest.raises(RuntimeError, match="seed must be a double vector of length 1"):
        r.call("tpg_cluster_pca", sc, k, ns, ni, r.int([1]))
    with pytest.raises(RuntimeError, match="whole number in"):
        r.call("tpg_cluster_pca", sc, k, ns, ni, r.real([0.5]))
    Xn = X.copy()
    Xn[3, 1] = np.nan
    with pytest.raises(RuntimeError, match="not finite"):
        r.call("tpg_cluster_pca", r.matrix(Xn), k, ns, ni, seed)
    wide = np.zeros((4, 65))
    with pytest.raises(RuntimeError, match="d = 65"):
        r.call("tpg_cluster_pca", r.matrix(wide), r.int([2]), ns, ni, seed)
    assert r.depth() == depth
