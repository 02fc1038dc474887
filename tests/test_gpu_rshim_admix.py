"""GPU: the R entry point of admixture, `.Call("_tidypopgen_tpg_admixture", BM, rowInd, colInd, k, seed, max_iter, tol, q0, p0)` of
shim/tpg_rshim.c (tpg_rshim_entries_admix[]), through the strict R mock: equal to the Python route bit for bit for a seeded
start and for a given q0 / p0, list names and matrix dims as INTEGRATION.md states them, protect stack balanced, backing file
untouched."""
import numpy as np
import pytest

from tests import admix_ref as ar
from tests import rmock

pytestmark = pytest.mark.gpu

CODE_012 = np.r_[0.0, 1.0, 2.0, np.full(253, np.nan)]


def _admix_entries(lib):
    tab = (rmock.Entry * 2).in_dll(lib, "tpg_rshim_entries_admix")
    out = {}
    for e in tab:
        if not e.name:
            break
        out[e.name.decode()] = (e.fun, e.numArgs)
    return out


@pytest.fixture(scope="module")
def r(tmp_path_factory):
    lib = rmock.build(tmp_path_factory.mktemp("rshim_admix"))
    lib.rmock_gctorture(1)
    lib.rmock_strict(1)
    s = rmock.Session(lib)
    s.ent = {**s.ent, **_admix_entries(lib)}
    yield s
    lib.rmock_gctorture(0)
    lib.rmock_strict(0)
    lib.R_unload_tpgshim(None)
    lib.rmock_reset()


def test_table_rows_and_arity(r):
    import os
    import re

    ent = _admix_entries(r.lib)
    assert {k: v[1] for k, v in ent.items()} == {"_tidypopgen_tpg_admixture": 9}
    assert not set(ent) & set(rmock.entries(r.lib))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "shim", "tpg_rshim.c")).read()
    for tab in set(re.findall(r"const R_CallMethodDef (tpg_rshim_entries\w*)\[\]", src)) - {"tpg_rshim_entries_admix"}:
        row = rmock.C.cast(rmock.C.addressof(rmock.Entry.in_dll(r.lib, tab)), rmock.C.POINTER(rmock.Entry))
        k = 0
        while row[k].name:
            assert row[k].name.decode() not in ent, tab
            k += 1
    ns = open(os.path.join(root, "shim", "tpgshim", "NAMESPACE")).read()
    rsrc = open(os.path.join(root, "shim", "tpgshim", "R", "tpgshim.R")).read()
    assert "export(gt_admixture_gpu)" in ns and "`_tidypopgen_tpg_admixture`" in rsrc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n,m,K", [(13, 300, 3), (65, 140, 8)])
def test_entry_equals_the_python_route(r, tmp_path, n, m, K):
    import tidypopgen_amd as tpg

    codes = ar.panel(40 + n, n + 2, m + 4, K, 0.1)[0]
    path = tmp_path / "geno.bk"
    path.write_bytes(codes.tobytes(order="F"))
    BM = r.fbm(path, n + 2, m + 4, CODE_012)
    rows, cols = np.arange(2, n + 2), np.arange(3, m + 3)  # 1-based subsets
    X = tpg.FBM.from_numpy(np.asfortranarray(codes), code256=tpg.CODE_012)
    v = tpg.View(X, rows, cols)
    nil = r.lib.rmock_nil()
    depth = r.depth()

    def check(out, want):
        assert r.lib.TYPEOF(out) == 19 and r.names(out) == ["Q", "P", "loglik", "n_iter", "converged"]
        q_s, p_s = r.lib.VECTOR_ELT(out, 0), r.lib.VECTOR_ELT(out, 1)
        assert r.lib.TYPEOF(q_s) == 14 and r.lib.TYPEOF(p_s) == 14 and r.dim(q_s) == (n, K) and r.dim(p_s) == (m, K)
        assert np.array_equal(_bits(r.as_numpy(q_s, (n, K))), _bits(want["Q"]))
        assert np.array_equal(_bits(r.as_numpy(p_s, (m, K))), _bits(want["P"]))
        ll, nit, conv = r.lib.VECTOR_ELT(out, 2), r.lib.VECTOR_ELT(out, 3), r.lib.VECTOR_ELT(out, 4)
        assert r.lib.TYPEOF(ll) == 14 and r.lib.TYPEOF(nit) == 13 and r.lib.TYPEOF(conv) == 10
        assert r.as_numpy(ll)[0] == want["loglik"] and int(r.as_numpy(nit)[0]) == want["n_iter"]
        assert bool(r.as_numpy(conv)[0]) == want["converged"]

    # a seeded start (k as R holds it: integer or double)
    for k_sexp in (r.int([K]), r.real([float(K)])):
        out = r.call("tpg_admixture", BM, r.int(rows), r.index(cols, double=True), k_sexp, r.real([12345.0]), r.int([4]),
                     r.real([1e-4]), nil, nil)
        check(out, tpg.admix_em(v, K, seed=12345, max_iter=4, tol=1e-4))
    # a given start
    rng = np.random.default_rng(n)
    Q0, F0 = rng.uniform(0.1, 1.0, size=(n, K)), rng.uniform(0.0, 1.0, size=(m, K))
    out = r.call("tpg_admixture", BM, r.int(rows), r.int(cols), r.int([K]), r.real([0.0]), r.int([3]), r.real([0.0]),
                 r.matrix(Q0), r.matrix(F0))
    check(out, tpg.admix_em(v, K, Q0=Q0, F0=F0, max_iter=3, tol=0.0))
    assert r.depth() == depth
    assert np.array_equal(np.frombuffer(path.read_bytes(), dtype=np.uint8), codes.ravel(order="F"))


def test_bad_arguments_are_r_errors(r, tmp_path):
    n, m, K = 13, 60, 2
    codes = ar.panel(9, n, m, K, 0.1)[0]
    path = tmp_path / "g.bk"
    path.write_bytes(codes.tobytes(order="F"))
    BM = r.fbm(path, n, m, CODE_012)
    rows, cols = r.int(np.arange(1, n + 1)), r.int(np.arange(1, m + 1))
    nil = r.lib.rmock_nil()
    k, seed, mi, tol = r.int([K]), r.real([1.0]), r.int([2]), r.real([1e-4])
    depth = r.depth()
    with pytest.raises(RuntimeError, match="k must be a positive integer"):
        r.call("tpg_admixture", BM, rows, cols, r.int([0]), seed, mi, tol, nil, nil)
    with pytest.raises(RuntimeError, match="K = 33"):
        r.call("tpg_admixture", BM, rows, cols, r.int([33]), seed, mi, tol, nil, nil)
    with pytest.raises(RuntimeError, match="seed must be a double vector of length 1"):
        r.call("tpg_admixture", BM, rows, cols, k, r.int([1]), mi, tol, nil, nil)
    with pytest.raises(RuntimeError, match="whole number"):
        r.call("tpg_admixture", BM, rows, cols, k, r.real([-1.0]), mi, tol, nil, nil)
    with pytest.raises(RuntimeError, match="max_iter must be"):
        r.call("tpg_admixture", BM, rows, cols, k, seed, r.int([-1]), tol, nil, nil)
    with pytest.raises(RuntimeError, match="tol must be"):
        r.call("tpg_admixture", BM, rows, cols, k, seed, mi, r.real([-1.0]), nil, nil)
    with pytest.raises(RuntimeError, match="q0 must be"):
        r.call("tpg_admixture", BM, rows, cols, k, seed, mi, tol, r.real(np.ones(n * K - 1)), nil)
    with pytest.raises(RuntimeError, match="p0 must be"):
        r.call("tpg_admixture", BM, rows, cols, k, seed, mi, tol, nil, r.real(np.ones(m * K + 1)))
    q = np.ones(n * K)
    q[3] = 0.0
    with pytest.raises(RuntimeError, match="not finite or not positive"):
        r.call("tpg_admixture", BM, rows, cols, k, seed, mi, tol, r.real(q), nil)
    assert r.depth() == depth
