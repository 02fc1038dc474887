"""GPU: the R entry point of sNMF, `.Call("_tidypopgen_tpg_snmf", BM, rowInd, colInd, k, alpha, tolerance, iterations, seed,
percentage, q0)` of shim/tpg_rshim.c (tpg_rshim_entries_snmf[]), through the strict R mock: equal to the Python route bit for bit
for a seeded start and for a given q0, with and without the hold-out, list names, types and lengths as INTEGRATION.md states
them, protect stack balanced, backing file untouched."""
import os
import re

import numpy as np
import pytest

from tests import admix_ref as ar
from tests import rmock

pytestmark = pytest.mark.gpu

CODE_012 = np.r_[0.0, 1.0, 2.0, np.full(253, np.nan)]
NAMES = ["Q", "P", "G", "ls", "n_iter", "converged", "cv", "cv_all"]


def _snmf_entries(lib):
    tab = (rmock.Entry * 2).in_dll(lib, "tpg_rshim_entries_snmf")
    out = {}
    for e in tab:
        if not e.name:
            break
        out[e.name.decode()] = (e.fun, e.numArgs)
    return out


@pytest.fixture(scope="module")
def r(tmp_path_factory):
    lib = rmock.build(tmp_path_factory.mktemp("rshim_snmf"))
    lib.rmock_gctorture(1)
    lib.rmock_strict(1)
    s = rmock.Session(lib)
    s.ent = {**s.ent, **_snmf_entries(lib)}
    yield s
    lib.rmock_gctorture(0)
    lib.rmock_strict(0)
    lib.R_unload_tpgshim(None)
    lib.rmock_reset()


def test_table_rows_and_arity(r):
    ent = _snmf_entries(r.lib)
    assert {k: v[1] for k, v in ent.items()} == {"_tidypopgen_tpg_snmf": 10}
    assert not set(ent) & set(rmock.entries(r.lib))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "shim", "tpg_rshim.c")).read()
    for tab in set(re.findall(r"const R_CallMethodDef (tpg_rshim_entries\w*)\[\]", src)) - {"tpg_rshim_entries_snmf"}:
        row = rmock.C.cast(rmock.C.addressof(rmock.Entry.in_dll(r.lib, tab)), rmock.C.POINTER(rmock.Entry))
        k = 0
        while row[k].name:
            assert row[k].name.decode() not in ent, tab
            k += 1
    assert "#pragma weak tpg_snmf" in src and "TPG_NEEDS(tpg_snmf)" in src
    ns = open(os.path.join(root, "shim", "tpgshim", "NAMESPACE")).read()
    rsrc = open(os.path.join(root, "shim", "tpgshim", "R", "tpgshim.R")).read()
    assert "export(gt_snmf_gpu)" in ns and "`_tidypopgen_tpg_snmf`" in rsrc


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

    def check(out, want, ce):
        assert r.lib.TYPEOF(out) == 19 and r.names(out) == NAMES
        q_s, p_s, g_s = (r.lib.VECTOR_ELT(out, i) for i in range(3))
        assert all(r.lib.TYPEOF(x) == 14 for x in (q_s, p_s, g_s))
        assert r.dim(q_s) == (n, K) and r.dim(p_s) == (m, K) and r.dim(g_s) == (3 * m, K)
        assert np.array_equal(_bits(r.as_numpy(q_s, (n, K))), _bits(want["Q"]))
        assert np.array_equal(_bits(r.as_numpy(p_s, (m, K))), _bits(want["P"]))
        assert np.array_equal(_bits(r.as_numpy(g_s, (3 * m, K))), _bits(want["G"]))
        ls, nit, conv, cv, cva = (r.lib.VECTOR_ELT(out, i) for i in range(3, 8))
        assert [r.lib.TYPEOF(x) for x in (ls, nit, conv, cv, cva)] == [14, 13, 10, 14, 14]
        assert all(r.lib.XLENGTH(x) == 1 for x in (ls, nit, conv, cv, cva))
        assert r.as_numpy(ls)[0] == want["ls"] and int(r.as_numpy(nit)[0]) == want["n_iter"]
        assert bool(r.as_numpy(conv)[0]) == want["converged"]
        if ce is None:
            assert r.lib.R_IsNA(r.as_numpy(cv)[0]) and r.lib.R_IsNA(r.as_numpy(cva)[0])
        else:
            assert _bits(r.as_numpy(cv)[0]) == _bits(ce["masked"]) and _bits(r.as_numpy(cva)[0]) == _bits(ce["all"])

    # a seeded start (k as R holds it: integer or double), no hold-out
    for k_sexp in (r.int([K]), r.real([float(K)])):
        out = r.call("tpg_snmf", BM, r.int(rows), r.index(cols, double=True), k_sexp, r.real([10.0]), r.real([1e-5]), r.int([4]),
                     r.real([12345.0]), nil, nil)
        check(out, tpg.snmf(v, K, seed=12345, alpha=10.0, tol=1e-5, max_iter=4), None)
    # a seeded start with the hold-out: the fit is on the training view, the cross-entropies from the pair
    out = r.call("tpg_snmf", BM, r.int(rows), r.int(cols), r.int([K]), r.int([10]), r.real([1e-5]), r.int([4]), r.real([77.0]),
                 r.real([0.1]), nil)
    t = v.holdout_fraction(0.1, 77)
    want = tpg.snmf(t, K, seed=77, alpha=10.0, tol=1e-5, max_iter=4)
    check(out, want, tpg.snmf_cross_entropy(v, t, want["Q"], want["G"]))
    # a given start
    Q0 = np.random.default_rng(n).uniform(0.1, 1.0, size=(n, K))
    out = r.call("tpg_snmf", BM, r.int(rows), r.int(cols), r.int([K]), r.real([2.5]), r.real([0.0]), r.int([3]), r.real([0.0]), nil,
                 r.matrix(Q0))
    check(out, tpg.snmf(v, K, Q0=Q0, alpha=2.5, tol=0.0, max_iter=3), None)
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
    k, al, tol, it, seed = r.int([K]), r.real([10.0]), r.real([1e-5]), r.int([2]), r.real([1.0])
    depth = r.depth()
    with pytest.raises(RuntimeError, match="k must be a positive integer"):
        r.call("tpg_snmf", BM, rows, cols, r.int([0]), al, tol, it, seed, nil, nil)
    with pytest.raises(RuntimeError, match="K = 17"):
        r.call("tpg_snmf", BM, rows, cols, r.int([17]), al, tol, it, seed, nil, nil)
    with pytest.raises(RuntimeError, match="alpha must be"):
        r.call("tpg_snmf", BM, rows, cols, k, r.real([-1.0]), tol, it, seed, nil, nil)
    with pytest.raises(RuntimeError, match="tolerance must be"):
        r.call("tpg_snmf", BM, rows, cols, k, al, r.real([-1.0]), it, seed, nil, nil)
    with pytest.raises(RuntimeError, match="iterations must be"):
        r.call("tpg_snmf", BM, rows, cols, k, al, tol, r.int([-1]), seed, nil, nil)
    with pytest.raises(RuntimeError, match="seed must be a double vector of length 1"):
        r.call("tpg_snmf", BM, rows, cols, k, al, tol, it, r.int([1]), nil, nil)
    with pytest.raises(RuntimeError, match="whole number"):
        r.call("tpg_snmf", BM, rows, cols, k, al, tol, it, r.real([0.5]), nil, nil)
    for bad in (0.0, 1.0, -0.2):
        with pytest.raises(RuntimeError, match="percentage must lie strictly between 0 and 1"):
            r.call("tpg_snmf", BM, rows, cols, k, al, tol, it, seed, r.real([bad]), nil)
    with pytest.raises(RuntimeError, match="q0 must be length"):
        r.call("tpg_snmf", BM, rows, cols, k, al, tol, it, seed, nil, r.real(np.ones(n * K - 1)))
    q = np.ones((n, K))
    q[3, 1] = np.nan
    with pytest.raises(RuntimeError, match="q0 has an entry that is not finite or not positive"):
        r.call("tpg_snmf", BM, rows, cols, k, al, tol, it, seed, nil, r.matrix(q))
    assert r.depth() == depth
