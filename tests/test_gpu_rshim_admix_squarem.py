"""GPU: the R entry points of the accelerated admixture, `.Call("_tidypopgen_tpg_admixture_squarem", BM, rowInd, colInd, k, seed,
max_iter, tol, q0, p0)` (tpg_rshim_entries_admix_squarem[]) and `.Call("_tidypopgen_tpg_admixture_cv_squarem", ..., folds,
cv_seed)` (tpg_rshim_entries_admix_cv_squarem[]) of shim/tpg_rshim.c, through the strict R mock: equal to the Python route
(accel="squarem") bit for bit for a seeded start and for a given q0 / p0, list names, types and dims as INTEGRATION.md states
them, protect stack balanced, backing file untouched; the plain rows keep their tables and arities."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import admix_ref as ar
from tests import rmock
from tests.test_gpu_rshim_admix_cv import _build

pytestmark = pytest.mark.gpu

CODE_012 = np.r_[0.0, 1.0, 2.0, np.full(253, np.nan)]
EM, CV = "_tidypopgen_tpg_admixture_squarem", "_tidypopgen_tpg_admixture_cv_squarem"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(lib, name):
    tab = (rmock.Entry * 2).in_dll(lib, name)
    out = {}
    for e in tab:
        if not e.name:
            break
        out[e.name.decode()] = (e.fun, e.numArgs)
    return out


@pytest.fixture(scope="module")
def r(tmp_path_factory):
    lib = _build(tmp_path_factory.mktemp("rshim_admix_squarem"))  # the shim, the mock runtime and the 11-argument trampoline
    lib.rmock_gctorture(1)
    lib.rmock_strict(1)
    s = rmock.Session(lib)
    s.ent = {**s.ent, **_table(lib, "tpg_rshim_entries_admix_squarem"), **_table(lib, "tpg_rshim_entries_admix_cv_squarem"),
             **_table(lib, "tpg_rshim_entries_admix")}  # the plain row, to call it beside the accelerated one
    yield s
    lib.rmock_gctorture(0)
    lib.rmock_strict(0)
    lib.R_unload_tpgshim(None)
    lib.rmock_reset()


def _call_cv(r, *args):
    """the 11 arguments of the cross-validation row: ten through rmock_call_named, the last parked in the trampoline and held to
    the strict rule here (as tests/test_gpu_rshim_admix_cv.py does)"""
    fn, arity = r.ent[CV]
    assert arity == len(args) == 11, (CV, arity, len(args))
    last = args[10]
    before = (r.lib.TYPEOF(last), r.as_numpy(last).tobytes())
    r.lib.rmock_call11_set(fn, last)
    arr = (C.c_void_p * 10)(*args[:10])
    out = r.lib.rmock_call_named(b"tpg_admixture_cv_squarem", C.cast(r.lib.rmock_call11_trampoline, C.c_void_p), 10, arr)
    assert (r.lib.TYPEOF(last), r.as_numpy(last).tobytes()) == before
    if out is None:
        raise RuntimeError(r.lib.rmock_last_error().decode())
    return out


def test_table_rows_and_arity(r):
    em, cv = _table(r.lib, "tpg_rshim_entries_admix_squarem"), _table(r.lib, "tpg_rshim_entries_admix_cv_squarem")
    assert {k: v[1] for k, v in em.items()} == {EM: 9} and {k: v[1] for k, v in cv.items()} == {CV: 11}
    # the plain rows are where they were
    assert {k: v[1] for k, v in _table(r.lib, "tpg_rshim_entries_admix").items()} == {"_tidypopgen_tpg_admixture": 9}
    assert {k: v[1] for k, v in _table(r.lib, "tpg_rshim_entries_admix_cv").items()} == {"_tidypopgen_tpg_admixture_cv": 11}
    assert not (set(em) | set(cv)) & set(rmock.entries(r.lib))
    src = open(os.path.join(ROOT, "shim", "tpg_rshim.c")).read()
    tables = set(re.findall(r"const R_CallMethodDef (tpg_rshim_entries\w*)\[\]", src))
    own = {"tpg_rshim_entries_admix_squarem", "tpg_rshim_entries_admix_cv_squarem"}
    assert own <= tables
    for tab in tables - own:
        row = rmock.C.cast(rmock.C.addressof(rmock.Entry.in_dll(r.lib, tab)), rmock.C.POINTER(rmock.Entry))
        k = 0
        while row[k].name:
            assert row[k].name.decode() not in em and row[k].name.decode() not in cv, tab
            k += 1
    for tab in own:  # registered in the stand-alone concatenation
        assert f"for (const R_CallMethodDef* e = {tab}; e->name; e++) all[k++] = *e;" in src
        assert f"sizeof({tab}) / sizeof({tab}[0])" in src
    for sym in ("tpg_admix_em_squarem", "tpg_admix_cv_squarem"):
        assert f"#pragma weak {sym}\n" in src and f"TPG_NEEDS({sym})" in src
    ns = open(os.path.join(ROOT, "shim", "tpgshim", "NAMESPACE")).read()
    rsrc = open(os.path.join(ROOT, "shim", "tpgshim", "R", "tpgshim.R")).read()
    assert "export(gt_admixture_squarem_gpu)" in ns and f"`{EM}`" in rsrc and f"`{CV}`" in rsrc
    # a wrong number of arguments is refused before the call, as for every row
    nil = r.lib.rmock_nil()
    with pytest.raises(AssertionError, match="tpg_admixture_squarem"):
        r.call("tpg_admixture_squarem", *([nil] * 8))
    with pytest.raises(AssertionError, match="tpg_admixture_cv_squarem"):
        _call_cv(r, *([nil] * 10))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _panel(r, tmp_path, n, m, K):
    import tidypopgen_amd as tpg

    codes = ar.panel(40 + n, n + 2, m + 4, K, 0.1)[0]
    path = tmp_path / "geno.bk"
    path.write_bytes(codes.tobytes(order="F"))
    BM = r.fbm(path, n + 2, m + 4, CODE_012)
    rows, cols = np.arange(2, n + 2), np.arange(3, m + 3)  # 1-based subsets
    X = tpg.FBM.from_numpy(np.asfortranarray(codes), code256=tpg.CODE_012)
    return codes, path, BM, rows, cols, tpg.View(X, rows, cols)


@pytest.mark.parametrize("n,m,K", [(13, 300, 3), (65, 140, 8)])
def test_em_entry_equals_the_python_route(r, tmp_path, n, m, K):
    import tidypopgen_amd as tpg

    codes, path, BM, rows, cols, v = _panel(r, tmp_path, n, m, K)
    nil = r.lib.rmock_nil()
    depth = r.depth()

    def check(out, want):
        assert r.lib.TYPEOF(out) == 19 and r.names(out) == ["Q", "P", "loglik", "n_iter", "converged", "n_cycles", "n_rejected"]
        elt = [r.lib.VECTOR_ELT(out, k) for k in range(7)]
        assert [r.lib.TYPEOF(e) for e in elt] == [14, 14, 14, 13, 10, 13, 13]
        assert r.dim(elt[0]) == (n, K) and r.dim(elt[1]) == (m, K) and [r.lib.XLENGTH(e) for e in elt[2:]] == [1] * 5
        assert np.array_equal(_bits(r.as_numpy(elt[0], (n, K))), _bits(want["Q"]))
        assert np.array_equal(_bits(r.as_numpy(elt[1], (m, K))), _bits(want["P"]))
        assert r.as_numpy(elt[2])[0] == want["loglik"] and int(r.as_numpy(elt[3])[0]) == want["n_iter"]
        assert bool(r.as_numpy(elt[4])[0]) == want["converged"]
        assert int(r.as_numpy(elt[5])[0]) == want["n_cycles"] and int(r.as_numpy(elt[6])[0]) == want["n_rejected"]

    # a seeded start (k as R holds it: integer or double)
    for k_sexp in (r.int([K]), r.real([float(K)])):
        out = r.call("tpg_admixture_squarem", BM, r.int(rows), r.index(cols, double=True), k_sexp, r.real([12345.0]), r.int([10]),
                     r.real([1e-4]), nil, nil)
        want = tpg.admix_em(v, K, seed=12345, max_iter=10, tol=1e-4, accel="squarem")
        assert want["n_cycles"] == 3
        check(out, want)
    # a given start
    rng = np.random.default_rng(n)
    Q0, F0 = rng.uniform(0.1, 1.0, size=(n, K)), rng.uniform(0.0, 1.0, size=(m, K))
    out = r.call("tpg_admixture_squarem", BM, r.int(rows), r.int(cols), r.int([K]), r.real([0.0]), r.int([6]), r.real([0.0]),
                 r.matrix(Q0), r.matrix(F0))
    check(out, tpg.admix_em(v, K, Q0=Q0, F0=F0, max_iter=6, tol=0.0, accel="squarem"))
    # the plain row beside it still answers the plain EM
    out = r.call("tpg_admixture", BM, r.int(rows), r.int(cols), r.int([K]), r.real([0.0]), r.int([6]), r.real([0.0]), r.matrix(Q0),
                 r.matrix(F0))
    assert r.names(out) == ["Q", "P", "loglik", "n_iter", "converged"]
    assert np.array_equal(_bits(r.list_elt(out, 0, (n, K))), _bits(tpg.admix_em(v, K, Q0=Q0, F0=F0, max_iter=6, tol=0.0)["Q"]))
    assert r.depth() == depth
    assert np.array_equal(np.frombuffer(path.read_bytes(), dtype=np.uint8), codes.ravel(order="F"))


@pytest.mark.parametrize("n,m,K", [(13, 300, 3), (65, 140, 8)])
def test_cv_entry_equals_the_python_route(r, tmp_path, n, m, K):
    import tidypopgen_amd as tpg

    codes, path, BM, rows, cols, v = _panel(r, tmp_path, n, m, K)
    nil = r.lib.rmock_nil()
    depth = r.depth()

    def check(out, want, folds):
        assert r.lib.TYPEOF(out) == 19
        assert r.names(out) == ["cv_error", "fold_deviance", "fold_count", "fold_n_iter", "fold_converged"]
        elt = [r.lib.VECTOR_ELT(out, k) for k in range(5)]
        assert [r.lib.TYPEOF(e) for e in elt] == [14, 14, 14, 13, 10]
        assert [r.lib.XLENGTH(e) for e in elt] == [1, folds, folds, folds, folds]
        assert _bits(r.as_numpy(elt[0]))[0] == _bits(want["cv_error"])[0]
        assert np.array_equal(_bits(r.as_numpy(elt[1])), _bits(want["fold_deviance"]))
        assert np.array_equal(r.as_numpy(elt[2]), want["fold_count"].astype(np.float64))
        assert np.array_equal(r.as_numpy(elt[3]), want["fold_n_iter"])
        assert np.array_equal(r.as_numpy(elt[4]).astype(bool), want["fold_converged"])

    for k_sexp, f_sexp in ((r.int([K]), r.int([3])), (r.real([float(K)]), r.real([3.0]))):
        out = _call_cv(r, BM, r.int(rows), r.index(cols, double=True), k_sexp, r.real([12345.0]), r.int([7]), r.real([1e-4]), nil, nil,
                       f_sexp, r.real([77.0]))
        want = tpg.admix_cv(v, K, folds=3, cv_seed=77, seed=12345, max_iter=7, tol=1e-4, accel="squarem")
        check(out, want, 3)
    plain = tpg.admix_cv(v, K, folds=3, cv_seed=77, seed=12345, max_iter=7, tol=1e-4)
    assert _bits(plain["cv_error"])[0] != _bits(want["cv_error"])[0]  # (the accelerated refits are not the plain ones)
    rng = np.random.default_rng(n)
    Q0, F0 = rng.uniform(0.1, 1.0, size=(n, K)), rng.uniform(0.0, 1.0, size=(m, K))
    out = _call_cv(r, BM, r.int(rows), r.int(cols), r.int([K]), r.real([0.0]), r.int([6]), r.real([0.0]), r.matrix(Q0), r.matrix(F0),
                   r.int([5]), r.real([0.0]))
    check(out, tpg.admix_cv(v, K, folds=5, cv_seed=0, Q0=Q0, F0=F0, max_iter=6, tol=0.0, accel="squarem"), 5)
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
    k, seed, mi, tol, folds, cvs = r.int([K]), r.real([1.0]), r.int([4]), r.real([1e-4]), r.int([3]), r.real([5.0])
    depth = r.depth()
    q = np.ones(n * K)
    q[3] = 0.0
    bad = [("k must be a positive integer", (r.int([0]), seed, mi, tol, nil, nil)), ("K = 33", (r.int([33]), seed, mi, tol, nil, nil)),
           ("seed must be a double vector of length 1", (k, r.int([1]), mi, tol, nil, nil)),
           ("whole number", (k, r.real([-1.0]), mi, tol, nil, nil)), ("max_iter must be", (k, seed, r.int([-1]), tol, nil, nil)),
           ("tol must be", (k, seed, mi, r.real([-1.0]), nil, nil)), ("q0 must be", (k, seed, mi, tol, r.real(np.ones(n * K - 1)), nil)),
           ("p0 must be", (k, seed, mi, tol, nil, r.real(np.ones(m * K + 1)))),
           ("not finite or not positive", (k, seed, mi, tol, r.real(q), nil))]
    for match, args in bad:
        with pytest.raises(RuntimeError, match=match):
            r.call("tpg_admixture_squarem", BM, rows, cols, *args)
        with pytest.raises(RuntimeError, match=match):
            _call_cv(r, BM, rows, cols, *args, folds, cvs)
    for nf in (1, 65, 0):
        with pytest.raises(RuntimeError, match=r"folds must be an integer in \[2, 64\]"):
            _call_cv(r, BM, rows, cols, k, seed, mi, tol, nil, nil, r.int([nf]), cvs)
    with pytest.raises(RuntimeError, match="cv_seed must be a whole number"):
        _call_cv(r, BM, rows, cols, k, seed, mi, tol, nil, nil, folds, r.real([0.5]))
    assert r.depth() == depth
    out = _call_cv(r, BM, rows, cols, k, seed, mi, tol, nil, nil, folds, cvs)  # all good: the same call succeeds
    assert r.as_numpy(r.lib.VECTOR_ELT(out, 0))[0] > 0
    out = r.call("tpg_admixture_squarem", BM, rows, cols, k, seed, mi, tol, nil, nil)
    assert int(r.list_elt(out, 3)[0]) == 4 and int(r.list_elt(out, 5)[0]) == 1
    assert r.depth() == depth
