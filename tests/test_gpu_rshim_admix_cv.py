"""GPU: the R entry point of admixture cross-validation, `.Call("_tidypopgen_tpg_admixture_cv", BM, rowInd, colInd, k, seed, max_iter,
tol, q0, p0, folds, cv_seed)` of shim/tpg_rshim.c (tpg_rshim_entries_admix_cv[]), through the strict R mock: equal to the Python
route bit for bit for a seeded start and for a given q0 / p0, list names, types and lengths as INTEGRATION.md states them, protect
stack balanced, backing file untouched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import admix_ref as ar
from tests import rmock

pytestmark = pytest.mark.gpu

CODE_012 = np.r_[0.0, 1.0, 2.0, np.full(253, np.nan)]
NAME = "_tidypopgen_tpg_admixture_cv"


def _cv_entries(lib):
    tab = (rmock.Entry * 2).in_dll(lib, "tpg_rshim_entries_admix_cv")
    out = {}
    for e in tab:
        if not e.name:
            break
        out[e.name.decode()] = (e.fun, e.numArgs)
    return out


def _build(out_dir):
    """rmock.build with tests/rmock/call11.c beside the mock runtime: the trampoline for an entry point of 11 arguments"""
    out = os.path.join(str(out_dir), "libtpgshim_mock11.so")
    libdir = os.path.join(rmock.ROOT, "tidypopgen_amd")
    cmd = ["gcc", *rmock.CFLAGS, "-shared", "-fPIC", "-I" + rmock.HERE, "-I" + os.path.join(rmock.ROOT, "include"),
           os.path.join(rmock.ROOT, "shim", "tpg_rshim.c"), os.path.join(rmock.HERE, "rmock.c"), os.path.join(rmock.HERE, "call11.c"),
           "-o", out, "-lm", "-L" + libdir, "-ltpg_hip", "-Wl,-rpath," + libdir]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(res.stderr)
    lib = rmock.bind(C.CDLL(out))
    lib.rmock_call11_set.restype, lib.rmock_call11_set.argtypes = None, [C.c_void_p, C.c_void_p]
    return lib


def _call(r, *args):
    """r.call for the 11 arguments of the entry: the first ten through rmock_call_named (protect depth, GC torture, strict
    arguments), the last parked in the trampoline and held to the strict rule here"""
    fn, arity = r.ent[NAME]
    assert arity == len(args) == 11
    last = args[10]
    before = (r.lib.TYPEOF(last), r.as_numpy(last).tobytes())
    r.lib.rmock_call11_set(fn, last)
    arr = (C.c_void_p * 10)(*args[:10])
    out = r.lib.rmock_call_named(b"tpg_admixture_cv", C.cast(r.lib.rmock_call11_trampoline, C.c_void_p), 10, arr)
    assert (r.lib.TYPEOF(last), r.as_numpy(last).tobytes()) == before
    if out is None:
        raise RuntimeError(r.lib.rmock_last_error().decode())
    return out


@pytest.fixture(scope="module")
def r(tmp_path_factory):
    lib = _build(tmp_path_factory.mktemp("rshim_admix_cv"))
    lib.rmock_gctorture(1)
    lib.rmock_strict(1)
    s = rmock.Session(lib)
    s.ent = {**s.ent, **_cv_entries(lib)}
    yield s
    lib.rmock_gctorture(0)
    lib.rmock_strict(0)
    lib.R_unload_tpgshim(None)
    lib.rmock_reset()


def test_table_rows_and_arity(r):
    import os
    import re

    ent = _cv_entries(r.lib)
    assert {k: v[1] for k, v in ent.items()} == {NAME: 11}
    assert not set(ent) & set(rmock.entries(r.lib))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "shim", "tpg_rshim.c")).read()
    tabs = set(re.findall(r"const R_CallMethodDef (tpg_rshim_entries\w*)\[\]", src))
    assert {"tpg_rshim_entries_admix", "tpg_rshim_entries_admix_cv"} <= tabs
    for tab in tabs:
        assert f"e = {tab};" in src, tab  # registered in the stand-alone concatenation
    for tab in tabs - {"tpg_rshim_entries_admix_cv"}:
        row = rmock.C.cast(rmock.C.addressof(rmock.Entry.in_dll(r.lib, tab)), rmock.C.POINTER(rmock.Entry))
        k = 0
        while row[k].name:
            assert row[k].name.decode() not in ent, tab
            k += 1
    ns = open(os.path.join(root, "shim", "tpgshim", "NAMESPACE")).read()
    rsrc = open(os.path.join(root, "shim", "tpgshim", "R", "tpgshim.R")).read()
    assert "export(gt_admixture_gpu)" in ns and f"`{NAME}`" in rsrc
    assert "crossval = FALSE, cv_folds = 5L, cv_seed = 0) {" in rsrc[rsrc.index("gt_admixture_gpu <- function("):]
    assert "adm_list$cv <- cvres$cv_error" in rsrc


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

    # a seeded start (k and folds as R holds them: integer or double)
    for k_sexp, f_sexp in ((r.int([K]), r.int([3])), (r.real([float(K)]), r.real([3.0]))):
        out = _call(r, BM, r.int(rows), r.index(cols, double=True), k_sexp, r.real([12345.0]), r.int([4]),
                     r.real([1e-4]), nil, nil, f_sexp, r.real([77.0]))
        check(out, tpg.admix_cv(v, K, folds=3, cv_seed=77, seed=12345, max_iter=4, tol=1e-4), 3)
    # a given start
    rng = np.random.default_rng(n)
    Q0, F0 = rng.uniform(0.1, 1.0, size=(n, K)), rng.uniform(0.0, 1.0, size=(m, K))
    out = _call(r, BM, r.int(rows), r.int(cols), r.int([K]), r.real([0.0]), r.int([3]), r.real([0.0]),
                 r.matrix(Q0), r.matrix(F0), r.int([5]), r.real([0.0]))
    check(out, tpg.admix_cv(v, K, folds=5, cv_seed=0, Q0=Q0, F0=F0, max_iter=3, tol=0.0), 5)
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
    k, seed, mi, tol, folds, cvs = r.int([K]), r.real([1.0]), r.int([2]), r.real([1e-4]), r.int([3]), r.real([5.0])
    depth = r.depth()

    def call(*args):
        return _call(r, BM, rows, cols, *args)

    with pytest.raises(RuntimeError, match="k must be a positive integer"):
        call(r.int([0]), seed, mi, tol, nil, nil, folds, cvs)
    with pytest.raises(RuntimeError, match="K = 33"):
        call(r.int([33]), seed, mi, tol, nil, nil, folds, cvs)
    with pytest.raises(RuntimeError, match="seed must be a double vector of length 1"):
        call(k, r.int([1]), mi, tol, nil, nil, folds, cvs)
    with pytest.raises(RuntimeError, match="whole number"):
        call(k, r.real([-1.0]), mi, tol, nil, nil, folds, cvs)
    with pytest.raises(RuntimeError, match="max_iter must be"):
        call(k, seed, r.int([-1]), tol, nil, nil, folds, cvs)
    with pytest.raises(RuntimeError, match="tol must be"):
        call(k, seed, mi, r.real([-1.0]), nil, nil, folds, cvs)
    with pytest.raises(RuntimeError, match="q0 must be"):
        call(k, seed, mi, tol, r.real(np.ones(n * K - 1)), nil, folds, cvs)
    with pytest.raises(RuntimeError, match="p0 must be"):
        call(k, seed, mi, tol, nil, r.real(np.ones(m * K + 1)), folds, cvs)
    q = np.ones(n * K)
    q[3] = 0.0
    with pytest.raises(RuntimeError, match="not finite or not positive"):
        call(k, seed, mi, tol, r.real(q), nil, folds, cvs)
    for bad in (1, 65, 0):
        with pytest.raises(RuntimeError, match=r"folds must be an integer in \[2, 64\]"):
            call(k, seed, mi, tol, nil, nil, r.int([bad]), cvs)
    with pytest.raises(RuntimeError, match="cv_seed must be a double vector of length 1"):
        call(k, seed, mi, tol, nil, nil, folds, r.int([1]))
    with pytest.raises(RuntimeError, match="cv_seed must be a whole number"):
        call(k, seed, mi, tol, nil, nil, folds, r.real([0.5]))
    assert r.depth() == depth
    out = call(k, seed, mi, tol, nil, nil, folds, cvs)  # all good: the same call succeeds
    assert r.as_numpy(r.lib.VECTOR_ELT(out, 0))[0] > 0
    assert r.depth() == depth
