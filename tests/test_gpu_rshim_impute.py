"""GPU: the R entry point of simple imputation, `.Call("_tidypopgen_tpg_impute_simple", BM, method, seed)` of shim/tpg_rshim.c,
through the strict R mock: the backing file's bytes afterwards are what tests/impute_ref.py says, a second call is the
reference's R error and leaves the file alone, the protect stack is balanced.  The entry point rewrites the backing file, so
it is registered in a table of its own, tpg_rshim_entries_write[] (tpg_rshim_entries[] holds what leaves the FBM alone)."""
import ctypes as C

import numpy as np
import pytest

from tests import impute_ref as ir
from tests import rmock

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r(tmp_path_factory):
    lib = rmock.build(tmp_path_factory.mktemp("rshim_impute"))
    lib.rmock_gctorture(1)
    lib.rmock_strict(1)
    yield WriteSession(lib)
    lib.rmock_gctorture(0)
    lib.rmock_strict(0)
    lib.R_unload_tpgshim(None)
    lib.rmock_reset()


def _write_entries(lib):
    """tpg_rshim_entries_write[]: {name: (function pointer, arity)}"""
    tab = (rmock.Entry * 8).in_dll(lib, "tpg_rshim_entries_write")
    out = {}
    for e in tab:
        if not e.name:
            break
        out[e.name.decode()] = (e.fun, e.numArgs)
    return out


class WriteSession(rmock.Session):
    """a Session whose call() also finds the entry points of the write table"""

    def __init__(self, lib):
        super().__init__(lib)
        self.ent = {**self.ent, **_write_entries(lib)}


def test_write_table(r):
    w = _write_entries(r.lib)
    assert w == {"_tidypopgen_tpg_impute_simple": (w["_tidypopgen_tpg_impute_simple"][0], 3)}
    assert w["_tidypopgen_tpg_impute_simple"][0]
    assert not set(w) & set(rmock.entries(r.lib))  # a name is registered once: R_init_tpgshim lays the tables end to end
    fn = C.cast(r.lib._tidypopgen_tpg_impute_simple, C.c_void_p).value
    assert w["_tidypopgen_tpg_impute_simple"][0] == fn


def _raw(n, m, seed):
    rng = np.random.default_rng(seed)
    g = rng.binomial(2, rng.random(m)[None, :], size=(n, m)).astype(np.uint8)
    rate = rng.choice([0.0, 0.02, 0.5, 1.0], size=m)
    g[rng.random((n, m)) < rate[None, :]] = 3
    return np.asfortranarray(g)


@pytest.mark.parametrize("method", [1, 2, 3])
@pytest.mark.parametrize("n,m", [(7, 6), (65, 129), (301, 2051)])
def test_raw_matrix_in_imputed_bytes_out(r, tmp_path, n, m, method):
    raw = _raw(n, m, 100 * n + method)
    path = tmp_path / "geno.bk"
    path.write_bytes(raw.tobytes(order="F"))
    BM = r.fbm(path, n, m, np.r_[0.0, 1.0, 2.0, np.full(253, np.nan)])
    depth = r.lib.rmock_protect_depth()
    out = r.as_numpy(r.call("tpg_impute_simple", BM, r.int([method]), r.real([12345.0])))
    assert r.lib.rmock_protect_depth() == depth
    name = ir.METHODS[method - 1]
    got = np.frombuffer(path.read_bytes(), dtype=np.uint8).reshape((n, m), order="F")
    assert np.array_equal(got, ir.store_bytes(raw, name, 12345))
    rep = ir.report(raw)
    assert out.tolist() == [float(rep["imputed"]), float(rep["loci_all_missing"])]
    # a second call: the reference's error, the file as it was
    with pytest.raises(RuntimeError, match="object x is already imputed"):
        r.call("tpg_impute_simple", BM, r.int([method]), r.real([12345.0]))
    assert r.lib.rmock_protect_depth() == depth
    again = np.frombuffer(path.read_bytes(), dtype=np.uint8).reshape((n, m), order="F")
    assert np.array_equal(again, got)


def test_bad_arguments_are_r_errors(r, tmp_path):
    raw = _raw(20, 30, 1)
    path = tmp_path / "g.bk"
    path.write_bytes(raw.tobytes(order="F"))
    BM = r.fbm(path, 20, 30)
    with pytest.raises(RuntimeError, match="impute method"):
        r.call("tpg_impute_simple", BM, r.int([4]), r.real([0.0]))
    with pytest.raises(RuntimeError, match="seed"):
        r.call("tpg_impute_simple", BM, r.int([1]), r.real([-1.0]))
    assert np.array_equal(np.frombuffer(path.read_bytes(), dtype=np.uint8), raw.ravel(order="F"))
