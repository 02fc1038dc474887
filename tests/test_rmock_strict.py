"""CPU: the rules of the mock R runtime (tests/rmock) on toy .Call functions (tests/rmock/toys.c), each of which breaks
one rule: a stack imbalance, an unprotected vector used after another allocation (GC torture), a write into an argument
(strict mode), R's coercion of c(1.9, NaN) to integer, a failing allocation.  Without these the shim's tests could pass
on a mock that accepts anything."""
import ctypes as C
import shutil

import numpy as np
import pytest

from tests import rmock

pytestmark = pytest.mark.skipif(shutil.which("gcc") is None, reason="no host compiler")

NA_INTEGER = -(2 ** 31)


@pytest.fixture(scope="module")
def toys(tmp_path_factory):
    lib = rmock.build_toys(tmp_path_factory.mktemp("toys"))
    yield lib
    lib.rmock_reset()


def _call(lib, name, *args):
    fn = C.cast(getattr(lib, name), C.c_void_p)
    arr = (C.c_void_p * max(1, len(args)))(*args)
    out = lib.rmock_call_named(name.encode(), fn, len(args), arr)
    return out, lib.rmock_last_error().decode()


def _session(lib):
    s = rmock.Session.__new__(rmock.Session)
    s.lib = lib
    return s


@pytest.mark.parametrize("torture,strict", [(0, 0), (1, 1)])
def test_a_correct_function_passes(toys, torture, strict):
    toys.rmock_gctorture(torture)
    toys.rmock_strict(strict)
    s = _session(toys)
    depth = toys.rmock_protect_depth()
    out, err = _call(toys, "toy_correct", s.real([1.5, -2.0]))
    toys.rmock_gctorture(0)
    toys.rmock_strict(0)
    assert out is not None, err
    assert s.names(out) == ["a", "b"]
    assert np.array_equal(s.list_elt(out, 0), [3.0, -4.0])
    assert s.strings(toys.VECTOR_ELT(out, 1)) == ["b"]
    assert toys.rmock_protect_depth() == depth


def test_a_forgotten_unprotect_is_a_stack_imbalance(toys):
    depth = toys.rmock_protect_depth()
    out, err = _call(toys, "toy_forget_unprotect", toys.rmock_nil())
    assert out is None and "stack imbalance in 'toy_forget_unprotect'" in err
    assert toys.rmock_protect_depth() == depth


def test_an_error_unwinds_the_protect_stack(toys):
    depth = toys.rmock_protect_depth()
    out, err = _call(toys, "toy_error_after_protect", toys.rmock_nil())
    assert out is None and err == "toy error"
    assert toys.rmock_protect_depth() == depth


def test_gc_torture_reports_an_unprotected_vector(toys):
    out, err = _call(toys, "toy_unprotected_use", toys.rmock_nil())
    assert out is not None, err  # without torture nothing is ever collected
    toys.rmock_gctorture(1)
    try:
        out, err = _call(toys, "toy_unprotected_use", toys.rmock_nil())
    finally:
        toys.rmock_gctorture(0)
    assert out is None and "use of an unprotected object" in err


def test_strict_mode_reports_a_write_into_an_argument(toys):
    s = _session(toys)
    x = s.real([1.0, 2.0])
    toys.rmock_strict(1)
    try:
        out, err = _call(toys, "toy_write_arg", x)
    finally:
        toys.rmock_strict(0)
    assert out is None and "'toy_write_arg' modified its argument 1" in err
    out, err = _call(toys, "toy_correct", x)  # reading it is fine
    assert out is not None, err


def test_coercion_follows_r(toys):
    s = _session(toys)
    out, err = _call(toys, "toy_coerce", s.real([1.9, np.nan, -1.9, rmock.na_real(), 3e9, -0.5]))
    assert out is not None, err
    assert toys.TYPEOF(out) == 13
    assert s.as_numpy(out).tolist() == [1, NA_INTEGER, -1, NA_INTEGER, NA_INTEGER, 0]
    # integer NA -> NA_real_ (R_IsNA), not any NaN
    back = C.cast(toys.Rf_coerceVector, C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_uint))(out, 14)
    v = s.as_numpy(back)
    assert rmock.is_na(v).tolist() == [False, True, False, True, True, False]
    assert toys.R_IsNA(rmock.na_real()) and not toys.R_IsNA(float("nan"))


def test_a_failing_allocation_is_an_r_error(toys):
    s = _session(toys)
    x = s.real([1.0])
    depth = toys.rmock_protect_depth()
    for k in (1, 2, 3, 4):
        toys.rmock_fail_alloc_at(k)
        out, err = _call(toys, "toy_correct", x)
        assert out is None and err.startswith("cannot allocate vector"), (k, err)
        assert toys.rmock_protect_depth() == depth
    toys.rmock_fail_alloc_at(5)  # toy_correct makes four allocations: the fifth never comes
    out, err = _call(toys, "toy_correct", x)
    assert out is not None, err
    out, err = _call(toys, "toy_correct", x)  # the mode is for one call only
    assert out is not None, err
