"""CPU: the restatement tests/admix_squarem_ref.py of include/tpg.h "admixture, accelerated" against itself, and the host-only
state machine of the library (tidypopgen_amd/csrc/host/host_squarem.h) as a stand-alone program under the host sanitizers.

The float route of the two sums is held against the exact Fraction sums within the bounds of the header, |d sr| <= (nn + 3) u sr
and |d sv| <= 2 sum |v| |dv| + (nn + 3) u sv.  Over whole runs of the restated driver the likelihoods at the starts of the cycles
do not decrease beyond the rounding bound of the likelihood, and a rejected cycle continues from theta2."""
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import admix_ref as ar
from tests import admix_squarem_ref as sq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _three_states(seed, n, m, K, miss):
    codes = ar.panel(seed, n, m, K, miss)[0]
    Q0, F0 = ar.start(seed, n, m, K)
    Q1, F1, _ = ar.em_step(codes, Q0, F0)
    Q2, F2, _ = ar.em_step(codes, Q1, F1)
    return codes, (Q0, F0, Q1, F1, Q2, F2)


@pytest.mark.parametrize("update_q,update_f", [(True, True), (True, False), (False, True)])
def test_float_sums_within_the_bounds_of_the_exact_sums(update_q, update_f):
    n, m, K = 13, 31, 3
    _, th = _three_states(21, n, m, K, 0.1)
    sr, sv, nn = sq.sums(*th, update_q, update_f)
    assert nn == (n * K if update_q else 0) + (m * K if update_f else 0)
    xr, xv = sq.sums_exact(*th, update_q, update_f)
    # the exact sums are over the unrounded differences of the given doubles
    dr, dv = abs(float(Fraction(sr) - xr)), abs(float(Fraction(sv) - xv))
    print("sums", update_q, update_f, sr, dr, sq.bound_sr(nn, xr), sv, dv, sq.bound_sv(*th, xv, update_q, update_f))
    assert sr > 0 and sv > 0
    assert dr <= sq.bound_sr(nn, xr)
    assert dv <= sq.bound_sv(*th, xv, update_q, update_f)


def test_exact_fma_rounds_once():
    # products that a multiply-then-add rounds twice: (1 + 2^-30)^2 - 1 keeps its 2^-60 term only when fused
    a = np.array([1.0 + 2.0 ** -30, 3.0, 0.1])
    c = np.array([-1.0, 0.5, -0.01])
    got = sq.fma_exact(a, a, c)
    assert got[0] == 2.0 ** -29 + 2.0 ** -60 and got[0] != a[0] * a[0] + c[0]
    assert got[1] == 9.5 and got[2] == float(Fraction(0.1) ** 2 + Fraction(-0.01))


def test_alpha_clip_limit_and_accept_rules():
    assert sq.alpha_of(9.0, 1.0, 4.0) == (-3.0, False) and sq.alpha_of(100.0, 1.0, 4.0) == (-4.0, True)
    assert sq.alpha_of(16.0, 1.0, 4.0) == (-4.0, False) and sq.alpha_of(1.0, 4.0, 4.0) == (-1.0, False)
    for sr, sv in ((1.0, 0.0), (0.0, 0.0), (np.inf, 1.0), (np.nan, 1.0), (1.0, np.nan)):
        assert sq.alpha_of(sr, sv, 4.0) == (-1.0, False)
    assert sq.accept(-1.0, -1.0) and not sq.accept(np.nan, -1.0) and not sq.accept(-2.0, -1.0) and not sq.accept(-np.inf, -1.0)
    assert sq.next_limit(4.0, True, True) == 16.0 and sq.next_limit(4.0, True, False) == 4.0
    assert sq.next_limit(4.0, False, True) == 1.0 and sq.next_limit(1.0, False, False) == 1.0 and sq.next_limit(64.0, False, False) == 16.0


def test_projection_is_feasible_and_keeps_rows_that_did_not_move():
    n, m, K = 13, 31, 3
    codes, th = _three_states(21, n, m, K, 0.1)
    Q0, F0, Q1, F1, Q2, F2 = th
    # theta2 - theta1 = 0.98 r with a wide limit: v = -0.02 r, alpha near -50, theta' raw near theta0 + 50 r leaves the feasible set
    p = sq.point(Q0, F0, Q1, F1, Q1 + 0.98 * (Q1 - Q0), F1 + 0.98 * (F1 - F0), a_max=64.0)
    assert -51.0 < p["alpha"] < -49.0
    assert (p["Q_raw"] < 0).any() and ((p["P_raw"] < 0) | (p["P_raw"] > 1)).any()
    assert (p["P"] >= ar.EPS).all() and (p["P"] <= 1 - ar.EPS).all() and (p["Q"] > 0).all()
    row_missing, col_missing = n - 1, 0  # planted by ar.panel
    moved = np.ones(n, dtype=bool)
    moved[row_missing] = False
    assert np.allclose(p["Q"][moved].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert np.array_equal(p["Q"][row_missing], Q0[row_missing]) and np.array_equal(p["P"][col_missing], F0[col_missing])


def test_whole_runs_cycle_starts_do_not_decrease_and_a_rejected_cycle_continues_from_theta2():
    n, m, K = 65, 600, 2
    codes = ar.panel(3, n, m, K, 0.05)[0]
    Q0, F0 = ar.start(3, n, m, K)
    T = int((codes != ar.MISSING).sum())
    plain = sq.em_plain(codes, Q0, F0, tol=1e-4, max_iter=3000)
    acc = sq.em_squarem(codes, Q0, F0, tol=1e-4, max_iter=3000)
    print("plain", plain["n_iter"], plain["loglik"], "accelerated", acc["n_iter"], acc["loglik"], "cycles", acc["n_cycles"],
          "rejected", acc["n_rejected"], "min alpha", acc["alpha"].min(), "gap", plain["loglik"] - acc["loglik"])
    assert plain["converged"] and acc["converged"]
    assert acc["n_iter"] <= 0.5 * plain["n_iter"]
    assert len(acc["trace"]) == acc["n_iter"] + 1 and acc["n_cycles"] == len(acc["cycles"]) and acc["n_rejected"] > 0
    tr = acc["trace"]
    starts = [c["start"] for c in acc["cycles"]]
    assert starts == list(range(0, 3 * acc["n_cycles"], 3))
    for a, b in zip(starts, starts[1:]):
        assert tr[b] >= tr[a] - ar.bound_ll(T, K, tr[a])
    for c, ok in zip(acc["cycles"], acc["accepted"]):
        assert ok == (tr[c["start"] + 2] >= tr[c["start"] + 1])
        if not ok:
            assert c["next"][0] is c["theta2"][0] and c["next"][1] is c["theta2"][1]
    # max_iter inside a cycle: the last state a step produced; at its end: the next start
    for mi in (1, 2, 3, 4, 5):
        s = sq.em_squarem(codes, Q0, F0, tol=0.0, max_iter=mi)
        assert s["n_iter"] == mi and len(s["trace"]) == mi + 1 and s["n_cycles"] == mi // 3


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_state_machine_stand_alone_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "squarem_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc"), os.path.join(ROOT, "tests", "host", "squarem_san.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.split("\n")
    assert "ok squarem" in lines and "FAILED" not in r.stdout
    for want in ("alpha ok", "accept ok", "limit ok", "sv = 0 ok", "NaN ok", "growth ok", "shrink ok", "stop rule ok",
                 *(f"max_iter {k} ok" for k in range(1, 7))):
        assert want in lines, want


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no host compiler")
def test_shim_rows_report_a_library_without_the_accelerated_symbols(tmp_path):
    """the shim linked against the host-only stand-in of the library (tests/host/tpg_stub.c), which has neither symbol: the weak
    references are null, and each of the two rows is an R error that names what is missing, before any argument is looked at"""
    import ctypes as C

    from tests import rmock

    so = str(tmp_path / "libshim_stub.so")
    cmd = ["gcc", *rmock.CFLAGS, "-Wno-unknown-pragmas", "-shared", "-fPIC", "-I" + rmock.HERE, "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "shim", "tpg_rshim.c"), os.path.join(rmock.HERE, "rmock.c"), os.path.join(rmock.HERE, "call11.c"),
           os.path.join(ROOT, "tests", "host", "tpg_stub.c"), os.path.join(ROOT, "oracle", "tpg_oracle.c"), "-o", so, "-lm"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    lib = rmock.bind(C.CDLL(so))
    lib.rmock_call11_set.restype, lib.rmock_call11_set.argtypes = None, [C.c_void_p, C.c_void_p]
    nil = lib.rmock_nil()
    for table, name, arity, sym in (("tpg_rshim_entries_admix_squarem", "_tidypopgen_tpg_admixture_squarem", 9, "tpg_admix_em_squarem"),
                                    ("tpg_rshim_entries_admix_cv_squarem", "_tidypopgen_tpg_admixture_cv_squarem", 11, "tpg_admix_cv_squarem")):
        row = (rmock.Entry * 2).in_dll(lib, table)
        assert row[0].name.decode() == name and row[0].numArgs == arity and not row[1].name
        arr = (C.c_void_p * 10)(*([nil] * 10))
        if arity == 11:
            lib.rmock_call11_set(row[0].fun, nil)
            out = lib.rmock_call_named(name.encode(), C.cast(lib.rmock_call11_trampoline, C.c_void_p), 10, arr)
        else:
            out = lib.rmock_call_named(name.encode(), row[0].fun, arity, arr)
        assert out is None and lib.rmock_last_error().decode() == f"tidypopgen (GPU): this libtpg_hip has no {sym}"
    assert lib.rmock_protect_depth() == 0
    lib.rmock_reset()


def test_header_and_binding_name_the_accelerated_block():
    from tidypopgen_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "tpg.h")).read()
    at = hdr.index("---- admixture, accelerated")
    assert hdr.index("---- admixture cross-validation") < at < hdr.index("---- sNMF")
    block = hdr[at:hdr.index("---- sNMF")]
    assert "Varadhan and Roland 2008" in block and "RECALLED, NOT" in block and "(nn + 3) u sr" in block
    for name in ("tpg_admix_em_squarem", "tpg_admix_cv_squarem", "tpg_admix_squarem_point"):
        assert re.search(r"\bint " + name + r"\(", block) and name in _lib.PROTOTYPES and hasattr(_lib.lib, name)


def test_accel_argument_errors_need_no_device():
    import tidypopgen_amd as tpg

    for fn in (lambda: tpg.admix_em(None, 2, accel="newton"), lambda: tpg.admix_cv(None, 2, accel="newton"),
               lambda: tpg.gt_admixture(None, k=[2, 3], accel="newton")):
        with pytest.raises(ValueError, match="accel must be None or 'squarem'"):
            fn()
