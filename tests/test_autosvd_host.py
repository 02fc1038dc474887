"""CPU-only: the definition of include/tpg.h "autoSVD" as tests/autosvd_ref.py restates it -- the medcouple over ratios against
the classical kernel, the normal quantile and the weights against an independent route, the finder of outlier runs, the planted
panel -- and the host pieces of the library (csrc/host/host_autosvd.h) as a stand-alone program under the host sanitizers.

Tolerances.  Medcouple: the ratio form and the classical (a - b) / (a + b) form round differently (one division against a
sum, a difference and a division), each within a few ulp of a value in [-1, 1]: 4 ulp of 1.  qnorm_upper and the weights against
statistics.NormalDist().inv_cdf: 1e-12 relative; both sit a few ulp from the true value (the tail's relative slope is the
hazard phi(x) / p >= 1 / x-ish for x >= 0.67, so an ulp of p moves x by less than an ulp of x times p / (x phi(x)) <= 1.5)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import autosvd_ref as ar
from tests import ld_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP1 = 2.0 ** -52


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def _contents():
    rng = np.random.default_rng(11)
    return {
        "normal": rng.standard_normal(101),
        "normal_even": rng.standard_normal(64),
        "exponential": rng.exponential(size=97),
        "small_integers": rng.integers(0, 4, 80).astype(np.float64),
        "ties_at_median": np.r_[np.zeros(9), rng.standard_normal(20)],
        "all_equal": np.full(13, 2.5),
    }


@pytest.mark.parametrize("kind", sorted(_contents()))
def test_ratio_medcouple_is_the_classical_one(kind):
    x = _contents()[kind]
    brute, classical, bisect = ar.medcouple_brute(x), ar.medcouple_classical(x), ar.medcouple_bisect(x)
    assert abs(brute - classical) <= 4 * ULP1, (brute, classical)
    assert _same(brute, bisect), (brute, bisect)


@pytest.mark.parametrize("c", [1, 2, 3, 4, 5])
def test_ratio_medcouple_on_tiny_counts(c):
    rng = np.random.default_rng(c)
    for x in (rng.standard_normal(c), rng.integers(0, 3, c).astype(np.float64), np.arange(c, dtype=np.float64)):
        brute, classical, bisect = ar.medcouple_brute(x), ar.medcouple_classical(x), ar.medcouple_bisect(x)
        assert abs(brute - classical) <= 4 * ULP1, (x, brute, classical)
        assert _same(brute, bisect), (x, brute, bisect)
    assert math.isnan(ar.medcouple_brute([])) and math.isnan(ar.medcouple_bisect([np.nan, np.inf]))


def test_medcouple_sees_skewness():
    rng = np.random.default_rng(3)
    assert ar.medcouple_brute(rng.exponential(size=400)) > 0.2
    assert abs(ar.medcouple_brute(rng.standard_normal(400))) < 0.15
    x = rng.exponential(size=300)
    assert _same(ar.medcouple_brute(-x), -ar.medcouple_brute(x)) or abs(ar.medcouple_brute(-x) + ar.medcouple_brute(x)) <= 4 * ULP1


QNORM_P = (0.25, 0.5, 0.75, 0.025, 1e-3, 2.5e-5, 1e-10)


def test_qnorm_and_weights_agree_with_the_independent_route():
    for p in QNORM_P:
        a, b = ar.qnorm_upper(p), ar.qnorm_upper_indep(p)
        assert abs(a - b) <= 1e-12 * max(abs(b), 1e-300) or (p == 0.5 and abs(a) <= 1e-15), (p, a, b)
    for radius in (1, 4, 5, 50):
        w, wi = ar.weights(radius), ar.weights(radius, qnorm=ar.qnorm_upper_indep)
        assert len(w) == 2 * radius + 1 and np.allclose(w, w[::-1], rtol=1e-13, atol=0) and np.argmax(w) == radius
        assert np.all(np.abs(w - wi) <= 1e-12 * wi)
    assert np.array_equal(ar.weights(0), [1.0])
    # Tukey's 1.5 at the tail probability of its fence: (qnorm_upper(p) - z75) / (2 z75) = 1.5 <=> qnorm_upper(p) = 4 z75
    z75 = ar.qnorm_upper(0.25)
    assert abs((ar.qnorm_upper(ar.pnorm_upper(4 * z75)) - z75) / (2 * z75) - 1.5) <= 1e-12


def test_library_qnorm_and_weights_are_the_restatement():
    from tidypopgen_amd import _lib

    lib = _lib.lib
    for p in QNORM_P + (1e-100, 1e-300, 0.999):
        out = C.c_double()
        assert lib.tpg_qnorm_upper(p, C.byref(out)) == 0
        assert abs(out.value - ar.qnorm_upper(p)) <= 4 * ULP1 * abs(out.value), p  # (the two libm erfc may differ by an ulp)
    assert lib.tpg_qnorm_upper(0.0, C.byref(C.c_double())) != 0 and lib.tpg_qnorm_upper(1.0, C.byref(C.c_double())) != 0
    assert lib.tpg_qnorm_upper(0.5, None) != 0
    for radius in (0, 1, 4, 5, 50):
        w = np.zeros(2 * radius + 1)
        assert lib.tpg_rollmean_weights(radius, w.ctypes.data_as(C.c_void_p)) == 0
        assert np.all(np.abs(w - ar.weights(radius)) <= 1e-13 * w)
    assert lib.tpg_rollmean_weights(-1, np.zeros(1).ctypes.data_as(C.c_void_p)) != 0
    assert lib.tpg_rollmean_weights(1025, np.zeros(2051).ctypes.data_as(C.c_void_p)) != 0


def test_rollmean_loops_and_their_fast_form_agree():
    rng = np.random.default_rng(4)
    x = rng.exponential(size=70)
    seg = np.array([0, 11, 23, 70])
    for radius in (0, 1, 4, 5):
        assert np.array_equal(ar.rollmean(x, seg, radius), ar.rollmean_fast(x, seg, radius))
    with pytest.raises(ValueError, match="roll_size exceeds"):
        ar.rollmean(x, seg, 6)
    flat = ar.rollmean(np.full(30, 3.0), np.array([0, 30]), 4)
    assert np.all(np.abs(flat - 3.0) <= 4 * ULP1 * 3.0)


def test_outlier_runs_on_hand_made_lists():
    ms = 4  # int_min_size
    pos = [2, 3, 4, 10, 11, 12, 13, 20, 21, 22, 23, 24, 40]
    ch = [1] * 13
    assert ar.outlier_runs(pos, ch, ms) == [(3, 6), (7, 11)]  # the run of ms - 1 is left out, the run of exactly ms is in
    assert ar.outlier_runs(pos, ch, 1) == [(0, 2), (3, 6), (7, 11), (12, 12)]
    # a run cut by a chromosome boundary: 5 consecutive positions, 3 + 2
    pos, ch = [7, 8, 9, 10, 11], [1, 1, 1, 2, 2]
    assert ar.outlier_runs(pos, ch, 3) == [(0, 2)] and ar.outlier_runs(pos, ch, 2) == [(0, 2), (3, 4)]
    assert ar.outlier_runs(pos, [1] * 5, 5) == [(0, 4)] and ar.outlier_runs([], [], 1) == []


def test_definition_removes_the_planted_block():
    G, hi, r = ar.planted_reference()
    margin = ar.check_planted_reference(G, r)
    assert margin >= 1e-2  # 1.5e-2 at generator seed 1
    assert not np.isin(ar.LOW_MAC, r["kept"]).any()
    assert len(r["history"][0]["runs"]) == 1 and r["history"][0]["runs"][0][0] <= ar.BLOCK[0] and r["history"][0]["runs"][0][1] >= ar.BLOCK[-1]


def _build_san(tmp_path):
    exe = str(tmp_path / "autosvd_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "autosvd_san.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _f(hexbits):
    return float(np.uint64(int(hexbits, 16)).view(np.float64))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_host_pieces_stand_alone_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build_san(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines[-1] == "ok autosvd", r.stdout[-2000:] + r.stderr[-4000:]
    rows = [ln.split() for ln in lines[:-1]]
    q = {_f(p): _f(x) for tag, p, x in (row for row in rows if row[0] == "qnorm")}
    assert len(q) == 10
    for p, x in q.items():
        assert abs(x - ar.qnorm_upper(p)) <= 4 * ULP1 * abs(x), p
        if p >= 1e-10:
            assert abs(x - ar.qnorm_upper_indep(p)) <= 1e-12 * abs(x) or p == 0.5, p
    for radius in (0, 1, 4, 5, 50, 1024):
        w = np.array([_f(v) for tag, rr, i, v in (row for row in rows if row[0] == "w") if int(rr) == radius])
        assert len(w) == 2 * radius + 1 and np.all(np.abs(w - ar.weights(radius)) <= 1e-13 * w)
    ties = [(int(k), int(nb), int(c, 16), int(v)) for tag, k, nb, c, v in (row for row in rows if row[0] == "tie")]
    assert len(ties) == 5 * 3 * 6
    for k, nb, c, v in ties:
        assert v == ar.tie_count(k, nb, c), (k, nb, c)
    z75 = ar.qnorm_upper(0.25)
    coef = (ar.qnorm_upper(0.05 / 2000.0) - z75) / (2.0 * z75)
    fences = [(_f(a), _f(b)) for tag, a, b in (row for row in rows if row[0] == "fence")]
    for (cf, thr), mc in zip(fences, (0.1, -0.1)):
        want = 2.0 + coef * (2.0 - 1.0) * (math.exp(3.0 * mc) if mc >= 0 else math.exp(4.0 * mc))
        assert abs(cf - coef) <= 1e-13 * coef and abs(thr - want) <= 1e-13 * want
    pos, ch = [3, 4, 5, 9, 10, 11, 12, 18, 19, 20, 21, 30], [1] * 9 + [2] * 3
    for ms in (1, 2, 3, 4, 5):
        got = [(int(a), int(b)) for tag, s, a, b in (row for row in rows if row[0] == "run") if int(s) == ms]
        assert got == ar.outlier_runs(pos, ch, ms), ms
