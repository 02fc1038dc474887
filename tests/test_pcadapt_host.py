"""CPU-only: the definition of include/tpg.h "pcadapt" as tests/pcadapt_ref.py restates it, the host pieces of the library
(chi-square median, log Q, the OGK glue) against it, and those pieces as a stand-alone program under the host sanitizers.

Tolerances.  log Q: |d| <= 1e-12 (1 + |log Q|) against logq_ref (pure math), the contract the device function is held to as
well; odd K at x >= 1500, where the erfc form underflows, against mpmath alone.  The chi-square median: 1 ulp of logq_ref's own
root for K = 1 .. 64 (both bisect the same finite sums)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import pcadapt_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- medians ----------------------------------------------------------------------------------------------------------------
def _sorted_median(xs):
    s = sorted(float(x) + 0.0 for x in xs if math.isfinite(x))
    c = len(s)
    if c == 0:
        return math.nan
    return s[(c - 1) // 2] if c % 2 else (s[c // 2 - 1] + s[c // 2]) / 2


def _sorted_mad(xs):
    f = [float(x) + 0.0 for x in xs if math.isfinite(x)]
    c0 = _sorted_median(f)
    return _sorted_median([abs(x - c0) for x in f])


EDGE_LISTS = [
    [3.0], [1.0, 2.0], [2.0, 1.0, 3.0], [4.0, 1.0, 3.0, 2.0],
    [5.0] * 7,                                            # all equal: mad = 0
    [-2.0, -1.0, 1.0, 2.0],                               # the two middle values on both sides of zero
    [1 + j * 2.0 ** -40 for j in range(9)],               # keys that share their high bytes
    [0.0, -0.0, 0.0, -0.0, -0.0],                         # +-0 mixed
    [5e-324, -5e-324, 1e-310, -1e-310, 0.0, 2e-320],      # subnormals
    [1e300, -1e300, 1e300, -1e300],
    [0.0] * 5 + [1.0, -1.0, 0.5],                         # heavy ties around the median
    [math.nan, 1.0, math.nan, 3.0, 2.0, math.inf, -math.inf],  # non-finite entries are left out
    [math.nan, math.nan],                                 # no finite entry: NaN
]


@pytest.mark.parametrize("xs", EDGE_LISTS, ids=range(len(EDGE_LISTS)))
def test_median_and_mad_are_the_sorted_definition(xs):
    a, b = pr.med(xs), _sorted_median(xs)
    assert (math.isnan(a) and math.isnan(b)) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)
    a, b = pr.mad(xs), _sorted_mad(xs)
    assert (math.isnan(a) and math.isnan(b)) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)
    f = np.array([x for x in xs if math.isfinite(x)]) + 0.0
    if len(f):  # and numpy's median of the same values
        assert np.float64(pr.med(xs)).view(np.uint64) == np.float64(np.median(f)).view(np.uint64)


# ---- the definition on a panel with planted loci ----------------------------------------------------------------------------
def test_definition_finds_the_planted_loci():
    G = pr.panel(0)
    assert G.shape == (96, 1500)
    U = pr.svd_scores(G, 2)
    r = pr.pcadapt_ref(G, U)
    zs, o = r["zs"], r["ogk"]
    # conditions on the reference alone: a drifted generator is caught here
    assert int((~zs["valid"]).sum()) == 3 and sorted(np.flatnonzero(~zs["valid"])) == sorted(pr.MONO)
    assert min(o["gaps"]) >= 1e-2, o["gaps"]
    amp = zs["tot"][zs["valid"]] / zs["rss"][zs["valid"]]
    assert amp.max() <= 16, amp.max()
    # what the scan is for
    top = np.argsort(-np.nan_to_num(r["dist"], nan=-1.0))[:15]
    assert sorted(top.tolist()) == pr.PLANTED.tolist()
    assert 0.9 <= r["gc_lambda"] <= 1.1, r["gc_lambda"]
    assert np.isnan(r["dist"][sorted(pr.MONO)]).all() and r["n_valid"] == 1497


def test_ogk_reduces_to_the_scaled_square_for_one_column():
    rng = np.random.default_rng(5)
    z = rng.standard_normal(301)
    z[[3, 77]] = np.nan
    o = pr.ogk_ref(z[:, None])
    want = ((z - pr.med(z)) / pr.sigma(z)) ** 2
    ok = np.isfinite(z)
    assert np.allclose(o["dist"][ok], want[ok], rtol=1e-14, atol=0) and np.isnan(o["dist"][~ok]).all()
    assert abs(o["center"][0] - pr.med(z)) <= 4e-16 * max(1.0, abs(pr.med(z))) and np.isclose(o["cov"][0, 0], pr.sigma(z) ** 2, rtol=1e-14)


def test_ogk_is_unchanged_by_a_sign_flip_of_an_eigenvector():
    rng = np.random.default_rng(6)
    Z = rng.standard_normal((200, 3)) @ np.array([[1.0, 0.4, 0.1], [0.0, 1.0, 0.3], [0.0, 0.0, 1.0]])
    a = pr.ogk_ref(Z)
    # columns of E1 flipped by S1: the second iteration sees S1 R2 S1, whose eigenvectors are S1 E2 (and may be flipped too)
    s1, s2 = np.array([1.0, -1.0, 1.0]), np.array([-1.0, 1.0, -1.0])
    flipped = [a["E"][0] * s1, (s1[:, None] * a["E"][1]) * s2]
    b = pr.ogk_ref(Z, basis=flipped)
    assert np.array_equal(a["dist"], b["dist"])
    assert np.array_equal(b["R"][1], s1[:, None] * a["R"][1] * s1)


# ---- chi-square -------------------------------------------------------------------------------------------------------------
LOGQ_K, ODD_FAR, logq_points = pr.LOGQ_K, pr.ODD_FAR, pr.logq_points


def _lib():
    from tidypopgen_amd import _lib

    return _lib.lib


def test_chisq_median_is_the_reference_root():
    lib = _lib()
    for K in range(1, 65):
        out = C.c_double()
        assert lib.tpg_qchisq_median(K, C.byref(out)) == 0
        want = pr.qchisq_median_ref(K)
        assert pr.ulp_diff(np.array([out.value]), np.array([want]))[0] <= 1, (K, out.value, want)
        assert abs(pr.logq_ref(K, out.value) - math.log(0.5)) < 1e-13
    assert lib.tpg_qchisq_median(0, C.byref(C.c_double())) != 0 and lib.tpg_qchisq_median(3, None) != 0


def _build_san(tmp_path, sanitize=True):
    exe = str(tmp_path / "pcadapt_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd += ["-Wall", "-Wextra", "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc"), os.path.join(ROOT, "tests", "host", "pcadapt_san.cpp"),
            "-o", exe]
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
    assert r.returncode == 0 and lines[-1] == "ok pcadapt", r.stdout[-2000:] + r.stderr[-4000:]
    rows = [ln.split() for ln in lines[:-1]]
    # log Q at the points of the test: the header against logq_ref
    got = {(int(k), _f(x)): _f(v) for tag, k, x, v in (row for row in rows if row[0] == "logq")}
    for K in LOGQ_K:
        for x in logq_points(K):
            want = pr.logq_ref(K, float(x))
            assert abs(got[(K, float(x))] - want) <= 1e-12 * (1 + abs(want)), (K, x, got[(K, float(x))], want)
    # the chi-square median of every K: the library's and the restatement's
    q50 = {int(k): _f(v) for tag, k, v in (row for row in rows if row[0] == "q50")}
    assert sorted(q50) == list(range(1, 65))
    for K, v in q50.items():
        assert pr.ulp_diff(np.array([v]), np.array([pr.qchisq_median_ref(K)]))[0] <= 1, K
    # the OGK glue: R as the header states it, E orthonormal and diagonalising R, the map back as the restatement's loops
    for K in (1, 3, 5):
        def mat(tag, count):
            vals = {int(i): _f(v) for t, k, i, v in (row for row in rows if row[0] == tag and int(row[1]) == K)}
            return np.array([vals[i] for i in range(count)])

        R, E = mat("ogkR", K * K).reshape((K, K), order="F"), mat("ogkE", K * K).reshape((K, K), order="F")
        P = K * (K - 1) // 2
        Rw = np.eye(K)
        for p, (a, b) in enumerate(pr._pairs(K)):
            sp = pr.MAD_SCALE * ((1.0 + 0.07 * (p % 4)) / pr.MAD_SCALE)
            sm = pr.MAD_SCALE * ((0.9 - 0.05 * (p % 3)) / pr.MAD_SCALE)
            Rw[a, b] = Rw[b, a] = (sp * sp - sm * sm) / 4
        assert P == len(pr._pairs(K)) and np.array_equal(R, Rw)
        eps = 2.0 ** -52
        assert np.abs(E.T @ E - np.eye(K)).max() <= 64 * K * eps
        D = E.T @ R @ E
        assert np.abs(D - np.diag(np.diag(D))).max() <= 64 * K * eps * np.linalg.norm(R, 2)
        assert (np.diff(np.diag(D)) <= 64 * K * eps).all()  # descending
        k = np.arange(K)
        center, cov = pr.backmap(K, 1.5 + 0.25 * k, E, 0.75 + 0.125 * k, E, 0.1 * (k - 1), 1.0 + 0.3 * k)
        assert np.array_equal(mat("ogkc", K), center) and np.array_equal(mat("ogkV", K * K).reshape((K, K), order="F"), cov)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_log_q_far_in_the_tail_against_mpmath(tmp_path):
    pytest.importorskip("mpmath")
    exe = _build_san(tmp_path, sanitize=False)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {(int(row[1]), _f(row[2])): _f(row[3]) for row in (ln.split() for ln in r.stdout.splitlines()) if row[0] == "logq"}
    for K in LOGQ_K:
        for x in ODD_FAR + (50.0, 700.0):
            want = pr.logq_mp(K, x)
            assert math.isfinite(got[(K, x)]) and abs(got[(K, x)] - want) <= 1e-12 * (1 + abs(want)), (K, x, got[(K, x)], want)
    # and the restatement itself where both exist
    for K in LOGQ_K:
        for x in (1e-8, float(K), 50.0, 700.0):
            want = pr.logq_mp(K, x)
            assert abs(pr.logq_ref(K, x) - want) <= 1e-12 * (1 + abs(want)), (K, x)
