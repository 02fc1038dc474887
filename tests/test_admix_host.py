"""CPU: the admixture restatement tests/admix_ref.py against itself, and the library's constants against it.

The float route (em_step, loglik) is held against the exact Fraction route within the bounds of include/tpg.h "admixture":
|df'| <= (2 N + 4 K + 40) u f', |dq'| <= (2 T_i + 2 K + 16) u q', |dl| <= u [(2 T + 2) |l| + 2 (K + 4) T], u = 2^-52.  The
exact route gives row sums of exactly 1 and, at K = 1, exactly the alt-allele frequency.  The hash start is held against values
computed by hand (Python integers) for three (seed, i, k) triples."""
from fractions import Fraction

import numpy as np
import pytest

from tests import admix_ref as ar

N, M = 7, 9


def _case(K, miss=0.15):
    codes, _, _, planted = ar.panel(100 + K, N, M, K, miss)
    Q0, F0 = ar.start(5 + K, N, M, K)
    return codes, Q0, F0, planted


@pytest.mark.parametrize("K", [1, 2, 3])
def test_float_step_within_the_bounds_of_the_exact_step(K):
    codes, Q0, F0, planted = _case(K)
    qf, _, f_raw = ar.em_step(codes, Q0, F0)
    qx, fx = ar.em_step_exact(codes, Q0, F0)
    t_i = (codes != ar.MISSING).sum(axis=1)
    qx_f = np.array([[float(x) for x in row] for row in qx])
    fx_f = np.array([[float(x) for x in row] for row in fx])
    dq = np.array([[abs(float(Fraction(float(qf[i, k])) - qx[i][k])) for k in range(K)] for i in range(N)])
    df = np.array([[abs(float(Fraction(float(f_raw[j, k])) - fx[j][k])) for k in range(K)] for j in range(M)])
    assert (dq <= ar.bound_q(t_i, K, qx_f)).all()
    assert (df <= ar.bound_f(N, K, fx_f)).all()
    # the planted locus nobody is typed at and the row typed nowhere stay as they are, bit for bit
    assert np.array_equal(f_raw[planted["col_missing"]], F0[planted["col_missing"]])
    assert np.array_equal(qf[planted["row_missing"]], Q0[planted["row_missing"]])
    assert fx[planted["col_all0"]] == [0] * K and fx[planted["col_all2"]] == [1] * K


@pytest.mark.parametrize("K", [1, 2, 3])
def test_exact_rows_sum_to_one(K):
    codes, Q0, F0, planted = _case(K)
    # the exact step keeps a row sum of exactly 1 only from a row that sums to exactly 1: take exact rational rows
    rng = np.random.default_rng(K)
    w = rng.integers(1, 1 << 20, size=(N, K)).astype(np.float64)
    w[:, K - 1] = 2.0 ** 22 - w[:, : K - 1].sum(axis=1)  # every row sums to 2^22 exactly
    Q = w / 2.0 ** 22
    assert (Q > 0).all()
    qx, _ = ar.em_step_exact(codes, Q, F0)
    for i in range(N):
        assert sum(qx[i]) == 1


def test_k1_gives_the_alt_allele_frequency_exactly():
    codes, _, F0, planted = _case(1)
    Q = np.ones((N, 1))
    _, fx = ar.em_step_exact(codes, Q, F0)
    typed = codes != ar.MISSING
    for j in range(M):
        nv = int(typed[:, j].sum())
        if nv == 0:
            assert fx[j][0] == Fraction(float(F0[j, 0]))
        else:
            assert fx[j][0] == Fraction(int(codes[typed[:, j], j].sum()), 2 * nv)


@pytest.mark.parametrize("K", [2, 3])
def test_loglik_does_not_decrease_over_50_float_steps(K):
    codes, Q, F, _ = _case(K, miss=0.1)
    T = int((codes != ar.MISSING).sum())
    F = ar.clamp(F)
    prev = ar.loglik(codes, Q, F)
    first = prev
    for _ in range(50):
        Q, F, _ = ar.em_step(codes, Q, F)
        ll = ar.loglik(codes, Q, F)
        assert ll >= prev - ar.bound_ll(T, K, prev) - ar.bound_ll(T, K, ll)
        prev = ll
    assert prev > first
    assert np.allclose(Q.sum(axis=1), 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("K", [1, 2, 3])
def test_float_loglik_within_the_bound_of_the_exact_one(K):
    codes, Q0, F0, _ = _case(K)
    T = int((codes != ar.MISSING).sum())
    lx = ar.loglik_exact(codes, Q0, F0)
    assert abs(ar.loglik(codes, Q0, F0) - lx) <= ar.bound_ll(T, K, lx)


# (seed, i, k) -> the hash h of the Q start and of the F start at (j = i, k), computed by hand with Python integers:
# h_Q = M(M(seed ^ M(i)) ^ M(k)), h_F = M(M((seed ^ 0xF0F0F0F0F0F0F0F0) ^ M(i)) ^ M(k))
HAND = [
    (0, 0, 0, 0xA7F72697A2731486, 0x9A71F7B90FD05403),
    (7, 12, 2, 0xF1AC7CD88340E01F, 0xD7B0D2613A5C261B),
    (0xDEADBEEFCAFEF00D, 129, 31, 0x171DBDAECB55633F, 0x682132B64CB2CD84),
]


@pytest.mark.parametrize("seed,i,k,hq,hf", HAND)
def test_hash_start_equals_hand_computed_values(seed, i, k, hq, hf):
    assert ar.mix64_int(ar.mix64_int(seed ^ ar.mix64_int(i)) ^ ar.mix64_int(k)) == hq
    K = k + 1
    Q0, F0 = ar.start(seed, i + 1, i + 1, K)
    u = lambda h: (float(h >> 11) + 0.5) * 2.0 ** -53  # noqa: E731
    assert F0[i, k] == 0.1 + 0.8 * u(hf)
    row = 0.0
    for kk in range(K):
        row += u(ar.mix64_int(ar.mix64_int(seed ^ ar.mix64_int(i)) ^ ar.mix64_int(kk)))
    assert Q0[i, k] == u(hq) / row
    assert (F0 >= 0.1).all() and (F0 <= 0.9).all() and (Q0 > 0).all()


def test_hand_values_in_decimal():
    """the first triple spelled out: u = (floor(h / 2^11) + 0.5) / 2^53"""
    assert (float(0xA7F72697A2731486 >> 11) + 0.5) * 2.0 ** -53 == 0.6561149711801131
    assert (0.1 + 0.8 * ((float(0x9A71F7B90FD05403 >> 11) + 0.5) * 2.0 ** -53)).hex() == "0x1.2a4ff2c1b2e6fp-1"


def test_library_constants_match_the_restatement():
    from tidypopgen_amd import _lib, api

    pr = _lib.AdmixParams()
    assert _lib.lib.tpg_admix_params_default(pr) == 0
    assert (pr.max_iter, pr.tol, pr.update_q, pr.update_f, pr.seed) == (1000, 1e-4, 1, 1, 0)
    assert api.ADMIX_CHUNK_LOCI == int(_lib.lib.tpg_admix_chunk_loci()) and api.ADMIX_CHUNK_LOCI % 128 == 0
    import re, os

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tpg.h")).read()
    assert float(re.search(r"#define TPG_ADMIX_EPS (\S+)", hdr).group(1)) == ar.EPS
    assert int(re.search(r"#define TPG_ADMIX_CHUNK_LOCI (\d+)", hdr).group(1)) == api.ADMIX_CHUNK_LOCI


def test_gt_admixture_seed_rule_needs_no_device():
    import tidypopgen_amd as tpg

    with pytest.raises(ValueError, match=r"'seed' should be a vector of length 'n_runs' OR 'n_runs' \* length\(k\)"):
        tpg.gt_admixture(None, k=[2, 3], n_runs=2, seed=[1, 2, 3])
