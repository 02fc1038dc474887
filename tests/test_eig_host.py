"""CPU: the prescribed-spectrum builder of tests/eig_ref.py against LAPACK, so that a failure of tests/test_gpu_eig.py
cannot be the reference's own fault.  The bound, 1e-13 lam_1, is four orders under anything the GPU tests assert."""
import numpy as np
import pytest

from tests import eig_ref as er

NAMES = list(er.SPECTRA) + [er.rank(5), er.rank(20)]
BOUND = 1e-13


@pytest.mark.parametrize("n", [17, 64, 129, 257])
@pytest.mark.parametrize("name", NAMES, ids=lambda s: s if isinstance(s, str) else s.__name__)
def test_builder_has_the_prescribed_spectrum_and_eigenvectors(name, n):
    K, lam, Q = er.build(name, n)
    l1 = lam[0] if lam[0] > 0 else 1.0
    assert K.shape == (n, n) and np.array_equal(K, K.T)
    assert np.all(np.diff(lam) <= 0)
    ev = np.linalg.eigvalsh(K)[::-1]
    assert np.abs(ev - lam).max() <= BOUND * l1
    assert np.abs(K @ Q - Q * lam).max() <= BOUND * l1
    assert np.linalg.norm(K @ Q - Q * lam, 2) <= BOUND * l1
    assert np.abs(Q.T @ Q - np.eye(n)).max() <= BOUND


def test_named_spectra_are_the_documented_ones():
    assert np.array_equal(er.spectrum("geo", 4), [1.0, 0.9, 0.9 ** 2, 0.9 ** 3])
    assert np.array_equal(er.spectrum("spikes", 5), [50.0, 30.0, 20.0, 1.2, 0.8])
    assert np.array_equal(er.spectrum("triple", 8)[:7], [5.0, 4.0, 3.0, 3.0, 3.0, 2.0, 1.0])
    c = er.spectrum("cluster", 300)
    assert c[2] == 3.0 and 0 < c[2] - c[3] < 4e-10 and 0 < c[3] - c[4] < 4e-10 and c[5] == 2.0
    assert np.array_equal(er.spectrum(er.rank(3), 5), [5.0, 3.0, 1.0, 0.0, 0.0])
    assert np.array_equal(er.spectrum("identity", 3), np.ones(3)) and not er.spectrum("zero", 3).any()


def test_check_refuses_a_wrong_answer_and_a_lost_subspace_check():
    """`check` bites: a swapped pair of rows, an eigenvalue off by 1e-8 lam_1, and a zero gap nobody announced"""
    K, lam, Q = er.build("geo", 33)
    er.check(K, lam, Q, lam[:5], Q[:, :5], 5)
    U = Q[:, :5].copy()
    U[[3, 4]] = U[[4, 3]]
    with pytest.raises(AssertionError):
        er.check(K, lam, Q, lam[:5], U, 5)
    bad = lam[:5].copy()
    bad[2] += 1e-8
    with pytest.raises(AssertionError):
        er.check(K, lam, Q, bad, Q[:, :5], 5)
    K, lam, Q = er.build("identity", 33)
    with pytest.raises(AssertionError):
        er.check(K, lam, Q, lam[:5], Q[:, :5], 5)
    er.check(K, lam, Q, lam[:5], Q[:, :5], 5, subspace_undetermined=True)
