"""Reference for the eigen solver tests: symmetric PSD matrices with a prescribed spectrum and known eigenvectors, plain numpy.

K = Q diag(lam) Q' with Q = (I - 2 v v')(I - 2 w w') for two seeded unit vectors: a product of two Householder reflections is
orthogonal to rounding whatever n is, dense (no zero and no repeated entry for an edge lane to hide behind), and both Q and K
come from rank-one updates alone -- O(n^2) work, so n = 4097 costs what its 134 MB cost to write.  tests/test_eig_host.py pins
the builder to LAPACK; tests/test_gpu_eig.py holds tpg.sym_eig_topk to `check`.
"""
import numpy as np


def _geo(n):
    return 0.9 ** np.arange(n)


def _lin(n):
    return np.linspace(1.0, 0.01, n)


def _spikes(n):
    return np.concatenate([[50.0, 30.0, 20.0], np.linspace(1.2, 0.8, n - 3)])


def _triple(n):
    return np.concatenate([[5.0, 4.0, 3.0, 3.0, 3.0, 2.0], np.linspace(1.0, 0.1, n - 6)])


def _cluster(n):
    lam = _triple(n)
    lam[2:5] = [3.0, 3.0 * (1 - 1e-10), 3.0 * (1 - 2e-10)]
    return lam


def _identity(n):
    return np.ones(n)


def _zero(n):
    return np.zeros(n)


def rank(r):
    """linspace(5, 1, r), then zeros"""

    def f(n):
        rr = min(r, n)
        return np.concatenate([np.linspace(5.0, 1.0, rr), np.zeros(n - rr)])

    f.__name__ = f"rank({r})"
    return f


SPECTRA = dict(geo=_geo, lin=_lin, spikes=_spikes, triple=_triple, cluster=_cluster, identity=_identity, zero=_zero)


def spectrum(name, n):
    """the named spectrum at size n, descending; `name` is a key of SPECTRA or a callable such as rank(5)"""
    lam = np.asarray((SPECTRA[name] if isinstance(name, str) else name)(n), dtype=float)
    assert lam.shape == (n,) and np.all(np.diff(lam) <= 0) and np.all(lam >= 0)
    return lam


def _unit(rng, n):
    x = rng.standard_normal(n)
    return x / np.linalg.norm(x)


def build(name, n, seed=0):
    """(K, lam, Q): K = Q diag(lam) Q' symmetrised, lam descending, the columns of Q its eigenvectors"""
    lam = spectrum(name, n)
    rng = np.random.default_rng(1000 * seed + n)
    v, w = _unit(rng, n), _unit(rng, n)
    # Q = H_v H_w = I - 2 v v' - 2 w w' + 4 (v'w) v w'
    Q = np.eye(n)
    Q -= 2.0 * np.outer(v, v)
    Q -= 2.0 * np.outer(w, w)
    Q += (4.0 * (v @ w)) * np.outer(v, w)
    # K = H_v (H_w D H_w) H_v, each reflection pair as a symmetric rank-two update: H M H = M - 2 h (M h)' - 2 (M h) h' +
    # 4 (h' M h) h h'
    M = np.diag(lam)
    for h in (w, v):
        Mh = M @ h
        hMh = h @ Mh
        M -= 2.0 * np.outer(h, Mh)
        M -= 2.0 * np.outer(Mh, h)
        M += (4.0 * hMh) * np.outer(h, h)
    K = 0.5 * (M + M.T)
    return K, lam, Q


def figures(K, lam_true, Q_true, lam, U, k):
    """the quantities `check` bounds, each relative to its bound's own scale; `sub` and `gap` are None where the top-k subspace
    is not determined (k = n, or lam_k = lam_{k+1})"""
    n = K.shape[0]
    lam, U = np.asarray(lam, dtype=float), np.asarray(U, dtype=float)
    assert lam.shape == (k,) and U.shape == (n, k)
    l1 = lam_true[0] if lam_true[0] > 0 else 1.0
    # scaled by an exact power of two before anything is multiplied: the figures are those of the matrix at unit scale
    e = int(np.frexp(l1)[1])
    Ks, ls, lt = np.ldexp(K, -e), np.ldexp(lam, -e), np.ldexp(lam_true, -e)
    l1s = np.ldexp(l1, -e)
    out = dict(n=n, k=k)
    out["lam"] = float(np.abs(ls - lt[:k]).max() / l1s)
    out["order"] = float(np.diff(ls).max() / l1s) if k > 1 else 0.0
    out["res"] = float(np.abs(Ks @ U - U * ls).max() / l1s)
    out["orth"] = float(np.abs(U.T @ U - np.eye(k)).max())
    gap = float((lt[k - 1] - lt[k]) / l1s) if k < n else None
    out["gap"], out["sub"] = gap, None
    if k < n and gap > 0:
        Qk = Q_true[:, :k]
        out["sub"] = float(np.abs(Qk @ Qk.T - U @ U.T).max())
    return out


def check(K, lam_true, Q_true, lam, U, k, subspace_undetermined=False, label=""):
    """The contract of tpg_sym_eig_topk, each bound one the suite already holds the solver to (tests/test_gpu_parity.py,
    test_pca_more_than_52_components): eigenvalues and residual within 1e-9 lam_1, descending up to the solver's own
    acceptance tolerance 1e-12 lam_1, U orthonormal to 1e-9, and the projector on span(U) within 1e-9 / gap of the true one,
    gap = (lam_k - lam_{k+1}) / lam_1.  The projector is not compared when k = n (it is the identity: orthonormality says
    so) or when the gap is 0 -- and a zero gap is accepted only from a caller that says its case has one
    (`subspace_undetermined`), so no case loses the check by accident.  Returns the figures; a failure shows all of them."""
    f = figures(K, lam_true, Q_true, lam, U, k)
    f["case"] = label
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(U)), f
    assert f["lam"] <= 1e-9, f
    assert f["order"] <= 1e-12, f
    assert f["res"] <= 1e-9, f
    assert f["orth"] <= 1e-9, f
    if k < K.shape[0]:
        if f["gap"] > 0:
            assert not subspace_undetermined, ("the case claims a zero gap and has none", f)
            assert f["sub"] <= 1e-9 / f["gap"], f
        else:
            assert subspace_undetermined, ("zero gap below the k-th eigenvalue: the subspace check was lost", f)
    return f
