"""The admixture cross-validation of include/tpg.h "admixture cross-validation" restated in numpy on top of tests/admix_ref.py:
the fold of an entry in uint64 arithmetic, the hold-out view, the hold-out sums by a float route (admix_ref.loglik on the
complementary codes) and an exact route (admix_ref.loglik_exact), the deviance and the CV error in the stated operation order,
and the whole procedure with the numpy EM (cross_validate: slow, for figures worked out once on a CPU)."""
import math

import numpy as np

from tests import admix_ref as ar

CV_SALT = 0xC3C3C3C3C3C3C3C3
MAX_FOLDS = 64  # TPG_ADMIX_MAX_FOLDS
FOUR_LN2 = 2.772588722239781


def fold_int(cv_seed, i, j, folds):
    """fold(i, j) with Python integers"""
    key = ar.mix64_int(((cv_seed & ar.MASK) ^ CV_SALT) ^ ar.mix64_int(j))
    h = ar.mix64_int(key ^ ar.mix64_int(i))
    return ((h >> 32) * folds) >> 32


def folds_of(cv_seed, n, m, folds):
    """fold(i, j) of every position of an n x m view -> int64 (n, m)"""
    key = ar.mix64((np.uint64(cv_seed & ar.MASK) ^ np.uint64(CV_SALT)) ^ ar.mix64(np.arange(m, dtype=np.uint64)))
    h = ar.mix64(key[None, :] ^ ar.mix64(np.arange(n, dtype=np.uint64))[:, None])
    return (((h >> np.uint64(32)) * np.uint64(folds)) >> np.uint64(32)).astype(np.int64)


def holdout(codes, folds, fold, cv_seed):
    """train_f: every typed entry of fold `fold` set to code 3"""
    codes = np.asarray(codes)
    train = codes.copy()
    train[(codes != ar.MISSING) & (folds_of(cv_seed, codes.shape[0], codes.shape[1], folds) == fold)] = ar.MISSING
    return train


def complement(codes, train):
    """the codes typed only where held out: typed in `codes` and missing in `train`"""
    codes, train = np.asarray(codes), np.asarray(train)
    held = (codes != ar.MISSING) & (train == ar.MISSING)
    return np.where(held, codes, ar.MISSING).astype(np.uint8)


def holdout_sums(codes, train, Q, F, exact=False):
    """-> dict(ll, n_held, n_het) over the entries typed in `codes` and missing in `train`; Q and F as given"""
    comp = complement(codes, train)
    ll = ar.loglik_exact(comp, Q, F) if exact else ar.loglik(comp, Q, F)
    return dict(ll=ll, n_held=int((comp != ar.MISSING).sum()), n_het=int((comp == 1).sum()))


def deviance_direct(codes, train, Q, F):
    """sum over the held-out entries of 2 [g ln(g / 2p) + (2 - g) ln((2 - g) / 2 pbar)], 0 ln 0 = 0, term by term"""
    comp = complement(codes, train)
    Q, F = np.asarray(Q, dtype=np.float64), np.asarray(F, dtype=np.float64)
    terms = []
    for i, j in zip(*np.nonzero(comp != ar.MISSING)):
        g = int(comp[i, j])
        p = float(sum(Q[i, k] * F[j, k] for k in range(Q.shape[1])))
        pb = float(sum(Q[i, k] * (1.0 - F[j, k]) for k in range(Q.shape[1])))
        t = 0.0
        if g > 0:
            t += g * math.log(g / (2.0 * p))
        if g < 2:
            t += (2 - g) * math.log((2 - g) / (2.0 * pb))
        terms.append(2.0 * t)
    return math.fsum(terms)


def cv_error(fold_ll, fold_count, fold_het):
    """-> cv_error, fold_deviance: dev_f = -2.0 * ll_f - 4 ln 2 * (double)het_f (two products, one subtraction), the deviances added
    in ascending f, divided by the total count as a double"""
    dev = []
    for ll, het in zip(fold_ll, fold_het):
        a = np.float64(-2.0) * np.float64(ll)
        b = np.float64(FOUR_LN2) * np.float64(int(het))
        dev.append(a - b)
    s = dev[0]
    for d in dev[1:]:
        s = s + d
    return float(s / np.float64(int(sum(int(c) for c in fold_count)))), np.array(dev, dtype=np.float64)


def em(codes, Q, F, max_iter, tol):
    """the iteration of "admixture" with the float step: -> Q, F, n_iter"""
    ll, t = [], 0
    while t < max_iter:
        ll.append(ar.loglik(codes, Q, F))
        Q, F, _ = ar.em_step(codes, Q, F)
        t += 1
        if t >= 2 and ll[t - 1] - ll[t - 2] < tol:
            break
    return Q, F, t


def cross_validate(codes, K, folds, cv_seed, seed, max_iter, tol):
    """the whole procedure with the numpy EM from the seeded start -> cv_error, total held-out count"""
    n, m = codes.shape
    Q0, F0 = ar.start(seed, n, m, K)
    lls, cnts, hets = [], [], []
    for f in range(folds):
        train = holdout(codes, folds, f, cv_seed)
        Q, F, _ = em(train, Q0, F0, max_iter, tol)
        s = holdout_sums(codes, train, Q, F)
        lls.append(s["ll"]), cnts.append(s["n_held"]), hets.append(s["n_het"])
    return cv_error(lls, cnts, hets)[0], sum(cnts)
