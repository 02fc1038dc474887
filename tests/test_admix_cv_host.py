"""CPU: the cross-validation restatement tests/admix_cv_ref.py against itself, and the host-only tpg_admix_cv_error of the library
against it.

The fold hash is held against values computed by hand (Python integers) for three (cv_seed, i, j) triples; the folds split every
position evenly, are disjoint and cover the typed entries; the float route of the hold-out log-likelihood is within the bound of
include/tpg.h "admixture" (T = the held-out entries) of the exact route; -2 ll - 4 ln 2 het equals the deviance written out term by
term with 0 ln 0 = 0."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import admix_cv_ref as cr
from tests import admix_ref as ar

N, M = 7, 9

# (cv_seed, i, j, folds) -> key = M((cv_seed ^ 0xC3C3C3C3C3C3C3C3) ^ M(j)), h = M(key ^ M(i)), fold = ((h >> 32) * folds) >> 32
HAND = [
    (0, 0, 0, 5, 0xFA713F8ACBC9914D, 0x66CDBAD81BB42E32, 2),
    (1, 12, 399, 5, 0xAF0F9E051A734B75, 0x9C2BA645E944702F, 3),
    (0xDEADBEEFCAFEF00D, 129, 4096, 64, 0x759BF1FCB9DE8E65, 0x249E8E3CB72C3475, 9),
]


@pytest.mark.parametrize("cv_seed,i,j,folds,key,h,fold", HAND)
def test_fold_hash_equals_hand_computed_values(cv_seed, i, j, folds, key, h, fold):
    assert ar.mix64_int((cv_seed ^ cr.CV_SALT) ^ ar.mix64_int(j)) == key
    assert ar.mix64_int(key ^ ar.mix64_int(i)) == h
    assert ((h >> 32) * folds) >> 32 == fold  # the first triple: 0x66CDBAD8 * 5 = 0x2_0205_A638
    assert cr.fold_int(cv_seed, i, j, folds) == fold
    assert cr.folds_of(cv_seed, i + 1, j + 1, folds)[i, j] == fold


@pytest.mark.parametrize("n,m,folds,cv_seed", [(130, 400, 5, 1), (65, 600, 5, 1)])
def test_every_fold_takes_its_share_of_the_positions(n, m, folds, cv_seed):
    fo = cr.folds_of(cv_seed, n, m, folds)
    assert fo.min() == 0 and fo.max() == folds - 1
    shares = [(fo == f).mean() for f in range(folds)]
    print("fold shares", n, m, shares)
    assert all(abs(s - 0.2) <= 0.01 for s in shares)


@pytest.mark.parametrize("folds", [2, 5, 64])
def test_folds_are_disjoint_and_cover_every_typed_entry(folds):
    codes = ar.panel(3, 65, 33, 2, 0.1)[0]
    typed = codes != ar.MISSING
    held = np.zeros(codes.shape, dtype=np.int64)
    for f in range(folds):
        train = cr.holdout(codes, folds, f, 9)
        assert np.array_equal(train[train != ar.MISSING], codes[train != ar.MISSING])  # what stays typed is unchanged
        assert not (typed < (train != ar.MISSING)).any()                                # nothing missing becomes typed
        held += typed & (train == ar.MISSING)
    assert np.array_equal(held, typed.astype(np.int64))
    # another seed, another split; the same seed, the same split
    assert not np.array_equal(cr.holdout(codes, 5, 0, 9), cr.holdout(codes, 5, 0, 10))
    assert np.array_equal(cr.holdout(codes, 5, 0, 9), cr.holdout(codes, 5, 0, 9))


def _case(K):
    codes = ar.panel(100 + K, N, M, K, 0.15)[0]
    Q, F = ar.start(5 + K, N, M, K)
    return codes, Q, F


@pytest.mark.parametrize("K", [1, 2, 3])
def test_float_holdout_ll_within_the_bound_of_the_exact_one(K):
    codes, Q, F = _case(K)
    total = 0
    for f in range(3):
        train = cr.holdout(codes, 3, f, 4)
        a, x = cr.holdout_sums(codes, train, Q, F), cr.holdout_sums(codes, train, Q, F, exact=True)
        assert (a["n_held"], a["n_het"]) == (x["n_held"], x["n_het"]) and a["n_held"] > 0
        assert abs(a["ll"] - x["ll"]) <= ar.bound_ll(a["n_held"], K, x["ll"])
        total += a["n_held"]
    assert total == int((codes != ar.MISSING).sum())


@pytest.mark.parametrize("K", [1, 2, 3])
def test_deviance_identity(K):
    codes, Q, F = _case(K)
    train = cr.holdout(codes, 2, 1, 4)
    s = cr.holdout_sums(codes, train, Q, F, exact=True)
    assert s["n_het"] > 0
    direct = cr.deviance_direct(codes, train, Q, F)
    via_ll = -2.0 * s["ll"] - 4.0 * math.log(2.0) * s["n_het"]
    assert abs(via_ll - direct) <= 1e-12 * abs(direct)
    assert cr.FOUR_LN2 == 4.0 * math.log(2.0)


def _lib_cv_error(ll, cnt, het, folds=None, want_dev=True):
    from tidypopgen_amd import _lib

    ll = np.ascontiguousarray(ll, dtype=np.float64)
    cnt, het = np.ascontiguousarray(cnt, dtype=np.int64), np.ascontiguousarray(het, dtype=np.int64)
    dev, cv = np.full(64, 7.0), C.c_double(7.0)
    rc = _lib.lib.tpg_admix_cv_error(len(ll) if folds is None else folds, ll.ctypes.data, cnt.ctypes.data, het.ctypes.data,
                                     dev.ctypes.data if want_dev else None, C.byref(cv))
    return rc, cv.value, dev


def test_library_cv_error_equals_the_restatement_bit_for_bit():
    rng = np.random.default_rng(8)
    for folds in (2, 5, 64):
        cnt = rng.integers(1, 10 ** 7, size=folds)
        het = (cnt * rng.uniform(0.0, 1.0, size=folds)).astype(np.int64)
        ll = -cnt * rng.uniform(0.3, 1.4, size=folds)
        rc, cv, dev = _lib_cv_error(ll, cnt, het)
        want_cv, want_dev = cr.cv_error(ll, cnt, het)
        assert rc == 0 and np.float64(cv).view(np.uint64) == np.float64(want_cv).view(np.uint64)
        assert np.array_equal(dev[:folds].view(np.uint64), want_dev.view(np.uint64)) and (dev[folds:] == 7.0).all()
        rc, cv2, dev = _lib_cv_error(ll, cnt, het, want_dev=False)
        assert rc == 0 and cv2 == cv and (dev == 7.0).all()
    # the Python layer
    import tidypopgen_amd as tpg

    out = tpg.admix_cv_error(ll, cnt, het)
    assert out["cv_error"] == want_cv and np.array_equal(out["fold_deviance"].view(np.uint64), want_dev.view(np.uint64))


def test_library_cv_error_refusals_leave_the_outputs_untouched():
    import tidypopgen_amd as tpg
    from tidypopgen_amd import _lib

    EINVAL = 1
    ll, het = -np.arange(1.0, 66.0), np.zeros(65, dtype=np.int64)
    for folds, cnt in ((5, np.zeros(65, dtype=np.int64)), (1, np.ones(65, dtype=np.int64)), (0, np.ones(65, dtype=np.int64)),
                       (65, np.ones(65, dtype=np.int64))):
        rc, cv, dev = _lib_cv_error(ll, cnt, het, folds=folds)
        assert rc == EINVAL and cv == 7.0 and (dev == 7.0).all(), folds
    assert _lib_cv_error(ll[:64], np.ones(64, dtype=np.int64), het[:64])[0] == 0
    with pytest.raises(_lib.TpgError, match="no held-out entry"):
        tpg.admix_cv_error([-1.0, -2.0], [0, 0], [0, 0])
    with pytest.raises(_lib.TpgError, match=r"folds = 1 out of \[2, 64\]"):
        tpg.admix_cv_error([-1.0], [3], [0])
    with pytest.raises(ValueError, match="one entry per fold"):
        tpg.admix_cv_error([-1.0, -2.0], [3], [0, 0])


def test_header_constants_match_the_restatement():
    import os
    import re

    from tidypopgen_amd import api

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tpg.h")).read()
    assert int(re.search(r"#define TPG_ADMIX_MAX_FOLDS (\d+)", hdr).group(1)) == cr.MAX_FOLDS == api.ADMIX_MAX_FOLDS
    assert "0xC3C3C3C3C3C3C3C3" in hdr and "2.772588722239781" in hdr and "recalled, not pinned" in hdr.lower()


def test_gt_admixture_crossval_argument_errors_need_no_device():
    import tidypopgen_amd as tpg

    for bad in (1, 65, 0, 2.5, None):
        with pytest.raises(ValueError, match=r"'cv_folds' should be an integer in \[2, 64\]"):
            tpg.gt_admixture(None, k=[2, 3], crossval=True, cv_folds=bad)
    with pytest.raises(ValueError, match=r"'seed' should be a vector of length 'n_runs' OR 'n_runs' \* length\(k\)"):
        tpg.gt_admixture(None, k=[2, 3], n_runs=2, seed=[1, 2, 3], crossval=True)
