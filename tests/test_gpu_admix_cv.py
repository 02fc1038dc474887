"""GPU: admixture cross-validation (include/tpg.h "admixture cross-validation") against the numpy restatement
tests/admix_cv_ref.py.

What is compared how.  A hold-out view: byte for byte, and its count exactly.  The hold-out sums from a given (Q, F): the counts
exactly, ll within |dl| <= u [(2 T + 2) |l| + 2 (K + 4) T] (T = the held-out entries) of the float route, of the exact route on the
two smallest shapes, and of tpg_admix_loglik on the complementary view.  tpg_admix_cv: bit for bit the composition of its pieces
(View.holdout -> admix_em -> admix_holdout_sums -> admix_cv_error).  The choice of K on a simulated two-population panel: against
the CV errors the numpy EM gave on a CPU (admix_cv_ref.cross_validate, about 20 s, not rerun here).  The cases and their views are
those of tests/test_gpu_admix.py: row / column subsets of a larger store."""
import ctypes as C

import numpy as np
import pytest

from tests import admix_cv_ref as cr
from tests import admix_ref as ar
from tests.test_gpu_admix import _bits, _case, _check_step, _embed

pytestmark = pytest.mark.gpu

SHAPES = [(13, 1, 1, 0.0), (13, 31, 2, 0.1), (65, 33, 3, 0.1), (130, 129, 8, 0.1), (130, "chunk+1", 32, 0.1)]
SMALL = SHAPES[:2]
EINVAL = 1
# at (13, 1, 1) with folds = 2 this seed puts every typed entry of the one locus into fold 0 (found by a search over seeds with
# admix_cv_ref.folds_of): train_0 has a locus, and individuals, typed nowhere
EMPTYING_SEED = 4849


@pytest.mark.parametrize("n,m,K,miss", SHAPES)
def test_holdout_view_equals_the_restatement_byte_for_byte(n, m, K, miss):
    c = _case(n, m, K, miss)
    v, codes = c["v"], c["codes"]
    for folds in (2, 5, 64):
        for fold in (0, folds - 1):
            for cv_seed in (7, 0xDEADBEEFCAFEF00D):
                t = v.holdout(folds, fold, cv_seed)
                want = cr.holdout(codes, folds, fold, cv_seed)
                assert (t.n, t.m) == codes.shape
                assert np.array_equal(t.unpack(), want)
                assert t.n_held == int(((codes != ar.MISSING) & (want == ar.MISSING)).sum())
    assert np.array_equal(v.unpack(), codes)  # the view itself is as it was


def test_holdout_mask_ignores_store_positions_and_repeats():
    import tidypopgen_amd as tpg

    c = _case(65, 33, 3, 0.1)
    big2, rows2, cols2 = _embed(c["codes"], 991)  # the same panel at other rows / columns of another store
    assert not (np.array_equal(rows2, c["rows"]) and np.array_equal(cols2, c["cols"]))
    v2 = tpg.View(tpg.FBM.from_numpy(np.asfortranarray(big2), code256=tpg.CODE_012), rows2, cols2)
    a, b, again = c["v"].holdout(5, 3, 11), v2.holdout(5, 3, 11), c["v"].holdout(5, 3, 11)
    assert np.array_equal(a.unpack(), b.unpack()) and np.array_equal(a.unpack(), again.unpack())
    assert a.n_held == b.n_held == again.n_held > 0
    assert not np.array_equal(a.unpack(), c["v"].holdout(5, 3, 12).unpack())


def test_holdout_refuses_bad_folds():
    from tidypopgen_amd import _lib

    v = _case(13, 31, 2, 0.1)["v"]
    for folds, fold in ((1, 0), (0, 0), (65, 0), (-3, 0), (5, -1), (5, 5), (64, 64)):
        with pytest.raises(_lib.TpgError) as e:
            v.holdout(folds, fold)
        assert e.value.code == EINVAL, (folds, fold)
    assert v.holdout(64, 63).n == 13 and v.holdout(2, 1).m == 31


@pytest.mark.parametrize("n,m,K,miss", SHAPES)
def test_holdout_sums_from_a_given_state(n, m, K, miss):
    import tidypopgen_amd as tpg

    c = _case(n, m, K, miss)
    v, codes, Q, F = c["v"], c["codes"], c["Qs"], c["Fs"]
    folds, fold, cv_seed = 3, 1, 5
    t = v.holdout(folds, fold, cv_seed)
    train = cr.holdout(codes, folds, fold, cv_seed)
    got, ref = tpg.admix_holdout_sums(v, t, Q, F), cr.holdout_sums(codes, train, Q, F)
    assert (got["n_held"], got["n_het"]) == (ref["n_held"], ref["n_het"]) and got["n_held"] == t.n_held
    nh = ref["n_held"]
    print("hold-out ll", n, c["m"], K, nh, got["ll"], ref["ll"], abs(got["ll"] - ref["ll"]), ar.bound_ll(nh, K, ref["ll"]))
    assert abs(got["ll"] - ref["ll"]) <= ar.bound_ll(nh, K, ref["ll"])
    if (n, m, K, miss) in SMALL:
        lx = cr.holdout_sums(codes, train, Q, F, exact=True)["ll"]
        assert abs(got["ll"] - lx) <= ar.bound_ll(nh, K, lx)
    # the likelihood pass on the complementary view (typed only where held out)
    comp = cr.complement(codes, train)
    vc = tpg.View(tpg.FBM.from_numpy(np.asfortranarray(comp), code256=tpg.CODE_012))
    llc = tpg.admix_loglik(vc, Q, F)
    print("  admix_loglik of the complementary view", llc, "the same bits:", llc == got["ll"])
    assert abs(got["ll"] - llc) <= ar.bound_ll(nh, K, llc)
    # l(full) = l(train) + ll_h, each device value within its bound
    l_full, l_train = tpg.admix_loglik(v, Q, F), tpg.admix_loglik(t, Q, F)
    bound = ar.bound_ll(int((train != ar.MISSING).sum()), K, l_train) + ar.bound_ll(nh, K, got["ll"])
    print("  l(full) - (l(train) + ll_h)", l_full - (l_train + got["ll"]), bound)
    assert abs(l_full - (l_train + got["ll"])) <= bound
    # a second call gives the same bits
    assert tpg.admix_holdout_sums(v, t, Q, F) == got


def test_holdout_sums_refuse_mismatched_geometry_and_leave_the_outputs():
    from tidypopgen_amd import _lib
    from tidypopgen_amd.api import _ptr

    c, other = _case(13, 31, 2, 0.1), _case(65, 33, 3, 0.1)
    t = c["v"].holdout(5, 0, 1)
    Q, F = np.asfortranarray(c["Qs"]), np.asfortranarray(c["Fs"])

    def call(full, train, K=2):
        ll, cnt, het = C.c_double(7.0), C.c_int64(7), C.c_int64(7)
        rc = _lib.lib.tpg_admix_holdout_sums(full.ctx.h, full.h, train.h, K, _ptr(Q), _ptr(F), C.byref(ll), C.byref(cnt), C.byref(het))
        if rc != 0:
            assert (ll.value, cnt.value, het.value) == (7.0, 7, 7)
        return rc

    assert call(c["v"], other["v"]) == EINVAL and call(other["v"], t) == EINVAL
    assert call(c["v"], _case(13, 1, 1, 0.0)["v"]) == EINVAL  # the same n, another m
    assert call(c["v"], t, K=0) == EINVAL and call(c["v"], t, K=33) == EINVAL
    assert call(c["v"], t) == 0
    # NULL outputs are allowed
    assert _lib.lib.tpg_admix_holdout_sums(c["v"].ctx.h, c["v"].h, t.h, 2, _ptr(Q), _ptr(F), None, None, None) == 0


@pytest.mark.parametrize("n,m,K,miss,folds,fold,cv_seed", [(13, 1, 1, 0.0, 2, 0, EMPTYING_SEED), (13, 1, 1, 0.0, 2, 1, EMPTYING_SEED),
                                                           (65, 33, 3, 0.1, 5, 2, 3), (130, "chunk+1", 32, 0.1, 5, 4, 3)])
def test_one_em_step_on_a_holdout_view(n, m, K, miss, folds, fold, cv_seed):
    import tidypopgen_amd as tpg

    c = _case(n, m, K, miss)
    t = c["v"].holdout(folds, fold, cv_seed)
    train = cr.holdout(c["codes"], folds, fold, cv_seed)
    r = tpg.admix_em(t, K, Q0=c["Q0"], F0=c["F0"], max_iter=1)
    assert r["n_iter"] == 1
    _check_step(dict(c, codes=train), c["Qs"], c["Fs"], r["Q"], r["P"])
    if cv_seed == EMPTYING_SEED and fold == 0:  # the mask emptied the locus: everything keeps its start
        assert (train == ar.MISSING).all() and t.n_held == int((c["codes"] != ar.MISSING).sum())
        assert np.array_equal(_bits(r["P"]), _bits(c["Fs"])) and np.array_equal(_bits(r["Q"]), _bits(c["Qs"]))
        s = tpg.admix_holdout_sums(c["v"], t, r["Q"], r["P"])  # and the held-out entries are still predicted from it
        ref = cr.holdout_sums(c["codes"], train, r["Q"], r["P"])
        assert s["n_held"] == ref["n_held"] and abs(s["ll"] - ref["ll"]) <= ar.bound_ll(ref["n_held"], K, ref["ll"])
    # rows and loci the mask left untyped keep their start bit for bit
    dead_rows, dead_cols = (train == ar.MISSING).all(axis=1), (train == ar.MISSING).all(axis=0)
    assert np.array_equal(_bits(r["Q"][dead_rows]), _bits(c["Qs"][dead_rows]))
    assert np.array_equal(_bits(r["P"][dead_cols]), _bits(c["Fs"][dead_cols]))


def _compose(tpg, v, K, folds, cv_seed, **kw):
    ll, cnt, het, nit, conv = [], [], [], [], []
    for f in range(folds):
        t = v.holdout(folds, f, cv_seed)
        r = tpg.admix_em(t, K, **kw)
        s = tpg.admix_holdout_sums(v, t, r["Q"], r["P"])
        ll.append(s["ll"]), cnt.append(s["n_held"]), het.append(s["n_het"]), nit.append(r["n_iter"]), conv.append(r["converged"])
        t.free()
    e = tpg.admix_cv_error(ll, cnt, het)
    return dict(cv_error=e["cv_error"], fold_deviance=e["fold_deviance"], fold_ll=np.array(ll), fold_count=np.array(cnt),
                fold_het=np.array(het), fold_n_iter=np.array(nit), fold_converged=np.array(conv))


@pytest.mark.parametrize("n,m,K,miss,folds", [(13, 31, 2, 0.1, 2), (65, 33, 3, 0.1, 5), (130, 129, 8, 0.1, 5), (130, "chunk+1", 32, 0.1, 3)])
def test_admix_cv_is_the_composition_of_its_pieces_bit_for_bit(n, m, K, miss, folds):
    import tidypopgen_amd as tpg

    c = _case(n, m, K, miss)
    v = c["v"]
    for kw in (dict(Q0=c["Q0"], F0=c["F0"]), dict(seed=77)):
        got = tpg.admix_cv(v, K, folds=folds, cv_seed=9, max_iter=3, tol=0.0, **kw)
        want = _compose(tpg, v, K, folds, 9, max_iter=3, tol=0.0, **kw)
        assert sorted(got) == sorted(want)
        for name in ("fold_ll", "fold_deviance"):
            assert np.array_equal(_bits(got[name]), _bits(want[name])), name
        for name in ("fold_count", "fold_het", "fold_n_iter", "fold_converged"):
            assert np.array_equal(got[name], want[name]), name
        assert _bits(got["cv_error"]) == _bits(want["cv_error"])
        assert int(got["fold_count"].sum()) == int((c["codes"] != ar.MISSING).sum())
        assert (got["fold_n_iter"] == 3).all() and len(got["fold_ll"]) == folds
        want_cv, want_dev = cr.cv_error(got["fold_ll"], got["fold_count"], got["fold_het"])
        assert got["cv_error"] == want_cv and np.array_equal(_bits(got["fold_deviance"]), _bits(want_dev))
        again = tpg.admix_cv(v, K, folds=folds, cv_seed=9, max_iter=3, tol=0.0, **kw)
        assert _bits(again["cv_error"]) == _bits(got["cv_error"]) and np.array_equal(_bits(again["fold_ll"]), _bits(got["fold_ll"]))
    assert np.array_equal(v.unpack(), c["codes"])


def test_admix_cv_errors_leave_every_output_untouched():
    import tidypopgen_amd as tpg
    from tidypopgen_amd import _lib
    from tidypopgen_amd.api import _ptr

    c = _case(13, 31, 2, 0.1)
    v, n, K = c["v"], 13, 2

    def call(K=K, folds=3, q0=None, ploidy=None, **kw):
        pr = _lib.AdmixParams()
        _lib.lib.tpg_admix_params_default(pr)
        pr.max_iter = 2
        for name, val in kw.items():
            setattr(pr, name, val)
        cv, ll = C.c_double(7.0), np.full(64, 7.0)
        cnt, het = np.full(64, 7, dtype=np.int64), np.full(64, 7, dtype=np.int64)
        nit, conv = np.full(64, 7, dtype=np.int32), np.full(64, 7, dtype=np.int32)
        rc = _lib.lib.tpg_admix_cv(v.ctx.h, v.h, _ptr(ploidy), K, C.byref(pr), folds, 1, _ptr(q0), None, C.byref(cv), _ptr(ll),
                                   _ptr(cnt), _ptr(het), _ptr(nit), _ptr(conv))
        if rc != 0:
            assert cv.value == 7.0 and (ll == 7.0).all() and (cnt == 7).all() and (het == 7).all() and (nit == 7).all() and (conv == 7).all()
        else:
            assert (ll[folds:] == 7.0).all() and (nit[:folds] == 2).all()
        return rc

    assert call(K=33) == EINVAL and call(K=0) == EINVAL
    assert call(folds=1) == EINVAL and call(folds=65) == EINVAL and call(folds=0) == EINVAL
    q = np.asfortranarray(c["Q0"]).copy()
    q[7, 1] = np.nan
    assert call(q0=q) == EINVAL
    assert call(max_iter=-1) == EINVAL and call(tol=-1.0) == EINVAL
    pl = np.full(n, 2.0)
    pl[4] = 1.0
    assert call(ploidy=pl) == EINVAL
    assert call() == 0 and call(q0=np.asfortranarray(c["Q0"]), folds=64) == 0
    with pytest.raises(_lib.TpgError, match=r"folds = 1 out of \[2, 64\]"):
        tpg.admix_cv(v, K, folds=1)
    with pytest.raises(_lib.TpgError, match="K = 33"):
        tpg.admix_cv(v, 33)
    # the per-fold arrays may each be NULL
    pr = _lib.AdmixParams()
    _lib.lib.tpg_admix_params_default(pr)
    pr.max_iter = 1
    cv = C.c_double()
    assert _lib.lib.tpg_admix_cv(v.ctx.h, v.h, None, K, C.byref(pr), 2, 1, None, None, C.byref(cv), None, None, None, None, None) == 0
    assert cv.value > 0


# admix_cv_ref.cross_validate(ar.panel(11, 130, 400, 2, 0.1)[0], K, 5, 1, 42, 300, 1e-4) on a CPU: the numpy EM, float route
NUMPY_CV = {1: 1.3896729303902864, 2: 1.2564088131696918, 3: 1.2840951942523635}
NUMPY_HELD = 46280


def test_cv_error_chooses_the_simulated_k():
    """A panel simulated from two populations: K = 2 has the smallest CV error, on the device as in numpy.  The device and the
    numpy EM run up to 300 chained iterations each with their own roundings and their own stopping iteration, so their CV errors
    are not held to a rounding bound: each must lie within half the smaller gap between the numpy values, (1.28410 - 1.25641) / 2
    = 0.0138, which keeps the order.  Observed on an MI355X: see DESIGN.md 3.10."""
    import tidypopgen_amd as tpg

    codes = ar.panel(11, 130, 400, 2, 0.1)[0]
    big, rows, cols = _embed(codes, 5)
    v = tpg.View(tpg.FBM.from_numpy(np.asfortranarray(big), code256=tpg.CODE_012), rows, cols)
    half_gap = (min(NUMPY_CV[1], NUMPY_CV[3]) - NUMPY_CV[2]) / 2
    assert 0.0138 < half_gap < 0.0139
    cv = {}
    for K in (1, 2, 3):
        r = tpg.admix_cv(v, K, folds=5, cv_seed=1, seed=42, max_iter=300, tol=1e-4)
        cv[K] = r["cv_error"]
        print("cv error K =", K, "device", cv[K], "numpy", NUMPY_CV[K], "device - numpy", cv[K] - NUMPY_CV[K], "iterations per fold",
              r["fold_n_iter"].tolist(), "converged", r["fold_converged"].tolist())
        assert int(r["fold_count"].sum()) == NUMPY_HELD == int((codes != ar.MISSING).sum())
    assert cv[2] < cv[1] and cv[2] < cv[3]
    for K in (1, 2, 3):
        assert abs(cv[K] - NUMPY_CV[K]) < 0.0138


def test_gt_admixture_crossval():
    import tidypopgen_amd as tpg

    c = _case(65, 33, 3, 0.1)
    args = (c["X"], c["rows"], c["cols"])
    out = tpg.gt_admixture(*args, k=[2, 3], n_runs=2, seed=[5, 6, 7, 8], max_iter=6, crossval=True, cv_folds=3, cv_seed=2)
    assert out["k"] == [2, 2, 3, 3] and len(out["cv"]) == 4
    for a, (kk, seed) in enumerate(zip(out["k"], (5, 6, 7, 8))):
        want = tpg.admix_cv(c["v"], kk, folds=3, cv_seed=2, seed=seed, max_iter=6)
        assert _bits(out["cv"][a]) == _bits(want["cv_error"]) and np.isfinite(out["cv"][a]) and out["cv"][a] > 0
    # the defaults: five folds, cv_seed 0
    dflt = tpg.gt_admixture(*args, k=2, seed=[5], max_iter=6, crossval=True)
    assert _bits(dflt["cv"][0]) == _bits(tpg.admix_cv(c["v"], 2, seed=5, max_iter=6)["cv_error"])
    # without crossval: no cv, and the result of the runs is the same, bit for bit
    plain = tpg.gt_admixture(*args, k=[2, 3], n_runs=2, seed=[5, 6, 7, 8], max_iter=6)
    assert sorted(plain) == ["P", "Q", "converged", "k", "loglik", "n_iter"]
    for a, (kk, seed) in enumerate(zip(plain["k"], (5, 6, 7, 8))):
        r = tpg.admix_em(c["v"], kk, seed=seed, max_iter=6)
        for name in ("Q", "P"):
            assert np.array_equal(_bits(plain[name][a]), _bits(r[name])) and np.array_equal(_bits(out[name][a]), _bits(r[name]))
        assert plain["loglik"][a] == r["loglik"] == out["loglik"][a]
        assert plain["n_iter"][a] == r["n_iter"] and plain["converged"][a] == r["converged"]
