"""GPU: admixture by EM (include/tpg.h "admixture") against the numpy restatement tests/admix_ref.py.

What is compared how.  The seeded start: bit for bit.  One step from a given (Q0, F0): every cell of q' and of the unclamped f'
within TWICE the per-cell bounds of the header against the float route (both sides carry the bound against the exact value),
and within the bounds themselves against the exact Fraction route on the two smallest shapes; a cell whose exact value lies
within its bound of eps or 1 - eps may be clamped or not.  Chained steps feed the device's state t into em_step, so that every
iteration is held to the one-step bound and nothing drifts.  Likelihoods: |dl| <= u [(2 T + 2) |l| + 2 (K + 4) T] against
admix_ref.loglik of the same state.  Every view is a row / column subset of a larger
store."""
from fractions import Fraction

import numpy as np
import pytest

from tests import admix_ref as ar

pytestmark = pytest.mark.gpu


def _chunk():
    from tidypopgen_amd import api

    return api.ADMIX_CHUNK_LOCI


def _embed(codes, seed):
    """the panel as rows / columns of a larger store: -> bytes, ind_row, ind_col (1-based)"""
    n, m = codes.shape
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.permutation(n + 3)[:n])
    cols = np.sort(rng.permutation(m + 5)[:m])
    big = rng.integers(0, 4, size=(n + 3, m + 5)).astype(np.uint8)
    big[np.ix_(rows, cols)] = codes
    return big, rows + 1, cols + 1


_CASES = {}


def _case(n, m, K, miss):
    """codes, planted, the view, a given start (normalised / clamped as the library will), shared by the tests"""
    import tidypopgen_amd as tpg

    m = _chunk() + 1 if m == "chunk+1" else m
    key = (n, m, K, miss)
    if key not in _CASES:
        codes, _, _, planted = ar.panel(1000 + n + m + K, n, m, K, miss)
        big, rows, cols = _embed(codes, n + m)
        X = tpg.FBM.from_numpy(np.asfortranarray(big), code256=tpg.CODE_012)
        v = tpg.View(X, rows, cols)
        rng = np.random.default_rng(n * m + K)
        Q0 = rng.uniform(0.05, 1.0, size=(n, K))
        F0 = rng.uniform(0.02, 0.98, size=(m, K))
        _CASES[key] = dict(codes=codes, planted=planted, X=X, v=v, rows=rows, cols=cols, big=big, Q0=Q0, F0=F0,
                           Qs=ar.normalise_q(Q0), Fs=ar.clamp(F0), n=n, m=m, K=K)
    return _CASES[key]


# every value of each axis, and the (130, chunk + 1, 32) corner
SHAPES = [(13, 1, 1, 0.0), (13, 31, 2, 0.1), (65, 33, 3, 0.1), (65, 129, 8, 0.0), (130, 129, 32, 0.1), (13, "chunk+1", 3, 0.1),
          (130, "chunk+1", 32, 0.1)]
SMALL = [(13, 1, 1, 0.0), (13, 31, 2, 0.1)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_step(c, Qa, Fa, Qb, Fb, factor=2.0):
    """the device's (Qb, Fb) is one step from (Qa, Fa): within factor x the per-cell bounds of the float route"""
    codes, n, K = c["codes"], c["n"], c["K"]
    q_ref, f_ref, f_raw = ar.em_step(codes, Qa, Fa)
    t_i = (codes != ar.MISSING).sum(axis=1)
    assert (np.abs(Qb - q_ref) <= factor * ar.bound_q(t_i, K, q_ref)).all()
    bf = factor * ar.bound_f(n, K, f_raw)
    ok = np.abs(Fb - f_raw) <= bf
    # clamped cells: the device's unclamped value is not visible; the clamp applies where the raw value is beyond (or within its
    # bound of) the edge
    lo, hi = (Fb == ar.EPS) & (f_raw <= ar.EPS + bf), (Fb == 1 - ar.EPS) & (f_raw >= 1 - ar.EPS - bf)
    assert (ok | lo | hi).all()
    assert (Fb >= ar.EPS).all() and (Fb <= 1 - ar.EPS).all()


@pytest.mark.parametrize("n,m,K,miss", SHAPES)
def test_seeded_start_is_the_hash_start_bit_for_bit(n, m, K, miss):
    import tidypopgen_amd as tpg

    c = _case(n, m, K, miss)
    for seed in (0, 0xDEADBEEFCAFEF00D):
        r = tpg.admix_em(c["v"], K, seed=seed, max_iter=0, return_trace=True)
        Q0, F0 = ar.start(seed, n, c["m"], K)
        assert np.array_equal(_bits(r["Q"]), _bits(Q0)) and np.array_equal(_bits(r["P"]), _bits(F0))
        assert r["n_iter"] == 0 and not r["converged"] and len(r["trace"]) == 1 and r["trace"][0] == r["loglik"]
        T = int((c["codes"] != ar.MISSING).sum())
        ll = ar.loglik(c["codes"], Q0, F0)
        print("loglik", n, c["m"], K, r["loglik"], ll, abs(r["loglik"] - ll), ar.bound_ll(T, K, ll))
        assert abs(r["loglik"] - ll) <= ar.bound_ll(T, K, ll)


@pytest.mark.parametrize("n,m,K,miss", SHAPES)
def test_one_step_from_a_given_start(n, m, K, miss):
    import tidypopgen_amd as tpg

    c = _case(n, m, K, miss)
    r = tpg.admix_em(c["v"], K, Q0=c["Q0"], F0=c["F0"], max_iter=1)
    assert r["n_iter"] == 1
    _check_step(c, c["Qs"], c["Fs"], r["Q"], r["P"])
    pl = c["planted"]
    if pl["col_missing"] is not None:
        assert np.array_equal(_bits(r["P"][pl["col_missing"]]), _bits(c["Fs"][pl["col_missing"]]))
        assert (r["P"][pl["col_all0"]] == ar.EPS).all() and (r["P"][pl["col_all2"]] == 1 - ar.EPS).all()
    if pl["row_missing"] is not None:
        assert np.array_equal(_bits(r["Q"][pl["row_missing"]]), _bits(c["Qs"][pl["row_missing"]]))
    typed_rows = (c["codes"] != ar.MISSING).any(axis=1)
    assert np.allclose(r["Q"][typed_rows].sum(axis=1), 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("n,m,K,miss", SMALL)
def test_one_step_against_the_exact_route(n, m, K, miss):
    import tidypopgen_amd as tpg

    c = _case(n, m, K, miss)
    r = tpg.admix_em(c["v"], K, Q0=c["Q0"], F0=c["F0"], max_iter=1)
    qx, fx = ar.em_step_exact(c["codes"], c["Qs"], c["Fs"])
    t_i = (c["codes"] != ar.MISSING).sum(axis=1)
    for i in range(n):
        for k in range(K):
            assert abs(Fraction(float(r["Q"][i, k])) - qx[i][k]) <= Fraction((2 * int(t_i[i]) + 2 * K + 16)) * qx[i][k] / 2 ** 52
    for j in range(c["m"]):
        for k in range(K):
            b = Fraction(2 * n + 4 * K + 40) * fx[j][k] / 2 ** 52
            got = Fraction(float(r["P"][j, k]))
            lo, hi = Fraction(ar.EPS), Fraction(1 - ar.EPS)
            assert abs(got - fx[j][k]) <= b or (got == lo and fx[j][k] <= lo + b) or (got == hi and fx[j][k] >= hi - b)


@pytest.mark.parametrize("n,m", [(13, 31), (65, 129), (130, 33)])
def test_k1_gives_the_alt_allele_frequency(n, m):
    """From f = 1 / 2 the weights g / f and (2 - g) / (1 - f) are whole numbers, every sum of the step is exact, and P differs
    from n_alt / n_valid by the division and the add the issue counts: 4 u relative.  From the seeded start the weights are
    rounded quotients and their sums carry the one-step bound of the header instead; that figure is printed and held to it."""
    import tidypopgen_amd as tpg

    c = _case(n, m, 1, 0.1)
    af = tpg.alt_freq_dip_pseudo_cpp(c["v"], np.full(n, 2.0), as_counts=True)  # n_alt, n_valid
    typed = af[:, 1] > 0
    freq = af[typed, 0] / af[typed, 1]
    want = ar.clamp(freq)
    r = tpg.admix_em(c["v"], 1, Q0=np.ones((n, 1)), F0=np.full((m, 1), 0.5), max_iter=1)
    got = r["P"][typed, 0]
    err = np.abs(got - want) / want
    print("K = 1 from f = 1/2: max relative error in u", n, m, err.max() / ar.U)
    assert (err <= 4 * ar.U).all()
    assert np.array_equal(r["P"][~typed, 0], np.full((~typed).sum(), 0.5))
    r = tpg.admix_em(c["v"], 1, seed=3, max_iter=1)
    got = r["P"][typed, 0]
    inside = (freq > ar.EPS) & (freq < 1 - ar.EPS)
    err = np.abs(got - want)[inside] / want[inside]
    print("K = 1 from the seeded start: max relative error in u", n, m, err.max() / ar.U)
    assert (err <= (2 * n + 4 + 40) * ar.U).all()
    assert (got[~inside] == want[~inside]).all()
    assert np.allclose(r["Q"][(c["codes"] != ar.MISSING).any(axis=1)], 1.0, rtol=0, atol=1e-13)


@pytest.mark.parametrize("n,m,K,miss", [(65, 33, 3, 0.1), (130, 129, 8, 0.1), (13, "chunk+1", 3, 0.1)])
def test_chained_steps_each_within_the_one_step_bound(n, m, K, miss):
    import tidypopgen_amd as tpg

    c = _case(n, m, K, miss)
    T = int((c["codes"] != ar.MISSING).sum())
    Qa, Fa = c["Qs"], c["Fs"]
    r = tpg.admix_em(c["v"], K, Q0=c["Q0"], F0=c["F0"], max_iter=5, tol=0.0, return_trace=True)
    assert r["n_iter"] == 5 and len(r["trace"]) == 6
    for t in range(5):
        s = tpg.admix_em(c["v"], K, Q0=c["Q0"], F0=c["F0"], max_iter=t + 1, tol=0.0)
        ll = ar.loglik(c["codes"], Qa, Fa)
        assert abs(r["trace"][t] - ll) <= ar.bound_ll(T, K, ll)
        _check_step(c, Qa, Fa, s["Q"], s["P"])
        Qa, Fa = s["Q"], s["P"]  # the device's state t + 1 goes into the next step
    assert np.array_equal(_bits(Qa), _bits(r["Q"])) and np.array_equal(_bits(Fa), _bits(r["P"]))
    ll = ar.loglik(c["codes"], Qa, Fa)
    assert abs(r["loglik"] - ll) <= ar.bound_ll(T, K, ll) and r["loglik"] == r["trace"][5]
    assert abs(tpg.admix_loglik(c["v"], Qa, Fa) - ll) <= ar.bound_ll(T, K, ll)
    assert tpg.admix_loglik(c["v"], Qa, Fa) == r["loglik"]


def test_trace_does_not_decrease_on_a_simulated_panel():
    import tidypopgen_amd as tpg

    n, m, K, max_iter, tol = 130, 2000, 3, 200, 1e-4
    c = _case(n, m, K, 0.1)
    T = int((c["codes"] != ar.MISSING).sum())
    r = tpg.admix_em(c["v"], K, seed=11, max_iter=max_iter, tol=tol, return_trace=True)
    tr = r["trace"]
    assert len(tr) == r["n_iter"] + 1 and np.isfinite(tr).all()
    for t in range(1, len(tr)):
        assert tr[t] >= tr[t - 1] - ar.bound_ll(T, K, tr[t - 1])
    t = r["n_iter"]
    if r["converged"]:
        assert t >= 2 and tr[t - 1] - tr[t - 2] < tol
        assert all(not (tr[s - 1] - tr[s - 2] < tol) for s in range(2, t))  # and at no earlier iteration
    else:
        assert t == max_iter
    assert tr[-1] > tr[0]
    ll = ar.loglik(c["codes"], r["Q"], r["P"])
    assert abs(r["loglik"] - ll) <= ar.bound_ll(T, K, ll)
    assert abs(tpg.admix_loglik(c["v"], r["Q"], r["P"]) - ll) <= ar.bound_ll(T, K, ll)


def test_projection_keeps_the_fixed_half_bit_for_bit():
    import tidypopgen_amd as tpg

    c = _case(65, 129, 8, 0.0)
    K = 8
    r = tpg.admix_em(c["v"], K, Q0=c["Q0"], F0=c["F0"], max_iter=3, tol=0.0, update_f=False)
    assert np.array_equal(_bits(r["P"]), _bits(c["Fs"])) and not np.array_equal(r["Q"], c["Qs"])
    q1 = ar.em_step(c["codes"], c["Qs"], c["Fs"])[0]
    one = tpg.admix_em(c["v"], K, Q0=c["Q0"], F0=c["F0"], max_iter=1, update_f=False)
    t_i = (c["codes"] != ar.MISSING).sum(axis=1)
    assert (np.abs(one["Q"] - q1) <= 2 * ar.bound_q(t_i, K, q1)).all()
    r = tpg.admix_em(c["v"], K, Q0=c["Q0"], F0=c["F0"], max_iter=3, tol=0.0, update_q=False)
    assert np.array_equal(_bits(r["Q"]), _bits(c["Qs"])) and not np.array_equal(r["P"], c["Fs"])
    r = tpg.admix_em(c["v"], K, Q0=c["Q0"], F0=c["F0"], max_iter=3, tol=0.0, update_q=False, update_f=False)
    assert np.array_equal(_bits(r["Q"]), _bits(c["Qs"])) and np.array_equal(_bits(r["P"]), _bits(c["Fs"])) and r["n_iter"] >= 2


@pytest.mark.parametrize("n,m,K,miss", [(65, 129, 8, 0.0), (130, "chunk+1", 32, 0.1)])
def test_two_calls_block_plans_and_device_starts_give_the_same_bits(n, m, K, miss):
    import tidypopgen_amd as tpg

    c = _case(n, m, K, miss)
    v, ctx = c["v"], c["v"].ctx
    a = tpg.admix_em(v, K, Q0=c["Q0"], F0=c["F0"], max_iter=3, tol=0.0, return_trace=True)
    b = tpg.admix_em(v, K, Q0=c["Q0"], F0=c["F0"], max_iter=3, tol=0.0, return_trace=True)
    for name in ("Q", "P", "trace"):
        assert np.array_equal(_bits(a[name]), _bits(b[name]))
    # the same view over a store uploaded in column blocks
    big = np.asfortranarray(c["big"])
    X2 = tpg.FBM.alloc(big.shape[0], big.shape[1], ctx=ctx, code256=tpg.CODE_012)
    step = 37
    for c0 in range(0, big.shape[1], step):
        X2.upload_cols(np.asfortranarray(big[:, c0:c0 + step]), c0)
    v2 = tpg.View(X2, c["rows"], c["cols"])
    assert np.array_equal(v2.unpack(), c["codes"])
    b = tpg.admix_em(v2, K, Q0=c["Q0"], F0=c["F0"], max_iter=3, tol=0.0, return_trace=True)
    for name in ("Q", "P", "trace"):
        assert np.array_equal(_bits(a[name]), _bits(b[name]))
    # Q0 / F0 in device memory
    q0, f0 = np.asfortranarray(c["Q0"]), np.asfortranarray(c["F0"])
    dq, df = ctx.dev_alloc(q0.nbytes), ctx.dev_alloc(f0.nbytes)
    try:
        from tidypopgen_amd._lib import check, lib
        import ctypes as C

        check(lib.tpg_dev_from_host(ctx.h, dq, C.c_void_p(q0.ctypes.data), C.c_size_t(q0.nbytes)))
        check(lib.tpg_dev_from_host(ctx.h, df, C.c_void_p(f0.ctypes.data), C.c_size_t(f0.nbytes)))
        b = tpg.admix_em(v, K, Q0=int(dq.value), F0=int(df.value), max_iter=3, tol=0.0, return_trace=True)
    finally:
        ctx.dev_free(dq)
        ctx.dev_free(df)
    for name in ("Q", "P", "trace"):
        assert np.array_equal(_bits(a[name]), _bits(b[name]))


def test_errors_leave_q_and_p_untouched():
    import ctypes as C

    import tidypopgen_amd as tpg
    from tidypopgen_amd import _lib
    from tidypopgen_amd.api import _ptr

    c = _case(13, 31, 2, 0.1)
    v, n, m, K = c["v"], 13, 31, 2

    def call(K=K, q0=None, f0=None, ploidy=None, view=v, nn=n, mm=m, **kw):
        pr = _lib.AdmixParams()
        _lib.lib.tpg_admix_params_default(pr)
        for name, val in kw.items():
            setattr(pr, name, val)
        Q, P = np.full((nn, 40), 7.0, order="F"), np.full((mm, 40), 7.0, order="F")
        rc = _lib.lib.tpg_admix_em(view.ctx.h, view.h, _ptr(ploidy), C.c_int(K), C.byref(pr), _ptr(q0), _ptr(f0), _ptr(Q), _ptr(P),
                                   None, None, None, None)
        assert (Q == 7.0).all() and (P == 7.0).all()
        return rc

    EINVAL = 1
    q0, f0 = np.asfortranarray(c["Q0"]), np.asfortranarray(c["F0"])
    assert call(K=0) == EINVAL and call(K=-1) == EINVAL and call(K=33) == EINVAL
    assert call(max_iter=-1) == EINVAL and call(tol=-1e-9) == EINVAL and call(tol=float("nan")) == EINVAL
    pl = np.full(n, 2.0)
    pl[5] = 1.0
    assert call(ploidy=pl) == EINVAL
    for bad in (np.nan, np.inf, 0.0, -0.25):
        q = q0.copy()
        q[7, 1] = bad
        assert call(q0=q, f0=f0) == EINVAL and call(q0=q) == EINVAL
    for bad in (np.nan, -np.inf):
        f = f0.copy()
        f[30, 0] = bad
        assert call(q0=q0, f0=f) == EINVAL and call(f0=f) == EINVAL
    # the Python layer raises what the library answers
    with pytest.raises(_lib.TpgError, match="K = 33"):
        tpg.admix_em(v, 33)
    with pytest.raises(_lib.TpgError, match="not finite or not positive"):
        q = q0.copy()
        q[0, 0] = 0.0
        tpg.admix_em(v, K, Q0=q)
    # a view without loci or without individuals cannot be made (tpg_view_create refuses it), so the library's own N = 0 /
    # M = 0 answer has no route to it from here
    for rows, cols in ((c["rows"], c["cols"][:0]), (c["rows"][:0], c["cols"])):
        with pytest.raises(_lib.TpgError, match="empty view"):
            tpg.View(c["X"], rows, cols)
    # all good: the same call succeeds and writes
    r = tpg.admix_em(v, K, Q0=q0, F0=f0, max_iter=1, ploidy=np.full(n, 2.0))
    assert np.isfinite(r["Q"]).all() and np.isfinite(r["P"]).all()


def test_gt_admixture_shapes_and_seed_rule():
    import tidypopgen_amd as tpg

    c = _case(65, 129, 3, 0.1)
    n, m = 65, 129
    out = tpg.gt_admixture(c["X"], c["rows"], c["cols"], k=[2, 3], n_runs=2, seed=[5, 6, 7, 8], max_iter=20)
    assert out["k"] == [2, 2, 3, 3]
    for name in ("Q", "P", "loglik", "n_iter", "converged"):
        assert len(out[name]) == 4
    for a, kk in enumerate(out["k"]):
        assert out["Q"][a].shape == (n, kk) and out["P"][a].shape == (m, kk) and np.isfinite(out["loglik"][a])
        assert 1 <= out["n_iter"][a] <= 20
    # the seeds are used run by run: run 1 equals a direct call with seed 6
    r = tpg.admix_em(c["v"], 2, seed=6, max_iter=20)
    assert np.array_equal(_bits(out["Q"][1]), _bits(r["Q"])) and out["loglik"][1] == r["loglik"]
    two = tpg.gt_admixture(c["X"], c["rows"], c["cols"], k=[2, 3], n_runs=2, seed=[5, 6], max_iter=2)
    assert two["k"] == [2, 2, 3, 3]
    one = tpg.gt_admixture(c["X"], c["rows"], c["cols"], k=2, max_iter=2)
    assert one["k"] == [2] and one["Q"][0].shape == (n, 2)
    with pytest.raises(ValueError, match=r"'seed' should be a vector of length 'n_runs' OR 'n_runs' \* length\(k\)"):
        tpg.gt_admixture(c["X"], c["rows"], c["cols"], k=[2, 3], n_runs=2, seed=[1, 2, 3])
