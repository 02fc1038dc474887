"""GPU: the accelerated admixture EM (include/tpg.h "admixture, accelerated") against the numpy restatement
tests/admix_squarem_ref.py.

What is compared how.  The point primitive (steps 3 to 7 for given theta0, theta1, theta2): sr and sv within the bounds of the
header of the exact Fraction sums on the two smallest shapes, within TWICE the bounds of the float route on the rest (both sides
carry the bound); alpha bit for bit from the returned sums; theta' raw bit for bit from the returned alpha (an exact fused
multiply-add on the host); the projection bit for bit from the returned raw.  The driver: every state is fed back into
admix_ref.em_step, so each EM step is held to the one-step bounds of "admixture" and nothing drifts; alpha of every cycle equals
the point primitive's on the device's own three states; a cycle is accepted exactly when its own trace says so."""
import ctypes as C

import numpy as np
import pytest

from fractions import Fraction

from tests import admix_ref as ar
from tests import admix_squarem_ref as sq
from tests.test_gpu_admix import _bits, _case, _check_step, _embed

pytestmark = pytest.mark.gpu

_STATES = {}


def _states(n, m, K, miss):
    """theta0 (a given start as the library normalises / clamps it), theta1, theta2 from admix_ref.em_step, computed once"""
    c = _case(n, m, K, miss)
    key = (n, c["m"], K, miss)
    if key not in _STATES:
        Q1, F1, _ = ar.em_step(c["codes"], c["Qs"], c["Fs"])
        Q2, F2, _ = ar.em_step(c["codes"], Q1, F1)
        _STATES[key] = (c["Qs"], c["Fs"], Q1, F1, Q2, F2)
    return c, _STATES[key]


def _check_point(th, got, a_max, update_q, update_f, exact):
    Q0, F0, Q1, F1, Q2, F2 = th
    sr, sv, nn = sq.sums(*th, update_q, update_f)
    if exact:
        xr, xv = sq.sums_exact(*th, update_q, update_f)
        dr, dv = abs(float(Fraction(got["sr"]) - xr)), abs(float(Fraction(got["sv"]) - xv))
        br, bv = sq.bound_sr(nn, xr), sq.bound_sv(*th, xv, update_q, update_f)
    else:
        dr, dv = abs(got["sr"] - sr), abs(got["sv"] - sv)
        br, bv = 2 * sq.bound_sr(nn, sr), 2 * sq.bound_sv(*th, sv, update_q, update_f)
    print("sr", got["sr"], dr, br, "sv", got["sv"], dv, bv, "alpha", got["alpha"], "entries", nn, "exact" if exact else "float")
    assert dr <= br and dv <= bv
    # alpha from the returned sums, bit for bit
    assert _bits(got["alpha"])[0] == _bits(sq.alpha_of(got["sr"], got["sv"], a_max)[0])[0]
    assert -a_max <= got["alpha"] <= -1.0
    # theta' raw from the returned alpha, the projection from the returned raw, bit for bit; a half not updated is theta0
    if update_q:
        assert np.array_equal(_bits(got["Q_raw"]), _bits(sq.raw(Q0, Q1, Q2, got["alpha"])))
        assert np.array_equal(_bits(got["Q"]), _bits(sq.project_q(got["Q_raw"], Q0, Q1, Q2)))
    else:
        assert np.array_equal(_bits(got["Q_raw"]), _bits(Q0)) and np.array_equal(_bits(got["Q"]), _bits(Q0))
    if update_f:
        assert np.array_equal(_bits(got["P_raw"]), _bits(sq.raw(F0, F1, F2, got["alpha"])))
        assert np.array_equal(_bits(got["P"]), _bits(sq.project_f(got["P_raw"], F0, F1, F2)))
        assert (got["P"] >= ar.EPS).all() and (got["P"] <= 1 - ar.EPS).all()
    else:
        assert np.array_equal(_bits(got["P_raw"]), _bits(F0)) and np.array_equal(_bits(got["P"]), _bits(F0))
    moved = sq._moved(Q0, Q1, Q2)
    assert np.allclose(got["Q"][moved].sum(axis=1), 1.0, rtol=0, atol=1e-12) and (got["Q"] > 0).all()


# K = 5 pads the state to 8 columns; the two smallest shapes are held to the exact sums
POINT = [(13, 31, 3, 0.1, True, True, True), (65, 129, 8, 0.0, True, True, True), (13, 31, 5, 0.1, True, True, False),
         (130, "chunk+1", 32, 0.1, True, True, False), (65, 129, 8, 0.0, False, True, False), (65, 129, 8, 0.0, True, False, False)]


@pytest.mark.parametrize("n,m,K,miss,update_q,update_f,exact", POINT)
def test_point_sums_alpha_raw_and_projection(n, m, K, miss, update_q, update_f, exact):
    import tidypopgen_amd as tpg

    c, th = _states(n, m, K, miss)
    for a_max in (4.0, 1.0):
        got = tpg.admix_squarem_point(*th, a_max=a_max, update_q=update_q, update_f=update_f, ctx=c["v"].ctx)
        _check_point(th, got, a_max, update_q, update_f, exact and a_max == 4.0)
    # the individual and the locus typed nowhere did not move: theta0, bit for bit
    pl = c["planted"]
    if pl["row_missing"] is not None and pl["col_missing"] is not None:
        i, j = pl["row_missing"], pl["col_missing"]
        assert np.array_equal(_bits(got["Q"][i]), _bits(th[0][i])) and np.array_equal(_bits(got["P"][j]), _bits(th[1][j]))
    again = tpg.admix_squarem_point(*th, a_max=a_max, update_q=update_q, update_f=update_f, ctx=c["v"].ctx)
    for name in ("Q", "P", "Q_raw", "P_raw"):
        assert np.array_equal(_bits(again[name]), _bits(got[name]))
    assert (again["sr"], again["sv"], again["alpha"]) == (got["sr"], got["sv"], got["alpha"])


@pytest.mark.parametrize("n,m,K,miss", [(13, 31, 3, 0.1), (13, 31, 5, 0.1), (65, 129, 8, 0.0)])
def test_point_projection_of_a_raw_state_outside_the_feasible_set(n, m, K, miss):
    """theta2 - theta1 = 0.98 r: v = -0.02 r, alpha near -50 under a limit of 64, theta' raw near theta0 + 50 r"""
    import tidypopgen_amd as tpg

    c, (Q0, F0, Q1, F1, _, _) = _states(n, m, K, miss)
    th = (Q0, F0, Q1, F1, Q1 + 0.98 * (Q1 - Q0), F1 + 0.98 * (F1 - F0))
    got = tpg.admix_squarem_point(*th, a_max=64.0, ctx=c["v"].ctx)
    assert -51.0 < got["alpha"] < -49.0
    assert (got["Q_raw"] < 0).any() and (got["P_raw"] < 0).any() and (got["P_raw"] > 1).any()
    _check_point(th, got, 64.0, True, True, False)
    assert (got["P"] == ar.EPS).any() and (got["P"] == 1 - ar.EPS).any()
    # and clipped at the limit
    got = tpg.admix_squarem_point(*th, a_max=16.0, ctx=c["v"].ctx)
    assert got["alpha"] == -16.0
    _check_point(th, got, 16.0, True, True, False)


def test_point_degenerate_sums_give_a_plain_step():
    import tidypopgen_amd as tpg

    c, (Q0, F0, Q1, F1, _, _) = _states(13, 31, 3, 0.1)
    ctx = c["v"].ctx
    # nothing moved: sr = sv = 0, alpha = -1, theta' = theta0 as given
    got = tpg.admix_squarem_point(Q0, F0, Q0, F0, Q0, F0, ctx=ctx)
    assert (got["sr"], got["sv"], got["alpha"]) == (0.0, 0.0, -1.0)
    assert np.array_equal(_bits(got["Q"]), _bits(Q0)) and np.array_equal(_bits(got["P"]), _bits(F0))
    # a linear move: v = 0 exactly (steps of 2^-10 from multiples of 2^-10), sv = 0, alpha = -1, theta' raw = theta2
    Qa, Fa = np.round(Q0 * 1024) / 1024 + 0.25, np.round(F0 * 512) / 1024 + 0.125
    d = 2.0 ** -10
    got = tpg.admix_squarem_point(Qa, Fa, Qa + d, Fa + d, Qa + 2 * d, Fa + 2 * d, ctx=ctx)
    assert got["sv"] == 0.0 and got["sr"] == (Q0.size + F0.size) * d * d and got["alpha"] == -1.0
    assert np.array_equal(_bits(got["Q_raw"]), _bits(Qa + 2 * d)) and np.array_equal(_bits(got["P_raw"]), _bits(Fa + 2 * d))


def _run(tpg, c, K, max_iter, **kw):
    return tpg.admix_em(c["v"], K, Q0=c["Q0"], F0=c["F0"], max_iter=max_iter, tol=0.0, return_trace=True, accel="squarem", **kw)


def _verify_cycles(tpg, c, K, ncycles, update_q=True, update_f=True):
    """every EM step and every extrapolation of ncycles cycles from the given start, on the device's own states"""
    codes = c["codes"]
    T = int((codes != ar.MISSING).sum())
    kw = dict(update_q=update_q, update_f=update_f)
    full = _run(tpg, c, K, 3 * ncycles, **kw)
    assert full["n_iter"] == 3 * ncycles and full["n_cycles"] == ncycles and len(full["trace"]) == 3 * ncycles + 1
    assert len(full["alpha"]) == ncycles and len(full["accepted"]) == ncycles and full["n_rejected"] == int((~full["accepted"]).sum())
    at = {t: _run(tpg, c, K, t, **kw) for t in range(3 * ncycles)}  # the state after t steps: a run is a prefix of a longer one
    at[3 * ncycles] = full
    for t, s in at.items():
        assert s["n_iter"] == t and not s["converged"] and s["n_cycles"] == t // 3
        assert np.array_equal(_bits(s["trace"][:t]), _bits(full["trace"][:t]))
        assert s["trace"][t] == s["loglik"]
    assert np.array_equal(_bits(at[0]["Q"]), _bits(c["Qs"])) and np.array_equal(_bits(at[0]["P"]), _bits(c["Fs"]))

    def one_step(a, b):
        q_ref, f_ref, _ = ar.em_step(codes, a["Q"], a["P"])
        if update_q and update_f:
            _check_step(c, a["Q"], a["P"], b["Q"], b["P"])
        elif update_q:
            t_i = (codes != ar.MISSING).sum(axis=1)
            assert (np.abs(b["Q"] - q_ref) <= 2 * ar.bound_q(t_i, K, q_ref)).all() and np.array_equal(_bits(b["P"]), _bits(a["P"]))
        else:
            _check_step(c, a["Q"], a["P"], q_ref, b["P"])
            assert np.array_equal(_bits(b["Q"]), _bits(a["Q"]))

    def ll_ok(value, Q, P):
        ll = ar.loglik(codes, Q, P)
        assert abs(value - ll) <= ar.bound_ll(T, K, ll)

    a_max = 4.0
    for cyc in range(ncycles):
        th0, th1, th2, nxt = at[3 * cyc], at[3 * cyc + 1], at[3 * cyc + 2], at[3 * cyc + 3]
        one_step(th0, th1)
        one_step(th1, th2)
        tr = full["trace"][3 * cyc: 3 * cyc + 3]
        ll_ok(tr[0], th0["Q"], th0["P"])
        ll_ok(tr[1], th1["Q"], th1["P"])
        p = tpg.admix_squarem_point(th0["Q"], th0["P"], th1["Q"], th1["P"], th2["Q"], th2["P"], a_max=a_max, update_q=update_q,
                                    update_f=update_f, ctx=c["v"].ctx)
        assert _bits(full["alpha"][cyc])[0] == _bits(p["alpha"])[0]
        ll_ok(tr[2], p["Q"], p["P"])  # l(theta'): the state the third step was applied to
        ok = bool(np.isfinite(tr[2]) and tr[2] >= tr[1])
        assert bool(full["accepted"][cyc]) == ok
        print("cycle", cyc, "alpha", p["alpha"], "a_max", a_max, "accepted", ok, "l", tr.tolist())
        if ok:
            one_step(dict(Q=p["Q"], P=p["P"]), nxt)  # theta'' is one step from theta'
        else:
            assert np.array_equal(_bits(nxt["Q"]), _bits(th2["Q"])) and np.array_equal(_bits(nxt["P"]), _bits(th2["P"]))
        a_max = sq.next_limit(a_max, ok, sq.alpha_of(p["sr"], p["sv"], a_max)[1])
    ll_ok(full["loglik"], full["Q"], full["P"])
    return full, at


@pytest.mark.parametrize("n,m,K,miss", [(65, 33, 3, 0.1), (13, 31, 5, 0.1), (130, 129, 8, 0.1), (13, "chunk+1", 3, 0.1)])
def test_one_cycle_through_the_driver(n, m, K, miss):
    import tidypopgen_amd as tpg

    c = _case(n, m, K, miss)
    full, at = _verify_cycles(tpg, c, K, 1)
    # the first two steps are plain EM steps: the same sweeps, the same bits
    for t in (1, 2):
        plain = tpg.admix_em(c["v"], K, Q0=c["Q0"], F0=c["F0"], max_iter=t, tol=0.0, return_trace=True)
        assert np.array_equal(_bits(plain["Q"]), _bits(at[t]["Q"])) and np.array_equal(_bits(plain["P"]), _bits(at[t]["P"]))
        assert np.array_equal(_bits(plain["trace"]), _bits(at[t]["trace"]))


@pytest.mark.parametrize("n,m,K,miss,update_q,update_f", [(65, 33, 3, 0.1, True, True), (130, 129, 8, 0.1, True, True),
                                                           (65, 129, 8, 0.0, True, False), (65, 129, 8, 0.0, False, True)])
def test_three_chained_cycles(n, m, K, miss, update_q, update_f):
    import tidypopgen_amd as tpg

    c = _case(n, m, K, miss)
    full, _ = _verify_cycles(tpg, c, K, 3, update_q, update_f)
    if not update_q:
        assert np.array_equal(_bits(full["Q"]), _bits(c["Qs"]))
    if not update_f:
        assert np.array_equal(_bits(full["P"]), _bits(c["Fs"]))


@pytest.mark.parametrize("max_iter", [1, 2, 4, 5])
def test_max_iter_inside_a_cycle_returns_the_last_state_a_step_produced(max_iter):
    import tidypopgen_amd as tpg

    c = _case(65, 33, 3, 0.1)
    K = 3
    r = _run(tpg, c, K, max_iter)
    assert r["n_iter"] == max_iter and len(r["trace"]) == max_iter + 1 and r["n_cycles"] == max_iter // 3 and not r["converged"]
    assert len(r["alpha"]) == r["n_cycles"]
    if max_iter <= 2:  # theta1, theta2 of the first cycle: plain EM steps
        plain = tpg.admix_em(c["v"], K, Q0=c["Q0"], F0=c["F0"], max_iter=max_iter, tol=0.0)
        assert np.array_equal(_bits(plain["Q"]), _bits(r["Q"])) and np.array_equal(_bits(plain["P"]), _bits(r["P"]))
    else:  # theta1, theta2 of the second cycle: one step from the state one step earlier
        before = _run(tpg, c, K, max_iter - 1)
        _check_step(c, before["Q"], before["P"], r["Q"], r["P"])
        assert np.array_equal(_bits(before["trace"][:max_iter - 1]), _bits(r["trace"][:max_iter - 1]))
    # max_iter = 0: the start and its likelihood
    z = _run(tpg, c, K, 0)
    assert z["n_iter"] == 0 and z["n_cycles"] == 0 and len(z["trace"]) == 1 and z["trace"][0] == z["loglik"]
    assert np.array_equal(_bits(z["Q"]), _bits(c["Qs"])) and np.array_equal(_bits(z["P"]), _bits(c["Fs"]))


# the numpy restatement on panel(3, 65, 600, 2, 0.05), seeded start 3, tol = 1e-4 (tests/test_admix_squarem_host.py prints it):
# plain 562 steps, loglik -41548.653420034694; accelerated 161 steps, loglik -41548.64617527104; |gap| = 0.007244763655762654
NUMPY_GAP = 0.007244763655762654
MARGIN = 10 * NUMPY_GAP


def test_convergence_in_at_most_half_the_em_steps():
    """panel(3, 65, 600, 2, 0.05), seeded start 3, tol = 1e-4, max_iter = 3000.  Both runs converge; the accelerated one takes at
    most half the EM steps of the plain one (the restatement: 161 against 562); its loglik is at most MARGIN below the plain one,
    MARGIN = 10 x the |gap| between the restatement's own two runs at this shape, measured as 0.0072448 (the accelerated run
    ended HIGHER there), so MARGIN = 0.072448; the likelihoods at the starts of the cycles do not decrease beyond bound_ll."""
    import tidypopgen_amd as tpg

    n, m, K = 65, 600, 2
    codes = ar.panel(3, n, m, K, 0.05)[0]
    big, rows, cols = _embed(codes, 17)
    v = tpg.View(tpg.FBM.from_numpy(np.asfortranarray(big), code256=tpg.CODE_012), rows, cols)
    T = int((codes != ar.MISSING).sum())
    plain = tpg.admix_em(v, K, seed=3, tol=1e-4, max_iter=3000)
    acc = tpg.admix_em(v, K, seed=3, tol=1e-4, max_iter=3000, accel="squarem", return_trace=True)
    print("plain", plain["n_iter"], plain["loglik"], "accelerated", acc["n_iter"], acc["loglik"], "cycles", acc["n_cycles"], "rejected",
          acc["n_rejected"], "min alpha", acc["alpha"].min() if acc["n_cycles"] else None, "plain - accelerated",
          plain["loglik"] - acc["loglik"], "margin", MARGIN)
    assert plain["converged"] and acc["converged"]
    assert acc["n_iter"] <= 0.5 * plain["n_iter"]
    assert acc["loglik"] >= plain["loglik"] - MARGIN
    tr = acc["trace"]
    assert len(tr) == acc["n_iter"] + 1 and np.isfinite(tr[[0, -1]]).all()
    # the run ended by the stop rule inside a cycle: two steps after the last whole cycle
    assert acc["n_iter"] == 3 * acc["n_cycles"] + 2 and tr[-2] - tr[-3] < 1e-4
    starts = tr[0: 3 * acc["n_cycles"] + 1: 3]
    for a, b in zip(starts, starts[1:]):
        assert b >= a - ar.bound_ll(T, K, a)
    for cyc in range(acc["n_cycles"]):
        assert bool(acc["accepted"][cyc]) == bool(np.isfinite(tr[3 * cyc + 2]) and tr[3 * cyc + 2] >= tr[3 * cyc + 1])
        assert not (tr[3 * cyc + 1] - tr[3 * cyc] < 1e-4)  # and the rule held at no earlier cycle
    assert (acc["alpha"] <= -1.0).all()
    ll = ar.loglik(codes, acc["Q"], acc["P"])
    assert abs(acc["loglik"] - ll) <= ar.bound_ll(T, K, ll)


@pytest.mark.parametrize("n,m,K,miss", [(65, 129, 8, 0.0), (130, "chunk+1", 32, 0.1)])
def test_two_calls_block_plans_and_device_starts_give_the_same_bits(n, m, K, miss):
    import tidypopgen_amd as tpg

    c = _case(n, m, K, miss)
    v, ctx = c["v"], c["v"].ctx
    names = ("Q", "P", "trace", "alpha")
    a = _run(tpg, c, K, 7)
    b = _run(tpg, c, K, 7)
    for name in names:
        assert np.array_equal(_bits(a[name]), _bits(b[name]))
    assert np.array_equal(a["accepted"], b["accepted"]) and a["n_cycles"] == 2
    # the same view over a store uploaded in column blocks
    big = np.asfortranarray(c["big"])
    X2 = tpg.FBM.alloc(big.shape[0], big.shape[1], ctx=ctx, code256=tpg.CODE_012)
    for c0 in range(0, big.shape[1], 37):
        X2.upload_cols(np.asfortranarray(big[:, c0:c0 + 37]), c0)
    v2 = tpg.View(X2, c["rows"], c["cols"])
    b = tpg.admix_em(v2, K, Q0=c["Q0"], F0=c["F0"], max_iter=7, tol=0.0, return_trace=True, accel="squarem")
    for name in names:
        assert np.array_equal(_bits(a[name]), _bits(b[name]))
    # Q0 / F0 in device memory
    q0, f0 = np.asfortranarray(c["Q0"]), np.asfortranarray(c["F0"])
    dq, df = ctx.dev_alloc(q0.nbytes), ctx.dev_alloc(f0.nbytes)
    try:
        from tidypopgen_amd._lib import check, lib

        check(lib.tpg_dev_from_host(ctx.h, dq, C.c_void_p(q0.ctypes.data), C.c_size_t(q0.nbytes)))
        check(lib.tpg_dev_from_host(ctx.h, df, C.c_void_p(f0.ctypes.data), C.c_size_t(f0.nbytes)))
        b = tpg.admix_em(v, K, Q0=int(dq.value), F0=int(df.value), max_iter=7, tol=0.0, return_trace=True, accel="squarem")
    finally:
        ctx.dev_free(dq)
        ctx.dev_free(df)
    for name in names:
        assert np.array_equal(_bits(a[name]), _bits(b[name]))


def _compose(tpg, v, K, folds, cv_seed, **kw):
    ll, cnt, het, nit, conv = [], [], [], [], []
    for f in range(folds):
        t = v.holdout(folds, f, cv_seed)
        r = tpg.admix_em(t, K, accel="squarem", **kw)
        s = tpg.admix_holdout_sums(v, t, r["Q"], r["P"])
        ll.append(s["ll"]), cnt.append(s["n_held"]), het.append(s["n_het"]), nit.append(r["n_iter"]), conv.append(r["converged"])
        t.free()
    e = tpg.admix_cv_error(ll, cnt, het)
    return dict(cv_error=e["cv_error"], fold_deviance=e["fold_deviance"], fold_ll=np.array(ll), fold_count=np.array(cnt),
                fold_het=np.array(het), fold_n_iter=np.array(nit), fold_converged=np.array(conv))


def test_admix_cv_squarem_is_the_composition_of_its_pieces_bit_for_bit():
    import tidypopgen_amd as tpg

    c = _case(65, 129, 3, 0.1)
    v, K, folds = c["v"], 3, 3
    for kw in (dict(Q0=c["Q0"], F0=c["F0"]), dict(seed=77)):
        got = tpg.admix_cv(v, K, folds=folds, cv_seed=9, max_iter=12, tol=0.0, accel="squarem", **kw)
        want = _compose(tpg, v, K, folds, 9, max_iter=12, tol=0.0, **kw)
        assert sorted(got) == sorted(want)
        for name in ("fold_ll", "fold_deviance"):
            assert np.array_equal(_bits(got[name]), _bits(want[name])), name
        for name in ("fold_count", "fold_het", "fold_n_iter", "fold_converged"):
            assert np.array_equal(got[name], want[name]), name
        assert _bits(got["cv_error"])[0] == _bits(want["cv_error"])[0]
        assert (got["fold_n_iter"] == 12).all() and int(got["fold_count"].sum()) == int((c["codes"] != ar.MISSING).sum())
        plain = tpg.admix_cv(v, K, folds=folds, cv_seed=9, max_iter=12, tol=0.0, **kw)
        assert np.array_equal(plain["fold_count"], got["fold_count"]) and not np.array_equal(_bits(plain["fold_ll"]), _bits(got["fold_ll"]))
    assert np.array_equal(v.unpack(), c["codes"])


def test_cv_error_under_acceleration_still_chooses_the_simulated_k():
    """the 130 x 400 two-population panel of tests/test_gpu_admix_cv.py: the smallest CV error is at K = 2; gt_admixture forwards
    accel to the fit and to the cross-validation"""
    import tidypopgen_amd as tpg

    codes = ar.panel(11, 130, 400, 2, 0.1)[0]
    big, rows, cols = _embed(codes, 5)
    X = tpg.FBM.from_numpy(np.asfortranarray(big), code256=tpg.CODE_012)
    v = tpg.View(X, rows, cols)
    cv = {}
    for K in (1, 2, 3):
        r = tpg.admix_cv(v, K, folds=5, cv_seed=1, seed=42, max_iter=300, tol=1e-4, accel="squarem")
        cv[K] = r["cv_error"]
        print("cv error K =", K, cv[K], "EM steps per fold", r["fold_n_iter"].tolist(), "converged", r["fold_converged"].tolist())
    assert cv[2] < cv[1] and cv[2] < cv[3]
    out = tpg.gt_admixture(X, rows, cols, k=[2], seed=[42], max_iter=300, crossval=True, cv_folds=5, cv_seed=1, accel="squarem")
    fit = tpg.admix_em(v, 2, seed=42, max_iter=300, accel="squarem")
    assert _bits(out["cv"][0])[0] == _bits(cv[2])[0] and np.array_equal(_bits(out["Q"][0]), _bits(fit["Q"]))
    assert out["n_iter"][0] == fit["n_iter"] and out["loglik"][0] == fit["loglik"]


def test_errors_leave_every_output_untouched():
    import tidypopgen_amd as tpg
    from tidypopgen_amd import _lib
    from tidypopgen_amd.api import _ptr

    c = _case(13, 31, 2, 0.1)
    v, n, m, K = c["v"], 13, 31, 2

    def call(K=K, q0=None, f0=None, ploidy=None, **kw):
        pr = _lib.AdmixParams()
        _lib.lib.tpg_admix_params_default(pr)
        pr.max_iter = 6
        for name, val in kw.items():
            setattr(pr, name, val)
        Q, P = np.full((n, 40), 7.0, order="F"), np.full((m, 40), 7.0, order="F")
        tr, al, ac = np.full(8, 7.0), np.full(3, 7.0), np.full(3, 7, dtype=np.int32)
        ll, nit, conv, ncyc, nrej = C.c_double(7.0), C.c_int32(7), C.c_int32(7), C.c_int32(7), C.c_int32(7)
        rc = _lib.lib.tpg_admix_em_squarem(v.ctx.h, v.h, _ptr(ploidy), C.c_int(K), C.byref(pr), _ptr(q0), _ptr(f0), _ptr(Q), _ptr(P),
                                           C.byref(ll), _ptr(tr), C.byref(nit), C.byref(conv), _ptr(al), _ptr(ac), C.byref(ncyc),
                                           C.byref(nrej))
        if rc != 0:
            assert (Q == 7.0).all() and (P == 7.0).all() and (tr == 7.0).all() and (al == 7.0).all() and (ac == 7).all()
            assert (ll.value, nit.value, conv.value, ncyc.value, nrej.value) == (7.0, 7, 7, 7, 7)
        else:
            assert tr[7] == 7.0 and al[2] == 7.0 and ac[2] == 7 and nit.value <= 6 and ncyc.value <= 2  # nothing past the room named
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
    assert call(q0=q0, f0=f0, tol=0.0) == 0 and call() == 0
    # every output of the accelerated entry may be NULL but Q and P
    pr = _lib.AdmixParams()
    _lib.lib.tpg_admix_params_default(pr)
    pr.max_iter = 4
    Q, P = np.zeros((n, K), order="F"), np.zeros((m, K), order="F")
    assert _lib.lib.tpg_admix_em_squarem(v.ctx.h, v.h, None, K, C.byref(pr), None, None, _ptr(Q), _ptr(P), None, None, None, None, None,
                                         None, None, None) == 0
    assert np.allclose(Q.sum(axis=1)[:-1], 1.0, rtol=0, atol=1e-12)
    # the point primitive's refusals
    th = _states(13, 31, 2, 0.1)[1]
    for bad in (0.5, float("nan"), -4.0):
        with pytest.raises(_lib.TpgError, match="a_max"):
            tpg.admix_squarem_point(*th, a_max=bad, ctx=v.ctx)
    # the Python layer raises what the library answers, and refuses another accelerator itself
    with pytest.raises(_lib.TpgError, match="K = 33"):
        tpg.admix_em(v, 33, accel="squarem")
    with pytest.raises(_lib.TpgError, match="not finite or not positive"):
        q = q0.copy()
        q[0, 0] = 0.0
        tpg.admix_em(v, K, Q0=q, accel="squarem")
    for fn in (tpg.admix_em, tpg.admix_cv):
        with pytest.raises(ValueError, match="accel must be None or 'squarem'"):
            fn(v, K, accel="newton")
    with pytest.raises(ValueError, match="accel must be None or 'squarem'"):
        tpg.gt_admixture(c["X"], c["rows"], c["cols"], k=2, accel="newton")
    # both halves fixed: the state never moves, as in the plain EM
    r = tpg.admix_em(v, K, Q0=q0, F0=f0, max_iter=6, tol=0.0, update_q=False, update_f=False, accel="squarem", return_trace=True)
    assert np.array_equal(_bits(r["Q"]), _bits(c["Qs"])) and np.array_equal(_bits(r["P"]), _bits(c["Fs"])) and r["n_iter"] == 6
    assert (r["alpha"] == -1.0).all() and r["accepted"].all() and len(set(r["trace"].tolist())) == 1
