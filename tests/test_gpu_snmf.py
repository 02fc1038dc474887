"""GPU: sNMF (include/tpg.h "sNMF") against the numpy restatement tests/snmf_ref.py, whose exact solver is scipy.optimize.nnls on
the Cholesky factor.

What is compared how.  nnls_shared: x >= 0, no unsolved system, the KKT residual evaluated in numpy, and the distance to scipy's
optimum.  One iteration is checked in its two halves: the device's G against g_half of the Q that went in, the device's Q' against
q_half of the DEVICE's G (so each half is held to the bound of one batch of solves and nothing drifts), ls against the value the
restatement gives for that pair.  The per-system bound is tol_x = [sqrt(K) tau |b|_inf + 2 (n_t + K + 4) u (|A|_F |x*|_2 + |b|_2)]
/ lambda_min: the contract's distance plus the rounding of the sums that feed A and b (n_t terms), carried through the solution
map, which is Lipschitz with constant 1 / lambda_min across a change of passive set.  After normalisation: (K + 1) tol_x / s*.
Cells whose reference sum lies within 1e3 tol_x of TPG_SNMF_TINY may fall on either side of the switch and are exempt; their
share must stay under 0.1 % per case.  Chained iterations feed the device's Q(t) into the restatement each time.  The seeded
start, tpg_snmf against the composition of tpg_snmf_step, and two calls: bit for bit.  The hold-out view: byte for byte.  The
cases and their views are those of tests/test_gpu_admix.py: row / column subsets of a larger store."""
import ctypes as C

import numpy as np
import pytest

from tests import admix_ref as ar
from tests import snmf_ref as sr
from tests.test_gpu_admix import _bits, _case, _embed

pytestmark = pytest.mark.gpu

SHAPES = [(13, 1, 1, 0.0), (13, 31, 2, 0.1), (65, 33, 3, 0.1), (65, 129, 8, 0.0), (130, 129, 16, 0.1), (13, "chunk+1", 3, 0.1),
          (130, "chunk+1", 16, 0.1)]
EINVAL = 1
ALPHA = 10.0


# ---- the solver alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8, 11, 16])
def test_nnls_shared_meets_the_contract(K):
    import tidypopgen_amd as tpg

    rng = np.random.default_rng(100 + K)
    Q = rng.dirichlet(np.full(K, 0.5), size=130)
    A = sr.ridge(Q.T @ Q)
    B = rng.uniform(0, 20, size=(257, K))  # more than one workgroup, and a last one that is not full
    B[::3] = 10 * rng.normal(size=B[::3].shape)  # a third with signs that force zeros
    B[5], B[6] = 0.0, -1.0
    X, unsolved = tpg.nnls_shared(A, B, return_unsolved=True)
    assert unsolved == 0 and (X >= 0).all() and (X[5] == 0).all() and (X[6] == 0).all()
    worst = 0.0
    for b, x in zip(B, X):
        if np.abs(b).max() > 0:
            worst = max(worst, sr.kkt_residual(A, b, x) / np.abs(b).max())
        assert sr.kkt_residual(A, b, x) <= sr.KKT_TOL * np.abs(b).max()
    Xs = sr.nnls_exact(A, B)
    bound = sr.bound_nnls(A, B)
    print("nnls K", K, "KKT residual / |b|_inf", worst, "max |x - x*| / bound", (np.abs(X - Xs).max(axis=1) / np.maximum(bound, 1e-300)).max())
    assert (np.abs(X - Xs).max(axis=1) <= bound).all()
    again = tpg.nnls_shared(A, B)
    assert np.array_equal(_bits(again), _bits(X))


# ---- one iteration ---------------------------------------------------------------------------------------------------------
def _check_g(c, Q_in, G_dev):
    """the device's G (3m x K) is the G step from Q_in"""
    codes, n, m, K = c["codes"], c["n"], c["m"], c["K"]
    ref = sr.g_half(codes, Q_in)
    Gd = sr.g_cube(G_dev)
    tol = sr.bound_x(ref["A"], ref["b"].reshape(3 * m, K), ref["gt"].reshape(3 * m, K), n).reshape(m, 3).max(axis=1)[:, None]  # (m, 1)
    s = ref["s"]  # (m, K)
    near = (s != 0) & (np.abs(s - sr.TINY) <= 1e3 * tol)  # an exact zero is no borderline case: it must come back as 1/3
    live, dead = (s > sr.TINY) & ~near, (s <= sr.TINY) & ~near
    assert near.mean() <= 1e-3, ("exempt share", near.mean())
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = (K + 1) * tol / s
    err = np.abs(Gd - ref["G"])
    for cl in range(3):
        assert (err[:, cl, :][live] <= bound[live]).all(), (cl, (err[:, cl, :][live] / bound[live]).max())
        assert (Gd[:, cl, :][dead] == 1.0 / 3.0).all()
    assert (Gd[:, :, :][np.broadcast_to((s == 0)[:, None, :], Gd.shape)] == 1.0 / 3.0).all()  # exact-zero sums: exactly 1/3
    assert (Gd >= 0).all() and np.abs(Gd.sum(axis=1) - 1.0).max() <= 4 * sr.U
    worst = float((err[:, 0, :][live] / bound[live]).max()) if live.any() else 0.0
    return ref, dict(worst=worst, zero_share=float((s == 0).mean()), small=int(((s > 0) & (s < 1e-3)).sum()))


def _check_q(c, G_dev, Q_dev, ls_dev, alpha=ALPHA):
    """the device's Q' and ls are the Q step from the device's G"""
    codes, m, K = c["codes"], c["m"], c["K"]
    ref = sr.q_half(codes, sr.g_cube(G_dev), alpha)
    tol = sr.bound_x(ref["B"], ref["b"], ref["qt"], 3 * m)  # (n,)
    r = ref["r"]
    near = (r != 0) & (np.abs(r - sr.TINY) <= 1e3 * tol)
    live, dead = (r > sr.TINY) & ~near, (r <= sr.TINY) & ~near
    assert near.mean() <= 1e-3
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = ((K + 1) * tol / r)[:, None]
    err = np.abs(Q_dev - ref["Q"])
    assert (err[live] <= np.broadcast_to(bound, err.shape)[live]).all(), (err[live] / np.broadcast_to(bound, err.shape)[live]).max()
    assert (Q_dev[dead] == 1.0 / K).all()
    assert (Q_dev >= 0).all() and np.abs(Q_dev.sum(axis=1) - 1.0).max() <= (K + 1) * sr.U
    b_ls = sr.bound_ls(3 * m, ref["T"], ref["sqb"], ref["dot"])
    print("  ls", ls_dev, ref["ls"], "|d|", abs(ls_dev - ref["ls"]), "bound", b_ls)
    assert abs(ls_dev - ref["ls"]) <= b_ls
    return ref


@pytest.mark.parametrize("n,m,K,miss", SHAPES)
def test_one_step_from_a_given_q(n, m, K, miss):
    import tidypopgen_amd as tpg

    c = _case(n, m, K, miss)
    r = tpg.snmf_step(c["v"], c["Qs"], ALPHA)
    assert r["n_unsolved"] == 0
    ref_g, info = _check_g(c, c["Qs"], r["G"])
    print("step", n, c["m"], K, "G worst err / bound", info["worst"], "exact-zero sums", info["zero_share"], "sums in (0, 1e-3)", info["small"])
    _check_q(c, r["G"], r["Q"], r["ls"])
    Gd, pl = sr.g_cube(r["G"]), c["planted"]
    if pl["col_missing"] is not None:
        assert (Gd[pl["col_missing"]] == 1.0 / 3.0).all()
    # a column of one genotype: the two other classes have b = 0, so G is exactly 1 in its class wherever the solve gives that
    # k a positive value, and 1/3 in all three where it gives 0 (at K = 16 the restatement itself zeroes some k of such a column)
    for col, cl in ((pl["col_all0"], 0), (pl["col_all2"], 2)):
        if col is None:
            continue
        others = [x for x in range(3) if x != cl]
        one = (Gd[col, cl, :] == 1.0) & (Gd[col, others, :] == 0.0).all(axis=0)
        third = (Gd[col] == 1.0 / 3.0).all(axis=0)
        assert (one | third).all() and one.any()
        assert np.array_equal(one, ref_g["s"][col] > sr.TINY)
    if pl["row_missing"] is not None:
        assert (r["Q"][pl["row_missing"]] == 1.0 / K).all()
    again = tpg.snmf_step(c["v"], c["Qs"], ALPHA)
    assert np.array_equal(_bits(again["Q"]), _bits(r["Q"])) and np.array_equal(_bits(again["G"]), _bits(r["G"]))
    assert _bits(again["ls"]) == _bits(r["ls"])
    assert np.array_equal(c["v"].unpack(), c["codes"])


@pytest.mark.parametrize("n,m,K,miss", [(65, 33, 3, 0.1), (65, 129, 8, 0.0), (130, 129, 16, 0.1)])
def test_ten_chained_steps_each_within_the_one_step_bound(n, m, K, miss):
    import tidypopgen_amd as tpg

    c = _case(n, m, K, miss)
    Q, ls = c["Qs"], []
    for t in range(10):
        r = tpg.snmf_step(c["v"], Q, ALPHA)
        assert r["n_unsolved"] == 0
        _check_g(c, Q, r["G"])
        _check_q(c, r["G"], r["Q"], r["ls"])
        Q = r["Q"]
        ls.append(r["ls"])
    print("chained ls", n, m, K, ls)
    assert ls[-1] < ls[0]


# ---- the run -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,K,miss", SHAPES)
def test_seeded_start_and_the_run_as_a_composition_of_steps(n, m, K, miss):
    import tidypopgen_amd as tpg

    c = _case(n, m, K, miss)
    v = c["v"]
    for seed in (0, 0xDEADBEEFCAFEF00D):
        r0 = tpg.snmf(v, K, seed=seed, max_iter=0, return_trace=True)
        Q0 = ar.start(seed, n, c["m"], K)[0]
        assert np.array_equal(_bits(r0["Q"]), _bits(Q0))
        assert (r0["G"] == 1.0 / 3.0).all() and r0["n_iter"] == 0 and not r0["converged"] and len(r0["trace"]) == 0 and np.isnan(r0["ls"])
        assert np.array_equal(_bits(r0["P"]), _bits(np.full((c["m"], K), (1.0 / 3.0) / 2.0 + 1.0 / 3.0)))
    # three iterations = the steps from the seeded start with the stop rule applied by hand, bit for bit (tol = 0 stops only where ls
    # repeats exactly, as it does at K = 1, whose Q cannot move)
    run = tpg.snmf(v, K, seed=7, max_iter=3, tol=0.0, alpha=ALPHA, return_trace=True)
    Q, ls, conv = ar.start(7, n, c["m"], K)[0], [], False
    while len(ls) < 3 and not conv:
        s = tpg.snmf_step(v, Q, ALPHA)
        Q = s["Q"]
        ls.append(s["ls"])
        conv = len(ls) >= 2 and abs(ls[-2] - ls[-1]) <= 0.0
    assert run["n_iter"] == len(ls) and run["converged"] == conv and (len(ls) == 3 or K == 1)
    assert run["n_unsolved"] == 0 and len(run["trace"]) == len(ls) and run["ls"] == run["trace"][-1]
    assert np.array_equal(_bits(run["Q"]), _bits(Q)) and np.array_equal(_bits(run["G"]), _bits(s["G"]))
    assert np.array_equal(_bits(run["trace"]), _bits(np.array(ls)))
    assert np.array_equal(_bits(run["P"]), _bits(sr.p_of(sr.g_cube(run["G"]))))
    again = tpg.snmf(v, K, seed=7, max_iter=3, tol=0.0, alpha=ALPHA)
    for name in ("Q", "G", "P"):
        assert np.array_equal(_bits(again[name]), _bits(run[name]))
    assert _bits(again["ls"]) == _bits(run["ls"])
    # a given q0 is normalised as tpg_admix_em normalises it
    given = tpg.snmf(v, K, Q0=c["Q0"], max_iter=1, alpha=ALPHA)
    one = tpg.snmf_step(v, c["Qs"], ALPHA)
    assert np.array_equal(_bits(given["Q"]), _bits(one["Q"])) and np.array_equal(_bits(given["G"]), _bits(one["G"]))


def test_stop_rule():
    import tidypopgen_amd as tpg

    c = _case(65, 33, 3, 0.1)
    r = tpg.snmf(c["v"], 3, seed=1, tol=1e-3, max_iter=200, return_trace=True)
    t, tr = r["n_iter"], r["trace"]
    assert r["converged"] and 2 <= t < 200 and len(tr) == t
    assert abs(tr[t - 2] - tr[t - 1]) <= 1e-3 * tr[t - 2]
    assert all(abs(tr[s - 2] - tr[s - 1]) > 1e-3 * tr[s - 2] for s in range(2, t))


# ---- hold-out and cross-entropy -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,K,miss", SHAPES)
def test_holdout_fraction_equals_the_restatement_byte_for_byte(n, m, K, miss):
    c = _case(n, m, K, miss)
    v, codes = c["v"], c["codes"]
    for fraction in (0.05, 0.5):
        for seed in (7, 0xDEADBEEFCAFEF00D):
            t = v.holdout_fraction(fraction, seed)
            want = sr.holdout_fraction(codes, fraction, seed)
            assert (t.n, t.m) == codes.shape
            assert np.array_equal(t.unpack(), want)
            assert t.n_held == int(((codes != sr.MISSING) & (want == sr.MISSING)).sum())
    assert np.array_equal(v.unpack(), codes)


@pytest.mark.parametrize("n,m,K,miss", SHAPES)
def test_cross_entropy_sums_from_a_given_state(n, m, K, miss):
    import tidypopgen_amd as tpg

    c = _case(n, m, K, miss)
    v, codes = c["v"], c["codes"]
    t = v.holdout_fraction(0.3, 5)
    train = sr.holdout_fraction(codes, 0.3, 5)
    G = sr.g_half(train, c["Qs"])["G"]
    got, ref = tpg.snmf_cross_entropy(v, t, c["Qs"], sr.g_matrix(G)), sr.cross_entropy_sums(codes, train, c["Qs"], G)
    assert (got["n_masked"], got["n_all"]) == (ref["n_masked"], ref["n_all"]) and got["n_masked"] == t.n_held
    for name, cnt in (("sum_masked", "n_masked"), ("sum_all", "n_all")):
        bound = sr.bound_ce(ref[cnt], K, ref[name])
        print("cross-entropy", n, c["m"], K, name, got[name], ref[name], abs(got[name] - ref[name]), bound)
        assert abs(got[name] - ref[name]) <= bound
    if ref["n_masked"]:
        assert got["masked"] == got["sum_masked"] / got["n_masked"]
    assert tpg.snmf_cross_entropy(v, t, c["Qs"], sr.g_matrix(G)) == got
    # the floor: a state that gives p = 0 somewhere costs -ln(floor) there, not infinity
    Gz = G.copy()
    Gz[:, 0, :] = 0.0
    z = tpg.snmf_cross_entropy(v, t, c["Qs"], sr.g_matrix(Gz))
    zr = sr.cross_entropy_sums(codes, train, c["Qs"], Gz)
    assert np.isfinite(z["sum_all"]) and abs(z["sum_all"] - zr["sum_all"]) <= sr.bound_ce(zr["n_all"], K, zr["sum_all"])


def test_cross_entropy_chooses_the_simulated_k():
    """A panel simulated from two populations (snmf_ref.k_panel): K = 2 has the smallest masked cross-entropy, on the device as in the
    restatement.  Both run up to 200 chained iterations with their own roundings and their own stopping iteration, so the values
    are not held to a rounding bound: each must lie within a quarter of the smallest gap between the restatement's values, which
    keeps the order.  Observed on an MI355X: see DESIGN.md 3.13."""
    import tidypopgen_amd as tpg

    codes, _ = sr.k_panel()
    big, rows, cols = _embed(codes, 5)
    X = tpg.FBM.from_numpy(np.asfortranarray(big), code256=tpg.CODE_012)
    ref = {K: sr.cross_entropy_of_k(codes, K, 0.05, 1, 1, ALPHA, 1e-5, 200) for K in (1, 2, 3)}
    gap = min(ref[1][0], ref[3][0]) - ref[2][0]
    assert gap > 0.005  # the restatement itself picks K = 2 by a clear margin
    out = tpg.gt_snmf(X, rows, cols, k=[1, 2, 3], n_runs=1, seed=[1], alpha=ALPHA, tolerance=1e-5, entropy=True, percentage=0.05, iterations=200)
    assert out["k"] == [1, 2, 3] and out["algorithm"] == "SNMF"
    for a, K in enumerate((1, 2, 3)):
        print("cross-entropy K =", K, "device", out["cv"][a], "restatement", ref[K][0], "device - restatement", out["cv"][a] - ref[K][0],
              "iterations", out["n_iter"][a], ref[K][1]["n_iter"], "quarter gap", gap / 4)
    assert out["cv"][1] < out["cv"][0] and out["cv"][1] < out["cv"][2]
    for a, K in enumerate((1, 2, 3)):
        assert abs(out["cv"][a] - ref[K][0]) <= gap / 4


def test_gt_snmf_is_its_pieces():
    import tidypopgen_amd as tpg

    c = _case(65, 33, 3, 0.1)
    args = (c["X"], c["rows"], c["cols"])
    out = tpg.gt_snmf(*args, k=[2, 3], n_runs=2, seed=[5, 6, 7, 8], iterations=4, entropy=True, percentage=0.2)
    assert out["k"] == [2, 2, 3, 3] and len(out["cv"]) == len(out["cv_all"]) == 4
    for a, (kk, seed) in enumerate(zip(out["k"], (5, 6, 7, 8))):
        t = c["v"].holdout_fraction(0.2, seed)
        r = tpg.snmf(t, kk, seed=seed, max_iter=4)
        ce = tpg.snmf_cross_entropy(c["v"], t, r["Q"], r["G"])
        for name in ("Q", "G", "P"):
            assert np.array_equal(_bits(out[name][a]), _bits(r[name]))
        assert _bits(out["cv"][a]) == _bits(ce["masked"]) and _bits(out["cv_all"][a]) == _bits(ce["all"]) and out["ls"][a] == r["ls"]
        assert out["Q"][a].shape == (65, kk) and out["G"][a].shape == (99, kk) and out["P"][a].shape == (33, kk)
    plain = tpg.gt_snmf(*args, k=2, seed=[5], iterations=4)
    assert sorted(plain) == ["G", "P", "Q", "algorithm", "converged", "k", "ls", "n_iter"]
    assert np.array_equal(_bits(plain["Q"][0]), _bits(tpg.snmf(c["v"], 2, seed=5, max_iter=4)["Q"]))
    with pytest.raises(ValueError):
        tpg.gt_snmf(*args, k=2, entropy=True, percentage=1.0)


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_errors_leave_every_output_untouched():
    from tidypopgen_amd import _lib
    from tidypopgen_amd.api import _ptr

    c, other = _case(13, 31, 2, 0.1), _case(65, 33, 3, 0.1)
    v, n, m = c["v"], 13, 31
    lib = _lib.lib

    def run(K=2, max_iter=2, tol=1e-5, alpha=10.0, q0=None, ploidy=None):
        Q, G, P = np.full((n, 16), 7.0, order="F"), np.full((3 * m, 16), 7.0, order="F"), np.full((m, 16), 7.0, order="F")
        ls, nit, conv, uns, tr = C.c_double(7.0), C.c_int(7), C.c_int(7), C.c_int64(7), np.full(8, 7.0)
        rc = lib.tpg_snmf(v.ctx.h, v.h, _ptr(ploidy), K, max_iter, tol, alpha, 1, _ptr(q0), _ptr(Q), _ptr(G), _ptr(P), C.byref(ls), _ptr(tr),
                          C.byref(nit), C.byref(conv), C.byref(uns))
        if rc != 0:
            assert (Q == 7).all() and (G == 7).all() and (P == 7).all() and (tr == 7).all()
            assert (ls.value, nit.value, conv.value, uns.value) == (7.0, 7, 7, 7)
        return rc

    assert run(K=0) == EINVAL and run(K=17) == EINVAL and run(K=-1) == EINVAL
    assert run(tol=-1.0) == EINVAL and run(tol=float("nan")) == EINVAL and run(max_iter=-1) == EINVAL and run(alpha=-1.0) == EINVAL
    for bad in (np.nan, np.inf, 0.0, -0.5):
        q = np.asfortranarray(c["Q0"]).copy()
        q[7, 1] = bad
        assert run(q0=q) == EINVAL, bad
    pl = np.full(n, 2.0)
    pl[4] = 1.0
    assert run(ploidy=pl) == EINVAL
    assert run() == 0 and run(K=16) == 0 and run(q0=np.asfortranarray(c["Q0"])) == 0

    def step(K=2, alpha=10.0):
        Q, G = np.full((n, 16), 7.0, order="F"), np.full((3 * m, 16), 7.0, order="F")
        ls, uns = C.c_double(7.0), C.c_int64(7)
        qin = np.asfortranarray(ar.start(0, n, m, max(1, min(K, 16)))[0])
        rc = lib.tpg_snmf_step(v.ctx.h, v.h, K, alpha, _ptr(qin), _ptr(Q), _ptr(G), C.byref(ls), C.byref(uns))
        if rc != 0:
            assert (Q == 7).all() and (G == 7).all() and (ls.value, uns.value) == (7.0, 7)
        return rc

    assert step(K=0) == EINVAL and step(K=17) == EINVAL and step(alpha=float("nan")) == EINVAL and step() == 0

    def holdout(fraction):
        h, held = C.c_void_p(), C.c_int64(7)
        rc = lib.tpg_view_holdout_fraction(v.ctx.h, v.h, fraction, 1, C.byref(h), C.byref(held))
        if rc != 0:
            assert h.value is None and held.value == 7
        else:
            lib.tpg_view_free(h)
        return rc

    assert holdout(0.0) == EINVAL and holdout(1.0) == EINVAL and holdout(-0.1) == EINVAL and holdout(float("nan")) == EINVAL
    assert holdout(0.05) == 0

    t = v.holdout_fraction(0.2, 1)
    Qs, G = np.asfortranarray(c["Qs"]), np.asfortranarray(np.full((3 * m, 2), 1.0 / 3.0))

    def sums(full, train, K=2):
        sm, sa, nm, na = C.c_double(7.0), C.c_double(7.0), C.c_int64(7), C.c_int64(7)
        rc = lib.tpg_snmf_cross_entropy_sums(full.ctx.h, full.h, train.h, K, _ptr(Qs), _ptr(G), C.byref(sm), C.byref(nm), C.byref(sa),
                                             C.byref(na))
        if rc != 0:
            assert (sm.value, sa.value, nm.value, na.value) == (7.0, 7.0, 7, 7)
        return rc

    assert sums(v, other["v"]) == EINVAL and sums(other["v"], t) == EINVAL and sums(v, _case(13, 1, 1, 0.0)["v"]) == EINVAL
    assert sums(v, t, K=0) == EINVAL and sums(v, t, K=17) == EINVAL and sums(v, t) == 0
    assert lib.tpg_snmf_cross_entropy_sums(v.ctx.h, v.h, t.h, 2, _ptr(Qs), _ptr(G), None, None, None, None) == 0

    A, B, Xo, uns = np.eye(2, order="F"), np.ones((4, 2), order="F"), np.full((4, 2), 7.0, order="F"), C.c_int64(7)
    for K in (0, 17):
        assert lib.tpg_nnls_shared(v.ctx.h, K, _ptr(A), _ptr(B), 4, _ptr(Xo), C.byref(uns)) == EINVAL
        assert (Xo == 7).all() and uns.value == 7
    assert lib.tpg_nnls_shared(v.ctx.h, 2, _ptr(A), _ptr(B), 4, _ptr(Xo), C.byref(uns)) == 0 and (Xo == 1).all() and uns.value == 0
    with pytest.raises(_lib.TpgError, match=r"K = 17 out of \[1, 16\]"):
        import tidypopgen_amd as tpg

        tpg.snmf(v, 17)
