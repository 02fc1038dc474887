"""The squared extrapolation of include/tpg.h "admixture, accelerated" restated in numpy on top of tests/admix_ref.py: one cycle
(the differences, the two sums, alpha, theta' raw through an exact fused multiply-add, the projection) and the driver with its
step limit, accept / reject rule and counting.  The header is the definition; this file follows it step by step.  The sums have
a float route (numpy's order) and an exact route in fractions.Fraction; theta' raw is formed with an fma that is exact by
construction (float(Fraction) rounds correctly), so it can be compared bit for bit with the device."""
from fractions import Fraction

import numpy as np

from tests import admix_ref as ar

U = ar.U
EPS = ar.EPS


# ---- step 3: the differences ------------------------------------------------------------------------------------------------
def differences(t0, t1, t2):
    """r = theta1 - theta0, v = (theta2 - theta1) - r: IEEE double, one rounding per operation"""
    t0, t1, t2 = (np.asarray(x, dtype=np.float64) for x in (t0, t1, t2))
    r = t1 - t0
    return r, (t2 - t1) - r


# ---- step 4: the sums -----------------------------------------------------------------------------------------------------------
def _halves(Q, F, update_q, update_f):
    return ([np.asarray(Q, dtype=np.float64).ravel()] if update_q else []) + ([np.asarray(F, dtype=np.float64).ravel()] if update_f else [])


def sums(Q0, F0, Q1, F1, Q2, F2, update_q=True, update_f=True):
    """float route -> sr, sv, nn (the number of entries summed)"""
    sr = sv = 0.0
    nn = 0
    for a, b, c in zip(_halves(Q0, F0, update_q, update_f), _halves(Q1, F1, update_q, update_f), _halves(Q2, F2, update_q, update_f)):
        r, v = differences(a, b, c)
        sr += float((r * r).sum())
        sv += float((v * v).sum())
        nn += a.size
    return sr, sv, nn


def sums_exact(Q0, F0, Q1, F1, Q2, F2, update_q=True, update_f=True):
    """the exact rational sums of (theta1 - theta0)^2 and ((theta2 - theta1) - (theta1 - theta0))^2 of the given doubles"""
    sr = sv = Fraction(0)
    for a, b, c in zip(_halves(Q0, F0, update_q, update_f), _halves(Q1, F1, update_q, update_f), _halves(Q2, F2, update_q, update_f)):
        for x, y, z in zip(a, b, c):
            x, y, z = Fraction(float(x)), Fraction(float(y)), Fraction(float(z))
            sr += (y - x) ** 2
            sv += ((z - y) - (y - x)) ** 2
    return sr, sv


def bound_sr(nn, sr):
    """|d sr| <= (nn + 3) u sr"""
    return (nn + 3) * U * abs(float(sr))


def bound_sv(Q0, F0, Q1, F1, Q2, F2, sv, update_q=True, update_f=True):
    """|d sv| <= 2 sum |v| |dv| + (nn + 3) u sv, |dv| <= u (|theta2 - theta1| + |r| + |v|)"""
    tot, nn = 0.0, 0
    for a, b, c in zip(_halves(Q0, F0, update_q, update_f), _halves(Q1, F1, update_q, update_f), _halves(Q2, F2, update_q, update_f)):
        r, v = differences(a, b, c)
        dv = U * (np.abs(c - b) + np.abs(r) + np.abs(v))
        tot += float((2.0 * np.abs(v) * dv).sum())
        nn += a.size
    return tot + (nn + 3) * U * abs(float(sv))


# ---- step 5: alpha and the step limit ------------------------------------------------------------------------------------------
def alpha_of(sr, sv, a_max):
    """-> alpha, at_limit.  numpy's division and square root are correctly rounded"""
    with np.errstate(divide="ignore", invalid="ignore"):
        a = -np.sqrt(np.float64(sr) / np.float64(sv))
    if sv == 0 or not np.isfinite(a):
        a = np.float64(-1.0)
    at_limit = bool(a < -a_max)
    if at_limit:
        a = np.float64(-a_max)
    if a > -1.0:
        a = np.float64(-1.0)
    return float(a), at_limit


def accept(l_prime, l_one):
    return bool(np.isfinite(l_prime) and l_prime >= l_one)


def next_limit(a_max, accepted, at_limit):
    if accepted:
        return 4.0 * a_max if at_limit else a_max
    return max(1.0, a_max / 4.0)


# ---- step 6: theta' raw ---------------------------------------------------------------------------------------------------------
def fma_exact(a, b, c):
    """a * b + c rounded once, element by element (finite doubles): float(Fraction(a) * Fraction(b) + Fraction(c)), written on
    the integer ratios a Fraction holds (without its gcd at every step): numerator / denominator of Python integers is correctly
    rounded, which is all float(Fraction) does"""
    a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (a, b, c)))
    out = np.empty(a.shape)
    flat = out.reshape(-1)
    for i, (x, y, z) in enumerate(zip(a.ravel().tolist(), b.ravel().tolist(), c.ravel().tolist())):
        (nx, dx), (ny, dy), (nz, dz) = x.as_integer_ratio(), y.as_integer_ratio(), z.as_integer_ratio()
        flat[i] = (nx * ny * dz + nz * dx * dy) / (dx * dy * dz)
    return out


def raw(t0, t1, t2, alpha):
    """fma(alpha * alpha rounded once, v, fma(-2 alpha, r, theta0))"""
    r, v = differences(t0, t1, t2)
    a2 = np.float64(alpha) * np.float64(alpha)
    return fma_exact(a2, v, fma_exact(-2.0 * np.float64(alpha), r, np.asarray(t0, dtype=np.float64)))


# ---- step 7: the projection -----------------------------------------------------------------------------------------------------
def _moved(t0, t1, t2):
    r, v = differences(t0, t1, t2)
    return ((r != 0) | (v != 0)).any(axis=1)


def project_q(x, t0, t1, t2):
    y = np.where(x < EPS, EPS, x)
    return np.where(_moved(t0, t1, t2)[:, None], ar.normalise_q(y), np.asarray(t0, dtype=np.float64))


def project_f(x, t0, t1, t2):
    return np.where(_moved(t0, t1, t2)[:, None], ar.clamp(x), np.asarray(t0, dtype=np.float64))


def point(Q0, F0, Q1, F1, Q2, F2, a_max=4.0, update_q=True, update_f=True, alpha=None):
    """steps 3 to 7 -> dict(sr, sv, nn, alpha, at_limit, Q_raw, P_raw, Q, P); alpha given: that alpha instead of the sums' own"""
    sr, sv, nn = sums(Q0, F0, Q1, F1, Q2, F2, update_q, update_f)
    al, at_limit = alpha_of(sr, sv, a_max)
    if alpha is not None:
        al = float(alpha)
    Q0, F0 = np.asarray(Q0, dtype=np.float64), np.asarray(F0, dtype=np.float64)
    q_raw = raw(Q0, Q1, Q2, al) if update_q else Q0.copy()
    f_raw = raw(F0, F1, F2, al) if update_f else F0.copy()
    return dict(sr=sr, sv=sv, nn=nn, alpha=al, at_limit=at_limit, Q_raw=q_raw, P_raw=f_raw,
                Q=project_q(q_raw, Q0, Q1, Q2) if update_q else Q0.copy(), P=project_f(f_raw, F0, F1, F2) if update_f else F0.copy())


# ---- the driver -----------------------------------------------------------------------------------------------------------------
def _step(codes, Q, F, update_q, update_f):
    q, f, _ = ar.em_step(codes, Q, F)
    return (q if update_q else Q), (f if update_f else F)


def em_plain(codes, Q0, F0, tol=1e-4, max_iter=1000, update_q=True, update_f=True):
    """the iteration of "admixture" -> dict(Q, P, loglik, n_iter, converged, trace)"""
    Q, F = np.asarray(Q0, dtype=np.float64), np.asarray(F0, dtype=np.float64)
    tr, t, conv = [], 0, False
    while t < max_iter:
        tr.append(ar.loglik(codes, Q, F))
        Q, F = _step(codes, Q, F, update_q, update_f)
        t += 1
        if t >= 2 and tr[t - 1] - tr[t - 2] < tol:
            conv = True
            break
    tr.append(ar.loglik(codes, Q, F))
    return dict(Q=Q, P=F, loglik=tr[-1], n_iter=t, converged=conv, trace=np.array(tr))


def em_squarem(codes, Q0, F0, tol=1e-4, max_iter=1000, update_q=True, update_f=True, a_max=4.0):
    """the driver of "admixture, accelerated" -> dict(Q, P, loglik, n_iter, converged, trace, alpha, accepted, n_cycles, n_rejected,
    cycles = per whole cycle dict(start = the trace index of l(theta0), theta2, next = the state the next cycle starts from))"""
    th0 = (np.asarray(Q0, dtype=np.float64), np.asarray(F0, dtype=np.float64))
    tr, alphas, acc, cycles = [], [], [], []
    t, conv, last = 0, False, th0
    while t < max_iter:
        start = t
        tr.append(ar.loglik(codes, *th0))
        th1 = _step(codes, *th0, update_q, update_f)
        t, last = t + 1, th1
        if t == max_iter:
            break
        tr.append(ar.loglik(codes, *th1))
        th2 = _step(codes, *th1, update_q, update_f)
        t, last = t + 1, th2
        if tr[-1] - tr[-2] < tol:
            conv = True
            break
        if t == max_iter:
            break
        l1 = tr[-1]
        p = point(th0[0], th0[1], th1[0], th1[1], th2[0], th2[1], a_max, update_q, update_f)
        thp = (p["Q"], p["P"])
        tr.append(ar.loglik(codes, *thp))
        thpp = _step(codes, *thp, update_q, update_f)
        t += 1
        ok = accept(tr[-1], l1)
        alphas.append(p["alpha"])
        acc.append(ok)
        a_max = next_limit(a_max, ok, p["at_limit"])
        th0 = thpp if ok else th2
        last = th0
        cycles.append(dict(start=start, theta2=th2, next=th0))
    tr.append(ar.loglik(codes, *last))
    return dict(Q=last[0], P=last[1], loglik=tr[-1], n_iter=t, converged=conv, trace=np.array(tr), alpha=np.array(alphas),
                accepted=np.array(acc, dtype=bool), n_cycles=len(acc), n_rejected=int(len(acc) - sum(acc)), cycles=cycles)
