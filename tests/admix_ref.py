"""The admixture EM of include/tpg.h "admixture" restated in numpy.  ADMIXTURE is not among the reference's sources, so the
header is the definition; this file follows it line by line.  Two routes: a float route (em_step, loglik: float64, numpy's
summation order, no fused multiply-add) and an exact route in fractions.Fraction (em_step_exact, p_exact, loglik_exact), so
that truth does not rest on an order of summation.  Q is n x K; F is held as m x K (the shape of a .P file): F[j, k] = f(k, j).
Also the seeded start in uint64 arithmetic, the rounding bounds of the header, and a small panel simulated from known Q and F
with the awkward columns and row planted."""
import math
from fractions import Fraction

import numpy as np

MISSING = 3
EPS = 1e-5  # TPG_ADMIX_EPS
U = 2.0 ** -52
F_SALT = 0xF0F0F0F0F0F0F0F0
MASK = (1 << 64) - 1


# ---- the hash start ---------------------------------------------------------------------------------------------------------
def mix64(x):
    """tpg_mix64 (the splitmix64 finaliser) on uint64 arrays"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def mix64_int(x):
    """the same on a Python integer"""
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def u_of(h):
    """u(h) = ((double)(h >> 11) + 0.5) * 2^-53 in IEEE double"""
    return ((np.asarray(h, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def start(seed, n, m, K):
    """the seeded start -> Q0 (n x K), F0 (m x K)"""
    seed = np.uint64(seed & MASK)
    ks = mix64(np.arange(K, dtype=np.uint64))[None, :]
    key_q = mix64(seed ^ mix64(np.arange(n, dtype=np.uint64)))[:, None]
    uq = u_of(mix64(key_q ^ ks))
    rs = np.zeros(n)
    for k in range(K):  # the row sum in ascending k
        rs = rs + uq[:, k]
    key_f = mix64((seed ^ np.uint64(F_SALT)) ^ mix64(np.arange(m, dtype=np.uint64)))[:, None]
    uf = u_of(mix64(key_f ^ ks))
    return uq / rs[:, None], 0.1 + 0.8 * uf


def normalise_q(Q0):
    Q0 = np.asarray(Q0, dtype=np.float64)
    rs = np.zeros(Q0.shape[0])
    for k in range(Q0.shape[1]):
        rs = rs + Q0[:, k]
    return Q0 / rs[:, None]


def clamp(F):
    return np.minimum(np.maximum(np.asarray(F, dtype=np.float64), EPS), 1.0 - EPS)


# ---- float route ------------------------------------------------------------------------------------------------------------
def _p_pbar(Q, F):
    n, K = Q.shape
    p, pb = np.zeros((n, F.shape[0])), np.zeros((n, F.shape[0]))
    for k in range(K):  # ascending k
        p = p + Q[:, k][:, None] * F[:, k][None, :]
        pb = pb + Q[:, k][:, None] * (1.0 - F[:, k])[None, :]
    return p, pb


def loglik(codes, Q, F):
    """l(Q, F) = sum over typed (i, j) of g ln p + (2 - g) ln pbar"""
    codes = np.asarray(codes)
    typed = codes != MISSING
    g = np.where(typed, codes, 0).astype(np.float64)
    p, pb = _p_pbar(np.asarray(Q, dtype=np.float64), np.asarray(F, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        term = g * np.log(p) + (2.0 - g) * np.log(pb)
    return float(np.where(typed, term, 0.0).sum())


def em_step(codes, Q, F):
    """one EM step from (Q, F) -> Q', F' (clamped), F' before the clamp"""
    codes = np.asarray(codes)
    Q, F = np.asarray(Q, dtype=np.float64), np.asarray(F, dtype=np.float64)
    typed = codes != MISSING
    g = np.where(typed, codes, 0).astype(np.float64)
    p, pb = _p_pbar(Q, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        w1 = np.where(typed, g / p, 0.0)
        w0 = np.where(typed, (2.0 - g) / pb, 0.0)
    a = F * (w1.T @ Q)             # m x K: f * sum_i q w1
    b = (1.0 - F) * (w0.T @ Q)
    with np.errstate(divide="ignore", invalid="ignore"):
        f_raw = a / (a + b)
    keep_f = (typed.sum(axis=0) == 0)[:, None] | ((a + b) == 0)
    f_raw = np.where(keep_f, F, f_raw)
    f_new = np.where(keep_f, F, clamp(f_raw))
    t_i = typed.sum(axis=1).astype(np.float64)
    s = w1 @ F + w0 @ (1.0 - F)    # n x K
    with np.errstate(divide="ignore", invalid="ignore"):
        q_new = (Q / (2.0 * t_i)[:, None]) * s
    q_new = np.where((t_i == 0)[:, None], Q, q_new)
    return q_new, f_new, f_raw


# ---- exact route ------------------------------------------------------------------------------------------------------------
def _frac(A):
    return [[Fraction(float(x)) for x in row] for row in np.asarray(A, dtype=np.float64)]


def p_exact(Q, F):
    """p, pbar of every (i, j) as Fractions of the doubles in Q and F"""
    q, f = _frac(Q), _frac(F)
    n, m, K = len(q), len(f), len(q[0])
    p = [[sum(q[i][k] * f[j][k] for k in range(K)) for j in range(m)] for i in range(n)]
    pb = [[sum(q[i][k] * (1 - f[j][k]) for k in range(K)) for j in range(m)] for i in range(n)]
    return p, pb


def em_step_exact(codes, Q, F):
    """the exact rational step -> q' (n x K), unclamped f' (m x K) as lists of Fractions; a kept f / row comes back as it is"""
    codes = np.asarray(codes)
    q, f = _frac(Q), _frac(F)
    n, m, K = len(q), len(f), len(q[0])
    p, pb = p_exact(Q, F)
    f_new = [[f[j][k] for k in range(K)] for j in range(m)]
    q_new = [[q[i][k] for k in range(K)] for i in range(n)]
    for j in range(m):
        rows = [i for i in range(n) if codes[i, j] != MISSING]
        if not rows:
            continue
        for k in range(K):
            a = f[j][k] * sum(q[i][k] * int(codes[i, j]) / p[i][j] for i in rows)
            b = (1 - f[j][k]) * sum(q[i][k] * (2 - int(codes[i, j])) / pb[i][j] for i in rows)
            if a + b != 0:
                f_new[j][k] = a / (a + b)
    for i in range(n):
        cols = [j for j in range(m) if codes[i, j] != MISSING]
        if not cols:
            continue
        for k in range(K):
            s = sum(f[j][k] * int(codes[i, j]) / p[i][j] + (1 - f[j][k]) * (2 - int(codes[i, j])) / pb[i][j] for j in cols)
            q_new[i][k] = q[i][k] / (2 * len(cols)) * s
    return q_new, f_new


def _ln_frac(x):
    """math.log of the correctly rounded exact value"""
    return math.log(x.numerator / x.denominator)  # int / int is correctly rounded in Python


def loglik_exact(codes, Q, F):
    """the exact p and pbar, correctly rounded, through math.log; the terms added with math.fsum"""
    codes = np.asarray(codes)
    p, pb = p_exact(Q, F)
    terms = []
    for i in range(codes.shape[0]):
        for j in range(codes.shape[1]):
            g = int(codes[i, j])
            if g == MISSING:
                continue
            if g > 0:
                terms.append(g * _ln_frac(p[i][j]))
            if g < 2:
                terms.append((2 - g) * _ln_frac(pb[i][j]))
    return math.fsum(terms)


# ---- the bounds of the header ---------------------------------------------------------------------------------------------------
def bound_f(n, K, f):
    return (2 * n + 4 * K + 40) * U * np.abs(f)


def bound_q(t_i, K, q):
    return (2 * np.asarray(t_i, dtype=np.float64)[:, None] + 2 * K + 16) * U * np.abs(q)


def bound_ll(T, K, ll):
    return U * ((2 * T + 2) * abs(ll) + 2 * (K + 4) * T)


# ---- a panel ------------------------------------------------------------------------------------------------------------------
def panel(seed, n, m, K, miss):
    """n x m uint8 codes simulated from a known Q (Dirichlet rows) and F (uniform 0.05 .. 0.95), a share `miss` of the entries
    missing; planted: column 0 all missing, column 1 all 0, column 2 all 2 (as far as m reaches), and the last row all missing
    (n > 1).  -> codes, Q_true, F_true (m x K), planted = dict(col_missing, col_all0, col_all2, row_missing) of indices / None"""
    rng = np.random.default_rng(seed)
    Qt = rng.dirichlet(np.full(K, 0.5), size=n)
    Ft = rng.uniform(0.05, 0.95, size=(m, K))
    codes = rng.binomial(2, Qt @ Ft.T).astype(np.uint8)
    if miss > 0:
        codes[rng.random((n, m)) < miss] = MISSING
    planted = dict(col_missing=None, col_all0=None, col_all2=None, row_missing=None)
    if m > 3:
        codes[:, 0] = MISSING
        planted["col_missing"] = 0
        codes[:, 1] = np.where(codes[:, 1] == MISSING, MISSING, 0)
        codes[0, 1] = 0
        planted["col_all0"] = 1
        codes[:, 2] = np.where(codes[:, 2] == MISSING, MISSING, 2)
        codes[0, 2] = 2
        planted["col_all2"] = 2
    if n > 1:
        codes[n - 1, :] = MISSING
        planted["row_missing"] = n - 1
    return codes, Qt, Ft, planted
