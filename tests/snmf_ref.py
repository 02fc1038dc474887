"""The sNMF of include/tpg.h "sNMF" restated in numpy.  LEA is not among the reference's sources, so the header is the definition;
this file follows it line by line.  The exact solver is scipy.optimize.nnls on the Cholesky factor: with C = R'R,
argmin_{x >= 0} x'Cx / 2 - b'x = argmin_{x >= 0} |R x - R^-T b|^2.  An iteration is two halves, g_half (Q -> G) and q_half (G -> Q'),
so that a test can feed the device's own G into the second half.  G is held as (m, 3, K); g_matrix() gives the 3M x K form of
the C ABI (row 3 j + c).  Also the hold-out by fraction in uint64 arithmetic, the cross-entropy sums, the bounds the GPU tests
use, and the two-population panel of the choice-of-K test."""
import numpy as np
import scipy.linalg
import scipy.optimize

from tests import admix_ref as ar

MISSING = 3
MAX_K = 16          # TPG_SNMF_MAX_K
RIDGE = 1e-10       # TPG_SNMF_RIDGE
TINY = 1e-9         # TPG_SNMF_TINY
KKT_TOL = 1e-12     # TPG_SNMF_KKT_TOL
P_FLOOR = 1e-9      # TPG_SNMF_P_FLOOR
U = 2.0 ** -52
CV_SALT = 0xC3C3C3C3C3C3C3C3


# ---- the pieces of one iteration ------------------------------------------------------------------------------------------
def ridge(C, alpha=0.0):
    """ridge(C + alpha 1 1'): rho = (RIDGE * trace) / K, the trace in ascending k"""
    C = np.asarray(C, dtype=np.float64) + alpha
    K = C.shape[0]
    tr = 0.0
    for k in range(K):
        tr = tr + C[k, k]
    return C + ((RIDGE * tr) / K) * np.eye(K)


def nnls_exact(A, B):
    """NNLS(A, b) for every row b of B -> X (rows x K)"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    R = np.linalg.cholesky(A).T
    Y = scipy.linalg.solve_triangular(R.T, B.T, lower=True).T
    X = np.zeros_like(B)
    for r in range(B.shape[0]):
        if (B[r] > 0).any():  # b <= 0 everywhere: x = 0
            X[r] = scipy.optimize.nnls(R, Y[r])[0]
    return X


def kkt_residual(A, b, x):
    """the residual of the contract: max over k of |w(k)| where x(k) > 0 and of max(w(k), 0) where x(k) = 0, w = b - A x"""
    w = b - A @ x
    return float(np.max(np.where(x > 0, np.abs(w), np.maximum(w, 0.0))))


def rhs_g(codes, Q):
    """b(j, c, .) = sum over the i with g(i, j) = c of Q(i, .) -> (m, 3, K)"""
    codes = np.asarray(codes)
    return np.stack([(codes == c).T.astype(np.float64) @ Q for c in range(3)], axis=1)


def rhs_q(codes, G):
    """b_i = sum over the typed j of G(j, g(i, j), .) -> (n, K)"""
    codes = np.asarray(codes)
    out = np.zeros((codes.shape[0], G.shape[2]))
    for c in range(3):
        out = out + (codes == c).astype(np.float64) @ G[:, c, :]
    return out


def g_half(codes, Q):
    """steps 1 - 3 -> dict(G (m, 3, K), gt (unnormalised), s (m, K), A, b (m, 3, K))"""
    Q = np.asarray(Q, dtype=np.float64)
    m, K = np.asarray(codes).shape[1], Q.shape[1]
    A = ridge(Q.T @ Q)
    b = rhs_g(codes, Q)
    gt = nnls_exact(A, b.reshape(3 * m, K)).reshape(m, 3, K)
    s = (gt[:, 0, :] + gt[:, 1, :]) + gt[:, 2, :]
    live = s > TINY
    with np.errstate(divide="ignore", invalid="ignore"):
        G = np.where(live[:, None, :], gt / s[:, None, :], 1.0 / 3.0)
    return dict(G=G, gt=gt, s=s, A=A, b=b)


def q_half(codes, G, alpha):
    """steps 4 - 5 and the criterion -> dict(Q (n, K), qt, r (n), B, b (n, K), GG, ls, T)"""
    codes, G = np.asarray(codes), np.asarray(G, dtype=np.float64)
    m, _, K = G.shape
    G2 = G.reshape(3 * m, K)
    GG = G2.T @ G2
    B = ridge(GG, alpha)
    b = rhs_q(codes, G)
    qt = nnls_exact(B, b)
    r = np.zeros(qt.shape[0])
    for k in range(K):
        r = r + qt[:, k]
    live = r > TINY
    with np.errstate(divide="ignore", invalid="ignore"):
        Q = np.where(live[:, None], qt / r[:, None], 1.0 / K)
    T = int((codes != MISSING).sum())
    sqb, dot = float((Q * b).sum()), float(((Q.T @ Q) * GG).sum())
    return dict(Q=Q, qt=qt, r=r, B=B, b=b, GG=GG, ls=(T - 2.0 * sqb) + dot, T=T, sqb=sqb, dot=dot)


def step(codes, Q, alpha):
    """one iteration from Q -> dict(Q, G (m, 3, K), ls)"""
    g = g_half(codes, Q)
    q = q_half(codes, g["G"], alpha)
    return dict(Q=q["Q"], G=g["G"], ls=q["ls"])


def run(codes, K, q0=None, seed=0, alpha=10.0, tol=1e-5, max_iter=200):
    """the iteration of the header -> dict(Q, G, ls, trace, n_iter, converged)"""
    n, m = np.asarray(codes).shape
    Q = ar.start(seed, n, m, K)[0] if q0 is None else ar.normalise_q(q0)
    G = np.full((m, 3, K), 1.0 / 3.0)
    trace, conv = [], False
    while len(trace) < max_iter:
        r = step(codes, Q, alpha)
        Q, G = r["Q"], r["G"]
        trace.append(r["ls"])
        t = len(trace)
        if t >= 2 and abs(trace[t - 2] - trace[t - 1]) <= tol * trace[t - 2]:
            conv = True
            break
    return dict(Q=Q, G=G, ls=trace[-1] if trace else float("nan"), trace=np.array(trace), n_iter=len(trace), converged=conv)


def g_matrix(G):
    """(m, 3, K) -> 3M x K, row 3 j + c"""
    G = np.asarray(G)
    return G.reshape(3 * G.shape[0], G.shape[2])


def g_cube(Gm):
    Gm = np.asarray(Gm)
    return Gm.reshape(Gm.shape[0] // 3, 3, Gm.shape[1])


def p_of(G):
    """P(j, k) = G(j, 1, k) / 2 + G(j, 2, k)"""
    return G[:, 1, :] / 2.0 + G[:, 2, :]


def loss_direct(codes, Q, G):
    """|X - Q G'|^2 formed directly: X the n x 3m indicator matrix (a missing entry: three zeros)"""
    codes = np.asarray(codes)
    X = np.stack([(codes == c) for c in range(3)], axis=2).astype(np.float64)  # n x m x 3
    fit = np.einsum("ik,jck->ijc", Q, G)
    return float(((X - fit) ** 2).sum())


# ---- hold-out and cross-entropy -----------------------------------------------------------------------------------------------
def hash_of(seed, n, m):
    """h(i, j) of "admixture cross-validation" for every position of an n x m view -> uint64 (n, m)"""
    key = ar.mix64((np.uint64(seed & ar.MASK) ^ np.uint64(CV_SALT)) ^ ar.mix64(np.arange(m, dtype=np.uint64)))
    return ar.mix64(key[None, :] ^ ar.mix64(np.arange(n, dtype=np.uint64))[:, None])


def holdout_fraction(codes, fraction, seed):
    """the training codes: every typed entry with (h >> 32) < floor(fraction 2^32) set to code 3"""
    codes = np.asarray(codes)
    thr = np.uint64(int(np.floor(fraction * 4294967296.0)))
    held = (codes != MISSING) & ((hash_of(seed, *codes.shape) >> np.uint64(32)) < thr)
    train = codes.copy()
    train[held] = MISSING
    return train


def cross_entropy_sums(codes, train, Q, G):
    """-> dict(sum_masked, n_masked, sum_all, n_all); G (m, 3, K); Q and G as given"""
    codes, train = np.asarray(codes), np.asarray(train)
    g = np.where(train != MISSING, train, codes)
    p = np.zeros(codes.shape)
    Gs = np.stack([G[np.arange(G.shape[0]), np.minimum(g[i], 2), :] for i in range(codes.shape[0])])  # n x m x K
    for k in range(Q.shape[1]):
        p = p + Q[:, k][:, None] * Gs[:, :, k]
    term = -np.log(np.maximum(p, P_FLOOR))
    allm, masked = train != MISSING, (train == MISSING) & (codes != MISSING)
    return dict(sum_masked=float(term[masked].sum()), n_masked=int(masked.sum()), sum_all=float(term[allm].sum()), n_all=int(allm.sum()))


# ---- the bounds ---------------------------------------------------------------------------------------------------------------
def bound_nnls(A, B):
    """|x - x*| <= sqrt(K) tau |b|_inf / lambda_min(A): two points that both meet the contract lie this close to the optimum (the
    solution map of a strongly convex problem is Lipschitz with constant 1 / lambda_min) -> one bound per row of B"""
    K = A.shape[0]
    return np.sqrt(K) * KKT_TOL * np.abs(B).max(axis=1) / np.linalg.eigvalsh(A)[0]


def bound_x(A, B, X, n_t):
    """tol_x per system: [sqrt(K) tau |b|_inf + 2 (n_t + K + 4) u (|A|_F |x*|_2 + |b|_2)] / lambda_min; n_t = the longest sum
    feeding A or b"""
    K = A.shape[0]
    lam = np.linalg.eigvalsh(A)[0]
    return (np.sqrt(K) * KKT_TOL * np.abs(B).max(axis=1)
            + 2 * (n_t + K + 4) * U * (np.linalg.norm(A) * np.linalg.norm(X, axis=1) + np.linalg.norm(B, axis=1))) / lam


def bound_ls(n_t, T, sqb, dot):
    """|d ls| <= 4 n_t u (T + |terms|): the three terms of ls are T, 2 sum q.b and the product of the Gram matrices"""
    return 4 * n_t * U * (T + 2 * abs(sqb) + abs(dot))


def bound_ce(T, K, S):
    return U * ((T + 2) * abs(S) + (K + 2) * T)


# ---- the panel of the choice-of-K test ------------------------------------------------------------------------------------------
def k_panel(seed=2024, n_each=(50, 50, 30), m=400, miss=0.02):
    """two populations with independent U(0.05, 0.95) frequencies; n_each = pure in the first, pure in the second, admixed
    (proportion U(0, 1)); a share `miss` of the entries missing -> codes (n x m uint8), Q_true"""
    rng = np.random.default_rng(seed)
    a, b, c = n_each
    q1 = np.concatenate([np.ones(a), np.zeros(b), rng.uniform(0, 1, size=c)])
    Qt = np.stack([q1, 1.0 - q1], axis=1)
    Ft = rng.uniform(0.05, 0.95, size=(m, 2))
    codes = rng.binomial(2, Qt @ Ft.T).astype(np.uint8)
    codes[rng.random(codes.shape) < miss] = MISSING
    return codes, Qt


def cross_entropy_of_k(codes, K, fraction, mask_seed, seed, alpha, tol, max_iter):
    """the reference's own masked cross-entropy of one K: the fit on the hold-out codes, as LEA's is"""
    train = holdout_fraction(codes, fraction, mask_seed)
    r = run(train, K, seed=seed, alpha=alpha, tol=tol, max_iter=max_iter)
    s = cross_entropy_sums(codes, train, r["Q"], r["G"])
    return s["sum_masked"] / s["n_masked"], r
