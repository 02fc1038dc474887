"""numpy restatement of include/tpg.h "pcadapt": z-scores of the regression on the PCA scores, medians and MADs as exact
selections, the OGK robust distance (median / MAD, two iterations), genomic control and the chi-square tail.

Two routes.  The float route follows the header statement for statement in IEEE doubles (numpy's elementwise operations round
once each and fuse nothing).  The extended route runs the same formulas in mpmath at 50 digits (where mpmath is there): it is
what the per-cell error bound of the z-scores is evaluated against and what measures the float route's own error in `dist`.
logq_ref is pure `math`: the finite sums of the header for an integer number of degrees of freedom."""
import math

import numpy as np

try:
    import mpmath
except ImportError:  # the tests that need it use pytest.importorskip
    mpmath = None

MAD_SCALE = 1.4826
EPS = 2.0 ** -53
MAX_K = 64


# ---- column statistics ------------------------------------------------------------------------------------------------------
def med(x):
    """median over the finite entries, -0 read as +0: s[(c-1)/2] or (s[c/2-1] + s[c/2]) / 2; NaN if there is none"""
    x = np.asarray(x, dtype=np.float64) + 0.0
    s = np.sort(x[np.isfinite(x)])
    c = len(s)
    if c == 0:
        return np.nan
    if c % 2:
        return s[(c - 1) // 2]
    return (s[c // 2 - 1] + s[c // 2]) / 2


def mad(x):
    x = np.asarray(x, dtype=np.float64) + 0.0
    x = x[np.isfinite(x)]
    with np.errstate(over="ignore", invalid="ignore"):
        return med(np.abs(x - med(x)))


def sigma(x):
    return MAD_SCALE * mad(x)


# ---- the panel of the definition-level test ---------------------------------------------------------------------------------
N_POP, PER_POP, M_PANEL, FST = 3, 32, 1500, 0.05
PLANTED = np.array([97 * i + 5 for i in range(15)])
MONO = {700: 0, 701: 2, 702: 1}  # locus -> the genotype everybody has


def panel(seed=0):
    """96 x 1500 genotypes (0 / 1 / 2) from one default_rng(seed), drawn in the order of the statements below: ancestral
    frequencies, Balding-Nichols population frequencies (one call), the planted loci overwritten, genotypes population by
    population, three loci made monomorphic"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, M_PANEL)
    P = rng.beta(p * (1 - FST) / FST, (1 - p) * (1 - FST) / FST, size=(N_POP, M_PANEL))
    P = np.clip(P, 0.02, 0.98)
    P[0, PLANTED], P[1, PLANTED], P[2, PLANTED] = 0.9, 0.1, 0.1
    G = np.concatenate([rng.binomial(2, P[g], size=(PER_POP, M_PANEL)) for g in range(N_POP)], axis=0)
    for j, g in MONO.items():
        G[:, j] = g
    return G.astype(np.int64)


def svd_scores(G, k):
    """the first k left singular vectors of the binomially scaled matrix (what a PCA of the panel returns as u)"""
    G = np.asarray(G, dtype=np.float64)
    mean = G.mean(axis=0)
    p = mean / 2
    sd = np.sqrt(2 * p * (1 - p))
    keep = sd > 0
    Z = (G[:, keep] - mean[keep]) / sd[keep]
    u, _, _ = np.linalg.svd(Z, full_matrices=False)
    return np.asfortranarray(u[:, :k])


# ---- z-scores ---------------------------------------------------------------------------------------------------------------
def counts_tot(G):
    """S1, S2 and tot = (n S2 - S1^2) / n from exact integers"""
    G = np.asarray(G, dtype=np.int64)
    n = G.shape[0]
    n1, n2 = (G == 1).sum(axis=0), (G == 2).sum(axis=0)
    S1, S2 = n1 + 2 * n2, n1 + 4 * n2
    return S1, S2, (n * S2 - S1 * S1).astype(np.float64) / float(n)


def zscores_ref(G, U):
    """float route -> dict(z (m x K, NaN rows where invalid), beta, tot, rss, valid)"""
    G = np.asarray(G, dtype=np.int64)
    U = np.asarray(U, dtype=np.float64)
    n, m = G.shape
    K = U.shape[1]
    S1, _, tot = counts_tot(G)
    mean = S1.astype(np.float64) / float(n)
    beta = (G.astype(np.float64) - mean).T @ U
    rss = tot.copy()
    for k in range(K):
        rss = rss - beta[:, k] * beta[:, k]
    valid = (tot != 0.0) & (rss > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = beta / np.sqrt(rss / float(n - K - 1))[:, None]
    z[~valid] = np.nan
    return dict(z=z, beta=beta, tot=tot, rss=rss, valid=valid)


def zscores_ext(G, U):
    """extended route: sum_i g_ij U_ik and sum_i U_ik by math.fsum (the products g U are exact, so each sum is the correctly
    rounded value of the exact one), the rest in mpmath at 50 digits -> dict of object arrays beta, rss, z and float tot"""
    mp = mpmath.mp.clone()
    mp.dps = 50
    G = np.asarray(G, dtype=np.int64)
    U = np.asarray(U, dtype=np.float64)
    n, m = G.shape
    K = U.shape[1]
    S1, S2, tot = counts_tot(G)
    colsum = [math.fsum(U[:, k]) for k in range(K)]
    beta = np.empty((m, K), dtype=object)
    rss = np.empty(m, dtype=object)
    z = np.empty((m, K), dtype=object)
    Uk = [U[:, k].tolist() for k in range(K)]
    for j in range(m):
        g = G[:, j].tolist()
        mean = mp.mpf(int(S1[j])) / n
        r = mp.mpf(int(n * S2[j] - S1[j] * S1[j])) / n
        for k in range(K):
            a = math.fsum(gi * ui for gi, ui in zip(g, Uk[k]))
            beta[j, k] = mp.mpf(a) - mean * mp.mpf(colsum[k])
            r = r - beta[j, k] * beta[j, k]
        rss[j] = r
        for k in range(K):
            z[j, k] = beta[j, k] / mp.sqrt(r / (n - K - 1)) if (tot[j] != 0 and r > 0) else mp.nan
    return dict(beta=beta, rss=rss, z=z, tot=tot)


def zscore_bounds(n, K, ext):
    """the per-cell bounds of the header on |d beta| and |d z|, evaluated from the extended route (float arrays, NaN rows where
    the locus is invalid)"""
    tot = ext["tot"]
    m = len(tot)
    beta = np.array([[float(b) for b in row] for row in ext["beta"]], dtype=np.float64).reshape(m, K)
    rss = np.array([float(r) for r in ext["rss"]], dtype=np.float64)
    z = np.array([[float(b) for b in row] for row in ext["z"]], dtype=np.float64).reshape(m, K)
    dbeta = n * EPS * np.sqrt(tot) + EPS * 2 * math.sqrt(n)
    drss = 2 * np.abs(beta).sum(axis=1) * dbeta + (K + 1) * EPS * tot
    with np.errstate(divide="ignore", invalid="ignore"):
        dz = dbeta[:, None] * np.sqrt((n - K - 1) / rss)[:, None] + np.abs(z) * (drss / (2 * rss))[:, None] + 3 * EPS * np.abs(z)
    return dict(beta=beta, rss=rss, z=z, dbeta=np.repeat(dbeta[:, None], K, axis=1), dz=dz)


# ---- OGK --------------------------------------------------------------------------------------------------------------------
def _pairs(K):
    return [(a, b) for a in range(K) for b in range(a + 1, K)]


def backmap(K, s1, E1, s2, E2, nu, gamma):
    """center = B nu, cov = B diag(gamma) B' with B = (D1 E1)(D2 E2), in the loop order of host_ogk_backmap"""
    B = [[0.0] * K for _ in range(K)]
    for i in range(K):
        for j in range(K):
            acc = 0.0
            for l in range(K):
                a1 = float(s1[i]) * float(E1[i][l])
                a2 = float(s2[l]) * float(E2[l][j])
                acc = acc + a1 * a2
            B[i][j] = acc
    center, cov = np.zeros(K), np.zeros((K, K))
    for i in range(K):
        acc = 0.0
        for k in range(K):
            acc = acc + B[i][k] * float(nu[k])
        center[i] = acc
        for j in range(K):
            c = 0.0
            for k in range(K):
                c = c + (B[i][k] * float(gamma[k])) * B[j][k]
            cov[i, j] = c
    return center, cov


def ogk_ref(Z, basis=None):
    """float route of step 3 -> dict(dist (NaN where the row is invalid), center, cov, R = [R1, R2], E = [E1, E2],
    gaps = the smallest eigengap of each iteration (inf for K = 1), n_valid).  basis: the two eigenvector matrices to use
    (columns = eigenvectors) instead of numpy's eigh.  Raises ValueError where the library returns TPG_ENUMERIC."""
    Z = np.asarray(Z, dtype=np.float64)
    m, K = Z.shape
    valid = np.isfinite(Z).all(axis=1)
    X = Z[valid].copy()
    if X.shape[0] < K + 2:
        raise ValueError("fewer than K + 2 valid rows")
    Rs, Es, ss, gaps = [], [], [], []
    for t in range(2):
        s = np.array([sigma(X[:, k]) for k in range(K)])
        if not (np.isfinite(s).all() and (s > 0).all()):
            raise ValueError("a column scale is zero or not finite")
        Y = X / s
        R = np.eye(K)
        for a, b in _pairs(K):
            sp, sm = sigma(Y[:, a] + Y[:, b]), sigma(Y[:, a] - Y[:, b])
            if not (np.isfinite([sp, sm]).all() and sp > 0 and sm > 0):
                raise ValueError("a pairwise scale is zero or not finite")
            R[a, b] = R[b, a] = (sp * sp - sm * sm) / 4
        if basis is not None:
            E = np.asarray(basis[t], dtype=np.float64)
            lam = np.sort(np.diag(E.T @ R @ E))[::-1]
        elif K == 1:
            E, lam = np.ones((1, 1)), np.ones(1)
        else:
            lam, E = np.linalg.eigh(R)
            lam, E = lam[::-1], E[:, ::-1]
        gaps.append(float(np.min(-np.diff(lam))) if K > 1 else math.inf)
        W = np.zeros_like(Y)
        for k in range(K):
            acc = np.zeros(Y.shape[0])
            for a in range(K):
                acc = acc + Y[:, a] * E[a, k]
            W[:, k] = acc
        X = W
        Rs.append(R), Es.append(E), ss.append(s)
    nu = np.array([med(X[:, k]) for k in range(K)])
    sg = np.array([sigma(X[:, k]) for k in range(K)])
    if not (np.isfinite(sg).all() and (sg > 0).all()):
        raise ValueError("a final scale is zero or not finite")
    gamma = sg * sg
    acc = np.zeros(X.shape[0])
    for k in range(K):
        d = X[:, k] - nu[k]
        acc = acc + (d * d) / gamma[k]
    dist = np.full(m, np.nan)
    dist[valid] = acc
    center, cov = backmap(K, ss[0], Es[0], ss[1], Es[1], nu, gamma)
    return dict(dist=dist, center=center, cov=cov, R=Rs, E=Es, gaps=gaps, n_valid=int(valid.sum()), nu=nu, gamma=gamma)


def ogk_ext(Z):
    """the same at 50 digits (mpmath; its own symmetric eigen solver) -> dist as floats (NaN where invalid)"""
    mp = mpmath.mp.clone()
    mp.dps = 50
    Z = np.asarray(Z, dtype=np.float64)
    m, K = Z.shape
    valid = np.isfinite(Z).all(axis=1)
    cols = [[mp.mpf(float(x)) for x in Z[valid, k]] for k in range(K)]
    M = len(cols[0])

    def xmed(v):
        s = sorted(v)
        c = len(s)
        return s[(c - 1) // 2] if c % 2 else (s[c // 2 - 1] + s[c // 2]) / 2

    def xsigma(v):
        c0 = xmed(v)
        return mp.mpf(MAD_SCALE) * xmed([abs(x - c0) for x in v])

    for _ in range(2):
        s = [xsigma(c) for c in cols]
        Y = [[x / s[k] for x in cols[k]] for k in range(K)]
        R = mp.eye(K)
        for a, b in _pairs(K):
            sp = xsigma([x + y for x, y in zip(Y[a], Y[b])])
            sm = xsigma([x - y for x, y in zip(Y[a], Y[b])])
            R[a, b] = R[b, a] = (sp * sp - sm * sm) / 4
        if K == 1:
            E = mp.eye(1)
        else:
            lam, E = mp.eigsy(R)
            order = sorted(range(K), key=lambda i: -lam[i])
            E = mp.matrix([[E[a, i] for i in order] for a in range(K)])
        cols = [[sum((Y[a][j] * E[a, k] for a in range(K)), mp.mpf(0)) for j in range(M)] for k in range(K)]
    nu = [xmed(c) for c in cols]
    gamma = [xsigma(c) ** 2 for c in cols]
    acc = [sum(((cols[k][j] - nu[k]) ** 2 / gamma[k] for k in range(K)), mp.mpf(0)) for j in range(M)]
    dist = np.full(m, np.nan)
    dist[valid] = [float(x) for x in acc]
    return dist


# ---- chi-square -------------------------------------------------------------------------------------------------------------
def logq_ref(K, x):
    """log of the upper tail of chi-square(K) at x in pure math, the finite sums: h = x / 2; even K: -h + log(sum_{i < K/2}
    h^i / i!); odd K: log(erfc(sqrt h) + e^-h sum_{i < (K-1)/2} h^(i + 1/2) / Gamma(i + 3/2))"""
    h = x / 2
    if K % 2 == 0:
        term, s = 1.0, 1.0
        for i in range(1, K // 2):
            term = term * h / float(i)
            s += term
        return -h + math.log(s)
    r = math.sqrt(h)
    term, s = r / 0.886226925452758013649, 0.0
    for i in range((K - 1) // 2):
        if i > 0:
            term = term * h / (float(i) + 0.5)
        s += term
    return math.log(math.erfc(r) + math.exp(-h) * s)


def logq_mp(K, x):
    """the same from mpmath's regularised upper incomplete gamma function at 50 digits (a float)"""
    mp = mpmath.mp.clone()
    mp.dps = 50
    if x == 0:
        return 0.0
    return float(mp.log(mp.gammainc(mp.mpf(K) / 2, mp.mpf(x) / 2, mp.inf, regularized=True)))


# the chi-square arguments the host and the GPU tests share
LOGQ_K = (1, 3, 21, 2, 20, 64)
ODD_FAR = (1500.0, 1e4, 1e6)  # where the erfc form of an odd K underflows: mpmath alone


def logq_points(K):
    """both ends, the series / continued-fraction switch x / 2 = K / 2 + 1 and its neighbours"""
    sw = float(K) + 2.0
    return [0.0, 1e-300, 1e-8, float(K), np.nextafter(sw, 0.0), sw, np.nextafter(sw, 1e9), 50.0, 700.0] + ([1e4, 1e6] if K % 2 == 0 else [])


def qchisq_median_ref(K):
    """the root of logq_ref(K, x) = log(1/2) by bisection on [0, 2 K + 8] to neighbouring doubles; the upper end"""
    target = math.log(0.5)
    lo, hi = 0.0, 2.0 * K + 8.0
    while True:
        mid = lo + (hi - lo) / 2
        if not (lo < mid < hi):
            break
        if logq_ref(K, mid) > target:
            lo = mid
        else:
            hi = mid
    return hi


def pcadapt_ref(G, U, basis=None):
    """steps 1 - 4 -> dict(z, dist, stat, log10p, gc_lambda, n_valid, ogk = the ogk_ref result)"""
    K = np.asarray(U).shape[1]
    zs = zscores_ref(G, U)
    o = ogk_ref(zs["z"], basis=basis)
    lam = med(o["dist"]) / qchisq_median_ref(K)
    stat = o["dist"] / lam
    return dict(z=zs["z"], dist=o["dist"], stat=stat, gc_lambda=lam, n_valid=int(zs["valid"].sum()), ogk=o, zs=zs)


def pcadapt_ext(G, U):
    """steps 1 - 3 at 50 digits: the extended z-scores (rounded to doubles once) through ogk_ext -> dict(ext = the zscores_ext
    result, dist as floats)"""
    ext = zscores_ext(G, U)
    m, K = ext["z"].shape
    z = np.array([[float(x) for x in row] for row in ext["z"]], dtype=np.float64).reshape(m, K)
    return dict(ext=ext, dist=ogk_ext(z))


def ulp_diff(a, b):
    """distance in units in the last place between two float64 arrays of one shape (NaN against NaN: 0)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    both_nan = np.isnan(a) & np.isnan(b)

    def lin(x):
        i = x.view(np.int64)
        return np.where(i < 0, np.int64(-(2 ** 63)) - i, i)  # int64: monotone in the value, -0 and +0 coincide

    d = np.abs(lin(a) - lin(b)).astype(np.float64)
    d[both_nan] = 0
    d[np.isnan(a) ^ np.isnan(b)] = np.inf
    return d
