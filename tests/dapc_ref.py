"""numpy restatement of include/tpg.h "DAPC" (it follows the header, not csrc/host/host_lda.h): the discriminant analysis by the
symmetric square root of W instead of its Cholesky factor -- the generalised eigenvectors of (B, W) with S'WS = I are unique up
to sign where the eigenvalues are distinct, and the header's sign rule settles that -- then the coordinates, the posteriors and
the per-locus loadings."""
import numpy as np

TILE = 256


class Refused(Exception):
    def __init__(self, code, why):
        super().__init__(why)
        self.code = code


def lda(X, grp, n_da=None):
    X = np.asarray(X, dtype=np.float64)
    grp = np.asarray(grp)
    n, d = X.shape
    G = int(grp.max()) + 1
    if G < 2 or n <= G or not 1 <= d <= 64 or grp.min() < 0:
        raise Refused(1, "shape")
    cnt = np.bincount(grp, minlength=G)
    if (cnt == 0).any():
        raise Refused(1, "an empty group")
    if not np.isfinite(X).all():
        raise Refused(4, "not finite")
    pi = cnt / n
    mg = np.stack([X[grp == g].mean(axis=0) for g in range(G)])
    mu = pi @ mg
    r = X - mg[grp]
    W = r.T @ r / (n - G)
    dm = mg - mu
    B = (dm * cnt[:, None]).T @ dm / (G - 1)
    # the header's refusal: a Cholesky pivot that is nothing beside the variable's total variance
    T = ((X - mu) ** 2).sum(axis=0) / (n - 1)
    Rc = np.zeros((d, d))
    for j in range(d):
        piv = W[j, j] - Rc[:j, j] @ Rc[:j, j]
        if not piv > T[j] * 2.0 ** -40:
            raise Refused(4, "W is singular")
        Rc[j, j] = np.sqrt(piv)
        Rc[j, j + 1:] = (W[j, j + 1:] - Rc[:j, j] @ Rc[:j, j + 1:]) / Rc[j, j]
    w, Q = np.linalg.eigh(W)
    Wm = Q @ np.diag(w ** -0.5) @ Q.T
    lam, E = np.linalg.eigh(Wm @ B @ Wm)
    lam, E = lam[::-1], E[:, ::-1]
    lmax = min(d, G - 1)
    L = 0
    while L < lmax and lam[L] > 1e-10:
        L += 1
    S = (Wm @ E)[:, :L].copy()
    for a in range(L):
        big = int(np.argmax(np.abs(S[:, a])))
        if S[big, a] < 0:
            S[:, a] = -S[:, a]
    nda = min(lmax if n_da is None else n_da, lmax, L)
    if nda < 1:
        raise Refused(4, "no discriminant function")
    Z = (X - mu) @ S[:, :nda]
    M = (mg - mu) @ S[:, :nda]
    q = 0.5 * ((Z[:, None, :] - M[None, :, :]) ** 2).sum(axis=2) - np.log(pi)[None, :]
    p = np.exp(-(q - q.min(axis=1, keepdims=True)))
    p /= p.sum(axis=1, keepdims=True)
    return dict(prior=pi, means=mg, mu=mu, W=W, B=B, scaling=S, svd=np.sqrt(np.maximum(lam[:L], 0.0)), n_da=nda, ind_coord=Z,
                grp_coord=np.stack([Z[grp == g].mean(axis=0) for g in range(G)]), posterior=p,
                assign=np.argmin(q, axis=1).astype(np.int32))


def var_contr(V, loadings):
    """var_load = V loadings; var_contr = squares over the column's sum of squares, zeros where that is below 1e-12"""
    vl = np.asarray(V, dtype=np.float64) @ np.asarray(loadings, dtype=np.float64)
    ss = (vl * vl).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        vc = np.where(ss[None, :] < 1e-12, 0.0, vl * vl / ss[None, :])
    return dict(var_load=vl, var_contr=vc, colss=ss)


EPS = 2.0 ** -52  # eps = 2 u, as in "k-means on PCA scores"


def bound_var_contr(V, loadings):
    """The header's rounding bounds of the per-locus loadings, entry by entry -> (E_load, E_contr).
    var_load(i,a) is a sum of n_pca fused terms: E = (n_pca + 1) eps sum_j |V_ij| |l_ja|.  Its square is then off by at most
    q = 2 |vl| E + E^2; the column sum c of m such squares by Ec = sum_i q_i + (m + 2) eps c; and the quotient vl^2 / c by
    q / c + (vl^2 / c) (Ec / c) + 2 eps vl^2 / c (to first order in Ec / c, which is of the order of 1e-13 here)."""
    V, ld = np.asarray(V, dtype=np.float64), np.asarray(loadings, dtype=np.float64)
    m, n_pca = V.shape
    vl = V @ ld
    E = (n_pca + 1) * EPS * (np.abs(V) @ np.abs(ld))
    q = 2 * np.abs(vl) * E + E * E
    c = (vl * vl).sum(axis=0)
    Ec = q.sum(axis=0) + (m + 2) * EPS * c
    with np.errstate(divide="ignore", invalid="ignore"):
        Econtr = np.where(c[None, :] < 1e-12, 0.0, q / c + (vl * vl / c) * (Ec / c) + 2 * EPS * vl * vl / c)
    return E, Econtr


def dapc(pca, grp, n_pca, n_da=None):
    """gt_dapc on a pca dict with labels grp (any values; levels are the sorted distinct ones)"""
    u, d = np.asarray(pca["u"]), np.asarray(pca["d"])
    levels, g0 = np.unique(np.asarray(grp), return_inverse=True)
    tab = (u * d[None, :])[:, :n_pca]
    r = lda(tab, g0, n_da)
    nda = r["n_da"]
    out = {"n.pca": n_pca, "n.da": nda, "tab": tab, "grp": np.asarray(grp), "var": d[:n_pca].sum() / d.sum(), "eig": r["svd"] ** 2,
           "loadings": r["scaling"][:, :nda], "means": r["means"], "ind.coord": r["ind_coord"], "grp.coord": r["grp_coord"],
           "prior": r["prior"], "posterior": r["posterior"], "assign": levels[r["assign"]]}
    vc = var_contr(np.asarray(pca["v"])[:, :n_pca], out["loadings"])
    out["var.contr"], out["var.load"] = vc["var_contr"], vc["var_load"]
    return out
