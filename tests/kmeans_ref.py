"""numpy restatement of include/tpg.h "k-means on PCA scores" (it follows the header, not csrc/kmeans.hip): the seeded start
rows, Lloyd's assign / update / stop, the WSS in the header's order, the rounding bounds as the header derives them, an exact
route in rationals for one step, and the host side of gt_cluster_pca and gt_cluster_pca_best_k restated independently of
tidypopgen_amd/api.py."""
from fractions import Fraction

import numpy as np

MASK = (1 << 64) - 1
TILE = 256       # TPG_KMEANS_TILE
EPS = 2.0 ** -52  # eps = 2 u of the header's bounds


def mix64_int(x):
    """tpg_mix64 (csrc/synth_common.h) on a Python int"""
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def mix64(x):
    """the same on uint64 arrays (wraps modulo 2^64)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def start(seed, n, k):
    """Start: the k rows with the smallest (h_i, i), h_i = M(seed ^ M(i)), in that order"""
    h = mix64(np.uint64(seed & MASK) ^ mix64(np.arange(n, dtype=np.uint64)))
    return np.lexsort((np.arange(n), h))[:k].astype(np.int32)


def run_seed(seed, k, t):
    """the seed of start t at k clusters in gt_cluster_pca"""
    return mix64_int((seed & MASK) ^ mix64_int(((k << 32) + t) & MASK))


def dist(X, C):
    """D(i, c) in the direct form, j ascending from +0 (the device fuses the square into the sum; the bounds cover both)"""
    D = np.zeros((X.shape[0], C.shape[0]))
    for j in range(X.shape[1]):
        t = X[:, j, None] - C[None, :, j]
        D = D + t * t
    return D


def tile_sum(e):
    """WSS: pad to a multiple of TILE with +0, halve every tile, add the tile sums in ascending order"""
    e = np.asarray(e, dtype=np.float64)
    tiles = -(-len(e) // TILE)
    a = np.zeros(tiles * TILE)
    a[:len(e)] = e
    a = a.reshape(tiles, TILE).copy()
    s = TILE // 2
    while s >= 1:
        a[:, :s] = a[:, :s] + a[:, s:2 * s]
        s //= 2
    tot = 0.0
    for t in range(tiles):
        tot = tot + a[t, 0]
    return float(tot)


def assign(X, C):
    """-> labels (the smaller index wins a tie: argmin returns the first), the n x k distances"""
    D = dist(X, C)
    return np.argmin(D, axis=1).astype(np.int32), D


def update(X, labels, C):
    """means in ascending point order (cumsum adds one after the other); a centre that owns nothing stays -> centres, counts"""
    Cn = np.array(C, dtype=np.float64, copy=True)
    counts = np.bincount(labels, minlength=C.shape[0]).astype(np.int32)
    for c in range(C.shape[0]):
        if counts[c]:
            Cn[c] = np.cumsum(X[labels == c], axis=0)[-1] / float(counts[c])
    return Cn, counts


def step(X, C):
    """tpg_kmeans_step: wss is the value under C and the new labels"""
    labels, D = assign(X, C)
    Cn, counts = update(X, labels, C)
    return dict(labels=labels, centers=Cn, counts=counts, wss=tile_sum(D[np.arange(len(labels)), labels]))


def wss_of(X, C, labels):
    return tile_sum(dist(X, C)[np.arange(len(labels)), labels])


def rel_gap(D):
    """the smallest relative gap over the points between the best and the second-best distance (inf with one centre)"""
    if D.shape[1] < 2:
        return np.inf
    two = np.partition(D, 1, axis=1)[:, :2]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = (two[:, 1] - two[:, 0]) / two[:, 1]
    return float(np.min(np.where(two[:, 1] > 0, g, 0.0)))


def run(X, k, seed=None, centers0=None, max_iter=100000, trace=False):
    """a whole run -> dict(labels, centers, wss, n_iter, converged, n_empty, min_gap (over every assign), start[, wss_trace: the
    WSS under the centres each assign used])"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    idx = None
    if centers0 is None:
        idx = start(seed, n, k)
        C = X[idx].copy()
    else:
        C = np.array(centers0, dtype=np.float64, copy=True)
    labels = np.full(n, -1, dtype=np.int32)
    it, converged, gap, tr = 0, False, np.inf, []
    while it < max_iter:
        it += 1
        new, D = assign(X, C)
        gap = min(gap, rel_gap(D))
        if trace:
            tr.append(tile_sum(D[np.arange(n), new]))
        if np.array_equal(new, labels):
            converged = True
            break
        labels = new
        C, _ = update(X, labels, C)
    counts = np.bincount(labels, minlength=k)
    out = dict(labels=labels, centers=C, wss=wss_of(X, C, labels), n_iter=it, converged=converged, n_empty=int((counts == 0).sum()),
               min_gap=gap, start=idx)
    if trace:
        out["wss_trace"] = tr
    return out


# ---- the exact route for one step: rationals throughout (inputs are doubles, so every Fraction is exact)

def step_exact(X, C):
    """-> labels, counts, centres (Fractions, None where the centre owns nothing), wss (a Fraction) under C.  Integer-valued
    inputs go through Python integers (as exact, and much faster) for the distances"""
    n, d = X.shape
    k = C.shape[0]
    whole = bool(np.all(X == np.rint(X)) and np.all(C == np.rint(C)))
    conv = (lambda v: int(v)) if whole else (lambda v: Fraction(float(v)))
    XF = [[conv(v) for v in row] for row in X]
    CF = [[conv(v) for v in row] for row in C]
    labels, wss = [], Fraction(0)
    for i in range(n):
        best, bl = None, 0
        for c in range(k):
            s = sum((XF[i][j] - CF[c][j]) ** 2 for j in range(d))
            if best is None or s < best:
                best, bl = s, c
        labels.append(bl)
        wss += best
    counts = [labels.count(c) for c in range(k)]
    cen = [[Fraction(sum(XF[i][j] for i in range(n) if labels[i] == c)) / counts[c] for j in range(d)] if counts[c] else None
           for c in range(k)]
    return np.array(labels, dtype=np.int32), np.array(counts, dtype=np.int32), cen, wss


# ---- the header's rounding bounds, as derived there

def bound_dist(d, D):
    return (d + 2) * EPS * D


def bound_centre(n, A):
    return n * EPS * A


def bound_wss(n, d, A, wss):
    bc = bound_centre(n, A)
    return (n + d + 2) * EPS * wss + n * d * (4 * A + bc) * bc


# ---- gt_cluster_pca and gt_cluster_pca_best_k on the host, restated

def cluster_pca(scores, ks, n_start=10, seed=0, max_iter=100000):
    """-> dict(k, WSS, AIC, BIC, groups {k: 1-based}, winner {k: t}, runs {(k, t): run})"""
    scores = np.asarray(scores, dtype=np.float64)
    n = scores.shape[0]
    out = dict(k=list(ks), WSS=[], groups={}, winner={}, runs={})
    for k in ks:
        best = None
        for t in range(1 if k == 1 else n_start):
            r = run(scores, k, seed=run_seed(seed, k, t), max_iter=max_iter)
            out["runs"][(k, t)] = r
            if best is None or r["wss"] < out["runs"][(k, best)]["wss"]:
                best = t
        out["winner"][k] = best
        out["WSS"].append(out["runs"][(k, best)]["wss"])
        out["groups"][k] = out["runs"][(k, best)]["labels"] + 1
    w, kv = np.array(out["WSS"]), np.array(ks, dtype=np.float64)
    out["WSS"], out["AIC"], out["BIC"] = w, n * np.log(w / n) + 2 * kv, n * np.log(w / n) + np.log(n) * kv
    return out


def ward_d_two_groups(x):
    """hclust(dist(x), "ward.D") cut in two, written on clusters kept as a dict: the pair of smallest dissimilarity merges (the
    first such pair in the order of the cluster ids, which are the smallest member), then Lance-Williams for Ward"""
    x = [float(v) for v in x]
    cl = {i: [i] for i in range(len(x))}
    dis = {(i, j): abs(x[i] - x[j]) for i in range(len(x)) for j in range(i + 1, len(x))}
    while len(cl) > 2:
        ids = sorted(cl)
        pair = min(((a, b) for ia, a in enumerate(ids) for b in ids[ia + 1:]), key=lambda p: (dis[p], p))
        a, b = pair
        na, nb = len(cl[a]), len(cl[b])
        for c in ids:
            if c in (a, b):
                continue
            nc = len(cl[c])
            dac, dbc = dis[(min(a, c), max(a, c))], dis[(min(b, c), max(b, c))]
            dis[(min(a, c), max(a, c))] = ((na + nc) * dac + (nb + nc) * dbc - nc * dis[(a, b)]) / (na + nb + nc)
        cl[a] = cl[a] + cl[b]
        del cl[b]
    out = np.zeros(len(x), dtype=np.int64)
    for num, cid in enumerate(sorted(cl, key=lambda c: min(cl[c])), start=1):
        out[cl[cid]] = num
    return out


def best_k(series, criterion):
    """R/gt_cluster_pca_best_k.R:124-152 on a plain series -> the 1-based position R returns; ValueError where R has none"""
    s = np.asarray(series, dtype=np.float64)

    def rise(v):
        w = [i for i in range(len(v) - 1) if v[i + 1] - v[i] > 0]
        if not w:
            raise ValueError("never goes up")
        return w[0] + 1

    if criterion == "min":
        return int(np.argmin(s)) + 1
    if criterion == "goesup":
        return rise(s)
    if criterion == "goodfit":
        thr = s.min() + 0.1 * (s.max() - s.min())
        w = [i for i in range(len(s)) if s[i] < thr]
        if not w:
            raise ValueError("constant")
        return w[0] + 1 - 1
    if criterion == "diffNgroup":
        df = np.diff(s)
        g = ward_d_two_groups(df)
        m1, m2 = df[g == 1].mean(), df[g == 2].mean()
        good = 1 if m1 <= m2 else 2
        return max(i for i in range(len(df)) if g[i] == good) + 1 + 1
    if criterion == "smoothNgoesup":
        t = s.copy()
        for i in range(len(s) - 2):
            t[i + 1] = (s[i] + s[i + 1] + s[i + 2]) / 3.0
        return rise(t)
    raise ValueError(criterion)
