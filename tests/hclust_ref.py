"""numpy restatement of include/tpg.h "Ward clustering on PCA scores" (it follows the header, not csrc/hclust.hip): by brute
force -- at every step the global minimum with the tie rule over the live upper triangle, no nearest-neighbour list -- with the
recurrence in the stated operation order in FP64, the cut, R's merge matrix, the WSS of a labelling through tests/kmeans_ref.py,
and the host side of gt_cluster_pca_ward restated independently of tidypopgen_amd/api.py."""
import functools

import numpy as np

from tests import kmeans_ref as kr


# ---- a correctly rounded fused multiply-add on arrays (Python 3.10 has no math.fma): Boldo and Melquiond, "Emulation of a FMA and
# correctly rounded sums: proved algorithms using rounding to odd" (IEEE TC 2008).  a b = ph + pl exactly (Dekker's product),
# c + ph = th + tl exactly (Knuth's sum), and fma = RN(th + RO(tl + pl)) with RO rounding to odd.  Holds where nothing overflows
# or underflows, which the test inputs stay far from; tests/test_hclust_host.py checks it against rationals.

def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a  # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    ph, pl = _two_prod(a, b)
    th, tl = _two_sum(c, ph)
    v, w = _two_sum(tl, pl)
    even = (np.ascontiguousarray(v).view(np.int64) & 1) == 0
    v = np.where((w != 0) & even, np.nextafter(v, np.where(w > 0, np.inf, -np.inf)), v)  # to odd: the inexact even one moves on
    return th + v


def start_matrix(X, power):
    """S(i, j): D2 from +0, coordinates ascending, t = x_i - x_j, D2 = fma(t, t, D2); squared once more for power 2"""
    X = np.asarray(X, dtype=np.float64)
    D = np.zeros((X.shape[0], X.shape[0]))
    for j in range(X.shape[1]):
        t = X[:, j, None] - X[None, :, j]
        D = fma(t, t, D)
    return D if power == 1 else D * D


def ward(X, power=2):
    """-> dict(merge_a, merge_b (int32, 0-based slots), height (the S of the merged pair))"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    # U: S on the live upper triangle, +inf everywhere else, row-major: argmin returns the first minimum in the order (a, b),
    # which is the tie rule
    U = np.where(np.triu(np.ones((n, n), dtype=bool), 1), start_matrix(X, power), np.inf)
    live, size = np.ones(n, dtype=bool), np.ones(n)
    ma, mb, h = np.zeros(n - 1, dtype=np.int32), np.zeros(n - 1, dtype=np.int32), np.zeros(n - 1)
    for s in range(n - 1):
        flat = int(np.argmin(U))
        a, b = divmod(flat, n)
        if not (live[a] and live[b] and a < b):  # every live S is +inf (an overflow): the first live pair
            idx = np.nonzero(live)[0]
            a, b = int(idx[0]), int(idx[1])
        sab = U[a, b]
        ma[s], mb[s], h[s] = a, b, sab
        c = np.nonzero(live)[0]
        c = c[(c != a) & (c != b)]
        nc = size[c]
        p = (size[a] + nc) * U[np.minimum(a, c), np.maximum(a, c)]
        q = (size[b] + nc) * U[np.minimum(b, c), np.maximum(b, c)]
        r = nc * sab
        U[np.minimum(a, c), np.maximum(a, c)] = ((p + q) - r) / ((size[a] + size[b]) + nc)
        size[a] += size[b]
        live[b] = False
        U[b, :] = np.inf
        U[:, b] = np.inf
    return dict(merge_a=ma, merge_b=mb, height=h)


@functools.lru_cache(maxsize=None)
def _ward_cached(key, power):
    X = np.frombuffer(key[0], dtype=np.float64).reshape(key[1])
    t = ward(X, power)
    for v in t.values():
        v.setflags(write=False)
    return t


def ward_shared(X, power=2):
    """ward() computed once per (X, power) and shared among the tests; the arrays are read-only"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    return _ward_cached((X.tobytes(), X.shape), power)


def cut(n, merge_a, merge_b, k):
    """the first n - k merges, then 0, 1, .. in the order in which the clusters first appear in ascending i -> labels (int32)"""
    member = {i: [i] for i in range(n)}
    for s in range(n - k):
        member[int(merge_a[s])] += member.pop(int(merge_b[s]))
    lab = np.zeros(n, dtype=np.int32)
    for num, slot in enumerate(sorted(member, key=lambda c: min(member[c]))):
        lab[member[slot]] = num
    return lab


def r_merge(n, merge_a, merge_b):
    """hclust$merge: negative singletons, positive step numbers, a singleton before a cluster, the smaller of two within a row"""
    ident = {i: -(i + 1) for i in range(n)}
    out = np.zeros((n - 1, 2), dtype=np.int32)
    for s in range(n - 1):
        u, v = ident[int(merge_a[s])], ident[int(merge_b[s])]
        # two singletons: the smaller point, which is the larger of two negative numbers; otherwise the smaller number
        out[s] = (max(u, v), min(u, v)) if u < 0 and v < 0 else (min(u, v), max(u, v))
        ident[int(merge_a[s])] = s + 1
    return out


def wss_of_labels(X, labels, k):
    """the WSS of a labelling: centres by the Update rule, e_i and the sum as kmeans_ref has them"""
    X = np.asarray(X, dtype=np.float64)
    C, _ = kr.update(X, np.asarray(labels), np.zeros((k, X.shape[1])))
    return kr.wss_of(X, C, np.asarray(labels))


def cluster_pca_ward(scores, ks, power=2):
    """-> dict(k, WSS, AIC, BIC, groups {k: 1-based}, merge, height (the root, as hclust reports it))"""
    scores = np.asarray(scores, dtype=np.float64)
    n = scores.shape[0]
    t = ward_shared(scores, power)
    groups = {k: cut(n, t["merge_a"], t["merge_b"], k) + 1 for k in ks}
    w = np.array([wss_of_labels(scores, groups[k] - 1, k) for k in ks])
    kv = np.array(list(ks), dtype=np.float64)
    return dict(k=list(ks), WSS=w, AIC=n * np.log(w / n) + 2 * kv, BIC=n * np.log(w / n) + np.log(n) * kv, groups=groups,
                merge=r_merge(n, t["merge_a"], t["merge_b"]), height=np.sqrt(t["height"]))


# ---- the inputs the host and the GPU tests share

def blobs(seed, n, d, g=5, sep=6.0):
    """five Gaussian blobs, seeded: no two distances equal"""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.normal(size=(g, d))[np.arange(n) % g] * sep + rng.normal(size=(n, d)))


def lattice():
    """an 8 x 8 integer lattice plus 5 duplicated points: 69 points, zero distances, many equal ones"""
    g = np.array([(x, y) for x in range(8) for y in range(8)], dtype=np.float64)
    return np.asfortranarray(np.concatenate([g, g[[0, 9, 27, 27, 63]]]))


def collinear(n=100):
    return np.asfortranarray(np.arange(n, dtype=np.float64)[:, None])


def copies(n=40):
    return np.asfortranarray(np.tile(np.array([[1.5, -2.0, 0.25]]), (n, 1)))


def star(m=200, d=3, seed=3, centre_last=False):
    """one point at the origin and m points on a sphere around it at slightly different radii.  The nearest-neighbour list of
    the header's relation to the device looks at j > i only, so the rows share the centre as their neighbour when it comes last
    and lies nearer than the other points, which needs room: d = 64 puts random directions nearly at right angles"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(m, d))
    v /= np.linalg.norm(v, axis=1)[:, None]
    pts, zero = v * (1.0 + 1e-3 * np.arange(m))[:, None], np.zeros((1, d))
    return np.asfortranarray(np.concatenate([pts, zero] if centre_last else [zero, pts]))


def axis_star(d=64):
    """a star that is one by construction: the 2 d points +-r e_k on the axes, every radius r = 1 + i / 1000 its own, and the
    origin LAST.  Two of them lie at r_i^2 + r_j^2 (different axes) or (r_i + r_j)^2 (one axis) from each other, both above the
    r_i^2 to the origin, so the origin is the nearest neighbour of every row"""
    X = np.zeros((2 * d + 1, d))
    for i in range(2 * d):
        X[i, i // 2] = (1.0 + i / 1000.0) * (1 if i % 2 == 0 else -1)
    return np.asfortranarray(X)
