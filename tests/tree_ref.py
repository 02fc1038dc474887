"""numpy restatement of include/tpg.h "Trees from a pairwise matrix" (it follows the header, not csrc/tree.hip): by brute force --
at every step the global minimum with the tie rule over the live upper triangle, no nearest-neighbour list, no per-row scan --
with every recurrence in the stated operation order in FP64; hclust's order, ape's edge table and the leaf-to-leaf path lengths of
a tree; and the inputs the host and the GPU tests share."""
import functools

import numpy as np

from tests import hclust_ref as hr

METHODS = ("single", "complete", "average", "mcquitty", "ward.D")


def lower_sym(D):
    """the pair values as the header reads them: the strict lower triangle of D mirrored, 0 on the diagonal (never used)"""
    D = np.asarray(D, dtype=np.float64)
    L = np.tril(D, -1)
    return L + L.T


def linkage(D, method):
    """-> dict(merge_a, merge_b (int32, 0-based slots), height (the S of the merged pair))"""
    S = lower_sym(D)
    n = S.shape[0]
    # U: S on the live upper triangle, +inf everywhere else, row-major: argmin returns the first minimum in the order (a, b)
    U = np.where(np.triu(np.ones((n, n), dtype=bool), 1), S, np.inf)
    live, size = np.ones(n, dtype=bool), np.ones(n)
    ma, mb, h = np.zeros(max(n - 1, 0), dtype=np.int32), np.zeros(max(n - 1, 0), dtype=np.int32), np.zeros(max(n - 1, 0))
    for s in range(n - 1):
        a, b = divmod(int(np.argmin(U)), n)
        if not (live[a] and live[b] and a < b):  # every live S is +inf (an overflow): the first live pair
            idx = np.nonzero(live)[0]
            a, b = int(idx[0]), int(idx[1])
        sab = U[a, b]
        ma[s], mb[s], h[s] = a, b, sab
        c = np.nonzero(live)[0]
        c = c[(c != a) & (c != b)]
        x, y = U[np.minimum(a, c), np.maximum(a, c)], U[np.minimum(b, c), np.maximum(b, c)]
        na, nb, nc = size[a], size[b], size[c]
        if method == "single":
            new = np.where(y < x, y, x)
        elif method == "complete":
            new = np.where(y > x, y, x)
        elif method == "average":
            p = na * x
            q = nb * y
            new = (p + q) / (na + nb)
        elif method == "mcquitty":
            new = (x + y) * 0.5
        elif method == "ward.D":
            p = (na + nc) * x
            q = (nb + nc) * y
            r = nc * sab
            new = ((p + q) - r) / ((na + nb) + nc)
        else:
            raise ValueError(method)
        U[np.minimum(a, c), np.maximum(a, c)] = new
        size[a] += size[b]
        live[b] = False
        U[b, :] = np.inf
        U[:, b] = np.inf
    return dict(merge_a=ma, merge_b=mb, height=h)


def order(n, merge_a, merge_b):
    """hclust$order, 0-based: the leaves of a row of R's merge matrix are those of its first column, then of its second"""
    if n == 1:
        return np.zeros(1, dtype=np.int32)
    leaves = {}
    for s, (u, v) in enumerate(hr.r_merge(n, merge_a, merge_b).tolist()):
        leaves[s + 1] = ([-u - 1] if u < 0 else leaves.pop(u)) + ([-v - 1] if v < 0 else leaves.pop(v))
    return np.array(leaves[n - 1], dtype=np.int32)


class NoPair(Exception):
    """a join found every criterion value NaN: the library's TPG_ENUMERIC"""


def nj(D):
    """-> dict(join_a, join_b (int32, 0-based slots), len_a, len_b, last).  The live slots are kept compact in ascending order,
    so the row-major first minimum over the upper triangle is the lexicographic minimum of (q, a, b)."""
    S = lower_sym(D)
    n = S.shape[0]
    R = np.zeros(n)
    with np.errstate(over="ignore"):
        for j in range(n):  # ascending j from +0, one addition per j; j = i is left out
            R = np.where(np.arange(n) == j, R, R + S[:, j])
    slots = np.arange(n)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    J = max(n - 2, 0)
    ja, jb, la, lb = np.zeros(J, dtype=np.int32), np.zeros(J, dtype=np.int32), np.zeros(J), np.zeros(J)
    for s in range(J):
        r = len(slots)
        with np.errstate(over="ignore", invalid="ignore"):
            q = (np.float64(r - 2) * S - R[:, None]) - R[None, :]
        ok = upper[:r, :r] & ~np.isnan(q)
        if not ok.any():
            raise NoPair()
        k = int(np.argmin(np.where(ok, q, np.inf)))  # (row-major: the first minimum in the order (a, b))
        if not ok.ravel()[k]:  # (every valid q is +inf and another entry comes first: the first valid one)
            k = int(np.argmax(ok))
        a, b = divmod(k, r)
        d = S[a, b]
        ja[s], jb[s] = slots[a], slots[b]
        la[s] = 0.5 * d + (R[a] - R[b]) / (2.0 * np.float64(r - 2))
        lb[s] = d - la[s]
        x, y = S[a].copy(), S[b].copy()
        with np.errstate(over="ignore", invalid="ignore"):
            t = ((x + y) - d) * 0.5
            Rn = ((R - x) - y) + t
            Rn[a] = ((R[a] + R[b]) - np.float64(r) * d) * 0.5
        t[a] = 0.0
        S[a, :] = t
        S[:, a] = t
        keep = np.arange(r) != b
        S, R, slots = S[np.ix_(keep, keep)], Rn[keep], slots[keep]
    last = np.array([slots[0], slots[1], S[0, 1]], dtype=np.float64) if n >= 2 else np.zeros(0)
    return dict(n=n, join_a=ja, join_b=jb, len_a=la, len_b=lb, last=last)


def nj_edges(tree):
    """ape's phylo layout -> dict(edge ((2n - 3) x 2), edge_length, Nnode): tips 1 .. n, the node of join s is 2n - 2 - s, the root
    n + 1 with its a-child, b-child and the other slot left; preorder, a-child before b-child before the third"""
    n = tree["n"]
    node = {i: i + 1 for i in range(n)}
    kids = {}
    for s in range(n - 2):
        a, b = int(tree["join_a"][s]), int(tree["join_b"][s])
        new = 2 * n - 2 - s
        kids[new] = [(node[a], float(tree["len_a"][s])), (node.pop(b), float(tree["len_b"][s]))]
        node[a] = new
    x, y = int(tree["last"][0]), int(tree["last"][1])
    assert sorted(node) == [x, y] and n + 1 in (node[x], node[y])
    kids[n + 1].append((node[y] if node[x] == n + 1 else node[x], float(tree["last"][2])))
    edge, length = [], []
    todo = [(n + 1, c, l) for c, l in reversed(kids[n + 1])]
    while todo:
        p, c, l = todo.pop()
        edge.append((p, c))
        length.append(l)
        todo += [(c, cc, ll) for cc, ll in reversed(kids.get(c, []))]
    return dict(edge=np.array(edge, dtype=np.int32), edge_length=np.array(length), Nnode=n - 2)


def path_lengths(tree):
    """the n x n leaf-to-leaf sums of the branch lengths along the tree of nj(); for n = 2 the one branch"""
    n = tree["n"]
    if n == 1:
        return np.zeros((1, 1))
    if n == 2:
        return np.array([[0.0, tree["last"][2]], [tree["last"][2], 0.0]])
    e = nj_edges(tree)
    N = 2 * n - 2
    P = np.zeros((N + 1, N + 1))
    seen = [n + 1]
    for (p, c), l in zip(e["edge"].tolist(), e["edge_length"].tolist()):  # preorder: the parent is in already
        P[c, seen] = P[p, seen] + l
        P[seen, c] = P[c, seen]
        seen.append(c)
    return P[1:n + 1, 1:n + 1].copy()


# ---- trees computed once per input and shared among the tests; the arrays are read-only

def _freeze(t):
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _linkage_cached(key, method):
    return _freeze(linkage(np.frombuffer(key[0], dtype=np.float64).reshape(key[1]), method))


@functools.lru_cache(maxsize=None)
def _nj_cached(key):
    return _freeze(nj(np.frombuffer(key[0], dtype=np.float64).reshape(key[1])))


def _key(D):
    D = np.ascontiguousarray(lower_sym(D))
    return D.tobytes(), D.shape


def linkage_shared(D, method):
    return _linkage_cached(_key(D), method)


def nj_shared(D):
    return _nj_cached(_key(D))


# ---- inputs

def euclid(X):
    """Euclidean distances of the rows of X, symmetric by construction"""
    return np.sqrt(hr.start_matrix(X, 1))


def manhattan(X):
    X = np.asarray(X, dtype=np.float64)
    return np.abs(X[:, None, :] - X[None, :, :]).sum(axis=2)


def blob_matrix(n, seed=None):
    """the tie-free Euclidean matrix of hclust_ref.blobs on n points in 3 dimensions"""
    return euclid(hr.blobs(n + 3 if seed is None else seed, n, 3))


def tie_matrices():
    L = hr.lattice()
    return {"lattice_euclid": euclid(L), "lattice_manhattan": manhattan(L), "zeros": np.zeros((40, 40)), "axis_star": euclid(hr.axis_star())}


def additive_tree(n, seed):
    """the leaf-to-leaf path lengths of a random binary tree on n >= 2 leaves: sequential attachment (every new leaf hangs a new
    inner node into a random edge), branch lengths k / 64 with k in 1 .. 640 -- every sum of them is exact -- and the leaves
    shuffled"""
    rng = np.random.default_rng(seed)
    edges = [(0, 1)]  # leaves are 0 .. n - 1, inner nodes follow
    nxt = n
    for leaf in range(2, n):
        u, v = edges.pop(int(rng.integers(len(edges))))
        edges += [(u, nxt), (nxt, v), (nxt, leaf)]
        nxt += 1
    N = nxt
    adj = [[] for _ in range(N)]
    for u, v in edges:
        l = int(rng.integers(1, 641)) / 64.0
        adj[u].append((v, l))
        adj[v].append((u, l))
    D = np.zeros((n, n))
    for src in range(n):
        dist = np.full(N, -1.0)
        dist[src] = 0.0
        todo = [src]
        while todo:
            u = todo.pop()
            for v, l in adj[u]:
                if dist[v] < 0:
                    dist[v] = dist[u] + l
                    todo.append(v)
        D[src] = dist[:n]
    perm = rng.permutation(n)
    return np.ascontiguousarray(D[np.ix_(perm, perm)])
