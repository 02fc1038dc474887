"""numpy restatement of LD clumping (include/tpg.h "LD clumping"): dense, no tiling, int64 sums, the link comparison in
np.float64 in the stated order, a sequential greedy loop, the window from chromosome / position / size -- and a small
generator of panels with LD (the oracle's synthetic panel has independent loci and links almost nothing)."""
import numpy as np

MAX_ROUNDS = 32  # TPG_LD_MAX_ROUNDS of csrc/ld.hip: the parallel rounds before the walk in priority order


def ld_panel(seed: int, n: int, m: int, rho: float) -> np.ndarray:
    """n x m genotypes 0 / 1 / 2: a haplotype at locus j copies locus j - 1 with probability rho, otherwise it is drawn at
    the locus's own frequency; a genotype is the sum of two haplotypes"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, size=m)
    hap = np.empty((2 * n, m), dtype=np.uint8)
    hap[:, 0] = rng.random(2 * n) < p[0]
    for j in range(1, m):
        own = (rng.random(2 * n) < p[j]).astype(np.uint8)
        copy = rng.random(2 * n) < rho
        hap[:, j] = np.where(copy, hap[:, j - 1], own)
    return np.asfortranarray(hap[:n] + hap[n:])


def window_hi(chromosome, position=None, size=500.0, use_positions=True) -> np.ndarray:
    """hi[j] = last neighbour of j (0-based): same chromosome and |position difference| <= size * 1000, or without
    positions |index difference| <= size"""
    chrom = np.asarray(chromosome)
    m = len(chrom)
    hi = np.empty(m, dtype=np.int64)
    for c in np.unique(chrom):
        idx = np.flatnonzero(chrom == c)
        assert np.array_equal(idx, np.arange(idx[0], idx[-1] + 1)), "loci are not ordered"
        if use_positions:
            p = np.asarray(position, dtype=np.float64)[idx]
            assert np.all(p[1:] >= p[:-1]), "loci are not ordered"
            hi[idx] = idx[0] + np.searchsorted(p, p + float(size) * 1000.0, side="right") - 1
        else:
            hi[idx] = np.minimum(idx + int(np.floor(size)), idx[-1])
    return hi


def sums(G):
    """n, Sx, d = n Sxx - Sx^2 per locus, int64 (in blocks of loci: a large panel is not widened as a whole)"""
    G = np.asarray(G)
    n, m = G.shape
    sx, sxx = np.empty(m, dtype=np.int64), np.empty(m, dtype=np.int64)
    step = max(1, min(4096, (1 << 26) // max(n, 1)))
    for a in range(0, m, step):
        x = G[:, a:a + step].astype(np.int64)
        assert x.min(initial=0) >= 0 and x.max(initial=0) <= 2, "a missing genotype"
        sx[a:a + step], sxx[a:a + step] = x.sum(axis=0), (x * x).sum(axis=0)
    return n, sx, n * sxx - sx * sx


def link_rows(G, hi, thr_r2, rows=None):
    """{j: boolean array over k = j + 1 .. hi[j]} of the linked neighbours, for every row (or the rows given)"""
    G = np.asarray(G)
    n, sx, d = sums(G)
    thr = np.float64(thr_r2)
    out = {}
    for j in (range(G.shape[1]) if rows is None else rows):
        ks = np.arange(j + 1, int(hi[j]) + 1)
        sxy = G[:, j].astype(np.int64) @ G[:, j + 1:int(hi[j]) + 1].astype(np.int64) if len(ks) else np.zeros(0, dtype=np.int64)
        num = (n * sxy - sx[j] * sx[ks]).astype(np.float64)
        den = np.float64(d[j]) * d[ks].astype(np.float64)
        out[j] = num * num > thr * den
    return out


def band_bits(G, hi, thr_r2, stride=None, rows=None) -> np.ndarray:
    """the bit band of tpg_ld_band_links: (m, stride) uint32, bit b of row j <-> locus j + 1 + b"""
    m = np.asarray(G).shape[1]
    width = int((np.asarray(hi) - np.arange(m)).max(initial=0))
    if stride is None:
        stride = max(1, -(-width // 32))
    bits = np.zeros((m, stride), dtype=np.uint32)
    for j, lk in link_rows(G, hi, thr_r2, rows).items():
        for b in np.flatnonzero(lk):
            bits[j, b >> 5] |= np.uint32(1) << np.uint32(b & 31)
    return bits


def bits_to_adjacency(bits):
    """band -> list of linked neighbours (both directions) per locus"""
    m = bits.shape[0]
    adj = [[] for _ in range(m)]
    for j in range(m):
        for w in np.flatnonzero(bits[j]):
            word = int(bits[j, w])
            while word:
                b = (word & -word).bit_length() - 1
                word &= word - 1
                k = j + 1 + 32 * int(w) + b
                adj[j].append(k)
                adj[k].append(j)
    return adj


def priority_key(G, S=None):
    if S is not None:
        s = np.asarray(S, dtype=np.float64)
        assert not np.isnan(s).any()
        return s + 0.0  # -0.0 -> 0.0
    n, sx, _ = sums(G)
    return np.minimum(sx, 2 * n - sx)


def order_of(key):
    """R's order(key, decreasing = TRUE): stable, ties to the smaller index"""
    return np.argsort(-np.asarray(key, dtype=np.float64) if np.asarray(key).dtype.kind == "f" else -np.asarray(key), kind="stable")


def greedy(adj, key, exclude=None):
    """the sequential greedy keep set"""
    m = len(adj)
    standing = np.ones(m, dtype=bool)
    if exclude is not None:
        standing[np.asarray(exclude, dtype=bool)] = False
    keep = np.zeros(m, dtype=bool)
    for j in order_of(key):
        if standing[j]:
            keep[j] = True
            standing[j] = False
            for k in adj[j]:
                standing[k] = False
    return keep


def fixed_point_holds(adj, key, keep, exclude=None):
    """a non-excluded locus is kept iff no linked locus of higher priority is kept"""
    m = len(adj)
    rank = np.empty(m, dtype=np.int64)
    rank[order_of(key)] = np.arange(m)
    ex = np.zeros(m, dtype=bool) if exclude is None else np.asarray(exclude, dtype=bool)
    for j in range(m):
        blocked = any(keep[k] and rank[k] < rank[j] for k in adj[j])
        if keep[j] != ((not ex[j]) and not blocked):
            return False
    return True


def parallel_rounds(adj, key, exclude=None, max_rounds=None):
    """the Jacobi rounds of the device route: (keep so far, rounds run, loci left undecided)"""
    m = len(adj)
    rank = np.empty(m, dtype=np.int64)
    rank[order_of(key)] = np.arange(m)
    state = np.zeros(m, dtype=np.int8)  # 0 undecided, 1 kept, 2 fallen
    if exclude is not None:
        state[np.asarray(exclude, dtype=bool)] = 2
    higher = [[k for k in adj[j] if rank[k] < rank[j]] for j in range(m)]
    rounds = 0
    left = m
    while left > 0 and (max_rounds is None or rounds < max_rounds):
        new = state.copy()
        for j in np.flatnonzero(state == 0):
            s = state[higher[j]]
            if (s == 1).any():
                new[j] = 2
            elif (s == 2).all():
                new[j] = 1
        state = new
        rounds += 1
        left = int((state == 0).sum())
    return state == 1, rounds, left


def clump(G, hi, thr_r2, S=None, exclude=None):
    """keep set, number of links"""
    bits = band_bits(G, hi, thr_r2)
    adj = bits_to_adjacency(bits)
    return greedy(adj, priority_key(G, S), exclude), sum(len(a) for a in adj) // 2
