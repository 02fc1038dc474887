"""Tajima's D restated in numpy from the reference's text (R/pop_tajimas_d.R:151-166, src/gt_pi_diploid.cpp:22-35,
src/gt_grouped_pi_diploid.cpp:24-38, R/windows_stats_generic.R:113-176, R/windows_pop_tajimas_d.R:69-102); include/tpg.h
"Tajima's D" is the definition both follow.  Two routes: a float route (pi in the stated order, sum, D in double) and an
exact route in integers and fractions.Fraction for seg, k_hat and the numerator k_hat - seg / a1, so that truth does not rest
on a summation order.  And a small panel generator with the awkward columns planted."""
from fractions import Fraction

import numpy as np

MISSING = 3


# ---- float route ----------------------------------------------------------------------------------------------------------
def group_counts(codes, gid, G):
    """codes: n x m uint8 (0, 1, 2, 3 = missing) -> x, v (m x G int64): alternate alleles and twice the typed individuals"""
    codes = np.asarray(codes)
    gid = np.zeros(codes.shape[0], dtype=np.int64) if gid is None else np.asarray(gid)
    x = np.zeros((codes.shape[1], G), dtype=np.int64)
    v = np.zeros((codes.shape[1], G), dtype=np.int64)
    typed = codes != MISSING
    dos = np.where(typed, codes, 0).astype(np.int64)
    for g in range(G):
        rows = gid == g
        x[:, g] = dos[rows].sum(axis=0)
        v[:, g] = 2 * typed[rows].sum(axis=0)
    return x, v


def group_sizes(n, gid, G):
    return np.array([n]) if gid is None else np.bincount(np.asarray(gid), minlength=G)


def pi_float(x, v):
    """pi = x (v - x) / (v (v - 1) / 2) in this order in double; v = 0 gives NaN"""
    xf, vf = x.astype(np.float64), v.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return xf * (vf - xf) / (vf * (vf - 1) / 2)


def consts(n):
    """a1, a2, e1, e2 of n >= 2 sampled alleles in double, a1 and a2 summed in ascending order of i (cumsum adds one term
    after the other)"""
    i = np.arange(1, n, dtype=np.float64)
    a1, a2 = float(np.cumsum(1.0 / i)[-1]), float(np.cumsum(1.0 / (i * i))[-1])
    n = float(n)
    e1 = ((n + 1) / (3 * (n - 1)) - 1 / a1) / a1
    e2_num = 2 * (n * n + n + 3) / (9 * n * (n - 1)) - (n + 2) / (n * a1) + a2 / (a1 * a1)
    return a1, a2, e1, e2_num / (a1 * a1 + a2)


def var_d(n, seg):
    _, _, e1, e2 = consts(n)
    s = np.asarray(seg, dtype=np.float64)
    return e1 * s + e2 * s * (s - 1)


def d_from_sums(n, seg, k_hat):
    """D of n sampled alleles from seg and k_hat (arrays broadcast); n = 0: NaN"""
    s = np.asarray(seg, dtype=np.float64)
    k = np.asarray(k_hat, dtype=np.float64)
    if n < 2:
        return np.full(np.broadcast(s, k).shape, np.nan)
    a1 = consts(n)[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (k - s / a1) / np.sqrt(var_d(n, s))


def sums_float(pi):
    """pi: L x G -> seg (int64[G]), k_hat (the plain sum: a NaN propagates), n_loci (non-NaN entries)"""
    with np.errstate(invalid="ignore"):
        seg = ((pi > 0.0) & (pi < 1.0)).sum(axis=0).astype(np.int64)
    return seg, pi.sum(axis=0), (~np.isnan(pi)).sum(axis=0).astype(np.int64)


def pop_ref(codes, gid, G):
    """whole view -> dict(tajimas_d, seg, k_hat), G entries each; a group nobody belongs to: NaN, seg 0"""
    x, v = group_counts(codes, gid, G)
    size = group_sizes(codes.shape[0], gid, G)
    seg, k, _ = sums_float(pi_float(x, v))
    k = np.where(size > 0, k, np.nan)
    d = np.array([d_from_sums(2 * int(size[g]), seg[g], k[g]) for g in range(G)], dtype=np.float64)
    return dict(tajimas_d=d, seg=seg, k_hat=k)


def windows_ref(codes, gid, G, lo, hi, pad_na=None, min_loci=1):
    """-> dict(tajimas_d, seg, k_hat, n_loci), nw x G each; n_loci -1, seg 0 and k_hat NaN on a pad window; D NaN where the
    window is padded or holds fewer than min_loci non-NaN pi"""
    x, v = group_counts(codes, gid, G)
    size = group_sizes(codes.shape[0], gid, G)
    pi = pi_float(x, v)
    nw = len(lo)
    seg = np.zeros((nw, G), dtype=np.int64)
    k = np.full((nw, G), np.nan)
    nl = np.full((nw, G), -1, dtype=np.int64)
    for w in range(nw):
        if pad_na is not None and pad_na[w]:
            continue
        seg[w], k[w], nl[w] = sums_float(pi[lo[w]:hi[w]])
    k[:, size == 0] = np.nan
    d = np.stack([d_from_sums(2 * int(size[g]), seg[:, g], k[:, g]) for g in range(G)], axis=1).reshape(nw, G)
    d[nl < min_loci] = np.nan
    return dict(tajimas_d=d, seg=seg, k_hat=k, n_loci=nl)


# ---- exact route ----------------------------------------------------------------------------------------------------------
def a1_exact(n):
    return sum((Fraction(1, i) for i in range(1, n)), Fraction(0))


def sums_exact(x, v):
    """x, v: integer vectors of one group over a set of loci -> (seg, k_hat as a Fraction, or None where some v is 0)"""
    x, v = np.asarray(x, dtype=np.int64), np.asarray(v, dtype=np.int64)
    num, den = 2 * x * (v - x), v * (v - 1)  # pi = num / den
    seg = int(((num > 0) & (num < den)).sum())
    if (v == 0).any():
        return seg, None
    k = Fraction(0)
    for vv in np.unique(v):  # few distinct denominators: integer sums per denominator
        k += Fraction(int(num[v == vv].sum()), int(vv) * (int(vv) - 1))
    return seg, k


def numerator_exact(n, seg, k_hat):
    """k_hat - seg / a1 as a Fraction (n >= 2)"""
    return k_hat - Fraction(seg) / a1_exact(n)


# ---- panels ---------------------------------------------------------------------------------------------------------------
def panel(seed, n, m, G):
    """n x m codes and the group of every individual (None for G = 1).  Planted, where the shape has room: a group of one
    individual (n = 2: vd = 0), groups nobody belongs to (G > n: all but max(2, n // 3)), a locus at which group 0 is entirely
    missing (m // 3), a locus at which the only typed individual of the last non-empty group is heterozygous (m // 2: pi = 1),
    a monomorphic stretch (from m // 4, up to 70 loci: S = 0), and missingness around 10 % everywhere."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, size=m)
    codes = rng.binomial(2, p[None, :], size=(n, m)).astype(np.uint8)
    if G == 1:
        gid, last = None, 0
    else:
        k = G if G <= n else max(2, n // 3)  # G > n: the groups k .. G - 1 have no member
        gid = (np.arange(n) % k).astype(np.int32)
        gid[np.where(gid == k - 1)[0][1:]] = 0  # the last group with a member is a group of one
        last = k - 1

    def members(g):
        return np.arange(n) if gid is None else np.where(gid == g)[0]

    a, b = m // 4, min(m, m // 4 + 70)
    codes[:, a:b] = 0                                   # monomorphic stretch
    codes[rng.random((n, m)) < 0.10] = MISSING          # ordinary missingness
    if m > 2:
        codes[members(0), m // 3] = MISSING             # group 0 entirely missing at one locus
        rows = members(last)
        codes[rows, m // 2] = MISSING                   # one typed individual, heterozygous
        codes[rows[0], m // 2] = 1
    return codes, gid


def max_ulp(a, b):
    """largest distance in units of the last place between two double arrays, over the entries that are finite in both (the
    others must agree in kind: NaN with NaN, +Inf with +Inf)"""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))
    f = np.isfinite(a)
    assert np.array_equal(a[~f & ~np.isnan(a)], b[~f & ~np.isnan(b)])
    if not f.any():
        return 0.0
    return float(np.max(np.abs(a[f] - b[f]) / np.spacing(np.maximum(np.abs(a[f]), np.abs(b[f])))))
