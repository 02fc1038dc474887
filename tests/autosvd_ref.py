"""numpy + stdlib restatement of include/tpg.h "autoSVD": the upper normal quantile by bisection, the Gaussian weights and the
rolling mean as plain loops, type-7 quartiles, the medcouple three ways (brute force over all ratios, the classical
(a - b) / (a + b) kernel with the sign rule at the median, a vectorised bisection over the bit pattern for large counts), the
fence, the finder of outlier runs, a panel with a planted inversion-like block, and the whole loop on top of tests/ld_ref.py
and tests/pcadapt_ref.py."""
import math
import statistics

import numpy as np

from tests import ld_ref as lr
from tests import pcadapt_ref as pr

BITS_ONE, BITS_INF = 0x3FF0000000000000, 0x7FF0000000000000


# ---- normal quantile, weights, rolling mean ---------------------------------------------------------------------------------
def pnorm_upper(x):
    return 0.5 * math.erfc(x / 1.4142135623730951)


def qnorm_upper(p):
    """the root of pnorm_upper(x) = p by bisection on [-40, 40] until the ends are neighbouring doubles; the upper end"""
    lo, hi = -40.0, 40.0
    while True:
        mid = lo + (hi - lo) / 2
        if not (lo < mid < hi):
            return hi
        if pnorm_upper(mid) > p:
            lo = mid
        else:
            hi = mid


def qnorm_upper_indep(p):
    """an independent route: the standard library's inverse normal CDF"""
    return -statistics.NormalDist().inv_cdf(p)


def weights(radius, qnorm=qnorm_upper):
    ln = 2 * radius + 1
    if radius == 0:
        return np.ones(1)
    a = 3.0 / 8.0 if ln <= 10 else 0.5
    p1 = (1.0 - a) / (float(ln) + 1.0 - 2.0 * a)
    L = qnorm(p1)
    step = (2.0 * L) / float(ln - 1)
    w = np.empty(ln)
    for i in range(ln):
        t = -L + float(i) * step
        w[i] = math.exp(-(t * t) / 2.0) / 2.5066282746310002
    return w


def rollmean(x, seg_start, radius, w=None):
    """S2 per segment [seg_start[s], seg_start[s + 1]): plain loops in the stated order.  Raises ValueError where the library
    returns TPG_EINVAL"""
    x = np.asarray(x, dtype=np.float64)
    ln = 2 * radius + 1
    for a, b in zip(seg_start[:-1], seg_start[1:]):
        if b - a < ln:
            raise ValueError("roll_size exceeds the number of variants on at least one chromosome")
    if radius == 0:
        return x.copy()
    w = weights(radius) if w is None else np.asarray(w, dtype=np.float64)
    out = np.empty(len(x))
    for a, b in zip(seg_start[:-1], seg_start[1:]):
        for j in range(a, b):
            num, den = np.float64(0.0), np.float64(0.0)
            for i in range(ln):
                p = j - radius + i
                if a <= p < b:
                    num = num + w[i] * x[p]
                    den = den + w[i]
            out[j] = num / den
    return out


def rollmean_fast(x, seg_start, radius, w=None):
    """the same sums with the loop over i outermost (every element still adds its terms in ascending i from +0): bit for bit
    rollmean, at numpy speed"""
    x = np.asarray(x, dtype=np.float64)
    ln = 2 * radius + 1
    for a, b in zip(seg_start[:-1], seg_start[1:]):
        if b - a < ln:
            raise ValueError("roll_size exceeds the number of variants on at least one chromosome")
    if radius == 0:
        return x.copy()
    w = weights(radius) if w is None else np.asarray(w, dtype=np.float64)
    out = np.empty(len(x))
    for a, b in zip(seg_start[:-1], seg_start[1:]):
        seg = x[a:b]
        num, den = np.zeros(b - a), np.zeros(b - a)
        j = np.arange(b - a)
        for i in range(ln):
            p = j - radius + i
            ok = (p >= 0) & (p < b - a)
            num[ok] = num[ok] + w[i] * seg[p[ok]]
            den[ok] = den[ok] + w[i]
        out[a:b] = num / den
    return out


# ---- quartiles, medcouple, fence --------------------------------------------------------------------------------------------
def finite_sorted(x):
    x = np.asarray(x, dtype=np.float64) + 0.0
    return np.sort(x[np.isfinite(x)])


def quantile7(s, p):
    c = len(s)
    if c == 0:
        return np.nan
    h = float(c - 1) * p
    lo = int(math.floor(h))
    up = min(lo + 1, c - 1)
    return s[lo] + (h - float(lo)) * (s[up] - s[lo])


def _split(x):
    """A (z > 0), B (|z| for z <= 0, ascending), k (values equal to the median)"""
    s = finite_sorted(x)
    z = s - pr.med(s)
    return z[z > 0], np.sort(np.abs(z[z <= 0])), int((z == 0).sum())


def _g(r):
    return -1.0 if math.isinf(r) else (1.0 - r) / (1.0 + r)


def medcouple_brute(x):
    """all N ratios, sorted"""
    if len(finite_sorted(x)) == 0:
        return np.nan
    A, B, k = _split(x)
    with np.errstate(over="ignore"):
        r = (B[None, :] / A[:, None]).ravel()
    half = k * (k - 1) // 2
    r = np.sort(np.concatenate([r, np.full(k * (len(B) - k) + half, np.inf), np.zeros(half), np.ones(k)]))
    N = (len(A) + k) * len(B)
    assert len(r) == N
    return (_g(r[(N - 1) // 2]) + _g(r[N // 2])) / 2


def medcouple_classical(x):
    """the kernel h = (a - b) / (a + b) over z+ x z-, sign(k - 1 - i - j) where both are at the median; the mean of the two
    middle values"""
    s = finite_sorted(x)
    if len(s) == 0:
        return np.nan
    z = s - pr.med(s)
    zp, zm = z[z >= 0][::-1], z[z <= 0]  # descending, ascending: the k zeros end zp and end zm
    k = int((z == 0).sum())
    a, b = zp[:, None], -zm[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        h = (a - b) / (a + b)
    if k:
        i, j = np.arange(k)[:, None], np.arange(k)[None, :]
        h[len(zp) - k:, len(zm) - k:] = np.sign(k - 1 - i - j)
    h = np.sort(h.ravel())
    N = len(h)
    return (h[(N - 1) // 2] + h[N // 2]) / 2


def tie_count(k, nB, cand):
    half = k * (k - 1) // 2
    return half + (k if cand >= BITS_ONE else 0) + (half + k * (nB - k) if cand >= BITS_INF else 0)


def _prefix_counts(A, B, cand):
    """sum over a in A of the number of b in B (ascending) whose b / a has a bit pattern <= cand: a binary search per row"""
    lo, hi = np.zeros(len(A), dtype=np.int64), np.full(len(A), len(B), dtype=np.int64)
    while True:
        act = lo < hi
        if not act.any():
            return int(lo.sum())
        mid = (lo + hi) // 2
        with np.errstate(over="ignore"):
            r = B[np.minimum(mid, len(B) - 1)] / A
        le = r.view(np.uint64) <= np.uint64(cand)
        lo = np.where(act & le, mid + 1, lo)
        hi = np.where(act & ~le, mid, hi)


def medcouple_bisect(x):
    """the two middle ratios by bisection over the 63-bit pattern, counting without forming the ratios"""
    if len(finite_sorted(x)) == 0:
        return np.nan
    A, B, k = _split(x)
    N = (len(A) + k) * len(B)
    ratio = {}
    for rank in {(N - 1) // 2, N // 2}:
        P = 0
        for bit in range(62, -1, -1):
            cand = P | ((1 << bit) - 1)
            if _prefix_counts(A, B, cand) + tie_count(k, len(B), cand) < rank + 1:
                P |= 1 << bit
        ratio[rank] = float(np.uint64(P).view(np.float64))
    return (_g(ratio[(N - 1) // 2]) + _g(ratio[N // 2])) / 2


def tukey_mc_up(x, alpha=0.05, medcouple=medcouple_brute, qnorm=qnorm_upper):
    s = finite_sorted(x)
    c = len(s)
    if c == 0:
        return dict(n_finite=0, q1=np.nan, q3=np.nan, med=np.nan, mc=np.nan, coef=np.nan, thr=np.nan)
    q1, q3, mc = quantile7(s, 0.25), quantile7(s, 0.75), medcouple(x)
    z75 = qnorm(0.25)
    coef = (qnorm(alpha / float(c)) - z75) / (2.0 * z75)
    e = math.exp(3.0 * mc) if mc >= 0.0 else math.exp(4.0 * mc)
    return dict(n_finite=c, q1=q1, q3=q3, med=pr.med(s), mc=mc, coef=coef, thr=q3 + coef * (q3 - q1) * e)


# ---- runs of outliers -------------------------------------------------------------------------------------------------------
def outlier_runs(pos, chrom_of, min_size):
    """[(first, last)] as indices into pos: maximal stretches of consecutive positions on one chromosome, at least min_size"""
    runs, a = [], 0
    for i in range(1, len(pos) + 1):
        if i < len(pos) and pos[i] == pos[i - 1] + 1 and chrom_of[i] == chrom_of[i - 1]:
            continue
        if i - a >= min_size:
            runs.append((a, i - 1))
        a = i
    return runs


# ---- the planted panel ------------------------------------------------------------------------------------------------------
N_POP, PER_POP, FST = 3, 50, 0.05
CHROM_SIZES = (700, 900, 600)
M_PANEL = sum(CHROM_SIZES)
BLOCK = np.arange(1000, 1120)
LOW_MAC = np.array([10, 350, 720, 1300, 1700, 2100])
DELTA = 0.4  # difference of the allele frequency between the two arrangements, either side of the locus's own frequency
PANEL_K, PANEL_ROLL, PANEL_WINDOW, PANEL_THR = 4, 10, 50, 0.2
CHROM = np.repeat(np.arange(1, 4), CHROM_SIZES)
POSITION = np.concatenate([1000 * np.arange(1, s + 1) for s in CHROM_SIZES])


def planted_panel(seed=0, low_mac=True):
    """150 x 2200 genotypes from one default_rng(seed), drawn in the order of the statements below: ancestral frequencies,
    Balding-Nichols population frequencies, genotypes population by population; then the block: an arrangement per
    haplotype (frequency 1/2), the block's centre frequencies, the sign of each locus's shift, and the alleles of both
    haplotypes; at last the six loci of low minor allele count (3 + i heterozygotes at the first individuals)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, M_PANEL)
    P = rng.beta(p * (1 - FST) / FST, (1 - p) * (1 - FST) / FST, size=(N_POP, M_PANEL))
    P = np.clip(P, 0.1, 0.9)  # no locus of low minor allele count but the six written below
    G = np.concatenate([rng.binomial(2, P[g], size=(PER_POP, M_PANEL)) for g in range(N_POP)], axis=0)
    n = G.shape[0]
    arr = rng.random((2, n)) < 0.5
    centre = rng.uniform(0.35, 0.65, len(BLOCK))
    sign = np.where(rng.random(len(BLOCK)) < 0.5, -1.0, 1.0)
    hap = np.zeros((n, len(BLOCK)), dtype=np.int64)
    for h in range(2):
        freq = centre[None, :] + np.where(arr[h][:, None], 0.5, -0.5) * DELTA * sign[None, :]
        hap += rng.random((n, len(BLOCK))) < freq
    G[:, BLOCK] = hap
    if low_mac:
        for i, j in enumerate(LOW_MAC):
            G[:, j] = 0
            G[:3 + i, j] = 1
    return np.asfortranarray(G.astype(np.int64))


# ---- the whole loop ---------------------------------------------------------------------------------------------------------
def svd_loadings(G, k):
    """d, u, v, center, scale of the binomially scaled panel (numpy's SVD)"""
    G = np.asarray(G, dtype=np.float64)
    mean = G.mean(axis=0)
    sd = np.sqrt(2 * (mean / 2) * (1 - mean / 2))
    u, d, vt = np.linalg.svd((G - mean) / sd, full_matrices=False)
    return d[:k], u[:, :k], vt[:k].T, mean, sd


def segments_of(chrom_kept):
    c = np.asarray(chrom_kept)
    return np.r_[0, np.flatnonzero(c[1:] != c[:-1]) + 1, len(c)].astype(np.int64)


def detect(V, chrom_kept, roll_size, alpha):
    """steps 3 - 5 on the loadings of one iteration -> dict(S, S2, report, out (boolean))"""
    S = np.sqrt(pr.ogk_ref(V)["dist"])
    if not np.isfinite(S).all():
        raise ValueError("a robust distance that is not finite")
    S2 = rollmean_fast(S, segments_of(chrom_kept), roll_size)
    rep = tukey_mc_up(S2, alpha, medcouple=medcouple_bisect)
    return dict(S=S, S2=S2, report=rep, out=S2 > rep["thr"])


def autosvd_ref(G, chrom, hi=None, k=10, thr_r2=0.2, roll_size=50, alpha=0.05, min_mac=10, max_iter=5, int_min_size=20):
    """-> dict(kept (0-based loci), n_iter, converged, history = [dict(n_kept, n_outliers, pos0, idx0, report, S2, runs)])"""
    G = np.asarray(G)
    chrom = np.asarray(chrom)
    starts = segments_of(chrom)[:-1]
    if len(np.unique(chrom[starts])) != len(starts):
        raise ValueError("loci are not ordered")
    if (G < 0).any() or (G > 2).any():
        raise ValueError("a missing genotype")
    n, sx, _ = lr.sums(G)
    exclude = np.minimum(sx, 2 * n - sx) < min_mac
    keep = ~exclude if hi is None else lr.clump(G, hi, thr_r2, exclude=exclude)[0]
    kept = np.flatnonzero(keep)
    it, history, converged = 0, [], False
    while True:
        it += 1
        if it > max_iter:
            break
        V = svd_loadings(G[:, kept], k)[2]
        r = detect(V, chrom[kept], roll_size, alpha)
        pos = np.flatnonzero(r["out"])
        runs = [(int(kept[pos[a]]), int(kept[pos[b]])) for a, b in outlier_runs(pos, chrom[kept[pos]], int_min_size)]
        history.append(dict(n_kept=len(kept), n_outliers=len(pos), pos0=pos, idx0=kept[pos], report=r["report"], S2=r["S2"], runs=runs))
        if len(pos) == 0:
            converged = True
            break
        kept = kept[~r["out"]]
    return dict(kept=kept, n_iter=it, converged=converged, history=history)


# ---- the planted panel as the tests use it ----------------------------------------------------------------------------------
# generator seed 1: the smallest |S2 - thr| / thr over loci and iterations is 1.5e-2 (seeds 0 and 2: 2.6e-3 and 2.1e-2)
PANEL_SEED = 1


def planted_reference(seed=PANEL_SEED):
    """(G, hi, the reference's run) at k = 4, roll_size = 10, a window of 50 loci, thr_r2 = 0.2"""
    G = planted_panel(seed)
    hi = lr.window_hi(CHROM, None, PANEL_WINDOW, use_positions=False)
    return G, hi, autosvd_ref(G, CHROM, hi, k=PANEL_K, thr_r2=PANEL_THR, roll_size=PANEL_ROLL)


def check_planted_reference(G, r):
    """the conditions on the reference alone (a drifted generator is caught here) -> the margin"""
    assert G.shape == (150, 2200) and r["converged"] and r["n_iter"] == 2, (r["n_iter"], r["converged"])
    n, sx, _ = lr.sums(G)
    assert sorted(np.flatnonzero(np.minimum(sx, 2 * n - sx) < 10)) == sorted(LOW_MAC)
    removed = r["history"][0]["idx0"]
    assert removed.min() >= BLOCK[0] - PANEL_ROLL and removed.max() <= BLOCK[-1] + PANEL_ROLL
    assert np.isin(BLOCK, removed).sum() >= 100 and r["history"][1]["n_outliers"] == 0
    margin = min(float(np.min(np.abs(h["S2"] - h["report"]["thr"]) / h["report"]["thr"])) for h in r["history"])
    assert margin >= 1e-4, margin
    return margin
