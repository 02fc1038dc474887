"""Runs of homozygosity as include/tpg.h defines them ("Runs of homozygosity"), restated in numpy in two forms: a literal loop
over individuals, windows and loci, and a vectorised one on cumulative sums.  Everything is an integer except need[c] and the
density comparison, which are written exactly as the header states them.  Also the panels and locus tables of the tests."""
import math

import numpy as np

DEFAULTS = dict(window_size=15, threshold=0.05, min_snp=3, heterozygosity=False, max_opp_window=1, max_miss_window=1,
                max_gap=10**6, min_length_bps=1000, min_density=1 / 1000, max_opp_run=None, max_miss_run=None)
UNFILTERED = dict(min_snp=1, min_length_bps=0, min_density=0.0)
# (name, overrides on top of UNFILTERED, must leave runs): the filters of the non-vacuity list; "W" stands for the window size
FILTERS = (("min_snp", dict(min_snp="W+5"), True), ("min_length_bps", dict(min_length_bps=30000), True),
           ("max_opp_run", dict(max_opp_run=0), True), ("max_miss_run", dict(max_miss_run=0), True),
           ("threshold_0.5", dict(threshold=0.5), True), ("threshold_1.0", dict(threshold=1.0), True),
           ("clean_windows", dict(max_opp_window=0, max_miss_window=0), True),
           ("min_density", dict(min_density=1.0), False), ("max_gap", dict(max_gap=2000), False))


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    if p["min_snp"] == "W+5":
        p["min_snp"] = p["window_size"] + 5
    return p


def breaks(chrom, pos, max_gap):
    """brk[j], 0 <= j < m - 1; a position that decreases inside a chromosome is an error"""
    chrom, pos = np.asarray(chrom), np.asarray(pos, dtype=np.int64)
    same = chrom[1:] == chrom[:-1]
    d = pos[1:] - pos[:-1]
    if np.any(same & (d < 0)):
        raise ValueError("loci are not ordered: positions decrease inside a chromosome")
    return ~same | (d > max_gap)


def need_table(W, threshold):
    return np.array([0] + [max(1, math.ceil(threshold * float(c))) for c in range(1, W + 1)], dtype=np.int64)


def opp_miss(G, heterozygosity):
    G = np.asarray(G)
    return ((G == 0) | (G == 2)) if heterozygosity else (G == 1), G == 3


def status_loop(G, chrom, pos, p):
    """step 1 - 4, literally"""
    W = p["window_size"]
    opp, miss = opp_miss(G, p["heterozygosity"])
    n, m = opp.shape
    brk = breaks(chrom, pos, p["max_gap"])
    need = need_table(W, p["threshold"])
    out = np.zeros((n, m), dtype=bool)
    if m < W:
        return out
    for i in range(n):
        ok = []
        for w in range(m - W + 1):
            ok.append(int(opp[i, w:w + W].sum()) <= p["max_opp_window"] and int(miss[i, w:w + W].sum()) <= p["max_miss_window"]
                      and not brk[w:w + W - 1].any())
        for j in range(m):
            lo, hi = max(0, j - W + 1), min(j, m - W)
            hits = sum(ok[lo:hi + 1])
            out[i, j] = hits >= need[hi - lo + 1]
    return out


def status_vec(G, chrom, pos, p):
    W = p["window_size"]
    opp, miss = opp_miss(G, p["heterozygosity"])
    n, m = opp.shape
    if m < W:
        return np.zeros((n, m), dtype=bool)
    brk = breaks(chrom, pos, p["max_gap"])
    need = need_table(W, p["threshold"])
    nw = m - W + 1

    def csum(a):
        return np.concatenate([np.zeros(a.shape[:-1] + (1,), dtype=np.int64), np.cumsum(a, axis=-1, dtype=np.int64)], axis=-1)

    co, cm, cb = csum(opp), csum(miss), csum(brk)  # cb[j] = breaks among brk[0 .. j - 1], j = 0 .. m - 1
    w = np.arange(nw)
    ok = (co[:, w + W] - co[:, w] <= p["max_opp_window"]) & (cm[:, w + W] - cm[:, w] <= p["max_miss_window"])
    ok &= (cb[w + W - 1] - cb[w] == 0)[None, :]
    cq = csum(ok)
    j = np.arange(m)
    lo, hi = np.maximum(0, j - W + 1), np.minimum(j, m - W)
    return cq[:, hi + 1] - cq[:, lo] >= need[hi - lo + 1][None, :]


def _is_run(nsnp, length, nopp, nmiss, p):
    keep = nsnp >= p["min_snp"] and length >= p["min_length_bps"]
    keep = keep and float(nsnp) * 1000.0 >= p["min_density"] * float(length)
    if p["max_opp_run"] is not None and p["max_opp_run"] >= 0:
        keep = keep and nopp <= p["max_opp_run"]
    if p["max_miss_run"] is not None and p["max_miss_run"] >= 0:
        keep = keep and nmiss <= p["max_miss_run"]
    return keep


def _table(rows):
    a = np.array(rows, dtype=np.int64).reshape(-1, 5)
    return dict(indiv=a[:, 0], first=a[:, 1], last=a[:, 2], n_opp=a[:, 3], n_miss=a[:, 4])


def runs_loop(G, status, chrom, pos, p):
    """step 5, literally: walk the loci of every individual"""
    opp, miss = opp_miss(G, p["heterozygosity"])
    n, m = opp.shape
    pos = np.asarray(pos, dtype=np.int64)
    brk = breaks(chrom, pos, p["max_gap"])
    rows = []
    for i in range(n):
        a = None
        for j in range(m):
            if status[i, j] and a is None:
                a = j
            if a is not None and (j == m - 1 or not status[i, j + 1] or brk[j]):
                nopp, nmiss = int(opp[i, a:j + 1].sum()), int(miss[i, a:j + 1].sum())
                if _is_run(j - a + 1, int(pos[j] - pos[a]), nopp, nmiss, p):
                    rows.append((i, a, j, nopp, nmiss))
                a = None
    return _table(rows)


def runs_vec(G, status, chrom, pos, p):
    opp, miss = opp_miss(G, p["heterozygosity"])
    n, m = opp.shape
    pos = np.asarray(pos, dtype=np.int64)
    brk = breaks(chrom, pos, p["max_gap"])
    cut_before = np.concatenate([[True], brk])  # a segment cannot continue into locus j from j - 1
    cut_after = np.concatenate([brk, [True]])
    prev = np.concatenate([np.zeros((n, 1), dtype=bool), status[:, :-1]], axis=1)
    nxt = np.concatenate([status[:, 1:], np.zeros((n, 1), dtype=bool)], axis=1)
    si, sj = np.nonzero(status & (~prev | cut_before[None, :]))
    ei, ej = np.nonzero(status & (~nxt | cut_after[None, :]))
    assert np.array_equal(si, ei) and np.all(ej >= sj)
    co = np.concatenate([np.zeros((n, 1), dtype=np.int64), np.cumsum(opp, axis=1)], axis=1)
    cm = np.concatenate([np.zeros((n, 1), dtype=np.int64), np.cumsum(miss, axis=1)], axis=1)
    nopp, nmiss = co[si, ej + 1] - co[si, sj], cm[si, ej + 1] - cm[si, sj]
    nsnp, length = ej - sj + 1, pos[ej] - pos[sj]
    keep = (nsnp >= p["min_snp"]) & (length >= p["min_length_bps"])
    keep &= nsnp.astype(np.float64) * 1000.0 >= p["min_density"] * length.astype(np.float64)
    if p["max_opp_run"] is not None and p["max_opp_run"] >= 0:
        keep &= nopp <= p["max_opp_run"]
    if p["max_miss_run"] is not None and p["max_miss_run"] >= 0:
        keep &= nmiss <= p["max_miss_run"]
    return dict(indiv=si[keep], first=sj[keep], last=ej[keep], n_opp=nopp[keep], n_miss=nmiss[keep])


def roh_loop(G, chrom, pos, **kw):
    p = params(**kw)
    return runs_loop(G, status_loop(G, chrom, pos, p), chrom, pos, p)


def roh_vec(G, chrom, pos, **kw):
    p = params(**kw)
    return runs_vec(G, status_vec(G, chrom, pos, p), chrom, pos, p)


def same_runs(a, b):
    return all(np.array_equal(np.asarray(a[k], dtype=np.int64), np.asarray(b[k], dtype=np.int64))
               for k in ("indiv", "first", "last", "n_opp", "n_miss"))


def run_set(r):
    return set(zip(r["indiv"].tolist(), r["first"].tolist(), r["last"].tolist()))


def pack_bits(status, stride=None):
    """(n, m) bool -> (n, stride) uint32, bit j & 31 of word j >> 5; padding bits and unused words 0"""
    n, m = status.shape
    nw = -(-m // 32)
    stride = nw if stride is None else stride
    padded = np.zeros((n, stride * 32), dtype=np.uint8)
    padded[:, :m] = status
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint32).reshape(n, stride)


def indiv_summary(runs, n, pos):
    pos = np.asarray(pos, dtype=np.int64)
    n_runs = np.bincount(runs["indiv"], minlength=n).astype(np.int64)
    total = np.zeros(n, dtype=np.int64)
    np.add.at(total, runs["indiv"], pos[runs["last"]] - pos[runs["first"]])
    return n_runs, total


def locus_counts(runs, m):
    d = np.zeros(m + 1, dtype=np.int64)
    np.add.at(d, runs["first"], 1)
    np.add.at(d, runs["last"] + 1, -1)
    return np.cumsum(d)[:m].astype(np.int32)


# ---- panels -------------------------------------------------------------------------------------------------------------
def roh_panel(seed, n, m, W):
    """diploid draws at per-locus frequencies (most alleles rare, so that a short stretch between two breaks can be free of
    heterozygotes by chance), homozygous stretches of W / 2 .. 4 W loci planted into every individual (a heterozygote
    survives inside one with probability 0.03), about 1 % missing; codes 0, 1, 2 and 3 = missing"""
    rng = np.random.default_rng([seed, n, m, W])
    f = 0.02 + 0.48 * rng.random(m) ** 2
    G = rng.binomial(2, f[None, :], size=(n, m)).astype(np.uint8)
    for i in range(n):
        for _ in range(m // (8 * W) + 1):
            L = int(rng.integers(max(1, W // 2), 4 * W + 1))
            a = int(rng.integers(0, max(1, m - L + 1)))
            seg = G[i, a:a + L]
            fix = (seg == 1) & (rng.random(len(seg)) >= 0.03)
            seg[fix] = 2 * rng.integers(0, 2, int(fix.sum()), dtype=np.uint8)
    G[rng.random((n, m)) < 0.01] = 3
    return G


def roh_loci(seed, m, W=15, max_spacing=3000, zero_share=0.1, gap_share=None, max_gap=10**6):
    """chrom (int32) and pos (int64) of m ordered loci: up to three chromosomes (each several W long); spacings of up to
    max_spacing bp in sparse regions and a tenth of that in dense ones (regions of 4 W loci), a share of them zero, and a
    small share above max_gap, half of which are followed by a second one W .. 2 W loci later (a short stretch with a
    break on either side).  gap_share defaults to 1 / (16 W): unbroken stretches stay several windows long whatever W is."""
    rng = np.random.default_rng([seed, m, W, 7])
    nchrom = int(max(1, min(3, m // (4 * W))))
    cuts = np.sort(rng.choice(np.arange(1, m), nchrom - 1, replace=False)) if nchrom > 1 else np.array([], dtype=np.int64)
    chrom = np.searchsorted(cuts, np.arange(m), side="right").astype(np.int32) + 1
    gap_share = 1.0 / (16 * W) if gap_share is None else gap_share
    dense = rng.random(m // (4 * W) + 1) < 0.5
    scale = np.where(dense[np.arange(m) // (4 * W)], max(1, max_spacing // 10), max_spacing)
    sp = (1 + rng.random(m) * scale).astype(np.int64)
    u = rng.random(m)
    sp[u < zero_share] = 0
    gaps = np.flatnonzero(u > 1 - gap_share)
    second = gaps[rng.random(len(gaps)) < 0.5]
    second = second + rng.integers(W, 2 * W + 1, len(second))
    gaps = np.concatenate([gaps, second])
    sp[gaps[gaps < m]] = max_gap + 1 + rng.integers(0, 1000, int((gaps < m).sum()))
    pos = np.empty(m, dtype=np.int64)
    for c in range(1, nchrom + 1):
        idx = np.flatnonzero(chrom == c)
        pos[idx] = 1000 + np.cumsum(sp[idx])
    return chrom, pos


# the panels of the filter tests: (seed, n, m, W)
FILTER_PANELS = ((1, 33, 1000, 15), (2, 32, 128, 15), (3, 65, 257, 2), (4, 64, 4097, 50), (5, 33, 4097, 128))
# the filters that may empty the set
MAY_EMPTY = ("min_density", "max_gap")
