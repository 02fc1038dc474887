"""Site frequency spectra restated in Python from include/tpg.h "site frequency spectra" (the reference has no SFS code; the
definition is the header's, recalled from Marth et al. 2004 and Gutenkunst et al. 2009).  Two routes and the derived bounds:

  exact   rationals.  A projection row is a list of fractions.Fraction (exact_row).  The block sums keep, per group, ONE common
          denominator D_g = lcm over the v that occur of C(v, n_g), so that a weight is the integer h D_g and a cell of a
          spectrum an integer over D_g1 D_g2: the same rational numbers as a sum of Fractions, without a gcd per addition
          (test_sfs_host.py checks the two against each other).
  float   numpy doubles: the correctly rounded weights (an integer division in Python) and H'H by matmul.  With full-size
          projection every weight is 0 or 1 and this route is the exact integer histogram.

And a seeded panel builder with the awkward loci planted."""
from fractions import Fraction
from itertools import combinations
from math import comb, gcd

import numpy as np

MISSING = 3
U = 2.0 ** -53
TINY_ENTRY = Fraction(1, 2 ** 1000)  # below it an entry has no relative bound (csrc/host/host_sfs.h)
TINY_CELL = Fraction(1, 2 ** 900)    # ... and a cell (include/tpg.h)


# ---- bounds (derived in csrc/host/host_sfs.h and include/tpg.h by counting roundings; nothing here is measured) --------------
def entry_roundings(n):
    """9 n + 4: four per step of the recurrence (two conversions, a division, a product) over at most n steps, 5 n for the
    normalising sum (its n + 1 terms within 4 n each, n additions), one for the last division, three spare"""
    return 9 * n + 4


def cell_roundings(nmax, L):
    """18 n + L + 80: two weights, one product, at most L additions of the chain and 63 of the partial sums, the rest spare"""
    return 18 * nmax + L + 80


# ---- panel -------------------------------------------------------------------------------------------------------------------
def panel(seed, sizes, m, miss=0.1, plant_v=None):
    """-> codes (n x m uint8: 0, 1, 2, 3 = missing), gid (the groups interleaved), planted: dict(untyped=(locus, group) at which
    the whole group is missing, mono=(a, b) a stretch where every typed genotype is 0, exact=[loci] at which group g has exactly
    plant_v[g] typed alleles; with missing data, sparse: a locus with one typed individual per group and none in group 0)"""
    rng = np.random.default_rng(seed)
    sizes = list(sizes)
    G, n = len(sizes), int(sum(sizes))
    gid = rng.permutation(np.repeat(np.arange(G), sizes)).astype(np.int32)
    p = rng.uniform(0.03, 0.97, size=m)
    pg = np.clip(p[None, :] + rng.normal(0, 0.08, size=(G, m)), 0.0, 1.0)
    codes = rng.binomial(2, pg[gid, :]).astype(np.uint8)
    codes[rng.random((n, m)) < miss] = MISSING
    big = int(np.argmax(sizes))
    planted = dict(untyped=(m // 3, big), mono=(m // 2 + 11, m // 2 + 11 + 37), exact=[])
    codes[gid == big, m // 3] = MISSING
    a, b = planted["mono"]
    codes[:, a:b] = np.where(codes[:, a:b] == MISSING, MISSING, 0)
    if miss > 0:  # one typed individual per group, none in group 0: v = (0, 2, 2, ...)
        planted["sparse"] = m // 5
        for g in range(G):
            codes[np.flatnonzero(gid == g)[0 if g == 0 else 1:], m // 5] = MISSING
    if plant_v is not None:
        for j in (5, m // 4, m - 9):
            for g in range(G):
                idx = np.flatnonzero(gid == g)
                typed = int(plant_v[g]) // 2
                col = rng.binomial(2, 0.4, size=len(idx)).astype(np.uint8)
                col[rng.permutation(len(idx))[typed:]] = MISSING
                codes[idx, j] = col
            planted["exact"].append(j)
    return codes, gid, planted


def group_tables(codes, gid, G):
    """-> x (alternate alleles among the typed), v (twice the typed): m x G int64"""
    codes = np.asarray(codes)
    gid = np.zeros(codes.shape[0], dtype=np.int64) if gid is None else np.asarray(gid)
    typed = codes != MISSING
    dos = np.where(typed, codes, 0).astype(np.int64)
    x = np.stack([dos[gid == g].sum(axis=0) for g in range(G)], axis=1)
    v = np.stack([2 * typed[gid == g].sum(axis=0) for g in range(G)], axis=1).astype(np.int64)
    return x, v


def proj_sizes(gid, G, proj=None):
    N = np.bincount(np.zeros(0, dtype=np.int64) if gid is None else np.asarray(gid), minlength=G).astype(np.int64)
    pj = np.zeros(G, dtype=np.int64) if proj is None else np.asarray(proj, dtype=np.int64)
    return np.where(pj == 0, 2 * N, pj)


def offsets(n):
    return np.r_[0, np.cumsum(np.asarray(n) + 1)].astype(np.int64)


# ---- rows --------------------------------------------------------------------------------------------------------------------
def exact_row(x, v, n):
    d = comb(v, n)
    return [Fraction(comb(x, k) * comb(v - x, n - k), d) for k in range(n + 1)]


def float_row(x, v, n):
    d = comb(v, n)
    return np.array([comb(x, k) * comb(v - x, n - k) / d for k in range(n + 1)])  # int / int: correctly rounded


def brute_row(x, v, n):
    """the share of the C(v, n) subsets of v labelled alleles (the first x counted) that hold k counted ones"""
    cnt = [0] * (n + 1)
    for sub in combinations(range(v), n):
        cnt[sum(1 for a in sub if a < x)] += 1
    return [Fraction(c, comb(v, n)) for c in cnt]


# ---- tables of a panel -------------------------------------------------------------------------------------------------------
def usable(v, n, keep=None):
    t = v >= np.asarray(n)[None, :]
    return t if keep is None else t & (np.asarray(keep) != 0)[:, None]


def counted(x, v, flip=None):
    return x if flip is None else np.where((np.asarray(flip) != 0)[:, None], v - x, x)


def weights_int(x, v, n, t):
    """-> Hint (m x W, Python integers: h D_g, 0 where the locus is not usable for the group), D (per column)"""
    m, G = x.shape
    o = offsets(n)
    Hint = np.zeros((m, int(o[-1])), dtype=object)
    D = np.ones(int(o[-1]), dtype=object)
    for g in range(G):
        ng = int(n[g])
        vs = sorted({int(a) for a in v[t[:, g], g]})
        Dg = 1
        for a in vs:
            c = comb(a, ng)
            Dg = Dg * c // gcd(Dg, c)
        D[o[g]:o[g + 1]] = Dg
        rows = {}
        for j in np.flatnonzero(t[:, g]):
            key = (int(x[j, g]), int(v[j, g]))
            if key not in rows:
                s = Dg // comb(key[1], ng)
                rows[key] = [comb(key[0], k) * comb(key[1] - key[0], ng - k) * s for k in range(ng + 1)]
            Hint[j, o[g]:o[g + 1]] = rows[key]
    return Hint, D


def weights_float(x, v, n, t):
    m, G = x.shape
    o = offsets(n)
    H = np.zeros((m, int(o[-1])))
    for g in range(G):
        rows = {}
        for j in np.flatnonzero(t[:, g]):
            key = (int(x[j, g]), int(v[j, g]))
            if key not in rows:
                rows[key] = float_row(key[0], key[1], int(n[g]))
            H[j, o[g]:o[g + 1]] = rows[key]
    return H


def n_used(t, lo, hi):
    ti = t.astype(np.int64)
    n1 = np.stack([ti[a:b].sum(axis=0) for a, b in zip(lo, hi)], axis=1) if len(lo) else np.zeros((t.shape[1], 0), dtype=np.int64)
    n2 = (np.stack([ti[a:b].T @ ti[a:b] for a, b in zip(lo, hi)], axis=2) if len(lo)
          else np.zeros((t.shape[1], t.shape[1], 0), dtype=np.int64))
    return n1, n2


def blocks_exact(Hint, D, lo, hi, joint=True):
    """-> dict(sfs_num (W, nb), sfs_den (W), jsfs_num (W, W, nb), jsfs_den (W, W)): Python integers"""
    W, nb = Hint.shape[1], len(lo)
    out = dict(sfs_num=np.zeros((W, nb), dtype=object), sfs_den=D)
    if joint:
        out.update(jsfs_num=np.zeros((W, W, nb), dtype=object), jsfs_den=np.outer(D, D))
    for b, (a, e) in enumerate(zip(lo, hi)):
        Hb = Hint[int(a):int(e)]
        if len(Hb):
            out["sfs_num"][:, b] = Hb.sum(axis=0)
            if joint:
                out["jsfs_num"][:, :, b] = np.dot(Hb.T, Hb)
    return out


def blocks_float(H, lo, hi, joint=True):
    W, nb = H.shape[1], len(lo)
    out = dict(sfs=np.zeros((W, nb), order="F"))
    if joint:
        out["jsfs"] = np.zeros((W, W, nb), order="F")
    for b, (a, e) in enumerate(zip(lo, hi)):
        Hb = H[int(a):int(e)]
        out["sfs"][:, b] = Hb.sum(axis=0)
        if joint:
            out["jsfs"][:, :, b] = Hb.T @ Hb
    return out


def excess(got, num, den, roundings):
    """worst |got - exact| / (roundings u exact) over the cells, exact = num / den; got must be +0.0 exactly where num is 0 (the
    cap on cells left out is zero: every nonzero exact cell is asserted to be at least TINY_CELL, so that it has a bound).
    The quotient is formed in double from the correctly rounded exact value (one rounding of the reference, one of the
    difference: 2 u against bounds of 100 u and more); a cell above 0.9 is done again in Fractions."""
    got = np.asarray(got)
    den = np.broadcast_to(np.asarray(den, dtype=object)[..., None], got.shape)
    rnd = np.broadcast_to(np.asarray(roundings, dtype=np.float64), got.shape)
    zero = np.asarray(num == 0, dtype=bool)
    assert np.all(got[zero] == 0.0) and not np.signbit(got[zero]).any(), "a cell that is exactly zero is not +0.0"
    nz = ~zero
    if not nz.any():
        return 0.0
    nzn, nzd, nzr, nzg = num[nz], den[nz], rnd[nz], got[nz]
    ex = (nzn / nzd).astype(np.float64)
    assert ex.min() > float(TINY_CELL) * 2, "an exact cell has no relative bound: choose another panel"
    q = np.abs(nzg - ex) / (nzr * U * ex) + 2.0 / nzr
    for i in np.flatnonzero(q > 0.9):
        e = Fraction(int(nzn[i]), int(nzd[i]))
        q[i] = float(abs(Fraction(float(nzg[i])) - e) / (Fraction(int(nzr[i]), 2 ** 53) * e))
    return float(q.max())


# ---- folding and statistics, restated ---------------------------------------------------------------------------------------
def fold1(s):
    n = len(s) - 1
    out = [0 * s[0]] * (n + 1)
    for k in range(n + 1):
        if 2 * k < n:
            out[k] = s[k] + s[n - k]
        elif 2 * k == n:
            out[k] = s[k]
    return out


def fold2(J):
    n1, n2 = len(J) - 1, len(J[0]) - 1
    out = [[0 * J[0][0] for _ in range(n2 + 1)] for _ in range(n1 + 1)]
    for a in range(n1 + 1):
        for c in range(n2 + 1):
            if 2 * (a + c) < n1 + n2:
                out[a][c] = J[a][c] + J[n1 - a][n2 - c]
            elif 2 * (a + c) == n1 + n2:
                out[a][c] = (J[a][c] + J[n1 - a][n2 - c]) / 2
    return out


def stats(s):
    """the statistics of tidypopgen_amd.sfs_stats in Fractions where they are rational (S, theta_pi, theta_h, H)"""
    n = len(s) - 1
    S = sum((Fraction(s[k]) for k in range(1, n)), Fraction(0))
    c2 = Fraction(n * (n - 1), 2)
    pi = sum((Fraction(k * (n - k)) * Fraction(s[k]) for k in range(1, n)), Fraction(0)) / c2
    th = sum((Fraction(k * k) * Fraction(s[k]) for k in range(1, n)), Fraction(0)) / c2
    return dict(S=S, theta_pi=pi, theta_h=th, fay_wu_h=pi - th, a1=sum(Fraction(1, i) for i in range(1, n)))


def project_spectrum(s, n_to):
    """an exact spectrum at n -> n_to < n by the hypergeometric kernel"""
    n = len(s) - 1
    out = [Fraction(0)] * (n_to + 1)
    for x in range(n + 1):
        if s[x] != 0:
            for k, h in enumerate(exact_row(x, n, n_to)):
                out[k] += s[x] * h
    return out


# ---- the host routine as a stand-alone program ------------------------------------------------------------------------------
def build_host_program(exe, sanitize=True):
    """tests/host/sfs_san.cpp (csrc/host/host_sfs.h on the host) -> exe"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    san = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", *san, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-function",
           "-I" + os.path.join(root, "tidypopgen_amd", "csrc"), os.path.join(root, "tests", "host", "sfs_san.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_host_program(exe, path, queries):
    """one (x, v, n) per query -> one float64 array of n + 1 entries per query"""
    import subprocess

    with open(path, "w") as fh:
        fh.write("\n".join(f"{x} {v} {n}" for x, v, n in queries) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [np.array([int(w) for w in line.split()], dtype=np.uint64).view(np.float64) for line in out.stdout.splitlines()]
    assert len(rows) == len(queries)
    return rows
