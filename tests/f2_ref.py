"""Blocked f2, allele-frequency products and the f4 block jackknife restated in Python from include/tpg.h "f2 blocks" (the
arithmetic lives in admixtools, which is not among the reference's sources; R/gt_extract_f2.R:141-189 only calls it).  Two
routes: a float route (numpy, the formulas as written, sums in ascending locus order) and an exact route (integers and
fractions.Fraction for sum of terms / cnt, the filter decisions on integer counts so that none can flip on a rounding).  And a
panel generator with the awkward groups and loci planted."""
from fractions import Fraction
from math import gcd

import numpy as np

MISSING = 3
POLY_F2, POLY_AP = 1, 2
DEFAULTS = dict(maxmiss=0.0, minmaf=0.0, maxmaf=0.5, minac2=0, poly_only=POLY_F2, apply_corr=1, keep=None)


def params(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return {**DEFAULTS, **kw}


# ---- counts ---------------------------------------------------------------------------------------------------------------
def group_tables(codes, gid, G, ploidy=None):
    """codes: n x m uint8 (0, 1, 2, 3 = missing) -> alt2, c (m x G int64): TWICE the alternate alleles (a pseudohaploid adds
    half its code to the alleles, so twice that stays an integer) and the valid alleles (2 per typed diploid, 1 per typed
    pseudohaploid), as tpg_grouped_alt_freq_dip_pseudo counts them"""
    codes = np.asarray(codes)
    n, m = codes.shape
    gid = np.zeros(n, dtype=np.int64) if gid is None else np.asarray(gid)
    pl = np.full(n, 2.0) if ploidy is None else np.asarray(ploidy, dtype=np.float64)
    typed = codes != MISSING
    dos = np.where(typed, codes, 0).astype(np.int64)
    alt2 = np.zeros((m, G), dtype=np.int64)
    c = np.zeros((m, G), dtype=np.int64)
    for g in range(G):
        d, h = (gid == g) & (pl == 2.0), (gid == g) & (pl == 1.0)
        alt2[:, g] = 2 * dos[d].sum(axis=0) + dos[h].sum(axis=0)
        c[:, g] = 2 * typed[d].sum(axis=0) + typed[h].sum(axis=0)
    return alt2, c


# ---- float route ----------------------------------------------------------------------------------------------------------
def p_e_float(alt2, c, apply_corr):
    """p = alt / c and e = (p (1 - p)) / max(1, c - 1) in this order in double; NaN where c = 0"""
    cf = c.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = (alt2.astype(np.float64) * 0.5) / cf  # alt2 / 2 is exact
        e = (p * (1.0 - p)) / np.maximum(1.0, cf - 1.0) if apply_corr else np.where(c > 0, 0.0, np.nan)
    return p, e


def flags_float(alt2, c, pr):
    """-> kept, poly (bool[m]) with the float arithmetic of the definition"""
    m, G = c.shape
    p, _ = p_e_float(alt2, c, 0)
    t = c > 0
    ntyped = t.sum(axis=1)
    kept = ntyped > 0
    kept &= ~((G - ntyped).astype(np.float64) / float(G) > pr["maxmiss"])
    s = np.zeros(m)
    for g in range(G):  # ascending g, one term after the other
        s = np.where(t[:, g], s + np.where(t[:, g], p[:, g], 0.0), s)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = s / ntyped.astype(np.float64)
        r = 1.0 - f
        maf = np.where(f < r, f, r)
        kept &= ~((maf < pr["minmaf"]) | (maf > pr["maxmaf"]))
    if pr["minac2"]:
        kept &= ~(c < 2).any(axis=1)
    if pr["keep"] is not None:
        kept &= np.asarray(pr["keep"]) != 0
    first = np.argmax(t, axis=1)
    pf = p[np.arange(m), first]
    poly = (t & (p != pf[:, None])).any(axis=1)
    return kept, poly


def blocks_float(alt2, c, lo, hi, pr, flags=None):
    """the float route -> dict(f2, cnt, ap, ap_cnt (G, G, nb), n_kept).  flags = (kept, poly) overrides the float decisions (a
    caller that wants the exact route's)."""
    m, G = c.shape
    kept, poly = flags_float(alt2, c, pr) if flags is None else flags
    p, e = p_e_float(alt2, c, pr["apply_corr"])
    t = c > 0
    p0, e0 = np.where(t, p, 0.0), np.where(t, e, 0.0)
    w_f = kept & (poly | (pr["poly_only"] & POLY_F2 == 0))
    w_a = kept & (poly | (pr["poly_only"] & POLY_AP == 0))
    nb = len(lo)
    out = dict(f2=np.full((G, G, nb), np.nan), cnt=np.zeros((G, G, nb), dtype=np.int32), ap=np.full((G, G, nb), np.nan),
               ap_cnt=np.zeros((G, G, nb), dtype=np.int32), n_kept=np.zeros(nb, dtype=np.int64))
    for b in range(nb):
        sl = slice(int(lo[b]), int(hi[b]))
        out["n_kept"][b] = kept[sl].sum()
        mf = (t[sl] & w_f[sl, None]).astype(np.float64)
        ma = (t[sl] & w_a[sl, None]).astype(np.float64)
        pb, eb = p0[sl], e0[sl]
        n_f, n_a = mf.T @ mf, ma.T @ ma  # sums of products of zeros and ones: exact in any order
        pa = pb * ma
        s_a = pa.T @ pa                   # sum of p1 p2 over the loci kept for ap: a dot product per pair
        with np.errstate(invalid="ignore", divide="ignore"):
            out["ap"][:, :, b] = np.where(n_a > 0, s_a / n_a, np.nan)
        out["cnt"][:, :, b], out["ap_cnt"][:, :, b] = n_f, n_a
        for g1 in range(G):
            d = pb[:, g1, None] - pb[:, g1:]
            term = (d * d - eb[:, g1, None] - eb[:, g1:]) * (mf[:, g1, None] * mf[:, g1:])
            n = n_f[g1, g1:]
            with np.errstate(invalid="ignore", divide="ignore"):
                v = np.where(n > 0, term.sum(axis=0) / n, np.nan)
            if n[0] > 0:
                v[0] = 0.0
            out["f2"][g1, g1:, b] = out["f2"][g1:, g1, b] = v
    return out


# ---- exact route ----------------------------------------------------------------------------------------------------------
def flags_exact(alt2, c, pr):
    """the filter decisions on integers and Fractions: maxmiss as Fraction(missing, G) > Fraction(maxmiss), maf as a Fraction
    against Fraction(minmaf) and Fraction(maxmaf), poly by cross-multiplication"""
    m, G = c.shape
    t = c > 0
    ntyped = t.sum(axis=1)
    kept = ntyped > 0
    mm = Fraction(pr["maxmiss"])
    kept &= np.array([Fraction(int(G - k), G) <= mm for k in range(G + 1)])[ntyped]
    lo_f, hi_f = Fraction(pr["minmaf"]), Fraction(pr["maxmaf"])
    if lo_f > 0 or hi_f < Fraction(1, 2):
        for j in np.flatnonzero(kept):
            f = sum((Fraction(int(alt2[j, g]), 2 * int(c[j, g])) for g in range(G) if t[j, g]), Fraction(0)) / int(ntyped[j])
            maf = min(f, 1 - f)
            if maf < lo_f or maf > hi_f:
                kept[j] = False
    if pr["minac2"]:
        kept &= ~(c < 2).any(axis=1)
    if pr["keep"] is not None:
        kept &= np.asarray(pr["keep"]) != 0
    first = np.argmax(t, axis=1)
    af, cf = alt2[np.arange(m), first], c[np.arange(m), first]
    poly = (t & (alt2 * cf[:, None] != af[:, None] * c)).any(axis=1)  # alt2 / c != alt2_first / c_first
    return kept, poly


def _lcm(values):
    k = 1
    for v in values:
        k = k * int(v) // gcd(k, int(v))
    return k


def _scaled(num, den):
    """column-wise common denominators: num / den (m x G int64, den > 0 where it counts, num = 0 elsewhere) -> (N, K) with
    num / den = N / K[g]; N is int64 where every sum over the loci fits, Python integers otherwise"""
    m, G = num.shape
    K = [_lcm(np.unique(den[:, g][den[:, g] > 0])) for g in range(G)]
    big = max(K) ** 2 * max(m, 1) >= 2 ** 62
    N = np.zeros((m, G), dtype=object if big else np.int64)
    for g in range(G):
        ok = den[:, g] > 0
        if big:
            mult = {int(d): K[g] // int(d) for d in np.unique(den[ok, g])}
            N[ok, g] = [int(a) * mult[int(d)] for a, d in zip(num[ok, g], den[ok, g])]
        else:
            N[ok, g] = num[ok, g] * (K[g] // den[ok, g])
    return N, K


def blocks_exact(alt2, c, lo, hi, pr):
    """the exact route -> dict(cnt, ap_cnt (G, G, nb) int, n_kept, f2, ap: (G, G, nb) object arrays of Fraction, None where the
    count is 0; the diagonal of f2 is Fraction(0) where cnt > 0)"""
    m, G = c.shape
    kept, poly = flags_exact(alt2, c, pr)
    t = c > 0
    w_f = kept & (poly | (pr["poly_only"] & POLY_F2 == 0))
    w_a = kept & (poly | (pr["poly_only"] & POLY_AP == 0))
    cm1 = np.maximum(1, c - 1)
    # p = alt2 / (2 c);  a = p^2 - e = (alt2^2 max(1, c - 1) - alt2 (2 c - alt2)) / (4 c^2 max(1, c - 1))
    P, Kp = _scaled(np.where(t, alt2, 0), np.where(t, 2 * c, 0))
    corr = 1 if pr["apply_corr"] else 0
    A, Ka = _scaled(np.where(t, alt2 * alt2 * cm1 - corr * alt2 * (2 * c - alt2), 0), np.where(t, 4 * c * c * cm1, 0))
    nb = len(lo)
    out = dict(f2=np.full((G, G, nb), None, dtype=object), ap=np.full((G, G, nb), None, dtype=object),
               cnt=np.zeros((G, G, nb), dtype=np.int64), ap_cnt=np.zeros((G, G, nb), dtype=np.int64),
               n_kept=np.zeros(nb, dtype=np.int64))
    for b in range(nb):
        sl = slice(int(lo[b]), int(hi[b]))
        out["n_kept"][b] = kept[sl].sum()
        Mf = (t[sl] & w_f[sl, None]).astype(np.int64)
        Ma = (t[sl] & w_a[sl, None]).astype(np.int64)
        cnt, acnt = Mf.T @ Mf, Ma.T @ Ma
        SA = (A[sl] * Mf).T.dot(Mf.astype(A.dtype))   # [g1, g2] = Ka[g1] sum a1 m1 m2
        Pf, Pa = P[sl] * Mf, P[sl] * Ma
        SC, SCa = Pf.T.dot(Pf), Pa.T.dot(Pa)          # [g1, g2] = Kp[g1] Kp[g2] sum p1 p2 m1 m2
        out["cnt"][:, :, b], out["ap_cnt"][:, :, b] = cnt, acnt
        for g1 in range(G):
            for g2 in range(g1, G):
                if cnt[g1, g2] > 0:
                    s = Fraction(0)
                    if g1 != g2:
                        s = (Fraction(int(SA[g1, g2]), Ka[g1]) + Fraction(int(SA[g2, g1]), Ka[g2])
                             - 2 * Fraction(int(SC[g1, g2]), Kp[g1] * Kp[g2])) / int(cnt[g1, g2])
                    out["f2"][g1, g2, b] = out["f2"][g2, g1, b] = s
                if acnt[g1, g2] > 0:
                    out["ap"][g1, g2, b] = out["ap"][g2, g1, b] = Fraction(int(SCa[g1, g2]), Kp[g1] * Kp[g2] * int(acnt[g1, g2]))
    return out


def bound(lo, hi):
    """(4 L + 16) 2^-52 per block: p, e and the products carry at most about 12 roundings of values <= 1 per term, a sum of L
    such terms in any order adds at most L 2^-53 per unit of sum |terms| <= cnt, there are four sums, and the division by cnt
    >= the number of nonzero terms leaves about (4 L + 13) 2^-53; the bound is twice that"""
    return (4.0 * (np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64)) + 16.0) * 2.0 ** -52


def max_excess(got, exact, lo, hi):
    """largest |got - exact| / bound over ALL cells with a value (the caller asserts <= 1), after checking that NaN sits
    exactly where the exact route has no value"""
    bd = bound(lo, hi)
    nan = np.isnan(got)
    assert np.array_equal(nan, np.frompyfunc(lambda x: x is None, 1, 1)(exact).astype(bool)), "NaN cells differ"
    worst = 0.0
    for idx in zip(*np.nonzero(~nan)):
        err = abs(Fraction(float(got[idx])) - exact[idx])
        worst = max(worst, float(err / Fraction(float(bd[idx[2]]))))
    return worst


# ---- f4 / f3 block jackknife ----------------------------------------------------------------------------------------------
def f4_jackknife(f2, block_len, quad):
    """one quadruple (A, B, C, D), the operation order of include/tpg.h -> (est, se, n_used); numpy float64 scalars"""
    A, B, C, D = quad
    f2 = np.asarray(f2, dtype=np.float64)
    h = np.float64(0.5)
    with np.errstate(invalid="ignore", divide="ignore"):
        th = [h * (f2[A, D, b] + f2[B, C, b] - f2[A, C, b] - f2[B, D, b]) for b in range(f2.shape[2])]
        use = [b for b in range(len(th)) if not np.isnan(th[b]) and block_len[b] > 0]
        g = len(use)
        n, ws = np.float64(0.0), np.float64(0.0)
        for b in use:
            nbk = np.float64(block_len[b])
            n = n + nbk
            ws = ws + nbk * th[b]
        theta = ws / n if g > 0 else np.float64(np.nan)
        if g < 2:
            return theta, np.float64(np.nan), g
        sub = np.float64(0.0)
        for b in use:
            nbk = np.float64(block_len[b])
            loo = (n * theta - nbk * th[b]) / (n - nbk)
            sub = sub + (np.float64(1.0) - nbk / n) * loo
        est = np.float64(g) * theta - sub
        var = np.float64(0.0)
        for b in use:
            nbk = np.float64(block_len[b])
            loo = (n * theta - nbk * th[b]) / (n - nbk)
            hb = n / nbk
            tau = hb * theta - (hb - np.float64(1.0)) * loo
            dlt = tau - est
            var = var + dlt * dlt / (hb - np.float64(1.0))
        return est, np.sqrt(np.float64(1.0) / np.float64(g) * var), g


# ---- block ranges ---------------------------------------------------------------------------------------------------------
def block_ranges(chromosome, dist, blgsize):
    """the loop the definition describes, one locus at a time"""
    lo = []
    start = 0
    for j in range(len(chromosome)):
        if j == 0 or chromosome[j] != chromosome[j - 1] or float(dist[j]) - float(dist[start]) >= blgsize:
            start = j
            lo.append(j)
    lo = np.asarray(lo, dtype=np.int64)
    return lo, np.r_[lo[1:], len(chromosome)].astype(np.int64)


# ---- panels ---------------------------------------------------------------------------------------------------------------
def panel(seed, n, m, G, hap=True):
    """n x m codes, the group of every individual (None for G = 1) and the ploidy vector (None without pseudohaploids).
    Planted, where the shape has room (G >= 3 and n >= G + 1 for the groups):
      group G - 1 has no member; group G - 2 is one diploid individual (c - 1 = 1 and, where hap, group G - 3 gets a single
      pseudohaploid among its members: odd c, and c = 1 at locus m // 5 where it is the only one typed);
      locus m // 3: group 0 entirely missing;  loci m // 4 .. m // 4 + 9: monomorphic everywhere;
      loci m // 2 .. m // 2 + 4: everybody heterozygous (p = 1 / 2 in every group: equal but not monomorphic);
      locus 2 m // 3: typed in no group;  about 8 % missing elsewhere.
    Returns (codes, gid, ploidy, planted) with planted = dict of the loci above."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.05, 0.95, size=m)
    if G == 1:
        gid = None
        k = 1
    else:
        k = G - 1 if (G >= 3 and n >= G + 1) else G  # groups with members
        gid = (np.arange(n) % k).astype(np.int32)
        if k < G:
            gid[np.where(gid == k - 1)[0][1:]] = 0  # the last group with members is a singleton
    drift = rng.normal(0, 0.08, size=(k, m))
    g_of = np.zeros(n, dtype=np.int64) if gid is None else gid
    pj = np.clip(base[None, :] + drift[g_of], 0.02, 0.98)
    codes = rng.binomial(2, pj).astype(np.uint8)
    ploidy = None
    if hap and n >= 4:
        ploidy = np.full(n, 2.0)
        size = np.bincount(g_of, minlength=k)
        roomy = np.flatnonzero(size >= 2)  # the last group with company, so that c is odd there; otherwise the last row
        hrow = int(np.where(g_of == roomy[-1])[0][0]) if len(roomy) else n - 1
        ploidy[hrow] = 1.0
        codes[hrow] = np.where(codes[hrow] == 1, 2 * rng.integers(0, 2, size=m), codes[hrow])  # pseudohaploids are 0 / 2
    planted = dict(c1=m // 5, group0_missing=m // 3, mono=(m // 4, min(m, m // 4 + 10)), equal_p=(m // 2, min(m, m // 2 + 5)),
                   untyped=2 * m // 3)
    a, b = planted["mono"]
    codes[:, a:b] = 0
    codes[rng.random((n, m)) < 0.08] = MISSING
    a, b = planted["equal_p"]
    codes[:, a:b] = 1
    if ploidy is not None:  # a heterozygous code on a pseudohaploid row would count half an allele: keep p = 1 / 2 another way
        codes[ploidy == 1.0, a:b] = MISSING
    if m > 3:
        if ploidy is not None:  # the pseudohaploid is the only typed member of its group: c = 1
            codes[g_of == g_of[hrow], planted["c1"]] = MISSING
            codes[hrow, planted["c1"]] = 2
        codes[g_of == 0, planted["group0_missing"]] = MISSING
        codes[:, planted["untyped"]] = MISSING
    return codes, gid, ploidy, planted
