"""Windowed pairwise Fst restated in numpy (include/tpg.h "windowed pairwise Fst"; R/windows_pairwise_pop_fst.R:62-107 over
R/windows_stats_generic.R:113-179) from the by-locus numerators and denominators, and pbs_one_triplet of
R/nwise_pop_pbs.R:116-157.  Two routes for a window sum: a float route (the non-NaN doubles added one after the other in
ascending locus order) and an exact route (math.fsum, or fractions.Fraction, of the same doubles), so that truth does not rest
on a summation order."""
import math
from fractions import Fraction

import numpy as np


def window_sums(x, lo, hi, pad_na=None):
    """x: m x P doubles -> (sum of the non-NaN x over lo[w] .. hi[w]-1 added sequentially, their number, the sum of their
    absolute values), each nw x P; a pad_na window sums nothing"""
    x = np.asarray(x, dtype=np.float64)
    ok = ~np.isnan(x)
    x0 = np.where(ok, x, 0.0)  # adding +0.0 changes no bit of a running sum that started at +0.0
    nw, P = len(lo), x.shape[1]
    s, a, n = np.zeros((nw, P)), np.zeros((nw, P)), np.zeros((nw, P), dtype=np.int64)
    for w in range(nw):
        if (pad_na is not None and pad_na[w]) or hi[w] <= lo[w]:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            s[w] = np.cumsum(x0[lo[w]:hi[w]], axis=0)[-1]  # cumsum adds one term after the other
            a[w] = np.abs(x0[lo[w]:hi[w]]).sum(axis=0)
        n[w] = ok[lo[w]:hi[w]].sum(axis=0)
    return s, n, a


def _mean(s, n, pad, min_loci):
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s / n
    mean[(n == 0) | (n < min_loci) | pad[:, None]] = np.nan
    return mean


def windows_ref(num, den, lo, hi, pad_na=None, min_loci=1):
    """the float route -> dict(fst, mean_num, mean_den, n_num, n_den (int32, -1 on a pad_na window), abs_num, abs_den)"""
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    pad = np.zeros(len(lo), dtype=bool) if pad_na is None else np.asarray(pad_na).astype(bool)
    sn, nn, an = window_sums(num, lo, hi, pad)
    sd, nd, ad = window_sums(den, lo, hi, pad)
    mn, md = _mean(sn, nn, pad, min_loci), _mean(sd, nd, pad, min_loci)
    with np.errstate(invalid="ignore", divide="ignore"):
        fst = mn / md
    nn, nd = nn.astype(np.int32), nd.astype(np.int32)
    nn[pad], nd[pad] = -1, -1
    return dict(fst=fst, mean_num=mn, mean_den=md, n_num=nn, n_den=nd, abs_num=an, abs_den=ad)


def sum_exact(x):
    """the exact route: the correctly rounded sum of the non-NaN doubles of x (math.fsum); +-Inf or NaN if they hold infinities"""
    x = np.asarray(x, dtype=np.float64)
    x = x[~np.isnan(x)]
    if not np.all(np.isfinite(x)):
        with np.errstate(invalid="ignore"):
            return float(np.sum(x[~np.isfinite(x)]))
    return math.fsum(x.tolist())


def sum_fraction(x):
    """the same as a Fraction (finite doubles only): no rounding at all"""
    x = np.asarray(x, dtype=np.float64)
    return sum((Fraction(float(v)) for v in x[~np.isnan(x)]), Fraction(0))


def pbs_one_triplet(f12, f13, f23):
    """R/nwise_pop_pbs.R:138-149 -> (pbs_1, pbs_2, pbs_3, pbsn1_1, pbsn1_2, pbsn1_3)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        t12, t13, t23 = -np.log(1 - f12), -np.log(1 - f13), -np.log(1 - f23)
        p1, p2, p3 = (t12 + t13 - t23) / 2, (t12 + t23 - t13) / 2, (t13 + t23 - t12) / 2
        tot = 1 + p1 + p2 + p3
        return p1, p2, p3, p1 / tot, p2 / tot, p3 / tot
