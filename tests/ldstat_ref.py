"""numpy restatement of include/tpg.h "LD statistics" on tests/ld_ref.py's sums and window: dense rows, int64 sums, r2 as three
np.float64 operations in the stated order, q = floor(r2 * 2^30 + 0.5), uint64 sums, integer bins -- and a second, independent
route for small panels: r2 as an exact Fraction and q from it in integers."""
import os
import subprocess
from fractions import Fraction

import numpy as np

from tests import ld_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q_ONE = 1 << 30
MAX_BINS = 4096
STAT_KEYS = ("score_q", "n_partners", "bin_pairs", "bin_sum_q", "bin_sum_dist")


def q_of(r2):
    """the fixed-point value of an array of r2"""
    return np.floor(np.asarray(r2, dtype=np.float64) * np.float64(Q_ONE) + np.float64(0.5)).astype(np.uint64)


def rows(G, hi):
    """for every locus j: (ks = j + 1 .. hi[j], r2 of (j, k) as float64 with NaN for a pair that is not valid)"""
    G = np.asarray(G)
    n, sx, d = ld_ref.sums(G)
    dd = d.astype(np.float64)
    g = G.astype(np.int64)
    for j in range(G.shape[1]):
        ks = np.arange(j + 1, int(hi[j]) + 1)
        if len(ks) == 0:
            yield j, ks, np.zeros(0)
            continue
        sxy = g[:, j] @ g[:, ks]
        dn = (n * sxy - sx[j] * sx[ks]).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            r2 = (dn * dn) / (dd[j] * dd[ks])
        r2[~((d[j] > 0) & (d[ks] > 0))] = np.nan
        yield j, ks, r2


def band_tiles(hi):
    """32 x 32 tiles of the band: per row tile, its own tile up to the tile of the last neighbour of its last locus"""
    hi = np.asarray(hi, dtype=np.int64)
    m = len(hi)
    if int((hi - np.arange(m)).max(initial=0)) == 0:
        return 0
    last = np.minimum(np.arange(31, m + 31, 32), m - 1)
    return int(((hi[last] >> 5) - (last >> 5) + 1).sum())


def stats(G, hi, pos=None, bin_size=1, nbins=0):
    """tpg_ld_stats: score_q, n_partners, and with nbins > 0 the three bin arrays; report"""
    G = np.asarray(G)
    m = G.shape[1]
    hi = np.asarray(hi, dtype=np.int64)
    score = np.zeros(m, dtype=np.uint64)
    partners = np.zeros(m, dtype=np.int32)
    bp, bq, bd = np.zeros(nbins, dtype=np.int64), np.zeros(nbins, dtype=np.uint64), np.zeros(nbins, dtype=np.int64)
    p = np.arange(m, dtype=np.int64) if pos is None else np.asarray(pos, dtype=np.int64)
    valid = beyond = 0
    for j, ks, r2 in rows(G, hi):
        ok = ~np.isnan(r2)
        if not ok.any():
            continue
        ks, q = ks[ok], q_of(r2[ok])
        valid += len(ks)
        score[j] += q.sum(dtype=np.uint64)
        partners[j] += len(ks)
        score[ks] += q  # (ks are distinct)
        partners[ks] += 1
        if nbins > 0:
            dist = p[ks] - p[j]
            assert (dist >= 0).all()
            b = dist // np.int64(bin_size)
            inside = b < nbins
            beyond += int((~inside).sum())
            np.add.at(bp, b[inside], 1)
            np.add.at(bq, b[inside], q[inside])
            np.add.at(bd, b[inside], dist[inside])
    out = dict(score_q=score, n_partners=partners,
               report=dict(pairs=int((hi - np.arange(m)).sum()), pairs_valid=valid, pairs_beyond=beyond, band_tiles=band_tiles(hi)))
    if nbins > 0:
        out.update(bin_pairs=bp, bin_sum_q=bq, bin_sum_dist=bd)
    return out


def equal_stats(a, b):
    """every array the two results share to equality, bit for bit, and the reports"""
    for k in STAT_KEYS:
        if (k in a) != (k in b):
            return False
        if k in a and not (a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k])):
            return False
    return a["report"] == b["report"]


def same_bits(x, y):
    """two float64 arrays to the bit, every NaN counted as the same NaN"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.shape != y.shape or not np.array_equal(np.isnan(x), np.isnan(y)):
        return False
    ok = ~np.isnan(x)
    return np.array_equal(x[ok].view(np.uint64), y[ok].view(np.uint64))


def band_r2(G, hi, j0, j1, stride=None):
    """tpg_ld_band_r2: (j1 - j0, stride), entry [j - j0, b] = r2 of (j, j + 1 + b), NaN elsewhere"""
    hi = np.asarray(hi, dtype=np.int64)
    if stride is None:
        stride = max(1, int((hi[j0:j1] - np.arange(j0, j1)).max()))
    out = np.full((j1 - j0, stride), np.nan)
    for j, ks, r2 in rows(G, hi):
        if j0 <= j < j1:
            out[j - j0, :len(ks)] = r2
    return out


def region_r2(G, j0, j1):
    """the symmetric matrix of ld_region_r2: diagonal 1, NaN in the row and column of a monomorphic locus"""
    sub = np.asarray(G)[:, j0:j1]
    r = sub.shape[1]
    _, _, d = ld_ref.sums(sub)
    out = np.full((r, r), np.nan)
    for j, ks, r2 in rows(sub, np.full(r, r - 1, dtype=np.int64)):
        out[j, ks] = r2
        out[ks, j] = r2
        out[j, j] = 1.0 if d[j] > 0 else np.nan
    return out


def ld_score(G, hi, adjusted=True, include_self=True, s=None):
    """loci_ld_score from stats(G, hi) (s: that result, where the caller has it)"""
    G = np.asarray(G)
    n = G.shape[0]
    s = stats(G, hi) if s is None else s
    S, c = s["score_q"].astype(np.float64) / Q_ONE, s["n_partners"].astype(np.float64)
    out = S - (c - S) / (n - 2) if adjusted else S
    if include_self:
        out = out + 1.0
    out[ld_ref.sums(G)[2] == 0] = np.nan
    return out


def decay(G, hi, pos, bin_size, nbins, adjusted=False):
    G = np.asarray(G)
    s = stats(G, hi, pos, bin_size, nbins)
    npairs = s["bin_pairs"]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_r2 = np.where(npairs > 0, s["bin_sum_q"].astype(np.float64) / Q_ONE / npairs, np.nan)
        mean_dist = np.where(npairs > 0, s["bin_sum_dist"].astype(np.float64) / npairs, np.nan)
    if adjusted:
        mean_r2 = mean_r2 - (1.0 - mean_r2) / (G.shape[0] - 2)
    lo = np.arange(nbins, dtype=np.int64) * bin_size
    return dict(distance_lo=lo, distance_hi=lo + bin_size, mean_distance=mean_dist, n_pairs=npairs, mean_r2=mean_r2,
                pairs_beyond=s["report"]["pairs_beyond"])


# ---- the exact route --------------------------------------------------------------------------------------------------
def exact_rows(G, hi):
    """for every locus j: (ks, [r2 of (j, k) as a Fraction, or None for a pair that is not valid]) in Python integers"""
    G = np.asarray(G)
    n, m = G.shape
    cols = [[int(x) for x in G[:, j]] for j in range(m)]
    sx = [sum(c) for c in cols]
    d = [n * sum(x * x for x in c) - s * s for c, s in zip(cols, sx)]
    for j in range(m):
        ks = list(range(j + 1, int(hi[j]) + 1))
        out = []
        for k in ks:
            if d[j] > 0 and d[k] > 0:
                num = n * sum(x * y for x, y in zip(cols[j], cols[k])) - sx[j] * sx[k]
                out.append(Fraction(num * num, d[j] * d[k]))
            else:
                out.append(None)
        yield j, ks, out


def exact_q(r2: Fraction):
    """(floor(r2 2^30 + 1/2), the distance of r2 2^30 from the nearest half-integer) in exact arithmetic"""
    x = r2 * Q_ONE
    q = (x + Fraction(1, 2)).__floor__()
    frac = x - x.__floor__()
    return q, abs(frac - Fraction(1, 2))


# ---- the host program -------------------------------------------------------------------------------------------------
def build_host_program(exe, sanitize=True):
    """tests/host/ldstat_san.cpp (csrc/host/host_ldstat.h on the host) -> exe"""
    san = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", *san, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-function",
           "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc"), os.path.join(ROOT, "tests", "host", "ldstat_san.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_host_program(exe, path, lines):
    """one query per line ("R n sxy sxj sxk dj dk" or "B dist bin_size nbins") -> the output lines, split into integers"""
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return [[int(x) for x in line.split()] for line in out.stdout.splitlines()]
