"""AMOVA restated in Python from include/tpg.h "AMOVA" (the reference has no AMOVA: the header is the definition).

  sqdist         the squared distance from the genotype codes in integers (not from the accumulators), raw and adjusted.
  ordered        the class sums in the defined order: the included entries of row i over a chunk of C columns in ascending j from
                 0.0, the chunk partials in ascending order from 0.0, the rows of a class in ascending i from 0.0.  C comes from the
                 library's getter (or from the caller).  fault = one of FAULTS gives a WRONG sum on purpose: the host tests show
                 that the panels of the GPU test tell every one of them from the right one.
  exact          the same entries added as Python integers / fractions.Fraction.
  perm_labels    the r-th relabeling of the three schemes.
  from_sums      the finisher statement by statement in float64; from_sums_exact the same formulas in Fractions.
  amova          gt_amova by these pieces alone.
And the panels of the GPU test and the stand-alone host program."""
import os
import re
from fractions import Fraction

import numpy as np

MASK = (1 << 64) - 1
MISSING = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def constants():
    """-> chunk columns C, tile rows, batch B (the library's getters: host only), TPG_CLASSSUM_MAX_CLASSES (the header)"""
    from tidypopgen_amd import _lib

    txt = open(os.path.join(ROOT, "include", "tpg.h")).read()
    mx = int(re.search(r"#define TPG_CLASSSUM_MAX_CLASSES (\d+)", txt).group(1))
    return int(_lib.lib.tpg_classsum_chunk()), int(_lib.lib.tpg_classsum_tile_rows()), int(_lib.lib.tpg_classsum_batch()), mx


# ---- squared distance --------------------------------------------------------------------------------------------------------
def sqdist(codes, m=None):
    """codes: n x L uint8 (0, 1, 2, 3 = missing) -> raw (int64), V (int64), adjusted = (raw * m) / V as the header states it"""
    codes = np.asarray(codes)
    v = (codes != MISSING).astype(np.int64)
    d = (codes.astype(np.int64) - 1) * v
    s = (d * d) @ v.T  # s_ij = sum over the loci j is typed at of d_i^2 (d is 0 where i is not typed)
    raw = s + s.T - 2 * (d @ d.T)
    V = v @ v.T
    m = codes.shape[1] if m is None else m
    with np.errstate(invalid="ignore", divide="ignore"):
        adj = np.where(V == 0, np.nan, (raw * np.int64(m)).astype(np.float64) / V.astype(np.float64))
    return raw, V, adj


# ---- class sums --------------------------------------------------------------------------------------------------------------
FAULTS = ("swap_ij", "drop_diagonal", "chunks_descending", "minus_one_is_a_class", "skip_ragged_chunk", "skip_ragged_tile")


def ordered_class_sums(A, labels, nclasses, C, fault=None, tile_rows=None):
    """A: n x n doubles, labels: R x n -> (R, nclasses) doubles in the defined order"""
    A = np.asarray(A, dtype=np.float64)
    lab = np.asarray(labels, dtype=np.int64).reshape(-1, A.shape[0])
    R, n = lab.shape
    if fault == "swap_ij":
        A = A.T
    inside = lab >= 0
    if fault == "minus_one_is_a_class":
        inside = np.ones_like(inside)
    t = np.zeros((R, n))
    chunks = list(range(0, n, C))
    if fault == "skip_ragged_chunk" and n % C:
        chunks = chunks[:-1]
    if fault == "chunks_descending":
        chunks = chunks[::-1]
    for j0 in chunks:
        p = np.zeros((R, n))
        for j in range(j0, min(j0 + C, n)):
            inc = inside & (lab == lab[:, j:j + 1])  # (the label of column j is >= 0 whenever it equals an inside row's)
            if fault == "drop_diagonal":
                inc[:, j] = False
            p = p + np.where(inc, A[None, :, j], 0.0)  # adding +0.0 leaves a sum that started at +0.0 as it is
        t = t + p
    if fault == "skip_ragged_tile" and n % tile_rows:
        t[:, n - n % tile_rows:] = 0.0
    sums = np.zeros((R, nclasses))
    for i in range(n):
        rows = np.flatnonzero(inside[:, i])
        cls = lab[rows, i] if fault != "minus_one_is_a_class" else np.maximum(lab[rows, i], 0)
        sums[rows, cls] = sums[rows, cls] + t[rows, i]
    return sums


def exact_class_sums(A, label_row, nclasses):
    """one label row -> per class: the exact sum (Fraction, or None when a NaN is among its terms), sum |x| and the number of terms"""
    A = np.asarray(A, dtype=np.float64)
    lab = np.asarray(label_row)
    out = []
    for c in range(nclasses):
        idx = np.flatnonzero(lab == c)
        x = A[np.ix_(idx, idx)].ravel()
        if np.isnan(x).any():
            out.append((None, None, len(x)))
            continue
        out.append((sum((Fraction(float(v)) for v in x), Fraction(0)), sum((abs(Fraction(float(v))) for v in x), Fraction(0)), len(x)))
    return out


# ---- panels of the GPU test (built here so that the host tests can show that they catch every fault) -----------------------------
def matrix(kind, n, seed):
    """"int": asymmetric integers in [0, 1000); "real": asymmetric doubles of mixed sign and magnitude; "nan": "real" with one NaN
    off the diagonal, at (n // 3, n - 2)"""
    rng = np.random.default_rng(seed)
    if kind == "int":
        return np.asfortranarray(rng.integers(0, 1000, size=(n, n)).astype(np.float64))
    A = rng.normal(size=(n, n)) * np.exp(rng.uniform(-6, 6, size=(n, n)))
    if kind == "nan":
        A[n // 3, n - 2] = np.nan
    return np.asfortranarray(A)


def label_rows(seed, n, nclasses, R):
    """R label rows: row 0 random with a fifth of the individuals outside (-1), as rows 4, 8, ...; row 1 puts everybody into one
    class; row 2 leaves class nclasses - 1 empty; row 3 gives class 0 exactly one individual; the others are random"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, nclasses, size=(R, n)).astype(np.int32)
    for r in range(0, R, 4):
        lab[r, rng.random(n) < 0.2] = -1
    if R > 1:
        lab[1, :] = nclasses // 2
    if R > 2 and nclasses > 1:
        lab[2, lab[2] == nclasses - 1] = 0
    if R > 3 and nclasses > 1:
        lab[3, lab[3] == 0] = 1
        lab[3, int(rng.integers(0, n))] = 0
    return lab


# ---- the r-th relabeling -------------------------------------------------------------------------------------------------------
def mix64(x):
    """tpg_mix64 (csrc/synth_common.h) on a Python int"""
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def perm_labels(n, pop, npop, region_of_pop, nregion, scheme, seed, r):
    """-> pop_out (n int32), region_of_pop_out (npop int32, or None without regions)"""
    pop = [int(p) for p in pop]
    reg = [int(g) for g in region_of_pop] if nregion else None
    assert len(pop) == n
    pop_out, reg_out = list(pop), (list(reg) if nregion else None)

    def shuffle(E, src, dst):
        sigma = sorted(E, key=lambda u: (mix64((seed & MASK) ^ mix64(((r << 32) + u) & MASK)), u))
        for t, u in enumerate(sigma):
            dst[u] = src[E[t]]

    if r > 0:
        if scheme == 0:
            shuffle([i for i in range(n) if pop[i] >= 0], pop, pop_out)
        elif scheme == 1:
            for g in range(nregion):
                shuffle([i for i in range(n) if pop[i] >= 0 and reg[pop[i]] == g], pop, pop_out)
        else:
            shuffle(list(range(npop)), reg, reg_out)
    return np.array(pop_out, dtype=np.int32), (np.array(reg_out, dtype=np.int32) if nregion else None)


# ---- the finisher --------------------------------------------------------------------------------------------------------------
def from_sums(pop_size, pop_sum, total_sum, region_of_pop=None, region_sum=None):
    """include/tpg.h "AMOVA", tpg_amova_from_sums, one float64 statement after the other -> dict as tidypopgen_amd.amova_from_sums"""
    f = np.float64
    nan = f("nan")
    size = [int(x) for x in pop_size]
    P, N, sq = len(size), sum(size), sum(x * x for x in size)
    Nd = f(N)

    def over(x, d):
        return x / f(d) if d > 0 else nan

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ssd_t = f(total_sum) / (f(2.0) * Nd)
        ssd_wp = f(0.0)
        for p in range(P):
            ssd_wp = ssd_wp + f(pop_sum[p]) / (f(2.0) * f(size[p]))
        if region_of_pop is not None:
            reg = [int(g) for g in region_of_pop]
            G = len(region_sum)
            Ng = [sum(size[p] for p in range(P) if reg[p] == g) for g in range(G)]
            ssd_wr = f(0.0)
            for g in range(G):
                ssd_wr = ssd_wr + f(region_sum[g]) / (f(2.0) * f(Ng[g]))
            S1 = f(0.0)
            for p in range(P):
                S1 = S1 + f(size[p] * size[p]) / f(Ng[reg[p]])
            sqg = sum(x * x for x in Ng)
            d0, d1, d2 = G - 1, P - G, N - P
            df = [f(d0), f(d1), f(d2), f(N - 1)]
            ssd = [ssd_t - ssd_wr, ssd_wr - ssd_wp, ssd_wp, ssd_t]
            msd = [over(ssd[0], d0), over(ssd[1], d1), over(ssd[2], d2)]
            nc = [over(Nd - S1, d1), over(S1 - f(sq) / Nd, d0), over(Nd - f(sqg) / Nd, d0)]
            sc = msd[2]
            sb = (msd[1] - sc) / nc[0]
            t = msd[0] - sc
            t = t - nc[1] * sb
            sa = t / nc[2]
            sab = sa + sb
            st = sab + sc
            s2 = [sa, sb, sc, st]
            phi = [sa / st, sb / (sb + sc), sab / st]
        else:
            d1, d2 = P - 1, N - P
            df = [nan, f(d1), f(d2), f(N - 1)]
            ssd = [nan, ssd_t - ssd_wp, ssd_wp, ssd_t]
            msd = [nan, over(ssd[1], d1), over(ssd[2], d2)]
            nc = [over(Nd - f(sq) / Nd, d1), nan, nan]
            sc = msd[2]
            sb = (msd[1] - sc) / nc[0]
            st = sb + sc
            s2 = [nan, sb, sc, st]
            phi = [nan, nan, sb / st]
    return dict(df=np.array(df), ssd=np.array(ssd), msd=np.array(msd), ncoef=np.array(nc), sigma2=np.array(s2), phi=np.array(phi))


def from_sums_exact(pop_size, pop_sum, total_sum, region_of_pop=None, nregion=0, region_sum=None):
    """the same formulas in Fractions (every df positive) -> (sigma2_a or None, sigma2_b, sigma2_c), ssd (list)"""
    F = Fraction
    size = [int(x) for x in pop_size]
    P, N = len(size), sum(size)
    ssd_t = F(total_sum) / (2 * N)
    ssd_wp = sum(F(pop_sum[p]) / (2 * size[p]) for p in range(P))
    if region_of_pop is None:
        n0 = (N - F(sum(x * x for x in size), N)) / (P - 1)
        sc = ssd_wp / (N - P)
        sb = ((ssd_t - ssd_wp) / (P - 1) - sc) / n0
        return (None, sb, sc), [None, ssd_t - ssd_wp, ssd_wp, ssd_t]
    reg, G = [int(g) for g in region_of_pop], nregion
    Ng = [sum(size[p] for p in range(P) if reg[p] == g) for g in range(G)]
    ssd_wr = sum(F(region_sum[g]) / (2 * Ng[g]) for g in range(G))
    S1 = sum(F(size[p] * size[p], Ng[reg[p]]) for p in range(P))
    n = (N - S1) / (P - G)
    n1 = (S1 - F(sum(x * x for x in size), N)) / (G - 1)
    n2 = (N - F(sum(x * x for x in Ng), N)) / (G - 1)
    sc = ssd_wp / (N - P)
    sb = ((ssd_wr - ssd_wp) / (P - G) - sc) / n
    sa = ((ssd_t - ssd_wr) / (G - 1) - sc - n1 * sb) / n2
    return (sa, sb, sc), [ssd_t - ssd_wr, ssd_wr - ssd_wp, ssd_wp, ssd_t]


def class_sums_int(A, label_row, nclasses):
    """exact integer class sums of an integer-valued matrix (Python ints)"""
    lab = np.asarray(label_row)
    Ai = np.asarray(A).astype(object)
    return [int(Ai[np.ix_(np.flatnonzero(lab == c), np.flatnonzero(lab == c))].sum()) if (lab == c).any() else 0 for c in range(nclasses)]


# ---- the p-value and the driver ------------------------------------------------------------------------------------------------
def pvalue(obs, perm):
    fin = [x for x in perm if np.isfinite(x)]
    if not np.isfinite(obs):
        return float("nan"), len(fin)
    return (1 + sum(1 for x in fin if x >= obs)) / (1 + len(fin)), len(fin)


def amova(dist, pop, npop, region_of_pop, n_perm, seed, C):
    """gt_amova by the pieces above -> dict(obs = from_sums of the identity, phi, p_value, n_valid, perm = {scheme: dict(phi, sigma2)})"""
    dist = np.asarray(dist, dtype=np.float64)
    n = dist.shape[0]
    pop = np.asarray(pop, dtype=np.int32)
    reg = None if region_of_pop is None else np.asarray(region_of_pop, dtype=np.int32)
    G = 0 if reg is None else int(reg.max()) + 1
    size = np.bincount(pop[pop >= 0], minlength=npop)

    def induced(p, g):
        return np.where(p >= 0, g[np.maximum(p, 0)], -1)

    def one(p, g):
        T = ordered_class_sums(dist, np.where(pop >= 0, 0, -1), 1, C)[0, 0]
        W = ordered_class_sums(dist, p, npop, C)[0]
        Rg = ordered_class_sums(dist, induced(p, g), G, C)[0] if G else None
        return from_sums(size, W, T, g, Rg)

    obs = one(pop, reg)
    col = {"CT": 0, "SC": 1, "ST": 2}
    perm, p_value, n_valid = {}, np.full(3, np.nan), np.zeros(3, dtype=np.int64)
    for name, scheme in (("ST", 0), ("SC", 1), ("CT", 2)) if G else (("ST", 0),):
        rows = [one(*perm_labels(n, pop, npop, reg, G, scheme, seed, r)) for r in range(1, n_perm + 1)]
        perm[name] = dict(phi=np.stack([x["phi"] for x in rows]), sigma2=np.stack([x["sigma2"] for x in rows]))
        p_value[col[name]], n_valid[col[name]] = pvalue(obs["phi"][col[name]], perm[name]["phi"][:, col[name]])
    return dict(obs=obs, phi=obs["phi"], p_value=p_value, n_valid=n_valid, perm=perm)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_values(a, b):
    """the same bits, except that every NaN equals every NaN (the payload of a NaN is not part of the definition)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


# ---- the host pieces as a stand-alone program --------------------------------------------------------------------------------
def bits(x):
    return int(np.array(x, dtype=np.float64).view(np.int64))


def from_bits(b):
    return float(np.array(b, dtype=np.int64).view(np.float64))


def build_host_program(exe, sanitize=True):
    """tests/host/amova_san.cpp (csrc/host/host_amova.h on the host) -> exe"""
    import subprocess

    san = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", *san, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-function",
           "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc"), os.path.join(ROOT, "tests", "host", "amova_san.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_host_program(exe, path, queries):
    """one list of integers per query (see tests/host/amova_san.cpp) -> one list of integers per query"""
    import subprocess

    with open(path, "w") as fh:
        fh.write("\n".join(" ".join(str(int(x)) for x in q) for q in queries) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stderr[-4000:])
    rows = [[int(w) for w in line.split()] for line in out.stdout.splitlines()]
    assert len(rows) == len(queries)
    return rows
