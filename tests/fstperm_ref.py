"""Fst under relabelings restated in Python from include/tpg.h "Fst under relabelings" (the reference has no permutation test;
the per-locus terms ARE the reference's, through the oracle).

  terms     per-locus num and den of one relabeling: oracle.pairwise_pop_fst(..., ind_row = the rows with label >= 0,
            return_num_dem = True), grouped by those labels.
  ordered   the sums in the defined order: kept terms of a unit of U loci in ascending order from 0.0, the unit sums of a span of
            S loci in ascending order from 0.0, the span sums in ascending order from 0.0.  U and S come from the library's
            accessors (or from the caller: the host tests give wrong ones on purpose).
  exact     the same kept doubles added as fractions.Fraction.
And the r-th relabeling, the p-value, a seeded panel and the stand-alone host program."""
from fractions import Fraction

import numpy as np

from oracle import oracle as orc

MISSING = 3
MASK = (1 << 64) - 1


def unit_span():
    from tidypopgen_amd import _lib

    return int(_lib.lib.tpg_fstperm_unit_loci()), int(_lib.lib.tpg_fstperm_span_loci())


# ---- the r-th relabeling ---------------------------------------------------------------------------------------------------
def mix64(x):
    """tpg_mix64 (csrc/synth_common.h) on a Python int"""
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def perm_labels(n, gid, ngroups, scheme, a, b, seed, r):
    gid = [int(g) for g in gid]
    assert len(gid) == n

    def label(g):
        return g if scheme == 1 else 0 if g == a else 1 if g == b else -1

    out = [label(g) for g in gid]
    if r == 0:
        return np.array(out, dtype=np.int32)
    E = [i for i in range(n) if out[i] >= 0]
    sigma = sorted(E, key=lambda i: (mix64((seed & MASK) ^ mix64(((r << 32) + i) & MASK)), i))
    for t, i in enumerate(sigma):
        out[i] = label(gid[E[t]])
    return np.array(out, dtype=np.int32)


def pvalue(obs, perm):
    """-> (p, n_valid) of one pair: plain Python"""
    fin = [x for x in perm if np.isfinite(x)]
    if not np.isfinite(obs):
        return float("nan"), len(fin)
    return (1 + sum(1 for x in fin if x >= obs)) / (1 + len(fin)), len(fin)


# ---- panel -----------------------------------------------------------------------------------------------------------------
def panel(seed, n, m, miss=0.1):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, size=m)
    codes = rng.binomial(2, np.broadcast_to(p, (n, m))).astype(np.uint8)
    codes[rng.random((n, m)) < miss] = MISSING
    return np.asfortranarray(codes)


def label_rows(seed, n, G, R):
    """R label rows of n individuals in G groups: row 0 labels everybody; rows 1, 5, 9 ... put a fifth of the individuals outside
    (-1); row 2 leaves group G - 1 empty; row 3 gives group 0 exactly one individual"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, G, size=(R, n)).astype(np.int32)
    for r in range(1, R, 4):
        lab[r, rng.random(n) < 0.2] = -1
    if R > 2:
        lab[2, lab[2] == G - 1] = rng.integers(0, G - 1, size=int((lab[2] == G - 1).sum()))
    if R > 3:
        lab[3, lab[3] == 0] = 1
        lab[3, int(rng.integers(0, n))] = 0
    return lab


def pair_cols(G, pairs):
    """columns of utils::combn(G, 2) that hold the pairs (2 x P, 1-based, g1 < g2)"""
    pairs = np.asarray(pairs).reshape(2, -1)
    col = {}
    k = 0
    for a in range(1, G + 1):
        for b in range(a + 1, G + 1):
            col[(a, b)] = k
            k += 1
    return np.array([col[(int(a), int(b))] for a, b in pairs.T], dtype=np.int64)


# ---- terms and sums ----------------------------------------------------------------------------------------------------------
def terms(codes, label_row, G, method):
    """-> num, den (m x P_all, the columns of combn(G, 2)) of one relabeling"""
    label_row = np.asarray(label_row)
    rows = np.flatnonzero(label_row >= 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        nd = orc.pairwise_pop_fst(codes, (rows + 1).astype(np.int32), None, label_row[rows].astype(np.int32), G, method=method,
                                  return_num_dem=True)
    return np.asarray(nd["Fst_by_locus_num"]), np.asarray(nd["Fst_by_locus_den"])


def ordered_sums(num, den, U, S, keep_on_num_alone=False):
    """num, den: m x P doubles -> sum_num, sum_den (P), n_kept (P int64) in the defined order.  keep_on_num_alone: the WRONG
    rule that looks at num alone when it decides whether num is added (the host tests show that it changes bits)"""
    m, P = num.shape
    kept = ~np.isnan(num) & ~np.isnan(den)
    kept_n = ~np.isnan(num) if keep_on_num_alone else kept
    tot_n, tot_d = np.zeros(P), np.zeros(P)
    for s0 in range(0, m, S):
        sp_n, sp_d = np.zeros(P), np.zeros(P)
        for u0 in range(s0, min(s0 + S, m), U):
            un, ud = np.zeros(P), np.zeros(P)
            for j in range(u0, min(u0 + U, m)):
                un = np.where(kept_n[j], un + np.where(kept_n[j], num[j], 0.0), un)
                ud = np.where(kept[j], ud + np.where(kept[j], den[j], 0.0), ud)
            sp_n, sp_d = sp_n + un, sp_d + ud
        tot_n, tot_d = tot_n + sp_n, tot_d + sp_d
    return tot_n, tot_d, kept.sum(axis=0).astype(np.int64)


def exact_sums(num, den):
    """the kept doubles added exactly -> lists of Fraction (P each), and sum |x| as Fractions"""
    m, P = num.shape
    kept = ~np.isnan(num) & ~np.isnan(den)
    out = []
    for x in (num, den):
        s = [sum((Fraction(float(x[j, k])) for j in range(m) if kept[j, k]), Fraction(0)) for k in range(P)]
        a = [sum((abs(Fraction(float(x[j, k]))) for j in range(m) if kept[j, k]), Fraction(0)) for k in range(P)]
        out += [s, a]
    return out  # sum_num, abs_num, sum_den, abs_den


def reference(codes, labels, G, pairs, method, U=None, S=None):
    """-> sum_num, sum_den (R x P), n_kept (R x P int64), fst (R x P) of the label rows"""
    if U is None:
        U, S = unit_span()
    labels = np.asarray(labels).reshape(-1, codes.shape[0])
    cols = pair_cols(G, pairs)
    R, P = labels.shape[0], len(cols)
    sn, sd, nk = np.zeros((R, P)), np.zeros((R, P)), np.zeros((R, P), dtype=np.int64)
    for r in range(R):
        num, den = terms(codes, labels[r], G, method)
        sn[r], sd[r], nk[r] = ordered_sums(num[:, cols], den[:, cols], U, S)
    with np.errstate(invalid="ignore", divide="ignore"):
        return sn, sd, nk, sn / sd


def perm_test(codes, gid, G, method, n_perm, seed, pairs=None):
    """pairwise_pop_fst_test(scheme = "pairwise") by the reference alone -> fst (1 + n_perm, P), p, n_valid"""
    n = codes.shape[0]
    pairs = np.array([(a, b) for a in range(1, G + 1) for b in range(a + 1, G + 1)]).T if pairs is None else np.asarray(pairs).reshape(2, -1)
    P = pairs.shape[1]
    fst = np.zeros((1 + n_perm, P))
    one = np.array([[1], [2]])
    for k in range(P):
        lab = np.stack([perm_labels(n, gid, G, 0, int(pairs[0, k]) - 1, int(pairs[1, k]) - 1, seed, r) for r in range(1 + n_perm)])
        fst[:, k] = reference(codes, lab, 2, one, method)[3][:, 0]
    pv = [pvalue(fst[0, k], fst[1:, k]) for k in range(P)]
    return fst, np.array([p for p, _ in pv]), np.array([c for _, c in pv], dtype=np.int64)


def test_panel(seed=5):
    """60 individuals x 600 loci: groups 0 and 1 diverged from each other and from the rest, groups 2 and 3 one population split at
    random in two.  -> codes, gid"""
    rng = np.random.default_rng(seed)
    n, m = 60, 600
    pop = np.repeat([0, 1, 2], [15, 15, 30])
    base = rng.uniform(0.1, 0.9, size=m)
    pp = np.clip(base[None, :] + rng.normal(0, 0.25, size=(3, m)), 0.02, 0.98)
    codes = rng.binomial(2, pp[pop]).astype(np.uint8)
    codes[rng.random((n, m)) < 0.05] = MISSING
    gid = pop.copy()
    third = np.flatnonzero(pop == 2)
    gid[rng.permutation(third)[:15]] = 3
    return np.asfortranarray(codes), gid.astype(np.int32)


test_panel.__test__ = False  # (a builder, not a test)


# ---- the host pieces as a stand-alone program --------------------------------------------------------------------------------
def build_host_program(exe, sanitize=True):
    """tests/host/fstperm_san.cpp (csrc/host/host_fstperm.h on the host) -> exe"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    san = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", *san, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-function",
           "-I" + os.path.join(root, "tidypopgen_amd", "csrc"), os.path.join(root, "tests", "host", "fstperm_san.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_host_program(exe, path, queries):
    """one list of integers per query (see tests/host/fstperm_san.cpp) -> one list of integers per query"""
    import subprocess

    with open(path, "w") as fh:
        fh.write("\n".join(" ".join(str(int(x)) for x in q) for q in queries) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stderr[-4000:])
    rows = [[int(w) for w in line.split()] for line in out.stdout.splitlines()]
    assert len(rows) == len(queries)
    return rows
