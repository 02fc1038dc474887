"""Mantel tests restated in Python from include/tpg.h "Mantel tests" (the reference has no Mantel test: the header is the
definition; it is recalled from Mantel 1967, Smouse, Long & Sokal 1986 and vegan's mantel / mantel.partial, not pinned by a run of
vegan).

  ordered_sums   the cross sums in the defined order: per column j the L strided partials in ascending i from +0.0, every product
                 rounded before it is added, i = j skipped; the tree h = L/2 .. 1; the column terms in ascending j from +0.0.  L
                 comes from the library's getter (or from the caller).  fault = one of FAULTS gives a WRONG sum on purpose: the
                 host tests show that the panels of the GPU test tell every one of them from the right one.
  exact_sums     the same products added as Python integers / fractions.Fraction.
  perms          the permutation rule, within strata or not.
  from_sums, partial   the finishers statement by statement in float64; *_exact the same formulas in Fractions.
  moments, center, midranks, mantel   gt_mantel by these pieces alone.
And the panels of the GPU test and the stand-alone host program."""
import os
from fractions import Fraction

import numpy as np

from tests.amova_ref import bits, from_bits, mix64, pvalue, same_bits, same_values  # noqa: F401  (one rule, one restatement)

MASK = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lanes():
    """L = TPG_MANTEL_LANES from the library's getter (host only)"""
    from tidypopgen_amd import _lib

    return int(_lib.lib.tpg_mantel_lanes())


# ---- the ordered sum -----------------------------------------------------------------------------------------------------------
FAULTS = ("swap_ij", "rows_only", "inverse_perm", "with_diagonal", "tree_ascending", "contiguous_partials", "skip_ragged_stride",
          "fused_product", "columns_descending")


def _round_fraction(x):
    """a Fraction -> the nearest double, ties to even (Python's int / int division is correctly rounded)"""
    return x.numerator / x.denominator


def _column_terms(P, L, fault=None, fused=None):
    """P: n x n rounded products with +0.0 where a term is skipped -> the n column terms.  (A partial starts at +0.0 and can never
    become -0.0, so adding +0.0 is the same as skipping.)  fused = (X, Bq): the unrounded factors for the "fused_product" fault."""
    n = P.shape[0]
    K = -(-n // L)
    if fault == "skip_ragged_stride" and n % L:
        K -= 1
    pad = np.zeros((max(K, 0) * L, n))
    rows = min(n, K * L)
    pad[:rows] = P[:rows]
    if fault == "contiguous_partials":  # partial t takes the K consecutive rows t K .. t K + K - 1
        blocks = pad.reshape(L, K, n).transpose(1, 0, 2)
    else:
        blocks = pad.reshape(K, L, n)
    s = np.zeros((L, n))
    if fault == "fused_product":  # s = round(s + x * b) with the product exact: one rounding where the definition has two
        X, Bq = fused
        for k in range(K):
            for t in range(min(L, n - k * L)):
                i = k * L + t
                for j in range(n):
                    if i != j:
                        s[t, j] = _round_fraction(Fraction(float(s[t, j])) + Fraction(float(X[i, j])) * Fraction(float(Bq[i, j])))
    else:
        for k in range(K):
            s = s + blocks[k]
    hs = [L >> (b + 1) for b in range(L.bit_length() - 1)]  # L/2, L/4, .., 1
    if fault == "tree_ascending":
        hs = hs[::-1]
    for h in hs:
        s = s.copy()
        s[:h] = s[:h] + s[h:2 * h]
    return s[0]


def ordered_sums(A, Bs, perms, L, fault=None):
    """A: n x n doubles, Bs: a list of Q n x n doubles, perms: R x n -> (R, Q) doubles in the defined order"""
    A = np.asarray(A, dtype=np.float64)
    Bs = [np.asarray(B, dtype=np.float64) for B in Bs]
    n = A.shape[0]
    perms = np.asarray(perms, dtype=np.int64).reshape(-1, n)
    out = np.zeros((len(perms), len(Bs)))
    off = ~np.eye(n, dtype=bool)
    for r, p in enumerate(perms):
        if fault == "inverse_perm":
            p = np.argsort(p)
        if fault == "rows_only":
            X = A[p, :]
        elif fault == "swap_ij":
            X = A[np.ix_(p, p)].T
        else:
            X = A[np.ix_(p, p)]  # X[i, j] = A[p[i], p[j]]
        for q, B in enumerate(Bs):
            with np.errstate(invalid="ignore", over="ignore"):
                P = X * B
                if fault != "with_diagonal":
                    P = np.where(off, P, 0.0)
                c = _column_terms(P, L, fault, fused=(X, B))
                if fault == "columns_descending":
                    c = c[::-1]
                out[r, q] = np.cumsum(np.concatenate(([0.0], c)))[-1]  # (cumsum adds one term after the other)
    return out


def exact_sums(A, B, perm):
    """one permutation -> (the exact sum of the ROUNDED products as a Fraction, sum |product|, the number of terms), and the exact
    sum of the unrounded products"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    n = A.shape[0]
    p = np.asarray(perm, dtype=np.int64)
    X = A[np.ix_(p, p)]
    P = X * B
    tot, ab, raw = Fraction(0), Fraction(0), Fraction(0)
    for i in range(n):
        for j in range(n):
            if i != j:
                tot += Fraction(float(P[i, j]))
                ab += abs(Fraction(float(P[i, j])))
                raw += Fraction(float(X[i, j])) * Fraction(float(B[i, j]))
    return (tot, ab, n * (n - 1)), raw


def int_sums(A, B, perm):
    """the exact cross sum of two integer-valued matrices (a Python int)"""
    p = np.asarray(perm, dtype=np.int64)
    X = np.asarray(A)[np.ix_(p, p)].astype(np.int64)
    P = X * np.asarray(B).astype(np.int64)
    return int(P.sum() - np.trace(P))


# ---- panels of the GPU test (built here so that the host tests can show that they catch every fault) -----------------------------
def matrix(kind, n, seed):
    """"int": non-symmetric integers with |a| <= 2^10; "real": non-symmetric doubles of mixed sign and magnitude.  The diagonal
    holds values like any other entry: it must not be read"""
    rng = np.random.default_rng(seed)
    if kind == "int":
        return np.asfortranarray(rng.integers(-1024, 1025, size=(n, n)).astype(np.float64))
    return np.asfortranarray(rng.normal(size=(n, n)) * np.exp(rng.uniform(-6, 6, size=(n, n))))


def perm_rows(seed, n, R):
    """R permutations: row 0 the identity, row 1 the reversal, the others random"""
    rng = np.random.default_rng(seed)
    rows = [np.arange(n), np.arange(n)[::-1]] + [rng.permutation(n) for _ in range(max(R - 2, 0))]
    return np.ascontiguousarray(np.stack(rows[:R]), dtype=np.int32)


# ---- the permutation rule ------------------------------------------------------------------------------------------------------
def perms(n, seed, r0, R, strata=None):
    """rows r0 .. r0 + R - 1 of the permutation list -> (R, n) int32"""
    st = [0] * n if strata is None else [int(s) for s in strata]
    out = np.zeros((R, n), dtype=np.int32)
    for k in range(R):
        r = r0 + k
        pi = list(range(n))
        if r > 0:
            for s in sorted(set(st)):
                E = [i for i in range(n) if st[i] == s]
                sigma = sorted(E, key=lambda u: (mix64((seed & MASK) ^ mix64(((r << 32) + u) & MASK)), u))
                for t, u in enumerate(sigma):
                    pi[u] = E[t]
        out[k] = pi
    return out


# ---- the finishers -------------------------------------------------------------------------------------------------------------
def from_sums(N, Sa, Saa, Sb, Sbb, Sab):
    """include/tpg.h "Mantel tests", tpg_mantel_from_sums, one float64 statement after the other"""
    f = np.float64
    if N < 1:
        return f("nan")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        Nd = f(N)
        mab = f(Sa) * f(Sb)
        cab = f(Sab) - mab / Nd
        maa = f(Sa) * f(Sa)
        va = f(Saa) - maa / Nd
        mbb = f(Sb) * f(Sb)
        vb = f(Sbb) - mbb / Nd
        if not (va > 0.0) or not (vb > 0.0):
            return f("nan")
        den = np.sqrt(va * vb)
        return cab / den


def partial(r_ab, r_ac, r_bc):
    f = np.float64
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        fa = f(1.0) - f(r_ac) * f(r_ac)
        fb = f(1.0) - f(r_bc) * f(r_bc)
        if not (fa > 0.0) or not (fb > 0.0):
            return f("nan")
        num = f(r_ab) - f(r_ac) * f(r_bc)
        den = np.sqrt(fa * fb)
        return num / den


def from_sums_exact(N, Sa, Saa, Sb, Sbb, Sab):
    """-> (the covariance term, the product of the variance terms) in Fractions: r^2 = cov^2 / vv, sign(r) = sign(cov)"""
    F = Fraction
    cov = F(Sab) - F(Sa) * F(Sb) / N
    return cov, (F(Saa) - F(Sa) ** 2 / N) * (F(Sbb) - F(Sb) ** 2 / N)


def partial_exact(r_ab, r_ac, r_bc):
    """-> (numerator, the product under the root) in Fractions"""
    F = Fraction
    return F(r_ab) - F(r_ac) * F(r_bc), (1 - F(r_ac) ** 2) * (1 - F(r_bc) ** 2)


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def moments(A, L):
    """(S, SS) in the order of the cross sums: b = 1.0 (a * 1.0 is a) and b = a, identity permutation"""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    ident = np.arange(n).reshape(1, n)
    return (float(ordered_sums(A, [np.ones((n, n))], ident, L)[0, 0]), float(ordered_sums(A, [A], ident, L)[0, 0]))


def center(A, mean):
    A = np.asarray(A, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.eye(A.shape[0], dtype=bool), 0.0, A - np.float64(mean))


def midranks(M):
    """the strict lower triangle replaced by its mid-ranks (1-based), mirrored, +0.0 on the diagonal; one entry after the other"""
    M = np.asarray(M, dtype=np.float64)
    n = M.shape[0]
    assert all(M[i, j] == M[j, i] for i in range(n) for j in range(i))
    cells = [(i, j) for j in range(n) for i in range(j + 1, n)]
    vals = sorted(M[c] for c in cells)
    out = np.zeros((n, n))
    import bisect

    for (i, j) in cells:
        lo, hi = bisect.bisect_left(vals, M[i, j]), bisect.bisect_right(vals, M[i, j])
        out[i, j] = out[j, i] = (lo + 1 + hi) / 2.0
    return out


def mantel(A, y, L, n_perm, seed, z=None, strata=None, method="pearson"):
    """gt_mantel by the pieces above -> dict(statistic, p_value, n_valid, perm, and r_ab, r_ac, r_bc with z)"""
    mats = [np.asarray(M, dtype=np.float64) for M in ([A, y] + ([z] if z is not None else []))]
    n = mats[0].shape[0]
    N = n * (n - 1)
    if method == "spearman":
        mats = [midranks(M) for M in mats]
    mom = []
    for k, M in enumerate(mats):
        mats[k] = center(M, np.float64(moments(M, L)[0]) / np.float64(N) if N > 0 else 0.0)
        mom.append(moments(mats[k], L))
    P = perms(n, seed, 0, n_perm + 1, strata)
    sums = ordered_sums(mats[0], mats[1:], P, L)
    (Sa, Saa), (Sb, Sbb) = mom[0], mom[1]
    r_ab = np.array([from_sums(N, Sa, Saa, Sb, Sbb, s) for s in sums[:, 0]])
    out = {}
    if z is None:
        stat = r_ab
    else:
        Sc, Scc = mom[2]
        r_ac = np.array([from_sums(N, Sa, Saa, Sc, Scc, s) for s in sums[:, 1]])
        r_bc = from_sums(N, Sb, Sbb, Sc, Scc, ordered_sums(mats[1], [mats[2]], P[:1], L)[0, 0])
        stat = np.array([partial(a, c, r_bc) for a, c in zip(r_ab, r_ac)])
        out.update(r_ab=float(r_ab[0]), r_ac=float(r_ac[0]), r_bc=float(r_bc))
    p, nv = pvalue(stat[0], stat[1:])
    out.update(statistic=float(stat[0]), p_value=p, n_valid=nv, n_perm=n_perm, perm=stat[1:].copy())
    return out


def check_result(got, want):
    """every number of a gt_mantel(return_perm=True) result equals the restatement's"""
    keys = ["statistic", "p_value"] + [k for k in ("r_ab", "r_ac", "r_bc") if k in want]
    assert sorted(k for k in got if k.startswith("r_")) == sorted(k for k in want if k.startswith("r_"))
    for k in keys:
        assert same_values(got[k], want[k]), (k, got[k], want[k])
    assert got["n_valid"] == want["n_valid"] and got["n_perm"] == want["n_perm"]
    assert same_values(got["perm"], want["perm"])


def planted_case():
    """41 points uniform in a square; y = their Euclidean distances, A = y / max(y) + half a standard deviation of symmetric
    Gaussian noise"""
    rng = np.random.default_rng(2024)
    xy = rng.uniform(size=(41, 2))
    y = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(axis=2))
    base = y / y.max()
    noise = rng.normal(size=(41, 41))
    noise = (noise + noise.T) / np.sqrt(2.0)
    A = base + 0.5 * base[~np.eye(41, dtype=bool)].std() * noise
    np.fill_diagonal(A, 0.0)
    return np.asfortranarray(A), np.asfortranarray(y)


# ---- the host pieces as a stand-alone program --------------------------------------------------------------------------------
def build_host_program(exe, sanitize=True):
    """tests/host/mantel_san.cpp (csrc/host/host_mantel.h on the host) -> exe"""
    import subprocess

    san = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", *san, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-function", "-pthread",
           "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc"), os.path.join(ROOT, "tests", "host", "mantel_san.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_host_program(exe, path, queries):
    """one list of integers per query (see tests/host/mantel_san.cpp) -> one list of integers per query"""
    import subprocess

    with open(path, "w") as fh:
        fh.write("\n".join(" ".join(str(int(x)) for x in q) for q in queries) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stderr[-4000:])
    rows = [[int(w) for w in line.split()] for line in out.stdout.splitlines()]
    assert len(rows) == len(queries)
    return rows
