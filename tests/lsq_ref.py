"""include/tpg.h "least-squares projection" restated index by index, its exact route and its bounds.

Definition.  codes is n x m with 0, 1, 2 = dosage and 3 = missing; T_i the loci where individual i is typed, t_i = |T_i|.
  z_ij = (g_ij - center_j) * (1 / scale_j);  A_i[a,b] = sum_{j in T_i} V[j,a] V[j,b];  b_i[a] = sum_{j in T_i} z_ij V[j,a];
  A_i x_i = b_i by the packed Cholesky of csrc/host/host_lsq.h (solve_restated below is that text in Python floats, operation for
  operation: the same bits as the host program), with the singular rule t_i < L, or a pivot failing p_k > L 2^-52 A_i[k,k], or a
  pivot that is not finite -> the row is NaN and counted.

Exact route.  Sums and the solve in long double (eps_l = 2^-64 on x86-64): the sums term by term, the solve by a Cholesky
factorisation with three steps of iterative refinement.  Its own error against the true value is at most (t + 2) 2^-64 sum|.| for
a sum -- 2^-11 of the bounds below -- so the tests hold the code under test to (1 - 2^-10) of each bound: a stricter check, never
a wider one.  REF_SLACK is that factor.

Bounds, eps = 2^-53.
  A: every product V[j,a] V[j,b] is rounded once (relative eps), and a sum of t terms in ANY order has relative error at most
     (t - 1) eps / (1 - (t - 1) eps) per term; together (1 + eps)^t - 1 <= (t + 2) eps for t eps < 0.01.  A fused multiply-add
     removes the product's rounding.                       |dA_i[a,b]| <= (t_i + 2) eps sum_{j in T_i} |V[j,a] V[j,b]|
  b: z carries three roundings against (g - center) / scale -- the subtraction, the reciprocal, the product -- then the product
     with V and the sum as above: (1 + eps)^(t + 3) - 1.    |db_i[a]|   <= (t_i + 4) eps sum_{j in T_i} |z_ij V[j,a]|
  solve from given (A, b): Cholesky is backward stable, (A + dA) x^ = b with |dA|_2 <= e_c |A|_2, e_c = 4 L (3 L + 1) eps (Higham,
     Accuracy and Stability of Numerical Algorithms, Thm 10.4 with its constants rounded up -- RECALLED, NOT PINNED), hence
                                                            |x^ - x|_2 <= k e_c / (1 - k e_c) |x|_2,  k = kappa_2(A)
  whole chain: perturbations e_A = |bound_A|_F / |A_i|_2 of A and e_b = |bound_b|_2 / |b_i|_2 of b ahead of the solve
     (Higham Thm 7.2):                                      |x^ - x|_2 <= k (e_A + e_b + e_c) / (1 - k (e_A + e_c)) |x_i|_2
A row is held to the solve and chain bounds only when k (e_A + e_c) < 0.1; on the grids of the tests no non-singular row may be
left out (the tests assert that count is zero)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
REF_SLACK = 1.0 - 2.0 ** -10
LD = np.longdouble


def pairs(L):
    """the packed order: (a, b), a <= b, a-major"""
    return [(a, b) for a in range(L) for b in range(a, L)]


def pidx(L, a, b):
    return a * L - a * (a - 1) // 2 + (b - a)


def unpack(Ap_row, L):
    A = np.zeros((L, L), dtype=np.asarray(Ap_row).dtype)
    for p, (a, b) in enumerate(pairs(L)):
        A[a, b] = A[b, a] = Ap_row[p]
    return A


def normal_exact(codes, center, scale, V):
    """the exact route of the sums -> dict(A n x P, b n x L in long double, n_typed, SA = sum |V_a V_b| and Sb = sum |z V_a| over
    the typed loci, in float64: what the bounds multiply)"""
    codes = np.asarray(codes)
    n, m = codes.shape
    L = V.shape[1]
    mask = codes < 3
    Vl = np.asarray(V, dtype=LD)
    z = (codes.astype(LD) - np.asarray(center, dtype=LD)) / np.asarray(scale, dtype=LD)
    z = np.where(mask, z, LD(0))
    ml = mask.astype(LD)
    pr = pairs(L)
    A = np.zeros((n, len(pr)), dtype=LD)
    SA = np.zeros((n, len(pr)))
    for p, (a, b) in enumerate(pr):
        prod = Vl[:, a] * Vl[:, b]  # exact up to 2^-64: a product of two doubles has 106 bits
        A[:, p] = ml @ prod
        SA[:, p] = (ml @ np.abs(prod)).astype(np.float64)
    b = z @ Vl
    Sb = (np.abs(z) @ np.abs(Vl)).astype(np.float64)
    return dict(A=A, b=b, n_typed=mask.sum(axis=1).astype(np.int64), SA=SA, Sb=Sb)


def bound_A(ex):
    return (ex["n_typed"][:, None] + 2) * EPS * ex["SA"]


def bound_b(ex):
    return (ex["n_typed"][:, None] + 4) * EPS * ex["Sb"]


def normal_float(codes, center, scale, V):
    """the definition in float64 in the stated arithmetic of z, every sum in ascending locus order (one locus per step, all rows
    and columns at once: elementwise, so the bits are those of the scalar loops)"""
    codes = np.asarray(codes)
    n, m = codes.shape
    L = V.shape[1]
    pr = pairs(L)
    mask = codes < 3
    z = (codes.astype(np.float64) - np.asarray(center, dtype=np.float64)) * (1.0 / np.asarray(scale, dtype=np.float64))
    ia, ib = [a for a, _ in pr], [b for _, b in pr]
    A = np.zeros((n, len(pr)), order="F")
    b = np.zeros((n, L), order="F")
    for j in range(m):
        rows = mask[:, j]
        A[rows] += V[j, ia] * V[j, ib]
        b[rows] += z[rows, j][:, None] * V[j]
    return A, b, mask.sum(axis=1).astype(np.int64)


def solve_row_restated(Ap, b, t, cast=float):
    """csrc/host/host_lsq.h for one row, operation for operation (cast = float: Python floats are IEEE doubles without
    contraction; cast = np.float32 carries the same solve out in single precision) -> (x, singular)"""
    import math

    L = len(b)
    sq = math.sqrt if cast is float else np.sqrt
    R = [cast(v) for v in Ap]
    y = [cast(v) for v in b]
    x = [cast(0.0)] * L
    singular = t < L
    tol = cast(L * 2.0 ** -52)
    big = cast(np.finfo(np.float64 if cast is float else cast).max)
    for k in range(L):
        kk = pidx(L, k, k)
        akk = R[kk]
        s = cast(0.0)
        for c in range(k):
            r = R[pidx(L, c, k)]
            s = s + r * r
        piv = akk - s
        if not (piv > tol * akk) or not (piv <= big):
            singular = True
        rkk = sq(piv) if piv >= 0 else cast(np.nan)
        R[kk] = rkk
        for bc in range(k + 1, L):
            q = cast(0.0)
            for c in range(k):
                q = q + R[pidx(L, c, k)] * R[pidx(L, c, bc)]
            R[kk + bc - k] = _div(R[kk + bc - k] - q, rkk, cast)
    for k in range(L):
        q = cast(0.0)
        for c in range(k):
            q = q + R[pidx(L, c, k)] * y[c]
        y[k] = _div(y[k] - q, R[pidx(L, k, k)], cast)
    for k in range(L - 1, -1, -1):
        kk = pidx(L, k, k)
        q = cast(0.0)
        for c in range(k + 1, L):
            q = q + R[kk + c - k] * x[c]
        x[k] = _div(y[k] - q, R[kk], cast)
    out = np.array([float(v) for v in x])
    if singular:
        out[:] = np.nan
    return out, bool(singular)


def _div(a, b, cast):
    # IEEE division: x / 0 is +-inf or NaN, where Python raises
    with np.errstate(all="ignore"):
        return cast(np.float64(a) / np.float64(b)) if cast is float else a / b


def solve_restated(Ap, b, nt, cast=float):
    """every row -> (x n x L, n_singular)"""
    Ap, b = np.asarray(Ap), np.asarray(b)
    out = np.zeros(b.shape, order="F")
    sing = 0
    with np.errstate(all="ignore"):
        for i in range(b.shape[0]):
            out[i], s = solve_row_restated(Ap[i], b[i], int(nt[i]), cast=cast)
            sing += s
    return out, sing


def _chol_solve_ld(R, rhs):
    L = R.shape[0]
    y = np.zeros(L, dtype=LD)
    for k in range(L):
        y[k] = (rhs[k] - R[:k, k] @ y[:k]) / R[k, k]
    x = np.zeros(L, dtype=LD)
    for k in range(L - 1, -1, -1):
        x[k] = (y[k] - R[k, k + 1:] @ x[k + 1:]) / R[k, k]
    return x


def solve_exact_row(A, b):
    """A (L x L) and b in long double -> x in long double: Cholesky and three steps of refinement"""
    A, b = np.asarray(A, dtype=LD), np.asarray(b, dtype=LD)
    L = len(b)
    R = np.zeros((L, L), dtype=LD)
    for k in range(L):
        R[k, k] = np.sqrt(A[k, k] - R[:k, k] @ R[:k, k])
        for c in range(k + 1, L):
            R[k, c] = (A[k, c] - R[:k, k] @ R[:k, c]) / R[k, k]
    x = _chol_solve_ld(R, b)
    for _ in range(3):
        x = x + _chol_solve_ld(R, b - A @ x)
    return x


def row_numbers(Ap_row, b_row, bA_row, bb_row, L):
    """kappa_2, e_A, e_b, e_c of one row (from the exact A and b and their elementwise bounds)"""
    A = unpack(np.asarray(Ap_row, dtype=np.float64), L)
    sv = np.linalg.svd(A, compute_uv=False)
    kap = sv[0] / sv[-1] if sv[-1] > 0 else np.inf
    eA = np.linalg.norm(unpack(bA_row, L), "fro") / sv[0]
    nb = np.linalg.norm(np.asarray(b_row, dtype=np.float64))
    eb = np.linalg.norm(bb_row) / nb if nb > 0 else 0.0
    ec = 4.0 * L * (3 * L + 1) * EPS
    return kap, eA, eb, ec


def solve_bound(kap, ec, xnorm):
    return kap * ec / (1.0 - kap * ec) * xnorm


def chain_bound(kap, eA, eb, ec, xnorm):
    return kap * (eA + eb + ec) / (1.0 - kap * (eA + ec)) * xnorm


def held(kap, eA, ec):
    return kap * (eA + ec) < 0.1


def grid_case(seed, n, m, L, frac):
    """orthonormalised Gaussian loadings V (m x L; m >= L), binomial codes typed with probability frac (at least L + 1 typed loci
    per row where m allows), center = 2 p, scale = sqrt(2 p (1 - p)) -> (codes n x m uint8, center, scale, V)"""
    rng = np.random.default_rng(seed)
    V = np.asfortranarray(np.linalg.qr(rng.standard_normal((m, L)))[0])
    p = rng.uniform(0.1, 0.9, m)
    codes = rng.binomial(2, p, (n, m)).astype(np.uint8)
    miss = rng.random((n, m)) >= frac
    codes[miss] = 3
    return codes, 2.0 * p, np.sqrt(2.0 * p * (1.0 - p)), V


def build_host_program(exe, sanitize):
    """tests/host/lsq_san.cpp (csrc/host/host_lsq.h with a team of one) -> exe; sanitize: under the address and
    undefined-behaviour sanitizers"""
    san = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", *san, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-function",
           "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc"), os.path.join(ROOT, "tests", "host", "lsq_san.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _hex(a):
    return " ".join(f"{x:016x}" for x in np.asarray(a, dtype=np.float64).ravel(order="F").view(np.uint64))


def run_host_program(exe, tmp_path, Ap, b, nt, L=None):
    """-> (the code of the argument check, the n x L results or None, the count of singular rows or None)"""
    Ap, b = np.asarray(Ap, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = b.shape[0]
    L = b.shape[1] if L is None else L
    path = tmp_path / "lsq.txt"
    path.write_text(f"{n} {L}\n{_hex(Ap)}\n{_hex(b)}\n{' '.join(str(int(t)) for t in nt)}\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stderr[-4000:])
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok lsq"
    rc = int(lines[0].split()[1])
    if rc:
        return rc, None, None
    vals = np.array([int(v, 16) for v in lines[2].split()[1:]], dtype=np.uint64).view(np.float64)
    return rc, vals.reshape((n, L), order="F"), int(lines[1].split()[1])
