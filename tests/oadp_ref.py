"""include/tpg.h "OADP projection" restated in float64 numpy (LAPACK's SVD of M, then of C), and the brute-force form it
approximates: the SVD of the reference panel with the new row appended, then the Procrustes fit of its first n rows.  Also the
inputs the tests share and the driver of the stand-alone host program (tests/host/oadp_san.cpp)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEGENERATE = 2.0 ** -40


def oadp_row(l, s, d):
    """one individual: l (K) its row of XV, s its squared norm, d (K) the singular values -> (row (K), degenerate)"""
    l, d = np.asarray(l, dtype=np.float64), np.asarray(d, dtype=np.float64)
    K = len(d)
    rho2 = max(float(s) - float(l @ l), 0.0)
    M = np.zeros((K + 1, K + 1))
    M[:K, :K] = np.diag(d)
    M[K, :K] = l
    M[K, K] = np.sqrt(rho2)
    A, S, _ = np.linalg.svd(M)
    A, S = A[:, :K], S[:K]
    A1, a = A[:K], A[K]
    C = (S[:, None] * A1.T) * d[None, :]
    P, sg, Wt = np.linalg.svd(C)
    if not sg.min() > DEGENERATE * sg.max():
        return np.full(K, np.nan), True
    R = P @ Wt
    c = sg.sum() / np.sum((A1 * S) ** 2)
    return c * ((a * S) @ R), False


def oadp_proj(XV, X_norm, d):
    """every row -> (n x K, the count of degenerate rows): oadp_row with LAPACK called on stacks of matrices"""
    XV, s, d = np.asarray(XV, dtype=np.float64), np.asarray(X_norm, dtype=np.float64), np.asarray(d, dtype=np.float64)
    n, K = XV.shape
    M = np.zeros((n, K + 1, K + 1))
    M[:, :K, :K] = np.diag(d)
    M[:, K, :K] = XV
    M[:, K, K] = np.sqrt(np.maximum(s - (XV * XV).sum(axis=1), 0.0))
    A, S, _ = np.linalg.svd(M)
    A, S = A[:, :, :K], S[:, :K]
    A1, a = A[:, :K, :], A[:, K, :]
    C = (S[:, :, None] * np.swapaxes(A1, 1, 2)) * d[None, None, :]
    P, sg, Wt = np.linalg.svd(C)
    bad = ~(sg.min(axis=1) > DEGENERATE * sg.max(axis=1))
    with np.errstate(all="ignore"):  # (a degenerate row may divide by zero)
        c = sg.sum(axis=1) / ((A1 * S[:, None, :]) ** 2).sum(axis=(1, 2))
        out = c[:, None] * np.einsum("nk,nkj->nj", a * S, P @ Wt)
    out[bad] = np.nan
    return out, int(bad.sum())


def brute(Z, z, K):
    """Z (n x m) the scaled reference panel, z (m) a new scaled row: the K scores of z in the SVD of [Z; z], after the Procrustes
    fit (rotation and scale, no translation) of that SVD's first n rows onto the scores U D of Z alone"""
    U, d, _ = np.linalg.svd(Z, full_matrices=False)
    X0 = U[:, :K] * d[:K]
    Up, dp, _ = np.linalg.svd(np.vstack([Z, z]), full_matrices=False)
    Y = Up[:, :K] * dp[:K]
    C = Y[:-1].T @ X0
    P, sg, Wt = np.linalg.svd(C)
    return (sg.sum() / np.sum(Y[:-1] ** 2)) * (Y[-1] @ (P @ Wt))


def bound(l, s, d):
    """the elementwise bound of the shape grid: 256 (K + 1) eps (d_1 / d_K)^2 max(|l|_inf, sqrt(s))"""
    l, d = np.asarray(l, dtype=np.float64), np.asarray(d, dtype=np.float64)
    return 256.0 * (len(d) + 1) * 2.0 ** -52 * (d[0] / d[-1]) ** 2 * max(np.abs(l).max(), np.sqrt(s))


def grid_case(seed, n, K, ratio):
    """the inputs of the shape grid: d descending from 30 ratio to 30 (ratio = d_1 / d_K in {1.5, 10, 100}); l Gaussian times
    {0.1, 1, 10, 30} and rho^2 in {0, 1, 100, 400}, every combination present once n >= 16 -> (XV, X_norm, d)"""
    rng = np.random.default_rng(seed)
    d = np.sort(rng.uniform(1.0, ratio, K))[::-1] * 30.0
    d[0], d[-1] = 30.0 * ratio, 30.0  # (K = 1: d = 30)
    i = np.arange(n)
    XV = rng.standard_normal((n, K)) * np.array([0.1, 1.0, 10.0, 30.0])[i % 4][:, None]
    X_norm = (XV * XV).sum(axis=1) + np.array([0.0, 1.0, 100.0, 400.0])[(i // 4) % 4]
    return np.asfortranarray(XV), X_norm, np.ascontiguousarray(d)


def exact_case(seed=0, n=12, m=100, n_new=30):
    """Z random n x m with row scales in [0.5, 2] and n_new new rows -> (Z, new rows)"""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, m)) * rng.uniform(0.5, 2.0, (n, 1))
    return Z, rng.standard_normal((n_new, m))


def inputs(Z, Znew, K):
    """(XV, X_norm, d) of new rows against the SVD of Z"""
    _, d, Vt = np.linalg.svd(Z, full_matrices=False)
    return np.asfortranarray(Znew @ Vt[:K].T), (Znew * Znew).sum(axis=1), np.ascontiguousarray(d[:K])


def build_host_program(exe, sanitize):
    """tests/host/oadp_san.cpp (csrc/host/host_oadp.h with a team of one) -> exe; sanitize: under the address and
    undefined-behaviour sanitizers"""
    san = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", *san, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-function",
           "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc"), os.path.join(ROOT, "tests", "host", "oadp_san.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _hex(a):
    return " ".join(f"{x:016x}" for x in np.asarray(a, dtype=np.float64).ravel(order="F").view(np.uint64))


def run_host_program(exe, tmp_path, XV, nrm, d):
    """-> (the code of the check of d, the n x K results or None, the count of degenerate rows or None)"""
    path = tmp_path / "oadp.txt"
    path.write_text(f"{XV.shape[0]} {XV.shape[1]}\n{_hex(d)}\n{_hex(XV)}\n{_hex(nrm)}\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok oadp"
    rc = int(lines[0].split()[1])
    if rc:
        return rc, None, None
    vals = np.array([int(v, 16) for v in lines[2].split()[1:]], dtype=np.uint64).view(np.float64)
    return rc, vals.reshape(XV.shape, order="F"), int(lines[1].split()[1])


def binomial_panel(seed=1, n_ref=200, n_new=50, m=5000, npop=3):
    """the shrinkage panel: genotypes of npop populations -> (reference codes, new codes, labels of both)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, (npop, m))
    lab = rng.integers(0, npop, n_ref + n_new)
    G = rng.binomial(2, p[lab]).astype(np.uint8)
    return G[:n_ref], G[n_ref:], lab[:n_ref], lab[n_ref:]
