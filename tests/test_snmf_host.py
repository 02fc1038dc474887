"""CPU: the numpy restatement of include/tpg.h "sNMF" (tests/snmf_ref.py) checked against itself: the criterion falls, a planted
Q comes back, the identity form of ls is the loss formed directly, and the hold-out counts are those of a direct loop.  Also the
library's own NNLS solver (csrc/host/host_nnls.h, the text the device runs one thread per system) as a stand-alone program
under the host sanitizers, against scipy and the KKT contract of the header."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import admix_ref as ar
from tests import snmf_ref as sr


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _planted(seed=3, n=60, m=150):
    rng = np.random.default_rng(seed)
    q1 = np.concatenate([np.ones(n // 3), np.zeros(n // 3), rng.uniform(0.2, 0.8, size=n - 2 * (n // 3))])
    Qt = np.stack([q1, 1.0 - q1], axis=1)
    Ft = rng.uniform(0.05, 0.95, size=(m, 2))
    codes = rng.binomial(2, Qt @ Ft.T).astype(np.uint8)
    codes[rng.random(codes.shape) < 0.03] = sr.MISSING
    return codes, Qt


def test_step_lowers_ls_monotonically():
    codes, _ = _planted()
    Q = ar.start(5, codes.shape[0], codes.shape[1], 3)[0]
    ls = []
    for _ in range(20):
        r = sr.step(codes, Q, 10.0)
        Q = r["Q"]
        ls.append(r["ls"])
    assert all(b < a for a, b in zip(ls, ls[1:])), ls
    assert ls[-1] < 0.95 * ls[0]


def test_k2_run_recovers_the_planted_q_up_to_a_column_swap():
    codes, Qt = _planted()
    r = sr.run(codes, 2, seed=1)
    assert r["converged"] and 2 <= r["n_iter"] < 200
    err = min(np.abs(r["Q"] - Qt).mean(), np.abs(r["Q"][:, ::-1] - Qt).mean())
    assert err < 0.08, err
    assert np.allclose(r["Q"].sum(axis=1), 1.0) and np.allclose(r["G"].sum(axis=1), 1.0) and (r["Q"] >= 0).all() and (r["G"] >= 0).all()


def test_identity_form_of_ls_is_the_loss_formed_directly():
    codes, _, _, _ = ar.panel(7, 40, 90, 3, 0.1)
    Q = ar.start(2, 40, 90, 3)[0]
    for _ in range(3):
        g = sr.g_half(codes, Q)
        q = sr.q_half(codes, g["G"], 10.0)
        direct = sr.loss_direct(codes, q["Q"], g["G"])
        assert abs(q["ls"] - direct) <= 1e-9 * direct, (q["ls"], direct)
        Q = q["Q"]


def test_nnls_exact_meets_the_contract():
    rng = np.random.default_rng(0)
    for K in (1, 2, 3, 8, 16):
        Q = rng.dirichlet(np.full(K, 0.5), size=200)
        A = sr.ridge(Q.T @ Q)
        B = rng.normal(size=(60, K))
        X = sr.nnls_exact(A, B)
        assert (X >= 0).all()
        for b, x in zip(B, X):
            assert sr.kkt_residual(A, b, x) <= 1e-10 * np.abs(b).max()


def test_holdout_counts_match_a_direct_loop():
    codes, _, _, _ = ar.panel(9, 23, 37, 2, 0.1)
    for fraction in (0.05, 0.5):
        for seed in (1, 0xDEADBEEFCAFEF00D):
            train = sr.holdout_fraction(codes, fraction, seed)
            thr, held = int(np.floor(fraction * 2.0 ** 32)), 0
            for i in range(codes.shape[0]):
                for j in range(codes.shape[1]):
                    key = ar.mix64_int(((seed & ar.MASK) ^ sr.CV_SALT) ^ ar.mix64_int(j))
                    h = ar.mix64_int(key ^ ar.mix64_int(i))
                    want = codes[i, j] != sr.MISSING and (h >> 32) < thr
                    held += bool(want)
                    assert train[i, j] == (sr.MISSING if want else codes[i, j])
            assert held == int(((codes != sr.MISSING) & (train == sr.MISSING)).sum())
            typed = int((codes != sr.MISSING).sum())
            assert abs(held - fraction * typed) < 4 * np.sqrt(typed * fraction * (1 - fraction)) + 1
    # the sums split: all + masked of the hold-out pair = all of the pair (codes, codes)
    Q = ar.start(4, 23, 37, 2)[0]
    G = sr.g_half(codes, Q)["G"]
    train = sr.holdout_fraction(codes, 0.5, 1)
    a, b = sr.cross_entropy_sums(codes, train, Q, G), sr.cross_entropy_sums(codes, codes, Q, G)
    assert a["n_masked"] + a["n_all"] == b["n_all"] and b["n_masked"] == 0
    assert abs(a["sum_masked"] + a["sum_all"] - b["sum_all"]) <= 1e-10 * b["sum_all"]


def _hex(a):
    return " ".join(f"{x:016x}" for x in np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_library_nnls_solver_stand_alone_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "nnls_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "nnls_san.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    rng = np.random.default_rng(17)
    # the two kinds of matrix of an iteration: Q'Q of simplex rows, and GG' + alpha 1 1' (ill-conditioned by the rank-one term)
    for K in (1, 2, 3, 4, 5, 8, 11, 16):
        Q = rng.dirichlet(np.full(K, 0.5), size=130)
        G = rng.dirichlet(np.full(3, 0.7), size=(60, K)).transpose(0, 2, 1).reshape(180, K)
        for A in (sr.ridge(Q.T @ Q), sr.ridge(G.T @ G, 10.0)):
            B = rng.uniform(0, 20, size=(120, K))
            B[::3] = 10 * rng.normal(size=B[::3].shape)  # signs that force zeros
            B[5], B[6] = 0.0, -1.0
            path = tmp_path / "systems.txt"
            path.write_text(f"{K} {len(B)}\n{_hex(A)}\n{_hex(B)}\n")
            out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
            assert out.returncode == 0, out.stderr[-4000:]
            lines = out.stdout.splitlines()
            assert lines[-1] == "ok nnls" and len(lines) == len(B) + 1 and "PAD" not in out.stdout
            assert all(ln.split()[1] == "1" for ln in lines[:-1])  # the solver's own verdict: every system meets the contract
            X = np.array([[int(h, 16) for h in ln.split()[2:]] for ln in lines[:-1]], dtype=np.uint64).view(np.float64)
            assert (X >= 0).all() and (X[5] == 0).all() and (X[6] == 0).all()
            for b, x in zip(B, X):
                assert sr.kkt_residual(A, b, x) <= sr.KKT_TOL * np.abs(b).max()
            # both this x and scipy's lie within the contract's distance of the optimum
            assert (np.abs(X - sr.nnls_exact(A, B)).max(axis=1) <= 2 * sr.bound_nnls(A, B) + 1e-300).all()
