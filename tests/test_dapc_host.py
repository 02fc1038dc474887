"""CPU: the numpy restatement of include/tpg.h "DAPC" (tests/dapc_ref.py) checked against the section's own invariants, and the
library's discriminant analysis (csrc/host/host_lda.h) as a stand-alone program under the host sanitizers against it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dapc_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def groups_data(seed=0, n=120, d=5, G=4, sep=3.0):
    rng = np.random.default_rng(seed)
    grp = rng.permutation(np.arange(n) % G).astype(np.int32)
    A = rng.normal(size=(d, d))  # correlated coordinates
    X = rng.normal(size=(n, d)) @ A + (rng.normal(size=(G, d)) * sep)[grp]
    return X, grp


def test_scaling_whitens_w_and_diagonalises_b():
    for seed, (n, d, G) in enumerate([(120, 5, 4), (60, 2, 5), (300, 20, 3), (40, 1, 2)]):
        X, grp = groups_data(seed, n, d, G)
        r = dr.lda(X, grp)
        S, L = r["scaling"], len(r["svd"])
        assert L == min(d, G - 1)
        assert np.abs(S.T @ r["W"] @ S - np.eye(L)).max() <= 1e-10
        SBS = S.T @ r["B"] @ S
        assert np.abs(SBS - np.diag(r["svd"] ** 2)).max() <= 1e-10 * max(1.0, r["svd"][0] ** 2)
        assert all(a >= b for a, b in zip(r["svd"], r["svd"][1:]))
        for a in range(L):  # the sign rule
            assert S[np.argmax(np.abs(S[:, a])), a] > 0


def test_posteriors_sum_to_one_and_follow_the_coordinates():
    rng = np.random.default_rng(3)
    grp = (np.arange(150) % 4).astype(np.int32)
    X = rng.normal(size=(150, 6)) + rng.normal(size=(4, 6))[grp]  # overlapping groups: posteriors strictly inside (0, 1)
    for n_da in (None, 1, 2):
        r = dr.lda(X, grp, n_da)
        p = r["posterior"]
        assert np.abs(p.sum(axis=1) - 1.0).max() <= 1e-14 and (p >= 0).all()
        assert np.array_equal(r["assign"], np.argmax(p, axis=1))
        assert r["ind_coord"].shape == (150, r["n_da"]) and r["n_da"] == (3 if n_da is None else n_da)
        assert np.abs(r["prior"] @ r["grp_coord"]).max() <= 1e-10  # the coordinates are centred on the weighted grand mean
    assert 0.3 < (dr.lda(X, grp)["assign"] == grp).mean() < 1.0


def test_refusals():
    X, grp = groups_data(1, 60, 3, 3)
    Xc = X.copy()
    Xc[:, 1] = np.array([2.0, 5.0, 7.0])[grp]  # constant within the groups: MASS stops, so do we
    with pytest.raises(dr.Refused) as e:
        dr.lda(Xc, grp)
    assert e.value.code == 4
    Xd = np.concatenate([X, X[:, :1] + X[:, 1:2]], axis=1)  # a combination of the others
    with pytest.raises(dr.Refused) as e:
        dr.lda(Xd, grp)
    assert e.value.code == 4
    with pytest.raises(dr.Refused) as e:
        dr.lda(X, np.zeros(60, dtype=np.int32))  # one group
    assert e.value.code == 1
    g2 = grp.copy()
    g2[g2 == 1] = 3  # group 1 is empty
    with pytest.raises(dr.Refused) as e:
        dr.lda(X, g2)
    assert e.value.code == 1
    with pytest.raises(dr.Refused) as e:
        dr.lda(X[:3], np.arange(3))  # n <= G
    assert e.value.code == 1


def test_var_contr_columns_sum_to_one_or_are_zero():
    rng = np.random.default_rng(2)
    V, ld = rng.normal(size=(257, 4)), rng.normal(size=(4, 3))
    ld[:, 1] = 0.0
    r = dr.var_contr(V, ld)
    assert np.allclose(r["var_contr"].sum(axis=0), [1.0, 0.0, 1.0], rtol=0, atol=1e-13) and (r["var_contr"][:, 1] == 0).all()


def _hex(a):
    return " ".join(f"{x:016x}" for x in np.asarray(a, dtype=np.float64).ravel(order="F").view(np.uint64))


def _run_san(exe, tmp_path, X, grp, G, n_da):
    path = tmp_path / "lda.txt"
    path.write_text(f"{X.shape[0]} {X.shape[1]} {G} {n_da}\n{_hex(X)}\n{' '.join(str(int(g)) for g in grp)}\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok lda"
    rc = int(lines[0].split()[1])
    got = {}
    for ln in lines[1:-1]:
        name, *vals = ln.split()
        if name in ("dims", "assign"):
            got[name] = np.array([int(v) for v in vals])
        else:
            got[name] = np.array([int(v, 16) for v in vals], dtype=np.uint64).view(np.float64)
    return rc, got


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_library_lda_stand_alone_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "lda_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DTPG_HOST_NO_CLONES",
           "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc"), os.path.join(ROOT, "tests", "host", "lda_san.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]

    def close(a, b, scale=None):
        b = np.asarray(b, dtype=np.float64).ravel(order="F")
        assert a.shape == b.shape
        assert np.abs(a - b).max() <= 1e-9 * (np.abs(b).max() if scale is None else scale), (np.abs(a - b).max(), np.abs(b).max())

    for seed, (n, d, G, n_da) in enumerate([(120, 5, 4, 3), (61, 2, 5, 1), (300, 20, 3, 64), (40, 1, 2, 1), (200, 64, 6, 5)]):
        X, grp = groups_data(seed, n, d, G)
        rc, got = _run_san(exe, tmp_path, X, grp, G, n_da)
        ref = dr.lda(X, grp, n_da)
        assert rc == 0 and got["dims"].tolist() == [len(ref["svd"]), ref["n_da"]]
        close(got["prior"], ref["prior"])
        close(got["means"], ref["means"])
        close(got["mu"], ref["mu"])
        close(got["svd"], ref["svd"])
        for a in range(len(ref["svd"])):  # per column: a small singular value leaves its vector less determined than 1e-9 of the largest
            close(got["scaling"][a * d:(a + 1) * d], ref["scaling"][:, a])
        close(got["ind_coord"], ref["ind_coord"])
        close(got["grp_coord"], ref["grp_coord"], scale=np.abs(ref["ind_coord"]).max())
        assert np.abs(got["posterior"] - ref["posterior"].ravel(order="F")).max() <= 1e-9
        assert np.array_equal(got["assign"], ref["assign"])
    # the refusals carry the header's codes
    X, grp = groups_data(1, 60, 3, 3)
    Xc = X.copy()
    Xc[:, 1] = np.array([2.0, 5.0, 7.0])[grp]
    assert _run_san(exe, tmp_path, Xc, grp, 3, 2)[0] == 4
    assert _run_san(exe, tmp_path, np.concatenate([X, X[:, :1] + X[:, 1:2]], axis=1), grp, 3, 2)[0] == 4
    assert _run_san(exe, tmp_path, X, np.zeros(60, dtype=int), 1, 1)[0] == 1
    g2 = grp.copy()
    g2[g2 == 1] = 3
    assert _run_san(exe, tmp_path, X, g2, 4, 2)[0] == 1
    assert _run_san(exe, tmp_path, X[:3], np.arange(3), 3, 1)[0] == 1
    Xn = X.copy()
    Xn[5, 2] = np.nan
    assert _run_san(exe, tmp_path, Xn, grp, 3, 2)[0] == 4


def test_library_lda_through_the_binding_needs_no_device():
    # tpg_lda is host only: the ctypes route of tidypopgen_amd.lda against the restatement, and the header's error codes
    import tidypopgen_amd as tpg

    X, grp = groups_data(7, 90, 4, 3)
    got, ref = tpg.lda(X, grp), dr.lda(X, grp)
    assert got["n_da"] == ref["n_da"] == 2 and np.array_equal(got["assign"], ref["assign"])
    for name in ("prior", "means", "mu", "svd", "ind_coord", "posterior"):
        assert np.abs(got[name] - ref[name]).max() <= 1e-9 * max(np.abs(ref[name]).max(), 1.0), name
    assert tpg.lda(X, grp, n_da=1)["ind_coord"].shape == (90, 1)
    Xc = X.copy()
    Xc[:, 1] = 0.1 * np.array([2.0, 5.0, 7.0])[grp]  # constant within the groups up to the rounding of the group means
    for bad, code in ((lambda: tpg.lda(Xc, grp), 4), (lambda: tpg.lda(X, np.zeros(90, dtype=np.int32)), 1),
                      (lambda: tpg.lda(X[:3], np.arange(3)), 1), (lambda: tpg.lda(np.zeros((90, 65)), grp), 1)):
        with pytest.raises(tpg._lib.TpgError) as e:
            bad()
        assert e.value.code == code
