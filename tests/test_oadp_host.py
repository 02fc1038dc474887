"""CPU: the numpy restatement of include/tpg.h "OADP projection" (tests/oadp_ref.py) against the brute-force SVD of the panel
with the new row appended; the routine the kernel runs (csrc/host/host_oadp.h) as a stand-alone program under the host
sanitizers against the restatement; and the arithmetic of predict_gt_dapc against a direct numpy restatement of "DAPC"."""
import shutil

import numpy as np
import pytest

from tests import oadp_ref as oref


def test_ref_is_the_brute_force_projection_when_k_is_the_rank():
    Z, new = oref.exact_case()
    XV, nrm, d = oref.inputs(Z, new, 12)
    got, deg = oref.oadp_proj(XV, nrm, d)
    want = np.array([oref.brute(Z, z, 12) for z in new])
    assert deg == 0
    assert np.abs(got - want).max() <= 1e-10 * d[0]


def test_ref_is_an_approximation_below_the_rank():
    # K = 3 of rank 12: the augmented SVD mixes the dropped directions in, so the exact case above is not vacuous
    Z, new = oref.exact_case()
    XV, nrm, d = oref.inputs(Z, new, 3)
    got, _ = oref.oadp_proj(XV, nrm, d)
    want = np.array([oref.brute(Z, z, 3) for z in new])
    err = np.abs(got - want).max()
    assert 1e-3 < err < 1.0, err
    assert np.abs(want).max() > 1.0


def test_ref_edge_rows():
    d = np.array([90.0, 50.0, 30.0])
    zero = np.zeros(3)
    assert np.array_equal(oref.oadp_row(zero, 0.0, d)[0], zero)
    assert np.array_equal(oref.oadp_row(zero, 30.0 ** 2 / 4, d)[0], zero)
    row, bad = oref.oadp_row(zero, 4 * 30.0 ** 2, d)
    assert bad and np.isnan(row).all()


_run_san = oref.run_host_program


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_library_routine_stand_alone_under_address_and_undefined_sanitizers(tmp_path):
    exe = oref.build_host_program(str(tmp_path / "oadp_san"), sanitize=True)
    worst = 0.0
    for seed, (n, K, ratio) in enumerate([(33, 1, 1.5), (32, 2, 10.0), (32, 3, 100.0), (32, 10, 100.0), (32, 20, 100.0),
                                          (32, 31, 10.0), (32, 32, 100.0), (16, 32, 1.5)]):
        XV, nrm, d = oref.grid_case(seed, n, K, ratio)
        rc, got, deg = _run_san(exe, tmp_path, XV, nrm, d)
        want, wdeg = oref.oadp_proj(XV, nrm, d)
        assert rc == 0 and deg == wdeg == 0
        for i in range(n):
            ratio_i = np.abs(got[i] - want[i]).max() / oref.bound(XV[i], nrm[i], d)
            worst = max(worst, ratio_i)
            assert ratio_i < 1.0, (n, K, i, ratio_i)
    print("largest ratio to the bound:", worst)
    # the exact case, and the edge rows
    Z, new = oref.exact_case()
    XV, nrm, d = oref.inputs(Z, new, 12)
    rc, got, deg = _run_san(exe, tmp_path, XV, nrm, d)
    assert rc == 0 and deg == 0
    assert np.abs(got - np.array([oref.brute(Z, z, 12) for z in new])).max() <= 1e-10 * d[0]
    d = np.array([90.0, 50.0, 30.0])
    XV = np.asfortranarray(np.zeros((4, 3)))
    XV[3] = [1.0, -2.0, 0.5]
    nrm = np.array([0.0, 30.0 ** 2 / 4, 4 * 30.0 ** 2, 9.0])
    rc, got, deg = _run_san(exe, tmp_path, XV, nrm, d)
    assert rc == 0 and deg == 1
    assert np.array_equal(got[:2], np.zeros((2, 3))) and np.isnan(got[2]).all()
    assert np.abs(got[3] - oref.oadp_row(XV[3], nrm[3], d)[0]).max() < oref.bound(XV[3], nrm[3], d)
    # the check of the singular values
    assert _run_san(exe, tmp_path, XV, nrm, np.array([50.0, 90.0, 30.0]))[0] == 2
    assert _run_san(exe, tmp_path, XV, nrm, np.array([90.0, 50.0, 0.0]))[0] == 2
    assert _run_san(exe, tmp_path, XV, nrm, np.array([90.0, np.nan, 30.0]))[0] == 1


def _dapc_direct(dapc, scores):
    """include/tpg.h "DAPC" for new scores, written out index by index"""
    x = np.asarray(scores, dtype=np.float64)[:, :dapc["n.pca"]]
    prior, means, S = dapc["prior"], dapc["means"], dapc["loadings"]
    G = len(prior)
    mu = np.zeros(means.shape[1])
    for g in range(G):
        mu = mu + prior[g] * means[g]
    z = (x - mu) @ S
    mg = (means - mu) @ S
    post = np.zeros((len(x), G))
    assign = np.zeros(len(x), dtype=int)
    for i in range(len(x)):
        q = np.array([0.5 * np.sum((z[i] - mg[g]) ** 2) - np.log(prior[g]) for g in range(G)])
        assign[i] = int(np.argmin(q))
        e = np.exp(-(q - q.min()))
        post[i] = e / e.sum()
    return z, post, dapc["levels"][assign]


def test_predict_gt_dapc_arithmetic():
    import tidypopgen_amd as tpg
    from tests import dapc_ref as dr

    rng = np.random.default_rng(5)
    n, d, G = 90, 4, 3
    grp = rng.permutation(np.arange(n) % G).astype(np.int32)
    X = rng.normal(size=(n, d)) + (rng.normal(size=(G, d)) * 2.0)[grp]
    r = dr.lda(X, grp, 2)
    levels = np.array(["a", "b", "c"])
    dapc = {"n.pca": d, "n.da": r["n_da"], "prior": r["prior"], "means": r["means"], "loadings": r["scaling"][:, :r["n_da"]],
            "levels": levels}
    new = np.concatenate([rng.normal(size=(25, d)) * 3.0, rng.normal(size=(25, 1))], axis=1)  # one column beyond n.pca: unused
    got = tpg.predict_gt_dapc(dapc, new)
    z, post, assign = _dapc_direct(dapc, new)
    assert got["ind.coord"].shape == (25, 2) and got["posterior"].shape == (25, 3)
    assert np.abs(got["ind.coord"] - z).max() <= 1e-12 * np.abs(z).max()
    assert np.abs(got["posterior"] - post).max() <= 1e-12
    assert np.array_equal(got["assign"], assign)
    assert np.abs(got["posterior"].sum(axis=1) - 1.0).max() <= 1e-14
    # on the training scores it is the analysis itself
    back = tpg.predict_gt_dapc(dapc, X)
    assert np.abs(back["ind.coord"] - r["ind_coord"]).max() <= 1e-12 * np.abs(r["ind_coord"]).max()
    assert np.abs(back["posterior"] - r["posterior"]).max() <= 1e-12
    assert np.array_equal(back["assign"], levels[r["assign"]])
    with pytest.raises(ValueError):
        tpg.predict_gt_dapc(dapc, new[:, :3])
