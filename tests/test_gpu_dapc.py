"""GPU: gt_cluster_pca, gt_cluster_pca_best_k and gt_dapc (include/tpg.h "k-means on PCA scores", "DAPC") against the numpy
restatements tests/kmeans_ref.py and tests/dapc_ref.py.

What is compared how.  gt_cluster_pca: the restatement runs every (k, t) from the same run seeds; the smallest relative gap
between a point's best and second-best distance over ALL those runs must exceed 1e-9 on the restatement; then the groups are
equal, WSS lies within twice the header's bound, and AIC / BIC within what that leaves of n log(WSS / n).  gt_dapc: the
discriminant analysis is host code, held to 1e-9 relative against the restatement as in tests/test_dapc_host.py; var.load and
var.contr come off the device and are held to the header's rounding bounds around the product of the DEVICE's loadings."""
import os

import numpy as np
import pytest

from tests import dapc_ref as dr
from tests import fixtures as fx
from tests import kmeans_ref as kr

pytestmark = pytest.mark.gpu


def _fake_pca(seed=11, n=120, d=4, g=3, m=257, sep=7.0):
    """blobs as the scores u d of a pca dict"""
    rng = np.random.default_rng(seed)
    truth = np.arange(n) % g
    scores = rng.normal(size=(g, d))[truth] * sep + rng.normal(size=(n, d))
    dd = np.sort(np.sqrt((scores ** 2).sum(axis=0)))[::-1].copy()
    u = np.asfortranarray(scores / dd[None, :])
    return dict(u=u, d=dd, v=np.asfortranarray(rng.normal(size=(m, d)) / np.sqrt(m)), center=np.zeros(m), scale=np.ones(m)), truth


def _check_clusters(cl, scores, ks, n_start, seed):
    n, d = scores.shape
    ref = kr.cluster_pca(scores, ks, n_start=n_start, seed=seed)
    gap = min(r["min_gap"] for r in ref["runs"].values())
    assert gap > 1e-9, gap  # on the restatement, over every run of every k
    A = np.abs(scores).max()
    assert cl["k"] == list(ks)
    for pos, k in enumerate(ks):
        win = ref["runs"][(k, ref["winner"][k])]
        assert np.array_equal(cl["groups"][k], ref["groups"][k]), k
        assert cl["groups"][k].min() == 1 and cl["groups"][k].max() <= k
        bw = 2 * kr.bound_wss(n, d, A, ref["WSS"][pos])
        assert abs(cl["WSS"][pos] - ref["WSS"][pos]) <= bw, (k, cl["WSS"][pos], ref["WSS"][pos], bw)
        # n log(W / n): a relative error e of W moves the logarithm by e (1 + e); the rest are a few roundings of the value
        for name in ("AIC", "BIC"):
            tol = n * (bw / ref["WSS"][pos]) * 1.001 + 8 * kr.EPS * (abs(n * np.log(ref["WSS"][pos] / n)) + np.log(n) * k)
            assert abs(cl[name][pos] - ref[name][pos]) <= tol, (name, k)
        assert (cl["n_iter"][pos], cl["converged"][pos], cl["n_empty"][pos]) == (win["n_iter"], win["converged"], win["n_empty"])
    return ref


def test_gt_cluster_pca_on_blobs_follows_the_restatement():
    import tidypopgen_amd as tpg

    pca, truth = _fake_pca()
    scores = (pca["u"] * pca["d"][None, :])[:, :4]
    out = tpg.gt_cluster_pca(pca, k_clusters=(1, 6), n_start=4, seed=5)
    cl = out["clusters"]
    assert out["u"] is pca["u"] and cl["method"] == "kmeans" and cl["n_pca"] == 4
    ref = _check_clusters(cl, scores, range(1, 7), 4, 5)
    # k = 1: all ones, the total sum of squares about the column means
    tot = ((scores - scores.mean(axis=0)) ** 2).sum()
    assert (cl["groups"][1] == 1).all() and abs(cl["WSS"][0] - tot) <= 2 * kr.bound_wss(120, 4, np.abs(scores).max(), tot) + 1e-13 * tot
    # the planted blobs come back at k = 3
    assert len(set(zip(cl["groups"][3].tolist(), truth.tolist()))) == 3
    # the winner of n_start is the run of smallest WSS, the first of equals: all runs of k = 5 side by side
    seeds = [kr.run_seed(5, 5, t) for t in range(4)]
    runs = tpg.kmeans_batch(scores, [5] * 4, seeds)
    t = int(np.argmin(runs["wss"]))
    assert t == ref["winner"][5] and runs["wss"][t] == cl["WSS"][4] and np.array_equal(runs["labels"][:, t] + 1, cl["groups"][5])
    assert len(set(runs["wss"].tolist())) > 1  # the starts do differ: the choice is not vacuous
    # fewer components, one k
    one = tpg.gt_cluster_pca(pca, n_pca=2, k_clusters=3, n_start=3, seed=1)["clusters"]
    _check_clusters(one, scores[:, :2].copy(), [3], 3, 1)
    # the default range is 1 .. round(n / 10)
    dflt = tpg.gt_cluster_pca(pca, n_start=1, seed=2)["clusters"]
    assert dflt["k"] == list(range(1, 13)) and len(dflt["BIC"]) == 12
    with pytest.raises(NotImplementedError):
        tpg.gt_cluster_pca(pca, method="ward")
    with pytest.raises(ValueError):
        tpg.gt_cluster_pca(pca, k_clusters=(1, 2, 3))


def test_best_k_criteria_and_their_quirks():
    import tidypopgen_amd as tpg

    def best(series, crit, stat="BIC"):
        return tpg.gt_cluster_pca_best_k(dict(clusters={stat: np.array(series)}), stat=stat, criterion=crit)["best_k"]

    s = [10.0, 6.0, 3.0, 3.0, 4.0, 2.5, 5.0]
    elbow = [200.0, 150.0, 110.0, 65.0, 64.0, 64.5, 64.0]
    assert best(s, "min") == 6 and best([5.0, 1.0, 1.0, 2.0], "min") == 2
    assert best(s, "goesup") == 4 and best(s, "goodfit") == 2 and best([1.0, 9.0, 9.5], "goodfit") == 0
    assert best(s, "smoothNgoesup") == 5 and best(elbow, "diffNgroup") == 4 and best(elbow, "diffNgroup", stat="WSS") == 4
    for crit in ("goesup", "smoothNgoesup"):
        with pytest.raises(ValueError):
            best([5.0, 4.0, 3.0, 3.0], crit)
    rng = np.random.default_rng(3)
    for _ in range(20):
        series = np.cumsum(rng.normal(size=rng.integers(4, 12))) * 10
        for crit in ("min", "goesup", "goodfit", "diffNgroup", "smoothNgoesup"):
            try:
                want = kr.best_k(series, crit)
            except ValueError:
                with pytest.raises(ValueError):
                    best(series, crit)
                continue
            assert best(series, crit) == want, (series, crit)
    with pytest.raises(ValueError):
        tpg.gt_cluster_pca_best_k(dict(u=1))


def _close(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max() <= 1e-9 * (np.abs(b).max() if scale is None else scale), (np.abs(a - b).max(), np.abs(b).max())


def _check_dapc(got, pca, grp, n_pca, n_da):
    ref = dr.dapc(pca, grp, n_pca, n_da)
    assert (got["n.pca"], got["n.da"]) == (ref["n.pca"], ref["n.da"])
    assert np.array_equal(got["tab"], ref["tab"]) and np.array_equal(got["grp"], ref["grp"]) and got["var"] == ref["var"]
    for name in ("eig", "means", "prior", "ind.coord"):
        _close(got[name], ref[name])
    for a in range(ref["n.da"]):
        _close(got["loadings"][:, a], ref["loadings"][:, a])
    _close(got["grp.coord"], ref["grp.coord"], scale=np.abs(ref["ind.coord"]).max())
    assert np.abs(got["posterior"] - ref["posterior"]).max() <= 1e-9 and np.abs(got["posterior"].sum(axis=1) - 1).max() <= 1e-14
    assert np.array_equal(got["assign"], ref["assign"])
    # the device part, around the loadings it was given
    V = np.asarray(pca["v"])[:, :n_pca]
    vc = dr.var_contr(V, got["loadings"])
    E, Ec = dr.bound_var_contr(V, got["loadings"])
    assert (np.abs(got["var.load"] - vc["var_load"]) <= 2 * E).all()
    assert (np.abs(got["var.contr"] - vc["var_contr"]) <= 2 * Ec).all()
    assert np.abs(got["var.contr"].sum(axis=0) - 1).max() <= 1e-12
    return ref


def test_gt_dapc_every_field_against_the_restatement():
    import tidypopgen_amd as tpg

    pca, truth = _fake_pca(seed=12, n=150, d=5, g=4, sep=2.5)
    # pop as labels of any type
    names = np.array(["d", "a", "c", "b"])[truth]
    got = tpg.gt_dapc(pca, pop=names, n_pca=5)
    _check_dapc(got, pca, names, 5, None)
    assert got["n.da"] == 3 and set(got["assign"].tolist()) <= set("abcd")
    # fewer discriminant functions, fewer components; n_pca above the number of columns is cut to it
    _check_dapc(tpg.gt_dapc(pca, pop=names, n_pca=3, n_da=1), pca, names, 3, 1)
    _check_dapc(tpg.gt_dapc(pca, pop=names, n_pca=9, n_da=2), pca, names, 5, 2)
    # through the clusters: pop = None takes best_k, a number takes that position; n_pca defaults to the clusters' (cut to G - 1 if above G)
    cl = tpg.gt_cluster_pca(pca, k_clusters=(1, 5), n_start=3, seed=1)
    with pytest.raises(ValueError):
        tpg.gt_dapc(cl)
    cl = tpg.gt_cluster_pca_best_k(cl, stat="BIC", criterion="diffNgroup")
    k = cl["clusters"]["k"][cl["best_k"] - 1]
    grp = cl["clusters"]["groups"][k]
    got = tpg.gt_dapc(cl)
    want_pca = 5 if 5 <= k else k - 1
    _check_dapc(got, pca, grp, want_pca, None)
    _check_dapc(tpg.gt_dapc(cl, pop=2, n_pca=4, loadings_by_locus=True), pca, cl["clusters"]["groups"][2], 4, None)
    assert "var.load" not in tpg.gt_dapc(cl, pop=2, n_pca=4, loadings_by_locus=False)
    # refusals: no centring, a variable constant within the groups (MASS stops there)
    with pytest.raises(ValueError):
        tpg.gt_dapc({**pca, "center": None}, pop=names)
    bad = dict(pca)
    bad["u"] = pca["u"].copy()
    bad["u"][:, 1] = np.array([2.0, 5.0, 7.0, 9.0])[truth]
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.gt_dapc(bad, pop=names, n_pca=5)
    assert e.value.code == 4


@pytest.mark.parametrize("m", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("n_da", [1, 3])
def test_var_load_and_var_contr(m, n_da):
    import tidypopgen_amd as tpg

    rng = np.random.default_rng(m * 10 + n_da)
    n_pca = 7
    V = np.asfortranarray(rng.normal(size=(m, n_pca)))
    ld = np.asfortranarray(rng.normal(size=(n_pca, n_da)))
    if n_da == 3:
        ld[:, 1] = 0.0  # an all-zero column: its sum of squares is below 1e-12
    got = tpg.dapc_var_contr(V, ld)
    ref = dr.var_contr(V, ld)
    E, Ec = dr.bound_var_contr(V, ld)
    assert got["var_load"].shape == (m, n_da)
    assert (np.abs(got["var_load"] - ref["var_load"]) <= 2 * E).all()
    assert (np.abs(got["var_contr"] - ref["var_contr"]) <= 2 * Ec).all()
    if n_da == 3:
        assert (got["var_contr"][:, 1] == 0).all() and (got["var_load"][:, 1] == 0).all()
    assert np.abs(got["var_contr"][:, 0].sum() - 1) <= 1e-12
    again = tpg.dapc_var_contr(V, ld)
    assert again["var_contr"].tobytes(order="F") == got["var_contr"].tobytes(order="F")
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.dapc_var_contr(np.zeros((4, 65)), np.zeros((65, 1)))
    assert e.value.code == 1


def test_end_to_end_on_the_lobster_panel():
    import tidypopgen_amd as tpg

    X = tpg.FBM.open_bed(os.path.join(fx.GOLDEN, "lobster", "lobster.bed"), 176, 79)
    pca = tpg.gt_pca_partialSVD(X, k=10, impute="mode")
    cl = tpg.gt_cluster_pca(pca, k_clusters=(1, 5), seed=0)
    scores = (pca["u"] * pca["d"][None, :])[:, :10]
    ref = _check_clusters(cl["clusters"], scores, range(1, 6), 10, 0)
    for crit in ("min", "goodfit", "diffNgroup"):
        assert tpg.gt_cluster_pca_best_k(cl, criterion=crit)["best_k"] == kr.best_k(ref["BIC"], crit)
    cl = tpg.gt_cluster_pca_best_k(cl)
    k = cl["clusters"]["k"][cl["best_k"] - 1]
    assert 2 <= k <= 5
    got = tpg.gt_dapc(cl)
    _check_dapc(got, pca, cl["clusters"]["groups"][k], 10 if 10 <= k else k - 1, None)
    assert got["var.load"].shape == (79, got["n.da"]) and (got["assign"] == cl["clusters"]["groups"][k]).mean() > 0.9
