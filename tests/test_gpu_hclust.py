"""GPU: tpg_hclust_ward, tpg_cluster_wss and gt_cluster_pca_ward (include/tpg.h "Ward clustering on PCA scores") against the numpy
restatement tests/hclust_ref.py.

What is compared how.  The tree is a pure function of the scores, stated operation by operation in the header, so the device's
merge list equals the brute-force restatement's slot for slot and its heights bit for bit -- on tie-free blobs at sizes around a
wave, a 256-thread block and the 1024-thread pick block, and on inputs made of ties.  tpg_cluster_wss has no arithmetic of its
own: the labels of converged k-means runs give those runs' wss bit for bit.  gt_cluster_pca_ward: groups, merge and height equal,
WSS within twice the header's bound_wss, AIC and BIC within what that leaves."""
import ctypes as C

import numpy as np
import pytest

from tests import hclust_ref as hr
from tests import kmeans_ref as kr

pytestmark = pytest.mark.gpu

EINVAL, ENUMERIC = 1, 4  # TPG_EINVAL, TPG_ENUMERIC


def _same_tree(got, X, power):
    want = hr.ward_shared(X, power)
    n = X.shape[0]
    assert got["n"] == n and len(got["merge_a"]) == len(got["merge_b"]) == len(got["height"]) == n - 1
    first = np.nonzero((got["merge_a"] != want["merge_a"]) | (got["merge_b"] != want["merge_b"])
                       | (got["height"].view(np.uint64) != want["height"].view(np.uint64)))[0]
    assert len(first) == 0, (first[0], got["merge_a"][first[0]], got["merge_b"][first[0]], got["height"][first[0]],
                             want["merge_a"][first[0]], want["merge_b"][first[0]], want["height"][first[0]])
    assert np.array_equal(got["merge"], hr.r_merge(n, want["merge_a"], want["merge_b"]))


# every n with one d, every d at n = 65
SHAPES = [(1, 1), (2, 3), (3, 1), (63, 3), (64, 17), (65, 1), (65, 3), (65, 17), (65, 64), (257, 3), (301, 4), (1025, 3)]


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("n,d", SHAPES)
def test_tree_equals_the_restatement_merge_for_merge(n, d, power):
    import tidypopgen_amd as tpg

    X = hr.blobs(n + d, n, d)
    got = tpg.hclust_ward(X, power=power)
    if n == 1:
        assert got["n"] == 1 and len(got["merge_a"]) == len(got["height"]) == 0 and got["merge"].shape == (0, 2)
        assert tpg.hclust_cut(got, [1]).tolist() == [[0]]
        return
    _same_tree(got, X, power)


TIES = {"lattice": hr.lattice, "collinear": hr.collinear, "copies": hr.copies}


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("name", sorted(TIES))
def test_tree_on_inputs_made_of_ties(name, power):
    import tidypopgen_amd as tpg

    X = TIES[name]()
    assert X.shape[0] == {"lattice": 69, "collinear": 100, "copies": 40}[name]
    _same_tree(tpg.hclust_ward(X, power=power), X, power)


@pytest.mark.parametrize("power", [1, 2])
def test_star_many_rows_share_one_neighbour(power):
    import tidypopgen_amd as tpg

    X = hr.star()  # as stated: the origin, then 200 points on a sphere, d = 3
    assert X.shape == (201, 3)
    got = tpg.hclust_ward(X, power=power, return_list_len=True)
    _same_tree(got, X, power)
    print("star d = 3: recompute list, mean", got["list_len"][1:].mean(), "max", got["list_len"][1:].max())
    # In three dimensions the neighbours on the sphere are nearer than the centre, and the list looks at j > i only.  A star that
    # is one by construction (hclust_ref.axis_star: the origin last and nearest to every row): the first merge takes the point
    # of smallest radius, slot 0, and the origin, and every other row pointed at the origin: all 128 live rows are searched again
    Y = hr.axis_star()
    got = tpg.hclust_ward(Y, power=power, return_list_len=True)
    _same_tree(got, Y, power)
    print("axis star: recompute list, mean", got["list_len"][1:].mean(), "max", got["list_len"][1:].max())
    assert (got["merge_a"][0], got["merge_b"][0]) == (0, 128) and got["list_len"][0] == 129 and got["list_len"][1] == 128


def _raw_ward(ctx, xptr, n, d, power, fill=-7):
    import tidypopgen_amd as tpg

    m = max(n - 1, 1)
    ma, mb, h = np.full(m, fill, dtype=np.int32), np.full(m, fill, dtype=np.int32), np.full(m, float(fill))
    rc = tpg._lib.lib.tpg_hclust_ward(ctx.h, xptr, n, d, power, C.c_void_p(ma.ctypes.data), C.c_void_p(mb.ctypes.data), C.c_void_p(h.ctypes.data))
    return rc, ma, mb, h


def test_determinism_device_memory_and_refusals():
    import tidypopgen_amd as tpg

    ctx = tpg.default_context()
    X = hr.blobs(9, 301, 4)
    a, b = tpg.hclust_ward(X, power=2), tpg.hclust_ward(X, power=2)
    for name in ("merge_a", "merge_b", "merge"):
        assert np.array_equal(a[name], b[name])
    assert np.array_equal(a["height"].view(np.uint64), b["height"].view(np.uint64))
    # X in device memory, then the outputs there too (the library's own allocations: with torch imported after the library the
    # process would hold two HIP runtimes, README.md "with PyTorch in the same process")
    lib, bufs = tpg._lib.lib, []

    def dev(nbytes, src=None):
        p = ctx.dev_alloc(max(16, nbytes))
        bufs.append(p)
        if src is not None:
            tpg._lib.check(lib.tpg_dev_from_host(ctx.h, p, C.c_void_p(src.ctypes.data), C.c_size_t(src.nbytes)))
        return p

    def back(p, dtype, count):
        out = np.zeros(count, dtype=dtype)
        tpg._lib.check(lib.tpg_dev_to_host(ctx.h, C.c_void_p(out.ctypes.data), p, C.c_size_t(out.nbytes)))
        return out

    xd = dev(X.nbytes, X)
    rc, ma, mb, h = _raw_ward(ctx, xd, 301, 4, 2)
    assert rc == 0 and np.array_equal(ma, a["merge_a"]) and np.array_equal(mb, a["merge_b"])
    assert np.array_equal(h.view(np.uint64), a["height"].view(np.uint64))
    d_a, d_b, d_h = dev(1200), dev(1200), dev(2400)
    assert lib.tpg_hclust_ward(ctx.h, xd, 301, 4, 2, d_a, d_b, d_h) == 0
    assert np.array_equal(back(d_a, np.int32, 300), a["merge_a"]) and np.array_equal(back(d_b, np.int32, 300), a["merge_b"])
    assert np.array_equal(back(d_h, np.uint64, 300), a["height"].view(np.uint64))
    for p in bufs:
        ctx.dev_free(p)

    def refused(code, x, n, d, power):
        rc, ma, mb, h = _raw_ward(ctx, C.c_void_p(x.ctypes.data), n, d, power)
        assert rc == code, (rc, tpg._lib.lib.tpg_last_error())
        assert (ma == -7).all() and (mb == -7).all() and (h == -7.0).all()  # untouched

    Xs = hr.blobs(1, 65, 3)
    for bad in (np.nan, np.inf, -np.inf):
        Xn = Xs.copy(order="F")
        Xn[64, 2] = bad
        refused(ENUMERIC, Xn, 65, 3, 2)
    refused(EINVAL, Xs, 65, 0, 2)
    refused(EINVAL, np.zeros((4, 65), order="F"), 4, 65, 2)
    refused(EINVAL, Xs, 65, 3, 3)
    refused(EINVAL, Xs, 65, 3, 0)
    refused(EINVAL, Xs, 0, 3, 2)
    # n above the limit (the 8 n^2 bytes of S would be 8 GiB and more) is refused by the first checks, before any allocation
    refused(EINVAL, np.zeros(tpg.HCLUST_MAX_N + 1), tpg.HCLUST_MAX_N + 1, 1, 2)
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.hclust_ward(Xs, power=3)
    assert e.value.code == EINVAL
    # after a refusal the next call still runs
    _same_tree(tpg.hclust_ward(Xs, power=1), Xs, 1)


def test_cluster_wss_returns_the_bits_of_the_kmeans_runs_that_end_in_these_labels():
    import tidypopgen_amd as tpg

    X = hr.blobs(3, 301, 4)
    ks = [1, 2, 5, 17]
    runs = tpg.kmeans_batch(X, ks, [kr.run_seed(0, k, 0) for k in ks])
    assert runs["converged"].all()
    wss, counts = tpg.cluster_wss(X, runs["labels"], ks, return_counts=True)
    assert np.array_equal(wss.view(np.uint64), runs["wss"].view(np.uint64))
    for r, k in enumerate(ks):
        assert np.array_equal(counts[r], np.bincount(runs["labels"][:, r], minlength=k))
    # eleven labellings in one call equal each of them alone
    tree = tpg.hclust_ward(X, power=2)
    many = list(range(1, 10)) + [150, 301]
    labels = tpg.hclust_cut(tree, many)
    batch = tpg.cluster_wss(X, labels, many)
    A = np.abs(X).max()
    for r, k in enumerate(many):
        alone = tpg.cluster_wss(X, labels[:, r], [k])
        assert alone.view(np.uint64)[0] == batch.view(np.uint64)[r], k
        want = hr.wss_of_labels(X, labels[:, r], k)
        assert abs(batch[r] - want) <= 2 * kr.bound_wss(301, 4, A, want), k
    assert batch[-1] == 0.0  # k = n: every point is its own centre
    # a label out of range is refused, whichever labelling holds it
    for col, bad in ((4, many[4]), (0, -1), (10, 301)):  # (k itself is one past the last label)
        lab = labels.copy(order="F")
        lab[7, col] = bad
        with pytest.raises(tpg._lib.TpgError) as e:
            tpg.cluster_wss(X, lab, many)
        assert e.value.code == EINVAL
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.cluster_wss(X, labels[:, :1], [302])
    assert e.value.code == EINVAL
    assert np.array_equal(tpg.cluster_wss(X, labels, many).view(np.uint64), batch.view(np.uint64))


def _fake_pca(seed=11, n=120, d=4, g=3, m=257, sep=7.0):
    """three planted blobs as the scores u d of a pca dict"""
    rng = np.random.default_rng(seed)
    truth = np.arange(n) % g
    scores = rng.normal(size=(g, d))[truth] * sep + rng.normal(size=(n, d))
    dd = np.sort(np.sqrt((scores ** 2).sum(axis=0)))[::-1].copy()
    u = np.asfortranarray(scores / dd[None, :])
    return dict(u=u, d=dd, v=np.asfortranarray(rng.normal(size=(m, d)) / np.sqrt(m)), center=np.zeros(m), scale=np.ones(m)), truth


def _check_clusters(cl, scores, ks, criterion):
    n, d = scores.shape
    ref = hr.cluster_pca_ward(scores, ks, power=2 if criterion == "reference" else 1)
    A = np.abs(scores).max()
    assert cl["method"] == "ward" and cl["criterion"] == criterion and cl["k"] == list(ks)
    assert np.array_equal(cl["merge"], ref["merge"]) and np.array_equal(cl["height"].view(np.uint64), ref["height"].view(np.uint64))
    for pos, k in enumerate(ks):
        assert np.array_equal(cl["groups"][k], ref["groups"][k]), k
        assert cl["groups"][k].min() == 1 and cl["groups"][k].max() == k
        bw = 2 * kr.bound_wss(n, d, A, ref["WSS"][pos])
        assert abs(cl["WSS"][pos] - ref["WSS"][pos]) <= bw, (k, cl["WSS"][pos], ref["WSS"][pos], bw)
        # n log(W / n): a relative error e of W moves the logarithm by e (1 + e); the rest are a few roundings of the value
        for name in ("AIC", "BIC"):
            tol = n * (bw / ref["WSS"][pos]) * 1.001 + 8 * kr.EPS * (abs(n * np.log(ref["WSS"][pos] / n)) + np.log(n) * k)
            assert abs(cl[name][pos] - ref[name][pos]) <= tol, (name, k)
    return ref


def test_gt_cluster_pca_ward_on_blobs_follows_the_restatement():
    import tidypopgen_amd as tpg

    pca, truth = _fake_pca()
    scores = np.asfortranarray((pca["u"] * pca["d"][None, :])[:, :4])
    for criterion in ("reference", "ward"):
        out = tpg.gt_cluster_pca_ward(pca, k_clusters=(1, 6), criterion=criterion)
        cl = out["clusters"]
        assert out["u"] is pca["u"] and cl["n_pca"] == 4
        _check_clusters(cl, scores, range(1, 7), criterion)
        # the planted blobs come back at k = 3; k = 1 is the total sum of squares about the column means
        assert len(set(zip(cl["groups"][3].tolist(), truth.tolist()))) == 3
        tot = ((scores - scores.mean(axis=0)) ** 2).sum()
        assert (cl["groups"][1] == 1).all() and abs(cl["WSS"][0] - tot) <= 2 * kr.bound_wss(120, 4, np.abs(scores).max(), tot) + 1e-13 * tot
        # gt_cluster_pca_best_k and gt_dapc run on it unchanged
        best = tpg.gt_cluster_pca_best_k(out, stat="BIC", criterion="diffNgroup")
        assert best["best_k"] == kr.best_k(cl["BIC"], "diffNgroup") == 3
        dapc = tpg.gt_dapc(best)
        assert dapc["n.da"] == 2 and np.array_equal(dapc["grp"], cl["groups"][3]) and np.array_equal(dapc["assign"], cl["groups"][3])
    # fewer components, a single k
    one = tpg.gt_cluster_pca_ward(pca, n_pca=2, k_clusters=3)["clusters"]
    assert one["n_pca"] == 2 and one["criterion"] == "reference"
    _check_clusters(one, np.asfortranarray(scores[:, :2]), [3], "reference")
    # the default range is 1 .. round(n / 10)
    dflt = tpg.gt_cluster_pca_ward(pca)["clusters"]
    assert dflt["k"] == list(range(1, 13)) and len(dflt["BIC"]) == 12
    _check_clusters(dflt, scores, range(1, 13), "reference")
    with pytest.raises(ValueError):
        tpg.gt_cluster_pca_ward(pca, criterion="ward.D")
    with pytest.raises(ValueError):
        tpg.gt_cluster_pca_ward(pca, k_clusters=(1, 2, 3))
    # the switch of gt_cluster_pca is not forwarded yet
    with pytest.raises(NotImplementedError, match="gt_cluster_pca_ward"):
        tpg.gt_cluster_pca(pca, method="ward")
