"""GPU: the batched k-means (include/tpg.h "k-means on PCA scores") against the numpy restatement tests/kmeans_ref.py.

What is compared how.  One step on small integer coordinates, where every distance is exact: labels and counts equal the exact
route (planted ties go to the smaller index, a centre that owns nothing stays and is counted), the new centres and wss lie within
the header's bounds of the exact values.  The start rows: bit for bit.  Whole runs on Gaussian blobs: the restatement runs from
the same start and records the smallest relative gap between a point's best and second-best distance over all its iterations;
that gap must exceed 1e-9 ON THE RESTATEMENT (a relative error of (d + 2) 2^-52 < 1.5e-14 per distance cannot flip such a
label), and then labels, n_iter, converged and n_empty are equal and centres and wss lie within twice the bounds.  Batches: every
output of a run is the same bits alone and among eleven others, and from call to call.

Shapes: n = 1, 63, 64, 65, 301 around the tile of 256 points and the wave of 64; d = 1, 3, 17, 64 in each register bucket of the
assign kernel; k = 1, 2, 7, 65; and k d at, and one centre past, the LDS chunk the library reports."""
import numpy as np
import pytest

from tests import kmeans_ref as kr

pytestmark = pytest.mark.gpu

EINVAL, ENUMERIC = 1, 4


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _chunk():
    import tidypopgen_amd as tpg

    return tpg.KMEANS_CHUNK_DOUBLES


def _int_points(seed, n, d, k):
    """integer points and integer centres with a planted tie and a centre that owns nothing"""
    rng = np.random.default_rng(seed)
    X = rng.integers(-8, 9, size=(n, d)).astype(np.float64)
    C = X[rng.permutation(n)[:k]].copy()
    if k >= 3:
        C[k - 1] = C[0]       # equal distances to 0 and k - 1 for every point: k - 1 never wins
        C[k - 2] = 1000.0     # owns nothing
    return X, C


# (n, d, k); "edge" = floor(chunk / d) centres, exactly one LDS chunk; "edge+1" needs a second chunk
STEP_SHAPES = [(1, 1, 1), (63, 3, 2), (64, 17, 7), (65, 64, 65), (301, 1, 7), (301, 3, 65), (301, 17, 2), (301, 64, "edge"),
               (301, 64, "edge+1"), (301, 17, "edge"), (301, 17, "edge+1")]


def _k(k, d):
    if k == "edge":
        return _chunk() // d
    if k == "edge+1":
        return _chunk() // d + 1
    return k


@pytest.mark.parametrize("n,d,k", STEP_SHAPES)
def test_step_equals_the_exact_route_on_integer_points(n, d, k):
    import tidypopgen_amd as tpg

    k = _k(k, d)
    assert k <= n
    X, C = _int_points(1000 + n + d + k, n, d, k)
    r = tpg.kmeans_step(X, C)
    labels, counts, cen, wss = kr.step_exact(X, C)
    assert np.array_equal(r["labels"], labels)
    assert np.array_equal(r["counts"], counts) and counts.sum() == n
    if k >= 3:
        assert counts[k - 1] == 0 and counts[k - 2] == 0
    A = np.abs(X).max()
    worst = 0.0
    for c in range(k):
        if cen[c] is None:
            assert np.array_equal(_bits(r["centers"][c]), _bits(C[c]))  # it stays put, to the bit
        else:
            worst = max(worst, max(abs(float(cen[c][j]) - r["centers"][c, j]) for j in range(d)))
    bc, bw = kr.bound_centre(n, A), (n + d + 2) * kr.EPS * float(wss)
    print("step", (n, d, k), "centre error", worst, "bound", bc, "wss error", abs(r["wss"] - float(wss)), "bound", bw)
    assert worst <= bc
    assert abs(r["wss"] - float(wss)) <= bw
    # and the restatement, which the whole runs below lean on, agrees with both
    ref = kr.step(X, C)
    assert np.array_equal(ref["labels"], labels) and np.abs(ref["centers"] - r["centers"]).max() <= 2 * bc


def test_start_rows_equal_the_restatement_and_are_what_iteration_0_uses():
    import tidypopgen_amd as tpg

    for seed, n, k in [(0, 1, 1), (1, 63, 7), (2, 64, 64), (0xDEADBEEFCAFEF00D, 65, 2), (7, 301, 65), ((1 << 64) - 1, 5000, 500)]:
        assert np.array_equal(tpg.kmeans_start(seed, n, k), kr.start(seed, n, k)), (seed, n, k)
    # one iteration of a batch from the seeds = one step from the restatement's start rows (integer points: exact distances)
    X, _ = _int_points(5, 301, 3, 2)
    ks, seeds = [1, 2, 7, 65], [11, 0xDEADBEEFCAFEF00D, 13, (1 << 64) - 1]
    b = tpg.kmeans_batch(X, ks, seeds, max_iter=1)
    for r, (k, seed) in enumerate(zip(ks, seeds)):
        s = tpg.kmeans_step(X, X[kr.start(seed, 301, k)])
        assert np.array_equal(b["labels"][:, r], s["labels"]) and np.array_equal(b["labels"][:, r], kr.assign(X, X[kr.start(seed, 301, k)])[0])
        assert np.array_equal(_bits(b["centers"][r]), _bits(s["centers"]))
        assert b["n_iter"][r] == 1 and not b["converged"][r]


def _blobs(seed, n, d, g=3, sep=6.0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(g, d))[np.arange(n) % g] * sep + rng.normal(size=(n, d))


RUN_SHAPES = [(1, 1, 1), (63, 1, 2), (64, 3, 7), (65, 17, 2), (65, 64, 65), (301, 3, 7), (301, 17, 65), (301, 64, 7), (301, 64, "edge+1"),
              (301, 1, 65)]


@pytest.mark.parametrize("n,d,k", RUN_SHAPES)
def test_whole_runs_follow_the_restatement_label_for_label(n, d, k):
    import tidypopgen_amd as tpg

    k = _k(k, d)
    X = _blobs(2000 + n + d + k, n, d)
    seeds = [3, 0xDEADBEEFCAFEF00D]
    refs = [kr.run(X, k, seed=s) for s in seeds]
    for ref in refs:
        assert ref["min_gap"] > 1e-9, ref["min_gap"]  # on the restatement: otherwise the data seed changes, never this threshold
        assert ref["converged"]
    b = tpg.kmeans_batch(X, [k] * len(seeds), seeds)
    A = np.abs(X).max()
    for r, ref in enumerate(refs):
        assert np.array_equal(b["labels"][:, r], ref["labels"])
        assert (b["n_iter"][r], bool(b["converged"][r]), b["n_empty"][r]) == (ref["n_iter"], ref["converged"], ref["n_empty"])
        ec, ew = np.abs(b["centers"][r] - ref["centers"]).max(), abs(b["wss"][r] - ref["wss"])
        bc, bw = 2 * kr.bound_centre(n, A), 2 * kr.bound_wss(n, d, A, ref["wss"])
        print("run", (n, d, k), "iterations", ref["n_iter"], "min gap", ref["min_gap"], "centre error", ec, "bound", bc, "wss error", ew, "bound", bw)
        assert ec <= bc and ew <= bw


def test_a_run_that_hits_max_iter_stops_after_its_update():
    import tidypopgen_amd as tpg

    X = np.random.default_rng(8).normal(size=(301, 3))  # no structure: slow to converge
    ref = kr.run(X, 7, seed=5, max_iter=3)
    assert not ref["converged"] and ref["n_iter"] == 3 and ref["min_gap"] > 1e-9
    b = tpg.kmeans_batch(X, [7], [5], max_iter=3)
    assert np.array_equal(b["labels"][:, 0], ref["labels"]) and b["n_iter"][0] == 3 and not b["converged"][0]
    A = np.abs(X).max()
    assert np.abs(b["centers"][0] - ref["centers"]).max() <= 2 * kr.bound_centre(301, A)
    assert abs(b["wss"][0] - ref["wss"]) <= 2 * kr.bound_wss(301, 3, A, ref["wss"])
    # the centres that came back are the means of the labels that came back: one more step moves no centre by more than rounding
    s = kr.update(X, b["labels"][:, 0], b["centers"][0])[0]
    assert np.abs(s - b["centers"][0]).max() <= 2 * kr.bound_centre(301, A)


def test_a_centre_that_never_owns_a_point_stays_put_through_a_whole_run_and_is_counted():
    import tidypopgen_amd as tpg

    X = _blobs(21, 301, 3)
    c0 = np.concatenate([X[kr.start(4, 301, 3)], [[500.0, -500.0, 500.0]], X[kr.start(4, 301, 5)][3:]])  # k = 6, centre 3 far away
    ref = kr.run(X, 6, centers0=c0)
    assert ref["converged"] and ref["n_empty"] == 1 and ref["min_gap"] > 1e-9
    b = tpg.kmeans_batch(X, [6], centers0=[c0])
    assert np.array_equal(b["labels"][:, 0], ref["labels"])
    assert (b["n_iter"][0], bool(b["converged"][0]), b["n_empty"][0]) == (ref["n_iter"], True, 1)
    assert np.array_equal(_bits(b["centers"][0][3]), _bits(c0[3]))
    assert np.abs(b["centers"][0] - ref["centers"]).max() <= 2 * kr.bound_centre(301, np.abs(X).max())


def test_a_run_does_not_depend_on_its_batch_and_two_calls_give_the_same_bits():
    import tidypopgen_amd as tpg

    X = _blobs(77, 301, 3, sep=8.0)
    ks = [1, 2, 3, 3, 7, 7, 20, 65, 2, 3, 65, 1]
    seeds = [kr.run_seed(9, k, t) for t, k in enumerate(ks)]
    max_iter = 3
    refs = [kr.run(X, k, seed=s, max_iter=max_iter) for k, s in zip(ks, seeds)]
    # the mix the test is about, established on the restatement: some runs are done at iteration 2, some hit max_iter
    assert sum(r["converged"] and r["n_iter"] == 2 for r in refs) >= 2 and sum(not r["converged"] for r in refs) >= 2
    names = ("labels", "wss", "n_iter", "converged", "n_empty")
    whole = tpg.kmeans_batch(X, ks, seeds, max_iter=max_iter)
    again = tpg.kmeans_batch(X, ks, seeds, max_iter=max_iter)
    for name in names:
        assert np.array_equal(_bits(whole[name]), _bits(again[name])), name
    for r in range(len(ks)):
        assert np.array_equal(_bits(whole["centers"][r]), _bits(again["centers"][r]))
        one = tpg.kmeans_batch(X, [ks[r]], [seeds[r]], max_iter=max_iter)
        assert np.array_equal(one["labels"][:, 0], whole["labels"][:, r]), r
        assert np.array_equal(_bits(one["centers"][0]), _bits(whole["centers"][r])), r
        for name in names[1:]:
            assert np.array_equal(_bits(one[name][:1]), _bits(whole[name][r:r + 1])), (name, r)
        assert (whole["n_iter"][r], bool(whole["converged"][r])) == (refs[r]["n_iter"], refs[r]["converged"]), r
    # given start centres in the seeds' place: the same run, to the bit
    c0 = [X[kr.start(s, 301, k)] for k, s in zip(ks, seeds)]
    given = tpg.kmeans_batch(X, ks, centers0=c0, max_iter=max_iter)
    assert np.array_equal(given["labels"], whole["labels"]) and np.array_equal(_bits(given["wss"]), _bits(whole["wss"]))


def test_argument_errors():
    import tidypopgen_amd as tpg

    X = _blobs(1, 65, 3)

    def refused(code, *args, **kw):
        with pytest.raises(tpg._lib.TpgError) as e:
            tpg.kmeans_batch(*args, **kw)
        assert e.value.code == code, str(e.value)

    refused(EINVAL, X, [66], [0])                      # k > n
    refused(EINVAL, X, [0], [0])
    refused(EINVAL, X, [2], [0], max_iter=0)
    refused(EINVAL, np.zeros((65, 65)), [2], [0])      # d over the limit
    refused(EINVAL, np.zeros((1100, 1)), [1025], [0])  # k over the limit
    Xn = X.copy()
    Xn[64, 2] = np.nan
    refused(ENUMERIC, Xn, [2], [0])
    Xn[64, 2] = np.inf
    refused(ENUMERIC, Xn, [2], [0])
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.kmeans_step(X, np.zeros((66, 3)))
    assert e.value.code == EINVAL
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.kmeans_start(0, 5, 6)
    assert e.value.code == EINVAL
    # after a refusal the next call still runs
    assert tpg.kmeans_batch(X, [2], [0])["converged"][0]
