"""CPU: the numpy restatement of include/tpg.h "k-means on PCA scores" (tests/kmeans_ref.py) checked against itself -- the WSS
never rises, planted blobs come back, the exact route agrees, BIC has its minimum at the planted k where the formula lets it
and its elbow there otherwise, the best_k criteria and their quirks on hand-made series -- and the library's start rows (csrc/host/host_kmeans.h) as a stand-alone program under the host sanitizers,
bit for bit against the restatement."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import kmeans_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def blobs(seed=1, n=300, d=4, g=3, sep=12.0):
    rng = np.random.default_rng(seed)
    truth = np.arange(n) % g
    centres = rng.normal(size=(g, d)) * sep
    return centres[truth] + rng.normal(size=(n, d)), truth


def same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def test_wss_never_rises_from_one_iteration_to_the_next():
    rng = np.random.default_rng(0)
    X = rng.normal(size=(200, 3))  # no structure: many iterations
    for k, seed in ((2, 1), (7, 2), (20, 3)):
        r = kr.run(X, k, seed=seed, trace=True)
        tr = r["wss_trace"]
        assert r["converged"] and r["n_iter"] == len(tr) >= 3
        assert all(b <= a * (1 + 1e-14) for a, b in zip(tr, tr[1:])), tr
        assert tr[-1] < tr[0]
        assert abs(r["wss"] - tr[-1]) <= 2 * kr.bound_wss(200, 3, np.abs(X).max(), r["wss"])


def test_planted_blobs_come_back_exactly_up_to_relabelling():
    X, truth = blobs()
    ref = kr.cluster_pca(X, [3], n_start=10, seed=0)
    assert same_partition(ref["groups"][3], truth)
    assert ref["runs"][(3, ref["winner"][3])]["converged"]


BIC_D = 40


def test_bic_over_k_1_to_6_has_its_minimum_at_the_planted_3():
    """Three planted blobs, n = 300, in BIC_D = 40 dimensions; the dimension comes from the formula, not from a run.
    BIC = n log(WSS / n) + log(n) k (R/gt_cluster_pca.R:169) is free of the scale and of the separation of the blobs, so what
    decides whether it rises after the planted k is how much one more centre takes off WSS: BIC(4) > BIC(3) iff
    WSS(4) / WSS(3) > exp(-log(n) / n) = 0.9812 at n = 300.  Cutting one Gaussian blob of n / 3 = 100 points in two along its
    widest sample direction takes (2 / pi) lambda / d off that blob's sum of squares, lambda = (1 + sqrt(d / 100))^2 the largest
    eigenvalue of its sample covariance, a third of that off the total: 0.053 at d = 4 (the minimum is then at the largest k
    tried: the next test keeps that case and its elbow), 0.022 at d = 20, 0.014 at d = 40.  The minimum sits at the planted k
    once this is below 0.0188; d = 40 leaves a quarter of margin.  Two and three more centres take at most twice and three
    times as much against twice and three times the penalty."""
    n, d = 300, BIC_D
    cut = (2 / np.pi) * (1 + np.sqrt(d / (n / 3))) ** 2 / d / 3
    assert cut < 1 - np.exp(-np.log(n) / n)  # the reasoning above, for the shape used: 0.0141 < 0.0188
    X, truth = blobs(d=d)
    ref = kr.cluster_pca(X, range(1, 7), n_start=10, seed=0)
    print("BIC", ref["BIC"].tolist(), "WSS(4) / WSS(3)", ref["WSS"][3] / ref["WSS"][2], "predicted", 1 - cut)
    assert same_partition(ref["groups"][3], truth)
    assert int(np.argmin(ref["BIC"])) + 1 == 3
    assert kr.best_k(ref["BIC"], "min") == 3 and kr.best_k(ref["BIC"], "goesup") == 3


def test_bic_curve_has_its_elbow_at_the_planted_3_and_k_1_is_the_total_sum_of_squares():
    # d = 4: one more centre takes 5 % off WSS, 16 off n log(WSS / n) against a penalty of 5.7, so the curve keeps falling after
    # the planted k (BIC = 1505.0, 902.8, 425.0, 408.2, 392.5, 372.4) and bends there: the case "diffNgroup", the default, is for
    X, _ = blobs()
    ref = kr.cluster_pca(X, range(1, 7), n_start=10, seed=0)
    assert int(np.argmin(ref["BIC"])) + 1 == 6
    assert kr.best_k(ref["BIC"], "diffNgroup") == 3 and kr.best_k(ref["AIC"], "diffNgroup") == 3
    # k = 1: the total sum of squares about the column means
    tot = ((X - X.mean(axis=0)) ** 2).sum()
    assert abs(ref["WSS"][0] - tot) <= 1e-12 * tot and (ref["groups"][1] == 1).all()
    n = X.shape[0]
    assert np.array_equal(ref["AIC"], n * np.log(ref["WSS"] / n) + 2 * np.arange(1.0, 7.0))
    assert np.array_equal(ref["BIC"], n * np.log(ref["WSS"] / n) + np.log(n) * np.arange(1.0, 7.0))
    assert all(w2 < w1 for w1, w2 in zip(ref["WSS"], ref["WSS"][1:]))


def test_start_rows_are_distinct_and_nested_in_k():
    for seed in (0, 1, 0xDEADBEEFCAFEF00D):
        a = kr.start(seed, 301, 65)
        assert len(set(a.tolist())) == 65 and a.min() >= 0 and a.max() < 301
        assert np.array_equal(kr.start(seed, 301, 7), a[:7])
        h = [kr.mix64_int((seed & kr.MASK) ^ kr.mix64_int(i)) for i in range(301)]
        assert a.tolist() == sorted(range(301), key=lambda i: (h[i], i))[:65]
    assert kr.run_seed(3, 5, 2) == kr.mix64_int(3 ^ kr.mix64_int((5 << 32) + 2))


def test_exact_route_agrees_with_the_floating_point_step_including_ties_and_an_empty_centre():
    rng = np.random.default_rng(5)
    X = rng.integers(-20, 21, size=(40, 3)).astype(np.float64)
    C = X[:6].copy()
    C[4] = C[1]                  # a planted tie: centre 4 can never win against centre 1
    C[5] = [1000.0, 1000.0, 1000.0]  # owns nothing
    C[2] = C[0] + [2.0, 0.0, 0.0]
    X[7] = C[0] + [1.0, 0.0, 0.0]  # at distance 1 from centres 0 and 2, and no integer point is nearer: the smaller index wins
    r = kr.step(X, C)
    labels, counts, cen, wss = kr.step_exact(X, C)
    assert np.array_equal(r["labels"], labels) and np.array_equal(r["counts"], counts)
    assert counts[4] == 0 and counts[5] == 0 and labels[7] == 0
    assert np.array_equal(r["centers"][5], C[5]) and np.array_equal(r["centers"][4], C[4])
    A = np.abs(X).max()
    for c in range(6):
        if cen[c] is not None:
            assert max(abs(float(cen[c][j]) - r["centers"][c, j]) for j in range(3)) <= kr.bound_centre(40, A)
    assert abs(float(wss) - r["wss"]) <= (40 + 3 + 2) * kr.EPS * float(wss)


def test_tile_sum_is_the_header_order():
    e = np.random.default_rng(2).random(600)
    t = [e[:256], e[256:512], np.concatenate([e[512:], np.zeros(168)])]

    def halve(a):
        a = list(a)
        while len(a) > 1:
            h = len(a) // 2
            a = [a[i] + a[i + h] for i in range(h)]
        return a[0]

    assert kr.tile_sum(e) == (0.0 + halve(t[0]) + halve(t[1])) + halve(t[2])
    assert kr.tile_sum([3.0]) == 3.0


def test_best_k_criteria_on_hand_made_series():
    s = [10.0, 6.0, 3.0, 3.0, 4.0, 2.5, 5.0]
    assert kr.best_k(s, "min") == 6
    assert kr.best_k([5.0, 1.0, 1.0, 2.0], "min") == 2  # which.min: the first minimum
    assert kr.best_k(s, "goesup") == 4                   # the first positive difference is 3 -> 4: position 4
    with pytest.raises(ValueError):
        kr.best_k([5.0, 4.0, 3.0, 3.0], "goesup")        # never goes up
    # goodfit: the first value below min + 0.1 (max - min) = 3.25 is at position 3; the reference subtracts 1
    assert kr.best_k(s, "goodfit") == 2
    assert kr.best_k([1.0, 9.0, 9.5], "goodfit") == 0    # the quirk: position 1 gives 0
    # smoothNgoesup: the inner values become three-point means, the ends stay
    sm = [10.0, 19.0 / 3, 4.0, 10.0 / 3, 9.5 / 3, 11.5 / 3, 5.0]
    assert kr.best_k(s, "smoothNgoesup") == [i for i in range(6) if sm[i + 1] > sm[i]][0] + 1 == 5
    # diffNgroup: the differences -50, -40, -45 | -1, 0.5, -0.5 fall in two groups; the steep one ends at position 3 -> 4
    elbow = [200.0, 150.0, 110.0, 65.0, 64.0, 64.5, 64.0]
    assert kr.ward_d_two_groups(np.diff(elbow)).tolist() == [1, 1, 1, 2, 2, 2]
    assert kr.best_k(elbow, "diffNgroup") == 4


def test_ward_two_groups_against_the_centroid_form_of_wards_criterion():
    # For Ward.D on plain distances of scalars the Lance-Williams recurrence has no closed form to compare with in general, but
    # two well-separated groups must come back whatever the merge order inside them
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.normal(size=9), 50 + rng.normal(size=6)])
    p = rng.permutation(15)
    g = kr.ward_d_two_groups(x[p])
    assert same_partition(g, (p >= 9).astype(int)) and g[0] == 1
    # ties go to the first pair: 0, 1, 2 are equally spaced; (0, 1) merges first, so with k = 2 the value 2 is alone
    assert kr.ward_d_two_groups([0.0, 1.0, 2.0]).tolist() == [1, 1, 2]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_library_start_rows_stand_alone_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "kmeans_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc"), os.path.join(ROOT, "tests", "host", "kmeans_san.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    cases = [(0, 1, 1), (1, 63, 7), (2, 64, 64), (0xDEADBEEFCAFEF00D, 65, 2), (7, 301, 65), ((1 << 64) - 1, 5000, 500),
             (kr.run_seed(0, 500, 9), 5000, 1)]
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"{s:x} {n} {k}\n" for s, n, k in cases))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok kmeans" and len(lines) == len(cases) + 1
    for (s, n, k), ln in zip(cases, lines):
        assert [int(t) for t in ln.split()[1:]] == kr.start(s, n, k).tolist(), (s, n, k)


def test_library_start_rows_and_best_k_need_no_device():
    # tpg_kmeans_start is host only, and gt_cluster_pca_best_k is host-side Python: both run where no GPU is
    import tidypopgen_amd as tpg

    for seed, n, k in [(0, 1, 1), (1, 63, 7), (0xDEADBEEFCAFEF00D, 65, 2), (7, 301, 65)]:
        assert np.array_equal(tpg.kmeans_start(seed, n, k), kr.start(seed, n, k))
    assert tpg.kmeans_run_seed(3, 5, 2) == kr.run_seed(3, 5, 2)
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.kmeans_start(0, 5, 6)
    assert e.value.code == 1
    rng = np.random.default_rng(6)
    for _ in range(30):
        series = np.cumsum(rng.normal(size=rng.integers(4, 12))) * 10
        for crit in ("min", "goesup", "goodfit", "diffNgroup", "smoothNgoesup"):
            x = dict(clusters=dict(BIC=series))
            try:
                want = kr.best_k(series, crit)
            except ValueError:
                with pytest.raises(ValueError):
                    tpg.gt_cluster_pca_best_k(x, criterion=crit)
                continue
            assert tpg.gt_cluster_pca_best_k(x, criterion=crit)["best_k"] == want, (series, crit)
    with pytest.raises(NotImplementedError):
        tpg.gt_cluster_pca(dict(u=np.zeros((4, 1)), d=np.ones(1)), method="ward")
