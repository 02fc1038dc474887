"""CPU: the numpy restatement of include/tpg.h "Ward clustering on PCA scores" (tests/hclust_ref.py) against an independent
implementation (scipy's linkage), against the identity that ties Ward's heights to the within-group sum of squares, and on
examples written out by hand; the restatement's own fused multiply-add against rationals; and the library's cut and merge matrix
(csrc/host/host_hclust.h), through the C ABI and as a stand-alone program under the host sanitizers, against the restatement."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import hclust_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 1), (3, 1), (63, 3), (65, 17), (301, 4)]


def same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def test_the_restatements_fma_is_correctly_rounded():
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=3000), rng.normal(size=3000)
    c = rng.normal(size=3000) * rng.choice([1.0, 1e-8, 1e8, 0.0], 3000)
    c[:500] = -(a[:500] * b[:500])  # cancellation: the result is the product's rounding error
    got = hr.fma(a, b, c)
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got, want)
    assert (a * b + c != got).sum() > 100  # (the unfused expression is another function: the check can fail)


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("n,d", SHAPES)
def test_restatement_against_scipy_at_every_k(n, d, power):
    sch = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import pdist

    X = hr.blobs(n + d, n, d)
    t = hr.ward_shared(X, power)
    # scipy applies the recurrence to y^2 and returns the root: pdist(x)^2 is the reference's computation, pdist(x) the proper one
    Z = sch.linkage(pdist(X) ** power, "ward")
    mine, theirs = np.sort(np.sqrt(t["height"])), np.sort(Z[:, 2])
    worst = float(np.max(np.abs(mine - theirs) / theirs))
    print("n", n, "d", d, "power", power, "worst relative height difference", worst)
    assert worst <= 1e-12
    # scipy's partition at k: the first n - k rows of Z applied one after the other (row s forms cluster n + s)
    theirs, ident = np.arange(n), {i: i for i in range(n)}
    for k in range(n, 0, -1):
        assert same_partition(hr.cut(n, t["merge_a"], t["merge_b"], k), theirs), k
        if k > 1:
            s = n - k
            u, v = ident.pop(int(Z[s, 0])), ident.pop(int(Z[s, 1]))
            theirs = np.where(theirs == v, u, theirs)
            ident[n + s] = u
    assert same_partition(theirs, sch.cut_tree(Z, n_clusters=1).ravel())
    assert np.all(np.diff(t["height"]) >= 0)  # tie-free inputs: the heights do not fall


@pytest.mark.parametrize("n,d", [(301, 4), (1025, 3)])
def test_power_1_heights_are_twice_the_growth_of_the_wss(n, d):
    # Ward's criterion on d^2: the height of a merge is twice the growth of the within-group sum of squares it causes, so
    # WSS(k) = 1/2 sum of the first n - k heights
    X = hr.blobs(n + d, n, d)
    t = hr.ward_shared(X, 1)
    total = hr.wss_of_labels(X, np.zeros(n, dtype=np.int32), 1)
    for k in (1, 2, 3, 7, 50, n - 1, n):
        w = hr.wss_of_labels(X, hr.cut(n, t["merge_a"], t["merge_b"], k), k)
        half = 0.5 * float(np.sum(t["height"][:n - k]))
        print("n", n, "k", k, "relative gap", abs(w - half) / total)
        assert abs(w - half) <= 1e-12 * total


# six points on a line: 0, 1 | 4, 5 | 10 | 20.  Squared distances: (0,1) = 1 and (2,3) = 1 tie, the smaller a goes first.
# step 1: slots 0, 1 (two singletons)            -> R row (-1, -2)
# step 2: slots 2, 3 (two singletons)            -> R row (-3, -4)
# step 3: {0,1} with {2,3}: 2 (n_a n_b / (n_a + n_b)) (distance of the centres)^2 = 2 (4 / 4) 4^2 = 32 against {2,3} with 10:
#         2 (2 / 3) 5.5^2 = 40.3 -> slots 0, 2,
#         a cluster with a cluster: the earlier step first -> R row (1, 2)
# step 4: {0,1,2,3} (centre 2.5) with 10: 2 (4 / 5) 7.5^2 = 90 against 10 with 20: 2 (1 / 2) 10^2 = 100 -> slots 0, 4, a singleton with a
#         cluster: the singleton first -> R row (-5, 3)
# step 5: the rest with 20 -> slots 0, 5 -> R row (-6, 4)
HAND_X = np.array([[0.0], [1.0], [4.0], [5.0], [10.0], [20.0]])
HAND_A, HAND_B = [0, 2, 0, 0, 0], [1, 3, 2, 4, 5]
HAND_MERGE = [[-1, -2], [-3, -4], [1, 2], [-5, 3], [-6, 4]]
HAND_CUTS = {6: [0, 1, 2, 3, 4, 5], 5: [0, 0, 1, 2, 3, 4], 4: [0, 0, 1, 1, 2, 3], 3: [0, 0, 0, 0, 1, 2], 2: [0, 0, 0, 0, 0, 1],
             1: [0, 0, 0, 0, 0, 0]}


def test_hand_example_merges_cut_numbering_and_r_merge():
    t = hr.ward(HAND_X, 1)
    assert t["merge_a"].tolist() == HAND_A and t["merge_b"].tolist() == HAND_B
    assert t["height"][:2].tolist() == [1.0, 1.0]  # (the later ones pass through thirds: not exact)
    assert t["height"].tolist() == pytest.approx([1.0, 1.0, 32.0, 90.0, 2 * 5 / 6 * 16.0 ** 2], rel=1e-14)
    assert hr.r_merge(6, HAND_A, HAND_B).tolist() == HAND_MERGE
    for k, want in HAND_CUTS.items():
        assert hr.cut(6, HAND_A, HAND_B, k).tolist() == want
    # the numbering goes by first appearance in ascending i, not by the order of the merges: (1, 3) merges before (0, 2)
    assert hr.cut(4, [1, 0], [3, 2], 2).tolist() == [0, 1, 0, 1]
    assert hr.cut(4, [1, 0], [3, 2], 3).tolist() == [0, 1, 2, 1]


def test_tie_rule_on_collinear_points():
    # 0, 1, 2, 3: three pairs at distance 1; (0, 1) is first in the order (a, b).  Then (2, 3) at 1 beats {0,1}-2 at
    # ((1 + 1) 4 + (1 + 1) 1 - 1) / 3 = 3
    for power in (1, 2):
        t = hr.ward(np.arange(4.0)[:, None], power)
        assert t["merge_a"].tolist() == [0, 2, 0] and t["merge_b"].tolist() == [1, 3, 2]
    t = hr.ward(np.arange(4.0)[:, None], 1)
    assert t["height"].tolist() == pytest.approx([1.0, 1.0, 8.0], rel=1e-14)  # {0,1} with {2,3}: 2 (2 * 2 / 4) 2^2
    # copies of one point: every S is 0, the smallest slots merge: (0, 1), (0, 2), ...
    t = hr.ward(hr.copies(5), 2)
    assert t["merge_a"].tolist() == [0] * 4 and t["merge_b"].tolist() == [1, 2, 3, 4] and not t["height"].any()


def _trees():
    out = [(hr.lattice(), 2)]
    for seed, (n, d) in enumerate([(17, 2), (64, 3), (130, 5)]):
        out.append((hr.blobs(100 + seed, n, d), 1 + seed % 2))
    return [(X.shape[0], hr.ward_shared(X, power)) for X, power in out]


def test_library_cut_and_r_merge_need_no_device():
    import tidypopgen_amd as tpg

    for n, t in _trees():
        tree = dict(n=n, merge_a=t["merge_a"], merge_b=t["merge_b"])
        ks = [1, 2, 3, n // 2, n - 1, n]
        lab = tpg.hclust_cut(tree, ks)
        assert lab.shape == (n, len(ks)) and lab.dtype == np.int32
        for r, k in enumerate(ks):
            assert np.array_equal(lab[:, r], hr.cut(n, t["merge_a"], t["merge_b"], k)), (n, k)
        merge = np.zeros((n - 1, 2), dtype=np.int32, order="F")
        tpg._lib.check(tpg._lib.lib.tpg_hclust_r_merge(n, t["merge_a"].ctypes.data, t["merge_b"].ctypes.data, merge.ctypes.data))
        assert np.array_equal(merge, hr.r_merge(n, t["merge_a"], t["merge_b"]))
    tree = dict(n=6, merge_a=np.array(HAND_A, dtype=np.int32), merge_b=np.array(HAND_B, dtype=np.int32))
    assert tpg.hclust_cut(tree, [3]).ravel().tolist() == HAND_CUTS[3]
    for bad_k in ([0], [7]):
        with pytest.raises(tpg._lib.TpgError) as e:
            tpg.hclust_cut(tree, bad_k)
        assert e.value.code == 1
    for a, b in (([0, 2, 0, 1, 0], HAND_B),      # step 4 names slot 1, dead since step 1
                 ([0, 2, 0, 0, 0], [1, 3, 2, 4, 4]),  # slot 4 merged away twice
                 ([1, 2, 0, 0, 0], [1, 3, 2, 4, 5]),  # a = b
                 ([0, 2, 0, 0, 0], [1, 3, 2, 4, 6])):  # outside [0, n)
        with pytest.raises(tpg._lib.TpgError) as e:
            tpg.hclust_cut(dict(n=6, merge_a=a, merge_b=b), [2])
        assert e.value.code == 1
    with pytest.raises(NotImplementedError, match="gt_cluster_pca_ward"):
        tpg.gt_cluster_pca(dict(u=np.zeros((4, 1)), d=np.ones(1)), method="ward")
    # a range of k the WSS call would refuse is refused before the tree is built (no device is touched here): the default range
    # at n = 10 246 reaches 1025, and k > n
    for n, kc in ((10246, None), (30, (1, 31))):
        with pytest.raises(ValueError, match="the largest k the WSS is summed for"):
            tpg.gt_cluster_pca_ward(dict(u=np.zeros((n, 1)), d=np.ones(1)), k_clusters=kc)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_library_cut_and_r_merge_stand_alone_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "hclust_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc"), os.path.join(ROOT, "tests", "host", "hclust_san.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    cases = []
    for n, t in _trees():
        cases.append((n, [1, 2, 3, n // 2, n - 1, n], t["merge_a"].tolist(), t["merge_b"].tolist()))
    cases.append((1, [1], [], []))
    cases.append((6, [2], [0, 2, 0, 1, 0], HAND_B))  # names a dead slot: refused
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"{n} {len(ks)}\n{' '.join(map(str, ks))}\n{' '.join(map(str, a))}\n{' '.join(map(str, b))}\n"
                            for n, ks, a, b in cases))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok hclust"
    at = 0
    for n, ks, a, b in cases[:-1]:
        for k in ks:
            assert [int(v) for v in lines[at].split()[1:]] == hr.cut(n, a, b, k).tolist() and lines[at].startswith("labels"), (n, k)
            at += 1
        want = hr.r_merge(n, a, b).ravel(order="F").tolist() if n > 1 else []
        assert lines[at].startswith("merge") and [int(v) for v in lines[at].split()[1:]] == want, n
        at += 1
    assert lines[at] == "refused 1 1" and at + 2 == len(lines)
