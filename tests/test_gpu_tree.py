"""GPU: tpg_hclust_dist, tpg_nj and the drivers gt_hclust / gt_nj (include/tpg.h "Trees from a pairwise matrix") against the numpy
restatement tests/tree_ref.py.

What is compared how.  Both trees are pure functions of the strict lower triangle of the matrix, stated operation by operation in
the header, so the device's merge and join lists equal the brute-force restatement's slot for slot and the heights, branch
lengths and last bit for bit -- on tie-free Euclidean matrices at sizes around a wave, a 256-thread block, the 512 entries one
pass of the neighbour-joining row scan covers and the 1024-thread pick block, and on matrices made of ties.  Neighbour-joining on
an additive tree returns the tree's path lengths exactly, with no restatement in between."""
import ctypes as C

import numpy as np
import pytest

from tests import hclust_ref as hr
from tests import tree_ref as tr

pytestmark = pytest.mark.gpu

EINVAL, ENUMERIC = 1, 4  # TPG_EINVAL, TPG_ENUMERIC


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _same_linkage(got, D, method):
    want = tr.linkage_shared(D, method)
    n = D.shape[0]
    assert got["n"] == n and got["method"] == method and len(got["merge_a"]) == len(got["merge_b"]) == len(got["height"]) == n - 1
    first = np.nonzero((got["merge_a"] != want["merge_a"]) | (got["merge_b"] != want["merge_b"]) | (_bits(got["height"]) != _bits(want["height"])))[0]
    assert len(first) == 0, (first[0], got["merge_a"][first[0]], got["merge_b"][first[0]], got["height"][first[0]],
                             want["merge_a"][first[0]], want["merge_b"][first[0]], want["height"][first[0]])
    assert np.array_equal(got["merge"], hr.r_merge(n, want["merge_a"], want["merge_b"]))
    assert np.array_equal(got["order"], tr.order(n, want["merge_a"], want["merge_b"]) + 1)


def _same_nj(got, want):
    n = want["n"]
    assert got["n"] == n and len(got["join_a"]) == len(got["join_b"]) == len(got["len_a"]) == len(got["len_b"]) == max(n - 2, 0)
    first = np.nonzero((got["join_a"] != want["join_a"]) | (got["join_b"] != want["join_b"]) | (_bits(got["len_a"]) != _bits(want["len_a"]))
                       | (_bits(got["len_b"]) != _bits(want["len_b"])))[0]
    assert len(first) == 0, (first[0], got["join_a"][first[0]], got["join_b"][first[0]], got["len_a"][first[0]], got["len_b"][first[0]],
                             want["join_a"][first[0]], want["join_b"][first[0]], want["len_a"][first[0]], want["len_b"][first[0]])
    assert np.array_equal(_bits(got["last"]), _bits(want["last"])), (got["last"], want["last"])


@pytest.mark.parametrize("method", tr.METHODS)
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257, 301, 1025])
def test_linkage_equals_the_restatement_merge_for_merge(n, method):
    import tidypopgen_amd as tpg

    D = tr.blob_matrix(n)
    got = tpg.hclust_dist(D, method)
    if n == 1:
        assert got["n"] == 1 and len(got["merge_a"]) == len(got["height"]) == 0 and got["merge"].shape == (0, 2) and got["order"].tolist() == [1]
        assert tpg.hclust_cut(got, [1]).tolist() == [[0]]
        return
    _same_linkage(got, D, method)
    assert np.array_equal(tpg.hclust_cut(got, [2])[:, 0], hr.cut(n, got["merge_a"], got["merge_b"], 2))


@pytest.mark.parametrize("method", tr.METHODS)
@pytest.mark.parametrize("name", ["axis_star", "lattice_euclid", "lattice_manhattan", "zeros"])
def test_linkage_on_matrices_made_of_ties(name, method):
    import tidypopgen_amd as tpg

    D = tr.tie_matrices()[name]
    assert D.shape[0] == {"axis_star": 129, "lattice_euclid": 69, "lattice_manhattan": 69, "zeros": 40}[name]
    _same_linkage(tpg.hclust_dist(D, method), D, method)


# 511 .. 515: one pass of the row scan covers 256 pairs of columns
@pytest.mark.parametrize("n", [2, 3, 4, 5, 63, 64, 65, 129, 257, 301, 511, 512, 513, 514, 515, 1025])
def test_nj_equals_the_restatement_bit_for_bit(n):
    import tidypopgen_amd as tpg

    D = tr.blob_matrix(n)
    _same_nj(tpg.nj(D), tr.nj_shared(D))


@pytest.mark.parametrize("name", ["lattice_euclid", "lattice_manhattan", "zeros"])
def test_nj_on_matrices_made_of_ties(name):
    import tidypopgen_amd as tpg

    D = tr.tie_matrices()[name]
    _same_nj(tpg.nj(D), tr.nj_shared(D))


def test_nj_returns_an_additive_tree_exactly():
    import tidypopgen_amd as tpg

    D = tr.additive_tree(257, seed=257)
    t = tpg.nj(D)
    assert np.array_equal(tr.path_lengths(t), D)
    e = tpg.nj_edges(t)
    assert e["Nnode"] == 255 and e["edge"].shape == (511, 2) and (e["edge_length"] > 0).all()
    assert tpg.nj_newick(t).count(",") == 256


def test_only_the_strict_lower_triangle_is_read_and_it_must_be_finite():
    import tidypopgen_amd as tpg

    ctx = tpg.default_context()
    D = tr.blob_matrix(65)
    M = np.asfortranarray(D.copy())
    M[np.triu_indices(65)] = np.nan  # the upper triangle and the diagonal
    for method in ("complete", "average"):
        _same_linkage(tpg.hclust_dist(M, method), D, method)
    _same_nj(tpg.nj(M), tr.nj_shared(D))
    # an asymmetric matrix: the tree of its lower triangle
    A = np.asfortranarray(np.tril(D, -1) + np.triu(D, 1) * 3.0)
    _same_linkage(tpg.hclust_dist(A, "single"), D, "single")
    lib = tpg._lib.lib
    for bad in (np.nan, np.inf, -np.inf):
        for i, j in ((64, 0), (1, 0), (64, 63), (33, 17)):
            B = np.asfortranarray(D.copy())
            B[i, j] = bad
            ma, mb, h = np.full(64, -7, dtype=np.int32), np.full(64, -7, dtype=np.int32), np.full(64, -7.0)
            rc = lib.tpg_hclust_dist(ctx.h, C.c_void_p(B.ctypes.data), 65, 1, C.c_void_p(ma.ctypes.data), C.c_void_p(mb.ctypes.data), C.c_void_p(h.ctypes.data))
            assert rc == ENUMERIC and (ma == -7).all() and (mb == -7).all() and (h == -7.0).all()
            la, lb, last = np.full(63, -7.0), np.full(63, -7.0), np.full(3, -7.0)
            rc = lib.tpg_nj(ctx.h, C.c_void_p(B.ctypes.data), 65, C.c_void_p(ma.ctypes.data), C.c_void_p(mb.ctypes.data), C.c_void_p(la.ctypes.data),
                            C.c_void_p(lb.ctypes.data), C.c_void_p(last.ctypes.data))
            assert rc == ENUMERIC and (ma == -7).all() and (mb == -7).all() and (la == -7.0).all() and (lb == -7.0).all() and (last == -7.0).all()
    # negative values are allowed
    N = np.asfortranarray(D - 3.0)
    _same_linkage(tpg.hclust_dist(N, "complete"), N, "complete")
    _same_nj(tpg.nj(N), tr.nj_shared(N))


def test_determinism_device_memory_and_refusals():
    import tidypopgen_amd as tpg

    ctx = tpg.default_context()
    lib, bufs = tpg._lib.lib, []
    n = 301
    D = np.asfortranarray(tr.blob_matrix(n))
    a, b = tpg.hclust_dist(D, "average"), tpg.hclust_dist(D, "average")
    for name in ("merge_a", "merge_b", "merge", "order"):
        assert np.array_equal(a[name], b[name])
    assert np.array_equal(_bits(a["height"]), _bits(b["height"]))
    ja, jb = tpg.nj(D), tpg.nj(D)
    _same_nj(jb, ja)

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

    # D and the outputs in device memory
    dd = dev(D.nbytes, D)
    d_a, d_b, d_h = dev(4 * n), dev(4 * n), dev(8 * n)
    assert lib.tpg_hclust_dist(ctx.h, dd, n, 2, d_a, d_b, d_h) == 0
    assert np.array_equal(back(d_a, np.int32, n - 1), a["merge_a"]) and np.array_equal(back(d_b, np.int32, n - 1), a["merge_b"])
    assert np.array_equal(back(d_h, np.uint64, n - 1), _bits(a["height"]))
    d_la, d_lb, d_last = dev(8 * n), dev(8 * n), dev(24)
    assert lib.tpg_nj(ctx.h, dd, n, d_a, d_b, d_la, d_lb, d_last) == 0
    got = dict(n=n, join_a=back(d_a, np.int32, n - 2), join_b=back(d_b, np.int32, n - 2), len_a=back(d_la, np.float64, n - 2),
               len_b=back(d_lb, np.float64, n - 2), last=back(d_last, np.float64, 3))
    _same_nj(got, ja)
    assert np.array_equal(back(dd, np.uint64, n * n), _bits(D).ravel(order="F"))
    for p in bufs:
        ctx.dev_free(p)
    # a DeviceMatrix passed in has the same bytes after the calls
    M = tpg.DeviceMatrix.from_numpy(D)
    for method in ("single", "ward.D", "ward.D2"):
        tpg.hclust_dist(M, method)
    _same_nj(tpg.nj(M), ja)
    assert np.array_equal(_bits(M.to_numpy()), _bits(D))
    M.free()

    Ds = np.asfortranarray(tr.blob_matrix(65))

    def refused_hclust(code, x, nn, method):
        ma, mb, h = np.full(64, -7, dtype=np.int32), np.full(64, -7, dtype=np.int32), np.full(64, -7.0)
        rc = lib.tpg_hclust_dist(ctx.h, C.c_void_p(x.ctypes.data), nn, method, C.c_void_p(ma.ctypes.data), C.c_void_p(mb.ctypes.data), C.c_void_p(h.ctypes.data))
        assert rc == code, (rc, lib.tpg_last_error())
        assert (ma == -7).all() and (mb == -7).all() and (h == -7.0).all()

    def refused_nj(code, x, nn):
        ma, mb = np.full(64, -7, dtype=np.int32), np.full(64, -7, dtype=np.int32)
        la, lb, last = np.full(64, -7.0), np.full(64, -7.0), np.full(3, -7.0)
        rc = lib.tpg_nj(ctx.h, C.c_void_p(x.ctypes.data), nn, C.c_void_p(ma.ctypes.data), C.c_void_p(mb.ctypes.data), C.c_void_p(la.ctypes.data),
                        C.c_void_p(lb.ctypes.data), C.c_void_p(last.ctypes.data))
        assert rc == code, (rc, lib.tpg_last_error())
        assert (ma == -7).all() and (mb == -7).all() and (la == -7.0).all() and (lb == -7.0).all() and (last == -7.0).all()

    refused_hclust(EINVAL, Ds, 65, 5)
    refused_hclust(EINVAL, Ds, 65, -1)
    refused_hclust(EINVAL, Ds, 0, 1)
    refused_nj(EINVAL, Ds, 0)
    # n above the limit is refused by the first checks, before any allocation: nothing of the 8 n^2 bytes is read
    refused_hclust(EINVAL, Ds, tpg.HCLUST_MAX_N + 1, 1)
    refused_nj(EINVAL, Ds, tpg.HCLUST_MAX_N + 1)
    # 3e308 overflows, every row sum is +inf, every q is inf - inf
    refused_nj(ENUMERIC, np.full((5, 5), 1e308, order="F"), 5)
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.nj(np.full((5, 5), 1e308))
    assert e.value.code == ENUMERIC
    # after a refusal the next call still runs
    _same_linkage(tpg.hclust_dist(Ds, "complete"), Ds, "complete")
    _same_nj(tpg.nj(Ds), tr.nj_shared(Ds))


def test_drivers_from_genotypes_and_from_a_matrix():
    import tidypopgen_amd as tpg

    rng = np.random.default_rng(5)
    geno = rng.integers(0, 3, size=(65, 257)).astype(np.uint8)
    geno[rng.random(size=geno.shape) < 0.03] = 3  # missing
    X = tpg.FBM.from_numpy(geno)
    D = tpg.pairwise_sqdist(X)
    off = D[~np.eye(65, dtype=bool)]
    assert np.array_equal(off, np.round(off)) and off.min() > 0  # exact integers
    _same_nj(tpg.gt_nj(X), tr.nj_shared(D))
    _same_linkage(tpg.gt_hclust(X, method="average"), D, "average")
    _same_linkage(tpg.gt_hclust(X), D, "complete")
    # a matrix of the caller's: ward.D2 is ward.D on the squared matrix with the root of its heights
    dist = 1.0 - tpg.snp_ibs(X)
    d2 = tpg.gt_hclust(dist=dist, method="ward.D2")
    d1 = tpg.gt_hclust(dist=dist ** 2, method="ward.D")
    assert d2["method"] == "ward.D2" and np.array_equal(d2["merge_a"], d1["merge_a"]) and np.array_equal(d2["merge_b"], d1["merge_b"])
    assert np.array_equal(_bits(d2["height"]), _bits(np.sqrt(d1["height"]))) and np.array_equal(d2["order"], d1["order"])
    _same_linkage(d1, dist ** 2, "ward.D")
    _same_nj(tpg.gt_nj(dist=dist), tr.nj_shared(dist))
    with pytest.raises(ValueError):
        tpg.gt_hclust(X, dist=dist)
    with pytest.raises(ValueError):
        tpg.gt_hclust(X, method="centroid")


@pytest.mark.parametrize("n", [65, 301])
def test_ward_on_the_matrix_is_ward_on_the_scores(n):
    import tidypopgen_amd as tpg

    X = hr.blobs(n + 4, n, 4)
    want = tpg.hclust_ward(X, power=1)
    got = tpg.hclust_dist(hr.start_matrix(X, 1), "ward.D")
    assert np.array_equal(got["merge_a"], want["merge_a"]) and np.array_equal(got["merge_b"], want["merge_b"])
    assert np.array_equal(_bits(got["height"]), _bits(want["height"])) and np.array_equal(got["merge"], want["merge"])
