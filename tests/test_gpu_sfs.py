"""GPU: site frequency spectra (include/tpg.h "site frequency spectra") against the restatement tests/sfs_ref.py.

What is compared how.  n_used1 and n_used2 are integers: equality in every cell.  With full-size projection every term of a
spectrum is 0 or 1: sfs and jsfs equal the integer histograms of the float route bit for bit.  Projected, every cell against
the exact rational route within (18 n + L + 80) 2^-53, relatively (n the largest projection size, L the block's length: the
bound of the header, derived there, not measured), +0.0 exactly where the exact route is zero, no cell left out.  J is symmetric
bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import sfs_ref as sr

pytestmark = pytest.mark.gpu

SIZES = (1, 7, 8, 32, 33, 2)  # full widths 3, 15, 17, 65, 67, 5: either side of the 16-wide MFMA tile and the 64-wide tile
PROJ_A = (1, 5, 16, 17, 40, 3)
PROJ_B = (2, 6, 0, 20, 64, 2)   # the mixed vector: full size for one group, even sizes that v can equal
M = 1000
_CASES = {}


def _tpg():
    import tidypopgen_amd as tpg

    return tpg


def _case(name):
    """one panel, its store on the device and its count tables; made once"""
    if name not in _CASES:
        tpg = _tpg()
        sizes, m, miss, seed, plant = dict(
            main=(SIZES, M, 0.1, 41, (2, 6, 16, 20, 64, 2)), complete=(SIZES, M, 0.0, 42, None), one=((9,), 500, 0.1, 43, None),
            edge=((32, 32), 500, 0.05, 44, None), long=((3, 2), 64 * 1024 + 1, 0.02, 45, None))[name]
        codes, gid, planted = sr.panel(seed, sizes, m, miss=miss, plant_v=plant)
        G = len(sizes)
        X = tpg.FBM.from_numpy(np.asfortranarray(codes), code256=tpg.CODE_012)
        x, v = sr.group_tables(codes, gid, G)
        _CASES[name] = dict(codes=codes, gid=gid, planted=planted, X=X, v=tpg.View(X), xt=x, vt=v, G=G, m=m)
    return _CASES[name]


def _blocks(m):
    """lengths 0, 1, 3, 4, 5 (the MFMA's k = 4), C - 1, C, C + 1, 2 C + 1, two overlapping blocks, the whole view, (m, m)"""
    K = _tpg().SFS_CHUNK_LOCI
    assert K > 1
    lo, hi, at = [], [], 3
    for L in (0, 1, 3, 4, 5, K - 1, K, K + 1, 2 * K + 1):
        lo.append(at)
        hi.append(at + L)
        at += L + 2
    lo += [m // 2 - 40, m // 2 - 3, 0, m]
    hi += [m // 2 + 30, m // 2 + 90, m, m]
    assert max(hi) <= m
    return np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)


WHOLE = 11  # the block [0, m) of _blocks


def _run(cs, lo, hi, proj=None, keep=None, flip=None, joint=True, v=None, gid="case"):
    gid = cs["gid"] if isinstance(gid, str) else gid
    if cs["G"] == 1:
        gid = None
    return _tpg().sfs_blocks(cs["v"] if v is None else v, gid, cs["G"], lo, hi, proj=proj, keep=keep, flip=flip, joint=joint)


def _tables(cs, proj, keep=None, flip=None):
    n = sr.proj_sizes(cs["gid"], cs["G"], proj)
    t = sr.usable(cs["vt"], n, keep)
    return n, t, sr.counted(cs["xt"], cs["vt"], flip)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _assert_symmetric(J, tag=""):
    assert np.array_equal(_bits(J), _bits(np.transpose(J, (1, 0, 2)).copy(order="F"))), tag


def _assert_integers(cs, got, lo, hi, proj=None, keep=None, flip=None, tag=""):
    """full-size projection: the integer histograms, bit for bit"""
    n, t, x = _tables(cs, proj, keep, flip)
    assert np.array_equal(n, 2 * np.bincount(cs["gid"], minlength=cs["G"]))
    want = sr.blocks_float(sr.weights_float(x, cs["vt"], n, t), lo, hi)
    n1, n2 = sr.n_used(t, lo, hi)
    assert np.array_equal(got["n_used1"], n1) and np.array_equal(got["n_used2"], n2), tag
    assert np.array_equal(_bits(got["sfs"]), _bits(want["sfs"])), tag
    assert np.array_equal(_bits(got["jsfs"]), _bits(want["jsfs"])), tag
    _assert_symmetric(got["jsfs"], tag)
    return want, n1, n2


def _assert_exact(cs, got, lo, hi, proj, keep=None, flip=None, tag=""):
    n, t, x = _tables(cs, proj, keep, flip)
    Hint, D = sr.weights_int(x, cs["vt"], n, t)
    ex = sr.blocks_exact(Hint, D, lo, hi)
    n1, n2 = sr.n_used(t, lo, hi)
    assert np.array_equal(got["n"], n) and np.array_equal(got["offsets"], sr.offsets(n)), tag
    assert np.array_equal(got["n_used1"], n1) and np.array_equal(got["n_used2"], n2), tag
    rnd = [sr.cell_roundings(int(n.max()), int(b - a)) for a, b in zip(lo, hi)]
    w1 = sr.excess(got["sfs"], ex["sfs_num"], ex["sfs_den"], rnd)
    w2 = sr.excess(got["jsfs"], ex["jsfs_num"], ex["jsfs_den"], rnd)
    print(f"{tag} worst |got - exact| / bound: sfs {w1:.4f} jsfs {w2:.4f}")
    assert w1 <= 1.0 and w2 <= 1.0, (tag, w1, w2)
    _assert_symmetric(got["jsfs"], tag)
    return n, t


@pytest.mark.parametrize("name", ["main", "complete"])
def test_full_size_is_the_integer_histogram_bit_for_bit(name):
    cs = _case(name)
    lo, hi = _blocks(cs["m"])
    got = _run(cs, lo, hi)
    assert got["sfs"].shape == (172, len(lo)) and got["jsfs"].shape == (172, 172, len(lo))
    want, n1, n2 = _assert_integers(cs, got, lo, hi, tag=name)
    assert np.diag(n2[:, :, WHOLE]).min() > 0 and (n2[:, :, WHOLE] > 0).sum() > 20  # loci at which groups are typed in full
    assert not got["jsfs"][:, :, 0].any() and not got["sfs"][:, -1].any()  # the empty blocks
    u, g = cs["planted"]["untyped"]
    one = _run(cs, [u], [u + 1])
    assert one["n_used1"][g, 0] == 0 and not one["jsfs"][got["offsets"][g]:got["offsets"][g + 1]].any()
    a, b = cs["planted"]["mono"]
    mono = _run(cs, [a], [b])
    o = got["offsets"]
    assert all(mono["sfs"][o[k], 0] == mono["n_used1"][k, 0] for k in range(cs["G"])) and mono["sfs"].sum() == mono["n_used1"].sum()
    if name == "complete":
        assert (n1[:, WHOLE] == cs["m"] - (np.arange(cs["G"]) == g)).all()


@pytest.mark.parametrize("proj", [PROJ_A, PROJ_B], ids=["A", "B"])
def test_projected_against_the_exact_route(proj):
    cs = _case("main")
    lo, hi = _blocks(cs["m"])
    got = _run(cs, lo, hi, proj=proj)
    n, t = _assert_exact(cs, got, lo, hi, proj, tag=f"proj={proj}")
    # the reference tables hold what the case is about: per pair of groups a usable locus with v > n, a locus with v < n, and
    # a usable one with v = n (under PROJ_A, whose sizes are mostly odd, for the pairs with the full-size group)
    vt, G = cs["vt"], cs["G"]
    for g1 in range(G):
        for g2 in range(g1 + 1, G):
            both = t[:, g1] & t[:, g2]
            if n[g1] < 2 * SIZES[g1] or n[g2] < 2 * SIZES[g2]:  # (two full-size groups cannot have v > n)
                assert (both & ((vt[:, g1] > n[g1]) | (vt[:, g2] > n[g2]))).any(), (g1, g2)
            assert ((vt[:, g1] < n[g1]) | (vt[:, g2] < n[g2])).any(), (g1, g2)
            if proj == PROJ_B or n[g1] == 2 * SIZES[g1] or n[g2] == 2 * SIZES[g2]:
                assert (both & ((vt[:, g1] == n[g1]) | (vt[:, g2] == n[g2]))).any(), (g1, g2)
    if proj == PROJ_B:
        assert (n % 2 == 0).all() and all(t[j].all() and (vt[j] == n).all() for j in cs["planted"]["exact"])
    alone = _run(cs, lo, hi, proj=proj, joint=False)  # sfs without the joint spectra: the same bits
    assert set(alone) == {"sfs", "n_used1", "n", "offsets"}
    assert np.array_equal(_bits(alone["sfs"]), _bits(got["sfs"])) and np.array_equal(alone["n_used1"], got["n_used1"])


@pytest.mark.parametrize("which", ["keep", "flip", "both"])
def test_masks(which):
    cs = _case("main")
    lo, hi = _blocks(cs["m"])
    rng = np.random.default_rng(17)
    keep = (rng.random(cs["m"]) < 0.6).astype(np.uint8) if which != "flip" else None
    flip = (rng.random(cs["m"]) < 0.5).astype(np.uint8) if which != "keep" else None
    got = _run(cs, lo, hi, proj=PROJ_A, keep=keep, flip=flip)
    _assert_exact(cs, got, lo, hi, PROJ_A, keep, flip, tag=which)
    plain = _run(cs, lo, hi, proj=PROJ_A)
    assert not np.array_equal(_bits(plain["sfs"]), _bits(got["sfs"]))  # the mask bites
    full = _run(cs, lo, hi, keep=keep, flip=flip)
    _assert_integers(cs, full, lo, hi, keep=keep, flip=flip, tag=which + " full size")


def test_one_group_and_a_width_that_leaves_the_ones_alone_in_a_tile():
    cs = _case("one")
    lo, hi = _blocks(cs["m"])
    _assert_integers(cs, _run(cs, lo, hi), lo, hi, tag="G=1")
    _assert_exact(cs, _run(cs, lo, hi, proj=[5]), lo, hi, [5], tag="G=1 proj=5")
    cs = _case("edge")
    lo, hi = _blocks(cs["m"])
    got = _run(cs, lo, hi, proj=(0, 62))
    assert got["offsets"][-1] == 128  # W + 1 = 64 * 2 + 1: the column of ones is the only live one of the third tile
    _assert_exact(cs, got, lo, hi, (0, 62), tag="W=128")
    _assert_integers(cs, _run(cs, lo, hi), lo, hi, tag="W=130")
    assert _run(cs, lo[:1], hi[:1])["offsets"][-1] == 130


def test_a_cell_depends_on_its_block_alone():
    tpg = _tpg()
    cs = _case("main")
    lo, hi = _blocks(cs["m"])
    names = ("sfs", "n_used1", "jsfs", "n_used2")
    a = _run(cs, lo, hi, proj=PROJ_A)
    again = _run(cs, lo, hi, proj=PROJ_A)
    perm = np.random.default_rng(1).permutation(len(lo))
    longer = _run(cs, np.r_[lo[perm], lo[:3]], np.r_[hi[perm], hi[:3]], proj=PROJ_A)  # 16 blocks, every one at another place
    assert len(lo) + 3 == 16
    for k in names:
        assert np.array_equal(_bits(a[k]), _bits(again[k])), k
        assert np.array_equal(_bits(a[k][..., perm]), _bits(longer[k][..., :len(lo)])), k
        assert np.array_equal(_bits(a[k][..., :3]), _bits(longer[k][..., len(lo):])), k
    for b in (8, 10, WHOLE):  # alone
        one = _run(cs, lo[b:b + 1], hi[b:b + 1], proj=PROJ_A)
        for k in names:
            assert np.array_equal(_bits(one[k][..., 0]), _bits(a[k][..., b])), (k, b)
    # the individuals in another order (every group's rows permuted)
    p = np.random.default_rng(2).permutation(len(cs["gid"]))
    c = _run(cs, lo, hi, proj=PROJ_A, v=tpg.View(cs["X"], p + 1), gid=cs["gid"][p])
    for k in names:
        assert np.array_equal(_bits(a[k]), _bits(c[k])), k


def test_every_arm_of_the_split_rule():
    """a 12-wide spectrum (one tile): the smallest blocks that are cut into 1, 2 and 64 partial sums, the most the rule gives,
    over 65 537 loci; full size, so the sums are the integer histograms whatever the order of the partial sums"""
    tpg = _tpg()
    cs = _case("long")
    m, W = cs["m"], 12
    seg = tpg.sfs_segments
    L2 = next(L for L in range(1, m + 1) if seg(L, W) == 2)
    L64 = next(L for L in range(1, m + 1, 1) if seg(L, W) == 64) if seg(m, W) == 64 else None
    assert (L2, L64, seg(L2 - 1, W), seg(10 ** 9, W)) == (1025, 63 * 1024 + 1, 1, 64)  # the arms are reached, 64 is the largest
    lo = np.array([0, 7, 0, m - L64, 100], dtype=np.int64)
    hi = np.array([L2 - 1, 7 + L2, L64, m, 100 + 5 * 1024 + 3], dtype=np.int64)
    assert [seg(int(b - a), W) for a, b in zip(lo, hi)] == [1, 2, 64, 64, 6]
    got = _run(cs, lo, hi)
    assert got["offsets"][-1] == W
    _assert_integers(cs, got, lo, hi, tag="split")
    assert got["n_used2"][0, 1, 2] > 0.8 * L64
    pj = _run(cs, lo[:2], hi[:2], proj=(3, 2))  # and projected across a cut, against the exact route
    _assert_exact(cs, pj, lo[:2], hi[:2], (3, 2), tag="split, projected")


def test_S_and_theta_pi_against_tajimas_d():
    tpg = _tpg()
    cs = _case("complete")
    G, m = cs["G"], cs["m"]
    r = tpg.pop_sfs(cs["X"], None, None, cs["gid"], G)
    t = tpg.pop_tajimas_d(cs["X"], None, None, cs["gid"], G, return_sums=True)
    u, ug = cs["planted"]["untyped"]
    for g in range(G):
        if SIZES[g] < 2 or g == ug:  # (one individual: C(n, 2) of two alleles is 1 and D has no variance; the untyped locus
            continue                 # makes k_hat NaN by the Tajima section's rule)
        st = tpg.sfs_stats(r["sfs"][g])
        assert st["n"] == 2 * SIZES[g] and r["n_used"][g] == m
        assert st["S"] == t["seg"][g]
        assert abs(st["theta_pi"] - t["k_hat"][g]) <= (m + 8) * 2.0 ** -52 * t["k_hat"][g], g
    assert np.isnan(t["k_hat"][ug]) and r["n_used"][ug] == m - 1


def test_the_drivers_cut_fold_and_block():
    tpg = _tpg()
    cs = _case("main")
    G, m = cs["G"], cs["m"]
    whole = _run(cs, [0], [m], proj=PROJ_A)
    o = whole["offsets"]
    r = tpg.pop_sfs(cs["X"], None, None, cs["gid"], G, proj=PROJ_A)
    f = tpg.pop_sfs(cs["X"], None, None, cs["gid"], G, proj=PROJ_A, folded=True)
    for g in range(G):
        assert np.array_equal(_bits(r["sfs"][g]), _bits(whole["sfs"][o[g]:o[g + 1], 0]))
        assert np.array_equal(f["sfs"][g], tpg.sfs_fold(r["sfs"][g]))
    assert np.array_equal(r["n_used"], whole["n_used1"][:, 0])
    j = tpg.pairwise_pop_jsfs(cs["X"], None, None, cs["gid"], G, proj=PROJ_A)
    assert j["pairs"].shape == (2, 15) and len(j["jsfs"]) == 15
    for p, (a, b) in enumerate(j["pairs"].T - 1):
        assert np.array_equal(_bits(j["jsfs"][p]), _bits(whole["jsfs"][o[a]:o[a + 1], o[b]:o[b + 1], 0]))
        assert j["n_used"][p] == whole["n_used2"][a, b, 0]
    chrom = np.repeat([1, 2, 3], [400, 350, 250])
    jb = tpg.pairwise_pop_jsfs(cs["X"], None, None, cs["gid"], G, proj=PROJ_A, chromosome=chrom, block_size=128, folded=True)
    assert len(jb["lo"]) == 4 + 3 + 2 and jb["hi"][3] == 400 and jb["lo"][4] == 400 and jb["n_used"].shape == (15, 9)
    blk = _run(cs, jb["lo"], jb["hi"], proj=PROJ_A)
    assert np.array_equal(jb["jsfs"][6][:, :, 5], tpg.jsfs_fold(blk["jsfs"][o[1]:o[2], o[3]:o[4], 5]))
    assert np.array_equal(jb["n_used"].sum(axis=1), j["n_used"])  # disjoint blocks that cover the view


def test_scratch_and_argument_errors():
    tpg = _tpg()
    lib = tpg._lib.lib
    cs = _case("main")
    G, m = cs["G"], cs["m"]
    lo, hi = np.array([0], dtype=np.int64), np.array([m], dtype=np.int64)
    # the call checks its allocations against tpg_sfs_scratch_bytes itself (a mismatch is an error): both shapes of the plan ran
    # in the tests above; the formula does not grow with m or nb beyond its bound
    assert 0 < tpg.sfs_scratch_bytes(m, G, 172, 1, joint=False) < tpg.sfs_scratch_bytes(m, G, 172, 1) < 8 << 20
    assert tpg.sfs_scratch_bytes(10 ** 9, G, 172, 10 ** 6) < 200 << 20
    gid = np.ascontiguousarray(cs["gid"], dtype=np.int32)
    out = np.full((172, 1), 7.0, order="F")

    def call(G_=G, gid_=gid, proj=None, ploidy=None, lo_=lo, hi_=hi, nb=1):
        pj = None if proj is None else np.ascontiguousarray(proj, dtype=np.int32)
        pl = None if ploidy is None else np.ascontiguousarray(ploidy, dtype=np.float64)
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
        return lib.tpg_sfs_blocks(cs["v"].ctx.h, cs["v"].h, ptr(gid_), G_, ptr(pl), ptr(pj), None, None, ptr(lo_), ptr(hi_),
                                  C.c_int64(nb), ptr(out), None, None, None)

    EINVAL = 1
    assert call(G_=G + 1) == EINVAL  # a group nobody belongs to
    assert call(proj=(1, 5, 17, 17, 40, 3)) == EINVAL and call(proj=(1, 5, -1, 17, 40, 3)) == EINVAL  # proj outside [0, 2 N_g]
    assert call(ploidy=np.r_[1.0, np.full(len(gid) - 1, 2.0)]) == EINVAL  # diploid only
    assert call(G_=0) == EINVAL and call(gid_=np.full(len(gid), G, dtype=np.int32)) == EINVAL
    for a, b in (([5], [4]), ([0], [m + 1]), ([-1], [3])):
        assert call(lo_=np.array(a, dtype=np.int64), hi_=np.array(b, dtype=np.int64)) == EINVAL
    assert (out == 7.0).all()  # on any error the outputs are untouched
    assert call(nb=0) == 0 and (out == 7.0).all()  # nb = 0: nothing written
    assert call(ploidy=np.full(len(gid), 2.0)) == 0 and out.sum() == sr.n_used(sr.usable(cs["vt"], 2 * np.array(SIZES)), [0], [m])[0].sum()
    # W over the cap: 2049 groups cannot be, so many groups of two individuals: 1400 x (4 + 1) > 4096
    n_big = 2800
    codes = np.zeros((n_big, 8), dtype=np.uint8)
    Xb = tpg.FBM.from_numpy(np.asfortranarray(codes), code256=tpg.CODE_012)
    gb = (np.arange(n_big) // 2).astype(np.int32)
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.sfs_blocks(tpg.View(Xb), gb, 1400, [0], [8], joint=False)
    assert e.value.code == EINVAL
    ok = tpg.sfs_blocks(tpg.View(Xb), gb, 1400, [0], [8], proj=1, joint=False)  # W = 2800: fine, and every locus is x = 0
    assert ok["sfs"].shape == (2800, 1) and np.array_equal(ok["sfs"][:, 0], np.tile([8.0, 0.0], 1400))
