"""GPU: Fst under relabelings (csrc/fstperm.hip, include/tpg.h "Fst under relabelings") against tests/fstperm_ref.py.

The panel is 130 individuals (the one-hot crosses the 128-individual group of the L layout) x 2 S + U + 5 loci (span and unit
borders inside, a ragged last tile), a tenth of the genotypes missing, one locus missing for a whole class of row 0.  The label
rows of tests/fstperm_ref.py::label_rows: some individuals outside (-1), a row with an empty group, a row with a group of one.
sum_num, sum_den and n_kept are compared BIT FOR BIT with the reference's ordered sums of the oracle's per-locus terms, for the
three methods; G = 2, 3, 5, 32, 33, 64 groups (slots that fill a class tile and slots that do not, one and two tiles per
relabeling) x 1, 11, 23 rows (one class group and several, up to four rounds of epilogue tasks).  With 32 groups and more the
pair list is a sample that holds the first and last groups and pairs across the two class tiles."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import fstperm_ref as fr

pytestmark = pytest.mark.gpu

N = 130
GS = (2, 3, 5, 32, 33, 64)
RS = (1, 11, 23)
METHODS = ("Hudson", "WC84", "Nei87")


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


@functools.lru_cache(maxsize=None)
def _codes():
    U, S = fr.unit_span()
    codes = fr.panel(31, N, 2 * S + U + 5)
    for G in GS:  # a locus that is missing for the whole of group 0 of row 0 (one locus per G)
        codes[_labels(G)[0] == 0, 40 + G] = fr.MISSING
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def _labels(G):
    lab = fr.label_rows(100 + G, N, G, max(RS))
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def _pairs(G):
    if G < 32:
        return np.array([(a, b) for a in range(1, G + 1) for b in range(a + 1, G + 1)], dtype=np.int32).T
    rng = np.random.default_rng(G)
    ps = {(1, 2), (1, G), (G - 1, G), (31, 32), (31, 32 + (G > 32)), (2, G)}
    while len(ps) < 40:
        a, b = sorted(int(x) for x in rng.integers(1, G + 1, size=2))
        if a != b:
            ps.add((a, b))
    return np.array(sorted(ps), dtype=np.int32).T


@functools.lru_cache(maxsize=None)
def _ref(G, method):
    """the reference of all 23 rows, computed once (a row's reference depends on the row alone)"""
    out = fr.reference(np.array(_codes()), _labels(G), G, _pairs(G), method)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def view(tpg):
    X = tpg.FBM.from_numpy(np.array(_codes()))
    v = tpg.View(X)
    yield v
    v.free()
    X.free()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("G", GS)
def test_sums_equal_the_reference_bit_for_bit(tpg, view, G, R, method):
    sn, sd, nk, fst = (a[:R] for a in _ref(G, method))
    got = tpg.fst_relabel_sums(view, _labels(G)[:R], G, _pairs(G), method)
    bad = [(r, k) for r in range(R) for k in range(sn.shape[1])
           if not (_same_bits(got["sum_num"][r, k], sn[r, k]) and _same_bits(got["sum_den"][r, k], sd[r, k]))]
    print(f"G={G} R={R} {method}: {len(bad)} of {sn.size} cells differ in bits; n_kept in [{nk.min()}, {nk.max()}]")
    assert np.array_equal(got["n_kept"], nk)
    assert not bad, bad[:10]
    assert np.array_equal(np.isnan(got["fst"]), np.isnan(fst)) and _same_bits(np.nan_to_num(got["fst"]), np.nan_to_num(fst))
    if R > 2:  # the row with an empty group: +0.0, no locus kept, NaN for every pair that names the group
        k = np.flatnonzero((_pairs(G) == G).any(axis=0))
        assert len(k) and np.all(nk[2, k] == 0)
        assert _same_bits(got["sum_num"][2, k], np.zeros(len(k))) and _same_bits(got["sum_den"][2, k], np.zeros(len(k)))
        assert np.all(np.isnan(got["fst"][2, k]))
        assert (_labels(G)[3] == 0).sum() == 1  # and the row with a group of one is among the rows compared above
    assert nk[0, 0] < _codes().shape[1]  # the planted locus is dropped by row 0's pair (1, 2): group 1 is missing there


@pytest.mark.parametrize("method", METHODS)
def test_a_row_does_not_depend_on_its_batch(tpg, view, method):
    G = 3
    lab, pairs = _labels(G), _pairs(G)
    full = tpg.fst_relabel_sums(view, lab, G, pairs, method)
    again = tpg.fst_relabel_sums(view, lab, G, pairs, method)
    rev = tpg.fst_relabel_sums(view, lab[::-1], G, pairs, method)
    for key in ("sum_num", "sum_den"):
        assert _same_bits(full[key], again[key])  # two calls: the same bits
        assert _same_bits(full[key], rev[key][::-1])  # the reversed list
    assert np.array_equal(full["n_kept"], rev["n_kept"][::-1])
    for r in (0, 2, 3, 7, 22):  # alone
        one = tpg.fst_relabel_sums(view, lab[r], G, pairs, method)
        assert _same_bits(one["sum_num"][0], full["sum_num"][r]) and _same_bits(one["sum_den"][0], full["sum_den"][r])
        assert np.array_equal(one["n_kept"][0], full["n_kept"][r])
    sub = np.ascontiguousarray(pairs[:, 1:2])  # another pair list: the pair's own cell is unchanged
    one = tpg.fst_relabel_sums(view, lab, G, sub, method)
    assert _same_bits(one["sum_num"][:, 0], full["sum_num"][:, 1]) and _same_bits(one["sum_den"][:, 0], full["sum_den"][:, 1])


def test_the_internal_batches_do_not_show(tpg, view):
    # 64 groups: one relabeling per class group, and the library walks the rows in batches of at most 512 class groups, so 515
    # rows take two batches, the second with three rows
    G = 64
    lab23, pairs = _labels(G), _pairs(G)
    small = tpg.fst_relabel_sums(view, lab23, G, pairs, "Hudson")
    lab = np.ascontiguousarray(np.concatenate([lab23] * 23)[:515])
    big = tpg.fst_relabel_sums(view, lab, G, pairs, "Hudson")
    idx = np.arange(515) % 23
    for key in ("sum_num", "sum_den"):
        assert _same_bits(big[key], small[key][idx])
    assert np.array_equal(big["n_kept"], small["n_kept"][idx])
    assert _same_bits(small["sum_num"], _ref(G, "Hudson")[0])


@pytest.mark.parametrize("method", METHODS)
def test_the_identity_row_agrees_with_the_totals_kernels(tpg, method):
    """The identity labelling (r = 0: the populations as they are) of the 60 x 600 panel of tests/fstperm_ref.py::test_panel
    against tpg_pairwise_pop_fst_sums, which adds the same terms in another order and, for Hudson and WC84, forms them by other
    algebra: 1e-12 relative on every sum, the bound tests/test_gpu_fst_reduced.py holds for re-ordered sums.

    The panel has populations because the bound is relative to the sum itself: the Hudson totals kernel forms sum_num as
    (A B')[g1,g2] + (A B')[g2,g1] - 2 (C C')[g1,g2], sums of p^2 of a few hundred, so its own rounding is a few 1e-14 ABSOLUTE
    whatever the result.  On a labelling without structure (row 0 of the G = 5 rows above: random labels, sum_num = 0.049
    against sum |num| = 6.9) that is 1.65e-12 of the result, measured, for the pair (2, 3) and below 1e-12 for the other nine;
    the new path is 2e-16 from the exact sum of the reference's terms there (it equals the ordered reference bit for bit).  That
    figure is the totals kernel's cancellation and no property of the code under test, so the comparison is made where both
    routes are well conditioned, the split pair of this panel (Fst = -0.003) included."""
    codes, gid = fr.test_panel()
    G, pairs = 4, _pairs(4)
    X = tpg.FBM.from_numpy(codes)
    v = tpg.View(X)
    ident = tpg.fst_perm_labels(len(gid), gid, G, "global", 0, 0, 0, 0)
    assert np.array_equal(ident, gid)
    got = tpg.fst_relabel_sums(v, ident, G, pairs, method)
    want = tpg.pairwise_pop_fst(X, None, None, gid, G, method=method, pairwise_combn=pairs, sums=True)
    for key in ("sum_num", "sum_den"):
        rel = np.abs(got[key][0] - want[key]) / np.abs(want[key])
        print(method, key, "largest relative difference", rel.max(), "sums", want[key])
        assert rel.max() <= 1e-12
    assert np.allclose(got["fst"][0], want["fst_tot"], rtol=1e-12, atol=0)
    v.free()
    X.free()


def _raw(tpg, view, lab, R, G, method, pairs, P, outs):
    lab = None if lab is None else np.ascontiguousarray(lab, dtype=np.int32)
    pairs_c = None if pairs is None else np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(2, -1).T)
    ptr = lambda a: C.c_void_p(None) if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    return tpg._lib.lib.tpg_fst_relabel_sums(view.ctx.h, view.h, ptr(lab), R, G, method, ptr(pairs_c), P, *[ptr(o) for o in outs])


def test_every_error_returns_its_code_and_writes_nothing(tpg, view):
    G = 3
    lab, pairs = np.array(_labels(G)[:2]), _pairs(G)
    P = pairs.shape[1]

    def outs():
        return [np.full((2, P), -7.5), np.full((2, P), -7.5), np.full((2, P), -7, dtype=np.int64)]

    def refused(rc_want, *args):
        o = outs()
        rc = _raw(tpg, view, *args, o)
        assert rc == rc_want, (rc, args[1:5])
        assert np.all(o[0] == -7.5) and np.all(o[1] == -7.5) and np.all(o[2] == -7)

    hi, lo = lab.copy(), lab.copy()
    hi[1, 5], lo[0, 129] = G, -2
    refused(1, hi, 2, G, 0, pairs, P)
    refused(1, lo, 2, G, 0, pairs, P)
    refused(1, lab, 2, G, 0, [[0], [1]], 1)
    refused(1, lab, 2, G, 0, [[1], [G + 1]], 1)
    refused(1, lab, 2, G, 0, [[2], [2]], 1)
    refused(1, lab, 2, G, 0, pairs, 0)
    refused(1, lab, -1, G, 0, pairs, P)
    refused(1, lab, 2, G, 3, pairs, P)  # no such method
    refused(1, lab, 2, 1, 0, pairs, P)
    refused(0, lab, 0, G, 0, pairs, P)  # R = 0: fine, nothing written
    # above 64 groups: refused, with a message that points to the pairwise scheme
    refused(1, np.zeros((2, N), dtype=np.int32), 2, 65, 0, [[1], [65]], 1)
    assert b"pairwise scheme" in tpg._lib.lib.tpg_last_error()
    with pytest.raises(ValueError):
        tpg.pairwise_pop_fst_test(view.X, None, None, np.arange(N) % 65, 65, scheme="global", n_perm=1)
    # n_kept may be NULL
    o = outs()
    assert _raw(tpg, view, lab, 2, G, 0, pairs, P, [o[0], o[1], None]) == 0
    assert _same_bits(o[0], _ref(G, "Hudson")[0][:2])


# the seed of the permutation test below was checked with the reference alone, on the CPU, before it was fixed here:
# tests/fstperm_ref.py::perm_test on test_panel() gives p = 0.01 for the five diverged pairs and p >= 0.05 for the split pair
PERM_SEED = 1


@pytest.fixture(scope="module")
def perm_ref():
    codes, gid = fr.test_panel()
    return codes, gid, fr.perm_test(codes, gid, 4, "Hudson", 99, PERM_SEED)


def test_the_permutation_test(tpg, perm_ref):
    codes, gid, (fst, p, nv) = perm_ref
    X = tpg.FBM.from_numpy(codes)
    got = tpg.pairwise_pop_fst_test(X, None, None, gid, 4, method="Hudson", n_perm=99, seed=PERM_SEED, return_perm=True)
    split = 5  # the pair (3, 4) of combn(4, 2): one population cut at random in two
    print("fst", got["fst_tot"], "p", got["p_value"])
    assert np.all(got["p_value"][:split] == 0.01) and got["p_value"][split] >= 0.05
    assert _same_bits(got["perm_fst"], fst[1:]) and _same_bits(got["fst_tot"], fst[0])
    assert np.array_equal(got["p_value"], p) and np.array_equal(got["n_valid"], nv) and np.all(nv == 99)
    # fst_tot agrees with the totals call to rounding
    tot = tpg.pairwise_pop_fst(X, None, None, gid, 4, method="Hudson")["fst_tot"]
    assert np.allclose(got["fst_tot"], tot, rtol=1e-12, atol=0)
    # max_rows forcing several batches, and a pair list of the caller's: the same bits
    few = tpg.pairwise_pop_fst_test(X, None, None, gid, 4, method="Hudson", n_perm=99, seed=PERM_SEED, return_perm=True, max_rows=37)
    assert _same_bits(few["perm_fst"], got["perm_fst"]) and np.array_equal(few["p_value"], got["p_value"])
    sub = tpg.pairwise_pop_fst_test(X, None, None, gid, 4, method="Hudson", n_perm=99, seed=PERM_SEED, return_perm=True,
                                    pairwise_combn=[[3], [4]])
    assert _same_bits(sub["perm_fst"][:, 0], got["perm_fst"][:, split])
    X.free()


def test_the_global_scheme(tpg, perm_ref):
    codes, gid, _ = perm_ref
    X = tpg.FBM.from_numpy(codes)
    got = tpg.pairwise_pop_fst_test(X, None, None, gid, 4, method="WC84", n_perm=19, seed=3, scheme="global", return_perm=True)
    lab = np.stack([fr.perm_labels(60, gid, 4, 1, 0, 0, 3, r) for r in range(20)])
    pairs = np.array([(a, b) for a in range(1, 5) for b in range(a + 1, 5)]).T
    fst = fr.reference(codes, lab, 4, pairs, "WC84")[3]
    assert _same_bits(got["fst_tot"], fst[0]) and _same_bits(got["perm_fst"], fst[1:])
    p = [fr.pvalue(fst[0, k], fst[1:, k])[0] for k in range(6)]
    assert np.array_equal(got["p_value"], p)
    X.free()
