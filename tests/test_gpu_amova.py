"""GPU: AMOVA (csrc/amova.hip, the squared-distance epilogue of csrc/pairwise.hip, include/tpg.h "AMOVA") against
tests/amova_ref.py.

class_sums is compared BIT FOR BIT with the reference's ordered sums on the panels of amova_ref.matrix: n = one row tile + 3 and
n = two column chunks + 5 (ragged in the tile and in the chunk, two row tiles / five, one chunk / three), an integer-valued
matrix (which also equals the exact integers), an asymmetric real-valued one and one with a NaN; 1, 2, 3, 7 and the maximum
number of classes; the label rows of amova_ref.label_rows (individuals outside, everybody in one class, an empty class, a class
of one); R = 1, B - 1, B, B + 1, 2 B + 3 rows as prefixes of one list -- a row's sums depend on the row alone, so one reference of
2 B + 3 rows per panel serves them all; A from host memory and from a device buffer."""
import functools

import numpy as np
import pytest

from tests import amova_ref as ar

pytestmark = pytest.mark.gpu

KINDS = ("int", "real", "nan")
SYNTH_SEED, PERM_SEED, SHUFFLE_SEED = 21, 5, 3  # chosen on the CPU with amova_ref alone: see test_gt_amova_end_to_end


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


def _sizes():
    C, TR, B, MAX = ar.constants()
    return (TR + 3, 2 * C + 5), (1, B - 1, B, B + 1, 2 * B + 3), (1, 2, 3, 7, MAX)


@functools.lru_cache(maxsize=None)
def _matrix(kind, n):
    A = ar.matrix(kind, n, 1000 + n)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def _labels(n, k):
    lab = ar.label_rows(7 * n + k, n, k, max(_sizes()[1]))
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def _ref(kind, n, k):
    out = ar.ordered_class_sums(_matrix(kind, n), _labels(n, k), k, ar.constants()[0])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _device(kind, n):
    import tidypopgen_amd as t

    return t.DeviceMatrix.from_numpy(_matrix(kind, n))


# ---- f. bit for bit against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_index", range(5))
@pytest.mark.parametrize("n_index", range(2))
@pytest.mark.parametrize("kind", KINDS)
def test_class_sums_equal_the_restatement_bit_for_bit(tpg, kind, n_index, k_index):
    ns, Rs, ks = _sizes()
    n, k = ns[n_index], ks[k_index]
    A, lab, want = _matrix(kind, n), _labels(n, k), _ref(kind, n, k)
    for R in Rs:
        for src in (A, _device(kind, n)):
            got = tpg.class_sums(src, lab[:R], k)
            assert got.shape == (R, k)
            assert ar.same_values(got, want[:R]), (R, type(src).__name__)
            assert not np.signbit(got[got == 0]).any()  # an empty class: +0.0
    if kind == "int":  # ... which are the exact integers
        for r in (0, 1, 2, 3):
            assert [int(x) for x in want[r]] == ar.class_sums_int(A, lab[r], k)
    if kind == "nan":  # the NaN reaches exactly the classes that hold both ends of its pair
        i, j = n // 3, n - 2
        hit = np.zeros(want.shape, dtype=bool)
        for r in range(len(lab)):
            if lab[r, i] >= 0 and lab[r, i] == lab[r, j]:
                hit[r, lab[r, i]] = True
        assert np.array_equal(np.isnan(want), hit) and hit.any()


def test_the_real_valued_sums_lie_within_the_bound_of_the_exact_sums(tpg):
    ns, _, _ = _sizes()
    n, k = ns[0], 3
    A, lab = _matrix("real", n), _labels(n, k)
    got = tpg.class_sums(A, lab[:4], k)
    from fractions import Fraction

    for r in range(4):
        for c, (s, a, cnt) in enumerate(ar.exact_class_sums(A, lab[r], k)):
            assert abs(Fraction(float(got[r, c])) - s) <= Fraction(cnt, 2 ** 52) * a, (r, c)


# ---- g. a row's bits do not depend on the batch ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("real", "nan"))
def test_a_rows_bits_do_not_depend_on_the_batch(tpg, kind):
    ns, Rs, _ = _sizes()
    n, k = ns[1], 7
    A, lab = _device(kind, n), _labels(n, k)
    full = tpg.class_sums(A, lab, k)
    assert ar.same_values(full, _ref(kind, n, k))
    assert ar.same_values(tpg.class_sums(A, lab, k), full)  # two calls: the same bits
    assert ar.same_values(tpg.class_sums(A, lab[::-1], k)[::-1], full)  # the rows reversed
    for r in range(len(lab)):  # each row alone
        assert ar.same_values(tpg.class_sums(A, lab[r], k), full[r:r + 1]), r
    # the same rows with other classes beside them: more classes than any label uses
    assert ar.same_values(tpg.class_sums(A, lab[:5], k + 6)[:, :k], full[:5])


# ---- h. the squared distance -------------------------------------------------------------------------------------------------------
def test_pairwise_sqdist_equals_the_integer_restatement(tpg):
    rng = np.random.default_rng(17)
    n, m = 130, 700
    codes = rng.binomial(2, np.broadcast_to(rng.uniform(0.05, 0.95, size=m), (n, m))).astype(np.uint8)
    codes[rng.random((n, m)) < 0.1] = ar.MISSING
    codes[3, : m // 2] = ar.MISSING  # individuals 3 and 77 have no locus in common
    codes[77, m // 2:] = ar.MISSING
    raw, V, adj = ar.sqdist(codes)
    assert V[3, 77] == 0 and np.isnan(adj[3, 77]) and np.isnan(adj).sum() == 2
    X = tpg.FBM.from_numpy(np.asfortranarray(codes))
    got = tpg.pairwise_sqdist(X)
    assert got.dtype == np.float64 and np.array_equal(got, raw.astype(np.float64)) and (np.diag(got) == 0).all()
    assert ar.same_values(tpg.pairwise_sqdist(X, type="adjusted"), adj)
    dev = tpg.pairwise_sqdist(X, device=True)  # stays in HBM, and the next call accepts it
    assert isinstance(dev, tpg.DeviceMatrix) and np.array_equal(dev.to_numpy(), got)
    lab = np.stack([np.zeros(n, dtype=np.int32), (np.arange(n) % 3).astype(np.int32)])
    assert ar.same_values(tpg.class_sums(dev, lab, 3), ar.ordered_class_sums(raw.astype(np.float64), lab, 3, ar.constants()[0]))
    # a view: rows and columns picked, the distances of the sub-panel
    rows, cols = np.arange(5, 100, 2), np.arange(0, 650, 3)
    sub = tpg.pairwise_sqdist(X, rows + 1, cols + 1, type="adjusted")
    assert ar.same_values(sub, ar.sqdist(codes[np.ix_(rows, cols)])[2])
    # accumulators without the het x typed product cannot give the distance
    v = tpg.View(X, code256=None)
    pw = tpg.Pairwise(X.ctx, n)
    pw.accumulate(v, products=tpg.api.PW_FOR_AS)
    out = np.full((n, n), -7.0, order="F")
    with pytest.raises(tpg._lib.TpgError) as e:
        pw.sqdist("raw", out=out)
    assert e.value.code == 1 and (out == -7.0).all()
    with pytest.raises(tpg._lib.TpgError):
        tpg.Pairwise(X.ctx, n).sqdist("adjusted", m=0)


# ---- i. the driver -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _e2e():
    from oracle import oracle as orc

    n, m, P = 72, 600, 6
    codes = orc.synth_fbm(SYNTH_SEED, n, m, npop=P)
    raw = ar.sqdist(codes)[0].astype(np.float64)
    pop = (np.arange(n) % P).astype(np.int32)
    reg = np.array([0, 0, 1, 1, 2, 2], dtype=np.int32)
    shuffled = np.random.default_rng(SHUFFLE_SEED).permutation(pop).astype(np.int32)
    C = ar.constants()[0]
    return dict(codes=codes, raw=raw, pop=pop, reg=reg, shuffled=shuffled, ref=ar.amova(raw, pop, P, reg, 99, PERM_SEED, C),
                ref_shuffled=ar.amova(raw, shuffled, P, reg, 99, PERM_SEED, C), ref2=ar.amova(raw, pop, P, None, 99, PERM_SEED, C))


def _check_against(out, ref, levels):
    o, keep = ref["obs"], (slice(0, 4) if levels == 3 else slice(1, 4))
    t = out["table"]
    assert len(t["source"]) == (4 if levels == 3 else 3)
    assert ar.same_values(t["df"], o["df"][keep]) and ar.same_values(t["ssd"], o["ssd"][keep])
    assert ar.same_values(t["msd"], np.append(o["msd"], np.nan)[keep]) and ar.same_values(t["sigma2"], o["sigma2"][keep])
    assert ar.same_values(t["percent"], (100.0 * o["sigma2"] / o["sigma2"][3])[keep])
    assert ar.same_values(out["ncoef"], o["ncoef"]) and ar.same_values(out["phi"], ref["phi"])
    assert ar.same_values(out["p_value"], ref["p_value"]) and np.array_equal(out["n_valid"], ref["n_valid"])
    assert sorted(out["perm"]) == sorted(ref["perm"])
    for s in ref["perm"]:
        assert ar.same_values(out["perm"][s]["phi"], ref["perm"][s]["phi"]), s
        assert ar.same_values(out["perm"][s]["sigma2"], ref["perm"][s]["sigma2"]), s


def test_gt_amova_end_to_end(tpg):
    e = _e2e()
    # the seeds were chosen with the numpy reference alone: structure is found where it is, and not where the labels are shuffled
    assert e["ref"]["phi"][2] > 0 and e["ref"]["p_value"][2] == 0.01
    assert e["ref_shuffled"]["p_value"][2] > 0.05
    X = tpg.FBM.synth(SYNTH_SEED, 72, 600, npop=6)
    assert np.array_equal(X.to_numpy(), e["codes"])
    out = tpg.gt_amova(X, pop=e["pop"], npop=6, region_of_pop=e["reg"], n_perm=99, seed=PERM_SEED, return_perm=True)
    _check_against(out, e["ref"], 3)
    assert out["phi"][2] > 0 and out["p_value"][2] == 0.01 and (out["n_valid"] == 99).all()
    sh = tpg.gt_amova(X, pop=e["shuffled"], npop=6, region_of_pop=e["reg"], n_perm=99, seed=PERM_SEED, return_perm=True)
    _check_against(sh, e["ref_shuffled"], 3)
    assert sh["p_value"][2] > 0.05
    two = tpg.gt_amova(X, pop=e["pop"], npop=6, n_perm=99, seed=PERM_SEED, return_perm=True)  # two levels
    _check_against(two, e["ref2"], 2)
    host = tpg.gt_amova(dist=e["raw"], pop=e["pop"], npop=6, n_perm=99, seed=PERM_SEED)  # a host matrix instead of X
    assert ar.same_values(host["phi"], two["phi"]) and ar.same_values(host["p_value"], two["p_value"]) and "perm" not in host
    host3 = tpg.gt_amova(dist=e["raw"], pop=e["pop"], npop=6, region_of_pop=e["reg"], n_perm=99, seed=PERM_SEED)
    assert ar.same_values(host3["phi"], out["phi"]) and ar.same_values(host3["table"]["ssd"], out["table"]["ssd"])
    # some individuals left out (-1): they stay out of every relabeling and of T
    part = e["pop"].copy()
    part[[5, 6, 40]] = -1
    left = tpg.gt_amova(X, pop=part, npop=6, region_of_pop=e["reg"], n_perm=9, seed=PERM_SEED, return_perm=True)
    _check_against(left, ar.amova(e["raw"], part, 6, e["reg"], 9, PERM_SEED, ar.constants()[0]), 3)
    assert left["table"]["df"][3] == 72 - 3 - 1


# ---- j. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_alone(tpg):
    lib, ctx = tpg._lib.lib, tpg.default_context()
    C, TR, B, MAX = ar.constants()
    n = 40
    A = np.asfortranarray(np.random.default_rng(1).normal(size=(n, n)))
    lab = np.zeros((3, n), dtype=np.int32)
    bad_hi, bad_lo = lab.copy(), lab.copy()
    bad_hi[2, 7], bad_lo[1, 0] = 2, -2

    def call(labels, R, k, nn=n):
        sums = np.full((3, max(k, 1)), -7.0)
        rc = lib.tpg_class_sums(ctx.h, A.ctypes.data, nn, labels.ctypes.data, R, k, sums.ctypes.data)
        if rc != 0 or R == 0:
            assert (sums == -7.0).all()  # nothing written
        return rc

    assert call(lab, 3, MAX + 1) == 1 and call(lab, 3, 0) == 1  # nclasses out of range
    assert call(bad_hi, 3, 2) == 1 and call(bad_lo, 3, 2) == 1  # a label out of range
    assert call(lab, -1, 2) == 1 and call(lab, 3, 2, nn=0) == 1
    assert call(lab, 0, 2) == 0  # R = 0: fine, nothing written
    assert call(lab, 3, 2) == 0
    with pytest.raises(tpg._lib.TpgError) as e:  # an empty population
        tpg.gt_amova(dist=A, pop=np.arange(n) % 3, npop=4, n_perm=9)
    assert e.value.code == 1
    with pytest.raises(tpg._lib.TpgError) as e:  # an empty region
        tpg.gt_amova(dist=A, pop=np.arange(n) % 3, npop=3, region_of_pop=[0, 2, 2], n_perm=9)
    assert e.value.code == 1
