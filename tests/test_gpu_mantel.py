"""GPU: Mantel tests (csrc/mantel.hip, include/tpg.h "Mantel tests") against tests/mantel_ref.py.

mantel_sums is compared BIT FOR BIT with the reference's ordered sums on the panels of mantel_ref.matrix: n = 2, L - 1, L, L + 1 and
2 L + 3 (one pair; one stride, ragged, full, and one lane into the second; three strides with a ragged last one), non-symmetric
matrices of small integers (which also equal the exact integers) and of mixed-magnitude reals, Q = 1, 2 and 4 matrices B, R = 1,
31, 32, 33 and 67 permutations as prefixes of one list (the identity, the reversal, random ones) -- a sum depends on A, B_q and its
own permutation alone, so ONE reference of 67 rows and 4 columns per panel serves them all; A and B from host memory and from
device buffers."""
import ctypes
import functools

import numpy as np
import pytest

from tests import mantel_ref as mr

pytestmark = pytest.mark.gpu

KINDS = ("int", "real")
RS = (1, 31, 32, 33, 67)
QS = (1, 2, 4)
SYNTH_SEED, COORD_SEED, PERM_SEED = 21, 4, 5


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


def _sizes():
    L = mr.lanes()
    return (2, L - 1, L, L + 1, 2 * L + 3)


@functools.lru_cache(maxsize=None)
def _matrix(kind, n, which):
    """which = 0: A; 1 .. 4: B_0 .. B_3 (the seeds of tests/test_mantel_host.py's panel)"""
    M = mr.matrix(kind, n, 1000 * (which + 1) + n)
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def _perms(n):
    P = mr.perm_rows(7 * n, n, max(RS))
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def _ref(kind, n):
    out = mr.ordered_sums(_matrix(kind, n, 0), [_matrix(kind, n, q + 1) for q in range(4)], _perms(n), mr.lanes())
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _device(kind, n, which):
    import tidypopgen_amd as t

    return t.DeviceMatrix.from_numpy(_matrix(kind, n, which))


# ---- a. bit for bit against the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_index", range(5))
@pytest.mark.parametrize("kind", KINDS)
def test_mantel_sums_equal_the_restatement_bit_for_bit(tpg, kind, n_index):
    n = _sizes()[n_index]
    P, want = _perms(n), _ref(kind, n)
    for Q in QS:
        for R in RS:
            for dev in (False, True):
                A = _device(kind, n, 0) if dev else _matrix(kind, n, 0)
                Bs = [_device(kind, n, q + 1) if dev else _matrix(kind, n, q + 1) for q in range(Q)]
                got = tpg.mantel_sums(A, Bs, P[:R])
                assert got.shape == (R, Q)
                assert mr.same_bits(got, want[:R, :Q]), (Q, R, dev)
    mixed = tpg.mantel_sums(_device(kind, n, 0), [_matrix(kind, n, 1), _device(kind, n, 2)], P[:3])  # host and device beside each other
    assert mr.same_bits(mixed, want[:3, :2])
    if kind == "int":  # ... which are the exact integers
        for r in (0, 1, 2, 40):
            for q in (0, 3):
                assert int(want[r, q]) == mr.int_sums(_matrix(kind, n, 0), _matrix(kind, n, q + 1), P[r]) and want[r, q] == int(want[r, q])


def test_the_real_valued_sums_lie_within_the_bound_of_the_exact_sums(tpg):
    from fractions import Fraction

    n = 67
    A, B, P = mr.matrix("real", n, 32), mr.matrix("real", n, 33), mr.perm_rows(5, n, 3)
    got = tpg.mantel_sums(A, [B], P)
    for r in range(3):
        (s, ab, k), _ = mr.exact_sums(A, B, P[r])
        assert abs(Fraction(float(got[r, 0])) - s) <= Fraction(k, 2 ** 52) * ab, r


# ---- b. determinism ----------------------------------------------------------------------------------------------------------------
def test_a_sums_bits_depend_on_its_own_inputs_alone(tpg):
    n = _sizes()[4]
    A, Bs, P, want = _device("real", n, 0), [_device("real", n, q + 1) for q in range(4)], _perms(n), _ref("real", n)
    full = tpg.mantel_sums(A, Bs, P)
    assert mr.same_bits(full, want)
    assert mr.same_bits(tpg.mantel_sums(A, Bs, P), full)  # two calls: the same bits
    assert mr.same_bits(tpg.mantel_sums(A, Bs, P[::-1])[::-1], full)  # the list reversed
    for r in range(len(P)):  # each row alone
        assert mr.same_bits(tpg.mantel_sums(A, Bs[:1], P[r]), full[r:r + 1, :1]), r
    twice = tpg.mantel_sums(A, Bs[:2], np.stack([P[5], P[9], P[5]]))  # a row given twice
    assert mr.same_bits(twice[0], twice[2]) and mr.same_bits(twice[0], full[5, :2])
    # a column computed alone and beside three other matrices, in another place
    for q in range(4):
        assert mr.same_bits(tpg.mantel_sums(A, [Bs[q]], P[:9])[:, 0], full[:9, q])
    assert mr.same_bits(tpg.mantel_sums(A, [Bs[3], Bs[1], Bs[0], Bs[2]], P[:9]), full[:9][:, [3, 1, 0, 2]])


# ---- b2. the borders inside the library: its passes over R, the trips of the kernel's loop, a column above 64 KiB ----------------
def test_rows_on_both_sides_of_a_pass_border_keep_their_bits(tpg):
    n, Q = 3, 2
    pass_rows = tpg.mantel_pass_rows(n, Q)
    assert pass_rows == tpg.mantel_pass_rows(n, 1) and pass_rows % 32 == 0  # the row cap, not the cap on the column terms
    A, Bs = mr.matrix("real", n, 71), [mr.matrix("real", n, 72), mr.matrix("real", n, 73)]
    P = np.ascontiguousarray(mr.perm_rows(74, n, 2 * pass_rows + 76))
    want = mr.ordered_sums(A, Bs, P, mr.lanes())
    assert len({tuple(p) for p in P}) == 6 and len({x.tobytes() for x in want}) == 6  # all six permutations, six different rows
    for R in (pass_rows - 1, pass_rows, pass_rows + 1, 2 * pass_rows + 76):
        assert mr.same_bits(tpg.mantel_sums(A, Bs, P[:R]), want[:R]), R
    full = tpg.mantel_sums(A, Bs, P)
    for r in range(len(P)):  # ... and each row alone
        assert mr.same_bits(tpg.mantel_sums(A, Bs, P[r]), full[r:r + 1]), r


def _stride_sizes(Q):
    span = int(__import__("tidypopgen_amd")._lib.lib.tpg_mantel_strides(Q)) * mr.lanes()  # the rows of one trip of the kernel's loop
    return (span - 1, span, span + 1, 2 * span + 3)


def test_the_cap_on_the_column_terms_sets_the_pass_and_its_border_keeps_the_bits(tpg):
    n, Q = _stride_sizes(1)[3], 4
    pass_rows = tpg.mantel_pass_rows(n, Q)
    assert 32 <= pass_rows < tpg.mantel_pass_rows(n, 1) and pass_rows % 32 == 0  # this arm: fewer rows than the row cap
    A, B0, B1 = (_device("real", n, w) for w in range(3))
    Bs = [B0, B1, B0, B1]
    P = mr.perm_rows(7 * n, n, pass_rows + 5)
    full = tpg.mantel_sums(A, Bs, P)
    assert mr.same_bits(full[:, :2], full[:, 2:])
    lo = pass_rows - 3
    assert mr.same_bits(tpg.mantel_sums(A, Bs, P[lo:]), full[lo:])  # the same rows inside ONE pass
    rows = [pass_rows - 1, pass_rows]  # the last row of the first pass and the first of the second against the restatement
    want = mr.ordered_sums(_matrix("real", n, 0), [_matrix("real", n, 1), _matrix("real", n, 2)], P[rows], mr.lanes())
    assert mr.same_bits(full[rows][:, :2], want)


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("Q", (1, 2))
def test_sizes_around_a_trip_of_the_kernels_loop(tpg, Q, k):
    n = _stride_sizes(Q)[k]  # one trip with its last slot ragged, full, a second trip of one row, three trips
    A, Bs = _matrix("real", n, 0), [_matrix("real", n, q + 1) for q in range(Q)]
    P = np.ascontiguousarray(mr.perm_rows(7 * n, n, 3)[[0, 2]])  # the identity and a random one
    want = mr.ordered_sums(A, Bs, P, mr.lanes())
    assert mr.same_bits(tpg.mantel_sums(A, Bs, P), want)
    assert mr.same_bits(tpg.mantel_sums(_device("real", n, 0), [_device("real", n, q + 1) for q in range(Q)], P[1]), want[1:])


def test_a_column_above_64_kib_of_lds(tpg):
    n = 8192 + 8  # 8 n bytes of A's column: above what a launch gets without asking
    rng = np.random.default_rng(81)
    A, B = (np.asfortranarray(rng.integers(-1024, 1025, size=(n, n)).astype(np.float64)) for _ in range(2))
    P = np.ascontiguousarray(mr.perm_rows(82, n, 3)[2:])
    got = tpg.mantel_sums(A, [B], P)
    assert got[0, 0] == mr.int_sums(A, B, P[0]) and abs(got[0, 0]) < 2.0 ** 53  # small integers: every order gives the exact sum


# ---- c. NaN, n = 1 -----------------------------------------------------------------------------------------------------------------
def test_nan_on_a_diagonal_changes_nothing_and_off_it_reaches_its_column_alone(tpg):
    n = _sizes()[3]
    P, want = _perms(n)[:5], _ref("real", n)[:5, :3]
    A, Bs = _matrix("real", n, 0).copy(), [_matrix("real", n, q + 1).copy() for q in range(3)]
    A[3, 3] = A[n - 1, n - 1] = Bs[0][0, 0] = Bs[2][7, 7] = np.nan
    assert mr.same_bits(tpg.mantel_sums(A, Bs, P), want)
    Bs[1][n - 2, 4] = np.nan
    got = tpg.mantel_sums(A, Bs, P)
    assert np.isnan(got[:, 1]).all() and mr.same_bits(got[:, [0, 2]], want[:, [0, 2]])
    A[4, n - 3] = np.nan  # off the diagonal of A: every sum
    assert np.isnan(tpg.mantel_sums(A, Bs, P)).all()


def test_one_individual_gives_plus_zero(tpg):
    got = tpg.mantel_sums(np.array([[3.5]]), [np.array([[-2.0]]), np.array([[np.nan]])], np.zeros((3, 1), dtype=np.int32))
    assert got.shape == (3, 2) and (got == 0).all() and not np.signbit(got).any()
    assert tpg.offdiag_moments(np.array([[np.nan]])) == (0.0, 0.0)


# ---- d. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_alone(tpg):
    lib, ctx = tpg._lib.lib, tpg.default_context()
    n = 40
    A, B = mr.matrix("real", n, 1), mr.matrix("real", n, 2)
    P = mr.perm_rows(3, n, 3)
    dup, hi, lo = P.copy(), P.copy(), P.copy()
    dup[2, 7] = dup[2, 8]
    hi[1, 0], lo[0, 5] = n, -1

    def call(perms, R, Q=1, nn=n):
        sums = np.full((3, 4), -7.0)
        pb = (ctypes.c_void_p * 4)(*[B.ctypes.data] * 4)
        rc = lib.tpg_mantel_sums(ctx.h, A.ctypes.data, pb, Q, nn, perms.ctypes.data, R, sums.ctypes.data)
        if rc != 0 or R == 0:
            assert (sums == -7.0).all()  # nothing written
        return rc

    assert call(dup, 3) == 1 and call(hi, 3) == 1 and call(lo, 3) == 1  # not a bijection
    assert call(P, 3, Q=0) == 1 and call(P, 3, Q=5) == 1
    assert call(P, -1) == 1 and call(P, 3, nn=0) == 1 and call(P, 3, nn=16385) == 1
    assert call(P, 0) == 0  # R = 0: fine, nothing written
    assert call(dup, 2) == 0 and call(P, 3, Q=4) == 0
    # null pointers: A, the list B, one B[q], perms, sums
    sums = np.full((3, 2), -7.0)
    pb, hole = (ctypes.c_void_p * 2)(B.ctypes.data, B.ctypes.data), (ctypes.c_void_p * 2)(B.ctypes.data, None)
    a, pp, ss = A.ctypes.data, P.ctypes.data, sums.ctypes.data
    for args in ((None, pb, 2, n, pp, 3, ss), (a, None, 2, n, pp, 3, ss), (a, hole, 2, n, pp, 3, ss), (a, pb, 2, n, None, 3, ss),
                 (a, pb, 2, n, pp, 3, None)):
        assert lib.tpg_mantel_sums(ctx.h, *args) == 1 and (sums == -7.0).all(), args
    assert lib.tpg_mantel_from_sums(4, 0.0, 4.0, 0.0, 4.0, 4.0, None) == 1  # tpg_mantel_from_sums without an output
    assert lib.tpg_offdiag_moments(ctx.h, None, n, ss) == 1 and lib.tpg_offdiag_moments(ctx.h, a, n, None) == 1 and (sums == -7.0).all()
    assert lib.tpg_offdiag_center(ctx.h, None, n, 1.0, ss) == 1 and lib.tpg_offdiag_center(ctx.h, a, n, 1.0, None) == 1
    assert lib.tpg_mantel_perms(n, None, 0, 5, 1, 2, None) == 1
    # tpg_mantel_perms: a refusal writes nothing
    out = np.full((2, n), -7, dtype=np.int32)
    st = np.zeros(n, dtype=np.int32)
    st[3] = 2
    for args in ((n, None, 0, 5, -1, 2), (n, None, 0, 5, 2 ** 31 - 1, 2), (n, st.ctypes.data, 2, 5, 1, 2), (0, None, 0, 5, 1, 2),
                 (16385, None, 0, 5, 1, 2), (n, None, 0, 5, 1, -1)):
        assert lib.tpg_mantel_perms(*args, out.ctypes.data) == 1 and (out == -7).all(), args
    assert lib.tpg_mantel_perms(n, st.ctypes.data, 3, 5, 1, 2, out.ctypes.data) == 0 and sorted(out[1]) == list(range(n))
    # the moments and the centring refuse a size outside the limits
    two = np.full(2, -7.0)
    assert lib.tpg_offdiag_moments(ctx.h, A.ctypes.data, 0, two.ctypes.data) == 1 and (two == -7.0).all()
    keep = A.copy()
    assert lib.tpg_offdiag_center(ctx.h, A.ctypes.data, 16385, 1.0, A.ctypes.data) == 1 and mr.same_bits(A, keep)
    # gt_mantel: an off-diagonal NaN in any matrix is TPG_ENUMERIC; a NaN on a diagonal is not
    y = np.abs(B + B.T)
    sym = np.abs(A + A.T)
    bad = sym.copy()
    bad[3, 9] = bad[9, 3] = np.nan
    for kw in (dict(dist=bad, y=y), dict(dist=sym, y=bad), dict(dist=sym, y=y, z=bad)):
        with pytest.raises(tpg._lib.TpgError) as e:
            tpg.gt_mantel(n_perm=9, **kw)
        assert e.value.code == 4
    ok = sym.copy()
    ok[5, 5] = np.nan
    assert np.isfinite(tpg.gt_mantel(dist=ok, y=y, n_perm=9)["statistic"])
    with pytest.raises(ValueError):
        tpg.gt_mantel(dist=A, y=y, method="spearman", n_perm=9)  # ranks need a symmetric matrix


# ---- e. the moments and the centring ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_index", range(5))
def test_offdiag_moments_and_center_equal_the_restatement_bit_for_bit(tpg, n_index):
    n = _sizes()[n_index]
    L = mr.lanes()
    for kind in KINDS:
        A, dA = _matrix(kind, n, 0), _device(kind, n, 0)
        want = mr.moments(A, L)
        assert mr.same_bits(tpg.offdiag_moments(A), want) and mr.same_bits(tpg.offdiag_moments(dA), want)
        mean = want[0] / (n * (n - 1))
        cen = mr.center(A, mean)
        got = tpg.offdiag_center(A, mean)
        assert mr.same_bits(got, cen) and not np.signbit(np.diag(got)).any()
        second = tpg.offdiag_center(dA, mean)  # into a second matrix: A stays
        assert mr.same_bits(second.to_numpy(), cen) and mr.same_bits(dA.to_numpy(), A)
        again = tpg.offdiag_center(second, 0.25, out=second)  # in place
        assert again is second and mr.same_bits(second.to_numpy(), mr.center(cen, 0.25))
        assert mr.same_bits(tpg.offdiag_moments(second), mr.moments(mr.center(cen, 0.25), L))


# ---- f. the driver -----------------------------------------------------------------------------------------------------------------
def _coords(seed, n):
    rng = np.random.default_rng(seed)
    return rng.uniform(-20, 40, size=n), rng.uniform(30, 65, size=n)


def test_gt_mantel_from_genotypes(tpg):
    n, L = 72, mr.lanes()
    X = tpg.FBM.synth(SYNTH_SEED, n, 600, npop=6)
    raw = tpg.pairwise_sqdist(X)
    assert mr.same_bits(tpg.pairwise_sqdist(X, device=True).to_numpy(), raw)
    lon, lat = _coords(COORD_SEED, n)
    y = tpg.great_circle_dist(lon, lat)
    out = tpg.gt_mantel(X, coords=(lon, lat), n_perm=99, seed=PERM_SEED, return_perm=True)
    mr.check_result(out, mr.mantel(raw, y, L, 99, PERM_SEED))
    assert out["n_valid"] == 99 and out["perm"].shape == (99,) and -1 <= out["statistic"] <= 1
    same = tpg.gt_mantel(dist=raw, y=y, n_perm=99, seed=PERM_SEED)  # the matrices instead of X and coords
    assert "perm" not in same and mr.same_values([same["statistic"], same["p_value"]], [out["statistic"], out["p_value"]])
    # the partial test, with a second set of coordinates as z
    z = tpg.great_circle_dist(*_coords(COORD_SEED + 1, n))
    part = tpg.gt_mantel(X, y=y, z=z, n_perm=99, seed=PERM_SEED, return_perm=True)
    mr.check_result(part, mr.mantel(raw, y, L, 99, PERM_SEED, z=z))
    assert mr.same_values(part["r_ab"], out["statistic"])
    # strata: the six populations of the panel
    strata = (np.arange(n) % 6).astype(np.int32)
    strat = tpg.gt_mantel(X, y=y, strata=strata, n_perm=99, seed=PERM_SEED, return_perm=True)
    mr.check_result(strat, mr.mantel(raw, y, L, 99, PERM_SEED, strata=strata))
    assert mr.same_values(strat["statistic"], out["statistic"]) and not mr.same_values(strat["perm"], out["perm"])
    # Spearman's form
    rank = tpg.gt_mantel(X, y=y, method="spearman", n_perm=99, seed=PERM_SEED, return_perm=True)
    mr.check_result(rank, mr.mantel(raw, y, L, 99, PERM_SEED, method="spearman"))
    assert not mr.same_values(rank["statistic"], out["statistic"])


def test_gt_mantel_finds_the_planted_correlation(tpg):
    A, y = mr.planted_case()
    want = mr.mantel(A, y, mr.lanes(), 99, PERM_SEED)
    # (by the restatement alone: noise of half a standard deviation leaves r near 1 / sqrt(1.25) = 0.894; it gives r = 0.888 and
    # 0.127 as the largest of the 99 permuted values -- nowhere near the edge)
    assert want["statistic"] > 0.8 and want["perm"].max() < 0.4 and want["p_value"] == 0.01
    keep = A.copy()
    dA = tpg.DeviceMatrix.from_numpy(A)
    out = tpg.gt_mantel(dist=dA, y=y, n_perm=99, seed=PERM_SEED, return_perm=True)
    mr.check_result(out, want)
    assert out["p_value"] == 0.01
    assert mr.same_bits(dA.to_numpy(), keep)  # the caller's matrix is not centred in place
