"""GPU: lsq_normal, lsq_solve and predict_gt_pca_lsq (include/tpg.h "least-squares projection") against the exact route and the
bounds of tests/lsq_ref.py.

What is compared how.  Every element of A and b is held to its bound against the long-double sums ((t + 2) eps sum |V_a V_b|,
(t + 4) eps sum |z V_a|, times REF_SLACK for the reference's own error), n_typed exactly.  The solve is held to the Cholesky bound
against the exact solve of the very (A, b) it was given, the whole call to the chain bound against the exact route; no
non-singular row may fall outside kappa (e_A + e_c) < 0.1.  A row's bits are the same alone, at another offset and in the full
batch, the same as the host program's (csrc/host/host_lsq.h with a team of one), and the same on a second call."""
import os
import shutil

import numpy as np
import pytest

from oracle import oracle as orc
from tests import fixtures as fx
from tests import lsq_ref as lref

pytestmark = pytest.mark.gpu

EINVAL, ENUMERIC = 1, 4
LSQ_CHUNK_LOCI = 512  # csrc/lsq.hip: a chunk of the locus split is never shorter; 2 * 512 + 1 loci are split into uneven chunks of 4 and 5 blocks


def _loadings(seed, m, L):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((m, L))
    if m >= L:
        V = np.linalg.qr(V)[0]
    p = rng.uniform(0.1, 0.9, m)
    return np.asfortranarray(V), 2.0 * p, np.sqrt(2.0 * p * (1.0 - p))


# (n, m, L, miss): n across the MFMA row tile of 16 and the T tile of 32; m across the 128-locus block, one locus past
# LSQ_CHUNK_LOCI and a panel split into uneven chunks; L from 1 to 561 columns, across the 16-column tile (L = 5: 16 pair-and-count columns,
# L = 16, 17) and the 8-tile column pass (L = 10: 5 tiles, L = 16: 10, L = 17: 12, L = 32: 36)
GRID = [(1, 1, 1, 0.0), (15, 3, 2, 0.05), (16, 127, 3, 0.5), (17, 128, 10, 0.05), (33, 129, 16, 0.5), (70, 700, 17, 0.05),
        (70, 700, 32, 0.0), (33, 700, 32, 0.5), (17, 2 * LSQ_CHUNK_LOCI + 1, 3, 0.95), (16, LSQ_CHUNK_LOCI + 1, 10, 0.5),
        (1, 700, 32, 0.05), (15, 128, 1, 0.95), (70, 129, 2, 0.5), (33, 127, 17, 0.0), (17, 3, 1, 0.05), (16, 1, 2, 0.0),
        (70, 2 * LSQ_CHUNK_LOCI + 1, 16, 0.05), (15, 700, 10, 0.95), (33, 128, 32, 0.05), (1, 129, 3, 0.5), (16, 700, 16, 0.0),
        (17, 127, 2, 0.95), (70, 3, 3, 0.0), (15, 129, 17, 0.05), (33, 2 * LSQ_CHUNK_LOCI + 1, 32, 0.5), (1, 128, 16, 0.05),
        (16, 128, 5, 0.5), (17, 700, 1, 0.5), (70, 127, 10, 0.95), (33, 1, 1, 0.05), (15, 127, 32, 0.0), (70, 128, 17, 0.5),
        (1, 3, 3, 0.0), (16, 129, 32, 0.05), (17, 129, 5, 0.0), (33, 700, 3, 0.95), (70, 700, 2, 0.05), (15, 1, 1, 0.95),
        (33, LSQ_CHUNK_LOCI + 1, 17, 0.5), (70, 128, 1, 0.0)]


@pytest.mark.parametrize("n,m,L,miss", GRID)
def test_lsq_normal_and_solve_grid(n, m, L, miss):
    import tidypopgen_amd as tpg

    seed = 7 * n + 13 * m + 31 * L
    fbm = orc.synth_fbm(seed, n, m, npop=4, miss=miss)
    V, center, scale = _loadings(seed, m, L)
    got = tpg.lsq_normal(tpg.View(tpg.FBM.from_numpy(fbm), code256=tpg.CODE_IMPUTE_PRED), center, scale, V)
    ex = lref.normal_exact(fbm, center, scale, V)
    assert np.array_equal(got["n_typed"], ex["n_typed"])
    bA, bb = lref.bound_A(ex), lref.bound_b(ex)
    dA = np.abs(got["A_packed"].astype(lref.LD) - ex["A"]).astype(np.float64)
    db = np.abs(got["b"].astype(lref.LD) - ex["b"]).astype(np.float64)
    typed = ex["n_typed"] > 0
    assert not dA[~typed].any() and not db[~typed].any()  # no typed locus: exact zeros
    rA = (dA[typed] / bA[typed]).max() if typed.any() else 0.0
    rb = (db[typed] / np.maximum(bb[typed], 1e-300)).max() if typed.any() else 0.0
    print(f"n {n} m {m} L {L} miss {miss}: largest ratio to the bound A {rA:.3e} b {rb:.3e}")
    assert rA <= lref.REF_SLACK and rb <= lref.REF_SLACK
    for a in range(L):
        for c in range(L):
            assert np.array_equal(got["A"][:, a, c], got["A_packed"][:, lref.pidx(L, min(a, c), max(a, c))])
    # the solve on these very (A, b): the singular rows are the restatement's, the others within the Cholesky bound
    x, sing = tpg.lsq_solve(got["A_packed"], got["b"], got["n_typed"], return_singular=True)
    want, wsing = lref.solve_restated(got["A_packed"], got["b"], got["n_typed"])
    assert sing == wsing and np.array_equal(np.isnan(x), np.isnan(want))
    left_out, worst = 0, 0.0
    for i in [i for i in range(n) if not np.isnan(x[i]).any()]:
        kap, eA, eb, ec = lref.row_numbers(ex["A"][i], ex["b"][i], bA[i], bb[i], L)
        if not lref.held(kap, eA, ec):
            left_out += 1
            continue
        xs = lref.solve_exact_row(lref.unpack(got["A_packed"][i], L), got["b"][i])
        err = float(np.linalg.norm((x[i].astype(lref.LD) - xs).astype(np.float64)))
        bound = lref.solve_bound(kap, ec, float(np.linalg.norm(xs.astype(np.float64))))
        worst = max(worst, err / bound if bound > 0 else 0.0)
        assert err <= lref.REF_SLACK * bound, (i, err, bound, kap)
    print(f"  solve: largest ratio to the bound {worst:.3e}")
    assert left_out == 0


def _special_panel(L, m=300, n=40, seed=5):
    """random codes with row 3 fully typed, row 5 fully missing, row 17 typed at exactly L loci and row 18 at L - 1"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 3, (n, m)).astype(np.uint8)
    codes[rng.random((n, m)) < 0.2] = 3
    plain = codes.copy()
    codes[3] = rng.integers(0, 3, m)
    codes[5] = 3
    for row, t in ((17, L), (18, L - 1)):
        codes[row] = 3
        at = rng.choice(m, t, replace=False)
        codes[row, at] = rng.integers(0, 3, t)
    return codes, plain


@pytest.mark.parametrize("L", [1, 3, 10, 32])
def test_special_rows_inside_a_batch(L):
    import tidypopgen_amd as tpg

    codes, plain = _special_panel(L)
    V, center, scale = _loadings(90 + L, codes.shape[1], L)
    pca = dict(v=V, center=center, scale=scale)
    pcs = tuple(range(1, L + 1))
    x, sing, nt = tpg.predict_gt_pca_lsq(pca, tpg.FBM.from_numpy(codes), lsq_pcs=pcs, return_singular=True, return_n_typed=True)
    assert nt[3] == codes.shape[1] and nt[5] == 0 and nt[17] == L and nt[18] == L - 1
    assert np.isfinite(x[3]).all() and np.isnan(x[5]).all() and np.isnan(x[18]).all()
    if L == 1:
        assert nt[18] == 0
    nrm = tpg.lsq_normal(tpg.View(tpg.FBM.from_numpy(codes), code256=tpg.CODE_IMPUTE_PRED), center, scale, V)
    want, wsing = lref.solve_restated(nrm["A_packed"], nrm["b"], nrm["n_typed"])
    assert np.array_equal(np.isnan(x), np.isnan(want)) and sing == wsing and sing >= 2
    assert np.isnan(x).any(axis=1).sum() == sing  # a singular row is NaN in every component, no other row in any
    assert np.array_equal(np.isnan(x).all(axis=1), np.isnan(x).any(axis=1))
    # the neighbours are the rows of the batch without the special rows, bit for bit
    y = tpg.predict_gt_pca_lsq(pca, tpg.FBM.from_numpy(plain), lsq_pcs=pcs)
    others = [i for i in range(len(codes)) if i not in (3, 5, 17, 18)]
    assert np.array_equal(x[others].view(np.uint64), y[others].view(np.uint64))


def test_row_and_locus_subsets_equal_the_materialised_sub_panel():
    import tidypopgen_amd as tpg

    n, m, L = 90, 700, 3
    fbm = orc.synth_fbm(61, n, m, npop=4, miss=0.3)
    rng = np.random.default_rng(2)
    rows = rng.permutation(n)[:37] + 1        # unaligned, not ascending (1-based)
    cols = rng.permutation(m)[:333] + 1
    V, center, scale = _loadings(3, len(cols), L)
    pca = dict(v=V, center=center, scale=scale)
    a = tpg.predict_gt_pca_lsq(pca, tpg.FBM.from_numpy(fbm), rows.astype(np.int32), cols.astype(np.int32), lsq_pcs=(1, 2, 3))
    sub = np.asfortranarray(fbm[rows - 1][:, cols - 1])
    b = tpg.predict_gt_pca_lsq(pca, tpg.FBM.from_numpy(sub), lsq_pcs=(1, 2, 3))
    assert a.shape == (37, 3) and np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


_batch = {}


def _batch_case(L):
    if L not in _batch:
        codes, center, scale, V = lref.grid_case(300 + L, 257, 150, L, 0.4)
        codes[11] = 3  # a singular row inside the batch
        _batch[L] = lref.normal_float(codes, center, scale, V)
    return _batch[L]


@pytest.mark.parametrize("L", [2, 10, 20, 32])
def test_a_row_alone_at_another_offset_and_in_the_batch_are_bitwise_equal(L):
    import tidypopgen_amd as tpg

    A, b, nt = _batch_case(L)
    full = tpg.lsq_solve(A, b, nt)
    assert np.isnan(full[11]).all() and np.isfinite(np.delete(full, 11, axis=0)).all()
    for n in (1, 63, 64, 65, 257):
        part = tpg.lsq_solve(A[:n], b[:n], nt[:n])
        assert np.array_equal(part.view(np.uint64), full[:n].view(np.uint64)), n
    for i in (0, 1, 63, 64, 130, 256):
        alone = tpg.lsq_solve(A[i:i + 1], b[i:i + 1], nt[i:i + 1])
        assert np.array_equal(alone[0].view(np.uint64), full[i].view(np.uint64)), i
    part = tpg.lsq_solve(A[5:70], b[5:70], nt[5:70])
    assert np.array_equal(part.view(np.uint64), full[5:70].view(np.uint64))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_the_host_routine_and_the_kernel_agree_bit_for_bit(tmp_path):
    # csrc/host/host_lsq.h is one text for both: every sum is formed by one member of a team in ascending order and every
    # operation is a correctly rounded IEEE one without contraction on either side, so a team of one thread on the host and a
    # team of 4, 8 or 16 lanes give the same bits
    import tidypopgen_amd as tpg

    exe = lref.build_host_program(str(tmp_path / "lsq_host"), sanitize=False)
    for L in (1, 3, 10, 20, 32):
        codes, center, scale, V = lref.grid_case(400 + L, 70, 120, L, 0.4)
        codes[7] = 3
        A, b, nt = lref.normal_float(codes, center, scale, V)
        rc, host, sing = lref.run_host_program(exe, tmp_path, A, b, nt)
        got, gsing = tpg.lsq_solve(A, b, nt, return_singular=True)
        assert rc == 0 and sing == gsing >= 1
        assert np.array_equal(host.view(np.uint64), got.view(np.uint64)), L


_parity = {}


def _parity_setup(tpg):
    """the setup of tests/test_gpu_parity.py::test_predict_gt_pca_projections: 150 x 1200, k = 6, missing genotypes in the new rows"""
    if not _parity:
        n, m, k = 150, 1200, 6
        fbm = orc.synth_fbm(41, n, m, npop=4, miss=0.0)
        keep = np.where((fbm.sum(axis=0) > 0) & (fbm.sum(axis=0) < 2 * n))[0]
        cols = (keep + 1).astype(np.int32)
        pca = tpg.gt_pca_partialSVD(tpg.FBM.from_numpy(fbm), None, cols, k=k)
        _parity.update(pca=pca, cols=cols, new=orc.synth_fbm(42, 60, m, npop=4, miss=0.06))
    return _parity["pca"], _parity["cols"], _parity["new"]


@pytest.mark.parametrize("lsq", [(1, 2), (1, 2, 3), (2, 5), (6, 1)])
def test_predict_gt_pca_lsq_against_the_exact_route_the_oracle_and_the_old_route(lsq):
    import tidypopgen_amd as tpg

    pca, cols, new = _parity_setup(tpg)
    Xn = tpg.FBM.from_numpy(new)
    x, sing, nt = tpg.predict_gt_pca_lsq(pca, Xn, None, cols, lsq_pcs=lsq, return_singular=True, return_n_typed=True)
    assert sing == 0 and x.shape == (60, len(lsq))
    again = tpg.predict_gt_pca_lsq(pca, Xn, None, cols, lsq_pcs=lsq)
    assert np.array_equal(x.view(np.uint64), again.view(np.uint64))  # two calls, the same bits
    # the one call is the two calls
    Vs = np.asfortranarray(pca["v"][:, np.array(lsq) - 1])
    nrm = tpg.lsq_normal(tpg.View(Xn, None, cols, code256=tpg.CODE_IMPUTE_PRED), pca["center"], pca["scale"], Vs)
    two = tpg.lsq_solve(nrm["A_packed"], nrm["b"], nrm["n_typed"])
    assert np.array_equal(x.view(np.uint64), two.view(np.uint64)) and np.array_equal(nt, nrm["n_typed"])
    # the chain bound against the exact route
    sub = new[:, cols - 1]
    L = len(lsq)
    ex = lref.normal_exact(sub, pca["center"], pca["scale"], Vs)
    bA, bb = lref.bound_A(ex), lref.bound_b(ex)
    assert np.array_equal(nt, ex["n_typed"])
    left_out, worst = 0, 0.0
    for i in range(0, 60, 3):
        kap, eA, eb, ec = lref.row_numbers(ex["A"][i], ex["b"][i], bA[i], bb[i], L)
        if not lref.held(kap, eA, ec):
            left_out += 1
            continue
        xe = lref.solve_exact_row(lref.unpack(ex["A"][i], L), ex["b"][i])
        err = float(np.linalg.norm((x[i].astype(lref.LD) - xe).astype(np.float64)))
        bound = lref.chain_bound(kap, eA, eb, ec, float(np.linalg.norm(xe.astype(np.float64))))
        worst = max(worst, err / bound)
        assert err <= lref.REF_SLACK * bound, (i, err, bound, kap)
    print(f"lsq_pcs {lsq}: largest ratio to the chain bound {worst:.3e}")
    assert left_out == 0
    # the tolerance of the existing test, against the oracle and against today's route
    opca = dict(d=pca["d"], u=pca["u"], v=pca["v"], center=pca["center"], scale=pca["scale"])
    o = orc.predict_gt_pca(opca, new, None, cols, project_method="least_squares", lsq_pcs=lsq)
    t = tpg.predict_gt_pca(pca, Xn, None, cols, project_method="least_squares", lsq_pcs=lsq)
    assert np.allclose(x, o, rtol=1e-8, atol=1e-8 * np.abs(o).max())
    assert np.allclose(x, t, rtol=1e-8, atol=1e-8 * np.abs(o).max())


def test_bad_lsq_pcs_raise_what_predict_gt_pca_raises():
    import tidypopgen_amd as tpg

    pca, cols, new = _parity_setup(tpg)
    Xn = tpg.FBM.from_numpy(new)
    for bad in ((), (0, 1), (1, 1), (1, 7), (1.5, 2)):
        with pytest.raises(ValueError) as old:
            tpg.predict_gt_pca(pca, Xn, None, cols, project_method="least_squares", lsq_pcs=bad)
        with pytest.raises(ValueError) as neu:
            tpg.predict_gt_pca_lsq(pca, Xn, None, cols, lsq_pcs=bad)
        assert str(neu.value) == str(old.value), bad


def test_lobster_panel_projects_the_held_out_individuals():
    import tidypopgen_amd as tpg

    codes = np.asarray(fx.lobster_fbm())
    X = tpg.FBM.open_bed(os.path.join(fx.GOLDEN, "lobster", "lobster.bed"), 176, 79)
    ref = codes[:150]
    alt, typed = np.where(ref < 3, ref, 0).sum(axis=0), (ref < 3).sum(axis=0)
    cols = (np.where((alt > 0) & (alt < 2 * typed))[0] + 1).astype(np.int32)
    rows_ref, rows_new = np.arange(1, 151, dtype=np.int32), np.arange(151, 177, dtype=np.int32)
    pca = tpg.gt_pca_partialSVD(X, rows_ref, cols, k=5, impute="mode")
    x, sing, nt = tpg.predict_gt_pca_lsq(pca, X, rows_new, cols, lsq_pcs=(1, 2, 3), return_singular=True, return_n_typed=True)
    sub = codes[150:][:, cols - 1]
    assert (sub == 3).any()  # the held-out individuals have missing genotypes: the mask chain is not idle
    Vs = np.asfortranarray(pca["v"][:, :3])
    ex = lref.normal_exact(sub, pca["center"], pca["scale"], Vs)
    bA, bb = lref.bound_A(ex), lref.bound_b(ex)
    assert sing == 0 and np.array_equal(nt, ex["n_typed"])
    left_out = 0
    for i in range(len(sub)):
        kap, eA, eb, ec = lref.row_numbers(ex["A"][i], ex["b"][i], bA[i], bb[i], 3)
        if not lref.held(kap, eA, ec):
            left_out += 1
            continue
        xe = lref.solve_exact_row(lref.unpack(ex["A"][i], 3), ex["b"][i])
        err = float(np.linalg.norm((x[i].astype(lref.LD) - xe).astype(np.float64)))
        assert err <= lref.REF_SLACK * lref.chain_bound(kap, eA, eb, ec, float(np.linalg.norm(xe.astype(np.float64)))), i
    assert left_out == 0
    # and the float64 restatement agrees to the same tolerance the projections are compared at elsewhere
    Af, bf, ntf = lref.normal_float(sub, pca["center"], pca["scale"], Vs)
    want, _ = lref.solve_restated(Af, bf, ntf)
    assert np.allclose(x, want, rtol=1e-8, atol=1e-8 * np.abs(want).max())


def test_errors_and_the_empty_batch():
    import tidypopgen_amd as tpg

    n, m = 20, 200
    fbm = orc.synth_fbm(9, n, m, npop=4, miss=0.1)
    v = tpg.View(tpg.FBM.from_numpy(fbm), code256=tpg.CODE_IMPUTE_PRED)
    V, center, scale = _loadings(1, m, 33)
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.lsq_normal(v, center, scale, V)            # L = 33
    assert e.value.code == EINVAL
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.lsq_normal(v, center, scale, V[:, :0])     # L = 0
    assert e.value.code == EINVAL
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.lsq_solve(np.zeros((3, 33 * 34 // 2)), np.zeros((3, 33)), np.zeros(3, dtype=np.int64))
    assert e.value.code == EINVAL
    V3 = np.asfortranarray(V[:, :3])
    bad = V3.copy()
    bad[17, 1] = np.nan
    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.lsq_normal(v, center, scale, bad)
    assert e.value.code == ENUMERIC
    zero = scale.copy()
    zero[5] = 0.0
    for fn in (lambda: tpg.lsq_normal(v, center, zero, V3),
               lambda: tpg.predict_gt_pca_lsq(dict(v=V3, center=center, scale=zero), tpg.FBM.from_numpy(fbm), lsq_pcs=(1, 2, 3))):
        with pytest.raises(tpg._lib.TpgError) as e:
            fn()
        assert e.value.code == ENUMERIC
    # mismatched sizes: EINVAL, before the library reads past an array
    for fn in (lambda: tpg.lsq_normal(v, center[:-1], scale, V3), lambda: tpg.lsq_normal(v, center, scale, V3[:-1]),
               lambda: tpg.lsq_solve(np.zeros((3, 5)), np.zeros((3, 3)), np.zeros(3, dtype=np.int64)),
               lambda: tpg.lsq_solve(np.zeros((3, 6)), np.zeros((3, 3)), np.zeros(2, dtype=np.int64)),
               lambda: tpg.predict_gt_pca_lsq(dict(v=V3[:-1], center=center, scale=scale), tpg.FBM.from_numpy(fbm), lsq_pcs=(1, 2))):
        with pytest.raises(tpg._lib.TpgError) as e:
            fn()
        assert e.value.code == EINVAL
    # n = 0: an empty result
    x, sing = tpg.lsq_solve(np.zeros((0, 6)), np.zeros((0, 3)), np.zeros(0, dtype=np.int64), return_singular=True)
    assert x.shape == (0, 3) and sing == 0
