"""CPU-only: the numpy restatement of include/tpg.h "PC-Relate" (tests/pcrelate_ref.py) against its own extended-precision
route, the refusals of the basis, the K = 0 reduction, csrc/host/host_pcrelate.h stand-alone under the sanitizers, and the
definition itself on a simulated pedigree."""
import shutil

import numpy as np
import pytest

from tests import pcrelate_ref as pr

# (seed, n, m, K, miss)
GRID = [(1, 4, 3, 2, 0.0), (2, 17, 129, 1, 0.1), (3, 40, 700, 10, 0.1), (4, 70, 300, 32, 0.0), (5, 33, 1025, 0, 0.1), (6, 12, 128, 2, 0.3)]


def _case(spec):
    seed, n, m, K, miss = spec
    codes, V = pr.panel(seed, n, m, miss, K)
    Q = pr.basis(V, n)
    mean, c = pr.coef_float(codes, Q)
    mu = pr.mu_pinned(mean, c, Q)
    return codes, V, Q, mean, c, mu


def _ratio(got, ex, bound):
    d = np.abs(got.astype(pr.LD) - ex).astype(np.float64)
    assert not d[bound == 0].any()
    return float((d[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def test_restatement_stays_inside_its_own_bounds():
    worst = dict(c=0.0, num=0.0, den=0.0)
    for spec in GRID:
        codes, V, Q, mean, c, mu = _case(spec)
        assert np.abs(Q.T @ Q - np.eye(Q.shape[1])).max() < 1e-13  # orthonormal, and column 0 is the constant
        assert np.array_equal(Q[:, 0], np.full(len(Q), 1.0 / np.sqrt(float(len(Q)))))
        mean_x, c_x, cb = pr.coef_exact(codes, Q)
        assert np.array_equal(mean, mean_x)
        worst["c"] = max(worst["c"], _ratio(c, c_x, cb))
        valid, R, S, M = pr.operands(codes, mu, 0.01)
        num, den, cnt = pr.gram_float(R, S, M)
        ex = pr.gram_exact(codes, mu, 0.01)
        assert np.array_equal(cnt, ex["cnt"].astype(np.float64))
        worst["num"] = max(worst["num"], _ratio(num, ex["num"], ex["bnum"]))
        worst["den"] = max(worst["den"], _ratio(den, ex["den"], ex["bden"]))
        if codes.shape[1] >= 2:
            assert not valid[:, :2].any()  # wholly missing, monomorphic
    print("largest ratios to the bounds:", worst)
    assert max(worst.values()) <= pr.REF_SLACK


def test_teeth_single_precision_gram_and_one_perturbed_mu():
    seen = 0
    for spec in GRID[2:5]:
        codes, V, Q, mean, c, mu = _case(spec)
        ex = pr.gram_exact(codes, mu, 0.01)
        valid, R, S, M = pr.operands(codes, mu, 0.01)
        num32, den32, cnt32 = pr.gram_float(R, S, M, dtype=np.float32)
        ok = ex["bnum"] > 0
        assert (np.abs(num32.astype(pr.LD) - ex["num"]).astype(np.float64)[ok] > ex["bnum"][ok]).any()
        assert (np.abs(den32.astype(pr.LD) - ex["den"]).astype(np.float64)[ok] > ex["bden"][ok]).any()
        # one mu off by a relative 1e-6 (a cell away from mu = 1/2, where S is flat): the cell's R and S move, and row i of
        # Num and Den leaves its bounds (m eps sum |R R| is 1e-11 here against a change of 1e-7)
        cells = np.argwhere(valid & (np.abs(mu - 0.5) > 0.2))
        i, s = cells[len(cells) // 2]
        mu2 = mu.copy()
        mu2[i, s] *= 1.0 + 1e-6
        _, R2, S2, M2 = pr.operands(codes, mu2, 0.01)
        num2, den2, _ = pr.gram_float(R2, S2, M2)
        assert (np.abs(num2.astype(pr.LD) - ex["num"]).astype(np.float64)[i] > ex["bnum"][i]).any()
        assert (np.abs(den2.astype(pr.LD) - ex["den"]).astype(np.float64)[i] > ex["bden"][i]).any()
        seen += 1
    assert seen == 3


def test_rank_deficient_scores_and_too_few_individuals_are_refused():
    rng = np.random.default_rng(0)
    V = rng.standard_normal((20, 3))
    pr.basis(V)
    for bad in (np.column_stack([V[:, 0], V[:, 1], V[:, 0] - 2.0 * V[:, 1]]), np.column_stack([V[:, 0], np.full(20, 3.0)]),
                np.column_stack([V[:, 0], np.zeros(20)]), np.column_stack([V[:, 0], np.r_[np.nan, V[1:, 1]]])):
        with pytest.raises(pr.Refused):
            pr.basis(bad)
    pr.basis(rng.standard_normal((5, 3)))  # n = L + 1
    with pytest.raises(pr.Refused):
        pr.basis(rng.standard_normal((4, 3)))  # n = L
    with pytest.raises(pr.Refused):
        pr.basis(None, 1)
    with pytest.raises(pr.Refused):
        pr.basis(rng.standard_normal((40, 33)))


def test_library_basis_is_the_restatement_bit_for_bit():
    # tpg_pcrelate_basis is host only: no device, no context
    import tidypopgen_amd as tpg
    from tidypopgen_amd import _lib

    rng = np.random.default_rng(1)
    for n, K in ((2, 0), (3, 1), (20, 3), (150, 2), (70, 32)):
        V = np.asfortranarray(rng.standard_normal((n, K)) * 37.0) if K else None
        assert np.array_equal(tpg.pcrelate_basis(V, n).view(np.uint64), pr.basis(V, n).view(np.uint64))
    for bad in (np.asfortranarray(rng.standard_normal((4, 3))), np.asfortranarray(np.ones((20, 1)))):
        with pytest.raises(_lib.TpgError) as e:
            tpg.pcrelate_basis(bad)
        assert e.value.code == 1


def test_k0_reduces_to_the_locus_frequency_estimator():
    codes, _ = pr.panel(8, 25, 400, 0.1, 0)
    r = pr.pcrelate(codes, None, thr=0.01)
    mean, t = pr.locus_mean(codes)
    p = mean / 2.0
    use = (t > 0) & (p >= 0.01) & (p <= 0.99)
    typed = codes != 3
    g = codes.astype(np.float64)
    for i, j in ((0, 2), (3, 3), (7, 20), (24, 5)):
        both = use & typed[i] & typed[j]
        want = ((g[i] - 2 * p) * (g[j] - 2 * p))[both].sum() / (4.0 * (p * (1 - p))[both].sum())
        assert abs(r["kin"][i, j] - want) <= 1e-12 * max(1.0, abs(want))
        assert r["n_snp"][i, j] == both.sum()
    assert np.isnan(r["kin"][1]).all() and np.isnan(r["inbreeding"][1])  # individual 1 is wholly missing
    assert np.allclose(r["inbreeding"][[0, 2]], 2 * np.diag(r["kin"])[[0, 2]] - 1, rtol=0, atol=0)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_library_routines_stand_alone_under_address_and_undefined_sanitizers(tmp_path):
    exe = pr.build_host_program(str(tmp_path / "pcrelate_san"), sanitize=True)
    for spec in ((11, 2, 1, 0, 0.0), (12, 3, 5, 1, 0.0), (13, 9, 40, 2, 0.2), (14, 40, 33, 10, 0.1), (15, 36, 20, 32, 0.1)):
        seed, n, m, K, miss = spec
        codes, V = pr.panel(seed, n, m, miss, K)
        Q = pr.basis(V, n)
        mean, c = pr.coef_float(codes, Q)
        rc, gQ, gmu, gvalid, gR, gS = pr.run_host_program(exe, tmp_path, V, n, K, mean, c, codes, 0.01)
        assert rc == 0 and np.array_equal(gQ.view(np.uint64), Q.view(np.uint64)), spec
        mu = pr.mu_pinned(mean, c, Q)
        valid, R, S, _ = pr.operands(codes, mu, 0.01)
        assert np.array_equal(gmu.view(np.uint64), mu.view(np.uint64)) and np.array_equal(gvalid, valid), spec
        assert np.array_equal(gR.view(np.uint64), R.view(np.uint64)) and np.array_equal(gS.view(np.uint64), S.view(np.uint64)), spec
    rng = np.random.default_rng(2)
    V = rng.standard_normal((10, 2))
    assert pr.run_host_program(exe, tmp_path, np.column_stack([V[:, 0], 3.0 * V[:, 0]]), 10, 2, None, None, None, 0.01)[0] == 2
    assert pr.run_host_program(exe, tmp_path, np.column_stack([V[:, 0], np.ones(10)]), 10, 2, None, None, None, 0.01)[0] == 2
    assert pr.run_host_program(exe, tmp_path, V[:3], 3, 2, None, None, None, 0.01)[0] == 1  # n < L + 1
    assert pr.run_host_program(exe, tmp_path, None, 5, 33, None, None, None, 0.01)[0] == 1
    assert pr.run_host_program(exe, tmp_path, None, 5, -1, None, None, None, 0.01)[0] == 1


# The largest |kin - pedigree kinship| per pair class of the K = 2 estimate on the committed panel (pr.PED_SEED = 7), with the
# model (mean, c) from the 100 unrelated founders; the K = 0 figures of the same run for comparison.
PED_RECORD = dict(po=0.0234, fs=0.0204, unrel=0.0435, cross=0.0180)


def test_definition_on_a_simulated_admixed_pedigree():
    """Two source populations at Fst 0.1; 100 admixed founders with ancestry uniform on [0, 1], 25 of their pairs with two
    children each: 150 individuals, 19 9xx polymorphic loci, 1 % missing; 100 parent-offspring and 25 full-sib pairs (pedigree
    kinship 0.25), 11 025 unrelated pairs (0), of them the 'cross' pairs whose ancestries differ by more than 0.6.  The scores
    are numpy's (loadings from the founders, every row projected), and mean and c come from the founders: the hook of the
    header, without which the families -- two thirds of the sample -- enter the regression and pull every pair that involves
    them down by 0.01 - 0.02 (po / fs / unrel 0.048 / 0.047 / 0.053 with the whole sample as its own training set).

    Recorded with the committed seed, largest deviation per class:
        K = 2:  po 0.0234   fs 0.0204   unrelated 0.0435   cross 0.0180
        K = 0:  po 0.0313   fs 0.0270   unrelated 0.0578   cross 0.0578   (mean |kin| over the unrelated pairs 0.0139 against 0.0070 at K = 2)
    K = 0 reports structure as relatedness: pairs from opposite ends of the cline come out near -0.06, pairs from the same end
    near +0.06.  Seeds 20161 and 11 give a cross record of 0.029 and 0.021 against 0.062 and 0.059 at K = 0: the assertion below
    holds for them too, by a smaller margin."""
    codes, anc, pairs = pr.pedigree_panel()
    assert codes.shape[0] == 150 and 19900 < codes.shape[1] <= 20000
    F = pairs["founders"]
    V = pr.numpy_scores(codes, 2, F)
    k2 = pr.pcrelate_trained(codes, V, F)["kin"]
    k0 = pr.pcrelate_trained(codes, V[:, :0], F)["kin"]
    d2, d0 = pr.pedigree_deviations(k2, anc, pairs), pr.pedigree_deviations(k0, anc, pairs)
    un = pairs["unrel"]
    m2, m0 = np.abs(k2[un[:, 0], un[:, 1]]).mean(), np.abs(k0[un[:, 0], un[:, 1]]).mean()
    print("K = 2:", d2, "mean |kin| unrelated", m2)
    print("K = 0:", d0, "mean |kin| unrelated", m0)
    assert d2["n_cross"] > 1000
    for cls, rec in PED_RECORD.items():
        assert d2[cls] <= 2.0 * rec, (cls, d2[cls])
    assert d0["cross"] > 2.0 * PED_RECORD["cross"]
    assert d2["cross"] < d0["cross"] and d2["unrel"] < d0["unrel"] and m2 < m0  # nearer to the pedigree on the unrelated pairs
