"""GPU: oadp_proj, predict_gt_pca_oadp and predict_gt_dapc (include/tpg.h "OADP projection", "DAPC") against the numpy
restatement tests/oadp_ref.py.

What is compared how.  The shape grid holds every element of every row to 256 (K + 1) eps (d_1 / d_K)^2 max(|l|_inf, sqrt(s)):
(d_1 / d_K)^2 is the conditioning of S_K through M M', and two float64 routes on the host (the eigen-decomposition of M M' and
the SVD of M) differ by at most a sixth of it on these inputs.  With K the rank of the panel the projection is the brute-force
one (the SVD of the panel with the new row appended) to 1e-10 d_1.  A row's bits are the same alone and inside a batch."""
import shutil

import numpy as np
import pytest

from tests import oadp_ref as oref

pytestmark = pytest.mark.gpu

EINVAL, ENUMERIC = 1, 4
RATIOS = (1.5, 10.0, 100.0)


@pytest.mark.parametrize("K", [1, 2, 3, 10, 20, 32])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_oadp_proj_shape_grid(n, K):
    import tidypopgen_amd as tpg

    worst = 0.0
    for which, ratio in enumerate(RATIOS):
        XV, nrm, d = oref.grid_case(1000 * K + 3 * n + which, n, K, ratio)
        got, deg = tpg.oadp_proj(XV, nrm, d, return_degenerate=True)
        want, wdeg = oref.oadp_proj(XV, nrm, d)
        assert got.shape == (n, K) and deg == wdeg == 0
        bnd = np.array([oref.bound(XV[i], nrm[i], d) for i in range(n)])
        ratio_to_bound = (np.abs(got - want).max(axis=1) / bnd).max()
        worst = max(worst, ratio_to_bound)
        assert ratio_to_bound < 1.0, (n, K, ratio, ratio_to_bound)
    print(f"n {n} K {K}: largest ratio to the bound {worst:.3e}")


def test_oadp_proj_is_the_brute_force_projection_at_full_rank():
    import tidypopgen_amd as tpg

    Z, new = oref.exact_case()
    XV, nrm, d = oref.inputs(Z, new, 12)
    got, deg = tpg.oadp_proj(XV, nrm, d, return_degenerate=True)
    want = np.array([oref.brute(Z, z, 12) for z in new])
    assert deg == 0 and np.abs(got - want).max() <= 1e-10 * d[0]


@pytest.mark.parametrize("K", [2, 10, 20, 32])
def test_a_row_alone_and_in_a_batch_are_bitwise_equal(K):
    import tidypopgen_amd as tpg

    XV, nrm, d = oref.grid_case(77 + K, 257, K, 10.0)
    batch = tpg.oadp_proj(XV, nrm, d)
    for i in (0, 1, 63, 64, 130, 256):
        alone = tpg.oadp_proj(XV[i:i + 1], nrm[i:i + 1], d)
        assert np.array_equal(alone[0].view(np.uint64), batch[i].view(np.uint64)), (K, i)
    # and at another position of a shorter batch
    part = tpg.oadp_proj(np.asfortranarray(XV[5:70]), nrm[5:70], d)
    assert np.array_equal(part.view(np.uint64), batch[5:70].view(np.uint64))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_the_host_routine_and_the_kernel_agree_bit_for_bit(tmp_path):
    # csrc/host/host_oadp.h is one text for both: every sum is formed by one member of a team in ascending order and every
    # operation is a correctly rounded IEEE one without contraction on either side, so a team of one thread on the host and a
    # team of 4, 8 or 16 lanes give the same bits
    import tidypopgen_amd as tpg

    exe = oref.build_host_program(str(tmp_path / "oadp_host"), sanitize=False)
    for K, ratio in ((3, 100.0), (10, 1.5), (20, 10.0), (32, 100.0)):
        XV, nrm, d = oref.grid_case(40 + K, 70, K, ratio)
        rc, host, deg = oref.run_host_program(exe, tmp_path, XV, nrm, d)
        assert rc == 0 and deg == 0
        assert np.array_equal(host.view(np.uint64), tpg.oadp_proj(XV, nrm, d).view(np.uint64)), K


@pytest.mark.parametrize("K", [1, 3, 20])
def test_edge_rows(K):
    import tidypopgen_amd as tpg

    XV, nrm, d = oref.grid_case(5 + K, 70, K, 10.0)
    plain = tpg.oadp_proj(XV, nrm, d)
    dk2 = d[-1] ** 2
    for at, s, zero in ((0, 0.0, True), (17, dk2 / 4, True), (69, 4 * dk2, False)):
        xv, nr = XV.copy(order="F"), nrm.copy()
        xv[at], nr[at] = 0.0, s
        got, deg = tpg.oadp_proj(xv, nr, d, return_degenerate=True)
        if zero:
            assert deg == 0 and np.array_equal(got[at], np.zeros(K))
        else:
            assert deg == 1 and np.isnan(got[at]).all()
        others = np.arange(70) != at
        assert np.array_equal(got[others].view(np.uint64), plain[others].view(np.uint64))


def test_argument_errors():
    import tidypopgen_amd as tpg

    XV, nrm, d = oref.grid_case(3, 10, 3, 10.0)
    cases = [(np.zeros((4, 33), order="F"), np.zeros(4), np.arange(33, 0, -1.0), EINVAL),   # K = 33
             (XV, nrm, d[::-1].copy(), EINVAL),                                           # ascending
             (XV, nrm, np.array([d[0], d[1], 0.0]), EINVAL),                              # not positive
             (XV, nrm, np.array([d[0], np.nan, d[2]]), ENUMERIC)]
    bad_xv, bad_nrm = XV.copy(order="F"), nrm.copy()
    bad_xv[4, 1], bad_nrm[7] = np.inf, np.nan
    cases += [(bad_xv, nrm, d, ENUMERIC), (XV, bad_nrm, d, ENUMERIC)]
    for xv, nr, dd, code in cases:
        with pytest.raises(tpg._lib.TpgError) as e:
            tpg.oadp_proj(xv, nr, dd)
        assert e.value.code == code
    with pytest.raises(ValueError):
        tpg.oadp_proj(XV, nrm[:5], d)
    assert tpg.oadp_proj(XV[:0], nrm[:0], d).shape == (0, 3)


def test_predict_gt_pca_oadp_is_the_sweep_then_the_projection():
    import tidypopgen_amd as tpg
    from oracle import oracle as orc

    # the panel of test_predict_gt_pca_projections
    n, m, k = 150, 1200, 6
    fbm = orc.synth_fbm(41, n, m, npop=4, miss=0.0)
    keep = np.where((fbm.sum(axis=0) > 0) & (fbm.sum(axis=0) < 2 * n))[0]
    cols = (keep + 1).astype(np.int32)
    pca = tpg.gt_pca_partialSVD(tpg.FBM.from_numpy(fbm), None, cols, k=k)
    Xna = tpg.FBM.from_numpy(orc.synth_fbm(42, 60, m, npop=4, miss=0.06))
    got, deg = tpg.predict_gt_pca_oadp(pca, Xna, None, cols, return_degenerate=True)
    XV, nrm = tpg.oadp_inputs(pca, Xna, None, cols)
    want, wdeg = oref.oadp_proj(XV, nrm, pca["d"])
    assert deg == wdeg == 0 and got.shape == (60, k)
    tol = np.array([oref.bound(XV[i], nrm[i], pca["d"]) for i in range(60)])[:, None] + 1e-9 * np.abs(want)
    assert (np.abs(got - want) <= tol).all(), (np.abs(got - want) / tol).max()
    assert np.abs(got).max() > np.abs(XV).max()  # OADP stretches the shrunken scores
    with pytest.raises(NotImplementedError, match="predict_gt_pca_oadp"):
        tpg.predict_gt_pca(pca, Xna, None, cols, project_method="OADP")


@pytest.fixture(scope="module")
def binomial():
    """three populations, 200 reference and 50 new individuals at 5000 loci; the PCA of the reference with K = 2"""
    import tidypopgen_amd as tpg

    ref, new, lab_ref, lab_new = oref.binomial_panel()
    cols = (np.where((ref.sum(axis=0) > 0) & (ref.sum(axis=0) < 2 * len(ref)))[0] + 1).astype(np.int32)
    pca = tpg.gt_pca_partialSVD(tpg.FBM.from_numpy(ref), None, cols, k=2)
    Xn = tpg.FBM.from_numpy(new)
    return dict(pca=pca, cols=cols, Xn=Xn, lab_ref=lab_ref, lab_new=lab_new,
                simple=tpg.predict_gt_pca(pca, Xn, None, cols, project_method="simple"),
                oadp=tpg.predict_gt_pca_oadp(pca, Xn, None, cols))


def test_oadp_undoes_the_shrinkage_of_projected_scores(binomial):
    import tidypopgen_amd as tpg

    b = binomial
    UD = b["pca"]["u"] * b["pca"]["d"]
    cent = np.array([UD[b["lab_ref"] == g].mean(axis=0) for g in range(3)])[b["lab_new"]]
    dist_simple = np.sqrt(((b["simple"] - cent) ** 2).sum(axis=1)).mean()
    dist_oadp = np.sqrt(((b["oadp"] - cent) ** 2).sum(axis=1)).mean()
    print("mean distance to the population's centroid: simple", dist_simple, "OADP", dist_oadp)
    assert dist_oadp < dist_simple
    # it is the restatement's projection of the device's sweep, and it stretches the shrunken scores
    XV, nrm = tpg.oadp_inputs(b["pca"], b["Xn"], None, b["cols"])
    want, _ = oref.oadp_proj(XV, nrm, b["pca"]["d"])
    tol = np.array([oref.bound(XV[i], nrm[i], b["pca"]["d"]) for i in range(50)])[:, None] + 1e-9 * np.abs(want)
    assert (np.abs(b["oadp"] - want) <= tol).all()
    assert np.abs(b["oadp"]).max() > np.abs(b["simple"]).max()


def test_predict_gt_dapc_on_training_scores_and_on_projected_individuals(binomial):
    import tidypopgen_amd as tpg

    b = binomial
    names = np.array(["north", "south", "west"])
    dapc = tpg.gt_dapc(b["pca"], pop=names[b["lab_ref"]], n_pca=2, loadings_by_locus=False)
    back = tpg.predict_gt_dapc(dapc, dapc["tab"])
    assert np.abs(back["ind.coord"] - dapc["ind.coord"]).max() <= 1e-12 * np.abs(dapc["ind.coord"]).max()
    assert np.abs(back["posterior"] - dapc["posterior"]).max() <= 1e-12
    assert np.array_equal(back["assign"], dapc["assign"])
    new = tpg.predict_gt_dapc(dapc, b["oadp"])
    assert new["ind.coord"].shape == (50, dapc["n.da"]) and new["posterior"].shape == (50, 3)
    assert np.array_equal(new["assign"], names[b["lab_new"]])
