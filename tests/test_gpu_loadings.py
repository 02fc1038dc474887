"""GPU: tpg_pca_loadings (csrc/pca.hip: tpg_loadings_mfma_kernel and its digit kernels) against FP64 numpy Z'U / d.

The kernel splits every u into six 7-bit digits and works through the k * 6 digit columns in tiles of 32, up to four tiles a
launch: how many launches of which width depends on k alone, CT = ceil(6 k / 32).  k = 1, 5, 6, 11, 16, 17, 22, 27, 33, 43, 64
give CT = 1, 1, 2, 3, 3, 4, 5, 6, 7, 9, 12 -- every arm of the launch chain (1, 2, 3, 4, 4 + 1, 4 + 2, 4 + 3, 4 + 4 + 1,
4 + 4 + 4) -- and from k = 6 on components whose six digits straddle two tiles.  Both layouts of a view: rows (View) and
locus-major (the second member of View.pair when n is a multiple of 8).

What the 1e-9 bound below does NOT see: n = 130 and 136 are both Q = ceil(n / 128) = 2, one depth of the kernel's pipeline, and a
slip in a few rows -- a wrong lowest digit in one individual or in the 16 of one lane's piece, a dropped carry, a digit without its
sign in one byte position -- moves a result by a few 2^-33 max |u|, far below 1e-9.  tests/test_gpu_loadings_exact.py holds the
same kernels to integer sums bit for bit at every depth, and tests/test_loadings_host.py shows which slips pass here.
"""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

KS = [1, 5, 6, 11, 16, 17, 22, 27, 33, 43, 64]
M = 289


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


_panels = {}


def _panel(n):
    """genotypes (no missing, polymorphic loci only) of the panel of test_pca_loadings_entry_point_and_small_context_calls"""
    if n not in _panels:
        g = orc.synth_fbm(5, n, M, npop=3, miss=0.0, imputed_bytes=True)
        g = np.where(g > 3, g - 4, g).astype(np.uint8)
        g = g[:, (g.sum(0) > 0) & (g.sum(0) < 2 * n)]
        g.setflags(write=False)
        _panels[n] = g
    return _panels[n]


def _u_d(n, k):
    """orthonormal U whose first column is constant (it cancels exactly against `center`) and whose second is nearly the
    spike e_7 (max |u| ~ 1 sets the digit scale, so the other columns' entries of ~ n^-1/2 use the low digits)"""
    rng = np.random.default_rng(100 + k)
    B = rng.standard_normal((n, k))
    B[:, 0] = 1.0 / np.sqrt(n)
    if k > 1:
        B[:, 1] = 0.0
        B[7, 1] = 1.0
    U, _ = np.linalg.qr(B)
    if k == 1:
        U = np.full((n, 1), U[0, 0])  # (the Q factor of a constant column, made constant to the last bit)
    assert np.abs(U.T @ U - np.eye(k)).max() <= 1e-14
    return U, np.linspace(9.0, 2.0, k)


def _views(tpg, n):
    g = _panel(n)
    X = tpg.FBM.from_numpy(orc.fbm_from_genotypes(g))
    return g, tpg.View(X), tpg.View.pair(X)[1]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("layout,n", [("rows", 130), ("locus_major", 136)])
def test_loadings_against_fp64(tpg, layout, n, k):
    """max |got - want| <= 1e-9 max |want|, the suite's bound for this entry point.  The 2^-40 fixed point of the digits
    costs at most 2 n 2^-40 ~ 2.4e-10 at these n, so the bound has no slack to hide a digit lost or misplaced in EVERY row
    (2^-35 of max |u| at the least, per row).  A digit lost in a few rows it does hide: see the module docstring."""
    g, v_rows, v_lm = _views(tpg, n)
    v = v_rows if layout == "rows" else v_lm
    center, scale = tpg.pca_center_scale(v)
    U, d = _u_d(n, k)
    want = ((g.astype(float) - center) / scale).T @ U / d
    got = tpg.pca_loadings(v, center, scale, U, d)
    assert got.shape == want.shape
    if k == 1:
        _constant_column(n, g, center, scale, U, d, got)
        # the bound proper at k = 1, on a column that does not cancel: the near-spike
        U, d = _u_d(n, 2)[0][:, 1:2].copy(), np.array([9.0])
        want = ((g.astype(float) - center) / scale).T @ U / d
        got = tpg.pca_loadings(v, center, scale, U, d)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    assert err <= 1e-9, (layout, n, k, err)


def _constant_column(n, g, center, scale, U, d, got):
    """k = 1 is the constant column alone: Z'u is 0 exactly, and max |want| is nothing but the rounding of numpy's own sum
    (~ 1e-17), no scale to hold anybody to.  What the kernel owes there is FP64 rounding and nothing else.  Every u_i is the
    same double (`_u_d` makes it so), so every row is cut to the same multiple q of 2^-FU; the digit sums give
    gu = q sum_i g_i exactly (integers), and usum = n q exactly (40 + 8 bits fit a double in any order of adding).  The result
    (gu - center usum) / (scale d) is then off zero only by the rounding of `center` itself (a mean and a doubling: two
    roundings at the most) and of the product center * usum (one): |got_j| <= 3 * 2^-53 center_j n q / (scale_j d), and
    q <= max |u| (1 + 2^-39).  Asserted at 4 * 2^-53 = 2^-51.  A low digit lost in one row is 2^-40 max |u| off, 2000
    times this."""
    assert np.all(U == U[0, 0])
    bound = 2.0 ** -51 * np.abs(center) * n * np.abs(U).max() / (scale * d[0])
    worst = float((np.abs(got[:, 0]) / bound).max())
    assert worst <= 1.0, (n, worst)


@pytest.mark.parametrize("k", KS)
def test_loadings_layouts_agree_bit_for_bit(tpg, k):
    g, v_rows, v_lm = _views(tpg, 136)
    center, scale = tpg.pca_center_scale(v_rows)
    U, d = _u_d(136, k)
    assert np.array_equal(tpg.pca_loadings(v_rows, center, scale, U, d), tpg.pca_loadings(v_lm, center, scale, U, d))
