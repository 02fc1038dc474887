"""GPU: tpg_pca_loadings (csrc/pca.hip: tpg_u_digits_kernel, tpg_uq_colsum_kernel, tpg_loadings_mfma_kernel,
tpg_loadings_finalize_kernel) against integers, at every pipeline depth.

The output is a pure function of integers up to the last four FP64 operations of the finalize kernel (tests/loadings_ref.py), so
nothing here has a tolerance:

  EXACT tier    center in {0, 1/2, 1, 2}, scale and d powers of two: none of the four operations rounds, fused or not, and the
                device must give exact_loadings() in every bit (np.array_equal).  lr.EXACT_CASES: Q = ceil(n / 128) =
                1 .. 9 in the rows layout and in the locus-major one (odd Q included: the clamped half of the last pair), the locus
                edges m = 1 .. 289 and the column arms k = 1 .. 64 at Q = 1 / 3 / 5, prescribed digits (-64, 63, carries through
                all six, +-(2^40 - 1), amax at and one ulp below a power of two, a spike, amax = 1e-200 and 1e200, one nonzero
                individual per column), and genotypes with a single 1 or 2 per locus -- the last two at every byte position of
                every K step of the first and the last chunk.
  GENERAL tier  column means, binomial scales, d = linspace(9, 2, k), Gaussian U: |got - N / D| <= 2^-53 (|c usum| + 4 |N|) / |D|
                element by element, N and D exact rationals from the quantised u.  Derived in tests/loadings_ref.py, not measured.

tests/test_loadings_host.py shows on the CPU that the exact tier is exact, that the bound holds for both ways of compiling the
subtraction, and which slips of the kernels each panel catches.  The refusals (U all zero, NaN, infinite, |u| >= 1e300) are asserted
nowhere else and are asserted here.
"""
import ctypes as C

import numpy as np
import pytest

from tests import loadings_ref as lr

pytestmark = pytest.mark.gpu

ENUMERIC = 4


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


_panels, _views = {}, {}


def _exact_panel(n, m, k, kind):
    key = (n, m, k, kind)
    if key not in _panels:
        _panels[key] = lr.exact_panel(n, m, k, kind)
    return _panels[key]


def _view(tpg, p, layout):
    """rows: View; locus_major: the second member of View.pair (n a multiple of 8: the fast pack kernel writes it locus-major)"""
    key = (p.name, layout)
    if key not in _views:
        X = tpg.FBM.from_numpy(p.bytes())
        if layout == "rows":
            _views[key] = tpg.View(X)
        else:
            assert p.n % 8 == 0
            _views[key] = tpg.View.pair(X)[1]
    return _views[key]


def _run(tpg, p, layout):
    return tpg.pca_loadings(_view(tpg, p, layout), p.center, p.scale, p.U, p.d)


@pytest.mark.parametrize("case", lr.EXACT_CASES, ids=lr.case_id)
def test_exact_tier_bit_for_bit(tpg, case):
    layout, n, m, k, kind = case
    p = _exact_panel(n, m, k, kind)
    want = lr.exact_loadings(*p.args())
    got = _run(tpg, p, layout)
    assert got.shape == want.shape
    assert np.array_equal(got, want), (case, int((got != want).sum()), "cells differ")
    if layout == "locus_major":  # the same panel through the rows layout: the same bits
        assert np.array_equal(_run(tpg, p, "rows"), got), case


def test_single_entries_name_their_individual(tpg):
    """one 1 or 2 per locus: the loading of locus j IS (g W[rows[j], k] - c_j Wsum_k) 2^-FU / (s_j d_k), so a piece that reached
    the wrong lane, K step, byte or chunk shows as another individual's W.  Said here without the matrix product"""
    for layout, n in (("rows", 641), ("locus_major", 520)):
        p = _exact_panel(n, 256, 2, "single:full")
        G, rows = lr.single_entry_genotypes(n, 256)
        assert np.array_equal(G, p.G)
        _, FU = lr.exponent(p.U)
        W = lr.fixed(p.U, FU)
        g = G[rows, np.arange(256)]
        want = lr.finalize(g[:, None] * W[rows], W.sum(axis=0), FU, p.center, p.scale, p.d)
        assert np.array_equal(_run(tpg, p, layout), want), layout


@pytest.mark.parametrize("layout,ns", [("rows", lr.N_ROWS), ("locus_major", lr.N_LM)])
def test_general_tier_within_the_derived_bound(tpg, layout, ns):
    worst = 0.0
    for n in ns:
        p = lr.general_panel(n, 41, 21)
        got = _run(tpg, p, layout)
        w = lr.error_over_bound(got, *lr.rational_loadings(*p.args()))
        assert w <= 1.0, (layout, n, w)
        worst = max(worst, w)
    print(f"\nloadings general tier, {layout}: worst |error| / bound = {worst:.3f} over n = {list(ns)}")


def _svd(v, k):
    """tpg_pca_partial_svd on a view (tests/test_gpu_view_lm.py: the route that hands the loadings a locus-major view)"""
    from tidypopgen_amd.api import _ptr, check, lib

    d, u, vl = np.zeros(k), np.zeros((v.n, k), order="F"), np.zeros((v.m, k), order="F")
    center, scale, fro = np.zeros(v.m), np.zeros(v.m), C.c_double()
    check(lib.tpg_pca_partial_svd(v.ctx.h, v.h, k, _ptr(d), _ptr(u), _ptr(vl), _ptr(center), _ptr(scale), C.byref(fro)))
    return dict(d=d, u=u, v=vl, center=center, scale=scale)


@pytest.mark.parametrize("route,n", [("gt_pca_partialSVD", 264), ("gt_pca_partialSVD", 641), ("pair", 264)])
def test_loadings_in_place(tpg, route, n):
    """the loadings a PCA returns lie within the derived bound of the quantised reference computed from the u, d, center and scale
    it returns beside them.  "pair": tpg_pca_partial_svd on the locus-major member of View.pair"""
    k = 4
    p = lr.general_panel(n, 97, k)
    X = tpg.FBM.from_numpy(p.bytes())
    r = tpg.gt_pca_partialSVD(X, k=k) if route == "gt_pca_partialSVD" else _svd(tpg.View.pair(X)[1], k)
    assert (r["d"] > 0).all()
    w = lr.error_over_bound(r["v"], *lr.rational_loadings(p.G, r["u"], r["center"], r["scale"], r["d"]))
    print(f"\nloadings in place, {route} n = {n}: worst |error| / bound = {w:.3f}")
    assert w <= 1.0, (route, n, w)


@pytest.mark.parametrize("layout,n", [("rows", 257), ("locus_major", 264)])
def test_refusals_leave_the_output_untouched(tpg, layout, n):
    from tidypopgen_amd.api import _ptr, lib

    p = _exact_panel(n, 45, 5, "spike")
    v = _view(tpg, p, layout)
    bad = {"zero": np.zeros_like(p.U), "nan": p.U.copy(), "inf": p.U.copy(), "1e300": p.U.copy()}
    bad["nan"][n - 1, 4] = np.nan
    bad["inf"][0, 2] = -np.inf
    bad["1e300"][5, 0] = 1e300
    for name, U in bad.items():
        U = np.asfortranarray(U)
        out = np.full((p.m, p.k), 7.0, order="F")
        rc = lib.tpg_pca_loadings(v.ctx.h, v.h, _ptr(p.center), _ptr(p.scale), _ptr(U), _ptr(p.d), p.k, _ptr(out))
        assert rc == ENUMERIC, (name, rc)
        assert (out == 7.0).all(), name
    # and the view still serves
    assert np.array_equal(_run(tpg, p, layout), lr.exact_loadings(*p.args()))
