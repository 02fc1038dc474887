"""GPU: the digit-split Gram route of csrc/pca.hip on PRESCRIBED weights and panels (tests/gramdig_ref.py), bit for bit.

TPG_GRAM_DIGITS=1 sends pca_gram down the digit route whatever the class route's cost model says.  The route is integer
arithmetic, so with center = 0 the call returns ldexp((double)S, -F) for the integer matrix S = sum_j g_ij g_kj W_j that
gramdig_ref.exact_S forms on the CPU: every element is compared for EQUALITY where |S| < 2^53 and within one unit in the last
place above (the int64 -> double conversion; every T = 8 case is of that kind, see gramdig_ref).  The cases prescribe the weights
digit by digit -- T = 4 .. 8, i.e. tpg_pca_gram_kernel<4> alone and followed by <1>, <2>, <3>, <4> -- K ranges of every length
modulo three with ragged and full last groups, row tiles with 0 .. 3 remainder tiles, and the two patches of the unit order at
n = 1 185; each case asserts its arm on the launch plan restated for THIS device's CU count.  Panels: "onehot" (locus j typed in
one individual: the diagonal reads every W_j back, which separates the weights of tpg_pca_digits_kernel from the MFMA kernel;
it runs first), "pair" (locus j non-zero for its pair of individuals only: S[a, b] names its loci) and "dense".

test_weights_read_back settles whether the device's 1 / (s * s) has numpy's bits.  Every weight that scale_of() derives is stable
under +-4 units in the last place of 1 / s^2, so those cases would pass either way; the T = 8 scales (26 significant bits: s s
exact, one division) and the top_carry scales are the ones that need the division correctly rounded, and they pass: the
device's division is IEEE.  No T = 8 scale had to be left out.

Besides equality, for every center = 0 case: K exactly symmetric, a second call gives the same bits, and the true-weight bound
holds.  The centred calls (center = the column mean, which the library recognises, and a general center) are held to bound_mean /
bound_general, their asymmetry to asym_mean / asym_general (a centred element is ((S' - r_i) - r_k) + C, which need not round
as ((S' - r_k) - r_i) + C does), all derived in gramdig_ref.  The overflow cases -- the two panels whose sums pass 2^63 and one
whose largest weight would need a ninth digit -- return the class route's numbers, or TPG_ENUMERIC with the output untouched
when the digit route is forced.  Every test prints its worst error / bound ratio.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import gramcls_ref as gr
from tests import gramdig_ref as gd

pytestmark = pytest.mark.gpu

TPG_ENUMERIC = 4


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


@pytest.fixture(scope="module")
def cus():
    hip, n = C.CDLL("libamdhip64.so.7"), C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(n), 63, 0) == 0 and n.value > 0  # hipDeviceAttributeMultiprocessorCount
    return n.value


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _digits(tpg, v, center, scale):
    with _env(TPG_GRAM_DIGITS="1", TPG_GRAM_CLASSES=None):
        return tpg.pca_gram(v, center, scale)


def _zero(tpg, cus, name, kinds=None):
    """center = 0 on the case's panels: equality with the exact integer matrix, symmetry, the same bits twice, the true weights"""
    c = gd.BY_NAME[name]
    p = c.check_arm(cus)
    for kind in kinds or [k for k in c.kinds if k != "onehot"]:
        g, S = c.panel(kind)
        v = tpg.View(tpg.FBM.from_numpy(g))
        K = _digits(tpg, v, np.zeros(c.m), c.scale)
        again = _digits(tpg, v, np.zeros(c.m), c.scale)
        ok, n_exact, n_wide = gd.check_K0(K, S, c.F)
        ref = gd.exact_K0(S, c.F)
        bad = np.argwhere(K != ref)
        err = np.abs(K.astype(gd.LD) - gd.true_K0(g, c.scale))
        bound = gd.bound_true(g, c.scale, c.F, K)
        ratio = float((err / np.where(bound > 0, bound, 1)).max())
        print(f"gramdig {name:16s} {kind:6s} T={c.T} F={c.F} S={p.S} units={p.nun}: {len(bad)} of {K.size} elements differ from "
              f"ldexp(S, -F) ({n_wide} with |S| >= 2^53), true-weight error / bound = {ratio:.3g}")
        assert np.array_equal(K, K.T), (name, kind)
        assert ok, (name, kind, "first differences (i, k):", bad[:8].tolist(),
                    [(int(S[i, k]), float(K[i, k]) * 2.0 ** c.F) for i, k in bad[:4]])
        assert np.array_equal(again, K), (name, kind)
        assert np.all(err <= bound) and np.all(K[bound == 0] == 0), (name, kind, ratio)


@pytest.mark.parametrize("name", [c.name for c in gd.CASES if "onehot" in c.kinds])
def test_weights_read_back(tpg, cus, name):
    """locus j is typed in one individual only: K[a, a] = sum of g^2 W_j 2^-F over its few loci, nothing else is non-zero"""
    _zero(tpg, cus, name, kinds=["onehot"])


@pytest.mark.parametrize("name", gd.names("digits"))
def test_digits(tpg, cus, name):
    """T = 4 .. 8: <4> alone, <4> + <1>, <2>, <3>, <4>; all digits 63, -64 under a positive top digit, one digit at every position,
    borrow chains, W = 1 beside the largest weight a panel can hold; a top digit that needs the carry rule (top_carry_*)"""
    _zero(tpg, cus, name)


@pytest.mark.parametrize("name", gd.names("K ranges"))
def test_k_ranges(tpg, cus, name):
    """n = 130: one K range of 1, 2, 3, 4, 5, 7 groups with one locus or all 128 in the last one; 16, 17, 19, 24, 25 groups cut
    in two or three at 256 CUs (the arm asserts what this device's plan gives)"""
    _zero(tpg, cus, name)


def test_k_range_lengths_cover_every_residue(cus):
    seen = set()
    for name in gd.names("K ranges"):
        seen |= {(k1 - k0) % 3 for k0, k1 in gd.BY_NAME[name].check_arm(cus).ranges}
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("name", gd.names("row tiles"))
def test_row_tiles(tpg, cus, name):
    """n = 1 .. 289: no full super-tile with 1, 2, 3 remainder tiles, one with 0 .. 3, two with 0 and 2, partial last tiles"""
    _zero(tpg, cus, name)


def test_two_patches(tpg, cus):
    """n = 1 185: nine full super-tiles, i.e. a second patch of the unit order, and two remainder tiles"""
    _zero(tpg, cus, "patches_1185")


CENTRED = [n for n in gd.names("digits") + gd.names("row tiles")]


@pytest.mark.parametrize("name", CENTRED)
def test_centred(tpg, cus, name):
    """the dense panel again with center = the column mean (assemble without rvec, then the double centring kernels) and with a
    general center (rvec from the RAW sweep, Cc from 512 partial sums).  Exact symmetry is asserted for center = 0 only: a centred
    element is ((S'_ik - r_i) - r_k) + C, and (S' - r_i) - r_k need not round as (S' - r_k) - r_i does (digits_T8, whose row means
    differ by many binades, shows it in the last place); the centred calls are held to the derived asym_mean / asym_general"""
    c = gd.BY_NAME[name]
    c.check_arm(cus)
    g, S = c.panel("dense")
    v = tpg.View(tpg.FBM.from_numpy(g))
    mean = g.sum(axis=0, dtype=np.int64) / c.n  # (the double the library compares with: (n1 + 2 n2) / n)
    # S' itself is exact below 2^53; above, its conversion rounds once: a relative 2^-53 in bound_centred's first term
    rel = 0.0 if c.size == "exact" else gd.U
    K = _digits(tpg, v, mean, c.scale)
    err = float(np.abs(K.astype(gd.LD) - gd.centred_exact(S, c.F)).max())
    bound = gd.bound_centred(rel, gd.exact_K0(S, c.F), c.n)
    print(f"gramdig {name:16s} column mean   : error / bound = {err / bound if bound else 0.0:.3g}")
    assert np.array_equal(_digits(tpg, v, mean, c.scale), K)
    assert err <= bound, (name, err, bound)
    asym = float(np.abs(K - K.T).max())
    print(f"gramdig {name:16s} column mean   : asymmetry / bound = {asym / gd.asym_mean(S, c.F) if asym else 0.0:.3g}")
    assert asym <= gd.asym_mean(S, c.F), (name, asym)
    center = 0.75 * mean + 0.3
    assert not np.any(center == mean)
    K = _digits(tpg, v, center, c.scale)
    e = np.abs(K.astype(gd.LD) - gd.general_exact(g, c.W, c.F, center))
    b = gd.bound_general(g, c.W, c.F, center, S)
    print(f"gramdig {name:16s} general center: error / bound = {float((e / b).max()):.3g}")
    assert np.array_equal(_digits(tpg, v, center, c.scale), K)
    assert np.all(e <= b), (name, float((e / b).max()))
    sb = gd.asym_general(g, c.W, c.F, center, S)
    print(f"gramdig {name:16s} general center: asymmetry / bound = {float((np.abs(K - K.T) / sb).max()):.3g}")
    assert np.all(np.abs(K - K.T) <= sb), name


@pytest.mark.parametrize("name", list(gd.OVERFLOW_CASES))
def test_overflow_takes_the_class_route(tpg, name):
    """4 sum W >= 2^63, or a largest weight that asks for a ninth digit, and nothing forced: the class route's numbers whatever
    its cost model says, within rel_fold64"""
    g, scale = gd.overflow_case(name)
    _, T, F = gd.digit_plan(scale)
    assert T == 9 or not gd.guard(scale, F)
    v = tpg.View(tpg.FBM.from_numpy(g))
    with _env(TPG_GRAM_DIGITS=None, TPG_GRAM_CLASSES=None, TPG_GRAM_FOLD64=None):
        K = tpg.pca_gram(v, np.zeros(g.shape[1]), scale)
    meta = gr.describe(scale, w_max=2.0 ** 33)
    assert meta.nruns == 1  # one weight class: the mixed fold's deviation term is zero, rel_fold64 bounds either kernel
    R = gr.exact(g, scale)
    err = np.abs(K.astype(gd.LD) - R)
    bound = gd.LD(gr.rel_fold64(meta)) * R
    print(f"gramdig overflow {name}: T={T} F={F}, class route error / bound = {float((err / np.where(bound > 0, bound, 1)).max()):.3g}")
    assert np.array_equal(K, K.T)
    assert np.all(err <= bound)


@pytest.mark.parametrize("name", list(gd.OVERFLOW_CASES))
def test_overflow_refused_when_digits_are_forced(tpg, name):
    """TPG_GRAM_DIGITS=1: TPG_ENUMERIC, a message that names the bound, the output untouched, and the context still good"""
    from tidypopgen_amd import _lib
    from tidypopgen_amd.api import _ptr

    g, scale = gd.overflow_case(name)
    v = tpg.View(tpg.FBM.from_numpy(g))
    K = np.full((v.n, v.n), -7.0, order="F")
    center, sc = np.zeros(v.m), np.ascontiguousarray(scale)
    with _env(TPG_GRAM_DIGITS="1", TPG_GRAM_CLASSES=None):
        rc = _lib.lib.tpg_pca_gram(v.ctx.h, v.h, _ptr(center), _ptr(sc), _ptr(K))
        msg = _lib.lib.tpg_last_error().decode()
        with pytest.raises(_lib.TpgError) as e:
            tpg.pca_gram(v, center, sc)
    assert rc == TPG_ENUMERIC and e.value.code == TPG_ENUMERIC and ("ninth digit" if name == "ninth_digit" else "2^63") in msg, (rc, msg)
    assert np.all(K == -7.0)
    c = gd.BY_NAME["digits_T5"]
    g2, S2 = c.panel("dense")
    assert gd.check_K0(_digits(tpg, tpg.View(tpg.FBM.from_numpy(g2)), np.zeros(c.m), c.scale), S2, c.F)[0]
