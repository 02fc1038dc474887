"""CPU: the restatement of the digit-split Gram route (tests/gramdig_ref.py) against itself -- the builder's assertions, the
launch plan's properties, the model of the device's order of work against the exact integer matrix, the faults the model
can take, and the overflow threshold.  No GPU: what runs on the device is tests/test_gpu_gramdig.py, on the same cases.

Every fault of gramdig_ref.FAULTS is run on every panel of every case.  visible() PREDICTS from the case alone whether the
fault can move an element, and the test asserts that the model leaves exact_S() exactly there -- so the table of invisible
(fault, case) pairs is this function, with the reason in the string it returns:

  digit0_dropped        visible everywhere (every case has a weight whose lowest digit is not zero)
  borrow_lost           invisible on k_1_1: its one weight is the all-63 anchor, no digit of it borrows
  planes_swapped        visible everywhere
  pass2_shift           invisible at T = 4: one pass (digits_T4)
  pass2_base0           invisible at T = 4: one pass; and on k_1_1, whose one weight is the all-63 anchor: the digit the
                        second pass misreads (digit 0 of locus 0) equals the one it should read (digit 4)
  last_group_dropped    visible everywhere
  dead_unmasked         invisible where every K range is a multiple of three groups long (k_3_*), and where the last group of
                        every ragged range holds no locus past its first 32 (m = 128 (KG - 1) + 1 with one range: what the
                        unmasked steps 1 .. 3 read again is padding)
  dead1_kg              invisible where every K range is a multiple of three groups long (k_3_*)
  boundary_up           invisible where S = 1 and where S divides KG (k_16, k_24): no boundary is rounded
  rem_full_next_slab    invisible where there is no full super-tile or no remainder tile (n <= 128, n = 256)
  corner_tb_no_F4       invisible with no remainder tile, and with no full super-tile (F4 = 0: n <= 96)
  patch2_first_missing  visible on patches_1185 only: nsbf > 8 nowhere else
  pad_loci_digits       invisible EVERYWHERE: a padding locus carries code 3 on the A side, for which the v_perm selector
                        is the constant 0 whatever the digit planes hold -- the zero digits are a second safeguard, and no
                        test can tell whether they are there.  The model says so rather than pretending otherwise.

NAMED lists, per fault, the cases that were built for it; the prediction must say "visible" there.
"""
import numpy as np
import pytest

from tests import gramdig_ref as gd


def visible(fault, c, p):
    """None if the fault must move an element of S on case c under plan p, else the reason why it cannot"""
    lens = [k1 - k0 for k0, k1 in p.ranges]
    if fault == "borrow_lost":
        return None if not np.array_equal(gd.digits(c.W, c.T)[0], gd.digits(c.W, c.T, "borrow_lost")[0]) else "no digit borrows"
    if fault == "pass2_shift":
        return None if c.T > 4 else "one pass"
    if fault == "pass2_base0":
        if c.T == 4:
            return "one pass"
        D = np.zeros((c.T, 128 * p.KG), dtype=np.int64)
        D[:, :c.m] = gd.digits(c.W, c.T)[0]
        same = np.array_equal(gd.misread_pass2(D, c.T - 4)[:, :c.m], D[4:, :c.m])
        return "the misread digits equal the right ones" if same else None
    if fault == "dead1_kg":
        return None if any(n % 3 for n in lens) else "every range is whole triples"
    if fault == "dead_unmasked":
        if not any(n % 3 for n in lens):
            return "every range is whole triples"
        return None if any((k1 - k0) % 3 and 128 * (k1 - 1) + 32 < c.m for k0, k1 in p.ranges) else "steps 1 .. 3 of the last group are padding"
    if fault == "boundary_up":
        return None if any(p.KG * (ks + 1) % p.S for ks in range(p.S - 1)) else "no boundary is rounded"
    if fault == "rem_full_next_slab":
        return None if p.nsbf >= 1 and p.rem >= 1 else "no remainder x full unit"
    if fault == "corner_tb_no_F4":
        return None if p.nsbf >= 1 and p.rem >= 1 else "no corner, or F4 = 0"
    if fault == "patch2_first_missing":
        return None if p.nsbf > 8 else "one patch"
    if fault == "pad_loci_digits":
        return "code 3 selects the constant 0 on the A side"
    return None


NAMED = {
    "digit0_dropped": gd.names("digits"),
    "borrow_lost": [f"digits_T{T}" for T in (4, 5, 6, 7, 8)],
    "planes_swapped": gd.names("digits") + gd.names("row tiles"),
    "pass2_shift": ["digits_T5", "digits_T6", "digits_T7", "digits_T8", "top_carry_F", "top_carry_T"],
    "pass2_base0": ["digits_T5", "digits_T6", "digits_T7", "digits_T8", "top_carry_F", "top_carry_T"],
    "last_group_dropped": gd.names("K ranges"),
    "dead_unmasked": ["k_1_128", "k_2_256", "k_4_512", "k_5_640", "k_7_896", "k_16", "k_17", "k_19", "k_24", "k_25"],
    "dead1_kg": [n for n in gd.names("K ranges") if not n.startswith("k_3_")],
    "boundary_up": ["k_17", "k_19", "k_25"],
    "rem_full_next_slab": ["tiles_129", "tiles_160", "tiles_192", "tiles_224", "tiles_289", "patches_1185"] + gd.names("K ranges"),
    "corner_tb_no_F4": ["tiles_129", "tiles_160", "tiles_192", "tiles_224", "tiles_289", "patches_1185"],
    "patch2_first_missing": ["patches_1185"],
    "pad_loci_digits": [],
}


def test_named_cases_exist_and_cover_every_fault():
    assert set(NAMED) == set(gd.FAULTS)
    for fault, cases in NAMED.items():
        assert cases or fault == "pad_loci_digits"
        for name in cases:
            c = gd.BY_NAME[name]
            assert visible(fault, c, c.check_arm()) is None, (fault, name)


@pytest.mark.parametrize("num_cu", [256, 304, 64, 8])
def test_every_case_builds_and_holds_its_arm(num_cu):
    """the builder's own assertions (weights restated and stable under +-4 ulp, S inside its size class, inside the overflow
    condition) run when the panels are made; the arm of every case on the plan of four CU counts"""
    for c in gd.CASES:
        c.check_arm(num_cu)
        if num_cu == 256:
            for kind in c.kinds:
                c.panel(kind)
    seen = set()
    for name in gd.names("K ranges"):
        seen |= {(k1 - k0) % 3 for k0, k1 in gd.BY_NAME[name].check_arm(num_cu).ranges}
    assert seen == {0, 1, 2}


def test_digit_counts_and_passes():
    got = {c.T: gd.tds(c.T) for c in gd.CASES}
    assert got == {4: [4], 5: [4, 1], 6: [4, 2], 7: [4, 3], 8: [4, 4]}
    for c in gd.CASES:
        d, left = gd.digits(c.W, c.T)
        assert not left.any() and d.min() >= -64 and d.max() <= 63
        assert np.array_equal(sum(d[t] << (7 * t) for t in range(c.T)), c.W)


def test_top_digit_carry_is_what_the_plain_rule_loses():
    """w = 127 under T = (wbits + 29) / 7, F = 7 T - 1 - wbits: the weight 127 * 2^27 does not fit five balanced digits"""
    W = 127 << 27
    d, left = gd.digits([W], 5)
    assert left[0] == 1 and gd.from_digits(d[:, 0]) == W - 128 ** 5
    for name in ("top_carry_F", "top_carry_T"):
        c = gd.BY_NAME[name]
        assert not gd.digits(c.W, c.T)[1].any() and c.F >= 22


def test_plan_keeps_int32_sums():
    """the loci of one wave-unit's K range times 256 (the largest |2 digit * dosage| of a locus) stay below 2^31"""
    worst = 0
    for n in (1000, 2000, 5000, 10000):
        for m in (650_000, 1_000_000, 5_000_000, 20_000_000):
            worst = max(worst, gd.longest_range_loci(n, m, 256))
    for n, m in ((1000, 650_000), (5000, 10 ** 6), (5000, 2 * 10 ** 7), (1000, 2 * 10 ** 7)):
        assert gd.longest_range_loci(n, m, 256) * 256 < 2 ** 31
    assert worst == 3_333_376 and worst * 256 < 2 ** 31  # (2^31 / 256 = 8 388 608 loci allowed)


@pytest.mark.parametrize("name", [c.name for c in gd.CASES])
def test_model_equals_exact_and_faults_leave_it(name):
    c = gd.BY_NAME[name]
    p = c.check_arm()
    for kind in c.kinds:
        g, S = c.panel(kind)
        assert np.array_equal(gd.model(g, c.W, c.T), S), (name, kind)
        for fault in gd.FAULTS:
            reason = visible(fault, c, p)
            differs = not np.array_equal(gd.model(g, c.W, c.T, fault=fault), S)
            assert differs == (reason is None), (name, kind, fault, reason)


def test_model_at_other_cu_counts():
    """the K split depends on the CU count; the sum does not"""
    for name in ("k_16", "k_19", "k_25"):
        c = gd.BY_NAME[name]
        g, S = c.panel("dense")
        for cu in (8, 64, 304):
            assert np.array_equal(gd.model(g, c.W, c.T, num_cu=cu), S)


def test_check_K0_and_bounds_on_the_exact_matrix():
    for name in ("digits_T5", "digits_T7_wide", "digits_T8"):
        c = gd.BY_NAME[name]
        g, S = c.panel("dense")
        K = gd.exact_K0(S, c.F)
        ok, nx, nw = gd.check_K0(K, S, c.F)
        assert ok and (nw > 0) == (c.size == "wide")
        err = np.abs(K.astype(gd.LD) - gd.true_K0(g, c.scale))
        assert np.all(err <= gd.bound_true(g, c.scale, c.F, K))
        K2 = K.copy()
        K2[3, 5] = np.nextafter(np.nextafter(K2[3, 5], np.inf), np.inf)
        assert not gd.check_K0(K2, S, c.F)[0]
    # a weight that is off by little more than the bound's worth of units leaves the true-weight bound of its pair's element
    c = gd.BY_NAME["digits_T6"]
    g, S = c.panel("pair")
    W2 = c.W.copy()
    j = int(np.argmax(c.W))
    a, b = np.nonzero(g[:, j])[0]
    W2[j] += int(gd.bound_true(g, c.scale, c.F, gd.exact_K0(S, c.F))[a, b] * 2.0 ** c.F) + 2
    K = gd.exact_K0(gd.exact_S(g, W2), c.F)
    assert np.any(np.abs(K.astype(gd.LD) - gd.true_K0(g, c.scale)) > gd.bound_true(g, c.scale, c.F, K))


def test_centred_references():
    c = gd.BY_NAME["tiles_33"]
    g, S = c.panel("dense")
    ref = gd.centred_exact(S, c.F)
    assert float(np.abs(gd.centre(gd.exact_K0(S, c.F).astype(gd.LD)) - ref).max()) <= 2.0 ** -58 * float(S.max()) * 2.0 ** -c.F
    mean = g.sum(axis=0) / c.n
    assert float(np.abs(gd.general_exact(g, c.W, c.F, mean) - ref).max()) <= 2.0 ** -50 * float(S.max()) * 2.0 ** -c.F
    assert np.all(gd.bound_general(g, c.W, c.F, mean + 0.25, S) > 0)


def test_overflow_threshold():
    """4 sum W < 2^63 is the condition, the guard implies it, and the two panels of the issue are outside both: their sums
    pass 2^63 (a wrapped int64 would be what the library returned)"""
    for c in gd.CASES:
        assert gd.guard(c.scale, c.F) and gd.safe(c.W)
    g, scale = gd.overflow_case("ninth_digit")
    assert gd.digit_plan(scale) == (33, 9, 22) and gd.digits(gd.weights(scale, 22), 8)[1].all()  # eight digits lose the carry
    for name, lo in (("scale_1e-3", 34359), ("scale_1e-4", 343)):
        g, scale = gd.overflow_case(name)
        wbits, T, F = gd.digit_plan(scale)
        assert (T, F) == ((7, 28) if name == "scale_1e-3" else (8, 28))
        W = gd.weights(scale, F)
        assert not gd.safe(W) and not gd.guard(scale, F)
        S = gd.exact_S(g, W, wide=True)
        assert max(int(x) for x in S.reshape(-1)) >= 2 ** 63
        assert 2 ** 63 // int(W[0]) == lo  # sum g g of a pair up to 34 359 / 343 fits, one more wraps
    # the guard never admits a panel the condition does not: weights at the edge, with the sum moved across it
    rng = np.random.default_rng(1)
    for _ in range(200):
        T = int(rng.integers(6, 9))
        m = int(rng.integers(50, 4000))
        wbits = {6: 13, 7: 20, 8: 27}[T]
        F = 7 * T - 1 - wbits
        per = 2.0 ** 61 / m / 2.0 ** F * rng.uniform(0.9, 1.1)
        w = np.minimum(per * rng.uniform(0.5, 1.5, size=m), 0.97 * 2.0 ** wbits)
        scale = 1.0 / np.sqrt(w)
        W = gd.weights(scale, F)
        if gd.guard(scale, F):
            assert gd.safe(W)
