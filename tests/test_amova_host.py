"""CPU-only: the host side of include/tpg.h "AMOVA" -- tpg_amova_perm_labels against its restatement, the finisher
tpg_amova_from_sums on known answers and against its float64 restatement, the ordered class sum of tests/amova_ref.py against its
exact route and against wrong sums (the reference has teeth), and csrc/host/host_amova.h as a stand-alone program under the host
sanitizers."""
from fractions import Fraction

import numpy as np
import pytest

from tests import amova_ref as ar

SIZES = (3, 7, 2, 5, 4, 9, 1)  # an unbalanced design: seven populations in three regions
REGION = (0, 0, 1, 1, 1, 2, 2)
R_VALUES = (0, 1, 2, 7, 2 ** 31 - 1)


def _tpg():
    import tidypopgen_amd as t

    return t


def _design(seed=None, sizes=SIZES):
    pop = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    if seed is not None:
        pop = np.random.default_rng(seed).permutation(pop).astype(np.int32)
    return pop


# ---- a. the label rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1, 2])
@pytest.mark.parametrize("seed", [11, 2 ** 40 + 9])
def test_perm_labels_equal_the_restatement(scheme, seed):
    tpg = _tpg()
    pop = _design(3)
    pop[np.flatnonzero(pop == 5)[:2]] = -1  # two of the nine of population 5 are outside
    n, P, G = len(pop), len(SIZES), 3
    reg = np.array(REGION, dtype=np.int32)
    rows = {}
    for r in R_VALUES:
        po, go = tpg.amova_perm_labels(n, pop, P, reg, G, scheme, seed, r)
        wp, wg = ar.perm_labels(n, pop, P, reg, G, scheme, seed, r)
        assert np.array_equal(po, wp) and np.array_equal(go, wg), r
        assert np.array_equal(np.bincount(po[po >= 0], minlength=P), np.bincount(pop[pop >= 0], minlength=P))  # sizes preserved
        assert np.array_equal(po < 0, pop < 0)
        if scheme == 1:  # nobody leaves a region
            assert np.array_equal(reg[po[po >= 0]], reg[pop[pop >= 0]])
        if scheme == 2:  # the populations move as wholes: the regions keep their numbers of populations
            assert np.array_equal(po, pop) and np.array_equal(np.bincount(go, minlength=G), np.bincount(reg, minlength=G))
        else:
            assert np.array_equal(go, reg)
        rows[r] = (tuple(po), tuple(go))
    assert rows[0] == (tuple(pop), tuple(reg))  # r = 0 is the identity
    if scheme < 2:  # (seven populations in regions of 2, 3, 2 have only 210 arrangements: scheme 2 may repeat one)
        assert len(set(rows.values())) == len(rows)  # distinct r: distinct relabelings
        assert tpg.amova_perm_labels(n, pop, P, reg, G, scheme, seed + 1, 1)[0].tolist() != list(rows[1][0])
    else:
        assert len(set(rows.values())) >= 3
    name = ("ST", "SC", "CT")[scheme]
    assert np.array_equal(tpg.amova_perm_labels(n, pop, P, reg, G, name, seed, 7)[0], rows[7][0])


def test_scheme_0_is_the_global_scheme_of_the_fst_test():
    tpg = _tpg()
    pop = _design(5)
    n, P = len(pop), len(SIZES)
    for r in R_VALUES:
        want = tpg.fst_perm_labels(n, pop, P, "global", 0, 0, 77, r)
        assert np.array_equal(tpg.amova_perm_labels(n, pop, P, REGION, 3, 0, 77, r)[0], want)
        po, go = tpg.amova_perm_labels(n, pop, P, None, 0, 0, 77, r)  # without regions
        assert np.array_equal(po, want) and go is None


def test_perm_labels_refuse_bad_arguments():
    tpg = _tpg()
    pop = _design(1)
    n, P = len(pop), len(SIZES)
    ok = dict(pop=pop, npop=P, reg=REGION, G=3, scheme=0, r=1)
    bad_pop, empty = pop.copy(), pop.copy()
    bad_pop[3] = P
    empty[empty == 6] = 0  # population 6 is empty
    for kw in (dict(scheme=3), dict(scheme=-1), dict(r=-1), dict(r=2 ** 31), dict(pop=bad_pop), dict(pop=empty),
               dict(reg=(0, 0, 1, 1, 1, 3, 2)), dict(reg=(0, 0, 1, 1, 1, 1, 1)), dict(G=0, reg=None, scheme=1), dict(G=0, reg=None, scheme=2),
               dict(G=8, reg=(0, 1, 2, 3, 4, 5, 7))):
        a = dict(ok)
        a.update(kw)
        with pytest.raises(tpg._lib.TpgError) as e:
            tpg.amova_perm_labels(n, a["pop"], a["npop"], a["reg"], a["G"], a["scheme"], 5, a["r"])
        assert e.value.code == 1, kw
    tpg.amova_perm_labels(n, ok["pop"], P, REGION, 3, 0, 5, 1)


# ---- b. known answers of the finisher -----------------------------------------------------------------------------------------
def _expected_matrix(pop, reg, a, b, c):
    """0 on the diagonal, 2c inside a population, 2(b + c) inside a region, 2(a + b + c) elsewhere (object array of Fractions)"""
    n = len(pop)
    D = np.empty((n, n), dtype=object)
    for i in range(n):
        for j in range(n):
            D[i, j] = (Fraction(0) if i == j else 2 * c if pop[i] == pop[j] else 2 * (b + c) if reg is None or reg[pop[i]] == reg[pop[j]]
                       else 2 * (a + b + c))
    return D


def _sums_of(D, lab, k):
    return [sum((D[i, j] for i in np.flatnonzero(lab == c) for j in np.flatnonzero(lab == c)), Fraction(0)) for c in range(k)]


@pytest.mark.parametrize("levels", [3, 2])
def test_the_expected_distance_matrix_returns_its_components(levels):
    tpg = _tpg()
    a, b, c = Fraction(3, 7), Fraction(5, 11), Fraction(13, 4)
    pop = _design(9)
    reg = np.array(REGION) if levels == 3 else None
    D = _expected_matrix(pop, reg, a, b, c)
    T = _sums_of(D, np.zeros(len(pop), dtype=int), 1)[0]
    W = _sums_of(D, pop, len(SIZES))
    Rg = _sums_of(D, reg[pop], 3) if levels == 3 else None
    (sa, sb, sc), _ = ar.from_sums_exact(SIZES, W, T, reg, 3 if levels == 3 else 0, Rg)
    assert (sb, sc) == (b, c) and (sa == a if levels == 3 else sa is None)  # exact
    got = tpg.amova_from_sums(SIZES, [float(x) for x in W], float(T), reg, None if Rg is None else [float(x) for x in Rg])
    want = [float(a), float(b), float(c)] if levels == 3 else [float(b), float(c)]
    assert np.allclose(got["sigma2"][3 - len(want):3], want, rtol=1e-12, atol=0)
    tot = float(a + b + c) if levels == 3 else float(b + c)
    assert np.isclose(got["sigma2"][3], tot, rtol=1e-12)
    if levels == 3:
        assert np.allclose(got["phi"], [float(a) / tot, float(b / (b + c)), float(a + b) / tot], rtol=1e-12, atol=0)
        assert np.array_equal(got["df"], [2, 4, 24, 30])
    else:
        assert np.isnan(got["phi"][:2]).all() and np.isclose(got["phi"][2], float(b / (b + c)), rtol=1e-12)
        assert np.isnan(got["df"][0]) and np.array_equal(got["df"][1:], [6, 24, 30])


def test_the_ssd_are_the_nested_anova_sums_of_squares_of_the_dosages():
    pop = _design(13)
    reg = np.array(REGION)
    rng = np.random.default_rng(14)
    codes = rng.binomial(2, rng.uniform(0.1, 0.9, size=40), size=(len(pop), 40)).astype(np.uint8)  # complete: nothing missing
    raw, V, _ = ar.sqdist(codes)
    assert (V == 40).all() and (np.diag(raw) == 0).all()
    lab0 = np.zeros(len(pop), dtype=int)
    T = ar.class_sums_int(raw, lab0, 1)[0]
    W, Rg = ar.class_sums_int(raw, pop, len(SIZES)), ar.class_sums_int(raw, reg[pop], 3)
    _, ssd = ar.from_sums_exact(SIZES, W, T, reg, 3, Rg)

    def within(lab):  # sum over loci and classes of the squared deviations from the class mean
        tot = Fraction(0)
        for cl in np.unique(lab):
            x = codes[lab == cl].astype(int)
            for col in x.T:
                mean = Fraction(int(col.sum()), len(col))
                tot += sum((Fraction(int(v)) - mean) ** 2 for v in col)
        return tot

    assert ssd[3] == within(lab0)
    assert ssd[2] == within(pop)
    assert ssd[1] + ssd[2] == within(reg[pop])
    assert ssd[0] == within(lab0) - within(reg[pop])


# ---- c. the finisher against its restatement ------------------------------------------------------------------------------------
def _random_case(rng, sizes, reg):
    P = len(sizes)
    W = rng.uniform(0, 50, size=P) * np.array(sizes) ** 2
    G = 0 if reg is None else max(reg) + 1
    Rg = None if reg is None else np.array([W[np.array(reg) == g].sum() for g in range(G)]) * rng.uniform(1, 3, size=G)
    T = float((Rg.sum() if reg is not None else W.sum()) * rng.uniform(0.8, 4))
    return W, Rg, T


@pytest.mark.parametrize("sizes,reg", [(SIZES, REGION), (SIZES, None), ((4, 4, 4, 4), (0, 0, 1, 1)), ((2, 3), None),
                                       ((5, 6, 7), (0, 0, 0)),      # one region: df among regions = 0
                                       ((5, 6, 7), (0, 1, 2)),      # every population its own region: df among populations = 0
                                       ((1, 1, 1, 1), (0, 0, 1, 1)),  # populations of one: df within populations = 0
                                       ((3,), None)])               # one population without regions: df among populations = 0
def test_from_sums_equals_the_restatement_bit_for_bit(sizes, reg):
    tpg = _tpg()
    rng = np.random.default_rng(len(sizes) * 7 + (0 if reg is None else 1))
    for _ in range(20):
        W, Rg, T = _random_case(rng, sizes, reg)
        got = tpg.amova_from_sums(sizes, W, T, reg, Rg)
        want = ar.from_sums(sizes, W, T, reg, Rg)
        for key in ("df", "ssd", "msd", "ncoef", "sigma2", "phi"):
            assert ar.same_values(got[key], want[key]), (key, got[key], want[key])
    g = tpg.amova_from_sums(sizes, W, T, reg, Rg)
    if reg == (0, 0, 0):
        assert np.isnan(g["msd"][0]) and np.isnan(g["ncoef"][1:]).all() and np.isnan(g["sigma2"][[0, 3]]).all()
        assert np.isnan(g["phi"][[0, 2]]).all() and np.isfinite(g["phi"][1]) and np.isfinite(g["sigma2"][1:3]).all()
    if reg == (0, 1, 2):
        assert np.isnan(g["msd"][1]) and np.isnan(g["ncoef"][0]) and np.isnan(g["sigma2"][[0, 1, 3]]).all() and np.isnan(g["phi"]).all()
        assert np.isfinite(g["sigma2"][2])
    if sizes == (1, 1, 1, 1):
        assert np.isnan(g["msd"][2]) and np.isnan(g["sigma2"]).all() and np.isnan(g["phi"]).all()
    if sizes == (3,):
        assert np.isnan(g["msd"][1]) and np.isnan(g["ncoef"]).all() and np.isnan(g["phi"]).all() and np.isfinite(g["sigma2"][2])


def test_from_sums_refuses_bad_arguments():
    tpg = _tpg()
    for sizes, reg, rs in (((3, 0, 2), None, None), ((3, 4, 2), (0, 0, 2), (1.0, 1.0, 1.0)), ((3, 4, 2), (0, 0, 3), (1.0, 1.0, 1.0))):
        with pytest.raises((tpg._lib.TpgError, ValueError)):
            tpg.amova_from_sums(sizes, [1.0] * 3, 9.0, reg, rs)


# ---- d. the ordered sum: its bound, and its teeth --------------------------------------------------------------------------------
def test_the_ordered_sum_lies_within_its_bound_of_the_exact_sum():
    C, TR, B, _ = ar.constants()
    n = TR + 3
    lab = ar.label_rows(31, n, 3, 4)
    for kind in ("int", "real"):
        A = ar.matrix(kind, n, 32)
        got = ar.ordered_class_sums(A, lab, 3, C)
        for r in range(4):
            for c, (s, a, k) in enumerate(ar.exact_class_sums(A, lab[r], 3)):
                if kind == "int":
                    assert Fraction(float(got[r, c])) == s == ar.class_sums_int(A, lab[r], 3)[c]
                else:
                    assert abs(Fraction(float(got[r, c])) - s) <= Fraction(k, 2 ** 52) * a, (r, c)
    assert got[2, 2] == 0.0 and not np.signbit(got[2, 2])  # the empty class: +0.0


def test_the_reference_has_teeth():
    C, TR, B, _ = ar.constants()
    n = 2 * C + 5  # a panel of the GPU test: ragged in the chunk and in the row tile, three chunks
    assert n % C and n % TR
    lab = ar.label_rows(41, n, 3, 5)
    for kind in ("real", "int"):
        A = ar.matrix(kind, n, 42)
        right = ar.ordered_class_sums(A, lab, 3, C)
        for fault in ar.FAULTS:
            if kind == "int" and fault in ("chunks_descending", "swap_ij"):
                continue  # (integers below 2^53: every order gives the same sum, as the header says; a class holds (i, j) and (j, i))
            wrong = ar.ordered_class_sums(A, lab, 3, C, fault=fault, tile_rows=TR)
            assert not ar.same_values(wrong, right), (kind, fault)
        # another chunk size: other bits on the real-valued panel
        if kind == "real":
            assert not ar.same_values(ar.ordered_class_sums(A, lab, 3, C // 2), right)
    # the NaN of the "nan" panel reaches the class of its pair in the rows that hold both ends, and nothing else
    A = ar.matrix("nan", n, 42)
    i, j = n // 3, n - 2
    got = ar.ordered_class_sums(A, lab, 3, C)
    for r in range(len(lab)):
        for c in range(3):
            assert np.isnan(got[r, c]) == (lab[r, i] == c and lab[r, j] == c), (r, c)
    assert np.isnan(got).any()


def test_the_scratch_is_bounded_independently_of_R():
    lib = _tpg()._lib.lib
    C, TR, B, MAX = ar.constants()
    assert C % 4 == 0 and TR % 64 == 0 and B >= 1 and MAX >= 256
    a, b = lib.tpg_class_sums_scratch_bytes(5000, 10 ** 4, 6), lib.tpg_class_sums_scratch_bytes(5000, 10 ** 9, 6)
    assert 0 < a == b < 1 << 30
    assert 0 < lib.tpg_class_sums_scratch_bytes(5000, 1, 6) < a
    assert 0 < lib.tpg_class_sums_scratch_bytes(20000, 10 ** 9, 6) < 1 << 30
    for bad in ((0, 1, 1), (10, -1, 1), (10, 1, 0), (10, 1, MAX + 1), (2 ** 20 + 1, 1, 1)):
        assert lib.tpg_class_sums_scratch_bytes(*bad) == -1, bad


# ---- e. the host pieces under the sanitizers ---------------------------------------------------------------------------------------
def test_the_sanitized_host_program(tmp_path):
    exe = ar.build_host_program(str(tmp_path / "amova_san"))
    C, TR, B, MAX = ar.constants()
    rng = np.random.default_rng(8)
    queries, want = [], []
    pop = _design(3)
    pop[np.flatnonzero(pop == 5)[0]] = -1  # one of the nine of population 5 is outside
    n, P = len(pop), len(SIZES)
    for scheme in (0, 1, 2):
        for r in (0, 1, 9, 2 ** 31 - 1):
            queries.append([1, n, P, 3, scheme, 2 ** 40 + 9, r, *pop, *REGION])
            po, go = ar.perm_labels(n, pop, P, REGION, 3, scheme, 2 ** 40 + 9, r)
            want.append([0, *po, *go])
    queries.append([1, n, P, 0, 0, 5, 3, *pop])  # no regions
    want.append([0, *ar.perm_labels(n, pop, P, None, 0, 0, 5, 3)[0]])
    empty = np.where(pop == 6, 0, pop)
    for bad in ([1, n, P, 3, 3, 5, 1, *pop, *REGION], [1, n, P, 3, 0, 5, -1, *pop, *REGION], [1, n, P, 0, 1, 5, 1, *pop],
                [1, n, P, 3, 0, 5, 1, *empty, *REGION], [1, n, P, 3, 0, 5, 1, *pop, 0, 0, 1, 1, 1, 1, 1],
                [1, n, P, 3, 0, 5, 1, *pop, 0, 0, 1, 1, 1, 2, 3], [1, n, P - 1, 3, 0, 5, 1, *pop, *REGION[:-1]]):
        queries.append(bad)
        want.append([1])
    # the finisher: three levels, two levels, zero degrees of freedom, refusals
    for sizes, reg in ((SIZES, REGION), (SIZES, None), ((5, 6, 7), (0, 0, 0)), ((1, 1, 1, 1), (0, 0, 1, 1)), ((3,), None)):
        W, Rg, T = _random_case(rng, sizes, reg)
        G = 0 if reg is None else max(reg) + 1
        q = [2, len(sizes), G, ar.bits(T), *sizes, *[ar.bits(x) for x in W]]
        if G:
            q += [*reg, *[ar.bits(x) for x in Rg]]
        queries.append(q)
        w = ar.from_sums(sizes, W, T, reg, Rg)
        want.append([0, *[ar.bits(x) for key in ("df", "ssd", "msd", "ncoef", "sigma2", "phi") for x in w[key]]])
    queries.append([2, 3, 0, ar.bits(9.0), 3, 0, 2, *[ar.bits(1.0)] * 3])  # an empty population
    want.append([1])
    queries.append([2, 3, 3, ar.bits(9.0), 3, 4, 2, *[ar.bits(1.0)] * 3, 0, 0, 2, *[ar.bits(1.0)] * 3])  # an empty region
    want.append([1])
    # the checks and the label table of the class sums: a ragged last batch, a full one, and every refusal
    for nn, k, R in ((5, 3, 1), (7, 4, B), (3, 2, B + 1)):
        lab = rng.integers(-1, k, size=(R, nn))
        nb = -(-R // B)
        tab = np.full((nb, nn, B), -1, dtype=np.int64)
        for r in range(R):
            tab[r // B, :, r % B] = lab[r]
        queries.append([3, nn, k, R, *lab.ravel()])
        want.append([0, *tab.ravel()])
    queries.append([3, 4, 2, 0])  # R = 0 is fine
    want.append([0])
    for bad in ([3, 4, 2, 1, 0, 1, 2, 0], [3, 4, 2, 1, 0, -2, 1, 0], [3, 4, 0, 1, 0, 0, 0, 0], [3, 4, MAX + 1, 1, 0, 0, 0, 0], [3, 4, 2, -1],
                [3, 0, 2, 0]):
        queries.append(bad)
        want.append([1])
    got = ar.run_host_program(exe, tmp_path / "q.txt", queries)
    for q, g, w in zip(queries, got, want):
        if q[0] == 2 and w[0] == 0:  # doubles: NaN payloads aside
            a, b = np.array([ar.from_bits(x) for x in g[1:]]), np.array([ar.from_bits(x) for x in w[1:]])
            assert g[0] == 0 and ar.same_values(a, b), q[:4]
        else:
            assert g == [int(x) for x in w], q[:8]
