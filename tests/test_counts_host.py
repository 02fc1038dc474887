"""CPU: the cases, references and fault models of tests/counts_ref.py can tell a wrong count sweep from a right one.

tests/test_gpu_counts.py holds the count kernels of csrc/loci.hip and the partial counts of csrc/pack.hip to (g == c).sum() on
the case tables of counts_ref.  Here, without a GPU: every case carries the edge it names on the restated launch plan; the two
routes of every reference agree; the kernels restated without a fault give the reference (the accumulate kernel, literally in its
packed fields, on every case and panel of its table, the saturated rows at m = 480 and m = 960 among them: 15 in the 4-bit
fields and 30 in the bytes with nothing to spare); every fault model of counts_ref.FAULTS moves a count on the case CAUGHT_BY names.
"""
import numpy as np
import pytest

from tests import counts_ref as cr


def _ids(cases):
    return ["-".join(str(x) for x in c[:-1]) for c in cases]


# ---------------------------------------------------------------------------------------------------------------------
# every case asserts the edge it names
def _holds(plan, edge, case):
    assert edge, (case, "a case without a named edge")
    for key, want in edge.items():
        assert plan[key] == want, (case, key, plan[key], want)
    print(case, "->", ", ".join(f"{k} = {v}" for k, v in edge.items()))


@pytest.mark.parametrize("case", cr.LOCI_CASES, ids=_ids(cr.LOCI_CASES))
def test_loci_case_carries_its_edge(case):
    n, m, edge = case
    _holds(cr.loci_plan(n, m), edge, (n, m))


@pytest.mark.parametrize("case", cr.T_CASES, ids=_ids(cr.T_CASES))
def test_indiv_case_carries_its_edge(case):
    n, m, edge = case
    _holds(cr.indiv_plan(n, m), edge, (n, m))


@pytest.mark.parametrize("case", cr.ACC_CASES, ids=_ids(cr.ACC_CASES))
def test_accumulate_case_carries_its_edge(case):
    n, m, edge = case
    for cu in cr.CU_COUNTS:
        plan = cr.accumulate_plan(n, m, cu)
        assert plan["tiles"] == 30, (n, m, cu)
        _holds(plan, edge, (n, m, cu))
    if m >= 479:  # the run under a budget: at least three blocks, the last one narrower
        assert -(-m // cr.ACC_BLOCK_LOCI) >= 3 and m % cr.ACC_BLOCK_LOCI != 0


@pytest.mark.parametrize("case", cr.CLASS_CASES, ids=_ids(cr.CLASS_CASES))
def test_class_case_carries_its_edge(case):
    n, m, builder, G, edge = case
    gid, G, ploidy, cls, nclass = cr.class_case(n, builder, G)
    plan = cr.grouped_plan(n, m, nclass)
    plan["empty"] = len(cr.empty_class_tiles(cls, nclass)) > 0
    _holds(plan, edge, (n, m, builder, G))
    assert len(gid) == n and gid.min() >= 0 and gid.max() < G
    if builder == "hap":
        assert nclass == 2 * G and set(np.unique(ploidy)) == {1.0, 2.0}
    if builder == "edge":
        assert set(np.unique(gid)) == {0, 31, 32, 63, 64, G - 1}
    if builder == "last_only":
        assert set(np.unique(gid)) == {G - 1}
    if builder == "singletons":
        assert np.array_equal(np.bincount(gid), np.ones(n))


def test_the_tables_cover_what_they_were_asked_to():
    assert {c[0] for c in cr.LOCI_CASES} == {1, 8, 127, 128, 129, 248, 256, 264, 385, 512, 520, 640, 1025}
    assert {c[1] for c in cr.LOCI_CASES} == {1, 31, 32, 33, 128, 129, 1000}
    assert {cr.loci_plan(n, m)["Q"] for n, m, _ in cr.LOCI_CASES} == {1, 2, 3, 4, 5, 9}
    # one, two and three chunks of 256, full and ragged by 8
    assert {(cr.loci_plan(n, m)["chunks"], cr.loci_plan(n, m)["last_chunk_rows"]) for n, m, _ in cr.LOCI_CASES} >= {
        (1, 8), (1, 248), (1, 256), (2, 8), (2, 256), (3, 8), (3, 128)}
    assert {c[0] for c in cr.T_CASES} == {1, 33, 130, 136, 264} and {c[1] for c in cr.T_CASES} == {1, 127, 128, 129, 511, 513, 1153}
    assert {cr.indiv_plan(n, m)["KG"] for n, m, _ in cr.T_CASES} == {1, 2, 4, 5, 10}
    assert {c[0] for c in cr.ACC_CASES} == {1, 127, 129, 385, 513, 640}
    assert {c[1] for c in cr.ACC_CASES} == {1, 31, 33, 479, 480, 481, 959, 960, 961, 1921}
    assert {c[0] for c in cr.CLASS_CASES} == set(cr.CLASS_NS) and {c[1] for c in cr.CLASS_CASES} == {1, 33, 129, 500}
    assert {c[3] for c in cr.CLASS_CASES if c[2] != "hap"} - {127} == set(cr.CLASS_GS)
    assert {c[3] for c in cr.CLASS_CASES if c[2] == "hap"} == {16, 17, 33}
    assert {c[2] for c in cr.CLASS_CASES} == set(cr.CLASS_BUILDERS)
    plans = [cr.grouped_plan(n, m, cr.class_case(n, b, G)[4]) for n, m, b, G, _ in cr.CLASS_CASES]
    assert {p["Q"] for p in plans} == set(range(1, 11))
    assert {tuple(p["chain"]) for p in plans} == {(1,), (2,), (2, 1), (2, 2), (2, 2, 1)}
    assert max(c[0] for t in (cr.LOCI_CASES, cr.T_CASES, cr.ACC_CASES, cr.CLASS_CASES) for c in t) <= 1160
    assert max(c[1] for t in (cr.LOCI_CASES, cr.T_CASES, cr.ACC_CASES, cr.CLASS_CASES) for c in t) <= 2100


def test_panels_are_what_their_names_say():
    g = cr.rows_alternate(5, 7, 3, 0)
    assert g.flags.f_contiguous and g.dtype == np.uint8 and (g[0::2] == 3).all() and (g[1::2] == 0).all()
    g = cr.cols_alternate(5, 7, 3, 0)
    assert (g[:, 0::2] == 3).all() and (g[:, 1::2] == 0).all()
    g = cr.stripes(40, 70, 16, 32)
    assert g[15, 31] == 0 and g[16, 31] == 1 and g[15, 32] == 1 and g[16, 32] == 2 and g[39, 69] == (2 + 2) % 4
    g = cr.slots(300, 130)
    assert g[5, 5] == 1 and g[133, 5] == 2 and g[261, 5] == 1 and g[5, 6] == 0 and g[0, 128] == 1
    assert np.array_equal(cr.loci_counts(g)[:128, 1:3], [[2, 1]] * 44 + [[1, 1]] * 84)
    freq = np.bincount(cr.control(385, 1921).ravel(), minlength=4) / (385 * 1921)
    assert np.abs(freq - cr.CONTROL_P).max() < 0.01
    for c in range(4):
        assert (cr.const(3, 4, c) == c).all()


# ---------------------------------------------------------------------------------------------------------------------
# the two routes of every reference
SMALL = [(1, 1), (5, 33), (37, 9), (40, 40)]


@pytest.mark.parametrize("n,m", SMALL)
def test_the_two_routes_of_every_reference_agree(n, m):
    for spec in (("control",), ("stripes", 4, 1), ("rows_alternate", 3, 0), ("const", 3)):
        g = cr.panel(n, m, spec)
        assert np.array_equal(cr.loci_counts(g), cr.loci_counts_loop(g))
        assert np.array_equal(cr.indiv_counts(g), cr.indiv_counts_loop(g))
        assert cr.loci_counts(g).sum() == n * m and (cr.indiv_counts(g).sum(axis=1) == m).all()
        for builder, G in (("round_robin", 3), ("blocks", 7), ("last_only", 4), ("singletons", n)):
            gid, G, _ = cr.CLASS_BUILDERS[builder](n, G)
            assert np.array_equal(cr.class_counts(g, gid, G), cr.class_counts_loop(g, gid, G))
            assert np.array_equal(cr.class_missing(g, gid, G), cr.class_missing_loop(g, gid, G))
        gid, G, ploidy = cr.hap(n, 3)
        gh = cr.pseudohaploid(g, ploidy)
        assert not (gh[ploidy == 1.0] == 1).any() and np.array_equal(gh[ploidy == 2.0], g[ploidy == 2.0])
        assert np.array_equal(cr.hap_table(gh, gid, G, ploidy), cr.hap_table_loop(gh, gid, G, ploidy))


# ---------------------------------------------------------------------------------------------------------------------
# the kernels restated without a fault give the reference
@pytest.mark.parametrize("case", cr.ACC_CASES, ids=_ids(cr.ACC_CASES))
def test_accumulate_restated_in_its_packed_fields_equals_the_reference(case):
    n, m, _ = case
    for spec in cr.ACC_PANELS:
        g = cr.panel(n, m, spec)
        assert np.array_equal(cr.indiv_accumulate_model(g), cr.indiv_counts(g)), (n, m, cr.name(spec))


def test_saturated_rows_fill_the_fields_with_nothing_to_spare():
    assert ("rows_alternate", 3, 0) in cr.ACC_PANELS and {(129, 480), (127, 960)} <= {c[:2] for c in cr.ACC_CASES}
    for n, m in ((129, 480), (127, 960)):
        g = cr.panel(n, m, ("rows_alternate", 3, 0))
        got = cr.indiv_accumulate_model(g)
        assert np.array_equal(got, cr.indiv_counts(g))
        assert (got[0::2, 3] == m).all() and (got[1::2, 0] == m).all() and (got[1::2, 1:] == 0).all()
    # one more locus per 2-bit field, one more group per 4-bit field: the carry lands in the rows that must stay 0
    g = cr.panel(129, 480, ("rows_alternate", 3, 0))
    assert not np.array_equal(cr.indiv_accumulate_model(g, loci_per_field2=4)[1::2], cr.indiv_counts(g)[1::2])
    g = cr.panel(127, 960, ("rows_alternate", 3, 0))
    assert not np.array_equal(cr.indiv_accumulate_model(g, groups_per_field4=6)[1::2], cr.indiv_counts(g)[1::2])


@pytest.mark.parametrize("case", cr.LOCI_CASES, ids=_ids(cr.LOCI_CASES))
def test_loci_kernel_and_pack_partials_restated_equal_the_reference(case):
    n, m, _ = case
    for spec in cr.LOCI_PANELS:
        g = cr.panel(n, m, spec)
        assert np.array_equal(cr.loci_kernel_model(g), cr.loci_counts(g)), (n, m, cr.name(spec))
        if n % 8 == 0:
            assert np.array_equal(cr.pack_partials_model(g), cr.loci_counts(g)), (n, m, cr.name(spec))


@pytest.mark.parametrize("case", cr.T_CASES, ids=_ids(cr.T_CASES))
def test_indiv_kernel_restated_equals_the_reference(case):
    n, m, _ = case
    for spec in cr.T_PANELS:
        g = cr.panel(n, m, spec)
        assert np.array_equal(cr.indiv_kernel_model(g), cr.indiv_counts(g)), (n, m, cr.name(spec))


@pytest.mark.parametrize("case", cr.CLASS_CASES, ids=_ids(cr.CLASS_CASES))
def test_grouped_kernel_restated_equals_the_reference(case):
    n, m, builder, G, _ = case
    gid, G, ploidy, cls, nclass = cr.class_case(n, builder, G)
    for spec in (("const", 3), ("control",)):
        g = cr.panel(n, m, spec)
        if ploidy is not None:
            g = cr.pseudohaploid(g, ploidy)
        counts, missing = cr.grouped_kernel_model(g, cls, nclass)
        assert np.array_equal(counts, cr.class_counts(g, cls, nclass)) and np.array_equal(missing, cr.class_missing(g, cls, nclass))
        if spec == ("const", 3):
            assert not counts.any() and np.array_equal(missing, np.ones((m, 1), dtype=np.int64) * np.bincount(cls, minlength=nclass))


# ---------------------------------------------------------------------------------------------------------------------
# every fault model is caught, and by which case: fault -> (shape (and class case), panel)
CAUGHT_BY = {
    "loci_npad_kept": ((1, 1), ("const", 1)),
    "loci_npad_off_n0": ((127, 32), ("const", 1)),
    "loci_remainder_dropped": ((520, 1000), ("const", 1)),
    "indiv_pad_kept": ((33, 1), ("const", 1)),
    "acc_four_loci_per_2bit_field": ((129, 480), ("rows_alternate", 3, 0)),
    "acc_six_groups_per_4bit_field": ((127, 960), ("rows_alternate", 3, 0)),
    "acc_locus_mask_off": ((127, 31), ("const", 0)),
    "acc_piece_counts_its_first_tile_twice": ((129, 961), ("const", 1)),
    "acc_piece_skips_its_first_tile": ((385, 1921), ("rows_alternate", 1, 0)),
    "grouped_class_in_tile_c_mod_32": ((129, 1, "round_robin", 33), ("const", 1)),
    "grouped_last_group_twice": ((513, 500, "round_robin", 96), ("stripes", 64, 32)),
    "grouped_last_group_dropped": ((769, 33, "blocks", 129), ("const", 1)),
    "grouped_second_step_dropped": ((257, 129, "blocks", 64), ("slots",)),
    "grouped_csize_over_padded_count": ((1, 1, "round_robin", 1), ("const", 3)),
    "grouped_hap_interleave_swapped": ((129, 33, "hap", 16), ("const", 1)),
    "pack_field_wraps_at_256": ((256, 1000), ("const", 1)),
    "pack_half_thread_mask_off": ((8, 31), ("const", 1)),
}
TABLES = {"loci": (cr.LOCI_CASES, cr.LOCI_PANELS), "pack": (cr.LOCI_CASES, cr.LOCI_PANELS), "indiv": (cr.T_CASES, cr.T_PANELS),
          "acc": (cr.ACC_CASES, cr.ACC_PANELS), "grouped": (cr.CLASS_CASES, cr.CLASS_PANELS), "hap": (cr.CLASS_CASES, cr.CLASS_PANELS)}


def test_no_fault_is_left_uncaught():
    assert list(CAUGHT_BY) == list(cr.FAULTS)


@pytest.mark.parametrize("fault", list(cr.FAULTS))
def test_every_fault_moves_a_count_on_a_named_case(fault):
    family, run = cr.FAULTS[fault]
    case, spec = CAUGHT_BY[fault]
    cases, panels = TABLES[family]
    assert case in [c[:-1] for c in cases] and spec in panels, (fault, "not a case of the GPU file")
    g = cr.panel(case[0], case[1], spec)
    if family in ("loci", "pack"):
        assert family == "loci" or case[0] % 8 == 0
        got, want = run(g), cr.loci_counts(g)
    elif family in ("indiv", "acc"):
        got, want = run(g), cr.indiv_counts(g)
    else:
        gid, G, ploidy, cls, nclass = cr.class_case(case[0], case[2], case[3])
        if family == "hap":
            g = cr.pseudohaploid(g, ploidy)
            got, want = run(g, gid, G, ploidy), cr.hap_table(g, gid, G, ploidy)
        else:
            counts, missing = run(g, gid, G, ploidy)
            got = np.concatenate([counts, missing[None]])
            want = np.concatenate([cr.class_counts(g, cls, nclass), cr.class_missing(g, cls, nclass)[None]])
    assert got.shape == want.shape
    moved = int(np.count_nonzero(got != want))
    print(f"{fault}: caught by {case} on {cr.name(spec)}, {moved} of {want.size} counts moved")
    assert moved > 0, (fault, case, cr.name(spec))
