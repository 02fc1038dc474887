"""GPU: the integer count sweeps of csrc/loci.hip (tpg_loci_counts_kernel, tpg_loci_counts_sum_kernel over the partial counts of
tpg_pack_fast_kernel, tpg_indiv_accumulate_kernel, tpg_onehot_kernel + tpg_grouped_counts_kernel<1|2>) on the prescribed panels of
tests/counts_ref.py, at every launch arm.  Every comparison is np.array_equal against (g == c).sum(): no tolerance.  The cases and
the edge each one carries are the tables of counts_ref (asserted on the restated plans, and armed against counts_ref.FAULTS, by
tests/test_counts_host.py); in short:

Per-locus counts (counts_ref.LOCI_CASES), n -> Q blocks of the kernel over L in passes of 4 + remainder, chunks of 256 of the pack:
  1, 127 (Q = 1, npad 127 / 1)  128 (npad 0)  129 (Q = 2, remainder 2)  264 (Q = 3)  385, 512 (Q = 4: one full pass, no remainder,
  npad 127 / 0)  520, 640 (Q = 5 = 4 + 1)  1025 (Q = 9 = 4 + 4 + 1);  pack partials: 8 (one chunk of one half thread)  248 (one
  chunk ragged by 8)  128, 256 (one, half and full: a field of 256)  264 (two, the second of 8 rows)  512 (two full)  520 (three,
  ragged by 8)  640 (three, the last one half: PACK_NSUB's second chunk missing).  m: 1, 31, 32, 33 (one tile, ragged and full, two)
  128, 129, 1000 (KG = 1, 2, 8).  Routes: View(X) (fast pack + partials where n % 8 == 0, else generic pack + kernel over L), both
  members of View.pair (the second packed locus-major), a sorted column subset, all rows through a row index and a row subset
  (generic pack, kernel over L at the same Q).  v.unpack() is compared with the panel beside every count: a wrong count is then
  told from a wrong pack.
Per-individual counts from T (counts_ref.T_CASES), m -> KG: 1, 127, 128 (KG = 1, pad 127 / 1 / 0)  129 (2)  511 (4: one full pass)
  513 (5 = 4 + 1)  1153 (10 = 4 + 4 + 2).  T from the pack (View(X)), from tpg_l2t_kernel (pair[0]) and from tpg_lm2l_kernel +
  tpg_l2t_kernel (pair[1]) at n = 136, 264; at n = 1, 33, 130 the fast pack kernel does not run and all three are packed with T.
Per-individual counts from L, the streamed pass (counts_ref.ACC_CASES), tiles = 30 throughout: m = 1, 31, 33 (one tile of 1 / 31,
  two tiles)  479, 480 (one step of 15 tiles, ragged / full: 15 in the 4-bit fields)  481 (a second step of one tile of one locus)
  959, 960 (one piece of 30 tiles: 30 in the bytes)  961 (two pieces, the second one tile of one locus)  1921 (three pieces);
  n = 1, 127 (three idle waves)  129 (two)  385 (none)  513, 640 (two workgroups along x, three idle waves in the second).  Each in
  one block (a budget that holds the panel: without one the plan cuts about eight blocks and the kernel never meets more than
  256 loci here), under the plan's own cut and, from m = 479 up, under a budget that cuts blocks of 128 loci (>= 3 blocks, the
  last narrower: the atomics add block after block), and against tpg.indiv_counts of a resident view.
Per-class counts (counts_ref.CLASS_CASES): Q = 1 .. 10 through n = 1 / 127, 129, 257, ..., 1153 (Q = 5, 6, 7 and 9, 10: one to
  three groups past a full pass of the loop unrolled by 4); chains <1> (G = 1, 31, 32; hap 16)  <2> (33, 64; hap 17)  <2, 1> (65,
  96; hap 33)  <2, 2> (97, singletons 127)  <2, 2, 1> (129, 160); blocks / last_only / edge / singletons leave whole class tiles of
  a 128-group empty, edge sits on both sides of 31 | 32 and 63 | 64.  const(3) makes valid = class size - missing = 0 everywhere.
"""
import numpy as np
import pytest

from tests import counts_ref as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


def _ids(cases):
    return ["-".join(str(x) for x in c[:-1]) for c in cases]


def _where(got, want):
    """the first differing element, for the message: (index, got, want, how many differ)"""
    if got.shape != want.shape:
        return ("shape", got.shape, want.shape)
    bad = np.argwhere(got != want)
    return None if len(bad) == 0 else (tuple(int(x) for x in bad[0]), got[tuple(bad[0])].item(), want[tuple(bad[0])].item(), len(bad))


def _same(got, want, *what):
    assert got.dtype == want.dtype or np.issubdtype(got.dtype, np.floating), (what, got.dtype)
    assert np.array_equal(got, want), (what, _where(got, want))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cr.LOCI_CASES, ids=_ids(cr.LOCI_CASES))
def test_per_locus_counts(tpg, case):
    n, m, _ = case
    cols = np.delete(np.arange(m), m // 3) if m > 1 else np.arange(m)
    rows = np.delete(np.arange(n), n // 2) if n > 1 else np.arange(n)
    every = np.arange(n)
    for spec in cr.LOCI_PANELS:
        g = cr.panel(n, m, spec)
        X = tpg.FBM.from_numpy(g)
        a, b = tpg.View.pair(X, None, None, tpg.CODE_012, tpg.CODE_IMPUTE_PRED)
        routes = [("view", tpg.View(X), g), ("pair[0]", a, g), ("pair[1]", b, g),
                  ("columns", tpg.View(X, None, (cols + 1).astype(np.int32)), g[:, cols]),
                  ("all rows by index", tpg.View(X, (every + 1).astype(np.int32), None), g),
                  ("rows", tpg.View(X, (rows + 1).astype(np.int32), None), g[rows])]
        for route, v, sub in routes:
            assert (v.n, v.m) == sub.shape
            _same(tpg.loci_counts(v), cr.loci_counts(sub), n, m, cr.name(spec), route, "loci_counts")
            _same(v.unpack(), sub, n, m, cr.name(spec), route, "unpack")
            v.free()
        X.free()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cr.T_CASES, ids=_ids(cr.T_CASES))
def test_per_individual_counts_from_T(tpg, case):
    n, m, _ = case
    every = np.arange(n)
    for spec in cr.T_PANELS:
        g = cr.panel(n, m, spec)
        want = cr.indiv_counts(g)
        X = tpg.FBM.from_numpy(g)
        a, b = tpg.View.pair(X, None, None, tpg.CODE_012, tpg.CODE_IMPUTE_PRED)
        for origin, v in (("the pack", tpg.View(X)), ("l2t", a), ("lm2l + l2t", b),
                          ("the generic pack", tpg.View(X, (every + 1).astype(np.int32), None))):
            _same(tpg.indiv_counts(v), want, n, m, cr.name(spec), origin, "indiv_counts")
            _same(v.unpack(), g, n, m, cr.name(spec), origin, "unpack")
            v.free()
        X.free()


# ---------------------------------------------------------------------------------------------------------------------
_budgets = {}


def _budget(tpg, g):
    """a budget that cuts blocks of counts_ref.ACC_BLOCK_LOCI loci (it depends on the shape alone), once per shape"""
    from tests.test_gpu_stream_qc import _budget_for

    if g.shape not in _budgets:
        _budgets[g.shape] = _budget_for(tpg, g, cr.ACC_BLOCK_LOCI, indiv_counts=True)
    return _budgets[g.shape]


@pytest.mark.parametrize("case", cr.ACC_CASES, ids=_ids(cr.ACC_CASES))
def test_per_individual_counts_from_L_streamed(tpg, case):
    n, m, _ = case
    for spec in cr.ACC_PANELS:
        g = cr.panel(n, m, spec)
        want = cr.indiv_counts(g)
        st = tpg.Stream.from_numpy(g, budget_bytes=1 << 40)  # (a budget that holds the panel: the kernel sees all m loci at once)
        s = st.qc(indiv_counts=True)
        assert s["report"]["blocks"] == 1
        _same(s["indiv_counts"], want, n, m, cr.name(spec), "one block")
        st.close()
        st = tpg.Stream.from_numpy(g)  # no budget: the plan's own handful of blocks
        s = st.qc(indiv_counts=True)
        _same(s["indiv_counts"], want, n, m, cr.name(spec), "blocks of", s["report"]["block_loci"])
        st.close()
        if m >= 479:
            st = tpg.Stream.from_numpy(g, budget_bytes=_budget(tpg, g))
            s = st.qc(indiv_counts=True)
            rep = s["report"]
            assert rep["blocks"] >= 3 and m % rep["block_loci"] != 0, rep
            _same(s["indiv_counts"], want, n, m, cr.name(spec), "blocks of", rep["block_loci"])
            st.close()
        X = tpg.FBM.from_numpy(g)
        v = tpg.View(X)
        _same(tpg.indiv_counts(v), want, n, m, cr.name(spec), "resident")
        v.free()
        X.free()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cr.CLASS_CASES, ids=_ids(cr.CLASS_CASES))
def test_per_class_counts(tpg, case):
    n, m, builder, G, _ = case
    gid, G, ploidy, cls, nclass = cr.class_case(n, builder, G)
    for spec in cr.class_panels(m):
        g = cr.panel(n, m, spec)
        if ploidy is not None:
            g = cr.pseudohaploid(g, ploidy)
        X = tpg.FBM.from_numpy(g)
        v = tpg.View(X)
        if ploidy is not None:  # nclass = 2 G: the class plan 2 g + hap, read back by tpg_group_vals
            got = tpg.grouped_alt_freq_dip_pseudo_cpp(v, gid, G, ploidy, True)
            _same(got, cr.hap_table(g, gid, G, ploidy), n, m, builder, G, cr.name(spec), "alt / valid of 2 G classes")
            if spec == ("const", 3):
                assert not got.any()
        counts = tpg.grouped_genotype_counts(v, gid, G)
        _same(counts, cr.class_counts(g, gid, G), n, m, builder, G, cr.name(spec), "grouped_genotype_counts")
        missing = tpg.grouped_missingness_cpp(v, gid, G)
        _same(missing, cr.class_missing(g, gid, G).astype(float), n, m, builder, G, cr.name(spec), "grouped_missingness")
        if spec == ("const", 3):  # valid = class size - missing turned on itself
            assert not counts.any() and np.array_equal(missing, np.ones((m, 1)) * np.bincount(gid, minlength=G))
        v.free()
        X.free()


# ---------------------------------------------------------------------------------------------------------------------
def test_the_routes_launch_the_kernels_they_name(tpg):
    """the launch log of a context says which arm ran: the three origins of T, the launch chain of the grouped kernel, the pieces
    of the streamed pass in one launch"""
    n, m = 136, 129
    g = cr.panel(n, m, ("control",))
    X = tpg.FBM.from_numpy(g)
    ctx = X.ctx

    def launches(fn):
        ctx.sync(); ctx.prof_reset()
        out = fn()
        ctx.sync()
        return out, {k: c for k, (c, _) in ctx.prof_dump().items()}

    ctx.prof_enable(True)
    try:
        v, log = launches(lambda: tpg.View(X))
        assert log.get("pack") == 1 and "pack2" not in log, log
        _, log = launches(lambda: tpg.indiv_counts(v))
        assert log.get("indiv_counts") == 1 and "l2t" not in log and "lm2l" not in log, log  # T from the pack
        (a, b), log = launches(lambda: tpg.View.pair(X, None, None, tpg.CODE_012, tpg.CODE_IMPUTE_PRED))
        assert log.get("pack2") == 1, log
        _, log = launches(lambda: tpg.indiv_counts(a))
        assert log.get("l2t") == 1 and "lm2l" not in log, log
        _, log = launches(lambda: tpg.indiv_counts(b))
        assert log.get("l2t") == 1 and log.get("lm2l") == 1, log
        for builder, G in (("round_robin", 160), ("edge", 97), ("round_robin", 96), ("blocks", 64), ("last_only", 31)):
            gid = cr.CLASS_BUILDERS[builder](n, G)[0]
            _, log = launches(lambda: tpg.grouped_genotype_counts(v, gid, G))
            assert log.get("onehot") == 1 and log.get("grouped_counts") == len(cr.chain(-(-G // 32))), (G, log)
        gs = cr.panel(129, 1921, ("control",))
        st = tpg.Stream.from_numpy(gs, budget_bytes=1 << 40)
        _, log = launches(lambda: st.qc(indiv_counts=True))
        assert log.get("indiv_accumulate") == 1 and cr.accumulate_plan(129, 1921)["gy"] == 3, log
        st.close()
    finally:
        ctx.prof_enable(False)
    for w in (v, a, b):
        w.free()
    X.free()
