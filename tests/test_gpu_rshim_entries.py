"""GPU: every `.Call` entry point of shim/tpg_rshim.c against the CPU oracle, in R's layout (column-major, 1-based indices,
outputs shaped as the reference allocates them), through tests/rmock with GC torture on and the arguments checked for
writes.  What is pinned: the output types, dims, names and colnames; bit-for-bit values where the Python suite asserts
them for the same kernels; NA_real_ against NaN element by element; integer and double index vectors giving identical
results; the R errors of bad input.  The panels carry the edges where R-side indexing and the kernels' tails go wrong:
1 x 1, 7 x 6, one past the row and locus tiles (65 x 129), 300 x 2051, a locus missing for everybody, a monomorphic
locus, an individual with every genotype missing, imputed bytes 4..6."""
import math

import numpy as np
import pytest

from oracle import oracle as orc
from tests import fixtures as fx
from tests import rmock

pytestmark = pytest.mark.gpu

REALSXP, INTSXP, VECSXP = 14, 13, 19


@pytest.fixture(scope="module")
def r(tmp_path_factory):
    lib = rmock.build(tmp_path_factory.mktemp("rshim_entries"))
    lib.rmock_gctorture(1)
    lib.rmock_strict(1)
    yield rmock.Session(lib)
    lib.rmock_gctorture(0)
    lib.rmock_strict(0)
    lib.R_unload_tpgshim(None)
    lib.rmock_reset()


def _panel(n, m, seed, imputed=False):
    """a synthetic panel with the edges: locus 0 missing for everybody, locus 1 monomorphic, the last individual missing
    everywhere; imputed: some genotypes as the imputed bytes 4..6 of CODE_IMPUTE_PRED"""
    fbm = orc.synth_fbm(seed, n, m, npop=3, miss=0.08).copy(order="F")
    if m > 2:
        fbm[:, 0] = 3
        fbm[:, 1] = 2
    if n > 2:
        fbm[n - 1, :] = 3
    if imputed:
        rng = np.random.default_rng(seed)
        hit = (fbm < 3) & (rng.random(fbm.shape) < 0.2)
        fbm[hit] += 4
    return fbm


PANELS = {  # name: (n, m, code table, imputed bytes)
    "1x1": (1, 1, orc.CODE_012, False),
    "7x6": (7, 6, orc.CODE_012, False),
    "65x129": (65, 129, orc.CODE_IMPUTE_PRED, True),
    "300x2051": (300, 2051, orc.CODE_012, False),
}


@pytest.fixture(scope="module")
def panels(r, tmp_path_factory):
    d = tmp_path_factory.mktemp("panels")
    out = {}
    for k, (name, (n, m, code, imp)) in enumerate(PANELS.items()):
        if name == "7x6":  # the reference's own Fst test matrix (test_pairwise_pop_fst.R), NA as byte 3
            fbm = np.where(np.isnan(fx.FST_7x6), 3, np.nan_to_num(fx.FST_7x6)).astype(np.uint8, order="F")
        else:
            fbm = _panel(n, m, 61 + k, imp)
        bk = d / f"{name}.bk"
        np.asfortranarray(fbm).T.tofile(bk)
        out[name] = (fbm, r.fbm(bk, n, m, code), code)
    return out


def _same(got, want):
    """bit for bit, and NA_real_ where the oracle has NA_real_, a plain NaN where it has one"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=True), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5]
    if got.dtype == np.float64:
        assert np.array_equal(rmock.nan_class(got), rmock.nan_class(want)), "NA_real_ / NaN differ"


def _index_sets(n, m, seed):
    rng = np.random.default_rng(seed)
    rows_all, cols_all = np.arange(1, n + 1), np.arange(1, m + 1)
    sets = {"all": (rows_all, cols_all),
            "perm_rows_desc_cols": (rng.permutation(n)[: max(1, n - n // 3)] + 1, cols_all[::-1].copy()),
            "scattered": (rows_all, cols_all[::7].copy()),
            "one_col": (rng.permutation(n) + 1, np.array([m]))}
    return {k: (np.asarray(a, np.int32), np.asarray(b, np.int32)) for k, (a, b) in sets.items()}


def _groups(n, G, seed):
    """0-based group ids over n individuals; with G > 1 the last group has no member"""
    gid = (np.random.default_rng(seed).integers(0, max(1, G - 1), size=n) if G > 1 else np.zeros(n)).astype(np.int32)
    return gid


def _ploidy(n, seed, pseudo):
    p = np.full(n, 2.0)
    if pseudo:
        p[np.random.default_rng(seed).random(n) < 0.1] = 1.0
    return p


def _m(out, r, shape):
    return r.as_numpy(out, shape)


def _list(r, out, names, shape):
    assert r.lib.TYPEOF(out) == VECSXP and r.names(out) == names, r.names(out)
    return [r.list_elt(out, k, shape) for k in range(len(names))]


# ---- the per-locus entry points ----------------------------------------------------------------------------------

@pytest.mark.parametrize("panel", list(PANELS))
@pytest.mark.parametrize("double", [False, True])
def test_per_locus_entry_points_match_the_oracle(r, panels, panel, double):
    fbm, BM, code = panels[panel]
    n, m = fbm.shape
    lg, one = r.lib.rmock_lgl, r.int([1])
    for key, (rows, cols) in _index_sets(n, m, 3).items():
        nr, mc = len(rows), len(cols)
        ri, ci = r.index(rows, double), r.index(cols, double)
        for G, pseudo in ((1, False), (2, True), (51, False)):
            gid = _groups(nr, G, G + mc)
            pl = _ploidy(nr, G, pseudo)
            gi, ng = r.index(gid, double), r.index([G], double)
            for counts in (0, 1):
                out = r.call("grouped_alt_freq_dip_pseudo_cpp", BM, ri, ci, gi, ng, r.real(pl), one, lg(counts))
                assert r.lib.TYPEOF(out) == REALSXP and r.dim(out) == (mc, 2 * G)
                _same(_m(out, r, (mc, 2 * G)),
                      orc.grouped_alt_freq_dip_pseudo_cpp(fbm, rows, cols, gid, G, pl, bool(counts), code256=code))
            out = r.call("grouped_missingness_cpp", BM, ri, ci, gi, ng, one)
            assert r.lib.TYPEOF(out) == REALSXP and r.dim(out) == (mc, G)
            _same(_m(out, r, (mc, G)), orc.grouped_missingness_cpp(fbm, rows, cols, gid, G, code256=code))
            out = r.call("grouped_summaries_dip_pseudo_cpp", BM, ri, ci, gi, ng, r.real(pl), one)
            names = ["freq_alt", "freq_ref", "n", "het_obs"]
            want = orc.grouped_summaries_dip_pseudo_cpp(fbm, rows, cols, gid, G, pl, code256=code)
            for k, got in enumerate(_list(r, out, names, (mc, G))):
                assert r.dim(r.lib.VECTOR_ELT(out, k)) == (mc, G)
                _same(got, want[names[k]])
            out = r.call("gt_grouped_pi_diploid", BM, ri, ci, gi, ng, one)
            want = orc.gt_grouped_pi_diploid(fbm, rows, cols, gid, G, code256=code)
            for k, got in enumerate(_list(r, out, ["pi", "n"], (mc, G))):
                _same(got, want[["pi", "n"][k]])
        pl = _ploidy(nr, 5, key == "scattered")
        for counts in (0, 1):
            out = r.call("alt_freq_dip_pseudo_cpp", BM, ri, ci, r.real(pl), one, lg(counts))
            assert r.lib.TYPEOF(out) == REALSXP and r.dim(out) == (mc, 2)
            assert r.colnames(out) == (["n_alt", "n_valid"] if counts else ["freq", "n_valid"])
            _same(_m(out, r, (mc, 2)), orc.alt_freq_dip_pseudo_cpp(fbm, rows, cols, pl, bool(counts), code256=code))
        out = r.call("gt_ind_hetero", BM, ri, ci, one)
        assert r.lib.TYPEOF(out) == INTSXP and r.dim(out) == (2, nr)
        _same(_m(out, r, (2, nr)), orc.gt_ind_hetero(fbm, rows, cols, code256=code))
        out = r.call("gt_pi_diploid", BM, ri, ci, one)
        assert r.lib.TYPEOF(out) == REALSXP and r.dim(out) is None and r.lib.XLENGTH(out) == mc
        _same(r.as_numpy(out), orc.gt_pi_diploid(fbm, rows, cols, code256=code))
        if panel in ("65x129", "300x2051"):  # the locus missing for everybody: NA_real_, as the reference writes it
            assert rmock.is_na(r.as_numpy(out)).any() == (1 in cols)


def test_double_and_integer_indices_give_identical_bytes(r, panels):
    fbm, BM, code = panels["65x129"]
    rows = np.array([65, 3, 1, 40, 2], np.int32)
    cols = np.array([129, 1, 64, 65, 2, 100], np.int32)
    gid = np.array([0, 1, 1, 0, 1], np.int32)
    pl = np.full(5, 2.0)
    one = r.int([1])
    for double_groups in (False, True):
        outs = []
        for double in (False, True):
            ri, ci = r.index(rows, double), r.index(cols, double)
            gi, ng = r.index(gid, double and double_groups), r.index([2], double and double_groups)
            res = [r.call("grouped_summaries_dip_pseudo_cpp", BM, ri, ci, gi, ng, r.real(pl), one),
                   r.call("gt_ind_hetero", BM, ri, ci, one), r.call("gt_pi_diploid", BM, ri, ci, one)]
            outs.append([r.list_elt(res[0], k).tobytes() for k in range(4)] + [r.as_numpy(x).tobytes() for x in res[1:]])
        assert outs[0] == outs[1]


def test_per_locus_errors(r, panels, tmp_path):
    fbm, BM, code = panels["7x6"]
    one = r.int([1])
    with pytest.raises(RuntimeError, match="out of"):
        r.call("gt_pi_diploid", BM, r.int([1, 2]), r.real([1.0, 7.0]), one)
    with pytest.raises(RuntimeError, match="NA"):
        r.call("gt_pi_diploid", BM, r.real([1.0, np.nan]), r.int([1]), one)
    with pytest.raises(RuntimeError, match="NA"):
        r.call("gt_pi_diploid", BM, r.real([1.0, rmock.na_real()]), r.int([1]), one)
    # a fractional dosage under CODE_DOSAGE is an R error, never numbers
    dosage = np.full(256, np.nan)
    dosage[:3] = [0.0, 1.0, 2.0]
    dosage[7] = 0.5
    f = fbm.copy(order="F")
    f[2, 3] = 7
    bk = tmp_path / "dosage.bk"
    f.T.tofile(bk)
    BMd = r.fbm(bk, 7, 6, dosage)
    with pytest.raises(RuntimeError, match="tidypopgen"):
        r.call("gt_pi_diploid", BMd, r.int(np.arange(1, 8)), r.int(np.arange(1, 7)), one)
    assert r.depth() == 0


# ---- the Fst loops ------------------------------------------------------------------------------------------------

def _fst_inputs(fbm, code, G):
    n, m = fbm.shape
    rows, cols = np.arange(1, n + 1, dtype=np.int32), np.arange(1, m + 1, dtype=np.int32)
    # the panel's own populations (synth_fbm's i % 3), so that the totals are well away from 0; population G has no
    # member: n = 0 and freq NaN at every locus
    gid = (np.arange(n) % min(3, G - 1)).astype(np.int32)
    return orc.grouped_summaries_dip_pseudo_cpp(fbm, rows, cols, gid, G, np.full(n, 2.0), code256=code)


FST = {  # method: (symbol, the matrices after n, in the reference's argument order)
    "hudson": ("pairwise_fst_hudson_loop", ("freq_alt", "freq_ref")),
    "wc84": ("pairwise_fst_wc84_loop", ("freq_alt", "het_obs")),
    "nei87": ("pairwise_fst_nei87_loop", ("het_obs", "freq_alt", "freq_ref")),
}


@pytest.mark.parametrize("panel", ["7x6", "300x2051"])
@pytest.mark.parametrize("method", list(FST))
def test_fst_loops_match_the_oracle(r, panels, panel, method):
    fbm, _, code = panels[panel]
    G = 4
    S = _fst_inputs(fbm, code, G)
    if method == "nei87":  # n with NA_real_ entries (pairwise_fst_nei87_loop.cpp:50-62): one, then both of a pair
        S["n"] = S["n"].copy()
        S["n"][0, 0] = rmock.na_real()
        S["n"][-1, :2] = rmock.na_real()
    m = S["n"].shape[0]
    sym, mats = FST[method]
    pairs = np.array([[3, 1], [1, 2], [2, 4], [1, 3]], dtype=np.int32).T  # a subset, not sorted, one pair with the empty pop
    P = pairs.shape[1]
    ofn = getattr(orc, sym)
    nd = ofn(pairs.astype(float), S["n"], *[S[k] for k in mats], by_locus=True, return_num_dem=True)
    exact = np.zeros(P)
    for c in range(P):
        num, den = nd["Fst_by_locus_num"][:, c], nd["Fst_by_locus_den"][:, c]
        ok = ~(np.isnan(num) | np.isnan(den))
        with np.errstate(invalid="ignore", divide="ignore"):
            exact[c] = np.float64(math.fsum(num[ok])) / np.float64(math.fsum(den[ok]))
    for as_double in (False, True):
        pc = r.matrix(pairs.astype(float)) if as_double else r.int_matrix(pairs)
        for byl in (0, 1):
            for rnd in (0, 1):
                out = r.call(sym, pc, r.matrix(S["n"]), *[r.matrix(S[k]) for k in mats], r.lib.rmock_lgl(byl),
                             r.lib.rmock_lgl(rnd))
                want = ofn(pairs.astype(float), S["n"], *[S[k] for k in mats], by_locus=bool(byl), return_num_dem=bool(rnd))
                names = ["Fst_by_locus_num", "Fst_by_locus_den"] if rnd else ["fst_locus", "fst_tot"]
                assert r.lib.TYPEOF(out) == VECSXP and r.names(out) == names
                for k, nm in enumerate(names):
                    el = r.lib.VECTOR_ELT(out, k)
                    assert r.lib.TYPEOF(el) == REALSXP
                    if nm == "fst_tot":
                        # the per-locus terms are bit-identical (below); the total differs only by the order of a sum of
                        # mixed-sign terms, so it is held to the correctly rounded sum of those terms, as in
                        # tests/test_gpu_oracle_at_scale.py
                        assert r.dim(el) is None
                        got = r.as_numpy(el)
                        assert np.array_equal(np.isnan(got), np.isnan(want[nm]))
                        assert np.allclose(got, exact, rtol=1e-12, atol=0, equal_nan=True), (got, exact)
                        continue
                    shp = want[nm].shape
                    assert r.dim(el) == shp, (nm, byl, rnd, r.dim(el), shp)
                    assert shp == ((m, P) if (byl if nm in ("fst_locus", "Fst_by_locus_num") else rnd) else (0, 0))
                    _same(r.as_numpy(el, shp), want[nm])


def test_fst_loops_single_locus_and_bad_input(r, panels):
    fbm, _, code = panels["7x6"]
    S = _fst_inputs(fbm[:, 2:3].copy(order="F"), code, 2)  # m = 1
    pairs = np.array([[1], [2]], dtype=np.int32)
    out = r.call("pairwise_fst_hudson_loop", r.int_matrix(pairs), r.matrix(S["n"]), r.matrix(S["freq_alt"]),
                 r.matrix(S["freq_ref"]), r.lib.rmock_lgl(1), r.lib.rmock_lgl(0))
    want = orc.pairwise_fst_hudson_loop(pairs, S["n"], S["freq_alt"], S["freq_ref"], by_locus=True)
    _same(r.list_elt(out, 0, (1, 1)), want["fst_locus"])
    # an integer n (Rcpp's NumericMatrix coerces it)
    out = r.call("pairwise_fst_wc84_loop", r.int_matrix(pairs), r.int_matrix(S["n"].astype(np.int32)), r.matrix(S["freq_alt"]),
                 r.matrix(S["het_obs"]), r.lib.rmock_lgl(1), r.lib.rmock_lgl(0))
    _same(r.list_elt(out, 0, (1, 1)),
          orc.pairwise_fst_wc84_loop(pairs, S["n"], S["freq_alt"], S["het_obs"], by_locus=True)["fst_locus"])
    with pytest.raises(RuntimeError, match="freq_ref is not 1 - freq_alt"):
        r.call("pairwise_fst_hudson_loop", r.int_matrix(pairs), r.matrix(S["n"]), r.matrix(S["freq_alt"]),
               r.matrix(S["freq_ref"] + 0.25), r.lib.rmock_lgl(1), r.lib.rmock_lgl(0))
    with pytest.raises(RuntimeError, match="pairwise_combn"):
        r.call("pairwise_fst_hudson_loop", r.int_matrix(np.array([[1], [3]], np.int32)), r.matrix(S["n"]),
               r.matrix(S["freq_alt"]), r.matrix(S["freq_ref"]), r.lib.rmock_lgl(1), r.lib.rmock_lgl(0))
    assert r.depth() == 0


# ---- fbm256_prod_and_rowSumsSq --------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 7, 8, 9, 65])
def test_fbm256_prod_and_rowSumsSq_matches_the_oracle(r, panels, K):
    fbm, BM, code = panels["300x2051"]
    n, m = fbm.shape
    rng = np.random.default_rng(K)
    rows = (rng.permutation(n)[:257] + 1).astype(np.int32)
    cols = np.arange(m, 0, -3, dtype=np.int32)[: 700]
    center, scale = rng.uniform(0.3, 1.7, len(cols)), rng.uniform(0.4, 1.3, len(cols))
    V = rng.standard_normal((len(cols), K))
    XVo, rsso = orc.fbm256_prod_and_rowSumsSq(fbm, rows, cols, center, scale, V, code256=code)
    for double in (False, True):
        out = r.call("fbm256_prod_and_rowSumsSq", BM, r.index(rows, double), r.index(cols, double), r.real(center),
                     r.real(scale), r.matrix(V))
        assert r.lib.TYPEOF(out) == VECSXP and r.lib.XLENGTH(out) == 2 and r.names(out) is None
        XV, rss = r.list_elt(out, 0, (len(rows), K)), r.list_elt(out, 1)
        assert r.dim(r.lib.VECTOR_ELT(out, 0)) == (len(rows), K) and r.dim(r.lib.VECTOR_ELT(out, 1)) is None
        assert np.max(np.abs(XV - XVo)) <= 1e-9 * np.max(np.abs(XVo))
        assert np.allclose(rss, rsso, rtol=1e-10, atol=0)
    with pytest.raises(RuntimeError, match="Incompatibility between dimensions."):
        r.call("fbm256_prod_and_rowSumsSq", BM, r.int(rows), r.int(cols), r.real(center), r.real(scale),
               r.matrix(V[:-1]))
    assert r.depth() == 0


# ---- every row of the registration table ------------------------------------------------------------------------------

def test_every_registered_symbol_runs(r, panels, tmp_path, monkeypatch):
    monkeypatch.setenv("TPG_DEVICES", "1")
    n, m, code = 65, 129, orc.CODE_IMPUTE_PRED
    fbm = orc.synth_fbm(67, n, m, npop=3, miss=0.0).copy(order="F")  # no missing genotype: the PCA refuses them
    fbm[0, :], fbm[1, :] = 0, 2  # every locus polymorphic
    bk = tmp_path / "clean.bk"
    fbm.T.tofile(bk)
    BM = r.fbm(bk, n, m, code)
    rows = np.arange(1, n + 1, dtype=np.int32)
    cols = np.arange(1, m + 1, dtype=np.int32)
    G, one, lg = 3, r.int([1]), r.lib.rmock_lgl
    gid = (np.arange(n) % G).astype(np.int32)
    S = _fst_inputs(fbm, code, G)
    pairs = orc.combn2(G).astype(np.int32)

    def acc():
        p = tmp_path / f"acc{np.random.randint(1 << 30)}.bk"
        np.zeros(n * n).tofile(p)
        return r.fbm(p, n, n)

    sc = lambda: r.matrix(np.zeros((n, 1)))  # noqa: E731
    fst = lambda *k: (r.int_matrix(pairs), r.matrix(S["n"]), *[r.matrix(S[x]) for x in k], lg(1), lg(0))  # noqa: E731
    builders = {
        "alt_freq_dip_pseudo_cpp": lambda: (BM, r.int(rows), r.int(cols), r.real(np.full(n, 2.0)), one, lg(0)),
        "fbm256_prod_and_rowSumsSq": lambda: (BM, r.int(rows), r.int(cols), r.real(np.ones(len(cols))),
                                              r.real(np.ones(len(cols))), r.matrix(np.ones((len(cols), 2)))),
        "grouped_alt_freq_dip_pseudo_cpp": lambda: (BM, r.int(rows), r.int(cols), r.int(gid), r.int([G]),
                                                    r.real(np.full(n, 2.0)), one, lg(0)),
        "grouped_missingness_cpp": lambda: (BM, r.int(rows), r.int(cols), r.int(gid), r.int([G]), one),
        "grouped_summaries_dip_pseudo_cpp": lambda: (BM, r.int(rows), r.int(cols), r.int(gid), r.int([G]),
                                                     r.real(np.full(n, 2.0)), one),
        "gt_grouped_pi_diploid": lambda: (BM, r.int(rows), r.int(cols), r.int(gid), r.int([G]), one),
        "gt_ind_hetero": lambda: (BM, r.int(rows), r.int(cols), one),
        "gt_pi_diploid": lambda: (BM, r.int(rows), r.int(cols), one),
        "pairwise_fst_hudson_loop": lambda: fst("freq_alt", "freq_ref"),
        "pairwise_fst_nei87_loop": lambda: fst("het_obs", "freq_alt", "freq_ref"),
        "pairwise_fst_wc84_loop": lambda: fst("freq_alt", "het_obs"),
        "increment_as_counts": lambda: (acc(), acc(), sc(), sc(), BM, r.int(rows), r.int(cols)),
        "increment_ibs_counts": lambda: (acc(), acc(), sc(), sc(), sc(), BM, r.int(rows), r.int(cols)),
        "increment_king_numerator": lambda: (acc(), acc(), sc(), sc(), sc(), sc(), BM, r.int(rows), r.int(cols)),
        "tpg_flush": lambda: (),
        "tpg_release": lambda: (),
        "tpg_invalidate": lambda: (BM,),
        "tpg_snp_pairwise": lambda: (BM, r.real(rows), r.real(cols), lg(0), r.int([1 | 8])),
        "tpg_grouped_alt_freq": lambda: (BM, r.real(rows), r.real(cols), r.int(gid), r.int([G]), r.real(np.full(n, 2.0)), lg(0)),
        "tpg_pairwise_pop_fst": lambda: (BM, r.real(rows), r.real(cols), r.int(gid), r.int([G]), r.real(np.full(n, 2.0)),
                                         r.int([0]), r.matrix(pairs.astype(float)), lg(1), lg(0)),
        "tpg_pca_partial_svd": lambda: (BM, r.real(rows), r.real(cols), r.int([2])),
    }
    table = rmock.entries(r.lib)
    assert len(table) == 21
    missing = [k for k in table if k.removeprefix("_tidypopgen_") not in builders]
    assert not missing, f"registered symbols without an argument builder: {missing}"
    for name in table:
        short = name.removeprefix("_tidypopgen_")
        args = builders[short]()
        assert table[name][1] == len(args), name
        r.call(short, *args)  # raises on an R error, a stack imbalance, an unprotected object or a modified argument
        assert r.depth() == 0, name
