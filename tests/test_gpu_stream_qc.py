"""GPU: the streamed QC pass (tpg_stream_qc, include/tpg.h; Stream.qc, qc_report_loci, qc_report_indiv) against the resident
entry points of the same names on a View of the same selection -- bit for bit, counts and p-values alike --, against counts
taken with numpy from the bytes and the exact-arithmetic reference of tests/hwe_ref.py at the tolerance tests/test_gpu_hwe.py
states, and against PLINK's .hwe goldens; every kind of store; under a budget of an eighth of a panel."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import fixtures as fx
from tests import hwe_ref as hr
from tests.test_gpu_hwe import _check, _tables

pytestmark = pytest.mark.gpu

ALL = dict(loci_counts=True, hwe=True, grouped_counts=True, grouped_hwe=True, indiv_counts=True)
KEYS = ("loci_counts", "loci_hwe", "grouped_genotype_counts", "gt_grouped_hwe", "indiv_counts")


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


def _loci_hwe(tpg, v, mid_p):
    out = np.zeros(v.m)
    tpg._lib.check(tpg._lib.lib.tpg_loci_hwe(v.ctx.h, v.h, C.c_int(int(mid_p)), out.ctypes.data))
    return out


def _resident(tpg, X, rows, cols, code, gid, G, mid_p):
    v = tpg.View(X, rows, cols, code256=code)
    return dict(loci_counts=tpg.loci_counts(v), loci_hwe=_loci_hwe(tpg, v, mid_p),
                grouped_genotype_counts=tpg.grouped_genotype_counts(v, gid, G), gt_grouped_hwe=tpg.gt_grouped_hwe(v, gid, G, mid_p=mid_p),
                indiv_counts=tpg.indiv_counts(v))


def _same(s, r, keys=KEYS):
    for k in keys:
        assert s[k].shape == r[k].shape and s[k].dtype == r[k].dtype, k
        assert np.array_equal(s[k], r[k]), k


def _budget_for(tpg, fbm, block_loci, **kw):
    """a budget under which the plan cuts blocks of `block_loci` loci: the plan's bytes per locus in flight are read off the
    report of a run whose budget holds the panel in one block"""
    st = tpg.Stream.from_numpy(fbm, budget_bytes=1 << 40)
    rep = st.qc(**kw)["report"]
    st.close()
    assert rep["blocks"] == 1
    per = rep["planned_bytes"] // fbm.shape[1]
    return per * block_loci + per * 64


def _panel(seed, n, m, G, imputed=False):
    fbm = orc.synth_fbm(seed, n, m, npop=max(G, 2), miss=0.04, imputed_bytes=imputed)
    fbm[:, m // 3] = 3  # a locus nobody is typed at
    fbm[n // 2, :] = 3  # an individual typed nowhere
    rng = np.random.default_rng(seed)
    gid = rng.integers(0, G, size=n).astype(np.int32)
    if G > 1:
        gid[gid == G - 1] = 0  # an empty group
    return fbm, gid, rng


# n not a multiple of 128, m not a multiple of 32; blocks of 256 or 384 loci: at least three, the last one narrower
CASES = [(203, 1100, 3, 256), (1000, 2101, 51, 384), (65, 811, 1, 256), (2500, 1325, 7, 384)]


@pytest.mark.parametrize("n,m,G,bl", CASES)
def test_stream_equals_resident(tpg, n, m, G, bl):
    fbm, gid, rng = _panel(100 * G + n, n, m, G, imputed=True)
    X = tpg.FBM.from_numpy(fbm)
    rows = (rng.permutation(n)[: (2 * n) // 3] + 1).astype(np.int32)
    cols = (rng.permutation(m)[: (3 * m) // 4 + 1] + 1).astype(np.int32)  # scattered, not monotone
    for sel_r, sel_c, code in ((None, None, tpg.CODE_012), (rows, None, tpg.CODE_012), (None, cols, tpg.CODE_012),
                               (rows, cols, tpg.CODE_IMPUTE_PRED), (None, None, tpg.CODE_IMPUTE_PRED)):
        g = gid if sel_r is None else gid[sel_r - 1]
        mm = m if sel_c is None else len(sel_c)
        sub = fbm if sel_c is None else np.asfortranarray(fbm[:, sel_c - 1])
        budget = _budget_for(tpg, sub, bl, ind_row=sel_r, code256=code, groupIds=g, ngroups=G, **ALL)
        st = tpg.Stream.from_numpy(fbm, budget_bytes=budget)
        for mid_p in (True, False):
            s = st.qc(sel_r, sel_c, code256=code, groupIds=g, ngroups=G, mid_p=mid_p, **ALL)
            rep = s["report"]
            print(n, m, G, "blocks", rep["blocks"], "of", rep["block_loci"], "planned", rep["planned_bytes"], "budget", budget)
            assert rep["blocks"] >= 3 and mm % rep["block_loci"] != 0, rep
            assert rep["planned_bytes"] <= budget and rep["sweeps"] == 1
            assert rep["state_bytes"] == 16 * (n if sel_r is None else len(sel_r))
            _same(s, _resident(tpg, X, sel_r, sel_c, code, g, G, mid_p))
        st.close()
    # the imputed bytes count under CODE_IMPUTE_PRED and are missing under CODE_012: the two readings differ
    a = tpg.Stream.from_numpy(fbm).qc(indiv_counts=True)["indiv_counts"]
    b = tpg.Stream.from_numpy(fbm).qc(code256=tpg.CODE_IMPUTE_PRED, indiv_counts=True)["indiv_counts"]
    assert (a.sum(axis=1) == m).all() and (b.sum(axis=1) == m).all() and not np.array_equal(a, b)
    assert a[n // 2].tolist() == [0, 0, 0, m]


def test_against_numpy_counts_and_the_exact_reference(tpg):
    n, m, G = 65, 400, 3
    fbm, gid, _ = _panel(7, n, m, G)
    codes = np.where(fbm < 3, fbm, 3)
    budget = _budget_for(tpg, fbm, 128, groupIds=gid, ngroups=G, **ALL)
    st = tpg.Stream.from_numpy(fbm, budget_bytes=budget)
    for mid_p in (True, False):
        s = st.qc(groupIds=gid, ngroups=G, mid_p=mid_p, **ALL)
        assert s["report"]["blocks"] >= 3
        lc = np.stack([(codes == k).sum(axis=0) for k in range(4)], axis=1).astype(np.int32)
        ic = np.stack([(codes == k).sum(axis=1) for k in range(4)], axis=1).astype(np.int32)
        assert np.array_equal(s["loci_counts"], lc) and np.array_equal(s["indiv_counts"], ic)
        for k in range(3):
            for g in range(G):
                assert np.array_equal(s["grouped_genotype_counts"][k][:, g], (codes[gid == g] == k).sum(axis=0)), (k, g)
        tabs1 = _tables(codes)
        _check(s["loci_hwe"], tabs1, mid_p, len(tabs1) // 1000)
        tabs = _tables(codes, gid, G)
        _check(s["gt_grouped_hwe"].ravel(order="F"), tabs, mid_p, len(tabs) // 1000)
        # an empty group and an untyped locus give the n = 0 value, as the resident entry point documents
        none = 0.5 if mid_p else 1.0
        assert np.all(s["gt_grouped_hwe"][:, G - 1] == none) and np.all(s["gt_grouped_hwe"][m // 3] == none)
        assert s["loci_hwe"][m // 3] == none
    st.close()


@pytest.mark.parametrize("mid_p,name", [(False, "families_hwe.hwe"), (True, "families_hwe_midp.hwe")])
def test_families_against_plink(tpg, mid_p, name):
    rows = hr.read_plink_hwe(os.path.join(fx.GOLDEN, "related", name))
    st = tpg.Stream.open_bed(os.path.join(fx.GOLDEN, "related/families.bed"), 12, 961, budget_bytes=64 << 10)
    s = st.qc(hwe=True, mid_p=mid_p)
    assert s["report"]["blocks"] >= 2, s["report"]
    p = s["loci_hwe"]
    assert p.shape == (961,)
    for k, (snp, tab, want) in enumerate(rows):
        assert abs(p[k] - want) <= 5e-5, (snp, tab, p[k], want)
    X = tpg.FBM.from_numpy(fx.families_fbm())
    assert np.array_equal(tpg.loci_hwe(X, mid_p=mid_p), p)
    st.close()
    # the reports: a Stream and an FBM of the same genotypes give the same numbers
    st = tpg.Stream.open_bed(os.path.join(fx.GOLDEN, "related/families.bed"), 12, 961, budget_bytes=256 << 10)
    gid = (np.arange(12) % 2).astype(np.int32)
    for kw in ({}, dict(groupIds=gid, ngroups=2)):
        a, b = tpg.qc_report_loci(st, mid_p=mid_p, **kw), tpg.qc_report_loci(X, mid_p=mid_p, **kw)
        assert sorted(a) == ["hwe_p", "maf", "missingness"]
        for key in a:
            assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert np.array_equal(a["hwe_p"], tpg.gt_grouped_hwe(tpg.View(X), gid, 2, mid_p=mid_p).min(axis=1) * 2)
    cols = np.arange(5, 300, dtype=np.int32)
    a, b = tpg.qc_report_indiv(st, None, cols), tpg.qc_report_indiv(X, None, cols)
    het = tpg.gt_ind_hetero(tpg.View(X, None, cols))
    assert np.array_equal(a["het_n"], het[0]) and np.array_equal(a["na_n"], het[1])
    assert np.array_equal(a["het_obs"], het[0] / (961.0 - het[1])) and np.array_equal(a["missingness"], het[1] / 295.0)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    st.close()


def _bed_payload(fbm):
    """bytes 0, 1, 2, 3 (missing) of an FBM as a SNP-major PLINK payload: 2 bits per genotype 11, 10, 00, 01, first individual lowest"""
    n, m = fbm.shape
    code = np.array([3, 2, 0, 1], dtype=np.uint8)[fbm.T]  # m x n
    pad = np.zeros((m, (-n) % 4), dtype=np.uint8)
    c = np.concatenate([code, pad], axis=1).reshape(m, -1, 4)
    return np.ascontiguousarray(c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6))


def test_every_kind_of_store(tpg, tmp_path):
    n, m, G = 301, 1500, 5
    fbm, gid, _ = _panel(31, n, m, G)
    assert fbm.max() <= 3
    X = tpg.FBM.from_numpy(fbm)
    want = _resident(tpg, X, None, None, tpg.CODE_012, gid, G, True)
    budget = _budget_for(tpg, fbm, 384, groupIds=gid, ngroups=G, **ALL)
    bk = str(tmp_path / "panel.bk")
    np.ascontiguousarray(fbm.T).tofile(bk)
    bed = str(tmp_path / "panel.bed")
    with open(bed, "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(_bed_payload(fbm).tobytes())
    stores = [tpg.Stream.from_numpy(fbm, budget_bytes=budget),
              tpg.Stream.from_numpy(np.memmap(bk, dtype=np.uint8, mode="r", shape=(n, m), order="F"), budget_bytes=budget),
              tpg.Stream.open_bk(bk, n, m, budget_bytes=budget),
              tpg.Stream.open_bed(bed, n, m, budget_bytes=budget),
              tpg.Stream.from_bed_payload(_bed_payload(fbm), n, m, budget_bytes=0)]
    for st in stores:
        s = st.qc(groupIds=gid, ngroups=G, **ALL)
        _same(s, want)
        st.close()
    # the synthetic store: the panel FBM.synth generates, block by block on the device
    Xs = tpg.FBM.synth(5, n, 6000, npop=G, miss=0.02)
    st = tpg.Stream.synth(5, n, 6000, npop=G, miss=0.02, budget_bytes=512 << 10)
    s = st.qc(groupIds=gid, ngroups=G, **ALL)
    assert s["report"]["blocks"] >= 3
    _same(s, _resident(tpg, Xs, None, None, tpg.CODE_012, gid, G, True))
    with pytest.raises(tpg._lib.TpgError) as e:  # its rule of contiguous columns stands
        st.qc(None, np.array([3, 1, 2], dtype=np.int32), indiv_counts=True)
    assert e.value.code == 3
    st.close()


def test_only_what_is_asked(tpg):
    n, m, G = 130, 900, 4
    fbm, gid, _ = _panel(13, n, m, G)
    st = tpg.Stream.from_numpy(fbm, budget_bytes=_budget_for(tpg, fbm, 256, groupIds=gid, ngroups=G, **ALL))
    everything = st.qc(groupIds=gid, ngroups=G, **ALL)
    for flag, key in zip(ALL, KEYS):
        grouped = flag.startswith("grouped")
        s = st.qc(groupIds=gid if grouped else None, ngroups=G if grouped else 0, **{flag: True})
        assert sorted(s) == sorted([key, "report"])
        assert np.array_equal(s[key], everything[key]), key
        assert s["report"]["state_bytes"] == (16 * n if flag == "indiv_counts" else 0)
    # device memory on the output side: the same bits
    ctx = st.ctx
    lib = tpg._lib.lib
    job = tpg._lib.StreamQcJob()
    job.struct_size = C.sizeof(job)
    code = np.ascontiguousarray(tpg.CODE_012)
    job.code256, job.midp = code.ctypes.data, 1
    d_ic, d_p = ctx.dev_alloc(16 * n), ctx.dev_alloc(8 * m)
    job.indiv_counts, job.hwe_p = d_ic, d_p
    rep = tpg._lib.StreamReport()
    tpg._lib.check(lib.tpg_stream_qc(ctx.h, st.h, C.byref(job), C.byref(rep)))
    ic, p = np.zeros((n, 4), dtype=np.int32), np.zeros(m)
    tpg._lib.check(lib.tpg_dev_to_host(ctx.h, C.c_void_p(ic.ctypes.data), d_ic, C.c_size_t(ic.nbytes)))
    tpg._lib.check(lib.tpg_dev_to_host(ctx.h, C.c_void_p(p.ctypes.data), d_p, C.c_size_t(p.nbytes)))
    ctx.dev_free(d_ic)
    ctx.dev_free(d_p)
    assert np.array_equal(ic, everything["indiv_counts"]) and np.array_equal(p, everything["loci_hwe"])
    assert rep.blocks >= 2  # (the budget was sized for every output: fewer outputs, wider blocks)
    st.close()


def test_errors_leave_the_stream_usable(tpg):
    n, m = 40, 300
    fbm, gid, _ = _panel(3, n, m, 2)
    st = tpg.Stream.from_numpy(fbm)
    lib = tpg._lib.lib
    out = np.zeros((n, 4), dtype=np.int32)
    pg = np.zeros((m, 2), order="F")

    def job(**kw):
        j = tpg._lib.StreamQcJob()
        j.struct_size = C.sizeof(j)
        j.indiv_counts = out.ctypes.data
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def refused(j, code, word):
        assert lib.tpg_stream_qc(st.ctx.h, st.h, C.byref(j), None) == code
        assert word in lib.tpg_last_error().decode(), lib.tpg_last_error()

    refused(job(struct_size=C.sizeof(tpg._lib.StreamQcJob) - 8), 1, "tpg_stream_qc_job")
    refused(job(struct_size=C.sizeof(tpg._lib.StreamJob)), 1, "tpg_stream_qc_job")
    refused(job(indiv_counts=None), 1, "nothing")
    refused(job(grouped_hwe_p=pg.ctypes.data), 1, "groupIds")
    refused(job(grouped_hwe_p=pg.ctypes.data, groupIds0=gid.ctypes.data, ngroups=0), 1, "groupIds")
    refused(job(midp=2), 1, "midp")
    refused(job(midp=-1), 1, "midp")
    bad = gid.copy()
    bad[7] = 2
    refused(job(grouped_hwe_p=pg.ctypes.data, groupIds0=bad.ctypes.data, ngroups=2), 1, "groupIds[7]")
    cols = np.array([1, m + 1], dtype=np.int32)
    refused(job(colInd1=cols.ctypes.data, m=2), 1, "colInd")
    assert lib.tpg_stream_qc(st.ctx.h, st.h, C.byref(job()), None) == 0
    codes = np.where(fbm < 3, fbm, 3)
    assert np.array_equal(out, np.stack([(codes == k).sum(axis=1) for k in range(4)], axis=1))
    st.close()


def test_an_eighth_of_the_panel(tpg):
    """BASELINE config 2's shape, 1 000 x 650 000, with the HBM budget forced to 1 / 8 of the panel's bytes: planned within the
    budget, the device's memory grows by no more than budget + state (+ the slack of test_stream_config2_under_an_eighth_of_the_
    panel), and every output equals the run without a budget"""
    n, m, G = 1000, 650_000, 51
    X = tpg.FBM.synth(2, n, m, npop=G, miss=0.02)
    fbm = X.to_numpy()
    gid = (np.arange(n) % G).astype(np.int32)
    budget = n * m // 8
    st = tpg.Stream.from_numpy(fbm, budget_bytes=budget)
    s = st.qc(groupIds=gid, ngroups=G, **ALL)
    rep = s["report"]
    print(rep)
    assert rep["planned_bytes"] <= budget and rep["blocks"] >= 8 and rep["sweeps"] == 1
    assert rep["state_bytes"] == 16 * n
    assert rep["peak_device_bytes"] <= budget + rep["state_bytes"] + (64 << 20), rep
    st.close()
    free = tpg.Stream.from_numpy(fbm)
    f = free.qc(groupIds=gid, ngroups=G, **ALL)
    assert f["report"]["budget_bytes"] == 0 and f["report"]["blocks"] < rep["blocks"]
    _same(s, f)
    free.close()
    v = tpg.View(X)
    assert np.array_equal(s["indiv_counts"], tpg.indiv_counts(v)) and np.array_equal(s["loci_counts"], tpg.loci_counts(v))
    assert np.array_equal(s["loci_hwe"], _loci_hwe(tpg, v, True))
