"""Host side of the f2 blocks: f2_block_ranges on hand-made maps, tpg_f4_jackknife (host arithmetic in the library: loading it
needs no GPU) against tests/f2_ref.py by equality of bits, the restatement against itself (float route within the bound of
the exact route on the planted panel), the declarations in the header and the binding, the R shim's registration, and the
jackknife as a stand-alone program under the address and undefined-behaviour sanitizers.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import f2_ref as fr
from tests import rmock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("tpg_f2_params_default", "tpg_f2_blocks", "tpg_f4_jackknife")


# ---- block ranges ---------------------------------------------------------------------------------------------------------
def test_block_ranges_on_hand_made_maps():
    import tidypopgen_amd as tpg

    # a chromosome change starts a block whatever the distance; 0.05 apart starts one, just under does not
    chrom = [1, 1, 1, 1, 2, 2, 2]
    dist = [0.0, 0.02, 0.05, 0.0999, 0.0, 0.01, 0.07]
    lo, hi = tpg.f2_block_ranges(chrom, dist, 0.05)
    assert lo.tolist() == [0, 2, 4, 6] and hi.tolist() == [2, 4, 6, 7] and lo.dtype == np.int64 == hi.dtype
    # a boundary at exactly blgsize, in numbers a double holds exactly: >= starts the block
    lo, hi = tpg.f2_block_ranges(np.ones(5), [0.0, 0.25, 0.5, 0.625, 1.0], 0.5)
    assert lo.tolist() == [0, 2, 4] and hi.tolist() == [2, 4, 5]
    # the distance is measured from the start of the block, not from the previous locus
    lo, _ = tpg.f2_block_ranges(np.ones(6), [0, 0.03, 0.06, 0.09, 0.12, 0.15], 0.1)
    assert lo.tolist() == [0, 4]
    # bp mode: blgsize >= 100 and positions
    lo, hi = tpg.f2_block_ranges(["a", "a", "a", "b"], [100, 2_000_100, 2_000_101, 5], 2_000_000)
    assert lo.tolist() == [0, 1, 3] and hi.tolist() == [1, 3, 4]
    # a single locus, and none
    lo, hi = tpg.f2_block_ranges([7], [0.3], 0.05)
    assert lo.tolist() == [0] and hi.tolist() == [1]
    lo, hi = tpg.f2_block_ranges([], [], 0.05)
    assert len(lo) == 0 == len(hi)
    # the errors
    with pytest.raises(ValueError, match="sorted"):
        tpg.f2_block_ranges([1, 1, 1], [0.0, 0.2, 0.1], 0.05)
    with pytest.raises(ValueError, match="reappears"):
        tpg.f2_block_ranges([1, 2, 1], [0.0, 0.0, 0.1], 0.05)
    with pytest.raises(ValueError):
        tpg.f2_block_ranges([1, 1], [0.0], 0.05)
    with pytest.raises(ValueError):
        tpg.f2_block_ranges([1, 1], [0.0, 0.1], 0.0)
    assert [x.tolist() for x in tpg.f2_block_ranges([1, 2], [0.5, 0.1], 0.05)] == [[0, 1], [1, 2]]  # dist may restart


def test_block_ranges_equal_the_loop_of_the_definition():
    import tidypopgen_amd as tpg

    rng = np.random.default_rng(4)
    for m in (1, 2, 50, 3000):
        chrom = np.sort(rng.integers(1, 6, size=m))
        dist = np.concatenate([np.sort(np.round(rng.uniform(0, 0.5, size=int((chrom == k).sum())), 3)) for k in range(1, 6)])
        for blg in (0.05, 0.001, 10.0):
            got, want = tpg.f2_block_ranges(chrom, dist, blg), fr.block_ranges(chrom, dist, blg)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- jackknife ------------------------------------------------------------------------------------------------------------
def _jack(f2, bl, quads):
    from tidypopgen_amd import _lib

    f2 = np.asfortranarray(f2, dtype=np.float64)
    bl = np.ascontiguousarray(bl, dtype=np.int64)
    q = np.ascontiguousarray(quads, dtype=np.int32).reshape(-1, 4)
    est, se, used = np.zeros(len(q)), np.zeros(len(q)), np.zeros(len(q), dtype=np.int32)
    rc = _lib.lib.tpg_f4_jackknife(f2.ctypes.data, f2.shape[0], f2.shape[2], bl.ctypes.data, q.ctypes.data, len(q), est.ctypes.data,
                                   se.ctypes.data, used.ctypes.data)
    return rc, est, se, used


def _f2_array(seed, G, nb):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 0.3, size=(G, G, nb))
    a = a + np.transpose(a, (1, 0, 2))
    a[np.arange(G), np.arange(G), :] = 0.0
    return np.asfortranarray(a)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def test_jackknife_equals_the_restatement_bit_for_bit():
    G, nb = 5, 23
    f2 = _f2_array(1, G, nb)
    bl = np.random.default_rng(2).integers(1, 2000, size=nb)
    f2[1, 3, 4] = f2[3, 1, 4] = np.nan  # a NaN block: skipped by the quadruples that touch the pair (1, 3)
    bl[7] = 0                            # a block without loci: skipped by everybody
    quads = [(0, 1, 2, 3), (1, 0, 3, 4), (4, 3, 2, 1), (2, 0, 2, 1), (0, 0, 1, 2), (3, 1, 3, 1)]
    rc, est, se, used = _jack(f2, bl, quads)
    assert rc == 0
    for k, q in enumerate(quads):
        e, s, g = fr.f4_jackknife(f2, bl, q)
        assert _same_bits(est[k], e) and _same_bits(se[k], s) and used[k] == g, (q, est[k], e, se[k], s)
    assert used.tolist() == [21, 21, 21, 22, 22, 21]
    assert abs(est[4]) < 1e-16 and se[4] < 1e-16  # f4(A, A; C, D): x + y - y - x per block, a rounding away from 0
    # f3 through a repeated population needs the +0.0 diagonal: f3(C; A, B) = (f2[C,A] + f2[C,B] - f2[A,B]) / 2
    th = 0.5 * (f2[2, 1] + f2[0, 2] - f2[2, 2] - f2[0, 1])
    assert np.array_equal(th, 0.5 * (f2[2, 1] + f2[0, 2] - f2[0, 1]))


def test_jackknife_with_0_1_and_2_blocks():
    G = 4
    f2 = _f2_array(3, G, 6)
    quad = [(0, 1, 2, 3)]
    for usable in (0, 1, 2):
        bl = np.zeros(6, dtype=np.int64)
        bl[:usable] = [150, 70][:usable]
        f2b = f2.copy()
        f2b[0, 2, 3:] = np.nan  # NaN blocks among the empty ones
        rc, est, se, used = _jack(f2b, bl, quad)
        e, s, g = fr.f4_jackknife(f2b, bl, quad[0])
        assert rc == 0 and used[0] == usable == g and _same_bits(est[0], e) and _same_bits(se[0], s)
        if usable == 0:
            assert np.isnan(est[0]) and np.isnan(se[0])
        elif usable == 1:
            assert est[0] == 0.5 * (f2[0, 3, 0] + f2[1, 2, 0] - f2[0, 2, 0] - f2[1, 3, 0]) and np.isnan(se[0])
        else:
            assert np.isfinite(est[0]) and se[0] > 0
    rc, est, se, used = _jack(np.zeros((G, G, 0), order="F"), np.zeros(0, dtype=np.int64), quad)  # nb = 0
    assert rc == 0 and used[0] == 0 and np.isnan(est[0])


def test_jackknife_of_equal_blocks_is_the_textbook_one():
    # with equal block lengths the weighted estimator is the ordinary delete-one jackknife: est = mean, se^2 = var / g
    G, nb = 4, 40
    f2 = _f2_array(9, G, nb)
    rc, est, se, used = _jack(f2, np.full(nb, 500), [(0, 1, 2, 3)])
    th = 0.5 * (f2[0, 3] + f2[1, 2] - f2[0, 2] - f2[1, 3])
    assert rc == 0 and used[0] == nb
    assert abs(est[0] - th.mean()) < 1e-14 and abs(se[0] - th.std(ddof=1) / np.sqrt(nb)) < 1e-14


def test_jackknife_bad_index_and_python_wrappers():
    import tidypopgen_amd as tpg

    f2 = _f2_array(5, 3, 4)
    bl = np.array([10, 20, 30, 40])
    for bad in ((0, 1, 2, 3), (-1, 0, 1, 2), (0, 1, 3, 2)):
        assert _jack(f2, bl, [bad])[0] == 1  # TPG_EINVAL
        with pytest.raises(tpg._lib.TpgError):
            tpg.f4_from_f2_blocks(f2, bl, [bad])
    r = tpg.f4_from_f2_blocks(f2, bl, [(0, 1, 0, 2), (0, 1, 2, 0)])
    e, s, g = fr.f4_jackknife(f2, bl, (0, 1, 0, 2))
    assert _same_bits(r["est"][0], e) and _same_bits(r["se"][0], s) and r["n_blocks"][0] == g == 4
    assert _same_bits(r["z"][0], e / s)
    r3 = tpg.f3_from_f2_blocks(f2, bl, [(0, 1, 2)])
    assert _same_bits(r3["est"][0], r["est"][0]) and _same_bits(r3["se"][0], r["se"][0])
    assert r["est"][1] == -r["est"][0]  # f4(A, B; D, C) = -f4(A, B; C, D)
    with pytest.raises(ValueError):
        tpg.f4_from_f2_blocks(f2, bl[:3], [(0, 1, 0, 2)])
    with pytest.raises(ValueError):
        tpg.f4_from_f2_blocks(f2[:, :2], bl, [(0, 1, 0, 1)])
    assert tpg.F2_CHUNK_LOCI > 1


# ---- the restatement against itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,G", [(13, 1), (13, 3), (65, 17), (200, 3), (65, 65)])
def test_float_route_within_the_bound_of_the_exact_route(n, G):
    m = 400
    codes, gid, pl, planted = fr.panel(11, n, m, G)
    alt2, c = fr.group_tables(codes, gid, G, pl)
    # the planted things are there
    assert (c[planted["untyped"]] == 0).all() and c[planted["group0_missing"], 0] == 0
    assert (c % 2 == 1).any() and (c[planted["c1"]] == 1).any()
    a, b = planted["mono"]
    assert (alt2[a:b] == 0).all()
    a, b = planted["equal_p"]
    assert ((alt2[a:b] == c[a:b]) & (c[a:b].sum(axis=1, keepdims=True) > 0)).all()  # p = 1 / 2 wherever somebody is typed
    if G >= 3 and n >= G + 1:
        assert (c[:, G - 1] == 0).all() and c[:, G - 2].max() == 2
    lo = np.array([0, 0, 5, 5, 30, planted["untyped"], planted["mono"][0], planted["equal_p"][0], 100, 90])
    hi = np.array([m, 0, 6, 9, 47, planted["untyped"] + 1, planted["mono"][1], planted["equal_p"][1], 233, 120])
    for kw in (dict(maxmiss=1.0), dict(maxmiss=1.0, poly_only=3, apply_corr=0), dict(maxmiss=0.34, minmaf=0.07, maxmaf=0.41),
               dict(maxmiss=1.0, poly_only=0, keep=(np.arange(m) % 3 != 0))):
        pr = fr.params(**kw)
        ex, fl = fr.blocks_exact(alt2, c, lo, hi, pr), fr.blocks_float(alt2, c, lo, hi, pr)
        k_ex, p_ex = fr.flags_exact(alt2, c, pr)
        k_fl, p_fl = fr.flags_float(alt2, c, pr)
        assert np.array_equal(k_ex, k_fl) and np.array_equal(p_ex, p_fl)
        assert not p_ex[planted["equal_p"][0]] and not p_ex[planted["mono"][0]] and not k_ex[planted["untyped"]]
        for k in ("cnt", "ap_cnt", "n_kept"):
            assert np.array_equal(ex[k], fl[k]), (kw, k)
        assert fr.max_excess(fl["f2"], ex["f2"], lo, hi) <= 1.0 and fr.max_excess(fl["ap"], ex["ap"], lo, hi) <= 1.0
        d = fl["f2"][np.arange(G), np.arange(G), :]
        assert np.all((d == 0.0) | np.isnan(d)) and not np.signbit(d[d == 0.0]).any()
        if kw == dict(maxmiss=1.0):
            assert (fl["cnt"][:, :, 6] == 0).all() and (fl["cnt"][:, :, 7] == 0).all()  # no polymorphic locus in either block
            assert (fl["ap_cnt"][:, :, 7] > 0).any() and ex["n_kept"][5] == 0 and ex["n_kept"][7] == 5


def test_f2_of_a_hand_made_locus():
    # two groups, one locus: A has 2 diploids with 3 alt of 4, B one diploid with 0 alt of 2
    codes = np.array([[2], [1], [0]], dtype=np.uint8)
    alt2, c = fr.group_tables(codes, np.array([0, 0, 1]), 2)
    assert alt2.tolist() == [[6, 0]] and c.tolist() == [[4, 2]]
    ex = fr.blocks_exact(alt2, c, [0], [1], fr.params())
    from fractions import Fraction as F

    # (3/4 - 0)^2 - (3/4)(1/4)/3 - 0 = 9/16 - 1/16
    assert ex["f2"][0, 1, 0] == F(1, 2) and ex["f2"][0, 0, 0] == 0 and ex["ap"][0, 0, 0] == F(9, 16) and ex["ap"][0, 1, 0] == 0
    fl = fr.blocks_float(alt2, c, [0], [1], fr.params())
    assert fl["f2"][0, 1, 0] == 0.5 and fl["cnt"][0, 1, 0] == 1
    assert fr.blocks_exact(alt2, c, [0], [1], fr.params(apply_corr=0))["f2"][0, 1, 0] == F(9, 16)


# ---- declarations ---------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_functions():
    from tidypopgen_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "tpg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for f in FUNCTIONS:
        assert re.search(r"\bint " + f + r"\s*\(", code), f
        assert f in _lib.SYMBOLS and hasattr(_lib.lib, f) and getattr(_lib.lib, f).argtypes is not None
    assert re.search(r"\bint64_t tpg_f2_chunk_loci\s*\(", code) and "tpg_f2_chunk_loci" in _lib.SYMBOLS
    assert "f2 blocks" in hdr
    # the struct of the binding is the header's, field for field, and the defaults are the reference's
    body = re.search(r"typedef struct tpg_f2_params \{(.*?)\} tpg_f2_params;", code, flags=re.S).group(1)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f[0] for f in _lib.F2Params._fields_]
    pr = _lib.F2Params()
    assert _lib.lib.tpg_f2_params_default(C.byref(pr)) == 0 and _lib.lib.tpg_f2_params_default(None) == 1
    assert (pr.maxmiss, pr.minmaf, pr.maxmaf, pr.minac2, pr.poly_only, pr.apply_corr, pr.keep) == (0.0, 0.0, 0.5, 0, 1, 1, None)
    m = re.search(r"#define TPG_F2_CHUNK_LOCI (\d+)", hdr)
    assert int(m.group(1)) == _lib.lib.tpg_f2_chunk_loci()
    import tidypopgen_amd as tpg

    for f in ("f2_block_ranges", "f2_blocks", "gt_extract_f2", "f4_from_f2_blocks", "f3_from_f2_blocks"):
        assert callable(getattr(tpg, f))


def _table(lib, symbol):
    row = C.cast(C.addressof(rmock.Entry.in_dll(lib, symbol)), C.POINTER(rmock.Entry))
    out, k = {}, 0
    while row[k].name:
        out[row[k].name.decode()] = (row[k].fun, row[k].numArgs)
        k += 1
    return out


def test_shim_registers_the_entry_once(tmp_path):
    for extra in ((), ("-DTPG_RSHIM_STANDALONE",)):
        r = rmock.compile_only(extra)
        assert r.returncode == 0, r.stderr[-4000:]
    lib = rmock.build(tmp_path)  # links against libtpg_hip.so; loading it needs no GPU
    got = _table(lib, "tpg_rshim_entries_f2")
    assert {k: v[1] for k, v in got.items()} == {"_tidypopgen_tpg_f2_blocks": 9}
    assert got["_tidypopgen_tpg_f2_blocks"][0] == C.cast(lib._tidypopgen_tpg_f2_blocks, C.c_void_p).value
    src = open(os.path.join(ROOT, "shim", "tpg_rshim.c")).read()
    tables = set(re.findall(r"const R_CallMethodDef (tpg_rshim_entries\w*)\[\]", src)) - {"tpg_rshim_entries_f2"}
    assert {"tpg_rshim_entries", "tpg_rshim_entries_tajima"} <= tables
    for tab in tables:
        assert not set(got) & set(_table(lib, tab)), tab
    assert "#pragma weak tpg_f2_blocks" in src and "TPG_NEEDS(tpg_f2_blocks)" in src
    ns = open(os.path.join(ROOT, "shim", "tpgshim", "NAMESPACE")).read()
    rsrc = open(os.path.join(ROOT, "shim", "tpgshim", "R", "tpgshim.R")).read()
    assert "export(tpg_f2_blocks)" in ns and "`_tidypopgen_tpg_f2_blocks`" in rsrc


# ---- sanitizers -----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_jackknife_stand_alone_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "f2_jack_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "f2_jack_san.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok f4jack", r.stdout[-2000:] + r.stderr[-4000:]
    # the numbers it prints are the library's and the restatement's
    G, nb = 4, 9
    f2 = np.zeros((G, G, nb), order="F")
    for b in range(nb):
        for i in range(G):
            for j in range(G):
                f2[i, j, b] = 0.0 if i == j else 0.01 * (1 + (i + j) % 3) + 0.001 * ((7 * b + i * j) % 5)
    f2[0, 2, 3] = f2[2, 0, 3] = np.nan
    bl = np.array([100 + 37 * b for b in range(nb)])
    bl[5] = 0
    e, s, g = fr.f4_jackknife(f2, bl, (0, 1, 2, 3))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("f4 ")][0].split()
    assert int(line[3]) == g == 7
    assert np.array([int(line[1], 16), int(line[2], 16)], dtype=np.uint64).view(np.float64).tolist() == [float(e), float(s)]
