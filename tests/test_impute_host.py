"""Simple imputation without a GPU: the numpy restatement against hand-worked cases, and the ABI of the new entry points."""
import ctypes as C
import os
import re

import numpy as np

from tests import impute_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the literal matrix of the reference's own test (tests/testthat/test_gt_impute_simple.R:86-121), 3 = NA: row 6 is all missing
LITERAL = np.array([[0, 2, 1, 1, 0], [0, 0, 2, 0, 1], [2, 0, 0, 1, 1], [1, 1, 2, 2, 2], [0, 0, 2, 1, 1], [3, 3, 3, 3, 3]], dtype=np.uint8)


def test_literal_matrix_mode_and_mean0():
    mode = ir.impute_codes(LITERAL, "mode")
    mean0 = ir.impute_codes(LITERAL, "mean0")
    assert mode[5].tolist() == [0, 0, 2, 1, 1]
    assert mean0[5].tolist() == [1, 1, 1, 1, 1]
    for out in (mode, mean0):
        assert np.array_equal(out[:5], LITERAL[:5])
    assert ir.report(LITERAL) == {"imputed": 5, "loci_all_missing": 0}
    store = ir.store_bytes(LITERAL, "mode")
    assert store[5].tolist() == [4, 4, 6, 5, 5]
    assert np.array_equal(ir.decode_imputed(store), mode)


def test_ties_and_half_way_means():
    def fill(col, method):
        return int(ir.impute_codes(np.array(list(col) + [3], dtype=np.uint8)[:, None], method)[-1, 0])

    assert fill((1, 1, 0, 0), "mode") == 0
    assert fill((2, 2, 1, 1), "mode") == 1
    assert fill((2, 0, 2, 0), "mode") == 0
    assert fill((0, 1), "mean0") == 0          # mean exactly 0.5 -> 0 (half to even)
    assert fill((1, 2), "mean0") == 2          # mean exactly 1.5 -> 2
    assert fill((0, 0, 1), "mean0") == 0       # 1/3
    assert fill((0, 1, 1), "mean0") == 1       # 2/3
    assert fill((2, 2, 1, 2), "mean0") == 2    # 1.75
    assert fill((2, 1, 1, 1), "mean0") == 1    # 1.25


def test_all_missing_locus_stays_missing():
    x = np.array([[3, 0], [3, 3], [3, 2]], dtype=np.uint8)
    for method in ir.METHODS:
        out = ir.impute_codes(x, method, seed=5)
        assert out[:, 0].tolist() == [3, 3, 3]
        assert out[1, 1] in (0, 1, 2)
    assert ir.report(x) == {"imputed": 1, "loci_all_missing": 1}


def test_hash_array_form_equals_written_out_arithmetic():
    xs = [0, 1, 2, 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF, 1 << 63]
    assert [int(v) for v in ir.mix64(np.array(xs, dtype=np.uint64))] == [ir.mix64_int(x) for x in xs]
    # one draw by hand: key = M(seed ^ M(j)), h = M(key ^ M(i)), thr = (s << 31) / t
    seed, i, j, c = 77, 3, 4, (5, 3, 2)
    h = ir.mix64_int(ir.mix64_int(seed ^ ir.mix64_int(j)) ^ ir.mix64_int(i))
    thr = ((c[1] + 2 * c[2]) << 31) // sum(c)
    want = int((h >> 32) < thr) + int((h & 0xFFFFFFFF) < thr)
    cc = [np.full(6, v, dtype=np.int64) for v in c]
    assert int(ir.draws(seed, 8, 6, *cc)[i, j]) == want


def test_random_extremes_and_position_keying():
    n, m = 50, 7
    z = [np.full(m, v, dtype=np.int64) for v in (10, 0, 0)]
    assert not ir.draws(1, n, m, *z).any()                       # p = 0: always 0
    t = [np.full(m, v, dtype=np.int64) for v in (0, 0, 10)]
    assert (ir.draws(1, n, m, *t) == 2).all()                    # p = 1: thr = 2^32 exceeds every 32-bit uniform
    h = [np.full(m, v, dtype=np.int64) for v in (3, 4, 3)]
    whole = ir.draws(9, n, m, *h)
    assert np.array_equal(ir.draws(9, 20, 3, *[a[:3] for a in h], row0=10, col0=2), whole[10:30, 2:5])  # a block is a window
    assert not np.array_equal(ir.draws(10, n, m, *h), whole)


def test_library_exports_the_entry_points():
    from tidypopgen_amd import _lib

    for name in ("tpg_fbm_impute_simple", "tpg_view_impute"):
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.lib, name), name


def test_stream_job_layout_matches_the_header():
    """the ctypes struct is compiled against the header: same size, the two new fields last, the previous size what the header calls
    TPG_STREAM_JOB_SIZE_V1"""
    import subprocess
    import tempfile

    from tidypopgen_amd import _lib

    names = [f for f, _ in _lib.StreamJob._fields_]
    assert names[-2:] == ["impute_method", "impute_seed"] and names[-3] == "square_frobenius"
    src = ('#include <stdio.h>\n#include "tpg.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(tpg_stream_job), '
           "(size_t)TPG_STREAM_JOB_SIZE_V1, offsetof(tpg_stream_job, impute_method), offsetof(tpg_stream_job, impute_seed), "
           "sizeof(tpg_impute_report)); return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "s.c"), "w") as f:
            f.write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", exe])
        size, v1, off_m, off_s, rep = (int(x) for x in subprocess.check_output([exe]).split())
    assert size == C.sizeof(_lib.StreamJob)
    assert v1 == _lib.STREAM_JOB_SIZE_V1 == size - 16
    assert off_m == _lib.StreamJob.impute_method.offset == v1
    assert off_s == _lib.StreamJob.impute_seed.offset == v1 + 8
    assert rep == C.sizeof(_lib.ImputeReport) == 16
    # the plain-C example's refused size (sizeof job - 8) is neither of the two accepted ones
    assert size - 8 not in (size, v1)


def test_header_names_the_methods():
    h = open(os.path.join(ROOT, "include", "tpg.h")).read()
    got = dict(re.findall(r"#define (TPG_IMPUTE_[A-Z0-9]+) (\d+)", h))
    assert got == {"TPG_IMPUTE_NONE": "0", "TPG_IMPUTE_MODE": "1", "TPG_IMPUTE_MEAN0": "2", "TPG_IMPUTE_RANDOM": "3"}
    from tidypopgen_amd import api

    assert api.IMPUTE_METHODS == {"mode": 1, "mean0": 2, "random": 3}
