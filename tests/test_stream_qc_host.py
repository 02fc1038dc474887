"""The streamed QC pass without a GPU: the ABI of tpg_stream_qc (the ctypes struct against the compiled header) and the
arithmetic of qc_report_loci / qc_report_indiv on hand-made count tables against values worked out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_qc_job_layout_matches_the_header(tmp_path):
    from tidypopgen_amd import _lib

    names = [f for f, _ in _lib.StreamQcJob._fields_]
    assert names == ["struct_size", "rowInd1", "n", "colInd1", "m", "code256", "groupIds0", "ngroups", "midp", "loci_counts", "hwe_p",
                     "grouped_counts", "grouped_hwe_p", "indiv_counts"]
    offs = ", ".join(f"offsetof(tpg_stream_qc_job, {f})" for f in names)
    fmt = " ".join(["%zu"] * (len(names) + 1))
    src = ('#include <stdio.h>\n#include "tpg.h"\nint main(void) { printf("' + fmt + '\\n", sizeof(tpg_stream_qc_job), ' + offs +
           "); return 0; }\n")
    (tmp_path / "s.c").write_text(src)
    exe = str(tmp_path / "s")
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got[0] == C.sizeof(_lib.StreamQcJob)
    for f, off in zip(names, got[1:]):
        assert off == getattr(_lib.StreamQcJob, f).offset, f
    # the streamed job of tpg_stream_run did not move
    assert C.sizeof(_lib.StreamJob) == _lib.STREAM_JOB_SIZE_V1 + 16


def test_library_exports_the_entry_point():
    from tidypopgen_amd import _lib

    assert "tpg_stream_qc" in _lib.SYMBOLS
    assert hasattr(_lib.lib, "tpg_stream_qc")
    import tidypopgen_amd as tpg

    for name in ("qc_report_loci", "qc_report_indiv", "qc_loci_from_counts", "qc_indiv_from_counts"):
        assert callable(getattr(tpg, name)), name
    assert callable(tpg.Stream.qc)


def test_loci_arithmetic_on_hand_made_counts():
    import tidypopgen_amd as tpg

    #                  n0 n1 n2 nNA      f = (n1 + 2 n2) / (2 typed)
    counts = np.array([[6, 3, 1, 0],   # 5 / 20 = 0.25
                       [1, 2, 5, 2],   # 12 / 16 = 0.75 -> maf 0.25
                       [0, 0, 0, 10],  # nobody typed
                       [4, 0, 4, 2],   # 8 / 16 = 0.5
                       [9, 0, 0, 1]],  # monomorphic
                      dtype=np.int32)
    q = tpg.qc_loci_from_counts(counts)
    assert q["maf"][[0, 1, 3, 4]].tolist() == [0.25, 0.25, 0.5, 0.0]
    assert np.isnan(q["maf"][2])
    assert q["missingness"].tolist() == [0.0, 0.2, 1.0, 0.2, 0.1]


def test_indiv_arithmetic_uses_the_store_width():
    import tidypopgen_amd as tpg

    # three individuals over m = 8 selected loci of a store of 20
    counts = np.array([[4, 3, 1, 0], [2, 2, 0, 4], [0, 0, 0, 8]], dtype=np.int32)
    q = tpg.qc_indiv_from_counts(counts, 20)
    assert q["het_n"].tolist() == [3, 2, 0] and q["na_n"].tolist() == [0, 4, 8]
    assert q["het_n"].dtype == np.int32 and q["na_n"].dtype == np.int32
    assert q["missingness"].tolist() == [0.0, 0.5, 1.0]
    assert q["het_obs"].tolist() == [3 / 20, 2 / 16, 0 / 12]  # ncol(store) - na_n, not m - na_n
    # the whole store selected: the two readings agree
    full = tpg.qc_indiv_from_counts(counts, 8)
    assert full["het_obs"][:2].tolist() == [3 / 8, 2 / 4] and np.isnan(full["het_obs"][2])
