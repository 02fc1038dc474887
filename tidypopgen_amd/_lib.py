"""ctypes binding of libtpg_hip.so (the C ABI declared in include/tpg.h).

There is no CPU fallback: if the shared library has not been built, importing
this module raises; if no HIP device is usable, creating a context raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# TPG_LIB_PATH: another build of the same library (A/B timing of kernel variants inside one GPU job: tools/enc_ab.py)
LIB_PATH = os.environ.get("TPG_LIB_PATH") or os.path.join(_HERE, "libtpg_hip.so")


class TpgError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[tpg error {code}] {msg}")
        self.code = code


def build(force: bool = False) -> str:
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    import subprocess

    csrc = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", csrc, "-j8", "-s"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    return LIB_PATH


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build the HIP extension first "
        "(python -c 'import __graft_entry__ as g; g.build()' or make -C tidypopgen_amd/csrc). "
        "tidypopgen_amd has no CPU fallback."
    )

lib = C.CDLL(LIB_PATH)

# the ctypes spelling of the C types include/tpg.h uses.  Every pointer to a scalar, opaque handle and handle out-parameter is
# a c_void_p: it takes None, an int (a raw device address), a c_void_p, a byref() result and a ctypes array alike.
vp, cstr = C.c_void_p, C.c_char_p
ci, i64, u32, u64, sz, f64 = C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_size_t, C.c_double
P = C.POINTER  # of a struct mirrored below: takes byref(struct) and None
HOST_ALLREDUCE = C.CFUNCTYPE(ci, vp, vp, i64, ci)  # the allreduce callback of tpg_comm_init_host


class StreamJob(C.Structure):
    """tpg_stream_job of include/tpg.h, field for field"""
    _fields_ = [
        ("struct_size", C.c_size_t), ("rowInd1", vp), ("n", C.c_int64), ("colInd1", vp), ("m", C.c_int64),
        ("ibs_type", C.c_int), ("ibs", vp), ("king", vp), ("allele_sharing", vp), ("grm", vp),
        ("code256", vp), ("ploidy", vp), ("groupIds0", vp), ("ngroups", C.c_int), ("as_counts", C.c_int),
        ("alt_freq", vp), ("grouped_alt_freq", vp), ("grouped_missingness", vp), ("loci_counts", vp),
        ("nfst", C.c_int), ("fst_method", C.c_int * 3), ("pairs1", vp), ("P", C.c_int), ("fst_return_num_dem", C.c_int),
        ("fst_tot", vp * 3), ("fst_by_locus", vp * 3), ("fst_by_locus_den", vp * 3),
        ("code256_pca", vp), ("k", C.c_int), ("pca_tol", C.c_double),
        ("d", vp), ("u", vp), ("v", vp), ("center", vp), ("scale", vp), ("square_frobenius", vp),
        ("impute_method", C.c_int), ("impute_seed", C.c_uint64),
    ]


# TPG_STREAM_JOB_SIZE_V1: the struct before impute_method existed (tpg_stream_run accepts that size too)
STREAM_JOB_SIZE_V1 = StreamJob.square_frobenius.offset + C.sizeof(vp)


class StreamQcJob(C.Structure):
    """tpg_stream_qc_job of include/tpg.h, field for field"""
    _fields_ = [
        ("struct_size", C.c_size_t), ("rowInd1", vp), ("n", C.c_int64), ("colInd1", vp), ("m", C.c_int64),
        ("code256", vp), ("groupIds0", vp), ("ngroups", C.c_int), ("midp", C.c_int),
        ("loci_counts", vp), ("hwe_p", vp), ("grouped_counts", vp), ("grouped_hwe_p", vp), ("indiv_counts", vp),
    ]


class ImputeReport(C.Structure):
    """tpg_impute_report of include/tpg.h"""
    _fields_ = [("imputed", C.c_int64), ("loci_all_missing", C.c_int64)]


class LdReport(C.Structure):
    """tpg_ld_report of include/tpg.h"""
    _fields_ = [("links", C.c_int64), ("kept", C.c_int64), ("rounds", C.c_int64), ("finish_loci", C.c_int64),
                ("band_bytes", C.c_int64)]


class LdStatReport(C.Structure):
    """tpg_ldstat_report of include/tpg.h (tpg_ld_stats takes it as the four int64_t it consists of)"""
    _fields_ = [("pairs", C.c_int64), ("pairs_valid", C.c_int64), ("pairs_beyond", C.c_int64), ("band_tiles", C.c_int64)]


class RohParams(C.Structure):
    """tpg_roh_params of include/tpg.h, field for field"""
    _fields_ = [("window_size", C.c_int32), ("threshold", C.c_double), ("min_snp", C.c_int32), ("heterozygosity", C.c_int32),
                ("max_opp_window", C.c_int32), ("max_miss_window", C.c_int32), ("max_gap", C.c_int64),
                ("min_length_bps", C.c_int64), ("min_density", C.c_double), ("max_opp_run", C.c_int32),
                ("max_miss_run", C.c_int32)]


class F2Params(C.Structure):
    """tpg_f2_params of include/tpg.h, field for field"""
    _fields_ = [("maxmiss", C.c_double), ("minmaf", C.c_double), ("maxmaf", C.c_double), ("minac2", C.c_int32),
                ("poly_only", C.c_int32), ("apply_corr", C.c_int32), ("keep", vp)]


class AdmixParams(C.Structure):
    """tpg_admix_params of include/tpg.h, field for field"""
    _fields_ = [("max_iter", C.c_int32), ("tol", C.c_double), ("update_q", C.c_int32), ("update_f", C.c_int32),
                ("seed", C.c_uint64)]


class StreamReport(C.Structure):
    """tpg_stream_report of include/tpg.h"""
    _fields_ = [
        ("blocks", C.c_int64), ("block_loci", C.c_int64), ("sweeps", C.c_int), ("views_kept", C.c_int),
        ("bytes_up", C.c_size_t), ("bytes_down", C.c_size_t), ("budget_bytes", C.c_size_t), ("planned_bytes", C.c_size_t),
        ("state_bytes", C.c_size_t), ("peak_device_bytes", C.c_size_t), ("seconds", C.c_double),
        ("seconds_first_sweep", C.c_double),
    ]


# name ->(restype, argtypes) of every function include/tpg.h declares, in header order (tests/test_abi.py parses the header
# and checks each entry against it).  A new entry point gets its line here; nothing else declares a prototype.
PROTOTYPES = {
    "tpg_last_error": (cstr, []),
    "tpg_version": (cstr, []),
    # ---- context
    "tpg_device_count": (ci, [vp]),
    "tpg_ctx_create": (ci, [ci, vp]),
    "tpg_ctx_destroy": (None, [vp]),
    "tpg_host_bind_near_device": (ci, [ci, vp]),
    "tpg_ctx_set_stream": (ci, [vp, vp]),
    "tpg_ctx_sync": (ci, [vp]),
    "tpg_prof_enable": (ci, [vp, ci]),
    "tpg_prof_reset": (ci, [vp]),
    "tpg_prof_only": (ci, [vp, cstr]),
    "tpg_prof_get": (ci, [vp, cstr, vp, vp]),
    "tpg_prof_dump": (ci, [vp, vp, sz]),
    "tpg_dev_alloc": (ci, [vp, sz, vp]),
    "tpg_dev_free": (None, [vp]),
    "tpg_dev_to_host": (ci, [vp, vp, vp, sz]),
    "tpg_dev_from_host": (ci, [vp, vp, vp, sz]),
    # ---- genotype store
    "tpg_fbm_from_host": (ci, [vp, vp, i64, i64, vp]),
    "tpg_fbm_open_bk": (ci, [vp, cstr, i64, i64, vp]),
    "tpg_fbm_alloc": (ci, [vp, i64, i64, vp]),
    "tpg_fbm_upload_cols": (ci, [vp, vp, vp, i64, i64]),
    "tpg_fbm_synth": (ci, [vp, u64, i64, i64, i64, ci, u32, ci, vp]),
    "tpg_fbm_open_bed": (ci, [vp, cstr, i64, i64, vp]),
    "tpg_fbm_from_bed_host": (ci, [vp, vp, i64, i64, vp]),
    "tpg_fbm_alloc_bed": (ci, [vp, i64, i64, vp]),
    "tpg_fbm_upload_bed_snps": (ci, [vp, vp, vp, i64, i64]),
    "tpg_fbm_to_host": (ci, [vp, vp, vp]),
    "tpg_fbm_free": (None, [vp]),
    # ---- simple imputation
    "tpg_fbm_impute_simple": (ci, [vp, vp, ci, u64, P(ImputeReport)]),
    "tpg_fbm_impute_simple_at": (ci, [vp, vp, i64, ci, u64, P(ImputeReport)]),
    "tpg_view_impute": (ci, [vp, vp, ci, u64, vp, P(ImputeReport)]),
    "tpg_view_create": (ci, [vp, vp, vp, i64, vp, i64, vp, vp]),
    "tpg_view_create_pair": (ci, [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp]),
    "tpg_view_create_from_host": (ci, [vp, vp, i64, i64, vp, i64, vp, i64, vp, vp]),
    "tpg_view_free": (None, [vp]),
    "tpg_view_n": (i64, [vp]),
    "tpg_view_m": (i64, [vp]),
    "tpg_view_unpack": (ci, [vp, vp, vp]),
    # ---- per-locus sweeps
    "tpg_loci_counts": (ci, [vp, vp, vp]),
    "tpg_indiv_counts": (ci, [vp, vp, vp]),
    "tpg_gt_ind_hetero": (ci, [vp, vp, vp]),
    "tpg_gt_pi_diploid": (ci, [vp, vp, vp]),
    "tpg_gt_grouped_pi_diploid": (ci, [vp, vp, vp, ci, vp, vp]),
    "tpg_grouped_genotype_counts": (ci, [vp, vp, vp, ci, vp]),
    # ---- Hardy-Weinberg exact tests
    "tpg_hwe_exact_counts": (ci, [vp, vp, i64, ci, vp]),
    "tpg_loci_hwe": (ci, [vp, vp, ci, vp]),
    "tpg_gt_grouped_hwe": (ci, [vp, vp, vp, ci, ci, vp]),
    # ---- LD clumping
    "tpg_ld_band_links": (ci, [vp, vp, vp, f64, vp, i64, vp]),
    "tpg_ld_clump": (ci, [vp, vp, vp, f64, vp, vp, vp, P(LdReport)]),
    # ---- LD-kNN imputation
    "tpg_ld_top_neighbours": (ci, [vp, vp, vp, ci, f64, ci, vp, vp]),
    "tpg_view_impute_knn": (ci, [vp, vp, vp, ci, ci, f64, ci, vp, P(ImputeReport), vp]),
    "tpg_fbm_impute_knn": (ci, [vp, vp, vp, ci, ci, f64, ci, P(ImputeReport), vp]),
    "tpg_view_impute_errors": (ci, [vp, vp, vp, vp, vp, vp]),
    "tpg_knn_impute_scratch_bytes": (sz, [i64, i64, i64, ci]),
    # ---- LD statistics
    "tpg_ld_stats": (ci, [vp, vp, vp, vp, i64, ci, vp, vp, vp, vp, vp, vp]),
    "tpg_ld_band_r2": (ci, [vp, vp, vp, i64, i64, vp, i64]),
    # ---- runs of homozygosity
    "tpg_roh_chunk_loci": (i64, []),
    "tpg_roh_snp_status": (ci, [vp, vp, vp, vp, P(RohParams), vp, i64]),
    "tpg_roh_detect": (ci, [vp, vp, vp, vp, P(RohParams), vp]),
    "tpg_roh_count": (i64, [vp]),
    "tpg_roh_fetch": (ci, [vp, vp, vp, vp, vp, vp, vp]),
    "tpg_roh_indiv_summary": (ci, [vp, vp, vp, vp]),
    "tpg_roh_locus_counts": (ci, [vp, vp, vp]),
    "tpg_roh_free": (None, [vp]),
    # ---- IBD segments
    "tpg_ibd_chunk_loci": (i64, []),
    "tpg_ibd_genome_length": (ci, [vp, vp, i64, i64, vp]),
    "tpg_ibd_segments": (ci, [vp, vp, vp, vp, ci, i64, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    # ---- Tajima's D
    "tpg_tajimas_d_from_sums": (ci, [i64, i64, f64, vp]),
    "tpg_tajima_chunk_loci": (i64, []),
    "tpg_pop_tajimas_d": (ci, [vp, vp, vp, ci, vp, vp, vp, vp]),
    "tpg_windows_pop_tajimas_d": (ci, [vp, vp, vp, ci, vp, vp, vp, vp, i64, ci, vp, vp, vp, vp]),
    # ---- f2 blocks
    "tpg_f2_params_default": (ci, [P(F2Params)]),
    "tpg_f2_chunk_loci": (i64, []),
    "tpg_f2_blocks": (ci, [vp, vp, vp, ci, vp, P(F2Params), vp, vp, i64, vp, vp, vp, vp, vp]),
    "tpg_f4_jackknife": (ci, [vp, ci, i64, vp, vp, i64, vp, vp, vp]),
    # ---- site frequency spectra
    "tpg_sfs_chunk_loci": (i64, []),
    "tpg_sfs_segments": (i64, [i64, i64]),
    "tpg_sfs_scratch_bytes": (i64, [i64, ci, i64, i64, ci]),
    "tpg_sfs_project_row": (ci, [i64, i64, i64, vp]),
    "tpg_sfs_blocks": (ci, [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp]),
    # ---- admixture
    "tpg_admix_params_default": (ci, [P(AdmixParams)]),
    "tpg_admix_chunk_loci": (i64, []),
    "tpg_admix_em": (ci, [vp, vp, vp, ci, P(AdmixParams), vp, vp, vp, vp, vp, vp, vp, vp]),
    "tpg_admix_loglik": (ci, [vp, vp, ci, vp, vp, vp]),
    # ---- admixture cross-validation
    "tpg_view_holdout": (ci, [vp, vp, ci, ci, u64, vp, vp]),
    "tpg_admix_holdout_sums": (ci, [vp, vp, vp, ci, vp, vp, vp, vp, vp]),
    "tpg_admix_cv_error": (ci, [ci, vp, vp, vp, vp, vp]),
    "tpg_admix_cv": (ci, [vp, vp, vp, ci, P(AdmixParams), ci, u64, vp, vp, vp, vp, vp, vp, vp, vp]),
    # ---- admixture, accelerated
    "tpg_admix_em_squarem": (ci, [vp, vp, vp, ci, P(AdmixParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "tpg_admix_cv_squarem": (ci, [vp, vp, vp, ci, P(AdmixParams), ci, u64, vp, vp, vp, vp, vp, vp, vp, vp]),
    "tpg_admix_squarem_point": (ci, [vp, i64, i64, ci, ci, ci, vp, vp, vp, vp, vp, vp, f64, vp, vp, vp, vp, vp, vp, vp]),
    # ---- sNMF
    "tpg_snmf": (ci, [vp, vp, vp, ci, ci, f64, f64, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "tpg_snmf_step": (ci, [vp, vp, ci, f64, vp, vp, vp, vp, vp]),
    "tpg_nnls_shared": (ci, [vp, ci, vp, vp, i64, vp, vp]),
    "tpg_view_holdout_fraction": (ci, [vp, vp, f64, u64, vp, vp]),
    "tpg_snmf_cross_entropy_sums": (ci, [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]),
    "tpg_pop_global_stats": (ci, [vp, vp, vp, ci, vp, vp, vp]),
    "tpg_pop_basic_stats": (ci, [vp, vp, vp, ci, vp, ci, vp, vp]),
    "tpg_window_stats": (ci, [vp, vp, i64, ci, vp, vp, vp, i64, ci, ci, vp, vp]),
    "tpg_pbs_from_fst": (ci, [vp, vp, i64, ci, vp, ci, vp]),
    "tpg_alt_freq_dip_pseudo": (ci, [vp, vp, vp, ci, vp]),
    "tpg_grouped_alt_freq_dip_pseudo": (ci, [vp, vp, vp, ci, vp, ci, vp]),
    "tpg_grouped_missingness": (ci, [vp, vp, vp, ci, vp]),
    "tpg_grouped_summaries_dip_pseudo": (ci, [vp, vp, vp, ci, vp, vp, vp, vp, vp]),
    # ---- pairwise population Fst
    "tpg_pairwise_pop_fst": (ci, [vp, vp, vp, ci, vp, ci, vp, ci, ci, ci, vp, vp, vp]),
    "tpg_pairwise_pop_fst_sums": (ci, [vp, vp, vp, ci, vp, ci, vp, ci, vp, vp]),
    "tpg_pairwise_fst_loop": (ci, [vp, ci, vp, ci, i64, ci, vp, vp, vp, vp, ci, ci, vp, vp, vp]),
    # ---- windowed pairwise Fst
    "tpg_winfst_chunk_loci": (i64, []),
    "tpg_windows_fst_scratch_bytes": (i64, [i64, ci, ci, i64]),
    "tpg_windows_pairwise_pop_fst": (ci, [vp, vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, i64, ci, vp, vp, vp, vp, vp]),
    # ---- Fst under relabelings
    "tpg_fst_relabel_sums": (ci, [vp, vp, vp, i64, ci, ci, vp, ci, vp, vp, vp]),
    "tpg_fstperm_unit_loci": (i64, []),
    "tpg_fstperm_span_loci": (i64, []),
    "tpg_fst_relabel_scratch_bytes": (i64, [i64, i64, ci, ci]),
    "tpg_fst_perm_labels": (ci, [i64, vp, ci, ci, ci, ci, u64, i64, vp]),
    # ---- pairwise individual matrices
    "tpg_pairwise_buffer_bytes": (sz, [i64]),
    "tpg_pairwise_create": (ci, [vp, i64, vp, vp]),
    "tpg_pairwise_free": (None, [vp]),
    "tpg_pairwise_zero": (ci, [vp, vp]),
    "tpg_pairwise_accumulate": (ci, [vp, vp, vp, i64, i64]),
    "tpg_pairwise_accumulate_products": (ci, [vp, vp, vp, i64, i64, ci]),
    "tpg_pairwise_products": (ci, [vp]),
    "tpg_pairwise_set_as_pad_quirk": (ci, [vp, i64]),
    "tpg_as_pad_quirk_blocks": (i64, [i64, i64]),
    "tpg_pairwise_counts": (ci, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "tpg_pairwise_ibs": (ci, [vp, vp, ci, i64, vp]),
    "tpg_pairwise_king": (ci, [vp, vp, vp]),
    "tpg_pairwise_allele_sharing": (ci, [vp, vp, vp]),
    "tpg_pairwise_grm": (ci, [vp, vp, vp]),
    "tpg_pairwise_epilogues": (ci, [vp, vp, ci, i64, vp, vp, vp, vp]),
    "tpg_block_means": (ci, [vp, vp, i64, vp, ci, ci, vp, vp]),
    "tpg_filter_high_relatedness": (ci, [vp, vp, i64, f64, vp, vp]),
    "tpg_increment_defer": (ci, [vp, ci]),
    "tpg_increment_ibs_counts": (ci, [vp, vp, vp, vp, i64, i64, vp, i64, vp, i64]),
    "tpg_increment_king_numerator": (ci, [vp, vp, vp, vp, i64, i64, vp, i64, vp, i64]),
    "tpg_increment_as_counts": (ci, [vp, vp, vp, vp, i64, i64, vp, i64, vp, i64]),
    "tpg_increment_flush": (ci, [vp]),
    "tpg_resident_drop": (ci, [vp]),
    "tpg_increment_as_note_narrow_block": (ci, [vp, vp, i64]),
    # ---- AMOVA
    "tpg_pairwise_sqdist": (ci, [vp, vp, ci, i64, vp]),
    "tpg_class_sums": (ci, [vp, vp, i64, vp, i64, ci, vp]),
    "tpg_class_sums_scratch_bytes": (i64, [i64, i64, ci]),
    "tpg_classsum_chunk": (i64, []),
    "tpg_classsum_tile_rows": (i64, []),
    "tpg_classsum_batch": (i64, []),
    "tpg_amova_perm_labels": (ci, [i64, vp, ci, vp, ci, ci, u64, i64, vp, vp]),
    "tpg_amova_from_sums": (ci, [ci, vp, vp, ci, vp, vp, f64, vp]),
    "tpg_mantel_sums": (ci, [vp, vp, vp, ci, i64, vp, i64, vp]),
    "tpg_mantel_scratch_bytes": (i64, [i64, i64, ci]),
    "tpg_mantel_lanes": (i64, []),
    "tpg_mantel_pass_rows": (i64, [i64, ci]),
    "tpg_mantel_strides": (i64, [ci]),
    "tpg_offdiag_moments": (ci, [vp, vp, i64, vp]),
    "tpg_offdiag_center": (ci, [vp, vp, i64, f64, vp]),
    "tpg_mantel_perms": (ci, [i64, vp, ci, u64, i64, i64, vp]),
    "tpg_mantel_from_sums": (ci, [i64, f64, f64, f64, f64, f64, vp]),
    "tpg_mantel_partial": (f64, [f64, f64, f64]),
    # ---- SNP-block shards over the GPUs of one node
    "tpg_comm_unique_id": (ci, [vp]),
    "tpg_comm_init_rank": (ci, [vp, ci, ci, vp, vp]),
    "tpg_comm_init_host": (ci, [vp, ci, ci, HOST_ALLREDUCE, vp, vp]),
    "tpg_comm_destroy": (None, [vp]),
    "tpg_comm_transport": (cstr, [vp]),
    "tpg_comm_rank": (ci, [vp]),
    "tpg_comm_size": (ci, [vp]),
    "tpg_shard_loci": (ci, [i64, ci, ci, vp, vp]),
    "tpg_comm_allreduce_f64": (ci, [vp, vp, vp, i64]),
    "tpg_pairwise_buffer_bytes_sharded": (sz, [i64, ci]),
    "tpg_pairwise_create_sharded": (ci, [vp, vp, i64, vp]),
    "tpg_pairwise_reduce": (ci, [vp, vp, vp]),
    "tpg_pairwise_reduce_begin": (ci, [vp, vp, vp]),
    "tpg_pairwise_reduce_end": (ci, [vp, vp, vp]),
    "tpg_pairwise_band": (ci, [vp, vp, vp]),
    "tpg_pairwise_band_of": (ci, [i64, ci, ci, vp, vp]),
    "tpg_pairwise_epilogues_sharded": (ci, [vp, vp, vp, ci, i64, vp, vp, vp, vp]),
    "tpg_pca_partial_svd_sharded": (ci, [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]),
    "tpg_multi_create": (ci, [ci, vp, vp]),
    "tpg_multi_destroy": (None, [vp]),
    "tpg_multi_ndev": (ci, [vp]),
    "tpg_multi_ctx": (vp, [vp, ci]),
    "tpg_multi_comm": (vp, [vp, ci]),
    "tpg_multi_pairwise": (ci, [vp, vp, i64, i64, vp, i64, vp, i64, ci, vp, vp, vp, vp]),
    "tpg_multi_grouped_alt_freq": (ci, [vp, vp, i64, i64, vp, i64, vp, i64, vp, vp, ci, vp, ci, vp]),
    "tpg_multi_pop_fst": (ci, [vp, vp, i64, i64, vp, i64, vp, i64, vp, vp, ci, vp, ci, vp, ci, ci, ci, vp, vp, vp]),
    "tpg_multi_pca_partial_svd": (ci, [vp, vp, i64, i64, vp, i64, vp, i64, vp, ci, vp, vp, vp, vp, vp, vp]),
    # ---- streamed whole analyses
    "tpg_stream_open_host": (ci, [vp, vp, i64, i64, sz, vp]),
    "tpg_stream_open_bk": (ci, [vp, cstr, i64, i64, sz, vp]),
    "tpg_stream_open_bed": (ci, [vp, cstr, i64, i64, sz, vp]),
    "tpg_stream_open_bed_host": (ci, [vp, vp, i64, i64, sz, vp]),
    "tpg_stream_open_synth": (ci, [vp, u64, i64, i64, ci, u32, ci, sz, vp]),
    "tpg_stream_close": (None, [vp]),
    "tpg_stream_run": (ci, [vp, vp, P(StreamJob), P(StreamReport)]),
    "tpg_multi_stream_run": (ci, [vp, vp, P(StreamJob), P(StreamReport)]),
    "tpg_stream_qc": (ci, [vp, vp, P(StreamQcJob), P(StreamReport)]),
    # ---- PCA
    "tpg_pca_center_scale": (ci, [vp, vp, vp, vp]),
    "tpg_pca_gram": (ci, [vp, vp, vp, vp, vp]),
    "tpg_pca_gram_add": (ci, [vp, vp, vp, vp, vp]),
    "tpg_pca_partial_svd": (ci, [vp, vp, ci, vp, vp, vp, vp, vp, vp]),
    "tpg_pca_random_svd": (ci, [vp, vp, ci, f64, vp, vp, vp, vp, vp, vp]),
    "tpg_sym_eig_topk": (ci, [vp, vp, i64, ci, vp, vp]),
    "tpg_pca_loadings": (ci, [vp, vp, vp, vp, vp, vp, ci, vp]),
    "tpg_fbm256_prod_and_rowSumsSq": (ci, [vp, vp, vp, vp, vp, ci, vp, vp]),
    "tpg_square_frobenius": (ci, [vp, vp, vp, vp, vp]),
    "tpg_fbm256_valid_prod": (ci, [vp, vp, vp, ci, vp]),
    # ---- PCA by operator products
    "tpg_pca_zt_prod": (ci, [vp, vp, vp, vp, vp, ci, vp]),
    "tpg_pca_z_prod": (ci, [vp, vp, vp, vp, vp, ci, vp]),
    "tpg_pca_random_svd_op": (ci, [vp, vp, ci, f64, vp, vp, vp, vp, vp, vp, vp]),
    "tpg_pca_op_scratch_bytes": (sz, [i64, i64, ci]),
    "tpg_pca_gram_route_fits": (ci, [vp, i64, ci, vp]),
    # ---- pcadapt
    "tpg_select_tile": (i64, []),
    "tpg_col_median_mad": (ci, [vp, vp, i64, ci, i64, vp, vp, vp]),
    "tpg_pcadapt_zscores": (ci, [vp, vp, vp, ci, vp, vp]),
    "tpg_robust_dist_ogk": (ci, [vp, vp, i64, ci, vp, vp, vp, vp, vp]),
    "tpg_pchisq_log10_upper": (ci, [vp, vp, i64, ci, vp]),
    "tpg_qchisq_median": (ci, [ci, vp]),
    "tpg_pcadapt": (ci, [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]),
    # ---- autoSVD
    "tpg_view_select_loci": (ci, [vp, vp, vp, i64, vp]),
    "tpg_qnorm_upper": (ci, [f64, vp]),
    "tpg_rollmean_weights": (ci, [ci, vp]),
    "tpg_rollmean_segments": (ci, [vp, vp, i64, vp, i64, ci, vp]),
    "tpg_medcouple": (ci, [vp, vp, i64, vp]),
    "tpg_tukey_mc_up": (ci, [vp, vp, i64, f64, vp]),
    "tpg_pca_auto_svd": (ci, [vp, vp, vp, vp, ci, f64, ci, f64, i64, ci, vp]),
    "tpg_autosvd_count": (i64, [vp]),
    "tpg_autosvd_iters": (ci, [vp]),
    "tpg_autosvd_converged": (ci, [vp]),
    "tpg_autosvd_fetch": (ci, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "tpg_autosvd_history": (ci, [vp, ci, vp, vp, vp]),
    "tpg_autosvd_outliers": (ci, [vp, ci, vp, vp]),
    "tpg_autosvd_intervals": (ci, [vp, ci, i64, vp, vp, vp]),
    "tpg_autosvd_free": (None, [vp]),
    # ---- k-means on PCA scores
    "tpg_kmeans_chunk_doubles": (i64, []),
    "tpg_kmeans_start": (ci, [u64, i64, ci, vp]),
    "tpg_kmeans_step": (ci, [vp, vp, i64, ci, ci, vp, vp, vp, vp, vp]),
    "tpg_kmeans_batch": (ci, [vp, vp, i64, ci, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp]),
    "tpg_cluster_wss": (ci, [vp, vp, i64, ci, ci, vp, vp, vp, vp]),
    # ---- Ward clustering on PCA scores
    "tpg_hclust_ward": (ci, [vp, vp, i64, ci, ci, vp, vp, vp]),
    "tpg_hclust_ward_trace": (ci, [vp, vp, i64, ci, ci, vp, vp, vp, vp]),
    "tpg_hclust_cut": (ci, [i64, vp, vp, ci, vp, vp]),
    "tpg_hclust_r_merge": (ci, [i64, vp, vp, vp]),
    # ---- trees from a pairwise matrix
    "tpg_hclust_dist": (ci, [vp, vp, i64, ci, vp, vp, vp]),
    "tpg_hclust_order": (ci, [i64, vp, vp, vp]),
    "tpg_nj": (ci, [vp, vp, i64, vp, vp, vp, vp, vp]),
    "tpg_nj_edges": (ci, [i64, vp, vp, vp, vp, vp, vp, vp]),
    # ---- DAPC
    "tpg_lda": (ci, [vp, i64, ci, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "tpg_dapc_var_contr": (ci, [vp, vp, i64, i64, ci, vp, ci, vp, vp]),
    # ---- OADP projection
    "tpg_oadp_proj": (ci, [vp, vp, vp, i64, ci, vp, vp, vp]),
    "tpg_predict_oadp": (ci, [vp, vp, vp, vp, vp, ci, vp, vp, vp, vp]),
    # ---- least-squares projection
    "tpg_lsq_normal": (ci, [vp, vp, vp, vp, vp, ci, vp, vp, vp]),
    "tpg_lsq_solve": (ci, [vp, vp, vp, vp, i64, ci, vp, vp]),
    "tpg_predict_lsq": (ci, [vp, vp, vp, vp, vp, ci, vp, vp, vp]),
    # ---- PC-Relate
    "tpg_pcrelate_block_loci": (i64, [i64]),
    "tpg_pcrelate_scratch_bytes": (sz, [i64, i64, ci]),
    "tpg_pcrelate_isaf_max_cells": (i64, []),
    "tpg_pcrelate_basis": (ci, [vp, i64, ci, vp]),
    "tpg_pcrelate_coef": (ci, [vp, vp, vp, ci, vp, vp]),
    "tpg_pcrelate_isaf": (ci, [vp, vp, vp, vp, vp, ci, f64, vp, vp]),
    "tpg_pcrelate_gram": (ci, [vp, vp, vp, vp, vp, ci, f64, vp, vp, vp]),
    "tpg_pcrelate": (ci, [vp, vp, vp, ci, f64, vp, vp, vp]),
}

for _name, (_restype, _argtypes) in PROTOTYPES.items():
    if hasattr(lib, _name):  # (a library built before the entry point existed still imports: build() reports what it lacks)
        getattr(lib, _name).restype = _restype
        getattr(lib, _name).argtypes = _argtypes

SYMBOLS = list(PROTOTYPES)


def check(rc: int) -> None:
    if rc != 0:
        raise TpgError(rc, lib.tpg_last_error().decode("utf-8", "replace"))
