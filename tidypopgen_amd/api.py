"""Host-side mirror of tidypopgen's interface for the genotype-matrix hot path.

The reference's host language is R; R is not available in this image, so the
host side above the C ABI is Python, with the reference's function names,
argument meaning and error behaviour (an error is raised where the reference
raises an R error):

    snp_ibs / snp_king / snp_allele_sharing   R/snp_ibs.R:42, R/snp_king.R:32, R/snp_allele_sharing.R:33
    pairwise_grm                              R/pairwise_grm.R:30
    loci_alt_freq / loci_missingness          R/loci_alt_freq.R:328, R/loci_missingness.R:97
    grouped_* kernels                         R/RcppExports.R:16-26
    pairwise_pop_fst                          R/pairwise_pop_fst.R:71
    gt_pca_partialSVD, fbm256_prod_and_rowSumsSq   R/gt_pca_partialSVD.R:67, R/predict_gt_pca.R:248

Index vectors are 1-based (as in R) and matrices come back as Fortran-ordered
numpy arrays (as R stores them).  All arithmetic runs on the GPU through
libtpg_hip.so; nothing here falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np

from . import _lib
from ._lib import check, lib

CODE_012 = np.full(256, np.nan)
CODE_012[:3] = [0.0, 1.0, 2.0]
CODE_IMPUTE_PRED = np.full(256, np.nan)
CODE_IMPUTE_PRED[:3] = [0.0, 1.0, 2.0]
CODE_IMPUTE_PRED[4:7] = [0.0, 1.0, 2.0]

FST_METHODS = {"Hudson": 0, "Nei87": 1, "WC84": 2}
# include/tpg.h: TPG_IMPUTE_* (gt_impute_simple's methods; "mean2" needs fractional dosages: out of scope)
IMPUTE_METHODS = {"mode": 1, "mean0": 2, "random": 3}


def _impute_method(method) -> int:
    if method not in IMPUTE_METHODS:
        raise ValueError(f"impute method must be one of {sorted(IMPUTE_METHODS)}, not {method!r}")
    return IMPUTE_METHODS[method]
# cross-products of the pairwise accumulators (include/tpg.h: TPG_PW_*)
PW_V, PW_D, PW_H, PW_A = 1, 2, 4, 8
PW_FOR_AS, PW_FOR_IBS, PW_FOR_KING, PW_ALL = PW_V | PW_D, PW_V | PW_D | PW_H, PW_V | PW_D | PW_A, 15
PW_DH = 16  # D and H added up in one sum: all snp_ibs needs beside V (include/tpg.h)
PW_FOR_IBS_ALONE = PW_V | PW_DH


def _ptr(x):
    """numpy array -> its data pointer; int -> raw (device) pointer; None -> NULL.
    The caller must keep the array referenced until the C call returns (never pass a temporary)."""
    if x is None:
        return C.c_void_p(None)
    if isinstance(x, (int, np.integer)):
        return C.c_void_p(int(x))
    return C.c_void_p(x.ctypes.data)


def _i32(x):
    return None if x is None else np.ascontiguousarray(x, dtype=np.int32)


def _f64(x):
    return None if x is None else np.ascontiguousarray(x, dtype=np.float64)


class Context:
    """One GPU + one stream (tpg_ctx)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        check(lib.tpg_ctx_create(device, C.byref(h)))
        self.h = h
        self.device = device

    def set_stream(self, hip_stream: Optional[int]):
        check(lib.tpg_ctx_set_stream(self.h, hip_stream))

    def dev_alloc(self, nbytes: int) -> "C.c_void_p":
        """raw device memory for outputs that stay in HBM between two library calls; release with dev_free"""
        p = C.c_void_p()
        check(lib.tpg_dev_alloc(self.h, int(nbytes), C.byref(p)))
        return p

    def dev_free(self, p):
        lib.tpg_dev_free(p)

    def sync(self):
        check(lib.tpg_ctx_sync(self.h))

    def prof_enable(self, on: bool = True):
        check(lib.tpg_prof_enable(self.h, int(on)))

    def prof_reset(self):
        check(lib.tpg_prof_reset(self.h))

    def prof_only(self, names=None):
        """time only these launches (None: all); see include/tpg.h"""
        check(lib.tpg_prof_only(self.h, ",".join(names).encode() if names else None))

    def prof_get(self, prefix: str):
        ms = C.c_double()
        n = C.c_int64()
        check(lib.tpg_prof_get(self.h, prefix.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def prof_dump(self) -> dict:
        buf = C.create_string_buffer(1 << 16)
        check(lib.tpg_prof_dump(self.h, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, n, ms = line.split("\t")
            out[name] = (int(n), float(ms))
        return out

    def close(self):
        if self.h:
            lib.tpg_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx: Optional[Context] = None


def device_count() -> int:
    """HIP devices visible to this process"""
    c = C.c_int()
    check(lib.tpg_device_count(C.byref(c)))
    return c.value


def bind_host_near_device(device: int = 0) -> int:
    """Keep this thread, and the threads started from it afterwards, on the host NUMA node of GPU `device`
    (tpg_host_bind_near_device: what `numactl --cpunodebind` does for a one-process-per-GPU launcher).  Returns the node,
    or -1 when nothing was done (one node, node unknown, too few of this process's CPUs on it)."""
    node = C.c_int(-1)
    check(lib.tpg_host_bind_near_device(device, C.byref(node)))
    return node.value


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class FBM:
    """Genotype bytes resident in HBM (the role bigstatsr's mmapped FBM.code256 plays)."""

    def __init__(self, ctx: Context, handle, nrow: int, ncol: int, code256=None):
        self.ctx, self.h, self.nrow, self.ncol = ctx, handle, nrow, ncol
        self.code256 = CODE_012 if code256 is None else np.asarray(code256, dtype=float)

    @classmethod
    def from_numpy(cls, bytes_2d, ctx: Optional[Context] = None, code256=None) -> "FBM":
        ctx = ctx or default_context()
        a = np.asarray(bytes_2d)
        if a.dtype != np.uint8 or a.ndim != 2:
            raise TypeError("FBM bytes must be a 2-D uint8 array (individuals x loci)")
        a = np.asfortranarray(a)
        h = C.c_void_p()
        check(lib.tpg_fbm_from_host(ctx.h, _ptr(a), a.shape[0], a.shape[1], C.byref(h)))
        return cls(ctx, h, a.shape[0], a.shape[1], code256)

    @classmethod
    def alloc(cls, nrow: int, ncol: int, ctx: Optional[Context] = None, code256=None) -> "FBM":
        """HBM for an FBM whose columns arrive block by block (upload_cols)"""
        ctx = ctx or default_context()
        h = C.c_void_p()
        check(lib.tpg_fbm_alloc(ctx.h, nrow, ncol, C.byref(h)))
        return cls(ctx, h, nrow, ncol, code256)

    def upload_cols(self, host_cols, col0: int, ctx: Optional[Context] = None):
        """columns [col0, col0 + k) <- host bytes (nrow x k, Fortran order, e.g. a slice of a numpy memmap of the .bk);
        pass another Context (another stream) to run the upload beside kernels of this FBM's own context"""
        a = np.asarray(host_cols)
        assert a.dtype == np.uint8 and a.ndim == 2 and a.flags.f_contiguous and a.shape[0] == self.nrow
        check(lib.tpg_fbm_upload_cols((ctx or self.ctx).h, self.h, _ptr(a), col0, a.shape[1]))

    @classmethod
    def open_bk(cls, path: str, nrow: int, ncol: int, ctx: Optional[Context] = None, code256=None) -> "FBM":
        ctx = ctx or default_context()
        h = C.c_void_p()
        check(lib.tpg_fbm_open_bk(ctx.h, path.encode(), nrow, ncol, C.byref(h)))
        return cls(ctx, h, nrow, ncol, code256)

    @classmethod
    def open_bed(cls, path: str, n: int, m: int, ctx: Optional[Context] = None, code256=None) -> "FBM":
        """A PLINK .bed file as the genotype store (n, m = line counts of the .fam / .bim files)"""
        ctx = ctx or default_context()
        h = C.c_void_p()
        check(lib.tpg_fbm_open_bed(ctx.h, path.encode(), n, m, C.byref(h)))
        return cls(ctx, h, n, m, code256)

    @classmethod
    def alloc_bed(cls, n: int, m: int, ctx: Optional[Context] = None, code256=None) -> "FBM":
        """HBM for a .bed store whose SNPs arrive block by block (upload_bed_snps)"""
        ctx = ctx or default_context()
        h = C.c_void_p()
        check(lib.tpg_fbm_alloc_bed(ctx.h, n, m, C.byref(h)))
        return cls(ctx, h, n, m, code256)

    def upload_bed_snps(self, host_bytes, snp0: int, nsnps: int, ctx: Optional[Context] = None):
        """SNPs [snp0, snp0 + nsnps) <- nsnps * ceil(n / 4) payload bytes (e.g. a slice of a numpy memmap of the .bed behind
        its 3-byte magic); another Context (another stream) runs the upload beside kernels of this store's own context"""
        a = np.asarray(host_bytes)
        assert a.dtype == np.uint8 and a.flags.c_contiguous and a.size == nsnps * ((self.nrow + 3) // 4)
        check(lib.tpg_fbm_upload_bed_snps((ctx or self.ctx).h, self.h, _ptr(a), snp0, nsnps))

    @classmethod
    def synth(cls, seed: int, nrow: int, ncol: int, j0: int = 0, npop: int = 51, miss: float = 0.02,
              imputed_bytes: bool = False, ctx: Optional[Context] = None, code256=None) -> "FBM":
        ctx = ctx or default_context()
        thr = min(int(round(miss * 2 ** 32)), 2 ** 32 - 1)
        h = C.c_void_p()
        check(lib.tpg_fbm_synth(ctx.h, seed, nrow, ncol, j0, npop, thr, int(imputed_bytes), C.byref(h)))
        return cls(ctx, h, nrow, ncol, code256)

    def impute_simple(self, method: str = "mode", seed: int = 0) -> dict:
        """gt_impute_simple on the bytes in HBM, in place (tpg_fbm_impute_simple): a missing genotype (byte 3) becomes
        byte 4 + fill, which CODE_IMPUTE_PRED reads and the raw-byte analyses go on treating as missing.  Returns the
        report {"imputed", "loci_all_missing"}.  The FBM's code256 is left as it is (gt_impute_simple below switches it)."""
        rep = _lib.ImputeReport()
        check(lib.tpg_fbm_impute_simple(self.ctx.h, self.h, _impute_method(method), seed, C.byref(rep)))
        return {"imputed": int(rep.imputed), "loci_all_missing": int(rep.loci_all_missing)}

    def to_numpy(self) -> np.ndarray:
        out = np.zeros((self.nrow, self.ncol), dtype=np.uint8, order="F")
        check(lib.tpg_fbm_to_host(self.ctx.h, self.h, _ptr(out)))
        return out

    def free(self):
        if self.h:
            lib.tpg_fbm_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class View:
    """(FBM, rowInd, colInd, code256) packed to 2 bits in HBM (tpg_view)."""

    def __init__(self, X: FBM, ind_row=None, ind_col=None, code256="fbm"):
        self.X = X
        self.ctx = X.ctx
        r, c = _i32(ind_row), _i32(ind_col)
        if isinstance(code256, str):
            code = _f64(X.code256)
        else:
            code = _f64(code256)  # None = raw bytes
        h = C.c_void_p()
        check(lib.tpg_view_create(self.ctx.h, X.h, _ptr(r), 0 if r is None else len(r), _ptr(c),
                                  0 if c is None else len(c), _ptr(code), C.byref(h)))
        self.h = h
        self.n = int(lib.tpg_view_n(h))
        self.m = int(lib.tpg_view_m(h))

    @classmethod
    def pair(cls, X: FBM, ind_row=None, ind_col=None, code256_a=None, code256_b=CODE_IMPUTE_PRED):
        """two views of the same rows / columns through two code tables from one read of the FBM bytes
        (tpg_view_create_pair): by default the raw view of the pairwise statistics and the imputed view of the PCA"""
        r, c = _i32(ind_row), _i32(ind_col)
        ca, cb = _f64(code256_a), _f64(code256_b)
        ha, hb = C.c_void_p(), C.c_void_p()
        check(lib.tpg_view_create_pair(X.ctx.h, X.h, _ptr(r), 0 if r is None else len(r), _ptr(c),
                                       0 if c is None else len(c), _ptr(ca), _ptr(cb), C.byref(ha), C.byref(hb)))
        out = []
        for h in (ha, hb):
            v = cls.__new__(cls)
            v.X, v.ctx, v.h = X, X.ctx, h
            v.n, v.m = int(lib.tpg_view_n(h)), int(lib.tpg_view_m(h))
            out.append(v)
        return out[0], out[1]

    def impute(self, method: str = "mode", seed: int = 0) -> "View":
        """a new view of the same rows / columns with the missing genotypes of this (raw) view filled from the kept rows
        (tpg_view_impute): the only route for a .bed-form store.  The report is left in `.impute_report` of the result."""
        h = C.c_void_p()
        rep = _lib.ImputeReport()
        check(lib.tpg_view_impute(self.ctx.h, self.h, _impute_method(method), seed, C.byref(h), C.byref(rep)))
        v = View.__new__(View)
        v.X, v.ctx, v.h = self.X, self.ctx, h
        v.n, v.m = int(lib.tpg_view_n(h)), int(lib.tpg_view_m(h))
        v.impute_report = {"imputed": int(rep.imputed), "loci_all_missing": int(rep.loci_all_missing)}
        return v

    def holdout(self, folds: int, fold: int, cv_seed: int = 0) -> "View":
        """a new view of the same rows / columns with the typed genotypes of one cross-validation fold set to missing
        (tpg_view_holdout, include/tpg.h "admixture cross-validation"); their number is left in `.n_held` of the result"""
        h = C.c_void_p()
        held = C.c_int64()
        check(lib.tpg_view_holdout(self.ctx.h, self.h, int(folds), int(fold), int(cv_seed) & 0xFFFFFFFFFFFFFFFF, C.byref(h),
                                   C.byref(held)))
        v = View.__new__(View)
        v.X, v.ctx, v.h = self.X, self.ctx, h
        v.n, v.m = int(lib.tpg_view_n(h)), int(lib.tpg_view_m(h))
        v.n_held = int(held.value)
        return v

    def holdout_fraction(self, fraction: float, seed: int = 0) -> "View":
        """a new view of the same rows / columns with a share `fraction` of the typed genotypes set to missing, chosen by the hash of
        (seed, position) (tpg_view_holdout_fraction, include/tpg.h "sNMF"); their number is left in `.n_held` of the result"""
        h = C.c_void_p()
        held = C.c_int64()
        check(lib.tpg_view_holdout_fraction(self.ctx.h, self.h, float(fraction), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(h),
                                            C.byref(held)))
        v = View.__new__(View)
        v.X, v.ctx, v.h = self.X, self.ctx, h
        v.n, v.m = int(lib.tpg_view_n(h)), int(lib.tpg_view_m(h))
        v.n_held = int(held.value)
        return v

    def impute_knn(self, hi, l: int = 10, k: int = 8, min_r2: float = 0.0, _flags: int = 0) -> "View":
        """a new view of the same rows / columns with the missing genotypes of this (raw) view filled by LD-kNN imputation
        (tpg_view_impute_knn, include/tpg.h "LD-kNN imputation"): for a missing genotype at locus j the l loci in strongest LD
        with j inside the window `hi` (ld_window_hi) say which individuals are alike, and the k nearest vote.  The report
        {"imputed", "loci_all_missing", "entries_left", "loci_without_neighbours"} is left in `.impute_report` of the result."""
        hi = _ld_hi(self, hi)
        h = C.c_void_p()
        rep = _lib.ImputeReport()
        extra = (C.c_int64 * 2)()
        check(lib.tpg_view_impute_knn(self.ctx.h, self.h, _ptr(hi), int(l), int(k), float(min_r2), int(_flags), C.byref(h),
                                      C.byref(rep), extra))
        v = View.__new__(View)
        v.X, v.ctx, v.h = self.X, self.ctx, h
        v.n, v.m = int(lib.tpg_view_n(h)), int(lib.tpg_view_m(h))
        v.impute_report = _knn_report(rep, extra)
        return v

    def select_loci(self, idx) -> "View":
        """a new view of the loci idx (0-based positions in this view; any order, duplicates allowed) gathered on the device
        (tpg_view_select_loci): also works where the store cannot be packed again, as behind impute()"""
        idx = np.ascontiguousarray(idx, dtype=np.int64).ravel()
        h = C.c_void_p()
        check(lib.tpg_view_select_loci(self.ctx.h, self.h, _ptr(idx), len(idx), C.byref(h)))
        v = View.__new__(View)
        v.X, v.ctx, v.h = self.X, self.ctx, h
        v.n, v.m = int(lib.tpg_view_n(h)), int(lib.tpg_view_m(h))
        return v

    def unpack(self) -> np.ndarray:
        out = np.zeros((self.n, self.m), dtype=np.uint8, order="F")
        check(lib.tpg_view_unpack(self.ctx.h, self.h, _ptr(out)))
        return out

    def free(self):
        if self.h:
            lib.tpg_view_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Pairwise:
    """Integer N x N cross-product accumulators (tpg_pairwise)."""

    def __init__(self, ctx: Context, n: int, ext_buffer: Optional[int] = None):
        self.ctx, self.n = ctx, n
        h = C.c_void_p()
        check(lib.tpg_pairwise_create(ctx.h, n, ext_buffer, C.byref(h)))
        self.h = h

    @staticmethod
    def buffer_bytes(n: int) -> int:
        return int(lib.tpg_pairwise_buffer_bytes(n))

    def zero(self):
        check(lib.tpg_pairwise_zero(self.ctx.h, self.h))

    def accumulate(self, view: View, col_begin: int = 0, col_end: int = -1, products=None):
        """products: None = all five cross-products; else an OR of PW_V / PW_D / PW_H / PW_A or one of the sets
        PW_FOR_AS / PW_FOR_IBS / PW_FOR_KING (the kernel specialised for that set runs: include/tpg.h)"""
        if products is None:
            check(lib.tpg_pairwise_accumulate(self.ctx.h, self.h, view.h, col_begin, col_end))
        else:
            check(lib.tpg_pairwise_accumulate_products(self.ctx.h, self.h, view.h, col_begin, col_end, int(products)))

    def products(self) -> int:
        """the products whose sums are complete since the last zero()"""
        return int(lib.tpg_pairwise_products(self.h))

    def set_as_pad_quirk(self, narrow_blocks: int):
        """opt-in emulation of reference quirk Q1 (include/tpg.h): +narrow_blocks on every allele-sharing numerator"""
        check(lib.tpg_pairwise_set_as_pad_quirk(self.h, int(narrow_blocks)))

    def _mat(self):
        return np.zeros((self.n, self.n), order="F")

    def counts(self, which=("ibs", "ibs_valid", "king_num", "n_Aa_i", "as_num", "as_den")) -> dict:
        names = ("ibs", "ibs_valid", "king_num", "n_Aa_i", "as_num", "as_den")
        outs = {k: self._mat() for k in which}
        check(lib.tpg_pairwise_counts(self.ctx.h, self.h, *[_ptr(outs.get(k)) for k in names]))
        return outs

    def ibs(self, type: str = "proportion", m: int = 0) -> np.ndarray:
        out = self._mat()
        check(lib.tpg_pairwise_ibs(self.ctx.h, self.h, 0 if type == "proportion" else 1, m, _ptr(out)))
        return out

    def king(self) -> np.ndarray:
        out = self._mat()
        check(lib.tpg_pairwise_king(self.ctx.h, self.h, _ptr(out)))
        return out

    def allele_sharing(self) -> np.ndarray:
        out = self._mat()
        check(lib.tpg_pairwise_allele_sharing(self.ctx.h, self.h, _ptr(out)))
        return out

    def grm(self) -> np.ndarray:
        out = self._mat()
        check(lib.tpg_pairwise_grm(self.ctx.h, self.h, _ptr(out)))
        return out

    def sqdist(self, type: str = "raw", m: int = 0, out=None):
        """tpg_pairwise_sqdist (include/tpg.h "AMOVA"): the squared Euclidean distance of the dosages over the loci both
        individuals are typed at, "raw" or "adjusted" (raw * m / typed loci).  out: None (a new host matrix), a host matrix or a
        DeviceMatrix."""
        if type not in SQDIST_TYPES:
            raise ValueError("type must be 'raw' or 'adjusted'")
        if out is None:
            out = self._mat()
        check(lib.tpg_pairwise_sqdist(self.ctx.h, self.h, SQDIST_TYPES[type], int(m), out.p if isinstance(out, DeviceMatrix) else _ptr(out)))
        return out

    def epilogues(self, which=("ibs", "king", "allele_sharing", "grm"), ibs_type: str = "proportion", m: int = 0) -> dict:
        """IBS, KING, allele sharing and GRM from one pass over the accumulators"""
        names = ("ibs", "king", "allele_sharing", "grm")
        outs = {k: self._mat() for k in which}
        check(lib.tpg_pairwise_epilogues(self.ctx.h, self.h, 0 if ibs_type == "proportion" else 1, m,
                                         *[_ptr(outs.get(k)) for k in names]))
        return outs

    def free(self):
        if self.h:
            lib.tpg_pairwise_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Comm:
    """One rank of a group of GPUs that share an analysis sharded by loci (tpg_comm; include/tpg.h "SNP-block
    shards").  The library owns the collectives (RCCL); the launcher only has to deliver the 128-byte id."""

    def __init__(self, ctx: Context, handle, nranks: int, rank: int, keep=None):
        self.ctx, self.h, self.nranks, self.rank, self._keep = ctx, handle, nranks, rank, keep

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        check(lib.tpg_comm_unique_id(buf))
        return bytes(buf)

    @classmethod
    def init_rank(cls, ctx: Context, nranks: int, rank: int, unique_id: Optional[bytes]) -> "Comm":
        h = C.c_void_p()
        idbuf = (C.c_uint8 * 128).from_buffer_copy(unique_id) if unique_id is not None else None
        check(lib.tpg_comm_init_rank(ctx.h, nranks, rank, idbuf, C.byref(h)))
        return cls(ctx, h, nranks, rank)

    @classmethod
    def from_torch_distributed(cls, ctx: Context) -> "Comm":
        """Under torchrun: the process group (any backend -- gloo is enough) is only the control plane that carries
        the RCCL id from rank 0 to the others; the data path never goes through torch."""
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return cls.init_rank(ctx, 1, 0, None)
        # rank 0 always reaches the broadcast: a failure to make the id (no librccl.so ...) travels as a marker, so that
        # no rank is left waiting in the broadcast and every rank raises together
        box = [None]
        if dist.get_rank() == 0:
            try:
                box[0] = cls.unique_id()
            except Exception as e:  # noqa: BLE001
                box[0] = f"{type(e).__name__}: {e}"
        dist.broadcast_object_list(box, src=0)
        if not isinstance(box[0], (bytes, bytearray)):
            raise RuntimeError(f"rank 0 could not create the RCCL id: {box[0]}")
        return cls.init_rank(ctx, dist.get_world_size(), dist.get_rank(), box[0])

    @classmethod
    def host(cls, ctx: Context, nranks: int, rank: int, allreduce) -> "Comm":
        """Rehearsal transport (tests): allreduce(numpy array) sums the array in place over the ranks through host
        memory -- e.g. torch.distributed over gloo with several ranks on one GPU."""
        def _cb(user, buf, count, dtype):
            try:
                a = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_int32 if dtype == 0 else C.c_double)), shape=(count,))
                allreduce(a)
                return 0
            except Exception:  # never let an exception cross the C boundary
                return 1

        cb = _lib.HOST_ALLREDUCE(_cb)
        h = C.c_void_p()
        check(lib.tpg_comm_init_host(ctx.h, nranks, rank, cb, None, C.byref(h)))
        return cls(ctx, h, nranks, rank, keep=cb)

    def shard_loci(self, m_total: int):
        b, e = C.c_int64(), C.c_int64()
        check(lib.tpg_shard_loci(m_total, self.nranks, self.rank, C.byref(b), C.byref(e)))
        return b.value, e.value

    def allreduce_f64(self, buf, count: Optional[int] = None):
        """in-place sum over the ranks of a float64 numpy array, or of `count` doubles at a device pointer"""
        if isinstance(buf, np.ndarray):
            assert buf.dtype == np.float64 and buf.flags.c_contiguous or buf.flags.f_contiguous
            check(lib.tpg_comm_allreduce_f64(self.ctx.h, self.h, _ptr(buf), buf.size))
            return buf
        check(lib.tpg_comm_allreduce_f64(self.ctx.h, self.h, _ptr(buf), int(count)))
        return buf

    def transport(self) -> str:
        """'none', 'host callback' or 'rccl: <library as loaded>'"""
        return lib.tpg_comm_transport(self.h).decode()

    def close(self):
        if self.h:
            lib.tpg_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardedPairwise(Pairwise):
    """Pairwise accumulators of one rank: accumulate this rank's loci, reduce() (one reduce-scatter over the ranks),
    then counts() / epilogues() give this rank's band of the N x N outputs (band() tells which rows)."""

    def __init__(self, comm: Comm, n: int):
        self.ctx, self.n, self.comm = comm.ctx, n, comm
        h = C.c_void_p()
        check(lib.tpg_pairwise_create_sharded(comm.ctx.h, comm.h, n, C.byref(h)))
        self.h = h

    def reduce(self):
        check(lib.tpg_pairwise_reduce(self.ctx.h, self.comm.h, self.h))

    def reduce_begin(self, side_comm: "Comm"):
        """the reduce-scatter on a second communicator (one made on another context of the same device): runs beside what this
        context enqueues next; nothing may read the accumulators until reduce_end (include/tpg.h; opt-in)"""
        check(lib.tpg_pairwise_reduce_begin(self.ctx.h, side_comm.h, self.h))

    def reduce_end(self, side_comm: "Comm"):
        check(lib.tpg_pairwise_reduce_end(self.ctx.h, side_comm.h, self.h))

    def band(self):
        a, b = C.c_int64(), C.c_int64()
        check(lib.tpg_pairwise_band(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def epilogues(self, which=("ibs", "king", "allele_sharing", "grm"), ibs_type: str = "proportion", m: int = 0) -> dict:
        names = ("ibs", "king", "allele_sharing", "grm")
        outs = {k: np.full((self.n, self.n), np.nan, order="F") for k in which}  # outside the band: left as NaN
        check(lib.tpg_pairwise_epilogues_sharded(self.ctx.h, self.comm.h, self.h, 0 if ibs_type == "proportion" else 1,
                                                 m, *[_ptr(outs.get(k)) for k in names]))
        return outs


class Multi:
    """One process, several GPUs (tpg_multi): what an R session uses."""

    def __init__(self, ndev: int, devices=None):
        h = C.c_void_p()
        dv = _i32(devices)
        check(lib.tpg_multi_create(ndev, _ptr(dv), C.byref(h)))
        self.h, self.ndev = h, ndev

    def transport(self) -> str:
        """transport of the device threads' communicators: 'none', 'host callback' or 'rccl: <library as loaded>'"""
        return lib.tpg_comm_transport(lib.tpg_multi_comm(self.h, 0)).decode()

    def pairwise(self, X_bytes, ind_row=None, ind_col=None, which=("ibs", "king", "allele_sharing", "grm"),
                 ibs_type: str = "proportion") -> dict:
        """snp_ibs / snp_king / snp_allele_sharing / pairwise_grm of a host FBM (uint8, Fortran order) on all devices"""
        X_bytes = np.asarray(X_bytes)
        assert X_bytes.dtype == np.uint8 and X_bytes.flags.f_contiguous
        r, c = _i32(ind_row), _i32(ind_col)
        n = X_bytes.shape[0] if r is None else len(r)
        m = X_bytes.shape[1] if c is None else len(c)
        names = ("ibs", "king", "allele_sharing", "grm")
        outs = {k: np.full((n, n), np.nan, order="F") for k in which}
        check(lib.tpg_multi_pairwise(self.h, _ptr(X_bytes), X_bytes.shape[0], X_bytes.shape[1],
                                     _ptr(r), n, _ptr(c), m, 0 if ibs_type == "proportion" else 1,
                                     *[_ptr(outs.get(k)) for k in names]))
        return outs

    @staticmethod
    def _fbm_args(X_bytes, ind_row, ind_col):
        X_bytes = np.asarray(X_bytes)
        assert X_bytes.dtype == np.uint8 and X_bytes.flags.f_contiguous
        r, c = _i32(ind_row), _i32(ind_col)
        n = X_bytes.shape[0] if r is None else len(r)
        m = X_bytes.shape[1] if c is None else len(c)
        args = (_ptr(X_bytes), X_bytes.shape[0], X_bytes.shape[1], _ptr(r), n, _ptr(c), m)
        return args, n, m, (X_bytes, r, c)

    def loci_alt_freq(self, X_bytes, ind_row=None, ind_col=None, groupIds=None, ngroups: int = 0, ploidy=None,
                      as_counts: bool = False, code256=CODE_012) -> np.ndarray:
        """loci_alt_freq of a host FBM on all devices: m x 2G (grouped) or m x 2 ({n_alt | freq, n_valid})"""
        args, n, m, _keep = self._fbm_args(X_bytes, ind_row, ind_col)
        gid, code = _i32(groupIds), _f64(code256)
        pl = np.full(n, 2.0) if ploidy is None else _f64(ploidy)
        out = np.zeros((m, 2 * ngroups if gid is not None else 2), order="F")
        check(lib.tpg_multi_grouped_alt_freq(self.h, *args, _ptr(code), _ptr(gid), ngroups, _ptr(pl),
                                             int(as_counts), _ptr(out)))
        return out

    def pairwise_pop_fst(self, X_bytes, ind_row, ind_col, groupIds, ngroups: int, ploidy=None, method: str = "Hudson",
                         by_locus: bool = False, return_num_dem: bool = False, pairwise_combn=None, code256=CODE_012):
        """pairwise_pop_fst of a host FBM on all devices (same result layout as api.pairwise_pop_fst)"""
        args, n, m, _keep = self._fbm_args(X_bytes, ind_row, ind_col)
        if return_num_dem:
            by_locus = True
        pairs = combn2(ngroups) if pairwise_combn is None else np.asarray(pairwise_combn, dtype=np.int32)
        pairs_c = np.ascontiguousarray(pairs.T)
        P = pairs_c.shape[0]
        gid, code = _i32(groupIds), _f64(code256)
        pl = np.full(n, 2.0) if ploidy is None else _f64(ploidy)
        tot, a, b = _fst_outputs(m, P, by_locus, return_num_dem)
        check(lib.tpg_multi_pop_fst(self.h, *args, _ptr(code), _ptr(gid), ngroups, _ptr(pl),
                                    FST_METHODS[method], _ptr(pairs_c), P, int(by_locus),
                                    int(return_num_dem), _ptr(tot), _ptr(a), _ptr(b)))
        return _fst_result(tot, a, b, by_locus, return_num_dem)

    def gt_pca_partialSVD(self, X_bytes, ind_row=None, ind_col=None, k: int = 10, total_var: bool = True,
                          code256=CODE_IMPUTE_PRED) -> dict:
        """gt_pca_partialSVD of a host FBM on all devices (same result as api.gt_pca_partialSVD)"""
        args, n, m, _keep = self._fbm_args(X_bytes, ind_row, ind_col)
        code = _f64(code256)
        d = np.zeros(k)
        u = np.zeros((n, k), order="F")
        vl = np.zeros((m, k), order="F")
        center, scale = np.zeros(m), np.zeros(m)
        fro = C.c_double()
        check(lib.tpg_multi_pca_partial_svd(self.h, *args, _ptr(code), k, _ptr(d), _ptr(u), _ptr(vl), _ptr(center),
                                            _ptr(scale), C.byref(fro) if total_var else None))
        out = dict(d=d, u=u, v=vl, center=center, scale=scale, method="partialSVD")
        if total_var:
            out["square_frobenius"] = fro.value
        return out

    def close(self):
        if self.h:
            lib.tpg_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Stream:
    """A genotype store that stays on the HOST and is swept in blocks of loci (tpg_stream, include/tpg.h): the
    reference's own block loop (R/snp_ibs.R:59-82, R/loci_alt_freq.R:351-359, big_SVD's two sweeps behind
    R/gt_pca_partialSVD.R:82-89) inside the library.  budget_bytes bounds the HBM taken by store bytes + packed views +
    per-block scratch (0 = no bound)."""

    def __init__(self, ctx: Context, handle, nrow: int, ncol: int, keep=None):
        self.ctx, self.h, self.nrow, self.ncol, self._keep = ctx, handle, nrow, ncol, keep
        self.report = None

    @classmethod
    def from_numpy(cls, bytes_2d, budget_bytes: int = 0, ctx: Optional[Context] = None) -> "Stream":
        """host FBM bytes (uint8, Fortran order: a numpy memmap of the .bk works) -- not copied, kept referenced"""
        ctx = ctx or default_context()
        a = np.asarray(bytes_2d) if not isinstance(bytes_2d, np.memmap) else bytes_2d
        if a.dtype != np.uint8 or a.ndim != 2 or not a.flags.f_contiguous:
            raise TypeError("FBM bytes must be a 2-D uint8 array in Fortran order (individuals x loci)")
        h = C.c_void_p()
        check(lib.tpg_stream_open_host(ctx.h, _ptr(a), a.shape[0], a.shape[1], int(budget_bytes), C.byref(h)))
        return cls(ctx, h, a.shape[0], a.shape[1], keep=a)

    @classmethod
    def open_bk(cls, path: str, nrow: int, ncol: int, budget_bytes: int = 0, ctx: Optional[Context] = None) -> "Stream":
        ctx = ctx or default_context()
        h = C.c_void_p()
        check(lib.tpg_stream_open_bk(ctx.h, path.encode(), nrow, ncol, int(budget_bytes),
                                     C.byref(h)))
        return cls(ctx, h, nrow, ncol)

    @classmethod
    def open_bed(cls, path: str, n: int, m: int, budget_bytes: int = 0, ctx: Optional[Context] = None) -> "Stream":
        ctx = ctx or default_context()
        h = C.c_void_p()
        check(lib.tpg_stream_open_bed(ctx.h, path.encode(), n, m, int(budget_bytes),
                                      C.byref(h)))
        return cls(ctx, h, n, m)

    @classmethod
    def from_bed_payload(cls, payload, n: int, m: int, budget_bytes: int = 0, ctx: Optional[Context] = None) -> "Stream":
        """the bytes of a PLINK .bed behind its 3-byte magic (uint8, m * ceil(n / 4)) -- not copied, kept referenced"""
        ctx = ctx or default_context()
        a = np.ascontiguousarray(payload, dtype=np.uint8)
        assert a.size == m * ((n + 3) // 4)
        h = C.c_void_p()
        check(lib.tpg_stream_open_bed_host(ctx.h, _ptr(a), n, m, int(budget_bytes),
                                           C.byref(h)))
        return cls(ctx, h, n, m, keep=a)

    @classmethod
    def synth(cls, seed: int, nrow: int, ncol: int, npop: int = 51, miss: float = 0.02, imputed_bytes: bool = False,
              budget_bytes: int = 0, ctx: Optional[Context] = None) -> "Stream":
        """the synthetic panel of FBM.synth generated block by block on the device (panels larger than host memory)"""
        ctx = ctx or default_context()
        thr = min(int(round(miss * 2 ** 32)), 2 ** 32 - 1)
        h = C.c_void_p()
        check(lib.tpg_stream_open_synth(ctx.h, seed, nrow, ncol, npop, thr, int(imputed_bytes), int(budget_bytes),
                                        C.byref(h)))
        return cls(ctx, h, nrow, ncol)

    def run(self, ind_row=None, ind_col=None, pairwise=(), ibs_type: str = "proportion", code256=CODE_012, ploidy=None,
            groupIds=None, ngroups: int = 0, as_counts: bool = False, alt_freq: bool = False, grouped_alt_freq: bool = False,
            grouped_missingness: bool = False, loci_counts: bool = False, fst=(), fst_by_locus: bool = False,
            fst_return_num_dem: bool = False, pairwise_combn=None, k: int = 0, pca_tol: float = 0.0, code256_pca=CODE_IMPUTE_PRED, total_var: bool = True,
            multi: Optional["Multi"] = None, impute: Optional[str] = None, impute_seed: int = 0) -> dict:
        """One streamed pass for everything asked for (tpg_stream_run; with `multi`, tpg_multi_stream_run: the loci
        sharded over its devices).  pairwise: any of "ibs", "king", "allele_sharing", "grm"; fst: up to three of
        "Hudson", "Nei87", "WC84"; k > 0: gt_pca_partialSVD (pca_tol > 0: gt_pca_randomSVD's tolerance).  Returns the
        results under the names of the resident functions, plus "report" (blocks, bytes moved, peak HBM).
        impute = "mode" | "mean0" | "random": the PCA of every block runs on the imputed raw view (View.impute, keyed by
        the position in the selection: every block plan gives the same fill); code256_pca is then CODE_012."""
        r, c = _i32(ind_row), _i32(ind_col)
        n = self.nrow if r is None else len(r)
        m = self.ncol if c is None else len(c)
        job = _lib.StreamJob()
        job.struct_size = C.sizeof(_lib.StreamJob)
        keep = [r, c]
        job.rowInd1, job.n, job.colInd1, job.m = _ptr(r), n, _ptr(c), m
        out = {}
        job.ibs_type = 0 if ibs_type == "proportion" else 1
        for name in pairwise:
            if name not in ("ibs", "king", "allele_sharing", "grm"):
                raise ValueError(f"unknown pairwise output {name!r}")
            out[name] = np.empty((n, n), order="F")  # (every element is written: rows and their mirror images)
            setattr(job, name, _ptr(out[name]))
        code = _f64(code256)
        pl = None if ploidy is None else _f64(ploidy)
        gid = _i32(groupIds)
        keep += [code, pl, gid]
        job.code256, job.ploidy, job.groupIds0, job.ngroups, job.as_counts = _ptr(code), _ptr(pl), _ptr(gid), int(ngroups), int(as_counts)
        if alt_freq:
            out["alt_freq"] = np.empty((m, 2), order="F")
            job.alt_freq = _ptr(out["alt_freq"])
        if grouped_alt_freq:
            out["grouped_alt_freq"] = np.empty((m, 2 * ngroups), order="F")
            job.grouped_alt_freq = _ptr(out["grouped_alt_freq"])
        if grouped_missingness:
            out["grouped_missingness"] = np.empty((m, ngroups), order="F")
            job.grouped_missingness = _ptr(out["grouped_missingness"])
        if loci_counts:
            out["loci_counts"] = np.empty((m, 4), dtype=np.int32)
            job.loci_counts = _ptr(out["loci_counts"])
        if fst:
            pairs = combn2(ngroups) if pairwise_combn is None else np.asarray(pairwise_combn, dtype=np.int32)
            pairs_c = np.ascontiguousarray(pairs.T)
            keep.append(pairs_c)
            P = pairs_c.shape[0]
            job.nfst, job.pairs1, job.P = len(fst), _ptr(pairs_c), P
            if fst_return_num_dem:
                fst_by_locus = True  # R/pairwise_pop_fst.R:103-106
            job.fst_return_num_dem = int(fst_return_num_dem)
            out["fst_tot"], out["fst_locus"], out["fst_locus_den"] = {}, {}, {}
            for i, method in enumerate(fst):
                job.fst_method[i] = FST_METHODS[method]
                out["fst_tot"][method] = np.zeros(P)
                job.fst_tot[i] = out["fst_tot"][method].ctypes.data
                if fst_by_locus:
                    out["fst_locus"][method] = np.empty((m, P), order="F")  # (the numerators under fst_return_num_dem)
                    job.fst_by_locus[i] = out["fst_locus"][method].ctypes.data
                if fst_return_num_dem:
                    out["fst_locus_den"][method] = np.empty((m, P), order="F")
                    job.fst_by_locus_den[i] = out["fst_locus_den"][method].ctypes.data
            if not fst_by_locus:
                del out["fst_locus"]
            if not fst_return_num_dem:
                del out["fst_locus_den"]
        fro = C.c_double()
        if impute is not None:
            job.impute_method, job.impute_seed = _impute_method(impute), int(impute_seed)
        if k > 0:
            cp = _f64(CODE_012 if impute is not None else code256_pca)
            keep.append(cp)
            out.update(d=np.zeros(k), u=np.empty((n, k), order="F"), v=np.empty((m, k), order="F"), center=np.empty(m),
                       scale=np.empty(m), method="partialSVD" if pca_tol == 0 else "randomSVD")
            job.code256_pca, job.k, job.pca_tol = _ptr(cp), int(k), float(pca_tol)
            for name in ("d", "u", "v", "center", "scale"):
                setattr(job, name, _ptr(out[name]))
            if total_var:
                job.square_frobenius = C.cast(C.pointer(fro), C.c_void_p)
        rep = _lib.StreamReport()
        if multi is not None:
            check(lib.tpg_multi_stream_run(multi.h, self.h, C.byref(job), C.byref(rep)))
        else:
            check(lib.tpg_stream_run(self.ctx.h, self.h, C.byref(job), C.byref(rep)))
        if k > 0 and total_var:
            out["square_frobenius"] = fro.value
        self.report = {f: getattr(rep, f) for f, _ in _lib.StreamReport._fields_}
        out["report"] = self.report
        return out

    def qc(self, ind_row=None, ind_col=None, code256=CODE_012, groupIds=None, ngroups: int = 0, mid_p: bool = True,
           loci_counts: bool = False, hwe: bool = False, grouped_counts: bool = False, grouped_hwe: bool = False,
           indiv_counts: bool = False) -> dict:
        """The QC pass (tpg_stream_qc): one streamed sweep for the counts and exact tests behind qc_report_loci and
        qc_report_indiv.  Returns what was asked for under the names of the resident functions -- "loci_counts" (m, 4),
        "loci_hwe" (m,), "grouped_genotype_counts" (3, m, G), "gt_grouped_hwe" (m, G), "indiv_counts" (n, 4) -- bit for bit
        what those give on a resident View of the same selection, plus "report"."""
        r, c = _i32(ind_row), _i32(ind_col)
        n = self.nrow if r is None else len(r)
        m = self.ncol if c is None else len(c)
        G = int(ngroups)
        job = _lib.StreamQcJob()
        job.struct_size = C.sizeof(_lib.StreamQcJob)
        code, gid = _f64(code256), _i32(groupIds)
        job.rowInd1, job.n, job.colInd1, job.m = _ptr(r), n, _ptr(c), m
        job.code256, job.groupIds0, job.ngroups, job.midp = _ptr(code), _ptr(gid), G, int(bool(mid_p))
        out = {}
        if loci_counts:
            out["loci_counts"] = np.empty((m, 4), dtype=np.int32)
            job.loci_counts = _ptr(out["loci_counts"])
        if hwe:
            out["loci_hwe"] = np.empty(m)
            job.hwe_p = _ptr(out["loci_hwe"])
        gc = None
        if grouped_counts:
            gc = np.empty((3, max(G, 0), m), dtype=np.int32)  # three column-major m x G matrices
            job.grouped_counts = _ptr(gc)
        if grouped_hwe:
            out["gt_grouped_hwe"] = np.empty((m, max(G, 0)), order="F")
            job.grouped_hwe_p = _ptr(out["gt_grouped_hwe"])
        if indiv_counts:
            out["indiv_counts"] = np.empty((n, 4), dtype=np.int32)
            job.indiv_counts = _ptr(out["indiv_counts"])
        rep = _lib.StreamReport()
        check(lib.tpg_stream_qc(self.ctx.h, self.h, C.byref(job), C.byref(rep)))
        if gc is not None:
            out["grouped_genotype_counts"] = np.ascontiguousarray(gc.transpose(0, 2, 1))
        self.report = {f: getattr(rep, f) for f, _ in _lib.StreamReport._fields_}
        out["report"] = self.report
        return out

    def close(self):
        if self.h:
            lib.tpg_stream_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------
# R-level functions

def _raw_view(X: FBM, ind_row, ind_col) -> View:
    # increment_{ibs,king,as}_counts compare the RAW bytes with 0/1/2 (src/snp_ibs.cpp:47-54)
    return View(X, ind_row, ind_col, code256=None)


def _pairwise_pass(X: FBM, ind_row, ind_col, products=None):
    v = _raw_view(X, ind_row, ind_col)
    pw = Pairwise(X.ctx, v.n)
    pw.accumulate(v, products=products)
    return v, pw


def snp_ibs(X: FBM, ind_row=None, ind_col=None, type: str = "proportion", block_size=None):
    """R/snp_ibs.R:42-104.  block_size is accepted for signature compatibility; the whole locus
    range is swept in one device pass (results do not depend on it)."""
    if type not in ("proportion", "adjusted_counts", "raw_counts"):
        raise ValueError("'arg' should be one of 'proportion', 'adjusted_counts', 'raw_counts'")
    v, pw = _pairwise_pass(X, ind_row, ind_col, PW_FOR_IBS_ALONE)  # V and D + H: three MFMAs into two sums per tile pair
    if type == "raw_counts":
        c = pw.counts(("ibs", "ibs_valid"))
        return dict(ibs=c["ibs"], valid_n=c["ibs_valid"])
    return pw.ibs(type, v.m)


def snp_king(X: FBM, ind_row=None, ind_col=None, block_size=None):
    """R/snp_king.R:32-103"""
    _, pw = _pairwise_pass(X, ind_row, ind_col, PW_FOR_KING)  # V, D, A, A': 4 of 5
    return pw.king()


def as_pad_quirk_blocks(m: int, block_size: int) -> int:
    """blocks narrower than the widest when CutBySize(m, block_size) cuts m loci (R/local_reimplementations.R:13-15)"""
    return int(lib.tpg_as_pad_quirk_blocks(int(m), int(block_size)))


def _as_pass(X, ind_row, ind_col, block_size, emulate_as_pad_quirk):
    v, pw = _pairwise_pass(X, ind_row, ind_col, PW_FOR_AS)  # V, D: 2 of 5
    if emulate_as_pad_quirk:
        # what the reference BINARY returns: +1 on every numerator per narrower block (src/snp_as.cpp:57-63)
        pw.set_as_pad_quirk(as_pad_quirk_blocks(v.m, block_size or block_size_default(X.nrow)))
    return pw


def snp_allele_sharing(X: FBM, ind_row=None, ind_col=None, block_size=None, emulate_as_pad_quirk: bool = False):
    """R/snp_allele_sharing.R:33-82.  Default: the mathematically intended value (what the reference's test asserts
    through hierfstat::matching).  emulate_as_pad_quirk = True reproduces what the reference binary computes when
    its blocks are unequal (quirk Q1 of SURVEY.md 8a) for the given block_size (default bigstatsr::block_size)."""
    return _as_pass(X, ind_row, ind_col, block_size, emulate_as_pad_quirk).allele_sharing()


def pairwise_grm(X: FBM, ind_row=None, ind_col=None, block_size=None, emulate_as_pad_quirk: bool = False):
    """R/pairwise_grm.R:30-51 on top of snp_allele_sharing"""
    return _as_pass(X, ind_row, ind_col, block_size, emulate_as_pad_quirk).grm()


def block_means(A, groupIds, ngroups: int, skip_diag: bool = True, ctx: Optional[Context] = None):
    """mean(A[p1, p2], na.rm = TRUE) for every pair of groups (R/pop_fst.R:47-62) -> (G, G) means, (G, G) counts"""
    ctx = ctx or default_context()
    A = np.asfortranarray(A, dtype=np.float64)
    gid = _i32(groupIds)
    mean, cnt = np.zeros((ngroups, ngroups), order="F"), np.zeros((ngroups, ngroups), order="F")
    check(lib.tpg_block_means(ctx.h, _ptr(A), A.shape[0], _ptr(gid), ngroups,
                              int(skip_diag), _ptr(mean), _ptr(cnt)))
    return mean, cnt


def _as_block_stats(X, ind_row, ind_col, groupIds, ngroups, allele_sharing_mat):
    if ngroups < 1:
        raise ValueError(".x should be a grouped gen_tibble")
    if allele_sharing_mat is None:
        allele_sharing_mat = snp_allele_sharing(X, ind_row, ind_col)
    mMij, _ = block_means(allele_sharing_mat, groupIds, ngroups, skip_diag=True, ctx=X.ctx if X is not None else None)
    Fsts = np.diag(mMij).copy()
    # Mb: sum of the strictly lower triangle in the reference's loop order (i = 2..n_pop, j = 1..i-1), :53-63
    Mb = 0.0
    for i in range(1, ngroups):
        for j in range(i):
            Mb = Mb + mMij[i, j]
    with np.errstate(invalid="ignore", divide="ignore"):
        Mb = Mb * 2 / (ngroups * (ngroups - 1))
    return allele_sharing_mat, Fsts, Mb


def pop_fst(X: FBM, ind_row, ind_col, groupIds, ngroups: int, include_global: bool = False, allele_sharing_mat=None):
    """R/pop_fst.R:31-76 (Weir & Goudet 2017 population-specific Fst from the allele-sharing matrix)"""
    _, Fsts, Mb = _as_block_stats(X, ind_row, ind_col, groupIds, ngroups, allele_sharing_mat)
    with np.errstate(invalid="ignore", divide="ignore"):
        fst = (Fsts - Mb) / (1 - Mb)
        if include_global:
            fst = np.append(fst, np.nanmean(fst) if np.any(~np.isnan(fst)) else np.nan)
    return fst


def pop_fis_wg17(X: FBM, ind_row, ind_col, groupIds, ngroups: int, include_global: bool = False, allele_sharing_mat=None):
    """R/pop_fis.R:136-197 (method = "WG17")"""
    A, Fsts, _ = _as_block_stats(X, ind_row, ind_col, groupIds, ngroups, allele_sharing_mat)
    Mii = np.diag(np.asarray(A)) * 2 - 1
    gid = np.asarray(groupIds)
    out = np.full(ngroups, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        for g in range(ngroups):
            Fi = (Mii[gid == g] - Fsts[g]) / (1 - Fsts[g])
            if np.any(~np.isnan(Fi)):
                out[g] = np.nanmean(Fi)
        if include_global:
            out = np.append(out, np.nanmean(out) if np.any(~np.isnan(out)) else np.nan)
    return out


def filter_high_relatedness(matrix, kings_threshold, ids=None, ctx: Optional[Context] = None):
    """R/filter_high_relatedness.R:26-145 -> [ids that pass (in the order of decreasing mean relatedness), ids to
    remove, logical keep vector in the original order].  `matrix`: (n, n) numpy array, or a raw device pointer together
    with ids (its length gives n) -- e.g. the KING matrix left in HBM by Pairwise.king into a dev_alloc'ed buffer.
    ids default to "1" .. "n", as the reference names an unnamed matrix."""
    ctx = ctx or default_context()
    if kings_threshold is None:
        raise ValueError("argument \"kings_threshold\" is missing")
    if isinstance(matrix, (int, np.integer, C.c_void_p)):
        if ids is None:
            raise ValueError("ids are needed with a device matrix")
        n, mp = len(ids), (matrix if isinstance(matrix, C.c_void_p) else C.c_void_p(int(matrix)))
    else:
        A = np.asfortranarray(matrix, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise ValueError("matrix should be a square matrix")
        n, mp = A.shape[0], _ptr(A)
    ids = np.array([str(k) for k in range(1, n + 1)]) if ids is None else np.asarray(ids)
    keep, order = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32)
    check(lib.tpg_filter_high_relatedness(ctx.h, mp, n, float(kings_threshold), _ptr(keep),
                                          _ptr(order)))
    keepb = keep.astype(bool)
    passed = ids[order][keepb[order]]
    return [passed, ids[~keepb], keepb]


def increment_ibs_counts(k, k2, X_bytes, rowInd, colInd, ctx: Optional[Context] = None, flush: bool = True):
    """Literal mirror of src/snp_ibs.cpp:22-74 (X_bytes is the host FBM; every call uploads the columns of its own
    block, nothing of the FBM is kept).  flush = True (default): k, k2 are incremented when the call returns, as in the
    reference.  flush = False (tpg_increment_defer): the sums stay in device accumulators across the calls of a block loop
    and reach k, k2 at increment_flush()."""
    return _increment(lib.tpg_increment_ibs_counts, k, k2, X_bytes, rowInd, colInd, ctx, flush)


def increment_king_numerator(k, n_Aa_i, X_bytes, rowInd, colInd, ctx: Optional[Context] = None, flush: bool = True):
    """Literal mirror of src/snp_king.cpp:21-74"""
    return _increment(lib.tpg_increment_king_numerator, k, n_Aa_i, X_bytes, rowInd, colInd, ctx, flush)


def increment_as_counts(k, k2, X_bytes, rowInd, colInd, ctx: Optional[Context] = None, flush: bool = True,
                        scratch_cols: Optional[int] = None, emulate_as_pad_quirk: bool = False):
    """Literal mirror of src/snp_as.cpp:22-67.  scratch_cols = number of columns of the scratch matrices the R driver
    passes; with emulate_as_pad_quirk a block one column narrower than that adds +1 to every numerator (quirk Q1)."""
    ctx = ctx or default_context()
    _increment(lib.tpg_increment_as_counts, k, k2, X_bytes, rowInd, colInd, ctx, flush)
    if emulate_as_pad_quirk and scratch_cols is not None and scratch_cols == len(colInd) + 1:
        check(lib.tpg_increment_as_note_narrow_block(ctx.h, _ptr(k), k.shape[0]))


def increment_flush(ctx: Optional[Context] = None):
    """add the sums the increment_* mirrors hold on the device to their host matrices"""
    ctx = ctx or default_context()
    check(lib.tpg_increment_flush(ctx.h))


def resident_drop(ctx: Optional[Context] = None):
    """release the device scratch the increment_* mirrors keep between calls"""
    ctx = ctx or default_context()
    check(lib.tpg_resident_drop(ctx.h))


def _increment(fn, a, b, X_bytes, rowInd, colInd, ctx, flush):
    ctx = ctx or default_context()
    X_bytes = np.asarray(X_bytes)
    assert X_bytes.dtype == np.uint8 and X_bytes.flags.f_contiguous
    assert a.flags.f_contiguous and b.flags.f_contiguous and a.dtype == np.float64 and b.dtype == np.float64
    r, c = _i32(rowInd), _i32(colInd)
    check(lib.tpg_increment_defer(ctx.h, int(not flush)))  # switching it off flushes what is pending
    check(fn(ctx.h, _ptr(a), _ptr(b), _ptr(X_bytes), X_bytes.shape[0], X_bytes.shape[1],
             _ptr(r), len(r), _ptr(c), len(c)))


def _ploidy(v: View, ploidy):
    return np.full(v.n, 2.0) if ploidy is None else _f64(ploidy)


def loci_counts(v: View) -> np.ndarray:
    out = np.zeros((v.m, 4), dtype=np.int32)
    check(lib.tpg_loci_counts(v.ctx.h, v.h, _ptr(out)))
    return out


def indiv_counts(v: View) -> np.ndarray:
    out = np.zeros((v.n, 4), dtype=np.int32)
    check(lib.tpg_indiv_counts(v.ctx.h, v.h, _ptr(out)))
    return out


def gt_ind_hetero(v: View) -> np.ndarray:
    """src/gt_ind_hetero.cpp:11-42 -> (2, n) integer matrix: row 0 heterozygous loci, row 1 missing loci"""
    out = np.zeros((2, v.n), dtype=np.int32, order="F")
    check(lib.tpg_gt_ind_hetero(v.ctx.h, v.h, _ptr(out)))
    return out


def gt_pi_diploid(v: View) -> np.ndarray:
    """src/gt_pi_diploid.cpp:7-38"""
    out = np.zeros(v.m)
    check(lib.tpg_gt_pi_diploid(v.ctx.h, v.h, _ptr(out)))
    return out


def gt_grouped_pi_diploid(v: View, groupIds, ngroups: int) -> dict:
    """src/gt_grouped_pi_diploid.cpp:7-42"""
    pi, n = np.zeros((v.m, ngroups), order="F"), np.zeros((v.m, ngroups), order="F")
    gid = _i32(groupIds)
    check(lib.tpg_gt_grouped_pi_diploid(v.ctx.h, v.h, _ptr(gid), ngroups, _ptr(pi), _ptr(n)))
    return dict(pi=pi, n=n)


def grouped_genotype_counts(v: View, groupIds, ngroups: int) -> np.ndarray:
    """the genotype table of gt_grouped_hwe (src/hwe.cpp:238-250) -> (3, m, G) int32: [k] = individuals with k alternate alleles"""
    out = np.zeros((3, ngroups, v.m), dtype=np.int32)  # three column-major m x G matrices
    gid = _i32(groupIds)
    check(lib.tpg_grouped_genotype_counts(v.ctx.h, v.h, _ptr(gid), ngroups, _ptr(out)))
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def hwe_on_matrix(geno_counts, midp, ctx: Optional[Context] = None) -> np.ndarray:
    """src/hwe.cpp:203-213: the exact test on every column of a 3 x m count matrix, rows hom1 / het / hom2 as
    bigstatsr::big_counts gives them (tpg_hwe_exact_counts)"""
    ctx = ctx or default_context()
    g = np.asarray(geno_counts)
    if g.ndim != 2 or g.shape[0] < 3:
        raise ValueError("geno_counts must have the rows hom1, het, hom2")
    counts = np.ascontiguousarray(g[:3].T, dtype=np.int32)  # column-major 3 x m
    out = np.zeros(counts.shape[0])
    check(lib.tpg_hwe_exact_counts(ctx.h, _ptr(counts), counts.shape[0], bool(midp), _ptr(out)))
    return out


def SNPHWE2_R(obs_hets, obs_hom1, obs_hom2, midp, ctx: Optional[Context] = None) -> float:
    """src/hwe.cpp:193-200: one table; the heterozygotes come first"""
    return float(hwe_on_matrix(np.array([[obs_hom1], [obs_hets], [obs_hom2]]), midp, ctx)[0])


def gt_grouped_hwe(v: View, groupIds, ngroups: int, mid_p: bool = True) -> np.ndarray:
    """src/hwe.cpp:220-253 -> (m, G) p-values; counts and tests both on the device (tpg_gt_grouped_hwe)"""
    out = np.zeros((v.m, ngroups), order="F")
    gid = _i32(groupIds)
    check(lib.tpg_gt_grouped_hwe(v.ctx.h, v.h, _ptr(gid), ngroups, bool(mid_p), _ptr(out)))
    return out


def loci_hwe(X: FBM, ind_row=None, ind_col=None, mid_p: bool = True) -> np.ndarray:
    """R/loci_hwe.R:64-95 (ungrouped) -> (m,) p-values"""
    if (X.nrow if ind_row is None else len(ind_row)) < 2:
        raise ValueError("Not implemented for a single individual")
    v = View(X, ind_row, ind_col)
    out = np.zeros(v.m)
    check(lib.tpg_loci_hwe(v.ctx.h, v.h, bool(mid_p), _ptr(out)))
    return out


def qc_loci_from_counts(loci_counts) -> dict:
    """maf and missingness of qc_report_loci from the (m, 4) genotype counts {n0, n1, n2, nNA}: f = (n1 + 2 n2) /
    (2 (n - nNA)), maf = min(f, 1 - f) (R/loci_maf.R over loci_alt_freq: NaN at a locus nobody is typed at), missingness =
    nNA / n (R/loci_missingness.R)"""
    c = np.asarray(loci_counts, dtype=np.int64)
    n = c.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = (c[:, 1] + 2 * c[:, 2]) / (2.0 * (n - c[:, 3]))
        return dict(maf=np.minimum(f, 1.0 - f), missingness=c[:, 3] / n.astype(float))


def qc_indiv_from_counts(indiv_counts, store_ncol: int) -> dict:
    """the columns of qc_report_indiv from the (n, 4) per-individual counts {n0, n1, n2, nNA} over the m selected loci.
    het_obs follows R/indiv_het_obs.R:69 literally: het_n / (ncol(store) - na_n) -- the STORE's column count, not m; the
    two agree when every locus of the store is selected.  missingness = na_n / m."""
    c = np.asarray(indiv_counts, dtype=np.int64)
    m = c.sum(axis=1)
    het_n, na_n = c[:, 1].astype(np.int32), c[:, 3].astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(het_obs=het_n / (float(store_ncol) - na_n), missingness=na_n / m.astype(float), het_n=het_n, na_n=na_n)


def qc_report_loci(S, ind_row=None, ind_col=None, groupIds=None, ngroups: int = 0, mid_p: bool = True) -> dict:
    """qc_report_loci -> {"maf", "missingness", "hwe_p"}, each (m,).  Ungrouped (R/qc_report_loci.R:50-57): hwe_p as loci_hwe.
    With groupIds (R/qc_report_loci.R:96-107): the smallest of the locus's per-group p-values times ngroups; maf and
    missingness stay those of all selected individuals.  S is a Stream (one streamed pass, Stream.qc, through CODE_012) or an
    FBM (the resident functions through its own table): the report does not depend on where the store lives."""
    grouped = groupIds is not None
    if isinstance(S, Stream):
        q = S.qc(ind_row, ind_col, groupIds=groupIds, ngroups=ngroups, mid_p=mid_p, loci_counts=True, hwe=not grouped,
                 grouped_hwe=grouped)
        counts, p = q["loci_counts"], q["gt_grouped_hwe"] if grouped else q["loci_hwe"]
    else:
        v = View(S, ind_row, ind_col)
        counts = loci_counts(v)
        p = gt_grouped_hwe(v, groupIds, ngroups, mid_p) if grouped else loci_hwe(S, ind_row, ind_col, mid_p)
    out = qc_loci_from_counts(counts)
    out["hwe_p"] = p.min(axis=1) * ngroups if grouped else p
    return out


def qc_report_indiv(S, ind_row=None, ind_col=None) -> dict:
    """qc_report_indiv without its KING column (R/qc_report_indiv.R:77-84; Stream.run(pairwise=("king",)) gives that one) ->
    {"het_obs", "missingness", "het_n", "na_n"}, each (n,): het_n / na_n are the two rows of gt_ind_hetero, the other two as
    qc_indiv_from_counts states them (het_obs divides by the store's column count, as R/indiv_het_obs.R:69 does).  S is a
    Stream (one streamed pass) or an FBM (the resident functions)."""
    if isinstance(S, Stream):
        counts = S.qc(ind_row, ind_col, indiv_counts=True)["indiv_counts"]
    else:
        counts = indiv_counts(View(S, ind_row, ind_col))
    return qc_indiv_from_counts(counts, S.ncol)


GLOBAL_STATS_COLUMNS = ("Ho", "Hs", "Ht", "Dst", "Htp", "Dstp", "Fst", "Fstp", "Fis", "Dest")


def pop_global_stats(X: FBM, ind_row, ind_col, groupIds, ngroups: int, ploidy=None, by_locus: bool = False):
    """R/pop_global_stats.R:113-212 -> (m, 10) array (by_locus) or the 10 overall values; columns GLOBAL_STATS_COLUMNS"""
    v = View(X, ind_row, ind_col)
    gid = _i32(groupIds)
    pl = _ploidy(v, ploidy)
    loc = np.zeros((v.m, 10), order="F") if by_locus else None
    ov = np.zeros(10)
    check(lib.tpg_pop_global_stats(v.ctx.h, v.h, _ptr(gid), ngroups, _ptr(pl),
                                   _ptr(loc) if by_locus else None, _ptr(ov)))
    return loc if by_locus else ov


def _pop_basic(X, ind_row, ind_col, groupIds, ngroups, ploidy, which, by_locus, include_global, global_col):
    v = View(X, ind_row, ind_col)
    gid, pl = _i32(groupIds), _ploidy(v, ploidy)
    loc = np.zeros((v.m, ngroups), order="F") if by_locus else None
    cm = np.zeros(ngroups)
    check(lib.tpg_pop_basic_stats(v.ctx.h, v.h, _ptr(gid), ngroups, _ptr(pl), which,
                                  _ptr(loc) if by_locus else None, _ptr(cm)))
    if not include_global:
        return loc if by_locus else cm
    g_loc = pop_global_stats(X, ind_row, ind_col, groupIds, ngroups, ploidy, by_locus=True)[:, global_col]
    if by_locus:
        return np.column_stack([loc, g_loc])
    with np.errstate(invalid="ignore"):
        return np.append(cm, np.nanmean(g_loc) if np.any(~np.isnan(g_loc)) else np.nan)


def pop_het_obs(X: FBM, ind_row, ind_col, groupIds, ngroups: int, ploidy=None, by_locus=False, include_global=False):
    """R/pop_het_obs.R:52-92"""
    return _pop_basic(X, ind_row, ind_col, groupIds, ngroups, ploidy, 0, by_locus, include_global, 0)


def pop_het_exp(X: FBM, ind_row, ind_col, groupIds, ngroups: int, ploidy=None, by_locus=False, include_global=False):
    """R/pop_het_exp.R:53-104 (alias pop_gene_div)"""
    return _pop_basic(X, ind_row, ind_col, groupIds, ngroups, ploidy, 1, by_locus, include_global, 1)


pop_gene_div = pop_het_exp


def pop_fis(X: FBM, ind_row, ind_col, groupIds, ngroups: int, ploidy=None, method: str = "Nei87", by_locus=False,
            include_global=False, allele_sharing_mat=None):
    """R/pop_fis.R:56-133"""
    if method not in ("Nei87", "WG17"):
        raise ValueError("'arg' should be one of 'Nei87', 'WG17'")
    if method == "WG17":
        if by_locus:
            raise ValueError("by_locus not implemented for WG17")
        return pop_fis_wg17(X, ind_row, ind_col, groupIds, ngroups, include_global, allele_sharing_mat)
    if allele_sharing_mat is not None:
        raise ValueError("allele_sharing_mat not relevant for Nei87")
    if by_locus or not include_global:
        return _pop_basic(X, ind_row, ind_col, groupIds, ngroups, ploidy, 2, by_locus, include_global, 8)
    # by_locus = FALSE with the global value: the reference takes pop_global_stats(by_locus = FALSE)["Fis"], :126-130
    cm = _pop_basic(X, ind_row, ind_col, groupIds, ngroups, ploidy, 2, False, False, 8)
    return np.append(cm, pop_global_stats(X, ind_row, ind_col, groupIds, ngroups, ploidy, by_locus=False)[8])


def alt_freq_dip_pseudo_cpp(v: View, ploidy=None, as_counts: bool = False) -> np.ndarray:
    """src/alt_freq_dip_pseudo_cpp.cpp:8-58 -> (m, 2)"""
    out = np.zeros((v.m, 2), order="F")
    pl = _ploidy(v, ploidy)
    check(lib.tpg_alt_freq_dip_pseudo(v.ctx.h, v.h, _ptr(pl), int(as_counts), _ptr(out)))
    return out


def loci_alt_freq(X: FBM, ind_row=None, ind_col=None, ploidy=None, as_counts: bool = False, block_size=None):
    """R/loci_alt_freq.R:328-379"""
    v = View(X, ind_row, ind_col)
    freq = alt_freq_dip_pseudo_cpp(v, ploidy, as_counts)
    return freq if as_counts else freq[:, 0]


def loci_missingness(X: FBM, ind_row=None, ind_col=None, as_counts: bool = False, block_size=None):
    """R/loci_missingness.R:97-134"""
    v = View(X, ind_row, ind_col)
    n_na = loci_counts(v)[:, 3].astype(float)
    return n_na if as_counts else n_na / v.n


def grouped_alt_freq_dip_pseudo_cpp(v: View, groupIds, ngroups: int, ploidy=None, as_counts: bool = False):
    """src/grouped_alt_freq_dip_pseudo_cpp.cpp:8-58 -> (m, 2G)"""
    out = np.zeros((v.m, 2 * ngroups), order="F")
    gid, pl = _i32(groupIds), _ploidy(v, ploidy)
    check(lib.tpg_grouped_alt_freq_dip_pseudo(v.ctx.h, v.h, _ptr(gid), ngroups, _ptr(pl),
                                              int(as_counts), _ptr(out)))
    return out


def grouped_missingness_cpp(v: View, groupIds, ngroups: int):
    """src/grouped_missingness_cpp.cpp:8-33 -> (m, G)"""
    out = np.zeros((v.m, ngroups), order="F")
    gid = _i32(groupIds)
    check(lib.tpg_grouped_missingness(v.ctx.h, v.h, _ptr(gid), ngroups, _ptr(out)))
    return out


def grouped_summaries_dip_pseudo_cpp(v: View, groupIds, ngroups: int, ploidy=None) -> dict:
    """src/grouped_summaries_dip_pseudo_cpp.cpp:11-63"""
    outs = [np.zeros((v.m, ngroups), order="F") for _ in range(4)]
    gid, pl = _i32(groupIds), _ploidy(v, ploidy)
    check(lib.tpg_grouped_summaries_dip_pseudo(v.ctx.h, v.h, _ptr(gid), ngroups, _ptr(pl),
                                               *[_ptr(o) for o in outs]))
    return dict(freq_alt=outs[0], freq_ref=outs[1], n=outs[2], het_obs=outs[3])


def combn2(G: int) -> np.ndarray:
    """utils::combn(G, 2) (R/pairwise_pop_fst.R:119): 2 x P, 1-based"""
    cols = [(a, b) for a in range(1, G + 1) for b in range(a + 1, G + 1)]
    return np.array(cols, dtype=np.int32).T.reshape(2, -1)


def _fst_outputs(m, P, by_locus, return_num_dem):
    tot = np.zeros(P)
    a = np.zeros((m, P), order="F") if by_locus else None
    b = np.zeros((m, P), order="F") if return_num_dem else None
    return tot, a, b


def _fst_result(tot, a, b, by_locus, return_num_dem):
    if return_num_dem:
        return dict(Fst_by_locus_num=a, Fst_by_locus_den=b)
    return dict(fst_locus=a if by_locus else np.zeros((0, 0)), fst_tot=tot)


def pairwise_pop_fst(X: FBM, ind_row, ind_col, groupIds, ngroups: int, ploidy=None, method: str = "Hudson",
                     by_locus: bool = False, return_num_dem: bool = False, pairwise_combn=None, sums: bool = False):
    """R/pairwise_pop_fst.R:71-161 (numeric part; the tidy / matrix formatting is out of scope).  sums = True
    (not in the reference): also return the sums of numerators and denominators over the loci, the additive
    quantities a run sharded by loci exchanges."""
    if method not in FST_METHODS:
        raise ValueError("'arg' should be one of 'Hudson', 'Nei87', 'WC84'")
    if not isinstance(return_num_dem, (bool, np.bool_)):
        raise ValueError("return_num_dem must be a logical value (TRUE or FALSE)")
    if return_num_dem:
        by_locus = True
    v = View(X, ind_row, ind_col)
    pairs = combn2(ngroups) if pairwise_combn is None else np.asarray(pairwise_combn, dtype=np.int32)
    pairs_c = np.ascontiguousarray(pairs.T)  # (P, 2) row-major == 2 x P column-major
    P = pairs_c.shape[0]
    gid, pl = _i32(groupIds), _ploidy(v, ploidy)
    if sums:
        if by_locus:
            raise ValueError("sums = True returns totals only")
        sn, sd = np.zeros(P), np.zeros(P)
        check(lib.tpg_pairwise_pop_fst_sums(v.ctx.h, v.h, _ptr(gid), ngroups, _ptr(pl),
                                            FST_METHODS[method], _ptr(pairs_c), P, _ptr(sn), _ptr(sd)))
        with np.errstate(invalid="ignore", divide="ignore"):
            return dict(fst_tot=sn / sd, sum_num=sn, sum_den=sd)
    tot, a, b = _fst_outputs(v.m, P, by_locus, return_num_dem)
    check(lib.tpg_pairwise_pop_fst(v.ctx.h, v.h, _ptr(gid), ngroups, _ptr(pl),
                                   FST_METHODS[method], _ptr(pairs_c), P, int(by_locus),
                                   int(return_num_dem), _ptr(tot), _ptr(a), _ptr(b)))
    return _fst_result(tot, a, b, by_locus, return_num_dem)


def window_index_ranges(chromosome, position, window_size, step_size, size_unit="snp", complete=False):
    """Host part of windows_stats_generic (R/windows_stats_generic.R:113-141 and runner's window rule, recalled:
    the window ending at `at` holds the indices in (at - k, at]; with na_pad = TRUE a window that reaches outside
    the index range is NA).  Loci must be ordered by position inside a chromosome, chromosomes in blocks, as in a
    gen_tibble.  -> dict(chromosome, start, end, lo, hi, pad_na) with lo/hi 0-based half-open locus ranges."""
    if size_unit not in ("snp", "bp"):
        raise ValueError("'arg' should be one of 'snp', 'bp'")
    if not isinstance(complete, (bool, np.bool_)):
        raise ValueError("complete must be a boolean (logical).")
    if window_size <= 0:
        raise ValueError("window_size must be positive.")
    if step_size <= 0:
        raise ValueError("step_size must be positive.")
    chromosome = np.asarray(chromosome)
    if size_unit == "bp":
        if position is None:
            raise ValueError("loci_table must contain columns 'chromosome' and 'position' when size_unit is 'bp'.")
        position = np.asarray(position, dtype=np.float64)
    chroms, starts_, ends_, lo, hi, pad = [], [], [], [], [], []
    seen = []
    for ch in chromosome:  # unique(), order of first appearance
        if ch not in seen:
            seen.append(ch)
    for ch in seen:
        idx = np.where(chromosome == ch)[0]
        first = int(idx[0])
        if not np.array_equal(idx, np.arange(first, first + len(idx))):
            raise ValueError("the loci of a chromosome must be contiguous")
        pos = position[idx] if size_unit == "bp" else np.arange(1, len(idx) + 1, dtype=np.float64)
        if np.any(np.diff(pos) < 0):
            raise ValueError("positions must be sorted inside a chromosome")
        r0, r1 = math.ceil(pos.min() / window_size), math.ceil(pos.max() / window_size)
        at = np.arange(r0 * window_size, r1 * window_size + 1e-9 * step_size, step_size, dtype=np.float64)
        for a in at:
            w_lo = int(np.searchsorted(pos, a - window_size, side="right"))  # first index with pos > at - k
            w_hi = int(np.searchsorted(pos, a, side="right"))                # one past the last with pos <= at
            chroms.append(ch); starts_.append(a - window_size + 1); ends_.append(a)
            lo.append(first + w_lo); hi.append(first + w_hi)
            pad.append(bool(complete) and (a - window_size + 1 < pos[0] or a > pos[-1]))
    return dict(chromosome=np.array(chroms), start=np.array(starts_), end=np.array(ends_),
                lo=np.array(lo, dtype=np.int64), hi=np.array(hi, dtype=np.int64), pad_na=np.array(pad, dtype=np.uint8))


def _window_stats(ctx, x_ptr, m, ncol, wr, op, min_loci):
    nw = len(wr["lo"])
    stat = np.zeros((nw, ncol), order="F")
    nl = np.zeros((nw, ncol), dtype=np.int32, order="F")
    lo, hi, pad = wr["lo"], wr["hi"], wr["pad_na"]
    check(lib.tpg_window_stats(ctx.h, x_ptr, m, ncol, _ptr(lo), _ptr(hi), _ptr(pad), nw,
                               op, int(min_loci), _ptr(stat), _ptr(nl)))
    return stat, nl


def windows_stats_generic(x, chromosome, position=None, operator="mean", window_size=None, step_size=None,
                          size_unit="snp", min_loci=1, complete=False, ctx: Optional[Context] = None):
    """R/windows_stats_generic.R:47-184 for operator "mean" / "sum" -> dict(chromosome, start, end, stat, n_loci)"""
    if operator not in ("mean", "sum"):
        raise ValueError("'arg' should be one of 'mean', 'sum' (a custom function runs on the host in the reference; its one use, "
                         "Tajima's D, is windows_pop_tajimas_d)")
    x = np.ascontiguousarray(x, dtype=np.float64)
    if len(chromosome) != len(x):
        raise ValueError("loci_table must have the same number of rows as x.")
    if min_loci is not None and min_loci <= 0:
        raise ValueError("min_loci must be positive.")
    wr = window_index_ranges(chromosome, position, window_size, step_size, size_unit, complete)
    if min_loci > window_size:
        raise ValueError("min_loci must be less than window_size.")
    ctx = ctx or default_context()
    stat, nl = _window_stats(ctx, _ptr(x), len(x), 1, wr, 0 if operator == "mean" else 1, min_loci)
    n_loci = nl[:, 0].astype(float)
    n_loci[nl[:, 0] < 0] = np.nan
    return dict(chromosome=wr["chromosome"], start=wr["start"], end=wr["end"], stat=stat[:, 0], n_loci=n_loci)


def windows_pairwise_pop_fst(X: FBM, ind_row, ind_col, groupIds, ngroups: int, chromosome, position=None, ploidy=None,
                             window_size=None, step_size=None, size_unit="snp", min_loci=1, complete=False, route="staged"):
    """R/windows_pairwise_pop_fst.R:49-118 (type = "matrix"): window means of the by-locus Hudson numerators and
    denominators, then their ratio (the reference always takes Hudson here, whatever `method` says, :62-65).
    route = "staged": the two m x P matrices stay in HBM and tpg_window_stats reduces them; route = "fused":
    tpg_windows_pairwise_pop_fst goes from the count table to the windows and never forms them (windows_fst).
    -> dict(chromosome, start, end, fst (nw, P))"""
    if route not in ("staged", "fused"):
        raise ValueError("route must be 'staged' or 'fused'")
    v = View(X, ind_row, ind_col)
    if len(chromosome) != v.m:
        raise ValueError("loci_table must have the same number of rows as x.")
    wr = window_index_ranges(chromosome, position, window_size, step_size, size_unit, complete)
    if min_loci <= 0:
        raise ValueError("min_loci must be positive.")
    if min_loci > window_size:
        raise ValueError("min_loci must be less than window_size.")
    if route == "fused":
        r = windows_fst(v, groupIds, ngroups, wr["lo"], wr["hi"], wr["pad_na"], min_loci, ploidy, "Hudson")
        return dict(chromosome=wr["chromosome"], start=wr["start"], end=wr["end"], fst=r["fst"])
    pairs_c = np.ascontiguousarray(combn2(ngroups).T)
    P = pairs_c.shape[0]
    gid, pl = _i32(groupIds), _ploidy(v, ploidy)
    ctx = v.ctx
    nbytes = 8 * v.m * P
    d_num, d_den = ctx.dev_alloc(nbytes), ctx.dev_alloc(nbytes)
    try:
        check(lib.tpg_pairwise_pop_fst(ctx.h, v.h, _ptr(gid), ngroups, _ptr(pl), FST_METHODS["Hudson"],
                                       _ptr(pairs_c), P, 1, 1, None, d_num, d_den))
        num, _ = _window_stats(ctx, d_num, v.m, P, wr, 0, min_loci)
        den, _ = _window_stats(ctx, d_den, v.m, P, wr, 0, min_loci)
    finally:
        ctx.dev_free(d_num)
        ctx.dev_free(d_den)
    with np.errstate(invalid="ignore", divide="ignore"):
        fst = num / den
    return dict(chromosome=wr["chromosome"], start=wr["start"], end=wr["end"], fst=fst)


# include/tpg.h "windowed pairwise Fst": loci per chunk partial of the fused window scan (the order of a window's sum is
# defined in terms of it)
WINFST_CHUNK_LOCI = int(lib.tpg_winfst_chunk_loci()) if hasattr(lib, "tpg_winfst_chunk_loci") else 0


def windows_fst_scratch_bytes(m: int, ngroups: int, P: int, nw: int) -> int:
    """tpg_windows_fst_scratch_bytes: the device scratch one windows_fst call takes beyond the count table (host only)"""
    return int(lib.tpg_windows_fst_scratch_bytes(int(m), int(ngroups), int(P), int(nw)))


def _window_args(lo, hi, pad_na):
    lo, hi = np.ascontiguousarray(lo, dtype=np.int64), np.ascontiguousarray(hi, dtype=np.int64)
    pad = None if pad_na is None else np.ascontiguousarray(pad_na, dtype=np.uint8)
    if len(hi) != len(lo) or (pad is not None and len(pad) != len(lo)):
        raise ValueError("lo, hi and pad_na must have one entry per window")
    return lo, hi, pad


def windows_fst(v: View, groupIds, ngroups, lo, hi, pad_na=None, min_loci: int = 1, ploidy=None, method: str = "Hudson",
                pairwise_combn=None, return_parts: bool = False) -> dict:
    """tpg_windows_pairwise_pop_fst on explicit 0-based half-open locus ranges (include/tpg.h "windowed pairwise Fst"): from
    the view's count table to the windows, without the m x P by-locus matrices.  -> dict(fst (nw, P)); return_parts adds
    mean_num, mean_den (nw, P) and n_num, n_den (nw, P int32, -1 on a pad_na window)."""
    if method not in FST_METHODS:
        raise ValueError("'arg' should be one of 'Hudson', 'Nei87', 'WC84'")
    lo, hi, pad = _window_args(lo, hi, pad_na)
    nw = len(lo)
    pairs = combn2(ngroups) if pairwise_combn is None else np.asarray(pairwise_combn, dtype=np.int32)
    pairs_c = np.ascontiguousarray(pairs.T)  # (P, 2) row-major == 2 x P column-major
    P = pairs_c.shape[0]
    gid, pl = _i32(groupIds), _ploidy(v, ploidy)
    fst = np.zeros((nw, P), order="F")
    parts = [np.zeros((nw, P), order="F"), np.zeros((nw, P), order="F"), np.zeros((nw, P), dtype=np.int32, order="F"),
             np.zeros((nw, P), dtype=np.int32, order="F")] if return_parts else [None] * 4
    check(lib.tpg_windows_pairwise_pop_fst(v.ctx.h, v.h, _ptr(gid), int(ngroups), _ptr(pl), FST_METHODS[method], _ptr(pairs_c), P,
                                           _ptr(lo), _ptr(hi), _ptr(pad), nw, int(min_loci), _ptr(fst), *[_ptr(a) for a in parts]))
    out = dict(fst=fst)
    if return_parts:
        out.update(mean_num=parts[0], mean_den=parts[1], n_num=parts[2], n_den=parts[3])
    return out


def fst_relabel_sums(v: View, labels, ngroups: int, pairs=None, method: str = "Hudson") -> dict:
    """tpg_fst_relabel_sums (include/tpg.h "Fst under relabelings"): labels is R x n, -1 = outside the relabeling; pairs is
    2 x P, 1-based (default: every pair).  -> dict(sum_num, sum_den (R, P), n_kept (R, P int64), fst = sum_num / sum_den)."""
    if method not in FST_METHODS:
        raise ValueError("'arg' should be one of 'Hudson', 'Nei87', 'WC84'")
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    if lab.ndim == 1:
        lab = lab.reshape(1, -1)
    if lab.ndim != 2 or lab.shape[1] != v.n:
        raise ValueError("labels must have one column per individual of the view")
    R = lab.shape[0]
    pairs = combn2(ngroups) if pairs is None else np.asarray(pairs, dtype=np.int32)
    pairs_c = np.ascontiguousarray(pairs.T)  # (P, 2) row-major == 2 x P column-major
    P = pairs_c.shape[0]
    sn, sd, nk = np.zeros((R, P)), np.zeros((R, P)), np.zeros((R, P), dtype=np.int64)
    check(lib.tpg_fst_relabel_sums(v.ctx.h, v.h, _ptr(lab), R, int(ngroups), FST_METHODS[method], _ptr(pairs_c), P, _ptr(sn), _ptr(sd),
                                   _ptr(nk)))
    with np.errstate(invalid="ignore", divide="ignore"):
        return dict(sum_num=sn, sum_den=sd, n_kept=nk, fst=sn / sd)


FST_PERM_SCHEMES = {"pairwise": 0, "global": 1}


def fst_perm_labels(n: int, groupIds, ngroups: int, scheme, a: int, b: int, seed: int, r: int) -> np.ndarray:
    """tpg_fst_perm_labels: the r-th relabeling of the scheme ("pairwise" / 0: groups a and b, 0-based, become labels 0 and 1,
    everybody else -1; "global" / 1: everybody keeps a group); r = 0 is the identity.  Host only."""
    gid = _i32(groupIds)
    if gid is None or gid.shape != (n,):
        raise ValueError("groupIds must have one entry per individual")
    out = np.zeros(n, dtype=np.int32)
    sch = FST_PERM_SCHEMES[scheme] if isinstance(scheme, str) else int(scheme)
    check(lib.tpg_fst_perm_labels(int(n), _ptr(gid), int(ngroups), sch, int(a), int(b), int(seed) & 0xFFFFFFFFFFFFFFFF, int(r), _ptr(out)))
    return out


def fst_perm_pvalue(fst_obs, fst_perm):
    """the permutation p-value (host): fst_obs (P), fst_perm (n_perm, P) -> (p, n_valid); n_valid = the number of finite permuted
    values, p = (1 + #{finite permuted >= observed}) / (1 + n_valid), NaN where the observed value is not finite"""
    obs = np.atleast_1d(np.asarray(fst_obs, dtype=np.float64))
    perm = np.asarray(fst_perm, dtype=np.float64).reshape(-1, obs.shape[0])
    fin = np.isfinite(perm)
    n_valid = fin.sum(axis=0).astype(np.int64)
    with np.errstate(invalid="ignore"):
        ge = (fin & (perm >= obs[None, :])).sum(axis=0)
    p = (1.0 + ge) / (1.0 + n_valid)
    return np.where(np.isfinite(obs), p, np.nan), n_valid


def pairwise_pop_fst_test(X: FBM, ind_row, ind_col, groupIds, ngroups: int, method: str = "Hudson", n_perm: int = 999, seed: int = 0,
                          scheme: str = "pairwise", pairwise_combn=None, return_perm: bool = False, max_rows: int = 4096) -> dict:
    """Permutation test of pairwise Fst (no counterpart in the reference).  scheme = "pairwise": for every pair the individuals
    of its two populations are shuffled between them (rows r = 0 .. n_perm of tpg_fst_perm_labels scheme 0, two groups per
    relabeling), all pairs' rows going down in batches of at most max_rows; "global": everybody is shuffled, one label matrix of
    1 + n_perm rows with ngroups groups (at most 64).  -> dict(fst_tot, p_value, n_valid (P)), with return_perm also perm_fst
    (n_perm, P).  fst_tot is row 0, the identity, through the same kernel, so that ties compare like with like."""
    if method not in FST_METHODS:
        raise ValueError("'arg' should be one of 'Hudson', 'Nei87', 'WC84'")
    if scheme not in FST_PERM_SCHEMES:
        raise ValueError("scheme must be 'pairwise' or 'global'")
    if n_perm < 1 or max_rows < 1:
        raise ValueError("n_perm and max_rows must be positive")
    v = View(X, ind_row, ind_col)
    gid = _i32(groupIds)
    pairs = combn2(ngroups) if pairwise_combn is None else np.asarray(pairwise_combn, dtype=np.int32).reshape(2, -1)
    P, nr = pairs.shape[1], 1 + int(n_perm)
    fst = np.zeros((nr, P))
    if scheme == "global":
        if ngroups > 64:
            raise ValueError("scheme = 'global' holds at most 64 groups in one relabeling: use scheme = 'pairwise'")
        for r0 in range(0, nr, max_rows):
            lab = np.stack([fst_perm_labels(v.n, gid, ngroups, 1, 0, 0, seed, r) for r in range(r0, min(nr, r0 + max_rows))])
            fst[r0:r0 + len(lab)] = fst_relabel_sums(v, lab, ngroups, pairs, method)["fst"]
    else:
        one = np.array([[1], [2]], dtype=np.int32)
        todo = [(k, r) for k in range(P) for r in range(nr)]
        for t0 in range(0, len(todo), max_rows):
            part = todo[t0:t0 + max_rows]
            lab = np.stack([fst_perm_labels(v.n, gid, ngroups, 0, int(pairs[0, k]) - 1, int(pairs[1, k]) - 1, seed, r) for k, r in part])
            f = fst_relabel_sums(v, lab, 2, one, method)["fst"][:, 0]
            for (k, r), x in zip(part, f):
                fst[r, k] = x
    p, n_valid = fst_perm_pvalue(fst[0], fst[1:])
    out = dict(fst_tot=fst[0].copy(), p_value=p, n_valid=n_valid)
    if return_perm:
        out["perm_fst"] = fst[1:].copy()
    return out


class DeviceMatrix:
    """An n x n column-major matrix of doubles that stays in HBM between two library calls (tpg_dev_alloc): what
    pairwise_sqdist(device=True) returns and class_sums / gt_amova accept."""

    def __init__(self, ctx: Context, n: int):
        self.ctx, self.n = ctx, int(n)
        self.p = ctx.dev_alloc(8 * self.n * self.n)

    @classmethod
    def from_numpy(cls, A, ctx: Optional[Context] = None) -> "DeviceMatrix":
        a = np.asfortranarray(A, dtype=np.float64)
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError("A must be a square matrix")
        d = cls(ctx or default_context(), a.shape[0])
        check(lib.tpg_dev_from_host(d.ctx.h, d.p, _ptr(a), a.nbytes))
        return d

    def to_numpy(self) -> np.ndarray:
        out = np.zeros((self.n, self.n), order="F")
        check(lib.tpg_dev_to_host(self.ctx.h, _ptr(out), self.p, out.nbytes))
        return out

    def free(self):
        if self.p is not None:
            lib.tpg_dev_free(self.p)
            self.p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


SQDIST_TYPES = {"raw": 0, "adjusted": 1}


def pairwise_sqdist(X: FBM, ind_row=None, ind_col=None, type: str = "raw", device: bool = False):
    """Squared genotype distances between individuals from one pairwise pass with the KING set of products.  device = True:
    the matrix stays in HBM (a DeviceMatrix, which class_sums and gt_amova accept)."""
    if type not in SQDIST_TYPES:
        raise ValueError("type must be 'raw' or 'adjusted'")
    v, pw = _pairwise_pass(X, ind_row, ind_col, PW_FOR_KING)
    return pw.sqdist(type, v.m, DeviceMatrix(X.ctx, v.n) if device else None)


def class_sums(A, labels, nclasses: int, ctx: Optional[Context] = None) -> np.ndarray:
    """tpg_class_sums: A is n x n (a numpy array or a DeviceMatrix), labels is R x n with -1 = outside the labeling ->
    (R, nclasses) sums of A[i, j] over the ordered pairs of each class, in the order include/tpg.h "AMOVA" defines."""
    if isinstance(A, DeviceMatrix):
        ctx, n, pa, keep = A.ctx, A.n, A.p, A
    else:
        ctx = ctx or default_context()
        keep = np.asfortranarray(A, dtype=np.float64)
        if keep.ndim != 2 or keep.shape[0] != keep.shape[1]:
            raise ValueError("A must be a square matrix")
        n, pa = keep.shape[0], _ptr(keep)
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    if lab.ndim == 1:
        lab = lab.reshape(1, -1)
    if lab.ndim != 2 or lab.shape[1] != n:
        raise ValueError("labels must have one column per row of A")
    sums = np.zeros((lab.shape[0], max(int(nclasses), 0)))
    check(lib.tpg_class_sums(ctx.h, pa, n, _ptr(lab), lab.shape[0], int(nclasses), _ptr(sums)))
    return sums


AMOVA_SCHEMES = {"ST": 0, "SC": 1, "CT": 2}


def amova_perm_labels(n: int, pop, npop: int, region_of_pop, nregion: int, scheme, seed: int, r: int):
    """tpg_amova_perm_labels: the r-th relabeling of scheme "ST" / 0 (individuals among all populations), "SC" / 1 (inside every
    region) or "CT" / 2 (whole populations among the regions); r = 0 is the identity.  -> (pop (n), region_of_pop (npop) or None).
    Host only."""
    p0 = _i32(pop)
    if p0 is None or p0.shape != (n,):
        raise ValueError("pop must have one entry per individual")
    g0 = _i32(region_of_pop) if nregion > 0 else None
    if g0 is not None and g0.shape != (npop,):
        raise ValueError("region_of_pop must have one entry per population")
    sch = AMOVA_SCHEMES[scheme] if isinstance(scheme, str) else int(scheme)
    po, go = np.zeros(n, dtype=np.int32), (np.zeros(npop, dtype=np.int32) if g0 is not None else None)
    check(lib.tpg_amova_perm_labels(int(n), _ptr(p0), int(npop), _ptr(g0), int(nregion), sch, int(seed) & 0xFFFFFFFFFFFFFFFF, int(r),
                                    _ptr(po), _ptr(go)))
    return po, go


def amova_from_sums(pop_size, pop_sum, total_sum: float, region_of_pop=None, region_sum=None) -> dict:
    """tpg_amova_from_sums: one relabeling's class sums -> dict(df (4), ssd (4), msd (3), ncoef (3), sigma2 (4), phi (3)); rows
    (among regions, among populations within regions, within populations, total), phi = (CT, SC, ST).  Host only."""
    ps, pw = np.ascontiguousarray(pop_size, dtype=np.int64), _f64(pop_sum)
    if ps.ndim != 1 or pw.shape != ps.shape:
        raise ValueError("pop_size and pop_sum must have one entry per population")
    g0, rs = (_i32(region_of_pop), _f64(region_sum)) if region_of_pop is not None else (None, None)
    if g0 is not None and (g0.shape != ps.shape or rs is None or rs.ndim != 1 or (len(g0) and rs.shape[0] <= int(g0.max()))):
        raise ValueError("region_of_pop needs one entry per population and region_sum one per region")
    out = np.zeros(21)
    check(lib.tpg_amova_from_sums(len(ps), _ptr(ps), _ptr(pw), 0 if g0 is None else len(rs), _ptr(g0), _ptr(rs), float(total_sum), _ptr(out)))
    return dict(df=out[0:4].copy(), ssd=out[4:8].copy(), msd=out[8:11].copy(), ncoef=out[11:14].copy(), sigma2=out[14:18].copy(),
                phi=out[18:21].copy())


def gt_amova(X: Optional[FBM] = None, ind_row=None, ind_col=None, pop=None, npop: int = 0, region_of_pop=None, dist=None,
             dist_type: str = "raw", n_perm: int = 999, seed: int = 0, return_perm: bool = False) -> dict:
    """Analysis of molecular variance with permutation tests (no counterpart in the reference; include/tpg.h "AMOVA").  pop (n,
    0-based, -1 = left out) and region_of_pop (npop, 0-based; None: two levels) give the hierarchy.  The squared distances come
    from X by one pairwise pass (dist_type "raw" or "adjusted") and stay in HBM, or from dist (any n x n matrix or DeviceMatrix).
    One class_sums call per kind of labeling -- the all-zero row (T), the population rows, the region rows -- each holding the
    identity and the relabelings of the schemes that change it: "ST" shuffles individuals among all populations, "SC" inside
    every region (the region sums stay), "CT" whole populations among the regions (the population sums stay).
    -> dict(table = dict(source, df, ssd, msd, sigma2, percent), ncoef, phi, p_value, n_valid (each (CT, SC, ST))), with
    return_perm also perm = {scheme: dict(phi (n_perm, 3), sigma2 (n_perm, 4))}."""
    if pop is None or npop < 1:
        raise ValueError("pop and npop are required")
    if n_perm < 1:
        raise ValueError("n_perm must be positive")
    if (X is None) == (dist is None):
        raise ValueError("give either X or dist")
    A = pairwise_sqdist(X, ind_row, ind_col, dist_type, device=True) if dist is None else dist
    if not isinstance(A, DeviceMatrix):
        A = np.asfortranarray(A, dtype=np.float64)
    n = A.n if isinstance(A, DeviceMatrix) else A.shape[0]
    ctx = A.ctx if isinstance(A, DeviceMatrix) else (X.ctx if X is not None else None)
    p0 = _i32(pop)
    if p0.shape != (n,):
        raise ValueError("pop must have one entry per individual")
    g0 = _i32(region_of_pop) if region_of_pop is not None else None
    G = 0 if g0 is None else int(g0.max()) + 1 if len(g0) else 0
    amova_perm_labels(n, p0, npop, g0, G, 0, seed, 0)  # the checks of the design: an empty population, a bad id
    size = np.bincount(p0[p0 >= 0], minlength=npop).astype(np.int64)
    schemes = ["ST"] + (["SC", "CT"] if G else [])
    rel = {s: [amova_perm_labels(n, p0, npop, g0, G, s, seed, r) for r in range(1, n_perm + 1)] for s in schemes}
    T = class_sums(A, np.where(p0 >= 0, 0, -1), 1, ctx)[0, 0]
    W = class_sums(A, np.stack([p0] + [p for s in ("ST", "SC") if s in rel for p, _ in rel[s]]), npop, ctx)
    W_of = {"ST": W[1:1 + n_perm], "SC": W[1 + n_perm:1 + 2 * n_perm]}
    if G:
        def induced(p, g):  # the region of everybody's population, -1 staying outside
            return np.where(p >= 0, g[np.maximum(p, 0)], -1).astype(np.int32)

        Rg = class_sums(A, np.stack([induced(p0, g0)] + [induced(p, g0) for p, _ in rel["ST"]] + [induced(p0, g) for _, g in rel["CT"]]), G,
                        ctx)
        R_of = {"ST": Rg[1:1 + n_perm], "CT": Rg[1 + n_perm:1 + 2 * n_perm]}
    obs = amova_from_sums(size, W[0], T, g0, Rg[0] if G else None)
    perm = {}
    for s in schemes:
        rows = []
        for k in range(n_perm):
            w = W_of[s][k] if s != "CT" else W[0]
            rg = None if not G else R_of[s][k] if s != "SC" else Rg[0]
            rows.append(amova_from_sums(size, w, T, rel[s][k][1] if s == "CT" else g0, rg))
        perm[s] = dict(phi=np.stack([x["phi"] for x in rows]), sigma2=np.stack([x["sigma2"] for x in rows]))
    col = {"CT": 0, "SC": 1, "ST": 2}
    p_value, n_valid = np.full(3, np.nan), np.zeros(3, dtype=np.int64)
    for s in schemes:
        p, nv = fst_perm_pvalue(obs["phi"][col[s]], perm[s]["phi"][:, col[s]])
        p_value[col[s]], n_valid[col[s]] = p[0], nv[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        percent = 100.0 * obs["sigma2"] / obs["sigma2"][3]
    keep = slice(0, 4) if G else slice(1, 4)
    table = dict(source=["among regions", "among populations within regions", "within populations", "total"][keep] if G
                 else ["among populations", "within populations", "total"],
                 df=obs["df"][keep], ssd=obs["ssd"][keep], msd=np.append(obs["msd"], np.nan)[keep], sigma2=obs["sigma2"][keep],
                 percent=percent[keep])
    out = dict(table=table, ncoef=obs["ncoef"], phi=obs["phi"], p_value=p_value, n_valid=n_valid)
    if return_perm:
        out["perm"] = perm
    return out


def _square(A, ctx):
    """a numpy array or a DeviceMatrix -> (ctx, n, pointer, the object that keeps the memory alive)"""
    if isinstance(A, DeviceMatrix):
        return A.ctx, A.n, A.p, A
    keep = np.asfortranarray(A, dtype=np.float64)
    if keep.ndim != 2 or keep.shape[0] != keep.shape[1]:
        raise ValueError("a square matrix is required")
    return ctx, keep.shape[0], _ptr(keep), keep


def mantel_sums(A, Bs, perms, ctx: Optional[Context] = None) -> np.ndarray:
    """tpg_mantel_sums: A and every B of the list Bs are n x n (numpy arrays or DeviceMatrix), perms is R x n, every row a
    permutation of 0 .. n-1 -> (R, Q) sums over i != j of A[perm[i], perm[j]] * B_q[i, j], in the order include/tpg.h "Mantel
    tests" defines."""
    if isinstance(Bs, (np.ndarray, DeviceMatrix)):
        Bs = [Bs]
    for M in [A, *Bs]:
        if isinstance(M, DeviceMatrix):
            ctx = M.ctx
    ctx = ctx or default_context()
    _, n, pa, keep_a = _square(A, ctx)
    mats = [_square(B, ctx) for B in Bs]
    if any(m[1] != n for m in mats):
        raise ValueError("every matrix must be n x n")
    pm = np.ascontiguousarray(perms, dtype=np.int32)
    if pm.ndim == 1:
        pm = pm.reshape(1, -1)
    if pm.ndim != 2 or pm.shape[1] != n:
        raise ValueError("perms must have one column per row of A")
    Q = len(mats)
    pb = (C.c_void_p * max(Q, 1))(*[m[2] for m in mats])
    sums = np.zeros((pm.shape[0], Q))
    check(lib.tpg_mantel_sums(ctx.h, pa, pb, Q, n, _ptr(pm), pm.shape[0], _ptr(sums)))
    return sums


def mantel_pass_rows(n: int, Q: int) -> int:
    """tpg_mantel_pass_rows: the permutations of one internal pass of mantel_sums at (n, Q); -1 on a bad size"""
    return int(lib.tpg_mantel_pass_rows(int(n), int(Q)))


def mantel_scratch_bytes(n: int, R: int, Q: int) -> int:
    """tpg_mantel_scratch_bytes: the device scratch of a mantel_sums call, bounded independently of R; -1 on a bad size"""
    return int(lib.tpg_mantel_scratch_bytes(int(n), int(R), int(Q)))


def offdiag_moments(A, ctx: Optional[Context] = None):
    """tpg_offdiag_moments: -> (S, SS), the sums of a_ij and of a_ij^2 over i != j in the order of mantel_sums"""
    ctx, n, pa, keep = _square(A, ctx or (None if isinstance(A, DeviceMatrix) else default_context()))
    out = np.zeros(2)
    check(lib.tpg_offdiag_moments(ctx.h, pa, n, _ptr(out)))
    return float(out[0]), float(out[1])


def offdiag_center(A, mean: float, out=None, ctx: Optional[Context] = None):
    """tpg_offdiag_center: a_ij - mean off the diagonal, +0.0 on it.  A DeviceMatrix gives a DeviceMatrix (out=A: in place), a
    numpy array a new numpy array."""
    if isinstance(A, DeviceMatrix):
        out = DeviceMatrix(A.ctx, A.n) if out is None else out
        check(lib.tpg_offdiag_center(A.ctx.h, A.p, A.n, float(mean), out.p))
        return out
    ctx, n, pa, keep = _square(A, ctx or default_context())
    res = np.zeros((n, n), order="F")
    check(lib.tpg_offdiag_center(ctx.h, pa, n, float(mean), _ptr(res)))
    return res


def mantel_perms(n: int, seed: int, r0: int, R: int, strata=None, nstrata: int = 0) -> np.ndarray:
    """tpg_mantel_perms: rows r0 .. r0 + R - 1 of the permutation list in one call -> (R, n) int32; row r = 0 is the identity;
    strata (n, 0-based ids below nstrata): nobody leaves a stratum.  Host only."""
    st = _i32(strata)
    if st is not None and st.shape != (n,):
        raise ValueError("strata must have one entry per individual")
    out = np.zeros((max(int(R), 0), max(int(n), 0)), dtype=np.int32)
    check(lib.tpg_mantel_perms(int(n), _ptr(st), int(nstrata), int(seed) & 0xFFFFFFFFFFFFFFFF, int(r0), int(R), _ptr(out)))
    return out


def mantel_from_sums(N: int, Sa: float, Saa: float, Sb: float, Sbb: float, Sab: float) -> float:
    """tpg_mantel_from_sums: the correlation from the number of pairs, the moments of both matrices and the cross sum.  Host only."""
    out = np.zeros(1)
    check(lib.tpg_mantel_from_sums(int(N), float(Sa), float(Saa), float(Sb), float(Sbb), float(Sab), _ptr(out)))
    return float(out[0])


def mantel_partial(r_ab: float, r_ac: float, r_bc: float) -> float:
    """tpg_mantel_partial: the partial correlation of a and b given c.  Host only."""
    return float(lib.tpg_mantel_partial(float(r_ab), float(r_ac), float(r_bc)))


def great_circle_dist(lon, lat, radius_km: float = 6371.0088) -> np.ndarray:
    """Haversine distances in km between points given by longitude and latitude in degrees -> n x n, symmetric, zero diagonal.
    numpy on the host, not a device kernel: its bits are numpy's."""
    lon, lat = np.radians(np.asarray(lon, dtype=np.float64)), np.radians(np.asarray(lat, dtype=np.float64))
    if lon.ndim != 1 or lon.shape != lat.shape:
        raise ValueError("lon and lat must be vectors of one length")
    sdlat = np.sin((lat[:, None] - lat[None, :]) / 2.0)
    sdlon = np.sin((lon[:, None] - lon[None, :]) / 2.0)
    h = sdlat * sdlat + np.cos(lat)[:, None] * np.cos(lat)[None, :] * (sdlon * sdlon)
    d = 2.0 * radius_km * np.arcsin(np.sqrt(np.minimum(h, 1.0)))
    d = np.maximum(d, d.T)  # (h is symmetric up to the order of the two cosines: make it so)
    np.fill_diagonal(d, 0.0)
    return np.asfortranarray(d)


def offdiag_midranks(M) -> np.ndarray:
    """Spearman's transform of a symmetric matrix: the entries of the strict lower triangle replaced by their mid-ranks (1-based,
    ties share the mean of their ranks), mirrored; the diagonal +0.0.  numpy on the host."""
    M = np.asarray(M, dtype=np.float64)
    n = M.shape[0]
    il = np.tril_indices(n, -1)
    x = M[il]
    if not np.array_equal(x, M.T[il], equal_nan=True):
        raise ValueError("method='spearman' needs symmetric matrices")
    order = np.argsort(x, kind="stable")
    xs = x[order]
    first = np.concatenate(([True], xs[1:] != xs[:-1])) if len(xs) else np.zeros(0, dtype=bool)
    start = np.flatnonzero(first)
    count = np.diff(np.append(start, len(xs)))
    mid = start + (count + 1) / 2.0  # ranks start + 1 .. start + count: their mean
    ranks = np.empty(len(xs))
    ranks[order] = np.repeat(mid, count)
    ranks[np.isnan(x)] = np.nan
    out = np.zeros((n, n), order="F")
    out[il] = ranks
    out.T[il] = ranks
    return out


def _mantel_r(N, Sa, Saa, Sb, Sbb, Sab):
    """tpg_mantel_from_sums statement for statement on a vector of cross sums"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        Nd = np.float64(N)
        mab = np.float64(Sa) * np.float64(Sb)
        cab = np.asarray(Sab, dtype=np.float64) - mab / Nd
        maa = np.float64(Sa) * np.float64(Sa)
        va = np.float64(Saa) - maa / Nd
        mbb = np.float64(Sb) * np.float64(Sb)
        vb = np.float64(Sbb) - mbb / Nd
        if N < 1 or not (va > 0.0) or not (vb > 0.0):
            return np.full(np.shape(cab), np.nan)
        den = np.sqrt(va * vb)
        return cab / den


def _mantel_partial_r(r_ab, r_ac, r_bc):
    """tpg_mantel_partial statement for statement on vectors r_ab, r_ac"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        fa = 1.0 - r_ac * r_ac
        fb = np.float64(1.0) - np.float64(r_bc) * np.float64(r_bc)
        num = r_ab - r_ac * np.float64(r_bc)
        den = np.sqrt(fa * fb)
        return np.where((fa > 0.0) & (fb > 0.0), num / den, np.nan)


def gt_mantel(X: Optional[FBM] = None, ind_row=None, ind_col=None, dist=None, dist_type: str = "raw", y=None, z=None, coords=None,
              method: str = "pearson", strata=None, n_perm: int = 999, seed: int = 0, return_perm: bool = False) -> dict:
    """Mantel test of isolation by distance (no counterpart in the reference; include/tpg.h "Mantel tests"): the correlation of
    the genetic distances A -- from X by one pairwise pass (dist_type "raw" or "adjusted"), kept in HBM, or dist (n x n matrix
    or DeviceMatrix) -- with y (n x n) or the great-circle distances of coords = (lon, lat), tested by n_perm permutations of
    the individuals of A (inside strata, 0-based ids, when given).  z (n x n): the partial test of A and y given z.  method
    "spearman" replaces the entries of every matrix by mid-ranks on the host first (symmetric matrices only).  Population level:
    gt_mantel(dist=F / (1 - F), y=np.log(geo)) with F the fst_tot matrix of pairwise_pop_fst.
    -> dict(statistic, p_value (one-sided, permuted >= observed), n_valid, n_perm), for the partial test also r_ab, r_ac, r_bc;
    with return_perm also perm (n_perm,) the permuted statistics."""
    if method not in ("pearson", "spearman"):
        raise ValueError("method must be 'pearson' or 'spearman'")
    if n_perm < 1:
        raise ValueError("n_perm must be positive")
    if (X is None) == (dist is None):
        raise ValueError("give either X or dist")
    if (y is None) == (coords is None):
        raise ValueError("give either y or coords")
    A = pairwise_sqdist(X, ind_row, ind_col, dist_type, device=True) if dist is None else dist
    ctx = A.ctx if isinstance(A, DeviceMatrix) else (X.ctx if X is not None else default_context())
    n = A.n if isinstance(A, DeviceMatrix) else np.shape(A)[0]
    mats = [A, great_circle_dist(*coords) if y is None else y] + ([z] if z is not None else [])
    ours = [dist is None, False, False]  # a DeviceMatrix of the caller's is centred into a new one, never in place
    for k, M in enumerate(mats):
        if not isinstance(M, DeviceMatrix):
            M = np.asfortranarray(M, dtype=np.float64)
            if M.shape != (n, n):
                raise ValueError("every matrix must be n x n")
        elif M.n != n:
            raise ValueError("every matrix must be n x n")
        if method == "spearman":
            M = offdiag_midranks(M.to_numpy() if isinstance(M, DeviceMatrix) else M)
        if not isinstance(M, DeviceMatrix):
            M, ours[k] = DeviceMatrix.from_numpy(M, ctx), True
        mats[k] = M
    N = n * (n - 1)
    mom = []
    for k, M in enumerate(mats):  # centre by S / N, then the moments of what the cross sums see
        S, _ = offdiag_moments(M)
        mean = S / np.float64(N) if N > 0 else 0.0
        mats[k] = offdiag_center(M, mean, out=M if ours[k] else None)
        mom.append(offdiag_moments(mats[k]))
    st = _i32(strata)
    perms = mantel_perms(n, seed, 0, n_perm + 1, st, 0 if st is None else (int(st.max()) + 1 if len(st) else 0))
    sums = mantel_sums(mats[0], mats[1:], perms)
    if np.isnan(sums[0]).any() or np.isnan(np.array(mom)).any():
        raise _lib.TpgError(4, "gt_mantel: a matrix holds a missing value off its diagonal")  # TPG_ENUMERIC
    (Sa, Saa), (Sb, Sbb) = mom[0], mom[1]
    r_ab = _mantel_r(N, Sa, Saa, Sb, Sbb, sums[:, 0])
    out = {}
    if z is None:
        stat = r_ab
    else:
        Sc, Scc = mom[2]
        r_ac = _mantel_r(N, Sa, Saa, Sc, Scc, sums[:, 1])
        Sbc = mantel_sums(mats[1], [mats[2]], perms[:1])[0, 0]
        r_bc = mantel_from_sums(N, Sb, Sbb, Sc, Scc, Sbc)
        stat = _mantel_partial_r(r_ab, r_ac, r_bc)
        out.update(r_ab=float(r_ab[0]), r_ac=float(r_ac[0]), r_bc=r_bc)
    p, nv = fst_perm_pvalue(stat[:1], stat[1:].reshape(-1, 1))
    out.update(statistic=float(stat[0]), p_value=float(p[0]), n_valid=int(nv[0]), n_perm=int(n_perm))
    if return_perm:
        out["perm"] = stat[1:].copy()
    return out


def windows_nwise_pop_pbs(X: FBM, ind_row, ind_col, groupIds, ngroups: int, chromosome, position=None, ploidy=None,
                          fst_method: str = "Hudson", return_fst: bool = False, window_size=None, step_size=None, size_unit="snp",
                          min_loci=1, complete=False, triplets=None):
    """R/windows_nwise_pop_pbs.R:55-126, type = "matrix": the population branch statistic of every triplet of populations
    from windowed pairwise Fst.  fst_method is validated as nwise_pop_pbs validates it, but the windows are Hudson's: the
    reference's windows_pairwise_pop_fst sets method = "Hudson" whatever it is given (R/windows_pairwise_pop_fst.R:62-65),
    and that behaviour is kept.  The nw x P window Fst is written to device memory by the fused window scan and read there by
    the PBS kernel.  triplets (not in the reference): a list of 1-based (a, b, c) with a < b < c restricts the output to them.
    -> dict(chromosome, start, end, pbs (nw, 6 * n_triplets), names, [fst (nw, P)]), columns and names as nwise_pop_pbs."""
    if ngroups < 3:
        raise ValueError("At least 3 populations are required to compute PBS.")
    if not isinstance(return_fst, (bool, np.bool_)):
        raise ValueError("return_fst must be a logical value (TRUE or FALSE)")
    if fst_method not in FST_METHODS:
        raise ValueError("'arg' should be one of 'Hudson', 'Nei87', 'WC84'")
    trips, tcols = _pbs_triplets(ngroups)
    if triplets is not None:
        col = {t: k for k, t in enumerate(trips)}
        want = []
        for t in triplets:
            t = tuple(t)
            if len(t) != 3 or any(not isinstance(x, (int, np.integer)) for x in t) or not 1 <= t[0] < t[1] < t[2] <= ngroups:
                raise ValueError(f"a triplet must be three 1-based populations (a, b, c) with a < b < c <= {ngroups}, not {t!r}")
            want.append(tuple(int(x) for x in t))
        if not want:
            raise ValueError("triplets must name at least one triplet")
        tcols = np.ascontiguousarray(tcols[[col[t] for t in want]])
        trips = want
    v = View(X, ind_row, ind_col)
    if len(chromosome) != v.m:
        raise ValueError("loci_table must have the same number of rows as x.")
    wr = window_index_ranges(chromosome, position, window_size, step_size, size_unit, complete)
    if min_loci <= 0:
        raise ValueError("min_loci must be positive.")
    if min_loci > window_size:
        raise ValueError("min_loci must be less than window_size.")
    pairs_c = np.ascontiguousarray(combn2(ngroups).T)
    P = pairs_c.shape[0]
    gid, pl = _i32(groupIds), _ploidy(v, ploidy)
    lo, hi, pad = _window_args(wr["lo"], wr["hi"], wr["pad_na"])
    nw = len(lo)
    ctx = v.ctx
    res = dict(chromosome=wr["chromosome"], start=wr["start"], end=wr["end"])
    out = np.zeros((nw, 6 * len(trips)), order="F")
    f = np.zeros((nw, P), order="F") if return_fst else None
    if nw > 0:
        d_fst = ctx.dev_alloc(8 * nw * P)
        try:
            check(lib.tpg_windows_pairwise_pop_fst(ctx.h, v.h, _ptr(gid), int(ngroups), _ptr(pl), FST_METHODS["Hudson"],
                                                   _ptr(pairs_c), P, _ptr(lo), _ptr(hi), _ptr(pad), nw, int(min_loci), d_fst,
                                                   None, None, None, None))
            check(lib.tpg_pbs_from_fst(ctx.h, d_fst, nw, P, _ptr(tcols), len(trips), _ptr(out)))
            if return_fst:
                check(lib.tpg_dev_to_host(ctx.h, _ptr(f), d_fst, f.nbytes))
        finally:
            ctx.dev_free(d_fst)
    res["pbs"] = out
    if return_fst:
        res["fst"] = f
    res["names"] = _pbs_names(trips)
    return res


# include/tpg.h "Tajima's D": loci per partial sum of pop_tajimas_d (results do not depend on it)
TAJIMA_CHUNK_LOCI = int(lib.tpg_tajima_chunk_loci()) if hasattr(lib, "tpg_tajima_chunk_loci") else 0


def tajimas_d_from_sums(n_alleles: int, seg: int, k_hat: float) -> float:
    """R/pop_tajimas_d.R:151-166 from its additive pieces (tpg_tajimas_d_from_sums; host arithmetic, no device): seg and
    k_hat of shards or blocks of loci add up, D of the sums is D of the whole."""
    d = C.c_double()
    check(lib.tpg_tajimas_d_from_sums(int(n_alleles), int(seg), float(k_hat), C.byref(d)))
    return d.value


def _tajima_groups(v: View, groupIds, ngroups):
    if groupIds is None:
        return None, 1
    gid = _i32(groupIds)
    if len(gid) != v.n:
        raise ValueError("groupIds must have one entry per individual of ind_row")
    return gid, int(ngroups)


def pop_tajimas_d(X: FBM, ind_row=None, ind_col=None, groupIds=None, ngroups: int = 0, ploidy=None, return_sums: bool = False):
    """R/pop_tajimas_d.R:51-148 (include/tpg.h "Tajima's D"): ungrouped (groupIds=None) a float, NaN where the reference gives
    NA (a single individual: no device call); grouped an array of ngroups values.  return_sums: dict(tajimas_d, seg, k_hat)."""
    n = X.nrow if ind_row is None else len(ind_row)
    if groupIds is None and n <= 1:  # R/pop_tajimas_d.R:91-95
        if ploidy is not None and np.any(_f64(ploidy) != 2.0):
            raise _lib.TpgError(1, "Tajima's D only works on diploid data")  # TPG_EINVAL, as the library answers
        return dict(tajimas_d=np.nan, seg=0, k_hat=np.nan) if return_sums else np.nan
    v = View(X, ind_row, ind_col)
    gid, G = _tajima_groups(v, groupIds, ngroups)
    pl = _f64(ploidy)
    d, seg, k = np.zeros(G), np.zeros(G, dtype=np.int64), np.zeros(G)
    check(lib.tpg_pop_tajimas_d(v.ctx.h, v.h, _ptr(gid), G, _ptr(pl), _ptr(d), _ptr(seg), _ptr(k)))
    if groupIds is None:
        return dict(tajimas_d=float(d[0]), seg=int(seg[0]), k_hat=float(k[0])) if return_sums else float(d[0])
    return dict(tajimas_d=d, seg=seg, k_hat=k) if return_sums else d


def tajima_windows(v: View, groupIds, ngroups, lo, hi, pad_na=None, min_loci: int = 1, ploidy=None) -> dict:
    """tpg_windows_pop_tajimas_d on explicit 0-based half-open locus ranges -> dict(tajimas_d, seg, k_hat, n_loci), each
    (nw, G); n_loci is int32 with -1 on a pad_na window"""
    gid, G = _tajima_groups(v, groupIds, ngroups)
    lo, hi = np.ascontiguousarray(lo, dtype=np.int64), np.ascontiguousarray(hi, dtype=np.int64)
    pad = None if pad_na is None else np.ascontiguousarray(pad_na, dtype=np.uint8)
    nw = len(lo)
    if len(hi) != nw or (pad is not None and len(pad) != nw):
        raise ValueError("lo, hi and pad_na must have one entry per window")
    pl = _f64(ploidy)
    d, k = np.zeros((nw, G), order="F"), np.zeros((nw, G), order="F")
    seg, nl = np.zeros((nw, G), dtype=np.int64, order="F"), np.zeros((nw, G), dtype=np.int32, order="F")
    check(lib.tpg_windows_pop_tajimas_d(v.ctx.h, v.h, _ptr(gid), G, _ptr(pl), _ptr(lo), _ptr(hi), _ptr(pad),
                                        nw, int(min_loci), _ptr(d), _ptr(seg), _ptr(k), _ptr(nl)))
    return dict(tajimas_d=d, seg=seg, k_hat=k, n_loci=nl)


def windows_pop_tajimas_d(X: FBM, ind_row, ind_col, groupIds, ngroups: int, chromosome, position=None, ploidy=None,
                          window_size=None, step_size=None, size_unit="snp", min_loci=1, complete=False,
                          return_sums: bool = False):
    """R/windows_pop_tajimas_d.R:58-122 (type = "matrix"): the reference's runner call with a custom function per window and
    group, as one segmented reduction behind the count sweep; pi (m x G) stays in HBM.  groupIds=None: one group.
    -> dict(chromosome, start, end, n_loci (nw, G; NaN on a pad window), tajimas_d (nw, G)); return_sums adds seg, k_hat."""
    v = View(X, ind_row, ind_col)
    if len(chromosome) != v.m:
        raise ValueError("loci_table must have the same number of rows as x.")
    wr = window_index_ranges(chromosome, position, window_size, step_size, size_unit, complete)
    if min_loci <= 0:
        raise ValueError("min_loci must be positive.")
    if min_loci > window_size:
        raise ValueError("min_loci must be less than window_size.")
    r = tajima_windows(v, groupIds, ngroups, wr["lo"], wr["hi"], wr["pad_na"], min_loci, ploidy)
    n_loci = r["n_loci"].astype(float)
    n_loci[r["n_loci"] < 0] = np.nan
    out = dict(chromosome=wr["chromosome"], start=wr["start"], end=wr["end"], n_loci=n_loci, tajimas_d=r["tajimas_d"])
    if return_sums:
        out.update(seg=r["seg"], k_hat=r["k_hat"])
    return out


# include/tpg.h "f2 blocks": loci a workgroup stages at a time (results do not depend on it)
F2_CHUNK_LOCI = int(lib.tpg_f2_chunk_loci()) if hasattr(lib, "tpg_f2_chunk_loci") else 0
F2_POLY = {"f2": 1, "ap": 2}  # TPG_F2_POLY_F2, TPG_F2_POLY_AP


def f2_block_ranges(chromosome, dist, blgsize=0.05):
    """Jackknife blocks of admixtools (get_block_lengths, recalled) as 0-based half-open locus ranges (lo, hi): locus j starts a
    new block when its chromosome differs from the previous locus's or when dist[j] - dist[first locus of the block] >= blgsize.
    dist is the genetic distance in Morgans, or positions in bp when blgsize >= 100.  dist must not decrease within a
    chromosome and a chromosome must not reappear: ValueError."""
    chrom = np.asarray(chromosome)
    d = np.asarray(dist, dtype=np.float64)
    if chrom.ndim != 1 or d.shape != chrom.shape:
        raise ValueError("chromosome and dist must be vectors of one length")
    if not blgsize > 0:
        raise ValueError("blgsize must be positive")
    if np.isnan(d).any():
        raise ValueError("dist has missing values")
    m = len(chrom)
    if m == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    new_chrom = np.r_[True, chrom[1:] != chrom[:-1]]
    starts_c = np.flatnonzero(new_chrom)
    labels = chrom[starts_c].tolist()
    if len(set(labels)) != len(labels):
        raise ValueError("a chromosome reappears: the loci must be sorted by chromosome")
    if np.any((np.diff(d) < 0) & ~new_chrom[1:]):
        raise ValueError("dist must be sorted within each chromosome")
    lo = []
    for a, b in zip(starts_c, np.r_[starts_c[1:], m]):
        j = int(a)
        while j < b:  # one binary search per block
            lo.append(j)
            j += int(np.searchsorted(d[j:b] - d[j] >= blgsize, True))
    lo = np.asarray(lo, dtype=np.int64)
    return lo, np.r_[lo[1:], m].astype(np.int64)


def _f2_params(maxmiss, minmaf, maxmaf, minac2, poly_only, apply_corr, keep, m):
    if minac2 not in (0, 1, False, True):
        raise ValueError("minac2 must be FALSE / TRUE (0 / 1): admixtools' experimental minac2 = 2 is not supported")
    if isinstance(poly_only, (bool, np.bool_)):
        bits = 3 if poly_only else 0
    elif isinstance(poly_only, (int, np.integer)):
        bits = int(poly_only)
    else:
        names = [poly_only] if isinstance(poly_only, str) else list(poly_only)
        bad = [s for s in names if s not in F2_POLY]
        if bad:
            raise ValueError(f"poly_only: {bad} not supported (only 'f2' and 'ap'; fst is out of scope)")
        bits = sum({F2_POLY[s] for s in names})
    if not 0 <= bits <= 3:
        raise ValueError("poly_only out of range")
    pr = _lib.F2Params()
    check(lib.tpg_f2_params_default(C.byref(pr)))
    pr.maxmiss, pr.minmaf, pr.maxmaf = float(maxmiss), float(minmaf), float(maxmaf)
    pr.minac2, pr.poly_only, pr.apply_corr = int(minac2), bits, int(bool(apply_corr))
    keep_arr = None
    if keep is not None and not isinstance(keep, (int, np.integer)):
        keep_arr = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
        if keep_arr.shape != (m,):
            raise ValueError("keep must have one entry per locus of the view")
        pr.keep = keep_arr.ctypes.data
    elif keep is not None:
        pr.keep = int(keep)  # a device pointer
    return pr, keep_arr


def f2_blocks(v: View, groupIds, ngroups, lo, hi, ploidy=None, maxmiss=0.0, minmaf=0.0, maxmaf=0.5, minac2=False,
              poly_only=("f2",), apply_corr=True, keep=None, afprod=True, on_device=False) -> dict:
    """tpg_f2_blocks (include/tpg.h "f2 blocks") on explicit 0-based half-open locus ranges -> dict(f2, counts, ap, ap_counts:
    (G, G, nb) each, ap / ap_counts only with afprod; block_lengths: int64[nb], the kept loci).  groupIds=None: one group.
    on_device=True: the four arrays stay in HBM and come back as raw device pointers (release with v.ctx.dev_free);
    block_lengths is a host array all the same."""
    if groupIds is None:
        gid, G = None, 1
    else:
        gid, G = _i32(groupIds), int(ngroups)
        if len(gid) != v.n:
            raise ValueError("groupIds must have one entry per individual of ind_row")
    lo, hi = np.ascontiguousarray(lo, dtype=np.int64), np.ascontiguousarray(hi, dtype=np.int64)
    nb = len(lo)
    if lo.ndim != 1 or hi.shape != lo.shape:
        raise ValueError("lo and hi must have one entry per block")
    pr, keep_arr = _f2_params(maxmiss, minmaf, maxmaf, minac2, poly_only, apply_corr, keep, v.m)
    pl = _f64(ploidy)
    if pl is not None and len(pl) != v.n:
        raise ValueError("ploidy must have one entry per individual of ind_row")
    nk = np.zeros(nb, dtype=np.int64)
    names = ("f2", "counts") + (("ap", "ap_counts") if afprod else ())
    dtypes = dict(f2=np.float64, counts=np.int32, ap=np.float64, ap_counts=np.int32)
    cells = max(G, 1) * max(G, 1) * nb
    out, ptrs = {}, {}
    try:
        for k in names:
            if on_device:
                out[k] = v.ctx.dev_alloc(max(cells, 1) * np.dtype(dtypes[k]).itemsize)
                ptrs[k] = out[k]
            else:
                out[k] = np.zeros((G, G, nb), dtype=dtypes[k], order="F")
                ptrs[k] = _ptr(out[k])
        check(lib.tpg_f2_blocks(v.ctx.h, v.h, _ptr(gid), G, _ptr(pl), C.byref(pr), _ptr(lo), _ptr(hi), nb,
                                ptrs["f2"], ptrs["counts"], ptrs.get("ap"), ptrs.get("ap_counts"),
                                _ptr(nk)))
    except Exception:
        if on_device:
            for p in out.values():
                v.ctx.dev_free(p)
        raise
    del keep_arr  # alive until here: pr.keep points into it
    out["block_lengths"] = nk
    return out


def gt_extract_f2(X: FBM, ind_row, ind_col, groupIds, ngroups: int, chromosome, genetic_dist=None, position=None, blgsize=0.05,
                  maxmiss=0, minmaf=0, maxmaf=0.5, minac2=False, poly_only=("f2",), apply_corr=True, afprod=True, keep=None,
                  ploidy=None, **unsupported):
    """R/gt_extract_f2.R:86-193 without the directory of .rds files: gt_to_aftable, admixtools' discard_from_aftable and
    afs_to_f2_blocks as one device call; the m x 2G table never leaves HBM.  Blocks come from f2_block_ranges(chromosome,
    genetic_dist, blgsize), or from position when blgsize >= 100 (bp).  -> dict(f2, counts, ap, ap_counts (G, G, nb),
    block_lengths, lo, hi).  fst=, outpop / outpop_scale, transitions / transversions (locus-table filters: pass `keep`), outdir
    and minac2 = 2 are out of scope: an unsupported argument raises."""
    if unsupported:
        raise TypeError(f"gt_extract_f2: unsupported argument(s) {sorted(unsupported)}")
    v = View(X, ind_row, ind_col)
    if len(chromosome) != v.m:
        raise ValueError("chromosome must have one entry per locus of ind_col")
    dist = position if blgsize >= 100 else genetic_dist
    if dist is None:
        raise ValueError("blgsize >= 100 is in bp and needs position; smaller values are in Morgans and need genetic_dist")
    lo, hi = f2_block_ranges(chromosome, dist, blgsize)
    out = f2_blocks(v, groupIds, ngroups, lo, hi, ploidy, maxmiss, minmaf, maxmaf, minac2, poly_only, apply_corr, keep, afprod)
    out.update(lo=lo, hi=hi)
    return out


def f4_from_f2_blocks(f2, block_lengths, quads) -> dict:
    """f4(A, B; C, D) per row of quads (0-based group indices) with the weighted block jackknife (tpg_f4_jackknife: host
    arithmetic, no device) -> dict(est, se, z = est / se, n_blocks)"""
    f2 = np.asfortranarray(f2, dtype=np.float64)
    if f2.ndim != 3 or f2.shape[0] != f2.shape[1]:
        raise ValueError("f2 must be G x G x n_blocks")
    G, nb = f2.shape[0], f2.shape[2]
    bl = np.ascontiguousarray(block_lengths, dtype=np.int64)
    if bl.shape != (nb,):
        raise ValueError("block_lengths must have one entry per block")
    q = np.ascontiguousarray(np.asarray(quads, dtype=np.int32).reshape(-1, 4))
    nq = len(q)
    est, se, used = np.zeros(nq), np.zeros(nq), np.zeros(nq, dtype=np.int32)
    check(lib.tpg_f4_jackknife(_ptr(f2), G, nb, _ptr(bl), _ptr(q), nq, _ptr(est), _ptr(se), _ptr(used)))
    with np.errstate(invalid="ignore", divide="ignore"):
        z = est / se
    return dict(est=est, se=se, z=z, n_blocks=used)


def f3_from_f2_blocks(f2, block_lengths, triples) -> dict:
    """f3(C; A, B) per row (C, A, B) of triples: the quadruple (C, A; C, B) of f4_from_f2_blocks (the diagonal of f2 is +0.0)"""
    t = np.asarray(triples, dtype=np.int32).reshape(-1, 3)
    return f4_from_f2_blocks(f2, block_lengths, np.stack([t[:, 0], t[:, 1], t[:, 0], t[:, 2]], axis=1))


# include/tpg.h "site frequency spectra": loci staged at a time (results do not depend on it) and the widest operand
SFS_CHUNK_LOCI = int(lib.tpg_sfs_chunk_loci()) if hasattr(lib, "tpg_sfs_chunk_loci") else 0
SFS_MAX_WIDTH = 4096  # TPG_SFS_MAX_WIDTH


def sfs_segments(block_len: int, W: int) -> int:
    """tpg_sfs_segments: the partial sums a block of block_len loci is cut into at width W (-1: a bad size)"""
    return int(lib.tpg_sfs_segments(int(block_len), int(W)))


def sfs_scratch_bytes(m: int, ngroups: int, W: int, nb: int, joint: bool = True) -> int:
    """tpg_sfs_scratch_bytes: the device scratch of one sfs_blocks call (-1: a bad size)"""
    return int(lib.tpg_sfs_scratch_bytes(int(m), int(ngroups), int(W), int(nb), int(bool(joint))))


def sfs_project_row(x: int, v: int, n: int) -> np.ndarray:
    """tpg_sfs_project_row (host arithmetic, no device): the hypergeometric weights h[0 .. n] of x counted alleles among v typed
    ones projected to n, by the routine the device runs (csrc/host/host_sfs.h)"""
    h = np.full(max(int(n), 0) + 1, np.nan)
    check(lib.tpg_sfs_project_row(int(x), int(v), int(n), _ptr(h)))
    return h


def _sfs_mask(x, m, name):
    if x is None or isinstance(x, (int, np.integer)):
        return x  # nothing, or a device pointer
    a = np.ascontiguousarray(np.asarray(x) != 0, dtype=np.uint8)
    if a.shape != (m,):
        raise ValueError(f"{name} must have one entry per locus of the view")
    return a


def sfs_blocks(v: View, groupIds, ngroups, lo, hi, proj=None, keep=None, flip=None, joint=True, ploidy=None) -> dict:
    """tpg_sfs_blocks (include/tpg.h "site frequency spectra") on explicit 0-based half-open locus ranges -> dict(sfs (W, nb),
    n_used1 (G, nb), and with joint jsfs (W, W, nb), n_used2 (G, G, nb); n (G): the projection sizes, offsets (G + 1): o_g and
    W).  groupIds=None: one group.  proj: n_g per group, 0 or None = the group's 2 N_g."""
    if groupIds is None:
        gid, G = None, 1
        sizes = np.array([v.n], dtype=np.int64)
    else:
        gid, G = _i32(groupIds), int(ngroups)
        if len(gid) != v.n:
            raise ValueError("groupIds must have one entry per individual of ind_row")
        ok = (gid >= 0) & (gid < max(G, 1))
        sizes = np.bincount(gid[ok], minlength=max(G, 1))[:max(G, 1)].astype(np.int64)
    pj = None if proj is None else np.ascontiguousarray(np.broadcast_to(np.asarray(proj, dtype=np.int32), (max(G, 1),)))
    n = 2 * sizes if pj is None else np.where(pj == 0, 2 * sizes, pj.astype(np.int64))
    offsets = np.r_[0, np.cumsum(np.maximum(n, 0) + 1)].astype(np.int64)
    W = int(min(offsets[-1], SFS_MAX_WIDTH))  # (a wider request is refused by the library before it writes anything)
    lo, hi = np.ascontiguousarray(lo, dtype=np.int64), np.ascontiguousarray(hi, dtype=np.int64)
    nb = len(lo)
    if lo.ndim != 1 or hi.shape != lo.shape:
        raise ValueError("lo and hi must have one entry per block")
    kp, fl = _sfs_mask(keep, v.m, "keep"), _sfs_mask(flip, v.m, "flip")
    pl = _f64(ploidy)
    if pl is not None and len(pl) != v.n:
        raise ValueError("ploidy must have one entry per individual of ind_row")
    Gd = max(G, 1)
    out = dict(sfs=np.zeros((W, nb), order="F"), n_used1=np.zeros((Gd, nb), dtype=np.int64, order="F"))
    if joint:
        out.update(jsfs=np.zeros((W, W, nb), order="F"), n_used2=np.zeros((Gd, Gd, nb), dtype=np.int64, order="F"))
    check(lib.tpg_sfs_blocks(v.ctx.h, v.h, _ptr(gid), G, _ptr(pl), _ptr(pj), _ptr(kp), _ptr(fl), _ptr(lo), _ptr(hi), nb,
                             _ptr(out["sfs"]), _ptr(out["n_used1"]), _ptr(out.get("jsfs")), _ptr(out.get("n_used2"))))
    out.update(n=n.astype(np.int64), offsets=offsets)
    return out


def sfs_fold(sfs) -> np.ndarray:
    """Fold a 1-D spectrum of n + 1 entries (host): folded[k] = sfs[k] + sfs[n - k] for k < n / 2, the middle entry (n even)
    stays once, the entries above are 0"""
    s = np.asarray(sfs, dtype=np.float64)
    if s.ndim != 1 or len(s) < 2:
        raise ValueError("sfs must be a vector of n + 1 >= 2 entries")
    n = len(s) - 1
    out = np.zeros_like(s)
    for k in range(n // 2 + 1):
        out[k] = s[k] + s[n - k] if 2 * k < n else s[k]
    return out


def jsfs_fold(J) -> np.ndarray:
    """Fold a joint spectrum (n1 + 1) x (n2 + 1) (host; dadi's convention, recalled): an entry with a + c > (n1 + n2) / 2 is
    added to (n1 - a, n2 - c) and set to 0; the entries on the line a + c = (n1 + n2) / 2 become the mean of the two mirror
    cells"""
    J = np.asarray(J, dtype=np.float64)
    if J.ndim != 2 or min(J.shape) < 2:
        raise ValueError("J must be (n1 + 1) x (n2 + 1)")
    n1, n2 = J.shape[0] - 1, J.shape[1] - 1
    a, c = np.meshgrid(np.arange(n1 + 1), np.arange(n2 + 1), indexing="ij")
    mirror = J[::-1, ::-1]
    tot2 = 2 * (a + c)
    return np.where(tot2 < n1 + n2, J + mirror, np.where(tot2 == n1 + n2, (J + mirror) / 2.0, 0.0))


def sfs_stats(sfs) -> dict:
    """Summary statistics of a real-valued unfolded spectrum of n + 1 entries (host, plain double, every sum in ascending k in
    the order written): S = sum_{0<k<n} sfs[k], theta_w = S / a1, theta_pi = sum k (n - k) sfs[k] / C(n, 2), theta_h =
    sum k^2 sfs[k] / C(n, 2), fay_wu_h = theta_pi - theta_h, tajimas_d with the constants of the Tajima section of include/tpg.h"""
    s = np.asarray(sfs, dtype=np.float64)
    if s.ndim != 1 or len(s) < 3:
        raise ValueError("sfs must be a vector of n + 1 >= 3 entries")
    n = len(s) - 1
    S = pi = th = 0.0
    for k in range(1, n):
        x = float(s[k])
        S = S + x
        pi = pi + float(k * (n - k)) * x
        th = th + float(k * k) * x
    c2 = float(n * (n - 1) // 2)
    a1 = a2 = 0.0
    for i in range(1, n):
        a1 += 1.0 / float(i)
        a2 += 1.0 / (float(i) * float(i))
    nd = float(n)
    e1 = ((nd + 1) / (3 * (nd - 1)) - 1 / a1) / a1
    e2 = (2 * (nd * nd + nd + 3) / (9 * nd * (nd - 1)) - (nd + 2) / (nd * a1) + a2 / (a1 * a1)) / (a1 * a1 + a2)
    theta_pi, theta_h = pi / c2, th / c2
    with np.errstate(invalid="ignore", divide="ignore"):
        d = (np.float64(theta_pi) - np.float64(S) / a1) / np.sqrt(np.float64(e1 * S + e2 * S * (S - 1)))
    return dict(n=n, S=S, theta_w=S / a1, theta_pi=theta_pi, theta_h=theta_h, fay_wu_h=theta_pi - theta_h, tajimas_d=float(d))


def _sfs_cut(r, G):
    return [[r["sfs"][r["offsets"][g]:r["offsets"][g + 1], b] for g in range(G)] for b in range(r["sfs"].shape[1])]


def pop_sfs(X: FBM, ind_row=None, ind_col=None, groupIds=None, ngroups: int = 0, proj=None, flip=None, keep=None,
            folded: bool = False, ploidy=None) -> dict:
    """The site frequency spectrum of every group over the whole view, projected to proj[g] alleles (None or 0: the group's
    2 N_g; loci typed at fewer alleles are left out of that group).  flip marks the loci whose REFERENCE allele is the derived
    one.  -> dict(sfs: one vector of n_g + 1 entries per group, n_used: loci used per group, n: the projection sizes)"""
    v = View(X, ind_row, ind_col)
    G = 1 if groupIds is None else int(ngroups)
    r = sfs_blocks(v, groupIds, ngroups, [0], [v.m], proj, keep, flip, joint=False, ploidy=ploidy)
    spectra = _sfs_cut(r, G)[0]
    if folded:
        spectra = [sfs_fold(s) for s in spectra]
    return dict(sfs=[np.array(s) for s in spectra], n_used=r["n_used1"][:, 0].copy(), n=r["n"])


def sfs_block_ranges(chromosome, block_size: int):
    """Bootstrap blocks of block_size consecutive loci that do not cross a chromosome border, as 0-based half-open (lo, hi)"""
    chrom = np.asarray(chromosome)
    if chrom.ndim != 1 or int(block_size) < 1:
        raise ValueError("chromosome must be a vector and block_size positive")
    m, bs = len(chrom), int(block_size)
    starts = np.flatnonzero(np.r_[True, chrom[1:] != chrom[:-1]]) if m else np.zeros(0, dtype=np.int64)
    lo, hi = [], []
    for a, b in zip(starts, np.r_[starts[1:], m]):
        for s in range(int(a), int(b), bs):
            lo.append(s)
            hi.append(min(s + bs, int(b)))
    return np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)


def pairwise_pop_jsfs(X: FBM, ind_row, ind_col, groupIds, ngroups: int, proj=None, flip=None, keep=None, folded: bool = False,
                      blocks=None, chromosome=None, block_size=None, ploidy=None) -> dict:
    """The joint site frequency spectrum of every pair of groups g1 < g2 (combn2 order) over the loci usable in both, each
    projected to its proj[g].  -> dict(pairs (2 x P, 1-based), jsfs: one (n_g1 + 1) x (n_g2 + 1) array per pair, n_used: loci
    per pair, n).  With blocks=(lo, hi), or chromosome and block_size (sfs_block_ranges), the arrays are per block -- (n_g1 + 1)
    x (n_g2 + 1) x nb and n_used (P, nb), with lo and hi -- for a block bootstrap."""
    v = View(X, ind_row, ind_col)
    G = int(ngroups)
    per_block = blocks is not None or chromosome is not None
    if blocks is not None:
        lo, hi = blocks
    elif chromosome is not None:
        if block_size is None or len(chromosome) != v.m:
            raise ValueError("chromosome needs one entry per locus of ind_col and a block_size")
        lo, hi = sfs_block_ranges(chromosome, block_size)
    else:
        lo, hi = [0], [v.m]
    r = sfs_blocks(v, groupIds, G, lo, hi, proj, keep, flip, joint=True, ploidy=ploidy)
    o, pairs = r["offsets"], combn2(G)
    js, used = [], []
    for a, b in pairs.T - 1:
        J = r["jsfs"][o[a]:o[a + 1], o[b]:o[b + 1], :]
        if folded:
            J = np.stack([jsfs_fold(J[:, :, k]) for k in range(J.shape[2])], axis=2) if J.shape[2] else J
        js.append(np.array(J) if per_block else np.array(J[:, :, 0]))
        used.append(r["n_used2"][a, b, :] if per_block else r["n_used2"][a, b, 0])
    out = dict(pairs=pairs, jsfs=js, n_used=np.array(used, dtype=np.int64).reshape((pairs.shape[1], -1) if per_block else (-1,)),
               n=r["n"])
    if per_block:
        out.update(lo=np.asarray(lo, dtype=np.int64), hi=np.asarray(hi, dtype=np.int64))
    return out


# include/tpg.h "admixture": loci per partial sum of the Q update (results do not depend on launch geometry)
ADMIX_CHUNK_LOCI = int(lib.tpg_admix_chunk_loci()) if hasattr(lib, "tpg_admix_chunk_loci") else 0


def _admix_mat(x, rows: int, K: int, name: str):
    """a start / state matrix for the C ABI: a numpy (rows, K) array -> column-major doubles; an int -> a device pointer"""
    if x is None or isinstance(x, (int, np.integer)):
        return x
    a = np.asfortranarray(x, dtype=np.float64)
    if a.shape != (rows, K):
        raise ValueError(f"{name} must be {rows} x {K}, not {a.shape}")
    return a


def _admix_accel(accel) -> bool:
    """accel of admix_em / admix_cv / gt_admixture: None = the plain EM; "squarem" = the driver of include/tpg.h "admixture,
    accelerated"; anything else is a ValueError"""
    if accel is None:
        return False
    if accel == "squarem":
        return True
    raise ValueError(f"accel must be None or 'squarem', not {accel!r}")


def admix_em(v: View, K: int, Q0=None, F0=None, seed: int = 0, max_iter: int = 1000, tol: float = 1e-4, update_q: bool = True,
             update_f: bool = True, return_trace: bool = False, ploidy=None, accel=None) -> dict:
    """tpg_admix_em (include/tpg.h "admixture"): maximum-likelihood ancestry proportions of a resident view by EM.  Q0 (n x K)
    and F0 (m x K, the shape of a .P file) are numpy arrays or device pointers (int); None draws that half of the start from
    `seed`.  -> dict(Q (n x K), P (m x K, frequency of the counted allele), loglik, n_iter, converged[, trace = l(0 .. n_iter)])
    accel="squarem": tpg_admix_em_squarem (include/tpg.h "admixture, accelerated"), the same EM step under squared
    extrapolation; n_iter still counts EM steps, and the dict gains n_cycles, n_rejected[, alpha, accepted: one entry per cycle;
    trace = l of every state a step was applied to, then loglik]."""
    K = int(K)
    if _admix_accel(accel):
        return _admix_em_squarem(v, K, Q0, F0, seed, max_iter, tol, update_q, update_f, return_trace, ploidy)
    q0, f0 = _admix_mat(Q0, v.n, K, "Q0"), _admix_mat(F0, v.m, K, "F0")
    pr = _lib.AdmixParams(int(max_iter), float(tol), int(bool(update_q)), int(bool(update_f)), int(seed) & 0xFFFFFFFFFFFFFFFF)
    Q, P = np.zeros((v.n, max(K, 1)), order="F"), np.zeros((v.m, max(K, 1)), order="F")  # K < 1 is the library's to refuse
    trace = np.full(max(int(max_iter), 0) + 1, np.nan)
    ll, nit, conv = C.c_double(), C.c_int32(), C.c_int32()
    pl = _f64(ploidy)
    check(lib.tpg_admix_em(v.ctx.h, v.h, _ptr(pl), K, C.byref(pr), _ptr(q0), _ptr(f0), _ptr(Q), _ptr(P), C.byref(ll),
                           _ptr(trace), C.byref(nit), C.byref(conv)))
    out = dict(Q=Q, P=P, loglik=ll.value, n_iter=int(nit.value), converged=bool(conv.value))
    if return_trace:
        out["trace"] = trace[: nit.value + 1].copy()
    return out


def _admix_em_squarem(v, K, Q0, F0, seed, max_iter, tol, update_q, update_f, return_trace, ploidy) -> dict:
    q0, f0 = _admix_mat(Q0, v.n, K, "Q0"), _admix_mat(F0, v.m, K, "F0")
    pr = _lib.AdmixParams(int(max_iter), float(tol), int(bool(update_q)), int(bool(update_f)), int(seed) & 0xFFFFFFFFFFFFFFFF)
    Q, P = np.zeros((v.n, max(K, 1)), order="F"), np.zeros((v.m, max(K, 1)), order="F")  # K < 1 is the library's to refuse
    trace = np.full(max(int(max_iter), 0) + 1, np.nan)
    nc = max(int(max_iter), 0) // 3 + 1
    alpha, acc = np.full(nc, np.nan), np.zeros(nc, dtype=np.int32)
    ll, nit, conv, ncyc, nrej = C.c_double(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    pl = _f64(ploidy)
    check(lib.tpg_admix_em_squarem(v.ctx.h, v.h, _ptr(pl), K, C.byref(pr), _ptr(q0), _ptr(f0), _ptr(Q), _ptr(P), C.byref(ll),
                                   _ptr(trace), C.byref(nit), C.byref(conv), _ptr(alpha), _ptr(acc), C.byref(ncyc), C.byref(nrej)))
    out = dict(Q=Q, P=P, loglik=ll.value, n_iter=int(nit.value), converged=bool(conv.value), n_cycles=int(ncyc.value),
               n_rejected=int(nrej.value))
    if return_trace:
        out["trace"] = trace[: nit.value + 1].copy()
        out["alpha"] = alpha[: ncyc.value].copy()
        out["accepted"] = acc[: ncyc.value].astype(bool)
    return out


def admix_squarem_point(Q0, F0, Q1, F1, Q2, F2, a_max: float = 4.0, update_q: bool = True, update_f: bool = True, ctx=None) -> dict:
    """tpg_admix_squarem_point (include/tpg.h "admixture, accelerated", steps 3 to 7) for the caller's own theta0, theta1, theta2
    (Q*: n x K, F*: m x K numpy arrays, taken as given) -> dict(sr, sv, alpha, Q, P = the projected theta', Q_raw, P_raw = theta'
    before the projection).  ctx: a Context (None: the default one)."""
    q = [np.asfortranarray(x, dtype=np.float64) for x in (Q0, Q1, Q2)]
    f = [np.asfortranarray(x, dtype=np.float64) for x in (F0, F1, F2)]
    if q[0].ndim != 2 or f[0].ndim != 2 or q[0].shape[1] != f[0].shape[1]:
        raise ValueError("Q0 must be n x K and F0 m x K")
    (n, K), m = q[0].shape, f[0].shape[0]
    for a, name in zip(q[1:] + f[1:], ("Q1", "Q2", "F1", "F2")):
        _admix_mat(a, n if name[0] == "Q" else m, K, name)
    ctx = ctx if ctx is not None else default_context()
    out = [np.zeros((n, K), order="F"), np.zeros((m, K), order="F"), np.zeros((n, K), order="F"), np.zeros((m, K), order="F")]
    sr, sv, al = C.c_double(), C.c_double(), C.c_double()
    check(lib.tpg_admix_squarem_point(ctx.h, n, m, K, int(bool(update_q)), int(bool(update_f)), _ptr(q[0]), _ptr(f[0]), _ptr(q[1]),
                                      _ptr(f[1]), _ptr(q[2]), _ptr(f[2]), float(a_max), C.byref(sr), C.byref(sv), C.byref(al),
                                      _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3])))
    return dict(sr=sr.value, sv=sv.value, alpha=al.value, Q=out[0], P=out[1], Q_raw=out[2], P_raw=out[3])


def admix_loglik(v: View, Q, P) -> float:
    """tpg_admix_loglik: l(Q, P) of the caller's own state, taken as given (no normalisation, no clamp)"""
    if isinstance(Q, (int, np.integer)) or isinstance(P, (int, np.integer)):
        raise ValueError("admix_loglik takes numpy arrays (K is read from their shape)")
    q = np.asfortranarray(Q, dtype=np.float64)
    K = q.shape[1] if q.ndim == 2 else 0
    q, p = _admix_mat(q, v.n, K, "Q"), _admix_mat(P, v.m, K, "P")
    ll = C.c_double()
    check(lib.tpg_admix_loglik(v.ctx.h, v.h, K, _ptr(q), _ptr(p), C.byref(ll)))
    return ll.value


ADMIX_MAX_FOLDS = 64  # TPG_ADMIX_MAX_FOLDS of include/tpg.h


def admix_holdout_sums(full: View, train: View, Q, P) -> dict:
    """tpg_admix_holdout_sums: over the entries typed in `full` and missing in `train` (two views of the same geometry, as
    View.holdout makes them), from the caller's own (Q, P) taken as given -> dict(ll = sum ln(p^g pbar^(2-g)), n_held, n_het)"""
    if isinstance(Q, (int, np.integer)) or isinstance(P, (int, np.integer)):
        raise ValueError("admix_holdout_sums takes numpy arrays (K is read from their shape)")
    q = np.asfortranarray(Q, dtype=np.float64)
    K = q.shape[1] if q.ndim == 2 else 0
    q, p = _admix_mat(q, full.n, K, "Q"), _admix_mat(P, full.m, K, "P")
    ll, cnt, het = C.c_double(), C.c_int64(), C.c_int64()
    check(lib.tpg_admix_holdout_sums(full.ctx.h, full.h, train.h, K, _ptr(q), _ptr(p), C.byref(ll), C.byref(cnt), C.byref(het)))
    return dict(ll=ll.value, n_held=int(cnt.value), n_het=int(het.value))


def admix_cv_error(fold_ll, fold_count, fold_het) -> dict:
    """tpg_admix_cv_error (host only): the folds' hold-out sums -> dict(cv_error, fold_deviance); deviance of fold f =
    -2 ll_f - 4 ln 2 het_f, cv_error = their sum / the total count"""
    ll = np.ascontiguousarray(fold_ll, dtype=np.float64).ravel()
    cnt = np.ascontiguousarray(fold_count, dtype=np.int64).ravel()
    het = np.ascontiguousarray(fold_het, dtype=np.int64).ravel()
    if not (len(ll) == len(cnt) == len(het)):
        raise ValueError("fold_ll, fold_count and fold_het must have one entry per fold")
    dev = np.zeros(max(len(ll), 1))
    cv = C.c_double()
    check(lib.tpg_admix_cv_error(len(ll), _ptr(ll), _ptr(cnt), _ptr(het), _ptr(dev), C.byref(cv)))
    return dict(cv_error=cv.value, fold_deviance=dev[: len(ll)])


def admix_cv(v: View, K: int, folds: int = 5, cv_seed: int = 0, Q0=None, F0=None, seed: int = 0, max_iter: int = 1000,
             tol: float = 1e-4, update_q: bool = True, update_f: bool = True, ploidy=None, accel=None) -> dict:
    """tpg_admix_cv (include/tpg.h "admixture cross-validation"): for every fold, the EM on the view without the fold's genotypes
    (the same start each time: Q0 / F0 or the seeded one) and the deviance of the held-out genotypes under that fit, all on the
    device.  -> dict(cv_error, fold_deviance, fold_ll, fold_count, fold_het, fold_n_iter, fold_converged)
    accel="squarem": tpg_admix_cv_squarem, every fold refitted by the accelerated driver."""
    K, folds = int(K), int(folds)
    entry = lib.tpg_admix_cv_squarem if _admix_accel(accel) else lib.tpg_admix_cv
    q0, f0 = _admix_mat(Q0, v.n, K, "Q0"), _admix_mat(F0, v.m, K, "F0")
    pr = _lib.AdmixParams(int(max_iter), float(tol), int(bool(update_q)), int(bool(update_f)), int(seed) & 0xFFFFFFFFFFFFFFFF)
    nf = min(max(folds, 1), ADMIX_MAX_FOLDS)  # folds out of range is the library's to refuse
    ll, cnt, het = np.zeros(nf), np.zeros(nf, dtype=np.int64), np.zeros(nf, dtype=np.int64)
    nit, conv = np.zeros(nf, dtype=np.int32), np.zeros(nf, dtype=np.int32)
    cv = C.c_double()
    pl = _f64(ploidy)
    check(entry(v.ctx.h, v.h, _ptr(pl), K, C.byref(pr), folds, int(cv_seed) & 0xFFFFFFFFFFFFFFFF, _ptr(q0), _ptr(f0),
                C.byref(cv), _ptr(ll), _ptr(cnt), _ptr(het), _ptr(nit), _ptr(conv)))
    dev = admix_cv_error(ll, cnt, het)["fold_deviance"]
    return dict(cv_error=cv.value, fold_deviance=dev, fold_ll=ll, fold_count=cnt, fold_het=het, fold_n_iter=nit,
                fold_converged=conv.astype(bool))


def gt_admixture(X: FBM, ind_row=None, ind_col=None, k=None, n_runs: int = 1, seed=None, max_iter: int = 1000,
                 tol: float = 1e-4, crossval: bool = False, cv_folds: int = 5, cv_seed: int = 0, accel=None) -> dict:
    """R/gt_admixture.R:62-236 with the EM of include/tpg.h "admixture" in place of the outside binary: every k of `k` (a
    scalar or a list) is run n_runs times on one resident view.  seed has n_runs entries (repeated for every k) or
    n_runs * len(k), one per run in the order of the result (k by k); None: 0, 1, ... in that order.
    -> a gt_admix-shaped dict: k (one entry per run), Q, P, loglik as lists, plus n_iter and converged.
    crossval=True adds `cv`, parallel to `k` (the name the reference uses): the cv_folds-fold cross-validation error of that
    run's k and seed on the same resident view (admix_cv; include/tpg.h "admixture cross-validation" is the definition, so the
    number orders the k as ADMIXTURE's does without being ADMIXTURE's).  The smallest cv marks the k to use.
    accel="squarem" runs every fit and every cross-validation refit under squared extrapolation (include/tpg.h "admixture,
    accelerated"): the same likelihood in fewer EM steps; n_iter still counts EM steps.
    conda_env and outdir of the reference have no counterpart here: there is no outside program and no file; `log` is absent
    for the same reason.  P is the frequency of the counted allele."""
    if k is None:
        raise ValueError("k is required")
    _admix_accel(accel)
    ks = [int(x) for x in np.atleast_1d(k)]
    n_runs = int(n_runs)
    if seed is not None:
        seed = [int(s) for s in np.atleast_1d(seed)]
        if len(seed) != n_runs and len(seed) != n_runs * len(ks):
            raise ValueError("'seed' should be a vector of length 'n_runs' OR 'n_runs' * length(k)")
        if len(seed) == n_runs:
            seed = seed * len(ks)
    else:
        seed = list(range(n_runs * len(ks)))
    if crossval and not (isinstance(cv_folds, (int, np.integer)) and 2 <= cv_folds <= ADMIX_MAX_FOLDS):
        raise ValueError(f"'cv_folds' should be an integer in [2, {ADMIX_MAX_FOLDS}]")
    v = View(X, ind_row, ind_col)
    out = dict(k=[], Q=[], P=[], loglik=[], n_iter=[], converged=[])
    if crossval:
        out["cv"] = []
    for a, kk in enumerate(ks):
        for b in range(n_runs):
            r = admix_em(v, kk, seed=seed[a * n_runs + b], max_iter=max_iter, tol=tol, accel=accel)
            out["k"].append(kk)
            for name in ("Q", "P", "loglik", "n_iter", "converged"):
                out[name].append(r[name])
            if crossval:
                out["cv"].append(admix_cv(v, kk, folds=cv_folds, cv_seed=cv_seed, seed=seed[a * n_runs + b], max_iter=max_iter,
                                          tol=tol, accel=accel)["cv_error"])
    return out


SNMF_MAX_K = 16  # TPG_SNMF_MAX_K of include/tpg.h


def snmf(v: View, K: int, Q0=None, seed: int = 0, alpha: float = 10.0, tol: float = 1e-5, max_iter: int = 200,
         return_trace: bool = False, ploidy=None) -> dict:
    """tpg_snmf (include/tpg.h "sNMF"): ancestry proportions of a resident view by sparse non-negative matrix factorisation.  Q0
    (n x K) is a numpy array or a device pointer (int); None draws the start from `seed` (the seeded Q of admix_em).
    -> dict(Q (n x K), G (3m x K, row 3 j + c), P (m x K, frequency of the counted allele), ls, n_iter, converged, n_unsolved
    [, trace = ls(1 .. n_iter)])"""
    K = int(K)
    q0 = _admix_mat(Q0, v.n, K, "Q0")
    kk = max(K, 1)  # K < 1 is the library's to refuse
    Q, G, P = np.zeros((v.n, kk), order="F"), np.zeros((3 * v.m, kk), order="F"), np.zeros((v.m, kk), order="F")
    trace = np.full(max(int(max_iter), 0) + 1, np.nan)
    ls, nit, conv, uns = C.c_double(), C.c_int(), C.c_int(), C.c_int64()
    pl = _f64(ploidy)
    check(lib.tpg_snmf(v.ctx.h, v.h, _ptr(pl), K, int(max_iter), float(tol), float(alpha), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(q0),
                       _ptr(Q), _ptr(G), _ptr(P), C.byref(ls), _ptr(trace), C.byref(nit), C.byref(conv), C.byref(uns)))
    out = dict(Q=Q, G=G, P=P, ls=ls.value, n_iter=int(nit.value), converged=bool(conv.value), n_unsolved=int(uns.value))
    if return_trace:
        out["trace"] = trace[: nit.value].copy()
    return out


def snmf_step(v: View, Q, alpha: float = 10.0) -> dict:
    """tpg_snmf_step: one iteration from the caller's own Q (n x K, taken as given) -> dict(Q, G (3m x K), ls, n_unsolved)"""
    if isinstance(Q, (int, np.integer)):
        raise ValueError("snmf_step takes a numpy array (K is read from its shape)")
    q = np.asfortranarray(Q, dtype=np.float64)
    K = q.shape[1] if q.ndim == 2 else 0
    q = _admix_mat(q, v.n, K, "Q")
    Qn, G = np.zeros((v.n, max(K, 1)), order="F"), np.zeros((3 * v.m, max(K, 1)), order="F")
    ls, uns = C.c_double(), C.c_int64()
    check(lib.tpg_snmf_step(v.ctx.h, v.h, K, float(alpha), _ptr(q), _ptr(Qn), _ptr(G), C.byref(ls), C.byref(uns)))
    return dict(Q=Qn, G=G, ls=ls.value, n_unsolved=int(uns.value))


def nnls_shared(A, B, ctx: Optional[Context] = None, return_unsolved: bool = False):
    """tpg_nnls_shared: X(r, .) = argmin over x >= 0 of x'Ax / 2 - B(r, .)'x for every row of B (nrhs x K), A K x K symmetric
    positive definite -> X (nrhs x K) [, n_unsolved: the systems that miss the KKT contract of include/tpg.h "sNMF"]"""
    ctx = ctx or default_context()
    a, b = np.asfortranarray(A, dtype=np.float64), np.asfortranarray(B, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1] or b.ndim != 2 or b.shape[1] != a.shape[0]:
        raise ValueError(f"A must be K x K and B nrhs x K, not {a.shape} and {b.shape}")
    X = np.zeros(b.shape, order="F")
    uns = C.c_int64()
    check(lib.tpg_nnls_shared(ctx.h, a.shape[0], _ptr(a), _ptr(b), b.shape[0], _ptr(X), C.byref(uns)))
    return (X, int(uns.value)) if return_unsolved else X


def snmf_cross_entropy(full: View, train: View, Q, G) -> dict:
    """tpg_snmf_cross_entropy_sums: -ln max(p, floor) of the genotypes under (Q, G), taken as given, summed over the entries typed in
    `full` and missing in `train` (masked) and over those typed in `train` (all); two views of the same geometry, as
    View.holdout_fraction makes them -> dict(masked, all (the cross-entropies), sum_masked, n_masked, sum_all, n_all)"""
    if isinstance(Q, (int, np.integer)) or isinstance(G, (int, np.integer)):
        raise ValueError("snmf_cross_entropy takes numpy arrays (K is read from their shape)")
    q = np.asfortranarray(Q, dtype=np.float64)
    K = q.shape[1] if q.ndim == 2 else 0
    q, g = _admix_mat(q, full.n, K, "Q"), _admix_mat(G, 3 * full.m, K, "G")
    sm, sa, nm, na = C.c_double(), C.c_double(), C.c_int64(), C.c_int64()
    check(lib.tpg_snmf_cross_entropy_sums(full.ctx.h, full.h, train.h, K, _ptr(q), _ptr(g), C.byref(sm), C.byref(nm), C.byref(sa),
                                          C.byref(na)))
    return dict(masked=sm.value / nm.value if nm.value else float("nan"), all=sa.value / na.value if na.value else float("nan"),
                sum_masked=sm.value, n_masked=int(nm.value), sum_all=sa.value, n_all=int(na.value))


def gt_snmf(X: FBM, ind_row=None, ind_col=None, k=None, n_runs: int = 1, alpha: float = 10, tolerance: float = 1e-5,
            entropy: bool = False, percentage: float = 0.05, iterations: int = 200, seed=None, impute: Optional[str] = None) -> dict:
    """R/gt_snmf.R with the sNMF of include/tpg.h "sNMF" in place of LEA::snmf: every k of `k` (a scalar or a list) is run n_runs
    times on one resident view.  seed is handled as gt_admixture handles it: n_runs entries (repeated for every k) or
    n_runs * len(k), one per run in the order of the result; None: 0, 1, ... in that order.
    -> a gt_admix-shaped dict: k (one entry per run), Q, P (frequency of the counted allele), G (3m x K, LEA's .G order), ls,
    n_iter and converged as lists, algorithm = "SNMF".  entropy=True holds a share `percentage` of the typed genotypes out (the mask
    is drawn from the run's seed), fits on the hold-out view, as LEA does, and adds `cv` (the masked cross-entropy, the name the
    reference uses: the smallest marks the k to use) and `cv_all` (that of the genotypes the fit saw).
    impute = "mode" | "mean0" | "random" fills the missing genotypes first (View.impute); by default they stay in the loss as
    zeros.  project, I and a ploidy other than 2 of the reference have no counterpart here: there is no project file, the start is
    the seeded one, and the three-class encoding is the diploid one."""
    if k is None:
        raise ValueError("k is required")
    ks = [int(x) for x in np.atleast_1d(k)]
    n_runs = int(n_runs)
    if seed is not None:
        seed = [int(s) for s in np.atleast_1d(seed)]
        if len(seed) != n_runs and len(seed) != n_runs * len(ks):
            raise ValueError("'seed' should be a vector of length 'n_runs' OR 'n_runs' * length(k)")
        if len(seed) == n_runs:
            seed = seed * len(ks)
    else:
        seed = list(range(n_runs * len(ks)))
    if entropy and not 0.0 < float(percentage) < 1.0:
        raise ValueError("'percentage' should lie strictly between 0 and 1")
    v = View(X, ind_row, ind_col)
    if impute is not None:
        v = v.impute(impute)
    out = dict(k=[], Q=[], P=[], G=[], ls=[], n_iter=[], converged=[], algorithm="SNMF")
    if entropy:
        out["cv"], out["cv_all"] = [], []
    for a, kk in enumerate(ks):
        for b in range(n_runs):
            sd = seed[a * n_runs + b]
            train = v.holdout_fraction(percentage, sd) if entropy else v
            r = snmf(train, kk, seed=sd, alpha=alpha, tol=tolerance, max_iter=iterations)
            out["k"].append(kk)
            for name in ("Q", "P", "G", "ls", "n_iter", "converged"):
                out[name].append(r[name])
            if entropy:
                ce = snmf_cross_entropy(v, train, r["Q"], r["G"])
                out["cv"].append(ce["masked"])
                out["cv_all"].append(ce["all"])
                train.free()
    return out


# ---------------------------------------------------------------------------
# k-means on PCA scores and DAPC (include/tpg.h "k-means on PCA scores", "DAPC")

# doubles of centre coordinates one LDS chunk of the assign kernel holds (the tests put k * d around it)
KMEANS_CHUNK_DOUBLES = int(lib.tpg_kmeans_chunk_doubles())
_M64 = (1 << 64) - 1


def _mix64(x: int) -> int:
    """tpg_mix64 on a Python int (the splitmix64 finaliser)"""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def kmeans_run_seed(seed: int, k: int, t: int) -> int:
    """the seed of start t of gt_cluster_pca's runs at k clusters: M(seed ^ M((k << 32) + t))"""
    return _mix64((int(seed) & _M64) ^ _mix64(((int(k) << 32) + int(t)) & _M64))


def _scores(X):
    x = np.asfortranarray(X, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("X must be a matrix of n points x d coordinates")
    return x


def kmeans_start(seed: int, n: int, k: int) -> np.ndarray:
    """tpg_kmeans_start: the k start rows (0-based) of a run, a pure function of (seed, n, k)"""
    idx = np.zeros(max(int(k), 1), dtype=np.int32)
    check(lib.tpg_kmeans_start(int(seed) & _M64, int(n), int(k), _ptr(idx)))
    return idx[:k]


def kmeans_step(X, centers, ctx: Optional[Context] = None) -> dict:
    """tpg_kmeans_step: one assign and one update from the given centres (k x d) -> dict(labels (0-based), centers, counts, wss:
    the sum of the smallest squared distances under the GIVEN centres)"""
    ctx = ctx or default_context()
    x, c = _scores(X), _scores(centers)
    n, d = x.shape
    k = c.shape[0]
    if c.shape[1] != d:
        raise ValueError(f"centers must be k x {d}, not {c.shape}")
    labels, counts = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(k, 1), dtype=np.int32)
    cn, wss = np.zeros((max(k, 1), max(d, 1)), order="F"), C.c_double()
    check(lib.tpg_kmeans_step(ctx.h, _ptr(x), n, d, k, _ptr(c), _ptr(labels), _ptr(cn), _ptr(counts), C.byref(wss)))
    return dict(labels=labels, centers=cn, counts=counts, wss=wss.value)


def kmeans_batch(X, k, seed=None, max_iter: int = 100000, centers0=None, return_centers: bool = True,
                 ctx: Optional[Context] = None) -> dict:
    """tpg_kmeans_batch: len(k) independent Lloyd runs over the same points in one call.  k and seed: one entry per run;
    centers0 (instead of seed): a list of k_r x d start centres.  -> dict(labels (n x R, 0-based), centers (list of k_r x d), wss,
    n_iter, converged, n_empty)"""
    ctx = ctx or default_context()
    x = _scores(X)
    n, d = x.shape
    ks = np.ascontiguousarray(np.atleast_1d(k), dtype=np.int32)
    R = len(ks)
    if R < 1:
        raise ValueError("at least one run is needed")
    if (seed is None) == (centers0 is None):
        raise ValueError("give either one seed per run or the start centres")
    seeds = c0 = None
    if seed is not None:
        sd = [int(s) & _M64 for s in np.atleast_1d(np.asarray(seed, dtype=object))]
        if len(sd) != R:
            raise ValueError(f"{len(sd)} seeds for {R} runs")
        seeds = np.array(sd, dtype=np.uint64).view(np.int64)
    else:
        if len(centers0) != R:
            raise ValueError(f"{len(centers0)} start blocks for {R} runs")
        blocks = [_scores(c) for c in centers0]
        for kk, b in zip(ks, blocks):
            if b.shape != (kk, d):
                raise ValueError(f"a start block of shape {b.shape} for k = {kk}, d = {d}")
        c0 = np.concatenate([b.ravel(order="F") for b in blocks])
    ktot = int(np.maximum(ks, 0).sum())
    labels = np.zeros((max(n, 1), R), dtype=np.int32, order="F")
    cen = np.zeros(max(ktot * d, 1)) if return_centers else None
    wss, n_iter = np.zeros(R), np.zeros(R, dtype=np.int32)
    conv, n_empty = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
    check(lib.tpg_kmeans_batch(ctx.h, _ptr(x), n, d, R, _ptr(ks), _ptr(seeds), int(max_iter), _ptr(c0), _ptr(labels), _ptr(cen),
                               _ptr(wss), _ptr(n_iter), _ptr(conv), _ptr(n_empty)))
    out = dict(labels=labels[:n], wss=wss, n_iter=n_iter, converged=conv.astype(bool), n_empty=n_empty)
    if return_centers:
        off = np.concatenate([[0], np.cumsum(ks.astype(np.int64))]) * d
        out["centers"] = [cen[off[r]:off[r + 1]].reshape((int(ks[r]), d), order="F") for r in range(R)]
    return out


def gt_cluster_pca(pca: dict, n_pca: Optional[int] = None, k_clusters=None, n_iter: int = 100000, n_start: int = 10, seed: int = 0,
                   method: str = "kmeans", ctx: Optional[Context] = None) -> dict:
    """R/gt_cluster_pca.R:75-177 with the Lloyd k-means of include/tpg.h in place of stats::kmeans: scores = u d (the first n_pca
    columns); every k of k_clusters (one value, or (min, max); default (1, round(n / 10))) gets n_start runs from the seeds
    kmeans_run_seed(seed, k, t), ALL runs of ALL k in one tpg_kmeans_batch call; per k the run of smallest WSS wins (on a tie the
    smaller t).  k = 1 is one run (every start gives the column means).  -> the pca dict plus clusters = dict(method, n_pca, k,
    WSS, AIC, BIC, groups ({k: labels, 1-based as R's}), n_iter, converged, n_empty)."""
    if method == "ward":
        raise NotImplementedError("method = 'ward' is not forwarded from here yet: call gt_cluster_pca_ward (DESIGN.md section 3.14)")
    if method != "kmeans":
        raise ValueError("'method' should be one of 'kmeans', 'ward'")
    u, dd = np.asarray(pca["u"], dtype=np.float64), np.asarray(pca["d"], dtype=np.float64)
    n = u.shape[0]
    n_pca = len(dd) if n_pca is None else int(n_pca)
    if not 1 <= n_pca <= len(dd):
        raise ValueError(f"n_pca = {n_pca} outside [1, {len(dd)}]")
    kc = [int(round(n / 10))] if k_clusters is None else [int(x) for x in np.atleast_1d(k_clusters)]
    if k_clusters is None:
        kc = [1, max(kc[0], 1)]
    if len(kc) == 1:
        ks = kc
    elif len(kc) == 2:
        ks = list(range(kc[0], kc[1] + 1))
    else:
        raise ValueError("'k_clusters' should be either a single value, or the minimum and maximum to be tested")
    if not ks or ks[0] < 1:
        raise ValueError("'k_clusters' should name at least one k >= 1")
    n_start = int(n_start)
    if n_start < 1:
        raise ValueError("n_start must be at least 1")
    scores = np.asfortranarray((u * dd[None, :])[:, :n_pca])
    run_k, run_seed = [], []
    for kk in ks:
        for t in range(1 if kk == 1 else n_start):
            run_k.append(kk)
            run_seed.append(kmeans_run_seed(seed, kk, t))
    r = kmeans_batch(scores, run_k, run_seed, max_iter=int(n_iter), return_centers=False, ctx=ctx)
    wss, groups, iters, conv, empty = [], {}, [], [], []
    at = 0
    for kk in ks:
        cnt = 1 if kk == 1 else n_start
        best = at + int(np.argmin(r["wss"][at:at + cnt]))  # (the first minimum: the smaller t)
        wss.append(float(r["wss"][best]))
        groups[kk] = r["labels"][:, best].astype(np.int32) + 1
        iters.append(int(r["n_iter"][best]))
        conv.append(bool(r["converged"][best]))
        empty.append(int(r["n_empty"][best]))
        at += cnt
    wss, kv = np.array(wss), np.array(ks, dtype=np.float64)
    with np.errstate(divide="ignore"):
        base = n * np.log(wss / n)
    out = dict(pca)
    out["clusters"] = dict(method=method, n_pca=n_pca, k=list(ks), WSS=wss, AIC=base + 2 * kv, BIC=base + math.log(n) * kv,
                           groups=groups, n_iter=iters, converged=conv, n_empty=empty)
    return out


HCLUST_MAX_N = 32768  # TPG_HCLUST_MAX_N
KMEANS_MAX_K = 1024    # TPG_KMEANS_MAX_K: the largest k tpg_kmeans_batch and tpg_cluster_wss take


def hclust_ward(X, power: int = 2, ctx: Optional[Context] = None, *, return_list_len: bool = False) -> dict:
    """tpg_hclust_ward: the Ward tree of n points x d coordinates (include/tpg.h "Ward clustering on PCA scores").  power = 2 is
    the reference's hclust(dist(x)^2, "ward.D2"), the recurrence on d^4; power = 1 the proper criterion, on d^2.  -> dict(n,
    merge_a, merge_b (0-based slots), height (the S of every merge, NOT its root), merge ((n - 1) x 2, R's hclust$merge)[,
    list_len: the device's recompute list per step, a diagnostic])"""
    ctx = ctx or default_context()
    x = _scores(X)
    n, d = x.shape
    m = max(n - 1, 0)
    ma, mb, h = np.zeros(max(m, 1), dtype=np.int32), np.zeros(max(m, 1), dtype=np.int32), np.zeros(max(m, 1))
    ll = np.zeros(max(m, 1), dtype=np.int32) if return_list_len else None
    check(lib.tpg_hclust_ward_trace(ctx.h, _ptr(x), n, d, int(power), _ptr(ma), _ptr(mb), _ptr(h), _ptr(ll)))
    merge = np.zeros((m, 2), dtype=np.int32, order="F")
    check(lib.tpg_hclust_r_merge(n, _ptr(ma), _ptr(mb), _ptr(merge if m else None)))
    out = dict(n=n, merge_a=ma[:m], merge_b=mb[:m], height=h[:m], merge=merge)
    if return_list_len:
        out["list_len"] = ll[:m]
    return out


def hclust_cut(tree: dict, k) -> np.ndarray:
    """tpg_hclust_cut (host only): labels n x len(k), 0-based, column r the first n - k[r] merges of the tree, the clusters
    numbered in the order in which they first appear (cutree's numbering)"""
    n = int(tree["n"])
    ks = np.ascontiguousarray(np.atleast_1d(k), dtype=np.int32)
    ma, mb = _i32(tree["merge_a"]), _i32(tree["merge_b"])
    if len(ma) != n - 1 or len(mb) != n - 1:
        raise ValueError(f"a tree of {n} points has {n - 1} merges")
    labels = np.zeros((max(n, 1), len(ks)), dtype=np.int32, order="F")
    check(lib.tpg_hclust_cut(n, _ptr(ma if n > 1 else None), _ptr(mb if n > 1 else None), len(ks), _ptr(ks), _ptr(labels)))
    return labels[:n]


# ---- trees from a pairwise matrix (include/tpg.h "Trees from a pairwise matrix")

LINKAGES = {"single": 0, "complete": 1, "average": 2, "mcquitty": 3, "ward.D": 4, "ward.D2": 4}  # TPG_LINK_*


def _tree_operand(D, ctx):
    """D (numpy n x n or DeviceMatrix) -> (ctx, n, pointer, the object that keeps the pointer alive)"""
    if isinstance(D, DeviceMatrix):
        return D.ctx, D.n, D.p, D
    keep = np.asfortranarray(D, dtype=np.float64)
    if keep.ndim != 2 or keep.shape[0] != keep.shape[1]:
        raise ValueError("D must be a square matrix")
    return ctx or default_context(), keep.shape[0], _ptr(keep), keep


def hclust_order(tree: dict) -> np.ndarray:
    """tpg_hclust_order (host only): hclust$order of a tree of hclust_ward / hclust_dist, 1-based as R"""
    n = int(tree["n"])
    ma, mb = _i32(tree["merge_a"]), _i32(tree["merge_b"])
    if len(ma) != n - 1 or len(mb) != n - 1:
        raise ValueError(f"a tree of {n} points has {n - 1} merges")
    order = np.zeros(max(n, 1), dtype=np.int32)
    check(lib.tpg_hclust_order(n, _ptr(ma if n > 1 else None), _ptr(mb if n > 1 else None), _ptr(order)))
    return order[:n] + 1


def hclust_dist(D, method: str = "complete", ctx: Optional[Context] = None) -> dict:
    """tpg_hclust_dist: stats::hclust(as.dist(D), method) on the strict lower triangle of D (a numpy array or a DeviceMatrix,
    never modified).  method: single, complete, average, mcquitty, ward.D, ward.D2 (the recurrence of ward.D on the squared
    matrix, the root of its heights).  -> the dict of hclust_ward (n, merge_a, merge_b, height, merge) plus order (1-based, as R)
    and method; hclust_cut works on it unchanged."""
    if method not in LINKAGES:
        raise ValueError(f"method must be one of {', '.join(LINKAGES)}")
    ctx, n, p, keep = _tree_operand(D, ctx)
    if method == "ward.D2":  # squared on the host: the caller's matrix stays as it is
        keep = np.asfortranarray(keep.to_numpy() if isinstance(keep, DeviceMatrix) else keep) ** 2
        p = _ptr(keep)
    m = max(n - 1, 0)
    ma, mb, h = np.zeros(max(m, 1), dtype=np.int32), np.zeros(max(m, 1), dtype=np.int32), np.zeros(max(m, 1))
    check(lib.tpg_hclust_dist(ctx.h, p, n, LINKAGES[method], _ptr(ma), _ptr(mb), _ptr(h)))
    merge = np.zeros((m, 2), dtype=np.int32, order="F")
    check(lib.tpg_hclust_r_merge(n, _ptr(ma), _ptr(mb), _ptr(merge if m else None)))
    out = dict(n=n, merge_a=ma[:m], merge_b=mb[:m], height=np.sqrt(h[:m]) if method == "ward.D2" else h[:m], merge=merge, method=method)
    out["order"] = hclust_order(out)
    return out


def nj(D, ctx: Optional[Context] = None) -> dict:
    """tpg_nj: the neighbour-joining tree of the strict lower triangle of D (a numpy array or a DeviceMatrix, never modified).
    -> dict(n, join_a, join_b (0-based slots, n - 2 joins), len_a, len_b (the branch of either slot to the new node), last
    (x, y, S(x, y)) of the two slots left; empty for n = 1)"""
    ctx, n, p, keep = _tree_operand(D, ctx)
    j = max(n - 2, 0)
    ja, jb = np.zeros(max(j, 1), dtype=np.int32), np.zeros(max(j, 1), dtype=np.int32)
    la, lb, last = np.zeros(max(j, 1)), np.zeros(max(j, 1)), np.zeros(3)
    check(lib.tpg_nj(ctx.h, p, n, _ptr(ja), _ptr(jb), _ptr(la), _ptr(lb), _ptr(last)))
    return dict(n=n, join_a=ja[:j], join_b=jb[:j], len_a=la[:j], len_b=lb[:j], last=last if n >= 2 else last[:0])


def nj_edges(tree: dict) -> dict:
    """tpg_nj_edges (host only): a tree of nj() in ape's phylo layout -> dict(edge ((2n - 3) x 2, parent and child, tips 1 .. n,
    root n + 1, preorder), edge_length, Nnode = n - 2); n >= 3"""
    n = int(tree["n"])
    ja, jb, la, lb, last = _i32(tree["join_a"]), _i32(tree["join_b"]), _f64(tree["len_a"]), _f64(tree["len_b"]), _f64(tree["last"])
    if n >= 3 and (any(len(v) != n - 2 for v in (ja, jb, la, lb)) or len(last) != 3):
        raise ValueError(f"a tree of {n} tips has {n - 2} joins and a last of 3")
    e = max(2 * n - 3, 1)
    edge, length = np.zeros((e, 2), dtype=np.int32, order="F"), np.zeros(e)
    check(lib.tpg_nj_edges(n, _ptr(ja), _ptr(jb), _ptr(la), _ptr(lb), _ptr(last), _ptr(edge), _ptr(length)))
    return dict(edge=edge, edge_length=length, Nnode=n - 2)


def nj_newick(tree: dict, labels=None, fmt: str = "%.17g") -> str:
    """The tree of nj() as Newick text, unrooted with a trifurcation at the root; labels default "1" .. "n" """
    n = int(tree["n"])
    labels = [str(i + 1) for i in range(n)] if labels is None else [str(v) for v in labels]
    if len(labels) != n:
        raise ValueError("labels must name every tip")
    e = nj_edges(tree)
    kids = {}
    # preorder: the edges below a node follow its own, so going backwards every child is complete when its edge comes up
    for (parent, child), length in zip(e["edge"][::-1].tolist(), e["edge_length"][::-1].tolist()):
        text = labels[child - 1] if child <= n else "(" + ",".join(reversed(kids.pop(child))) + ")"
        kids.setdefault(parent, []).append(text + ":" + fmt % length)
    return "(" + ",".join(reversed(kids[n + 1])) + ");"


def _gt_tree_matrix(X, ind_row, ind_col, dist, dist_type):
    if (X is None) == (dist is None):
        raise ValueError("give either X or dist")
    return pairwise_sqdist(X, ind_row, ind_col, dist_type, device=True) if dist is None else dist


def gt_hclust(X: Optional[FBM] = None, ind_row=None, ind_col=None, dist=None, dist_type: str = "raw", method: str = "complete") -> dict:
    """The tree the reference's heatmaps order by, stats::hclust(as.dist(.), method): of the squared genotype distances of X (one
    pairwise pass, dist_type "raw" or "adjusted", kept in HBM), or of dist (n x n matrix or DeviceMatrix), e.g. 1 - snp_ibs(X)
    for individuals or the fst_tot matrix of pairwise_pop_fst for populations.  -> hclust_dist's dict."""
    if method not in LINKAGES:
        raise ValueError(f"method must be one of {', '.join(LINKAGES)}")
    return hclust_dist(_gt_tree_matrix(X, ind_row, ind_col, dist, dist_type), method, ctx=X.ctx if X is not None else None)


def gt_nj(X: Optional[FBM] = None, ind_row=None, ind_col=None, dist=None, dist_type: str = "raw") -> dict:
    """The neighbour-joining tree of the squared genotype distances of X (kept in HBM) or of dist, as gt_hclust takes them.
    -> nj's dict; nj_edges and nj_newick turn it into ape's layout and into text."""
    return nj(_gt_tree_matrix(X, ind_row, ind_col, dist, dist_type), ctx=X.ctx if X is not None else None)


def cluster_wss(X, labels, k, return_counts: bool = False, ctx: Optional[Context] = None):
    """tpg_cluster_wss: the within-group sum of squares of every column of labels (n x R, 0-based, column r in [0, k[r])) in one
    call, by the kernels a run of kmeans_batch ends in -> wss (R)[, counts: a list of k_r points per label]"""
    ctx = ctx or default_context()
    x = _scores(X)
    n, d = x.shape
    lab = np.asfortranarray(labels, dtype=np.int32)
    if lab.ndim == 1:
        lab = np.asfortranarray(lab[:, None])
    ks = np.ascontiguousarray(np.atleast_1d(k), dtype=np.int32)
    R = len(ks)
    if lab.shape != (n, R):
        raise ValueError(f"labels must be {n} x {R}, not {lab.shape}")
    wss = np.zeros(max(R, 1))
    cnt = np.zeros(max(int(np.maximum(ks, 0).sum()), 1), dtype=np.int32) if return_counts else None
    check(lib.tpg_cluster_wss(ctx.h, _ptr(x), n, d, R, _ptr(ks), _ptr(lab), _ptr(wss), _ptr(cnt)))
    if not return_counts:
        return wss[:R]
    off = np.concatenate([[0], np.cumsum(np.maximum(ks, 0).astype(np.int64))])
    return wss[:R], [cnt[off[r]:off[r + 1]] for r in range(R)]


def gt_cluster_pca_ward(pca: dict, n_pca: Optional[int] = None, k_clusters=None, criterion: str = "reference",
                        ctx: Optional[Context] = None) -> dict:
    """method = "ward" of R/gt_cluster_pca.R:156-169 with ONE tree for every k in place of the reference's hclust per k: scores,
    the range of k and its default as gt_cluster_pca; criterion = "reference" is the reference's hclust(dist(x)^2, "ward.D2")
    (Ward's recurrence on d^4), "ward" the proper criterion (on d^2).  The tree is cut at every k on the host and all WSS come
    from one cluster_wss call, which takes k up to KMEANS_MAX_K = 1024: the default range 1 .. round(n / 10) goes past that from
    n = 10 246, and a range that does is refused here, before the tree is built (give k_clusters then).  -> the pca dict plus
    clusters = dict(method="ward", criterion, n_pca, k, WSS, AIC, BIC, groups ({k: labels, 1-based as R's}), merge and height as
    hclust reports them (height the root of S))."""
    if criterion not in ("reference", "ward"):
        raise ValueError("'criterion' should be one of 'reference', 'ward'")
    u, dd = np.asarray(pca["u"], dtype=np.float64), np.asarray(pca["d"], dtype=np.float64)
    n = u.shape[0]
    n_pca = len(dd) if n_pca is None else int(n_pca)
    if not 1 <= n_pca <= len(dd):
        raise ValueError(f"n_pca = {n_pca} outside [1, {len(dd)}]")
    kc = [1, max(int(round(n / 10)), 1)] if k_clusters is None else [int(x) for x in np.atleast_1d(k_clusters)]
    if len(kc) == 1:
        ks = kc
    elif len(kc) == 2:
        ks = list(range(kc[0], kc[1] + 1))
    else:
        raise ValueError("'k_clusters' should be either a single value, or the minimum and maximum to be tested")
    if not ks or ks[0] < 1:
        raise ValueError("'k_clusters' should name at least one k >= 1")
    if ks[-1] > min(n, KMEANS_MAX_K):
        raise ValueError(f"'k_clusters' reaches k = {ks[-1]}, above min(n = {n}, {KMEANS_MAX_K}), the largest k the WSS is summed for")
    scores = np.asfortranarray((u * dd[None, :])[:, :n_pca])
    tree = hclust_ward(scores, power=2 if criterion == "reference" else 1, ctx=ctx)
    labels = hclust_cut(tree, ks)
    wss, kv = cluster_wss(scores, labels, ks, ctx=ctx), np.array(ks, dtype=np.float64)
    with np.errstate(divide="ignore"):
        base = n * np.log(wss / n)
    out = dict(pca)
    out["clusters"] = dict(method="ward", criterion=criterion, n_pca=n_pca, k=list(ks), WSS=wss, AIC=base + 2 * kv,
                           BIC=base + math.log(n) * kv, groups={kk: labels[:, r] + 1 for r, kk in enumerate(ks)},
                           merge=tree["merge"], height=np.sqrt(tree["height"]))
    return out


def _ward_d_two_groups(x: np.ndarray) -> np.ndarray:
    """cutree(hclust(dist(x), method = "ward.D"), k = 2) of scalars: agglomeration by the Lance-Williams update of Ward's
    criterion on the plain distances until two clusters are left; the closest pair merges, on a tie the first pair in the order
    (i, j), i < j, i ascending then j.  -> 1 / 2 per value, group 1 the one that holds the first value"""
    L = len(x)
    if L < 2:
        raise ValueError("the series is too short to be cut in two groups")
    D = np.abs(x[:, None] - x[None, :]).astype(np.float64)
    size, alive, member = np.ones(L), list(range(L)), [[i] for i in range(L)]
    while len(alive) > 2:
        bi = bj = -1
        best = np.inf
        for a in range(len(alive)):
            for b in range(a + 1, len(alive)):
                if D[alive[a], alive[b]] < best:
                    best, bi, bj = D[alive[a], alive[b]], alive[a], alive[b]
        for kx in alive:
            if kx != bi and kx != bj:
                tot = size[bi] + size[bj] + size[kx]
                D[bi, kx] = D[kx, bi] = ((size[bi] + size[kx]) * D[bi, kx] + (size[bj] + size[kx]) * D[bj, kx] - size[kx] * D[bi, bj]) / tot
        size[bi] += size[bj]
        member[bi] += member[bj]
        alive.remove(bj)
    out = np.zeros(L, dtype=np.int64)
    first = alive[0] if 0 in member[alive[0]] else alive[1]
    for a in alive:
        out[member[a]] = 1 if a == first else 2
    return out


def gt_cluster_pca_best_k(x: dict, stat: str = "BIC", criterion: str = "diffNgroup") -> dict:
    """R/gt_cluster_pca_best_k.R:102-166, the five criteria with their quirks: best_k is the 1-based POSITION in clusters["k"] as
    in R (the k itself when the range starts at 1); "goodfit" subtracts 1 from it; "goesup" / "smoothNgoesup" on a series that
    never goes up is an error.  -> x plus best_k"""
    if "clusters" not in x:
        raise ValueError("'x' should be a 'gt_cluster_pca' object generated with 'gt_cluster_pca()'")
    if stat not in ("BIC", "AIC", "WSS"):
        raise ValueError("'stat' should be one of 'BIC', 'AIC', 'WSS'")
    s = np.asarray(x["clusters"][stat], dtype=np.float64)

    def first_rise(v):
        up = np.nonzero(np.diff(v) > 0)[0]
        if len(up) == 0:
            raise ValueError(f"{stat} never goes up over the k that were tested")
        return int(up[0]) + 1

    if criterion == "min":
        n_clust = int(np.argmin(s)) + 1
    elif criterion == "goesup":
        n_clust = first_rise(s)
    elif criterion == "goodfit":
        below = np.nonzero(s < s.min() + 0.1 * (s.max() - s.min()))[0]
        if len(below) == 0:
            raise ValueError(f"{stat} is constant over the k that were tested")
        n_clust = int(below[0]) + 1 - 1
    elif criterion == "diffNgroup":
        df = np.diff(s)
        grp = _ward_d_two_groups(df)
        means = [df[grp == 1].mean(), df[grp == 2].mean()]
        good = 1 if means[0] <= means[1] else 2
        n_clust = int(np.nonzero(grp == good)[0].max()) + 1 + 1
    elif criterion == "smoothNgoesup":
        if len(s) < 3:
            raise ValueError("the series is too short to be smoothed")
        t = s.copy()
        t[1:-1] = (s[:-2] + s[1:-1] + s[2:]) / 3.0
        n_clust = first_rise(t)
    else:
        raise ValueError("'criterion' should be one of 'diffNgroup', 'min', 'goesup', 'smoothNgoesup', 'goodfit'")
    out = dict(x)
    out["best_k"] = n_clust
    return out


def lda(X, grp, n_da: Optional[int] = None) -> dict:
    """tpg_lda (host only): the discriminant analysis of include/tpg.h "DAPC" of n x d scores by the 0-based groups grp ->
    dict(prior, means (G x d), mu, scaling (d x L), svd (L), n_da, ind_coord (n x n_da), grp_coord (G x n_da), posterior (n x G),
    assign (0-based))"""
    x = _scores(X)
    n, d = x.shape
    g = np.ascontiguousarray(grp, dtype=np.int32)
    if g.shape != (n,):
        raise ValueError(f"grp must hold {n} labels")
    G = int(g.max()) + 1 if n else 0
    lmax = max(min(d, G - 1), 1)
    prior, means, mu = np.zeros(max(G, 1)), np.zeros((max(G, 1), max(d, 1)), order="F"), np.zeros(max(d, 1))
    scaling, svd = np.zeros((max(d, 1), lmax), order="F"), np.zeros(lmax)
    ind, gc = np.zeros((max(n, 1), lmax), order="F"), np.zeros((max(G, 1), lmax), order="F")
    post, assign = np.zeros((max(n, 1), max(G, 1)), order="F"), np.zeros(max(n, 1), dtype=np.int32)
    L, nda = C.c_int32(), C.c_int32()
    check(lib.tpg_lda(_ptr(x), n, d, _ptr(g), G, lmax if n_da is None else int(n_da), _ptr(prior), _ptr(means), _ptr(mu), _ptr(scaling),
                      _ptr(svd), C.byref(L), C.byref(nda), _ptr(ind), _ptr(gc), _ptr(post), _ptr(assign)))
    L, nda = L.value, nda.value
    return dict(prior=prior, means=means, mu=mu, scaling=scaling[:, :L], svd=svd[:L], n_da=nda, ind_coord=ind[:, :nda],
                grp_coord=gc[:, :nda], posterior=post, assign=assign)


def dapc_var_contr(V, loadings, ctx: Optional[Context] = None) -> dict:
    """tpg_dapc_var_contr: var_load = V loadings (V m x n_pca, loadings n_pca x n_da) and var_contr, its squares over the
    column's sum of squares (a column whose sum is below 1e-12: zeros)"""
    ctx = ctx or default_context()
    v, ld = _scores(V), _scores(loadings)
    m, n_pca = v.shape
    if ld.shape[0] != n_pca:
        raise ValueError(f"loadings must have {n_pca} rows, not {ld.shape[0]}")
    n_da = ld.shape[1]
    vl, vc = np.zeros((max(m, 1), max(n_da, 1)), order="F"), np.zeros((max(m, 1), max(n_da, 1)), order="F")
    check(lib.tpg_dapc_var_contr(ctx.h, _ptr(v), m, m, n_pca, _ptr(ld), n_da, _ptr(vl), _ptr(vc)))
    return dict(var_load=vl, var_contr=vc)


def gt_dapc(x: dict, pop=None, n_pca: Optional[int] = None, n_da: Optional[int] = None, loadings_by_locus: bool = True,
            ctx: Optional[Context] = None) -> dict:
    """R/gt_dapc.R:122-260 with the discriminant analysis of include/tpg.h "DAPC" in place of MASS::lda / predict.  pop: None (the
    groups of x["best_k"], a position in clusters["k"] as in R), a vector of n labels, or a number (that position in
    clusters["k"]).  -> dict with the reference's names: n.pca, n.da, tab, grp (the labels), var, eig, loadings, means, ind.coord,
    grp.coord, prior, posterior, assign (a label per individual) and, with loadings_by_locus, var.contr and var.load."""
    if x.get("center") is None:
        raise ValueError("'x' was run without centering; centering is necessary for 'gt_dapc'")
    u, dd = np.asarray(x["u"], dtype=np.float64), np.asarray(x["d"], dtype=np.float64)
    clustered = "clusters" in x
    if pop is None:
        if not clustered or x.get("best_k") is None:
            raise ValueError("if 'pop' is not set, 'x' should be a 'gt_cluster_pca'")
        pop = x["best_k"]
    if np.ndim(pop) == 0:
        if not (clustered and isinstance(pop, (int, np.integer))):
            raise ValueError("x does not include pre-defined populations, and `pop' is not provided")
        ks = x["clusters"]["k"]
        if not 1 <= int(pop) <= len(ks):
            raise ValueError(f"pop = {pop} is not a position in the k that were tested")
        grp = np.asarray(x["clusters"]["groups"][ks[int(pop) - 1]])
    else:
        grp = np.asarray(pop)
    if grp.shape != (u.shape[0],):
        raise ValueError(f"pop must hold {u.shape[0]} labels")
    levels, g0 = np.unique(grp, return_inverse=True)
    n_pop = len(levels)
    if n_pca is None:
        n_pca = x["clusters"]["n_pca"] if clustered else len(dd)
        if n_pca > n_pop:
            n_pca = n_pop - 1
    else:
        n_pca = min(int(n_pca), u.shape[1])
    if n_pca < 1:
        raise ValueError("n_pca must be at least 1")
    tab = np.asfortranarray((u * dd[None, :])[:, :n_pca])
    r = lda(tab, g0, None if n_da is None else int(round(n_da)))
    nda = r["n_da"]
    res = {"n.pca": n_pca, "n.da": nda, "tab": tab, "grp": grp, "var": float(dd[:n_pca].sum() / dd.sum()), "eig": r["svd"] ** 2,
           "loadings": np.asfortranarray(r["scaling"][:, :nda]), "means": r["means"], "ind.coord": r["ind_coord"],
           "grp.coord": r["grp_coord"], "prior": r["prior"], "posterior": r["posterior"], "assign": levels[r["assign"]],
           "levels": levels}
    if loadings_by_locus:
        vc = dapc_var_contr(np.asarray(x["v"])[:, :n_pca], res["loadings"], ctx=ctx)
        res["var.contr"], res["var.load"] = vc["var_contr"], vc["var_load"]
    return res


def predict_gt_dapc(dapc: dict, scores_new) -> dict:
    """predict() of a gt_dapc result for new individuals, include/tpg.h "DAPC": scores_new holds their PCA scores (the output of
    predict_gt_pca / predict_gt_pca_oadp on the PCA the DAPC was built on), of which the first dapc["n.pca"] columns are used
    -> dict(ind.coord (n x n.da), posterior (n x G), assign (a label of dapc["levels"] per individual)).  Host arithmetic on what
    gt_dapc returned: mu = sum_g prior_g means_g (g ascending), z = (x - mu) loadings, m_g = (means_g - mu) loadings,
    q_ig = |z_i - m_g|^2 / 2 - ln prior_g, the posterior exp(-(q_ig - min_g q_ig)) normalised, the smallest q (smaller g on a tie)
    assigned."""
    x = np.asarray(scores_new, dtype=np.float64)
    n_pca = int(dapc["n.pca"])
    if x.ndim != 2 or x.shape[1] < n_pca:
        raise ValueError(f"scores_new must be a matrix with at least n.pca = {n_pca} columns")
    x = x[:, :n_pca]
    prior, means = np.asarray(dapc["prior"], dtype=np.float64), np.asarray(dapc["means"], dtype=np.float64)
    S = np.asarray(dapc["loadings"], dtype=np.float64)
    G = len(prior)
    if means.shape != (G, n_pca) or S.shape[0] != n_pca:
        raise ValueError("dapc is not the result of gt_dapc: prior, means and loadings do not fit n.pca")
    mu = np.zeros(n_pca)
    for g in range(G):
        mu += prior[g] * means[g]
    z = (x - mu[None, :]) @ S
    mg = (means - mu[None, :]) @ S
    q = 0.5 * ((z[:, None, :] - mg[None, :, :]) ** 2).sum(axis=2) - np.log(prior)[None, :]
    best = np.argmin(q, axis=1)  # (the first of equal minima: the smaller g)
    post = np.exp(-(q - q[np.arange(len(q)), best][:, None])) if len(q) else np.zeros((0, G))
    post /= post.sum(axis=1, keepdims=True)
    return {"ind.coord": np.asfortranarray(z), "posterior": np.asfortranarray(post), "assign": np.asarray(dapc["levels"])[best]}


def _pbs_triplets(ngroups):
    """utils::combn(levels, 3) order, with the Fst columns of (p1.p2, p1.p3, p2.p3) in combn(levels, 2) order"""
    pairs = combn2(ngroups)  # (2, P), 1-based
    col = {(int(a), int(b)): k for k, (a, b) in enumerate(pairs.T)}
    trips, cols = [], []
    for a in range(1, ngroups + 1):
        for b in range(a + 1, ngroups + 1):
            for c in range(b + 1, ngroups + 1):
                trips.append((a, b, c))
                cols.append((col[(a, b)], col[(a, c)], col[(b, c)]))
    return trips, np.ascontiguousarray(cols, dtype=np.int32)


def _pbs_names(trips):
    """the six columns of every triplet, as R/nwise_pop_pbs.R names them"""
    names = []
    for (a, b, c) in trips:
        for stat in ("pbs", "pbsn1"):
            names += [f"{stat}_{a}.{b}.{c}", f"{stat}_{b}.{a}.{c}", f"{stat}_{c}.{a}.{b}"]
    return names


def nwise_pop_pbs(X: FBM, ind_row, ind_col, groupIds, ngroups: int, ploidy=None, fst_method: str = "Hudson",
                  return_fst: bool = False):
    """R/nwise_pop_pbs.R:36-156, type = "matrix": by-locus PBS and normalised PBS for every triplet of populations.
    -> dict(pbs (m, 6 * n_triplets), names, [fst (m, P)]); the by-locus Fst matrix stays in HBM in between."""
    if ngroups < 3:
        raise ValueError("At least 3 populations are required to compute PBS.")
    if not isinstance(return_fst, (bool, np.bool_)):
        raise ValueError("return_fst must be a logical value (TRUE or FALSE)")
    if fst_method not in FST_METHODS:
        raise ValueError("'arg' should be one of 'Hudson', 'Nei87', 'WC84'")
    v = View(X, ind_row, ind_col)
    pairs_c = np.ascontiguousarray(combn2(ngroups).T)
    P = pairs_c.shape[0]
    trips, tcols = _pbs_triplets(ngroups)
    gid, pl = _i32(groupIds), _ploidy(v, ploidy)
    ctx = v.ctx
    tot = np.zeros(P)
    d_fst = ctx.dev_alloc(8 * v.m * P)
    try:
        check(lib.tpg_pairwise_pop_fst(ctx.h, v.h, _ptr(gid), ngroups, _ptr(pl), FST_METHODS[fst_method],
                                       _ptr(pairs_c), P, 1, 0, _ptr(tot), d_fst, None))
        out = np.zeros((v.m, 6 * len(trips)), order="F")
        check(lib.tpg_pbs_from_fst(ctx.h, d_fst, v.m, P, _ptr(tcols), len(trips), _ptr(out)))
        res = dict(pbs=out)
        if return_fst:
            f = np.zeros((v.m, P), order="F")
            check(lib.tpg_dev_to_host(ctx.h, _ptr(f), d_fst, f.nbytes))
            res["fst"] = f
    finally:
        ctx.dev_free(d_fst)
    res["names"] = _pbs_names(trips)
    return res


def _fst_loop(method, pairwise_combn, n, freq_alt, freq_ref, het_obs, by_locus, return_num_dem, ctx):
    ctx = ctx or default_context()
    pairs_c = np.ascontiguousarray(np.asarray(pairwise_combn, dtype=np.int32).T)
    P = pairs_c.shape[0]
    n = np.asfortranarray(n, dtype=float)
    m, G = n.shape
    mats = [None if x is None else np.asfortranarray(x, dtype=float) for x in (freq_alt, freq_ref, het_obs)]
    tot, a, b = _fst_outputs(m, P, by_locus or return_num_dem, return_num_dem)
    check(lib.tpg_pairwise_fst_loop(ctx.h, FST_METHODS[method], _ptr(pairs_c), P, m,
                                    G, _ptr(n), *[_ptr(x) for x in mats], int(by_locus),
                                    int(return_num_dem), _ptr(tot), _ptr(a), _ptr(b)))
    return _fst_result(tot, a, b, by_locus or return_num_dem, return_num_dem)


def pairwise_fst_hudson_loop(pairwise_combn, n, freq_alt, freq_ref, by_locus=False, return_num_dem=False, ctx=None):
    """src/pairwise_fst_hudson_loop.cpp:5-63"""
    return _fst_loop("Hudson", pairwise_combn, n, freq_alt, freq_ref, None, by_locus, return_num_dem, ctx)


def pairwise_fst_wc84_loop(pairwise_combn, n, freq_alt, het_obs, by_locus=False, return_num_dem=False, ctx=None):
    """src/pairwise_fst_wc84_loop.cpp:5-121"""
    return _fst_loop("WC84", pairwise_combn, n, freq_alt, None, het_obs, by_locus, return_num_dem, ctx)


def pairwise_fst_nei87_loop(pairwise_combn, n, het_obs, freq_alt, freq_ref, by_locus=False, return_num_dem=False,
                            ctx=None):
    """src/pairwise_fst_nei87_loop.cpp:5-115"""
    return _fst_loop("Nei87", pairwise_combn, n, freq_alt, freq_ref, het_obs, by_locus, return_num_dem, ctx)


# ---------------------------------------------------------------------------
# PCA

def pca_center_scale(v: View):
    center, scale = np.zeros(v.m), np.zeros(v.m)
    check(lib.tpg_pca_center_scale(v.ctx.h, v.h, _ptr(center), _ptr(scale)))
    return center, scale


def pca_gram(v: View, center, scale) -> np.ndarray:
    K = np.zeros((v.n, v.n), order="F")
    center, scale = _f64(center), _f64(scale)
    check(lib.tpg_pca_gram(v.ctx.h, v.h, _ptr(center), _ptr(scale), _ptr(K)))
    return K


def sym_eig_topk(K, k: int, ctx: Optional[Context] = None):
    """top-k eigenpairs (descending) of a symmetric PSD matrix: (lambda[k], U n x k)"""
    ctx = ctx or default_context()
    K = np.asfortranarray(K, dtype=float)
    n = K.shape[0]
    lam, U = np.zeros(k), np.zeros((n, k), order="F")
    check(lib.tpg_sym_eig_topk(ctx.h, _ptr(K), n, k, _ptr(lam), _ptr(U)))
    return lam, U


def pca_loadings(v: View, center, scale, U, d) -> np.ndarray:
    """v = Z'u/d for the loci of the view (second sweep of big_SVD)"""
    center, scale, d = _f64(center), _f64(scale), _f64(d)
    U = np.asfortranarray(U, dtype=float)
    k = U.shape[1]
    out = np.zeros((v.m, k), order="F")
    check(lib.tpg_pca_loadings(v.ctx.h, v.h, _ptr(center), _ptr(scale), _ptr(U), _ptr(d), k, _ptr(out)))
    return out


def _pca_view(X: FBM, ind_row, ind_col, code256, impute, impute_seed) -> View:
    """the view a PCA reads: through code256, or -- impute = "mode" | "mean0" | "random" -- the raw view with its missing
    genotypes filled from the kept rows (View.impute; the store itself is not changed)"""
    if impute is None:
        return View(X, ind_row, ind_col, code256=code256)
    return View(X, ind_row, ind_col, code256=CODE_012).impute(impute, impute_seed)


def gt_pca_partialSVD(X: FBM, ind_row=None, ind_col=None, k: int = 10, total_var: bool = True,
                      code256=CODE_IMPUTE_PRED, impute: Optional[str] = None, impute_seed: int = 0) -> dict:
    """R/gt_pca_partialSVD.R:67-108: the imputed code table is switched on (:74-77), then
    bigstatsr::big_SVD with bigsnpr::snp_scaleBinom."""
    v = _pca_view(X, ind_row, ind_col, code256, impute, impute_seed)
    d = np.zeros(k)
    u = np.zeros((v.n, k), order="F")
    vl = np.zeros((v.m, k), order="F")
    center, scale = np.zeros(v.m), np.zeros(v.m)
    fro = C.c_double()
    check(lib.tpg_pca_partial_svd(v.ctx.h, v.h, k, _ptr(d), _ptr(u), _ptr(vl), _ptr(center), _ptr(scale),
                                  C.byref(fro) if total_var else None))
    out = dict(d=d, u=u, v=vl, center=center, scale=scale, method="partialSVD")
    if total_var:
        out["square_frobenius"] = fro.value
    return out


# ---------------------------------------------------------------------------
# pcadapt (include/tpg.h "pcadapt")

# keys per candidate list of the selection kernel (the tests put their row counts around it)
SELECT_TILE = int(lib.tpg_select_tile())


def col_median_mad(X, ctx: Optional[Context] = None, return_counts: bool = False):
    """tpg_col_median_mad: exact median and MAD (unscaled) of the finite entries of every column of X (rows x ncols; a
    Fortran-ordered array is read in place, and a view X = A[:rows, :] of a taller Fortran array goes down with its leading
    dimension).  -> (med, mad[, n_finite])"""
    ctx = ctx or default_context()
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be a matrix with at least one row and one column")
    if not (X.flags.f_contiguous or (X.strides[0] == 8 and X.strides[1] % 8 == 0 and X.strides[1] >= 8 * X.shape[0])):
        X = np.asfortranarray(X)
    rows, ncols = X.shape
    ld = X.strides[1] // 8 if ncols > 1 else rows
    med, mad, cnt = np.zeros(ncols), np.zeros(ncols), np.zeros(ncols, dtype=np.int64)
    check(lib.tpg_col_median_mad(ctx.h, _ptr(X), rows, ncols, ld, _ptr(med), _ptr(mad), _ptr(cnt)))
    return (med, mad, cnt) if return_counts else (med, mad)


def pcadapt_zscores(v: View, U, return_n_valid: bool = False):
    """tpg_pcadapt_zscores: the m x K z-scores of the regression of every locus on the columns of U (n x K, orthonormal); an
    invalid locus (monomorphic, or no residual variance) is a row of NaN"""
    U = np.asfortranarray(U, dtype=np.float64)
    if U.ndim != 2 or U.shape[0] != v.n:
        raise ValueError(f"U must have {v.n} rows, not shape {U.shape}")
    K = U.shape[1]
    z = np.zeros((v.m, max(K, 1)), order="F")
    nv = C.c_int64()
    check(lib.tpg_pcadapt_zscores(v.ctx.h, v.h, _ptr(U), K, _ptr(z), C.byref(nv)))
    return (z, int(nv.value)) if return_n_valid else z


def robust_dist_ogk(Z, return_basis: bool = False, ctx: Optional[Context] = None) -> dict:
    """tpg_robust_dist_ogk: the robust squared Mahalanobis distance of the rows of Z (m x K) from an OGK location / scatter
    with median and MAD.  -> dict(dist, center, cov, n_valid[, basis = (2, K, K): the eigenvectors of the two iterations])"""
    ctx = ctx or default_context()
    Z = np.asfortranarray(Z, dtype=np.float64)
    if Z.ndim != 2:
        raise ValueError("Z must be a matrix")
    m, K = Z.shape
    dist, center, cov = np.zeros(m), np.zeros(max(K, 1)), np.zeros((max(K, 1), max(K, 1)), order="F")
    basis = np.zeros(2 * max(K, 1) ** 2)
    nv = C.c_int64()
    check(lib.tpg_robust_dist_ogk(ctx.h, _ptr(Z), m, K, _ptr(dist), _ptr(center), _ptr(cov), _ptr(basis), C.byref(nv)))
    out = dict(dist=dist, center=center, cov=cov, n_valid=int(nv.value))
    if return_basis:
        out["basis"] = np.stack([basis[:K * K].reshape((K, K), order="F"), basis[K * K:].reshape((K, K), order="F")])
    return out


def pchisq_log10_upper(x, df: int, ctx: Optional[Context] = None) -> np.ndarray:
    """log10 of the upper tail of chi-square(df) at x: finite where the tail itself underflows"""
    ctx = ctx or default_context()
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros(x.shape)
    check(lib.tpg_pchisq_log10_upper(ctx.h, _ptr(x), x.size, int(df), _ptr(out)))
    return out


def qchisq_median(df: int) -> float:
    """the median of chi-square(df) (host only)"""
    out = C.c_double()
    check(lib.tpg_qchisq_median(int(df), C.byref(out)))
    return out.value


def pcadapt(v: View, U, return_zscores: bool = False) -> dict:
    """tpg_pcadapt: z-scores, robust distance, genomic control and log10 p-values in one call"""
    U = np.asfortranarray(U, dtype=np.float64)
    if U.ndim != 2 or U.shape[0] != v.n:
        raise ValueError(f"U must have {v.n} rows, not shape {U.shape}")
    K = U.shape[1]
    z = np.zeros((v.m, max(K, 1)), order="F") if return_zscores else None
    dist, stat, lp = np.zeros(v.m), np.zeros(v.m), np.zeros(v.m)
    lam, nv = C.c_double(), C.c_int64()
    check(lib.tpg_pcadapt(v.ctx.h, v.h, _ptr(U), K, _ptr(z), _ptr(dist), _ptr(stat), _ptr(lp), C.byref(lam), C.byref(nv)))
    out = dict(dist=dist, stat=stat, log10_p=lp, gc_lambda=lam.value, n_valid=int(nv.value))
    if return_zscores:
        out["zscores"] = z
    return out


def gt_pcadapt(X: FBM, pca: dict, k, ind_row=None, ind_col=None, impute: Optional[str] = None, impute_seed: int = 0,
               return_zscores: bool = False) -> dict:
    """R/gt_pcadapt.R:44-86: a genome scan for selection on the first k components of `pca` (a gt_pca_* result: its "u").
    As the reference, k must be a scalar no larger than the number of components in pca, and the genotypes must have no
    missing value (impute = "mode" | "mean0" | "random" fills them from the kept rows first, as in the PCA).
    -> dict(score (= dist / gc_lambda), dist, log10_p, p, gc_lambda, n_valid[, zscores])"""
    if np.ndim(k) != 0 or isinstance(k, (bool, np.bool_)) or int(k) != k:
        raise ValueError("'k' should be a single integer value")
    k = int(k)
    u = np.asarray(pca["u"], dtype=np.float64)
    if k > u.shape[1]:
        raise ValueError("K is too large: 'k' should not be larger than the number of components in 'x'")
    if k < 1:
        raise ValueError("'k' should be a single integer value")
    v = _pca_view(X, ind_row, ind_col, CODE_IMPUTE_PRED, impute, impute_seed)
    r = pcadapt(v, u[:, :k], return_zscores=return_zscores)
    out = dict(score=r["stat"], dist=r["dist"], log10_p=r["log10_p"], p=np.power(10.0, r["log10_p"]), gc_lambda=r["gc_lambda"],
               n_valid=r["n_valid"])
    if return_zscores:
        out["zscores"] = r["zscores"]
    return out


def ld_window_hi(chromosome, position=None, size=500.0, use_positions: bool = True, m: Optional[int] = None,
                 check_runs: bool = True) -> np.ndarray:
    """the window of include/tpg.h "LD clumping": hi[j] = last locus (0-based) that is a neighbour of j.  With positions,
    neighbours are loci of the same chromosome with |position difference| <= size * 1000; without, loci of the same
    chromosome with |index difference| <= size.  Loci must be ordered: every chromosome one contiguous run, positions
    non-decreasing inside it (is_loci_table_ordered stops the reference otherwise).  chromosome = None: one chromosome.
    check_runs = False leaves the check of the runs to the callee (gt_pca_autoSVD: the library refuses them)."""
    if chromosome is None:
        if m is None:
            m = len(position)
        chrom = np.zeros(m, dtype=np.int64)
    else:
        chrom = np.unique(np.asarray(chromosome), return_inverse=True)[1].astype(np.int64).ravel()
    m = len(chrom)
    starts = np.r_[0, np.flatnonzero(chrom[1:] != chrom[:-1]) + 1, m] if m else np.array([0, 0])
    if check_runs and len(np.unique(chrom[starts[:-1]])) != len(starts) - 1:
        raise ValueError("loci are not ordered: a chromosome appears in more than one run")
    hi = np.empty(m, dtype=np.int64)
    if use_positions:
        if position is None:
            raise ValueError("use_positions = True needs the positions of the loci")
        pos = np.asarray(position, dtype=np.float64)
        if len(pos) != m:
            raise ValueError("chromosome and position differ in length")
    for a, b in zip(starts[:-1], starts[1:]):
        if use_positions:
            p = pos[a:b]
            if np.any(p[1:] < p[:-1]):
                raise ValueError("loci are not ordered: positions decrease inside a chromosome")
            hi[a:b] = a + np.searchsorted(p, p + float(size) * 1000.0, side="right") - 1
        else:
            hi[a:b] = np.minimum(np.arange(a, b) + int(math.floor(size)), b - 1)
    return hi


def _ld_hi(v: View, hi) -> np.ndarray:
    hi = np.ascontiguousarray(hi, dtype=np.int64)
    if hi.shape != (v.m,):
        raise ValueError("hi must have one entry per locus of the view")
    return hi


def ld_band_links(v: View, hi, thr_r2: float = 0.2, return_links: bool = False):
    """tpg_ld_band_links: the link relation of neighbouring loci as a bit band, (m, stride) uint32: bit b of row j <->
    locus j + 1 + b is linked to j (include/tpg.h "LD clumping")"""
    hi = _ld_hi(v, hi)
    width = int((hi - np.arange(v.m)).max(initial=0))
    bits = np.zeros((v.m, max(1, -(-width // 32))), dtype=np.uint32)
    links = C.c_int64()
    check(lib.tpg_ld_band_links(v.ctx.h, v.h, _ptr(hi), thr_r2, _ptr(bits), bits.shape[1], C.byref(links)))
    return (bits, int(links.value)) if return_links else bits


def ld_clump(v: View, hi, thr_r2: float = 0.2, S=None, exclude=None, return_report: bool = False):
    """tpg_ld_clump on a view without missing genotypes: keep (m,) bool; exclude = (m,) 0 / 1"""
    hi = _ld_hi(v, hi)
    s = _f64(S)
    ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint8)
    if (s is not None and s.shape != (v.m,)) or (ex is not None and ex.shape != (v.m,)):
        raise ValueError("S and exclude must have one entry per locus of the view")
    keep = np.zeros(v.m, dtype=np.uint8)
    rep = _lib.LdReport()
    check(lib.tpg_ld_clump(v.ctx.h, v.h, _ptr(hi), thr_r2, _ptr(s), _ptr(ex), _ptr(keep), C.byref(rep)))
    keep = keep.astype(bool)
    if return_report:
        return keep, {f: int(getattr(rep, f)) for f, _ in _lib.LdReport._fields_}
    return keep


def loci_ld_clump(X: FBM, ind_row=None, ind_col=None, S=None, thr_r2: float = 0.2, size=None, chromosome=None,
                  position=None, use_positions: bool = True, exclude=None, return_id: bool = False,
                  impute: Optional[str] = None, impute_seed: int = 0):
    """R/loci_ld_clump.R:84-184 (around bigsnpr::snp_clumping; the definition is include/tpg.h "LD clumping"): loci are
    walked by decreasing S (default: minor allele frequency), a locus still standing is kept and removes its neighbours with
    r^2 > thr_r2.  chromosome / position describe the loci of ind_col, in order; without positions pass
    use_positions = False.  exclude = 1-based indices of loci never to keep.  A missing genotype is an error, as in the
    reference, unless impute = "mode" | "mean0" | "random" fills the view first (as for the PCA).  Returns a boolean per
    locus, or with return_id the 1-based indices of the kept loci."""
    if size is None:
        size = 100.0 / thr_r2
    v = _pca_view(X, ind_row, ind_col, "fbm", impute, impute_seed)
    if use_positions and position is None:
        raise ValueError("use_positions = TRUE needs positions; pass use_positions=False to count in loci")
    hi = ld_window_hi(chromosome, position, size, use_positions, m=v.m)
    if len(hi) != v.m:
        raise ValueError("chromosome / position must describe every locus of ind_col")
    ex = None
    if exclude is not None and len(exclude) > 0:
        e = np.asarray(exclude, dtype=np.int64)
        if e.min() < 1 or e.max() > v.m:
            raise ValueError("exclude out of range")
        ex = np.zeros(v.m, dtype=np.uint8)
        ex[e - 1] = 1
    keep = ld_clump(v, hi, thr_r2, S, ex)
    return np.flatnonzero(keep) + 1 if return_id else keep


# ---------------------------------------------------------------------------
# LD statistics (include/tpg.h "LD statistics")

LD_Q_ONE = 1 << 30          # the fixed point of every sum of r^2: q = floor(r2 * 2^30 + 0.5)
LD_MAX_BINS = 4096          # HOST_LDSTAT_MAX_BINS
LD_REGION_MAX_LOCI = 4096   # ld_region_r2: 4096 x 4095 values stay under the 2^26 of tpg_ld_band_r2


def _ld_positions(v: View, position):
    """positions as the int64 the library takes (None stays None); a fractional position is an error, not a rounding"""
    if position is None:
        return None
    p = np.asarray(position)
    if p.shape != (v.m,):
        raise ValueError("position must have one entry per locus of the view")
    if p.dtype.kind == "f":
        if not np.all(np.isfinite(p)) or np.any(p != np.floor(p)):
            raise ValueError("positions must be whole numbers")
    elif p.dtype.kind not in "iu":
        raise ValueError("positions must be numbers")
    return np.ascontiguousarray(p, dtype=np.int64)


def ld_stats(v: View, hi, position=None, bin_size: int = 1, n_bins: int = 0, scores: bool = True) -> dict:
    """tpg_ld_stats on a view without missing genotypes, the raw integers: with scores "score_q" (m,) uint64 and "n_partners"
    (m,) int32; with n_bins != 0 "bin_pairs" (n_bins,) int64, "bin_sum_q" uint64 and "bin_sum_dist" int64 over the distances
    position[k] - position[j] (k - j without positions); always "report" = {pairs, pairs_valid, pairs_beyond, band_tiles}.
    r^2 sums are score_q / LD_Q_ONE."""
    hi = _ld_hi(v, hi)
    n_bins = int(n_bins)
    pos = _ld_positions(v, position) if n_bins != 0 else None
    out = {}
    sq = npart = bp = bq = bd = None
    if scores:
        sq, npart = np.zeros(v.m, dtype=np.uint64), np.zeros(v.m, dtype=np.int32)
    if n_bins != 0:  # (a count the library refuses still reaches it: the arrays only have to exist)
        bp, bq, bd = (np.zeros(max(n_bins, 1), dtype=t) for t in (np.int64, np.uint64, np.int64))
    rep = _lib.LdStatReport()
    check(lib.tpg_ld_stats(v.ctx.h, v.h, _ptr(hi), _ptr(pos), int(bin_size), n_bins, _ptr(sq), _ptr(npart), _ptr(bp), _ptr(bq),
                           _ptr(bd), C.byref(rep)))
    if scores:
        out.update(score_q=sq, n_partners=npart)
    if n_bins != 0:
        out.update(bin_pairs=bp, bin_sum_q=bq, bin_sum_dist=bd)
    out["report"] = {f: int(getattr(rep, f)) for f, _ in _lib.LdStatReport._fields_}
    return out


def ld_band_r2(v: View, hi, j0: int, j1: int) -> np.ndarray:
    """tpg_ld_band_r2: r^2 of the loci j0 <= j < j1 (0-based) with the loci behind them in the window, (j1 - j0, stride)
    float64 with entry [j - j0, b] = r^2 of (j, j + 1 + b); NaN outside the window and for a pair with a monomorphic locus;
    stride = the widest window of the region (at least 1)"""
    hi = _ld_hi(v, hi)
    j0, j1 = int(j0), int(j1)
    if not 0 <= j0 < j1 <= v.m:
        raise ValueError("[j0, j1) must be a range of the loci of the view")
    stride = max(1, int((hi[j0:j1] - np.arange(j0, j1)).max()))
    r2 = np.zeros((j1 - j0, stride), dtype=np.float64)
    check(lib.tpg_ld_band_r2(v.ctx.h, v.h, _ptr(hi), j0, j1, _ptr(r2), stride))
    return r2


def ld_region_r2(X: FBM, j0: int, j1: int, ind_row=None, ind_col=None, impute: Optional[str] = None, impute_seed: int = 0) -> np.ndarray:
    """the r^2 matrix of the loci j0 <= j < j1 (0-based positions in ind_col; at most LD_REGION_MAX_LOCI of them) for a
    heatmap: symmetric (j1 - j0, j1 - j0) float64, diagonal 1; the row and column of a monomorphic locus are NaN, diagonal
    included.  A missing genotype is an error unless impute = "mode" | "mean0" | "random" fills the view first."""
    v = _pca_view(X, ind_row, ind_col, "fbm", impute, impute_seed)
    j0, j1 = int(j0), int(j1)
    if not 0 <= j0 < j1 <= v.m:
        raise ValueError("[j0, j1) must be a range of the loci of ind_col")
    r = j1 - j0
    if r > LD_REGION_MAX_LOCI:
        raise ValueError(f"a region of {r} loci: at most {LD_REGION_MAX_LOCI}")
    sub = v.select_loci(np.arange(j0, j1))
    band = ld_band_r2(sub, np.full(r, r - 1, dtype=np.int64), 0, r)
    poly = loci_counts(sub)[:, :3].max(axis=1) < sub.n
    sub.free()
    out = np.full((r, r), np.nan)
    a, b = np.triu_indices(r, 1)
    out[a, b] = band[a, b - a - 1]
    out[b, a] = out[a, b]
    out[np.arange(r), np.arange(r)] = np.where(poly, 1.0, np.nan)
    return out


def _ld_stat_view(X, ind_row, ind_col, size, chromosome, position, use_positions, impute, impute_seed):
    """the view and its window, as loci_ld_clump makes them"""
    v = _pca_view(X, ind_row, ind_col, "fbm", impute, impute_seed)
    if use_positions and position is None:
        raise ValueError("use_positions = TRUE needs positions; pass use_positions=False to count in loci")
    hi = ld_window_hi(chromosome, position, size, use_positions, m=v.m)
    if len(hi) != v.m:
        raise ValueError("chromosome / position must describe every locus of ind_col")
    return v, hi


def loci_ld_score(X: FBM, ind_row=None, ind_col=None, size=500.0, chromosome=None, position=None, use_positions: bool = True,
                  adjusted: bool = True, include_self: bool = True, impute: Optional[str] = None, impute_seed: int = 0) -> np.ndarray:
    """the LD score of every locus: the sum of r^2 with the loci of its window (ld_window_hi: size kb either side, or size
    loci with use_positions = False), (m,) float64.  adjusted: every r^2 in its bias-corrected form r^2 - (1 - r^2) / (n - 2),
    the form of LD score regression (Bulik-Sullivan et al. 2015); n < 3 is then an error.  include_self adds the locus's own
    r^2 = 1.  A monomorphic locus has no r^2 with anybody: NaN.  Missing genotypes as in loci_ld_clump."""
    v, hi = _ld_stat_view(X, ind_row, ind_col, size, chromosome, position, use_positions, impute, impute_seed)
    if adjusted and v.n < 3:
        raise ValueError("the adjusted LD score needs at least 3 individuals")
    r = ld_stats(v, hi)
    S = r["score_q"].astype(np.float64) / LD_Q_ONE
    c = r["n_partners"].astype(np.float64)
    score = S - (c - S) / (v.n - 2) if adjusted else S
    if include_self:
        score = score + 1.0
    score[loci_counts(v)[:, :3].max(axis=1) >= v.n] = np.nan
    return score


def _ld_decay_one(v, hi, pos, bin_size, n_bins, adjusted) -> dict:
    r = ld_stats(v, hi, pos, bin_size, n_bins, scores=False)
    npairs = r["bin_pairs"]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_r2 = np.where(npairs > 0, r["bin_sum_q"].astype(np.float64) / LD_Q_ONE / npairs, np.nan)
        mean_dist = np.where(npairs > 0, r["bin_sum_dist"].astype(np.float64) / npairs, np.nan)
    if adjusted:
        mean_r2 = mean_r2 - (1.0 - mean_r2) / (v.n - 2)
    lo = np.arange(n_bins, dtype=np.int64) * int(bin_size)
    return dict(distance_lo=lo, distance_hi=lo + int(bin_size), mean_distance=mean_dist, n_pairs=npairs, mean_r2=mean_r2,
                pairs_beyond=r["report"]["pairs_beyond"])


def ld_decay(X: FBM, ind_row=None, ind_col=None, size=500.0, chromosome=None, position=None, use_positions: bool = True,
             bin_size: Optional[int] = None, n_bins: Optional[int] = None, by_chromosome: bool = False, adjusted: bool = False,
             impute: Optional[str] = None, impute_seed: int = 0) -> dict:
    """the LD decay curve: mean r^2 of the pairs of loci inside the window (as loci_ld_score takes it) by distance -- in
    positions with use_positions, else in loci.  Bin b holds the distances [b bin_size, (b + 1) bin_size); bin_size defaults
    to 1000 positions or 1 locus, n_bins to what the window reaches (at most LD_MAX_BINS).  Returns "distance_lo",
    "distance_hi" (exclusive), "mean_distance", "n_pairs", "mean_r2" (NaN for an empty bin; adjusted: in the bias-corrected form
    of loci_ld_score) and "pairs_beyond", the pairs behind the last bin.  by_chromosome: one curve per chromosome, the arrays
    stacked as rows in the order of "chromosome"."""
    v, hi = _ld_stat_view(X, ind_row, ind_col, size, chromosome, position, use_positions, impute, impute_seed)
    if adjusted and v.n < 3:
        raise ValueError("the adjusted r^2 needs at least 3 individuals")
    if bin_size is None:
        bin_size = 1000 if use_positions else 1
    bin_size = int(bin_size)
    if bin_size < 1:
        raise ValueError("bin_size must be at least 1")
    if n_bins is None:
        reach = int(math.floor(float(size) * 1000.0)) if use_positions else int(math.floor(size))
        n_bins = min(LD_MAX_BINS, reach // bin_size + 1)
    n_bins = int(n_bins)
    if not 1 <= n_bins <= LD_MAX_BINS:
        raise ValueError(f"n_bins must lie in [1, {LD_MAX_BINS}]")
    pos = _ld_positions(v, position) if use_positions else None
    if not by_chromosome:
        return _ld_decay_one(v, hi, pos, bin_size, n_bins, adjusted)
    chrom = np.zeros(v.m, dtype=np.int64) if chromosome is None else np.asarray(chromosome)
    starts = np.r_[0, np.flatnonzero(chrom[1:] != chrom[:-1]) + 1, v.m]
    curves = []
    for a, b in zip(starts[:-1], starts[1:]):
        sub = v.select_loci(np.arange(a, b))
        curves.append(_ld_decay_one(sub, hi[a:b] - a, None if pos is None else pos[a:b], bin_size, n_bins, adjusted))
        sub.free()
    out = {k: np.stack([c[k] for c in curves]) for k in curves[0]}
    out["chromosome"] = chrom[starts[:-1]]
    return out


# ---------------------------------------------------------------------------
# autoSVD (include/tpg.h "autoSVD")

TUKEY_REPORT_FIELDS = ("n_finite", "q1", "q3", "med", "mc", "coef", "thr")


def qnorm_upper(p: float) -> float:
    """the upper quantile of the standard normal, the root of 0.5 erfc(x / sqrt 2) = p (host only)"""
    out = C.c_double()
    check(lib.tpg_qnorm_upper(float(p), C.byref(out)))
    return out.value


def rollmean_weights(roll_size: int) -> np.ndarray:
    """the 2 roll_size + 1 Gaussian weights of the rolling mean (host only)"""
    w = np.zeros(2 * max(int(roll_size), 0) + 1)
    check(lib.tpg_rollmean_weights(int(roll_size), _ptr(w)))
    return w


def _chrom_codes(chromosome, m: int) -> np.ndarray:
    if chromosome is None:
        return np.zeros(m, dtype=np.int32)
    chrom = np.unique(np.asarray(chromosome), return_inverse=True)[1].astype(np.int32).ravel()
    if len(chrom) != m:
        raise ValueError("chromosome must describe every locus")
    return chrom


def rollmean(x, chromosome=None, roll_size: int = 50, ctx: Optional[Context] = None) -> np.ndarray:
    """tpg_rollmean_segments: the Gaussian rolling mean of x with radius roll_size inside every run of equal chromosome"""
    ctx = ctx or default_context()
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    chrom = _chrom_codes(chromosome, len(x))
    seg = np.r_[0, np.flatnonzero(chrom[1:] != chrom[:-1]) + 1, len(x)].astype(np.int64)
    out = np.zeros(len(x))
    check(lib.tpg_rollmean_segments(ctx.h, _ptr(x), len(x), _ptr(seg), len(seg) - 1, int(roll_size), _ptr(out)))
    return out


def medcouple(x, ctx: Optional[Context] = None) -> float:
    """tpg_medcouple: the medcouple of the finite values of x, an exact selection on the device"""
    ctx = ctx or default_context()
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    out = C.c_double()
    check(lib.tpg_medcouple(ctx.h, _ptr(x) if len(x) else None, len(x), C.byref(out)))
    return out.value


def tukey_mc_up(x, alpha: float = 0.05, ctx: Optional[Context] = None) -> dict:
    """tpg_tukey_mc_up: the upper Tukey fence of x, corrected for skewness (medcouple) and multiplicity (alpha / count).
    -> dict(n_finite, q1, q3, med, mc, coef, thr)"""
    ctx = ctx or default_context()
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    rep = np.zeros(len(TUKEY_REPORT_FIELDS))
    check(lib.tpg_tukey_mc_up(ctx.h, _ptr(x) if len(x) else None, len(x), float(alpha), _ptr(rep)))
    out = dict(zip(TUKEY_REPORT_FIELDS, rep.tolist()))
    out["n_finite"] = int(out["n_finite"])
    return out


def pca_auto_svd(v: View, chrom, hi=None, k: int = 10, thr_r2: float = 0.2, roll_size: int = 50, alpha_tukey: float = 0.05,
                 min_mac: int = 10, max_iter: int = 5, int_min_size: int = 20) -> dict:
    """tpg_pca_auto_svd on a view: chrom (m,) int32 codes, hi the clumping window of ld_window_hi or None for no clumping.
    -> dict(d, u, v, center, scale, square_frobenius, idx0 (kept loci of the view, 0-based), n_iter, converged,
    history = [dict(n_kept, n_outliers, report, pos0, idx0, intervals = [(first locus, last locus), ...])])"""
    chrom = np.ascontiguousarray(chrom, dtype=np.int32)
    if chrom.shape != (v.m,):
        raise ValueError("chrom must have one entry per locus of the view")
    hi = None if hi is None else _ld_hi(v, hi)
    h = C.c_void_p()
    check(lib.tpg_pca_auto_svd(v.ctx.h, v.h, _ptr(chrom), _ptr(hi), int(k), 0.0 if hi is None else float(thr_r2), int(roll_size),
                               float(alpha_tukey), int(min_mac), int(max_iter), C.byref(h)))
    try:
        mk, iters = int(lib.tpg_autosvd_count(h)), int(lib.tpg_autosvd_iters(h))
        conv = bool(lib.tpg_autosvd_converged(h))
        d, u, vl = np.zeros(k), np.zeros((v.n, k), order="F"), np.zeros((mk, k), order="F")
        center, scale, idx0 = np.zeros(mk), np.zeros(mk), np.zeros(mk, dtype=np.int64)
        fro = C.c_double()
        check(lib.tpg_autosvd_fetch(h, _ptr(d), _ptr(u), _ptr(vl), _ptr(center), _ptr(scale), _ptr(idx0), C.byref(fro)))
        history = []
        for it in range(iters if conv else iters - 1):
            nk, no = C.c_int64(), C.c_int64()
            rep = np.zeros(len(TUKEY_REPORT_FIELDS))
            check(lib.tpg_autosvd_history(h, it, C.byref(nk), C.byref(no), _ptr(rep)))
            pos, oi = np.zeros(no.value, dtype=np.int64), np.zeros(no.value, dtype=np.int64)
            cap = max(1, no.value // max(1, int(int_min_size)))
            first, last, cnt = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64), C.c_int64()
            if no.value:
                check(lib.tpg_autosvd_outliers(h, it, _ptr(pos), _ptr(oi)))
            check(lib.tpg_autosvd_intervals(h, it, int(int_min_size), _ptr(first), _ptr(last), C.byref(cnt)))
            report = dict(zip(TUKEY_REPORT_FIELDS, rep.tolist()))
            report["n_finite"] = int(report["n_finite"])
            history.append(dict(n_kept=int(nk.value), n_outliers=int(no.value), report=report, pos0=pos, idx0=oi,
                                intervals=[(int(a), int(b)) for a, b in zip(first[:cnt.value], last[:cnt.value])]))
    finally:
        lib.tpg_autosvd_free(h)
    return dict(d=d, u=u, v=vl, center=center, scale=scale, square_frobenius=fro.value, idx0=idx0, n_iter=iters, converged=conv,
                history=history)


def gt_pca_autoSVD(X: FBM, ind_row=None, ind_col=None, k: int = 10, thr_r2: Optional[float] = 0.2, use_positions: bool = True,
                   size=None, roll_size: int = 50, int_min_size: int = 20, alpha_tukey: float = 0.05, min_mac: int = 10,
                   max_iter: int = 5, chromosome=None, position=None, total_var: bool = True, impute: Optional[str] = None,
                   impute_seed: int = 0) -> dict:
    """R/gt_pca_autoSVD.R (around bigsnpr::snp_autoSVD; the definition is include/tpg.h "autoSVD"): clump, compute the SVD,
    find the loci whose loadings are outliers in consecutive stretches (long-range LD regions), remove them, repeat until none
    is left or max_iter SVDs have been cleaned.  chromosome / position describe the loci of ind_col, in order.  thr_r2 = None
    skips clumping; size is the clumping window (default 100 / thr_r2: kb with use_positions, loci without).  A missing
    genotype is an error unless impute = "mode" | "mean0" | "random" fills the view first.
    -> dict(d, u, v, center, scale, method = "autoSVD", loci (1-based indices into ind_col of the kept loci), lrldr (only with
    positions: [(chromosome, position of the first, position of the last)] of every run of at least int_min_size outliers,
    accumulated over the iterations), n_iter, converged, history[, square_frobenius])"""
    v = _pca_view(X, ind_row, ind_col, CODE_IMPUTE_PRED, impute, impute_seed)
    chrom = _chrom_codes(chromosome, v.m)
    hi = None
    if thr_r2 is not None:
        if size is None:
            size = 100.0 / thr_r2
        if use_positions and position is None:
            raise ValueError("use_positions = TRUE needs positions; pass use_positions=False to count in loci")
        hi = ld_window_hi(chromosome, position, size, use_positions, m=v.m, check_runs=False)
        if len(hi) != v.m:
            raise ValueError("chromosome / position must describe every locus of ind_col")
    r = pca_auto_svd(v, chrom, hi, k=k, thr_r2=0.0 if thr_r2 is None else thr_r2, roll_size=roll_size, alpha_tukey=alpha_tukey,
                     min_mac=min_mac, max_iter=max_iter, int_min_size=int_min_size)
    out = dict(d=r["d"], u=r["u"], v=r["v"], center=r["center"], scale=r["scale"], method="autoSVD", loci=r["idx0"] + 1,
               n_iter=r["n_iter"], converged=r["converged"], history=r["history"])
    if position is not None:
        pos = np.asarray(position)
        if len(pos) != v.m:
            raise ValueError("position must describe every locus of ind_col")
        names = np.zeros(v.m, dtype=np.int64) if chromosome is None else np.asarray(chromosome)
        out["lrldr"] = [(names[a].item(), pos[a].item(), pos[b].item()) for h in r["history"] for a, b in h["intervals"]]
    if total_var:
        out["square_frobenius"] = r["square_frobenius"]
    return out


# include/tpg.h "Runs of homozygosity": loci per chunk of the status stage (results do not depend on it; the seam tests do)
ROH_CHUNK_LOCI = int(lib.tpg_roh_chunk_loci()) if hasattr(lib, "tpg_roh_chunk_loci") else 0


def _roh_params(window_size=15, threshold=0.05, min_snp=3, heterozygosity=False, max_opp_window=1, max_miss_window=1,
                max_gap=10**6, min_length_bps=1000, min_density=1 / 1000, max_opp_run=None, max_miss_run=None) -> "_lib.RohParams":
    if not 1 <= int(window_size) <= 512:
        raise ValueError("window_size must lie in 1..512")
    if not 0.0 <= float(threshold) <= 1.0:
        raise ValueError("threshold must lie in [0, 1]")
    return _lib.RohParams(int(window_size), float(threshold), int(min_snp), int(bool(heterozygosity)), int(max_opp_window),
                          int(max_miss_window), int(max_gap), int(min_length_bps), float(min_density),
                          -1 if max_opp_run is None else int(max_opp_run), -1 if max_miss_run is None else int(max_miss_run))


def _roh_loci(m: int, chromosome, position):
    """chromosome -> int32 codes (neighbours with equal labels get equal codes), position -> int64; loci must be ordered: positions
    non-decreasing inside a chromosome (neighbours are compared, as include/tpg.h states)"""
    if position is None:
        raise ValueError("runs of homozygosity need the positions of the loci")
    pos = np.ascontiguousarray(position, dtype=np.int64)
    if chromosome is None:
        chrom = np.zeros(len(pos), dtype=np.int32)
    else:
        c = np.asarray(chromosome).ravel()  # only neighbours are compared: the index of the stretch of equal labels will do
        chrom = np.zeros(len(c), dtype=np.int32)
        if len(c) > 1:
            np.cumsum(c[1:] != c[:-1], out=chrom[1:])
    if chrom.shape != (m,) or pos.shape != (m,):
        raise ValueError("chromosome / position must describe every locus of the view")
    if np.any((chrom[1:] == chrom[:-1]) & (pos[1:] < pos[:-1])):
        raise ValueError("loci are not ordered: positions decrease inside a chromosome")
    return chrom, pos


def roh_snp_status(v: View, chromosome, position, stride_words: Optional[int] = None, return_bits: bool = False, **params):
    """tpg_roh_snp_status: is locus j of individual i in a run (step 4 of include/tpg.h "Runs of homozygosity")?  (n, m) bool;
    with return_bits the packed rows as the library wrote them, (n, stride_words) uint32"""
    P = _roh_params(**params)
    chrom, pos = _roh_loci(v.m, chromosome, position)
    stride = -(-v.m // 32) if stride_words is None else int(stride_words)
    bits = np.full((v.n, stride), 0xFFFFFFFF, dtype=np.uint32)  # (every word is written: the library zeroes what it does not use)
    check(lib.tpg_roh_snp_status(v.ctx.h, v.h, _ptr(chrom), _ptr(pos), C.byref(P), _ptr(bits), stride))
    if return_bits:
        return bits
    return np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :v.m].astype(bool)


class Roh:
    """the runs of one tpg_roh_detect call, in device memory until fetched (tpg_roh)"""

    def __init__(self, v: View, chromosome, position, _loci=None, **params):
        P = _roh_params(**params)
        chrom, pos = _loci if _loci is not None else _roh_loci(v.m, chromosome, position)  # (_loci: what _roh_loci returned)
        self.ctx, self.n, self.m = v.ctx, v.n, v.m
        h = C.c_void_p()
        check(lib.tpg_roh_detect(v.ctx.h, v.h, _ptr(chrom), _ptr(pos), C.byref(P), C.byref(h)))
        self.h = h
        self.count = int(lib.tpg_roh_count(h))

    def fetch(self) -> dict:
        c = self.count
        out = dict(indiv=np.zeros(c, dtype=np.int32), first=np.zeros(c, dtype=np.int64), last=np.zeros(c, dtype=np.int64),
                   n_opp=np.zeros(c, dtype=np.int32), n_miss=np.zeros(c, dtype=np.int32))
        check(lib.tpg_roh_fetch(self.ctx.h, self.h, _ptr(out["indiv"]), _ptr(out["first"]), _ptr(out["last"]), _ptr(out["n_opp"]),
                                _ptr(out["n_miss"])))
        return out

    def indiv_summary(self):
        n_runs, total = np.zeros(self.n, dtype=np.int64), np.zeros(self.n, dtype=np.int64)
        check(lib.tpg_roh_indiv_summary(self.ctx.h, self.h, _ptr(n_runs), _ptr(total)))
        return n_runs, total

    def locus_counts(self) -> np.ndarray:
        counts = np.zeros(self.m, dtype=np.int32)
        check(lib.tpg_roh_locus_counts(self.ctx.h, self.h, _ptr(counts)))
        return counts

    def free(self):
        if self.h:
            lib.tpg_roh_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def windows_indiv_roh(X: FBM, ind_row=None, ind_col=None, chromosome=None, position=None, window_size=15, threshold=0.05,
                      min_snp=3, heterozygosity=False, max_opp_window=1, max_miss_window=1, max_gap=10**6, min_length_bps=1000,
                      min_density=1 / 1000, max_opp_run=None, max_miss_run=None, ids=None, groups=None,
                      return_report: bool = False):
    """R/windows_indiv_roh.R:65-150 (around detectRUNS::slidingRuns; the definition is include/tpg.h "Runs of homozygosity"):
    the per-individual loop of the reference in one call.  chromosome / position describe the loci of ind_col, in order.
    Returns the reference's seven columns (group, id, chrom, nSNP, from, to, lengthBps) as a dict of arrays, one entry per
    run, ordered by (individual, first locus), and first_locus / last_locus (0-based positions in ind_col), n_opp, n_miss.
    id defaults to the row index (0-based position in ind_row), group to id, as in the reference's ungrouped case.  With
    return_report also {n_runs, sum_length_bps (per individual), locus_counts (individuals with the locus inside a run)}."""
    P = dict(window_size=window_size, threshold=threshold, min_snp=min_snp, heterozygosity=heterozygosity,
             max_opp_window=max_opp_window, max_miss_window=max_miss_window, max_gap=max_gap, min_length_bps=min_length_bps,
             min_density=min_density, max_opp_run=max_opp_run, max_miss_run=max_miss_run)
    _roh_params(**P)  # (refuses a bad window before anything is packed)
    if position is None:
        raise ValueError("runs of homozygosity need the positions of the loci")
    m = X.ncol if ind_col is None else len(ind_col)
    loci = _roh_loci(m, chromosome, position)
    v = View(X, ind_row, ind_col)
    r = Roh(v, chromosome, position, _loci=loci, **P)
    runs = r.fetch()
    ids = np.arange(v.n) if ids is None else np.asarray(ids)
    groups = ids if groups is None else np.asarray(groups)
    if len(ids) != v.n or len(groups) != v.n:
        raise ValueError("ids / groups must have one entry per individual of ind_row")
    pos = np.asarray(position, dtype=np.int64)
    chrom = np.zeros(v.m, dtype=np.int64) if chromosome is None else np.asarray(chromosome)
    i, a, b = runs["indiv"], runs["first"], runs["last"]
    out = {"group": groups[i], "id": ids[i], "chrom": chrom[a], "nSNP": (b - a + 1).astype(np.int64), "from": pos[a],
           "to": pos[b], "lengthBps": pos[b] - pos[a], "first_locus": a, "last_locus": b, "n_opp": runs["n_opp"],
           "n_miss": runs["n_miss"]}
    if return_report:
        n_runs, total = r.indiv_summary()
        return out, {"n_runs": n_runs, "sum_length_bps": total, "locus_counts": r.locus_counts()}
    return out


# ---------------------------------------------------------------------------
# IBD segments (include/tpg.h "IBD segments")

# loci per chunk of the scan (results do not depend on it; the seam tests do)
IBD_CHUNK_LOCI = int(lib.tpg_ibd_chunk_loci()) if hasattr(lib, "tpg_ibd_chunk_loci") else 0


def ibd_genome_length(chromosome, position, max_gap: int = 10**6) -> int:
    """tpg_ibd_genome_length: the sum over the break-free regions of pos[last] - pos[first], what a pair that shares everything
    adds up to (host only)"""
    chrom, pos = _roh_loci(len(np.asarray(position)), chromosome, position)
    out = C.c_int64()
    check(lib.tpg_ibd_genome_length(_ptr(chrom), _ptr(pos), len(pos), int(max_gap), C.byref(out)))
    return int(out.value)


def ibd_segments(X_or_view, chromosome, position, kind: int = 1, min_snp: int = 200, min_length: int = 0, max_gap: int = 10**6,
                 bridge_min_snp: int = 50, max_err: int = -1, summary: bool = True, ind_row=None, ind_col=None, cap: Optional[int] = None) -> dict:
    """tpg_ibd_segments: where the pairs of individuals share DNA (include/tpg.h "IBD segments"; the output of `king --ibdseg` /
    IBIS on unphased genotypes).  kind 1: at least one haplotype shared (no opposite homozygotes), kind 2: both (equal
    genotypes).  X_or_view: a View, or an FBM with ind_row / ind_col (1-based; ind_row is the hook for a subset of individuals).
    chromosome / position describe the loci of the view, in order; position in any ordered integer unit.  The defaults are
    this project's own: segments of at least 200 typed loci, single bad loci bridged between stretches of at least 50, any
    number of them (max_err < 0: no limit).
    cap: the segments the first call has room for.  The library walks the panel to count and again to write; a call whose arrays
    are too short has counted for nothing and is repeated with room for all, which costs one more counting walk.  The default,
    one segment per pair up to 2^24, is no bound but is rarely passed (the arrays are untouched memory until written); a caller
    who knows better passes its own.
    -> {ind_a, ind_b, first, last (0-based), length (pos[last] - pos[first]), n_typed, n_err}, ordered by (ind_a, ind_b, first);
    with summary also n_seg and sum_length, (n, n), symmetric."""
    if position is None:
        raise ValueError("IBD segments need the positions of the loci")
    v = X_or_view if isinstance(X_or_view, View) else View(X_or_view, ind_row, ind_col)
    chrom, pos = _roh_loci(v.m, chromosome, position)
    n = v.n
    n_seg = np.zeros((n, n), dtype=np.int32) if summary else None
    total = np.zeros((n, n), dtype=np.int64) if summary else None
    cap = max(4096, min(n * (n - 1) // 2, 1 << 24)) if cap is None else int(cap)
    if cap < 0:
        raise ValueError("cap below 0")
    count = C.c_int64()
    while True:
        seg = dict(ind_a=np.empty(cap, dtype=np.int32), ind_b=np.empty(cap, dtype=np.int32), first=np.empty(cap, dtype=np.int64),
                   last=np.empty(cap, dtype=np.int64), n_typed=np.empty(cap, dtype=np.int32), n_err=np.empty(cap, dtype=np.int32))
        check(lib.tpg_ibd_segments(v.ctx.h, v.h, _ptr(chrom), _ptr(pos), int(kind), int(min_snp), int(min_length), int(max_gap),
                                   int(bridge_min_snp), int(max_err), cap, *(_ptr(seg[k]) if cap else None for k in
                                   ("ind_a", "ind_b", "first", "last", "n_typed", "n_err")), C.byref(count), _ptr(n_seg), _ptr(total)))
        if count.value <= cap:
            break
        cap = int(count.value)  # the arrays were too short and are untouched: once more with room for all
    c = int(count.value)
    out = {k: a[:c].copy() for k, a in seg.items()}  # (the arrays of cap entries go back)
    out["length"] = pos[out["last"]] - pos[out["first"]]
    if summary:
        out["n_seg"], out["sum_length"] = n_seg, total
    return out


def pairwise_ibd(X, chromosome, position, ind_row=None, ind_col=None, **params) -> dict:
    """IBD sharing of every pair from both kinds of segment (ibd_segments takes **params).  With L1 and L2 the per-pair sums of
    the kind-1 and kind-2 segment lengths and Lg the genome length: ibd1_prop = (L1 - L2) / Lg and ibd2_prop = L2 / Lg (IBD2
    lies inside IBD1), kin = (L1 + L2) / (4 Lg) -- a kinship estimate that uses no allele frequency and goes into
    filter_high_relatedness as it is.  -> {ibd1_prop, ibd2_prop, kin (n, n), genome_length, segments1, segments2}"""
    if "kind" in params or "summary" in params:
        raise ValueError("pairwise_ibd runs both kinds with the summary: kind / summary are not its parameters")
    if position is None:
        raise ValueError("IBD segments need the positions of the loci")
    Lg = ibd_genome_length(chromosome, position, params.get("max_gap", 10**6))  # (host only: before anything is packed or walked)
    if Lg <= 0:
        raise ValueError("the loci span no length: every break-free region holds one position")
    v = X if isinstance(X, View) else View(X, ind_row, ind_col)
    s1 = ibd_segments(v, chromosome, position, kind=1, summary=True, **params)
    s2 = ibd_segments(v, chromosome, position, kind=2, summary=True, **params)
    L1, L2 = s1.pop("sum_length").astype(np.float64), s2.pop("sum_length").astype(np.float64)
    return {"ibd1_prop": (L1 - L2) / Lg, "ibd2_prop": L2 / Lg, "kin": (L1 + L2) / (4.0 * Lg), "genome_length": Lg,
            "segments1": s1, "segments2": s2}


def gt_impute_simple(X: FBM, method: str = "mode", seed: int = 0) -> FBM:
    """R/gt_impute_simple.R:54-93: the missing genotypes of X are filled in place (FBM.impute_simple) and X then reads
    through CODE_IMPUTE_PRED, as the reference leaves the gen_tibble's FBM; the report is left in `X.impute_report`.
    An error where the reference stops: "object x is already imputed" (a store byte above 3), and a .bed-form store,
    which cannot hold an imputed byte (impute a View of it)."""
    X.impute_report = X.impute_simple(method, seed)
    X.code256 = CODE_IMPUTE_PRED.copy()
    return X


# ---------------------------------------------------------------------------
# LD-kNN imputation (include/tpg.h "LD-kNN imputation")

KNN_PROFILES_GLOBAL, KNN_SMALL_CHUNKS = 1, 2  # TPG_KNN_*: the tests' ways into the other paths; no result changes


def _knn_report(rep, extra) -> dict:
    return {"imputed": int(rep.imputed), "loci_all_missing": int(rep.loci_all_missing), "entries_left": int(extra[0]),
            "loci_without_neighbours": int(extra[1])}


def ld_top_neighbours(v: View, hi, l: int = 10, min_r2: float = 0.0, _flags: int = 0):
    """tpg_ld_top_neighbours on a view without missing genotypes (a locus typed nowhere is allowed and is nobody's neighbour):
    for every locus the l loci of largest r^2 inside the window hi -> (nbr (m, l) int32, -1 = unused; r2 (m, l) float64)"""
    hi = _ld_hi(v, hi)
    l = int(l)
    nbr = np.full((v.m, max(l, 0)), -1, dtype=np.int32)
    r2 = np.zeros((v.m, max(l, 0)), dtype=np.float64)
    check(lib.tpg_ld_top_neighbours(v.ctx.h, v.h, _ptr(hi), l, float(min_r2), int(_flags), _ptr(nbr), _ptr(r2)))
    return nbr, r2


def view_impute_errors(full: View, train: View, filled: View) -> dict:
    """tpg_view_impute_errors: per locus the entries typed in `full` and missing in `train`, and how many of them `filled` has
    wrong -> {"per_locus": (2, m) int64 [held; wrong], "held", "wrong"}"""
    per = np.zeros((full.m, 2), dtype=np.int64)
    tot = (C.c_int64 * 2)()
    check(lib.tpg_view_impute_errors(full.ctx.h, full.h, train.h, filled.h, _ptr(per), tot))
    return {"per_locus": np.ascontiguousarray(per.T), "held": int(tot[0]), "wrong": int(tot[1])}


def knn_impute_errors(v: View, hi, l: int = 10, k: int = 8, min_r2: float = 0.0, fraction: float = 0.05, seed: int = 0) -> dict:
    """the error estimate of LD-kNN imputation on the raw view v (the counterpart of gt_impute_xgboost's imputed_errors): a share
    `fraction` of the typed genotypes is held out (View.holdout_fraction), the rest imputed with the same hi, l, k and min_r2,
    and the held-out entries compared with their fills on the device -> view_impute_errors' dict, plus "error" = wrong / held"""
    train = v.holdout_fraction(fraction, seed)
    filled = train.impute_knn(hi, l, k, min_r2)
    out = view_impute_errors(v, train, filled)
    out["error"] = out["wrong"] / out["held"] if out["held"] else float("nan")
    train.free()
    filled.free()
    return out


def knn_impute_scratch_bytes(n: int, m: int, width: int, l: int = 10) -> int:
    """tpg_knn_impute_scratch_bytes: the device memory a View.impute_knn call plans beyond the raw view"""
    return int(lib.tpg_knn_impute_scratch_bytes(n, m, width, l))


def gt_impute_knn(X: FBM, l: int = 10, k: int = 8, size=100, chromosome=None, position=None, use_positions: bool = False,
                  min_r2: float = 0.0, append_error: bool = False, error_fraction: float = 0.05, seed: int = 0, _flags: int = 0) -> FBM:
    """LD-kNN imputation of the store X in place (tpg_fbm_impute_knn), where the reference offers gt_impute_xgboost: a missing
    byte 3 becomes 4 + fill and X then reads through CODE_IMPUTE_PRED, like gt_impute_simple.  The window comes from
    ld_window_hi(chromosome, position, size, use_positions): `size` loci either side, or size kb with use_positions.  The
    report is left in `X.impute_report`; with append_error the (2, m) table [held; wrong] of knn_impute_errors, computed on the
    store BEFORE it is filled, in `X.impute_errors`.  An error where gt_impute_simple stops: a store that is already imputed
    (a byte above 3), and a .bed-form store (impute a View of it)."""
    if use_positions and position is None:
        raise ValueError("use_positions = TRUE needs positions; pass use_positions=False to count in loci")
    hi = ld_window_hi(chromosome, position, size, use_positions, m=X.ncol)
    if len(hi) != X.ncol:
        raise ValueError("chromosome / position must describe every locus of the store")
    hi = np.ascontiguousarray(hi, dtype=np.int64)
    rep = _lib.ImputeReport()
    extra = (C.c_int64 * 2)()
    errors = None
    if append_error:
        raw = View(X, code256=None)  # (refuses nothing: an imputed store is refused by the call below, before anything is written)
        errors = knn_impute_errors(raw, hi, l, k, min_r2, error_fraction, seed)
        raw.free()
    check(lib.tpg_fbm_impute_knn(X.ctx.h, X.h, _ptr(hi), int(l), int(k), float(min_r2), int(_flags), C.byref(rep), extra))
    X.impute_report = _knn_report(rep, extra)
    if errors is not None:
        X.impute_errors = errors
    X.code256 = CODE_IMPUTE_PRED.copy()
    return X


PCA_OP_TOL_FLOOR = 1e-8  # TPG_PCA_OP_TOL_FLOOR of include/tpg.h: the tightest tol the operator route takes
PCA_ROUTES = ("gram", "operator", "auto")


def _pca_op_block(v: View, center, scale, X, rows: int, what: str) -> tuple:
    center, scale = _f64(center), _f64(scale)
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    if X.ndim != 2 or X.shape[0] != rows:
        raise ValueError(f"{what} must have {rows} rows, not shape {X.shape}")
    if center.shape != (v.m,) or scale.shape != (v.m,):
        raise ValueError(f"center and scale must have {v.m} entries")
    return center, scale, np.asfortranarray(X)


def pca_zt_prod(v: View, center, scale, Q) -> np.ndarray:
    """tpg_pca_zt_prod: W (m x b) = Z'Q on the int8 matrix cores, Z = (G - 1 center') / scale, Q n x b, 1 <= b <= 64
    (include/tpg.h "PCA by operator products")"""
    center, scale, Q = _pca_op_block(v, center, scale, Q, v.n, "Q")
    b = Q.shape[1]
    W = np.zeros((v.m, max(b, 1)), order="F")
    check(lib.tpg_pca_zt_prod(v.ctx.h, v.h, _ptr(center), _ptr(scale), _ptr(Q), b, _ptr(W)))
    return W


def pca_z_prod(v: View, center, scale, W) -> np.ndarray:
    """tpg_pca_z_prod: Y (n x b) = Z W on the int8 matrix cores, W m x b, 1 <= b <= 64"""
    center, scale, W = _pca_op_block(v, center, scale, W, v.m, "W")
    b = W.shape[1]
    Y = np.zeros((v.n, max(b, 1)), order="F")
    check(lib.tpg_pca_z_prod(v.ctx.h, v.h, _ptr(center), _ptr(scale), _ptr(W), b, _ptr(Y)))
    return Y


def pca_op_scratch_bytes(n: int, m: int, k: int) -> int:
    """tpg_pca_op_scratch_bytes: the device memory gt_pca_randomSVD(route="operator") plans beyond the view (host only)"""
    return int(lib.tpg_pca_op_scratch_bytes(int(n), int(m), int(k)))


def gt_pca_randomSVD(X: FBM, ind_row=None, ind_col=None, k: int = 10, tol: float = 1e-4, total_var: bool = True,
                     code256=CODE_IMPUTE_PRED, impute: Optional[str] = None, impute_seed: int = 0,
                     route: str = "gram") -> dict:
    """R/gt_pca_randomSVD.R:77-135.  The reference reaches the truncated SVD of the scaled matrix through
    bigstatsr::big_randomSVD (RSpectra::svds on the implicit operator), which accepts a singular triplet at the
    relative residual `tol`: |Z Z'u_j - d_j^2 u_j| <= tol * d_1^2.  Two routes to it, the same subspace iteration in both:
      "gram"      (default) the n x n Gram matrix of gt_pca_partialSVD, then the iteration on it: 8 n^2 bytes;
      "operator"  the iteration on Q -> Z (Z'Q) by the int8 operator products (pca_zt_prod, pca_z_prod): memory linear in n
                  and in m (pca_op_scratch_bytes), k <= 52, tol >= PCA_OP_TOL_FLOOR; the dict gains n_apply, the number of
                  operator applications;
      "auto"      the operator route only when the Gram route's memory does not fit in half of the device's free memory --
                  a rule about what can run, not about speed.
    The dict says which one ran: route = "gram" | "operator"."""
    if not (0 < tol < 1):
        raise ValueError("tol must be in (0, 1)")
    if route not in PCA_ROUTES:
        raise ValueError(f"route must be one of {PCA_ROUTES}, not {route!r}")
    v = _pca_view(X, ind_row, ind_col, code256, impute, impute_seed)
    if route == "auto":
        fits = C.c_int()
        check(lib.tpg_pca_gram_route_fits(v.ctx.h, v.n, k, C.byref(fits)))
        route = "gram" if fits.value else "operator"
    d = np.zeros(k)
    u = np.zeros((v.n, k), order="F")
    vl = np.zeros((v.m, k), order="F")
    center, scale = np.zeros(v.m), np.zeros(v.m)
    fro = C.c_double()
    napp = C.c_int()
    if route == "gram":
        check(lib.tpg_pca_random_svd(v.ctx.h, v.h, k, tol, _ptr(d), _ptr(u), _ptr(vl), _ptr(center),
                                     _ptr(scale), C.byref(fro) if total_var else None))
    else:
        check(lib.tpg_pca_random_svd_op(v.ctx.h, v.h, k, tol, _ptr(d), _ptr(u), _ptr(vl), _ptr(center),
                                        _ptr(scale), C.byref(fro) if total_var else None, C.byref(napp)))
    out = dict(d=d, u=u, v=vl, center=center, scale=scale, method="randomSVD", route=route)
    if route == "operator":
        out["n_apply"] = napp.value
    if total_var:
        out["square_frobenius"] = fro.value
    return out


def predict_gt_pca(pca: dict, X: Optional[FBM] = None, ind_row=None, ind_col=None, project_method: str = "none",
                   lsq_pcs=(1, 2), code256=CODE_IMPUTE_PRED):
    """predict.gt_pca (R/predict_gt_pca.R:73-236), numeric part: `pca` = the dict gt_pca_partialSVD returns; ind_col =
    the FBM columns of new_data that match the loci of the PCA, in the PCA's order (the reference derives them by
    matching locus names, :113-127).  X = None -> the scores U D of the data the PCA was built on (:101-106).
      "none"           X V on the imputed code table (bigstatsr::big_prodMat, :141-149; missing values are not allowed)
      "simple"         fbm256_prod_and_rowSumsSq, missing genotypes count as 0 (:157-175)
      "least_squares"  per individual, regress its non-missing scaled genotypes on v[, lsq_pcs] (:187-232); predict_gt_pca_lsq()
                       is the same projection as one device call, with the singular rows reported
      "OADP"           not forwarded from here: predict_gt_pca_oadp() is the projection (the device sweep, then the
                       per-individual transform of include/tpg.h "OADP projection" in one kernel); bigsnpr's OADP_proj is not in
                       the reference checkout, and oadp_inputs() returns the XV and X_norm it takes."""
    if project_method not in ("none", "simple", "OADP", "least_squares"):
        raise ValueError("'arg' should be one of 'none', 'simple', 'OADP', 'least_squares'")
    if X is None:
        return np.asfortranarray(pca["u"] * pca["d"])
    if project_method == "OADP":
        raise NotImplementedError("project_method = 'OADP' is not forwarded from predict_gt_pca: call predict_gt_pca_oadp() (the "
                                  "projection of include/tpg.h \"OADP projection\"; bigsnpr::OADP_proj itself is third-party and "
                                  "not in the reference checkout, oadp_inputs() returns the XV and X_norm it takes)")
    Vl = np.asfortranarray(pca["v"], dtype=float)
    if project_method in ("none", "simple"):
        v = View(X, ind_row, ind_col, code256=code256)
        if project_method == "none" and loci_counts(v)[:, 3].any():
            raise ValueError("You can't have missing values in 'X'.")  # bigstatsr's check on the code table
        XV, _ = _prod_and_rss(v, pca["center"], pca["scale"], Vl)
        return XV
    lsq = _lsq_pcs_index(lsq_pcs, Vl.shape[1])
    L = len(lsq)
    v = View(X, ind_row, ind_col, code256=code256)
    Vs = np.asfortranarray(Vl[:, lsq])
    # right-hand sides crossprod(v_sub, g_scaled): the missing -> 0 product; matrices crossprod(v_sub): masked sums of
    # the pairwise products of the chosen columns of v
    rhs, _ = _prod_and_rss(v, pca["center"], pca["scale"], Vs)
    pairs = [(a, b) for a in range(L) for b in range(a, L)]
    tab = np.asfortranarray(np.stack([Vs[:, a] * Vs[:, b] for a, b in pairs], axis=1))
    masked = np.zeros((v.n, len(pairs)), order="F")
    check(lib.tpg_fbm256_valid_prod(v.ctx.h, v.h, _ptr(tab), len(pairs), _ptr(masked)))
    out = np.zeros((v.n, L), order="F")
    for i in range(v.n):
        A = np.zeros((L, L))
        for (a, b), val in zip(pairs, masked[i]):
            A[a, b] = A[b, a] = val
        out[i] = np.linalg.solve(A, rhs[i])  # solve(crossprod(v_sub), crossprod(v_sub, genotypes_scaled)), :228
    return out


def _lsq_pcs_index(lsq_pcs, K: int):
    """the checks of R/predict_gt_pca.R:189-203 on lsq_pcs (1-based) against a PCA of K components -> 0-based indices"""
    lsq = np.asarray(lsq_pcs)
    if (len(lsq) == 0 or np.any(np.isnan(lsq.astype(float))) or np.any(lsq < 1) or np.any(lsq > K)
            or np.any(lsq != lsq.astype(int))):
        raise ValueError(f"lsq_pcs should be a vector of valid component indices (positive integers between 1 and "
                         f"{K}), e.g., c(1, 2) or c(1, 2, 3)")
    if len(set(lsq.tolist())) != len(lsq):
        raise ValueError("lsq_pcs should not contain duplicate values")
    return lsq.astype(int) - 1


def lsq_normal(v: View, center, scale, V) -> dict:
    """tpg_lsq_normal: the per-individual normal equations of include/tpg.h "least-squares projection" for the view `v`, from
    center, scale (m) and the loading columns V (m x L, L <= 32), in one sweep on the FP64 matrix cores -> {"A": n x L x L
    symmetric, "A_packed": n x L (L + 1) / 2 (pair (a, b), a <= b, a-major), "b": n x L, "n_typed": the typed loci (int64)}"""
    V = np.asfortranarray(V, dtype=float)
    center, scale = _f64(center), _f64(scale)
    if V.ndim != 2 or V.shape[0] != v.m or center.shape != (v.m,) or scale.shape != (v.m,):
        raise _lib.TpgError(1, f"the view has {v.m} loci: V must have {v.m} rows, center and scale {v.m} values")  # TPG_EINVAL
    L = V.shape[1]
    P = L * (L + 1) // 2
    Ap = np.zeros((v.n, P), order="F")
    b = np.zeros((v.n, L), order="F")
    nt = np.zeros(v.n, dtype=np.int64)
    check(lib.tpg_lsq_normal(v.ctx.h, v.h, _ptr(center), _ptr(scale), _ptr(V), L, _ptr(Ap), _ptr(b), _ptr(nt)))
    A = np.zeros((v.n, L, L))
    p = 0
    for a in range(L):
        for c in range(a, L):
            A[:, a, c] = A[:, c, a] = Ap[:, p]
            p += 1
    return {"A": A, "A_packed": Ap, "b": b, "n_typed": nt}


def lsq_solve(A_packed, b, n_typed, return_singular: bool = False, ctx: Optional[Context] = None):
    """tpg_lsq_solve: x_i = A_i^-1 b_i for every row by the packed Cholesky of include/tpg.h "least-squares projection"
    (A_packed n x L (L + 1) / 2, b n x L, n_typed n) -> x (n x L) [, n_singular: the rows the singular rule rejects; they are
    NaN].  A row's bits depend on that row alone."""
    ctx = ctx or default_context()
    Ap = np.asfortranarray(A_packed, dtype=np.float64)
    bb = np.asfortranarray(b, dtype=np.float64)
    nt = np.ascontiguousarray(n_typed, dtype=np.int64)
    if Ap.ndim != 2 or bb.ndim != 2:
        raise _lib.TpgError(1, "A_packed and b must be matrices")  # TPG_EINVAL: the sizes the C ABI cannot see
    n, L = bb.shape
    if Ap.shape != (n, L * (L + 1) // 2) or nt.shape != (n,):
        raise _lib.TpgError(1, f"b is {n} x {L}: A_packed must be {n} x {L * (L + 1) // 2} and n_typed hold {n} values")
    out = np.zeros((n, L), order="F")
    sing = C.c_int64()
    check(lib.tpg_lsq_solve(ctx.h, _ptr(Ap), _ptr(bb), _ptr(nt), n, L, _ptr(out), C.byref(sing)))
    return (out, int(sing.value)) if return_singular else out


def predict_gt_pca_lsq(pca: dict, X: FBM, ind_row=None, ind_col=None, lsq_pcs=(1, 2), code256=CODE_IMPUTE_PRED,
                       return_singular: bool = False, return_n_typed: bool = False):
    """predict(pca, new_data, project_method = "least_squares") (R/predict_gt_pca.R:187-232) as one device call
    (tpg_predict_lsq): the sweep that forms every individual's normal equations over the loci it is typed at, then the batched
    Cholesky solve, with nothing but the scores leaving the device.  Arguments and the checks on lsq_pcs as predict_gt_pca; at
    most 32 components -> the scores (n x len(lsq_pcs)), columns in the order of lsq_pcs (they can go to predict_gt_dapc)
    [, n_singular: rows typed at fewer loci than components or with a rank-deficient system; they are NaN] [, n_typed]"""
    Vl = np.asfortranarray(pca["v"], dtype=float)
    lsq = _lsq_pcs_index(lsq_pcs, Vl.shape[1])
    L = len(lsq)
    v = View(X, ind_row, ind_col, code256=code256)
    Vs = np.asfortranarray(Vl[:, lsq])
    center, scale = _f64(pca["center"]), _f64(pca["scale"])
    if Vl.shape[0] != v.m or center.shape != (v.m,) or scale.shape != (v.m,):
        raise _lib.TpgError(1, f"the view has {v.m} loci: the PCA's v must have {v.m} rows, center and scale {v.m} values")  # TPG_EINVAL
    out = np.zeros((v.n, L), order="F")
    nt = np.zeros(v.n, dtype=np.int64)
    sing = C.c_int64()
    check(lib.tpg_predict_lsq(v.ctx.h, v.h, _ptr(center), _ptr(scale), _ptr(Vs), L, _ptr(out), _ptr(nt), C.byref(sing)))
    res = (out,)
    if return_singular:
        res += (int(sing.value),)
    if return_n_typed:
        res += (nt,)
    return res if len(res) > 1 else out


def pcrelate_scratch_bytes(n: int, m: int, k: int) -> int:
    """tpg_pcrelate_scratch_bytes: the operand scratch a PC-Relate call on n x m holds -- bounded independently of m"""
    return int(lib.tpg_pcrelate_scratch_bytes(int(n), int(m), int(k)))


def pcrelate_block_loci(n: int) -> int:
    """tpg_pcrelate_block_loci: the loci of one operand block for n individuals"""
    return int(lib.tpg_pcrelate_block_loci(int(n)))


def pcrelate_basis(V, n: Optional[int] = None) -> np.ndarray:
    """tpg_pcrelate_basis (host only): the orthonormal basis Q (n x (K + 1)) of span[1, V] of include/tpg.h "PC-Relate", step 0.
    V: n x K scores; K = 0 needs n.  A rank-deficient design and n < K + 2 raise TpgError (TPG_EINVAL)."""
    V = np.zeros((int(n), 0), order="F") if V is None else np.asfortranarray(V, dtype=np.float64)
    if V.ndim != 2 or (n is not None and V.shape[0] != int(n)):
        raise _lib.TpgError(1, "V must be an n x K matrix")  # TPG_EINVAL: the sizes the C ABI cannot see
    nn, K = V.shape
    Q = np.zeros((nn, K + 1), order="F")
    check(lib.tpg_pcrelate_basis(_ptr(V) if K else None, nn, K, _ptr(Q)))
    return Q


def _pcrelate_model(v: View, mean, c, Q):
    mean = _f64(mean)
    c, Q = np.asfortranarray(c, dtype=np.float64), np.asfortranarray(Q, dtype=np.float64)
    if Q.ndim != 2 or c.ndim != 2 or Q.shape[0] != v.n or c.shape != (v.m, Q.shape[1]) or mean.shape != (v.m,):
        raise _lib.TpgError(1, f"the view is {v.n} x {v.m}: Q must be {v.n} x L, c {v.m} x L and mean hold {v.m} values")  # TPG_EINVAL
    return mean, c, Q


def pcrelate_coef(v: View, Q) -> dict:
    """tpg_pcrelate_coef, step 1: the regression of every mean-imputed locus of the view on the basis Q (n x L) ->
    {"mean": m (over the typed genotypes), "c": m x L}"""
    Q = np.asfortranarray(Q, dtype=np.float64)
    if Q.ndim != 2 or Q.shape[0] != v.n:
        raise _lib.TpgError(1, f"the view has {v.n} individuals: Q must have {v.n} rows")  # TPG_EINVAL
    L = Q.shape[1]
    mean, c = np.zeros(v.m), np.zeros((v.m, L), order="F")
    check(lib.tpg_pcrelate_coef(v.ctx.h, v.h, _ptr(Q), L, _ptr(mean), _ptr(c)))
    return {"mean": mean, "c": c}


def pcrelate_isaf(v: View, mean, c, Q, maf_bound: float = 0.01) -> dict:
    """tpg_pcrelate_isaf, step 2 as a dense result (tests and small panels: TpgError above the cell cap) ->
    {"mu": n x m individual-specific allele frequencies, "valid": n x m bool}"""
    mean, c, Q = _pcrelate_model(v, mean, c, Q)
    mu = np.zeros((v.n, v.m), order="F")
    valid = np.zeros((v.n, v.m), dtype=np.uint8, order="F")
    check(lib.tpg_pcrelate_isaf(v.ctx.h, v.h, _ptr(mean), _ptr(c), _ptr(Q), Q.shape[1], float(maf_bound), _ptr(mu), _ptr(valid)))
    return {"mu": mu, "valid": valid.astype(bool)}


def pcrelate_gram(v: View, mean, c, Q, maf_bound: float = 0.01) -> dict:
    """tpg_pcrelate_gram, steps 2 - 3: {"num": R R', "den": S S', "cnt": M M'} (n x n) from the model (mean, c) -- which may
    come from a training subset of the individuals -- and the basis rows Q of the view's individuals"""
    mean, c, Q = _pcrelate_model(v, mean, c, Q)
    num, den, cnt = (np.zeros((v.n, v.n), order="F") for _ in range(3))
    check(lib.tpg_pcrelate_gram(v.ctx.h, v.h, _ptr(mean), _ptr(c), _ptr(Q), Q.shape[1], float(maf_bound), _ptr(num), _ptr(den),
                                _ptr(cnt)))
    return {"num": num, "den": den, "cnt": cnt}


def pcrelate(v: View, V, maf_bound: float = 0.01, return_counts: bool = True) -> dict:
    """tpg_pcrelate: include/tpg.h "PC-Relate" on the view from the scores V (n x K; None: K = 0) in one call, bit for bit the
    staged calls -> {"kin": n x n, "inbreeding": n[, "n_snp": n x n int64]}"""
    V = np.zeros((v.n, 0), order="F") if V is None else np.asfortranarray(V, dtype=np.float64)
    if V.ndim != 2 or V.shape[0] != v.n:
        raise _lib.TpgError(1, f"the view has {v.n} individuals: V must have {v.n} rows")  # TPG_EINVAL
    K = V.shape[1]
    kin, f = np.zeros((v.n, v.n), order="F"), np.zeros(v.n)
    ns = np.zeros((v.n, v.n), dtype=np.int64, order="F") if return_counts else None
    check(lib.tpg_pcrelate(v.ctx.h, v.h, _ptr(V) if K else None, K, float(maf_bound), _ptr(kin), _ptr(f), _ptr(ns)))
    out = {"kin": kin, "inbreeding": f}
    if return_counts:
        out["n_snp"] = ns
    return out


def gt_pcrelate(X: FBM, pca: dict, k: Optional[int] = None, ind_row=None, ind_col=None, maf_bound: float = 0.01,
                return_counts: bool = True) -> dict:
    """PC-Relate kinship and inbreeding (Conomos et al. 2016) of the kept rows / columns of X from the first k components of
    `pca` (a gt_pca_* result of the same individuals; the scores are u * d; k = None: all of them, k = 0: the locus
    frequencies alone), missing genotypes allowed -> {"kin", "inbreeding"[, "n_snp"]}; "kin" goes as it is into
    filter_high_relatedness."""
    u, d = np.asarray(pca["u"], dtype=np.float64), np.asarray(pca["d"], dtype=np.float64)
    if k is None:
        k = u.shape[1]
    if np.ndim(k) != 0 or isinstance(k, (bool, np.bool_)) or int(k) != k or k < 0:
        raise ValueError("'k' should be a single non-negative integer value")
    k = int(k)
    if k > u.shape[1]:
        raise ValueError("K is too large: 'k' should not be larger than the number of components in 'pca'")
    v = _raw_view(X, ind_row, ind_col)
    return pcrelate(v, u[:, :k] * d[:k] if k else None, maf_bound=maf_bound, return_counts=return_counts)


def oadp_inputs(pca: dict, X: FBM, ind_row=None, ind_col=None, code256=CODE_IMPUTE_PRED):
    """(XV, X_norm) that predict(project_method = "OADP") hands to bigsnpr::OADP_proj (R/predict_gt_pca.R:157-181)"""
    v = View(X, ind_row, ind_col, code256=code256)
    return _prod_and_rss(v, pca["center"], pca["scale"], np.asfortranarray(pca["v"], dtype=float))


def oadp_proj(XV, X_norm, d, ctx: Optional[Context] = None, return_degenerate: bool = False):
    """tpg_oadp_proj: the OADP projection of include/tpg.h from the "simple" projection XV (n x K), the squared norms X_norm (n)
    of the new individuals and the K <= 32 singular values d of the PCA -> the projected scores (n x K) [, n_degenerate: the
    rows whose Procrustes rotation is not unique; they are NaN]"""
    ctx = ctx or default_context()
    xv, nrm, sv = _scores(XV), _f64(X_norm), _f64(d)
    n, K = xv.shape
    if nrm.shape != (n,) or sv.shape != (K,):
        raise ValueError(f"XV is {n} x {K}: X_norm must hold {n} values and d {K}")
    out = np.zeros((n, K), order="F")
    deg = C.c_int64()
    check(lib.tpg_oadp_proj(ctx.h, _ptr(xv), _ptr(nrm), n, K, _ptr(sv), _ptr(out), C.byref(deg)))
    return (out, int(deg.value)) if return_degenerate else out


def predict_gt_pca_oadp(pca: dict, X: FBM, ind_row=None, ind_col=None, code256=CODE_IMPUTE_PRED, return_degenerate: bool = False):
    """predict(pca, new_data, project_method = "OADP") (R/predict_gt_pca.R:153-186) with the transform of include/tpg.h "OADP
    projection" in place of bigsnpr::OADP_proj: the sweep of fbm256_prod_and_rowSumsSq over the new individuals, then the
    per-individual projection, without XV or the norms leaving the device (tpg_predict_oadp).  Arguments as predict_gt_pca;
    the PCA may hold at most 32 components -> the projected scores (n x K) [, n_degenerate]"""
    v = View(X, ind_row, ind_col, code256=code256)
    V = np.asfortranarray(pca["v"], dtype=float)
    if V.shape[0] != v.m:
        raise ValueError("Incompatibility between dimensions.")  # bigstatsr myassert_size
    K = V.shape[1]
    center, scale, sv = _f64(pca["center"]), _f64(pca["scale"]), _f64(pca["d"])
    if sv.shape != (K,):
        raise ValueError(f"pca['d'] must hold {K} singular values")
    out = np.zeros((v.n, K), order="F")
    deg = C.c_int64()
    check(lib.tpg_predict_oadp(v.ctx.h, v.h, _ptr(center), _ptr(scale), _ptr(V), K, _ptr(sv), _ptr(out), None, C.byref(deg)))
    return (out, int(deg.value)) if return_degenerate else out


def _prod_and_rss(v: View, center, scale, V):
    if V.shape[0] != v.m:
        raise ValueError("Incompatibility between dimensions.")  # bigstatsr myassert_size
    XV = np.zeros((v.n, V.shape[1]), order="F")
    rss = np.zeros(v.n)
    center, scale = _f64(center), _f64(scale)
    check(lib.tpg_fbm256_prod_and_rowSumsSq(v.ctx.h, v.h, _ptr(center), _ptr(scale), _ptr(V), V.shape[1],
                                            _ptr(XV), _ptr(rss)))
    return XV, rss


def fbm256_prod_and_rowSumsSq(X: FBM, ind_row, ind_col, center, scale, V, code256="fbm"):
    """src/fbm_prod_and_rowSumSq.cpp:10-47 -> (XV (n, K), rowSumsSq (n,))"""
    v = View(X, ind_row, ind_col, code256=code256)
    V = np.asfortranarray(V, dtype=float)
    if V.shape[0] != v.m:
        raise ValueError("Incompatibility between dimensions.")  # bigstatsr myassert_size
    XV = np.zeros((v.n, V.shape[1]), order="F")
    rss = np.zeros(v.n)
    center, scale = _f64(center), _f64(scale)
    check(lib.tpg_fbm256_prod_and_rowSumsSq(v.ctx.h, v.h, _ptr(center), _ptr(scale), _ptr(V),
                                            V.shape[1], _ptr(XV), _ptr(rss)))
    return XV, rss


def square_frobenius(X: FBM, ind_row, ind_col, center, scale, code256=CODE_IMPUTE_PRED) -> float:
    """R/square_frobenius.R:19-35"""
    v = View(X, ind_row, ind_col, code256=code256)
    center, scale = _f64(center), _f64(scale)
    if len(center) != v.m or len(scale) != v.m:
        raise ValueError("center and scale must be the same length as the number of columns in the matrix")
    out = C.c_double()
    check(lib.tpg_square_frobenius(v.ctx.h, v.h, _ptr(center), _ptr(scale), C.byref(out)))
    return out.value


def block_size(n: int, ncores: int = 1) -> int:
    """bigstatsr::block_size (recalled)"""
    return max(1, int(math.floor(1024.0 ** 3 / (8.0 * n * ncores))))


block_size_default = block_size


def cut_by_size(m: int, block_size: int):
    """CutBySize (R/local_reimplementations.R:13-15) = bigparallelr::split_len(m, nb = ceiling(m / block.size)) (third
    party, recalled: upper_b = round(b m / nb) with R's round-half-even): (lower, upper), 1-based inclusive -- the blocks the
    R drivers loop over (R/snp_ibs.R:59-82)"""
    nb = int(math.ceil(m / block_size))
    up = np.rint(np.arange(1, nb + 1, dtype=np.float64) * (m / nb)).astype(np.int64)
    lo = np.concatenate([[1], up[:-1] + 1])
    return lo.astype(np.int32), up.astype(np.int32)
