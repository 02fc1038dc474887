#!/usr/bin/env python3
"""bench.py -- throughput of the tidypopgen genotype-matrix hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--scaling strong|weak] [--full] [--dump-outputs DIR]

One "step" = one pass of the whole hot path over one synthetic SNP panel that is already resident in HBM as FBM
bytes (5 000 individuals x 1 000 000 SNPs, 51 populations, 2 % missing kept as imputed bytes -- BASELINE.json
configs[2..4]):

    pack (raw view)  -> loci_alt_freq / missingness counts -> grouped_alt_freq (51 pops)
    -> pairwise_pop_fst Hudson + WC84 -> IBS + KING + allele-sharing/GRM cross-products (FP4 MFMA, exact)
    -> [N > 1: reduce-scatter of the integer N x N partials, all-reduce of the Fst numerator/denominator sums]
    -> IBS / KING / GRM epilogues (every rank its band of the tiles)
    -> pack (imputed view) -> gt_pca_partialSVD (k = 20): center/scale, Gram [N > 1: all-reduce], eigen, loadings

Multi-GPU: SNP blocks shard across ranks, one process per GPU.  The collectives belong to the library (RCCL over
xGMI, csrc/comm.hip); torch.distributed (gloo) is only the control plane that carries the RCCL id and the timing.
  --scaling strong (default): the panel is FIXED (5 000 x 1 000 000, what BASELINE configs 3-5 say) and cut N ways;
  --scaling weak:             every rank owns --snps loci of a panel N times longer.
Rank 0 prints ONE JSON line.  `value` = N_indiv * M_total genotypes / wall second of the whole step.
A plain run sets up, warms up, times the K steps (HIP events only around the MFMA kernels `roofline` prices) and prints the
line.  --full adds what takes runs of its own: the per-kernel table pass, `standalone`, `end_to_end` with `dropin`, and
`cpu_baseline` with its `parity` against the oracle.  --dump-outputs DIR writes what the last timed step computed
(dump_outputs) so that two builds can be compared output for output on the same seeded panel.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scaling", choices=("strong", "weak"), default="strong")
    ap.add_argument("--indiv", "--n", dest="n", type=int, default=5000, help="individuals")
    ap.add_argument("--snps", "--m", dest="m", type=int, default=1000000,
                    help="SNPs of the whole panel (strong scaling) or per GPU (weak scaling)")
    ap.add_argument("--pops", type=int, default=51)
    ap.add_argument("--k", type=int, default=20, help="principal components")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample-loci", type=int, default=0, help="loci of the CPU baseline sample (default M / 20)")
    ap.add_argument("--no-end-to-end", action="store_true", help="skip the host file -> HBM -> host results measurement")
    ap.add_argument("--no-numa-bind", action="store_true", help="do not bind the rank to the host NUMA node of its GPU")
    ap.add_argument("--no-dropin", action="store_true", help="skip the R-shim block-loop measurement (part of end_to_end)")
    ap.add_argument("--no-standalone", action="store_true", help="skip the stand-alone pairwise_grm / snp_king / snp_ibs timings")
    ap.add_argument("--digest", default=None, help="rank 0 writes a small JSON digest of the results (tests)")
    ap.add_argument("--full", action="store_true",
                    help="also the secondary legs (per-kernel table pass, standalone, end_to_end + dropin, cpu_baseline with "
                         "parity); without it the run times the steps and prints the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step computed to DIR/<name>.npy (float64, a fixed sample of the large outputs)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


class Step:
    """Holds the resident panel (this rank's loci) and runs one pass of the hot path through the C ABI."""

    def __init__(self, args, rank, world, local_rank):
        import tidypopgen_amd as tpg
        from tidypopgen_amd import api

        self.tpg, self.api, self.lib = tpg, api, tpg._lib.lib
        self.args, self.rank, self.world = args, rank, world
        # rehearsals on one GPU: "1" = the ranks share device 0 and exchange through the host transport over gloo; "rccl" = they
        # share device 0 and call the nccl* entry points of the library TPG_RCCL_LIBRARY names (tests/host/mock_rccl.cpp --
        # RCCL itself refuses two ranks on one device)
        share = os.environ.get("TPG_BENCH_SHARE_GPU", "")
        share_gpu = share == "1"
        # a launcher may hand every rank ONE visible device (HIP_VISIBLE_DEVICES narrowed per rank) or all of them
        ndev = tpg.device_count()
        if share_gpu or share == "rccl" or (ndev == 1 and world > 1):
            device = 0
        elif local_rank < ndev:
            device = local_rank
        else:
            raise RuntimeError(f"rank {rank}: local rank {local_rank} but only {ndev} HIP device(s) visible")
        self.ctx = tpg.Context(device)
        if share_gpu:
            from tidypopgen_amd import sharding

            self.comm = api.Comm.host(self.ctx, world, rank, sharding.all_reduce_numpy)
        else:
            # RCCL; a single rank exchanges nothing.  If the communicator cannot be made on some rank (no librccl.so, a
            # refused peer mapping ...) every rank falls back to the host transport over gloo together -- correct, and
            # slow: the line says which transport ran (config.collectives)
            self.transport = "rccl"
            comm, err = None, ""
            try:
                comm = api.Comm.from_torch_distributed(self.ctx)
            except Exception as e:  # noqa: BLE001
                err = f"{type(e).__name__}: {e}"
            if world > 1:
                from tidypopgen_amd import sharding

                bad = float(sharding.all_reduce_numpy(np.array([0.0 if comm is not None else 1.0]))[0])
                if bad > 0:
                    if comm is not None:
                        comm.close()
                    if rank == 0:
                        print(f"[bench] RCCL communicator failed on {int(bad)} rank(s) ({err}); host transport over gloo",
                              file=sys.stderr)
                    comm = api.Comm.host(self.ctx, world, rank, sharding.all_reduce_numpy)
                    self.transport = "host (gloo) fallback"
            elif comm is None:
                raise RuntimeError(err)
            self.comm = comm
            if self.transport == "rccl" and world > 1:
                self.transport = comm.transport().replace("rccl: ", "rccl (") + ")"  # names the library that was loaded
                if share == "rccl":
                    self.transport += ", all ranks on ONE GPU (rehearsal of the nccl call sites)"
        # TPG_OVERLAP_REDUCE=1 (opt-in, several ranks over RCCL): the reduce-scatter of the pair counts goes to a SECOND
        # communicator on a second context / stream (tpg_pairwise_reduce_begin / _end) and runs beside the PCA instead of in
        # front of it; the epilogues then follow the PCA.  Rehearsed over the stream-ordered mock RCCL, never on two GPUs.
        self.side_ctx = self.side_comm = None
        if os.environ.get("TPG_OVERLAP_REDUCE") == "1" and world > 1 and not share_gpu and self.transport.startswith("rccl"):
            self.side_ctx = tpg.Context(device)
            self.side_comm = api.Comm.from_torch_distributed(self.side_ctx)
            self.transport += "; pair-count reduce-scatter on a second communicator beside the PCA"
        n, G = args.n, args.pops
        if args.scaling == "strong":
            self.m_total = args.m
            self.j0, j1 = self.comm.shard_loci(args.m)
        else:
            self.m_total = args.m * world
            self.j0, j1 = rank * args.m, (rank + 1) * args.m
        self.m = m = j1 - self.j0
        # FBM bytes resident in HBM before the timed region (the "input"); imputed bytes 4..6 where missing
        self.X = tpg.FBM.synth(3, n, m, j0=self.j0, npop=G, miss=0.02, imputed_bytes=True, ctx=self.ctx,
                               code256=tpg.CODE_012)
        self.gid = (np.arange(n) % G).astype(np.int32)
        self.ploidy = np.full(n, 2.0)
        self.pairs = np.ascontiguousarray(api.combn2(G).T)
        self.P = self.pairs.shape[0]
        self.code_imp = np.ascontiguousarray(tpg.CODE_IMPUTE_PRED)
        self.code_012 = np.ascontiguousarray(tpg.CODE_012)
        # device-resident outputs (PCIe excluded from `value`; `end_to_end` in the JSON line has the inclusive figure)
        self.d_freq = self._dalloc(8 * 2 * m)
        self.d_gfreq = self._dalloc(8 * 2 * G * m)
        self.d_nn = [self._dalloc(8 * n * n) for _ in range(3)]  # IBS, KING, GRM (this rank's band of each)
        self.pw = api.ShardedPairwise(self.comm, n)
        self.fst = {}
        self.has_pca = True
        # PCA setup (untimed): big_SVD stops on a zero scale, so monomorphic loci are dropped beforehand,
        # as a MAF filter does in the reference workflow (vignettes/articles/benchmark_hgdp.Rmd)
        vi = api.View(self.X, None, None, code256=self.code_imp)
        cnt = api.loci_counts(vi)
        vi.free()
        alt = cnt[:, 1] + 2 * cnt[:, 2]
        poly = (alt > 0) & (alt < 2 * n)
        self.pca_cols = None if poly.all() else (np.where(poly)[0] + 1).astype(np.int32)
        self.m_pca = int(poly.sum())
        k = args.k
        self.d_pca = {"u": self._dalloc(8 * n * k), "v": self._dalloc(8 * self.m_pca * k),
                      "center": self._dalloc(8 * self.m_pca), "scale": self._dalloc(8 * self.m_pca)}
        self.pca_d = np.zeros(k)
        self.pca_fro = C.c_double()
        self.fst_sums = np.zeros((4, self.P))  # Hudson num, den; WC84 num, den: read back only by fst_results()
        self.d_fst = self._dalloc(8 * 4 * self.P)  # the same, resident: the step leaves them in HBM like every other output

    def _dalloc(self, nbytes):
        return self.ctx.dev_alloc(max(int(nbytes), 16))

    def barrier_sync(self):
        self.ctx.sync()
        if self.world > 1:
            import torch.distributed as dist

            dist.barrier()

    def run(self, after_per_locus=None, after_nn=None):
        """one pass of the hot path; the two optional callbacks are called when the per-locus results (alt_freq, grouped_alt_freq)
        and the N x N results (IBS, KING, GRM) have been ENQUEUED -- the end-to-end routes synchronise there and start taking
        them down to the host beside the rest of the step"""
        tpg, api, lib, ctx, a = self.tpg, self.api, self.lib, self.ctx, self.args
        chk = tpg._lib.check
        n, G, P = a.n, a.pops, self.P
        # ---- raw view (bytes 0/1/2 valid, the rest missing); when the PCA takes the same loci, its imputed view is
        # packed from the same read of the FBM bytes (tpg_view_create_pair) ----
        v_pca = None
        if self.has_pca and self.pca_cols is None:
            v, v_pca = api.View.pair(self.X, None, None, self.code_012, self.code_imp)
        else:
            v = api.View(self.X, None, None, code256=self.code_012)
        chk(lib.tpg_alt_freq_dip_pseudo(ctx.h, v.h, api._ptr(self.ploidy), C.c_int(0), self.d_freq))
        chk(lib.tpg_grouped_alt_freq_dip_pseudo(ctx.h, v.h, api._ptr(self.gid), C.c_int(G), api._ptr(self.ploidy),
                                                C.c_int(0), self.d_gfreq))
        for row, code in ((0, 0), (2, 2)):  # Hudson, WC84: sums over this rank's loci, left in HBM (no host round trip)
            chk(lib.tpg_pairwise_pop_fst_sums(ctx.h, v.h, api._ptr(self.gid), C.c_int(G), api._ptr(self.ploidy),
                                              C.c_int(code), api._ptr(self.pairs), C.c_int(P),
                                              C.c_void_p(self.d_fst.value + 8 * P * row),
                                              C.c_void_p(self.d_fst.value + 8 * P * (row + 1))))
        if after_per_locus:
            after_per_locus()
        self.pw.zero()
        self.pw.accumulate(v)
        # data-path exchanges (identities on one rank): integer N x N partials, one reduce-scatter; 4 P doubles
        overlap = self.side_comm is not None

        def epilogues():
            chk(lib.tpg_pairwise_epilogues_sharded(ctx.h, self.comm.h, self.pw.h, C.c_int(0), C.c_int64(self.m_total),
                                                   self.d_nn[0], self.d_nn[1], C.c_void_p(None), self.d_nn[2]))
            if after_nn:
                after_nn()

        if overlap:
            self.pw.reduce_begin(self.side_comm)  # enqueued on the side stream behind the pairwise kernel; returns at once
        else:
            self.pw.reduce()
        self.comm.allreduce_f64(self.d_fst.value, 4 * P)
        if not overlap:
            epilogues()
        v.free()
        # ---- imputed view + PCA ----
        if self.has_pca:
            try:
                v = v_pca if v_pca is not None else api.View(self.X, None, self.pca_cols, code256=self.code_imp)
                chk(lib.tpg_pca_partial_svd_sharded(ctx.h, self.comm.h, v.h, C.c_int(a.k), api._ptr(self.pca_d),
                                                    self.d_pca["u"], self.d_pca["v"], self.d_pca["center"],
                                                    self.d_pca["scale"], C.byref(self.pca_fro)))
                v.free()
            except tpg._lib.TpgError as e:
                if e.code != 3:
                    raise
                self.has_pca = False
        elif v_pca is not None:
            v_pca.free()
        if overlap:
            self.pw.reduce_end(self.side_comm)
            epilogues()
        ctx.sync()


def fst_results(st):
    """the Fst ratios from the numerator / denominator sums the step left in HBM"""
    st.tpg._lib.check(st.lib.tpg_dev_to_host(st.ctx.h, st.api._ptr(st.fst_sums), st.d_fst, C.c_size_t(st.fst_sums.nbytes)))
    with np.errstate(invalid="ignore", divide="ignore"):
        st.fst["Hudson"] = st.fst_sums[0] / st.fst_sums[1]
        st.fst["WC84"] = st.fst_sums[2] / st.fst_sums[3]


def digest(st):
    """A few numbers that pin every output of the step (used to compare sharded and unsharded runs).  The N x N
    outputs are sharded by bands: every rank contributes the elements it wrote, summed over the ranks."""
    from tidypopgen_amd import sharding

    n, k = st.args.n, st.args.k
    chk = st.tpg._lib.check
    fst_results(st)
    out = {"fst_hudson": st.fst["Hudson"].tolist(), "fst_wc84": st.fst["WC84"].tolist(),
           "pca_d": st.pca_d.tolist(), "pca_fro": st.pca_fro.value}
    mask = sharding.band_mask(n, st.world, st.rank)
    for name, dptr in zip(("ibs", "king", "grm"), st.d_nn):
        a = np.zeros((n, n), order="F")
        chk(st.lib.tpg_dev_to_host(st.ctx.h, st.api._ptr(a), dptr, C.c_size_t(8 * n * n)))
        a = np.where(mask, a, 0.0)
        nan = np.isnan(a)
        full = sharding.all_reduce_numpy(np.ascontiguousarray(np.where(nan, 0.0, a)))
        nans = sharding.all_reduce_numpy(np.ascontiguousarray(nan.astype(np.float64)))
        out[name + "_sum"] = float(full.sum())
        out[name + "_corner"] = np.where(nans[:6, :6] > 0, np.nan, full[:6, :6]).tolist()
        out[name + "_last"] = np.where(nans[-3:, -3:] > 0, np.nan, full[-3:, -3:]).tolist()
        out[name + "_nan"] = int(nans.sum())
    u = np.zeros((n, k), order="F")
    chk(st.lib.tpg_dev_to_host(st.ctx.h, st.api._ptr(u), st.d_pca["u"], C.c_size_t(8 * n * k)))
    out["pca_u_abs_colsum"] = np.abs(u).sum(axis=0).tolist()
    return out


DUMP_INDIV, DUMP_LOCI, DUMP_BYTES = 512, 16384, 64 << 20


def dump_outputs(st, outdir):
    """What the last step computed, as a caller of the path receives it, into outdir/<name>.npy (float64): the Fst ratios
    and the PCA's d, u and square Frobenius norm whole; IBS / KING / GRM on a sample of individuals (rows and columns);
    alt_freq, grouped_alt_freq and the PCA's v, center, scale on a sample of loci (NaN: a locus the PCA dropped).  The
    samples are seeded and so the same for the same arguments (sample_individuals / sample_loci: their 0-based indices);
    23 MB at the bench size, at most DUMP_BYTES.  Every rank takes part (the N x N bands and the loci are spread over the
    ranks, each element is written by exactly one); rank 0 writes the files."""
    from tidypopgen_amd import sharding

    n, k, G = st.args.n, st.args.k, st.args.pops
    chk, api, lib, ctx = st.tpg._lib.check, st.api, st.lib, st.ctx
    rng = np.random.default_rng(20240601)
    ii = np.sort(rng.choice(n, min(n, DUMP_INDIV), replace=False))
    fixed = 8 * (3 * len(ii) ** 2 + n * k + 2 * st.P + k + 1 + len(ii))
    per_locus = 8 * (2 + 2 * G + k + 2 + 1)
    L = int(min(st.m_total, DUMP_LOCI, max(1, (DUMP_BYTES - fixed) // per_locus)))
    gl = np.sort(rng.choice(st.m_total, L, replace=False))

    def down(dptr, shape):
        h = np.empty(shape, order="F")
        chk(lib.tpg_dev_to_host(ctx.h, api._ptr(h), dptr, C.c_size_t(h.nbytes)))
        return h

    def over_ranks(val, own):
        """the entries every rank owns (own) put together; NaN travels as a mask of its own"""
        if st.world == 1:
            return val
        nan = own & np.isnan(val)
        full = sharding.all_reduce_numpy(np.ascontiguousarray(np.where(own & ~nan, val, 0.0)))
        nans = sharding.all_reduce_numpy(np.ascontiguousarray(nan.astype(np.float64)))
        return np.where(nans > 0, np.nan, full)

    fst_results(st)
    out = {"fst_hudson": st.fst["Hudson"], "fst_wc84": st.fst["WC84"],
           "sample_individuals": ii.astype(np.float64), "sample_loci": gl.astype(np.float64)}
    own_nn = sharding.band_mask(n, st.world, st.rank)[np.ix_(ii, ii)]
    for name, dptr in zip(("ibs", "king", "grm"), st.d_nn):
        out[name] = over_ranks(down(dptr, (n, n))[np.ix_(ii, ii)], own_nn)
    # per-locus outputs: this rank holds loci j0 .. j0 + m - 1 of the panel
    mine = (gl >= st.j0) & (gl < st.j0 + st.m)
    li = gl[mine] - st.j0
    for name, dptr, cols in (("alt_freq", st.d_freq, 2), ("grouped_alt_freq", st.d_gfreq, 2 * G)):
        v = np.zeros((L, cols))
        v[mine] = down(dptr, (st.m, cols))[li]
        out[name] = over_ranks(v, np.repeat(mine[:, None], cols, axis=1))
    if st.has_pca:
        out["pca_d"] = st.pca_d.copy()
        out["pca_square_frobenius"] = np.array([st.pca_fro.value])
        out["pca_u"] = down(st.d_pca["u"], (n, k))
        # the PCA's rows are this rank's polymorphic loci (pca_cols, 1-based) or all of them
        if st.pca_cols is None:
            row, hit = li, np.ones(len(li), dtype=bool)
        else:
            cols0 = st.pca_cols.astype(np.int64) - 1
            row = np.minimum(np.searchsorted(cols0, li), max(0, len(cols0) - 1))
            hit = (cols0[row] == li) if len(cols0) else np.zeros(len(li), dtype=bool)
        for name, shape in (("pca_v", (st.m_pca, k)), ("pca_center", (st.m_pca,)), ("pca_scale", (st.m_pca,))):
            h = down(st.d_pca[name[4:]], shape)
            v = np.full((L,) + shape[1:], np.nan)
            sel = np.where(mine)[0][hit]
            v[sel] = h[row[hit]]
            out[name] = over_ranks(v, np.broadcast_to(mine.reshape((L,) + (1,) * (len(shape) - 1)), v.shape))
    if st.rank == 0:
        os.makedirs(outdir, exist_ok=True)
        for name, arr in out.items():
            np.save(os.path.join(outdir, name + ".npy"), np.ascontiguousarray(arr, dtype=np.float64))


def _e2e_file(st):
    """the resident panel written out as a bigstatsr .bk (column-major bytes) in a RAM-backed or temporary directory"""
    n, m = st.args.n, st.m
    need = n * m + (1 << 28)
    # a real file system's page cache first (what a .bk on disk is read from; a hipMemcpy out of a shmem mapping is
    # slower: tools/xfer_probe.hip), /dev/shm only if there is no room
    for cand in (os.environ.get("TMPDIR", "/tmp"), "/dev/shm"):
        try:
            s = os.statvfs(cand)
            if s.f_bavail * s.f_frsize > need:
                path = os.path.join(cand, f"tpg_bench_{os.getpid()}.bk")
                st.X.to_numpy().T.tofile(path)  # column-major n x m bytes == row-major (m, n)
                os.sync()  # the file is "in the page cache, clean": its write-back must not run beside the timed uploads
                return path
        except (OSError, MemoryError):
            pass
    return None


def _e2e_bed_file(st, dirname):
    """the resident panel as a PLINK .bed payload (SNP-major, 2 bits per genotype, 3-byte magic): imputed genotypes where
    the panel has them -- a .bed cannot mark a genotype as imputed, so this is the file the imputed data set would be
    exported as (no missing genotypes; R/gen_tibble_bed.R:101-125 reads such a file into an FBM through bigsnpr)"""
    n, m = st.args.n, st.m
    lut = np.array([3, 2, 0, 1], dtype=np.uint8)  # dosage 0, 1, 2, missing -> .bed code (11, 10, 00, 01)
    path = os.path.join(dirname, f"tpg_bench_{os.getpid()}.bed")
    host = st.X.to_numpy()
    with open(path, "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        pad = (-n) % 4
        for c0 in range(0, m, 65536):
            blk = host[:, c0:c0 + 65536]
            code = lut[np.where(blk > 3, blk - 4, blk)].T  # loci x individuals
            if pad:
                code = np.concatenate([code, np.zeros((code.shape[0], pad), dtype=np.uint8)], axis=1)
            q = code.reshape(code.shape[0], -1, 4)
            f.write((q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8).tobytes())
    return path


def _e2e_bed(st, path):
    """.bed file -> HBM as it is (n m / 4 bytes, 4x fewer than the .bk route) -> the step -> every result in host memory"""
    tpg, api, lib, ctx, a = st.tpg, st.api, st.lib, st.ctx, st.args
    chk = tpg._lib.check
    n, m, k = a.n, st.m, a.k
    resident = st.X
    try:
        t0 = time.perf_counter()
        st.X = tpg.FBM.open_bed(path, n, m, ctx=ctx, code256=tpg.CODE_012)
        ctx.sync()
        t_up = time.perf_counter()
        host = {}
        down = _e2e_run_with_downloads(st, host)
        t1 = time.perf_counter()
        up = os.path.getsize(path)
        return {"value": n * m / (t1 - t0), "seconds": t1 - t0, "upload_s": t_up - t0, "step_and_download_s": t1 - t_up,
                "upload_GBps": up / (t_up - t0) / 1e9, "bytes_up": up, "bytes_down": down,
                "pca_d_max_rel_diff_vs_bk_route": None}
    finally:
        st.X.free()
        st.X = resident


def _e2e_download(st, ctx, d_nn, d_freq_blocks, d_gfreq_blocks, mbs, host):
    """results -> host memory (IBS / KING / GRM, per-locus and grouped frequencies)"""
    api, lib, chk = st.api, st.lib, st.tpg._lib.check
    n, G = st.args.n, st.args.pops
    total = 0
    for name, d in zip(("ibs", "king", "grm"), d_nn):
        host[name] = np.empty((n, n), order="F")
        chk(lib.tpg_dev_to_host(ctx.h, api._ptr(host[name]), d, C.c_size_t(8 * n * n)))
        total += 8 * n * n
    if mbs:  # (a caller that takes the per-locus results down itself keeps its own entries)
        host["freq"], host["gfreq"] = [], []
    for d, mb in zip(d_freq_blocks, mbs):
        a = np.empty((mb, 2), order="F")
        chk(lib.tpg_dev_to_host(ctx.h, api._ptr(a), d, C.c_size_t(a.nbytes)))
        host["freq"].append(a)
        total += a.nbytes
    for d, mb in zip(d_gfreq_blocks, mbs):
        a = np.empty((mb, 2 * G), order="F")
        chk(lib.tpg_dev_to_host(ctx.h, api._ptr(a), d, C.c_size_t(a.nbytes)))
        host["gfreq"].append(a)
        total += a.nbytes
    return total


def _e2e_run_with_downloads(st, host):
    """st.run() with the results going down to the host as soon as they exist: alt_freq / grouped_alt_freq (0.83 GB at 5 000 x
    1 000 000) beside the pairwise pass, IBS / KING / GRM (0.6 GB) beside the PCA, on a second thread with a stream of its own;
    the PCA's u and v after the step.  -> bytes taken down"""
    import queue
    import threading

    tpg, api, lib, ctx, a = st.tpg, st.api, st.lib, st.ctx, st.args
    chk = tpg._lib.check
    n, m, k, G = a.n, st.m, a.k, a.pops
    down_ctx = tpg.Context(ctx.device)
    q = queue.Queue()
    total, errors = [0], []
    trace = os.environ.get("TPG_E2E_TRACE") == "1"
    T0 = time.perf_counter()

    def stamp(what):
        if trace:
            print(f"[e2e] {1e3 * (time.perf_counter() - T0):7.2f} ms  {what}", file=sys.stderr, flush=True)

    def downloader():
        try:
            while True:
                what = q.get()
                stamp(f"downloader got {what}")
                if what is None:
                    return
                if what == "per_locus":
                    for key, dptr, cols in (("freq", st.d_freq, 2), ("gfreq", st.d_gfreq, 2 * G)):
                        arr = np.empty((m, cols), order="F")
                        chk(lib.tpg_dev_to_host(down_ctx.h, api._ptr(arr), dptr, C.c_size_t(arr.nbytes)))
                        host[key] = [arr]
                        total[0] += arr.nbytes
                        stamp(f"{key} down ({arr.nbytes / 1e6:.0f} MB)")
                elif what == "nn":
                    total[0] += _e2e_download(st, down_ctx, st.d_nn, [], [], [], host)
                    stamp("N x N down")
                else:  # the PCA's u and v: from THIS thread too -- a device -> host copy issued by the main thread right after
                    # the large copies of this one stood still for 48 ms (800 KB!), whatever the runtime does there
                    u = np.empty((n, k), order="F")
                    chk(lib.tpg_dev_to_host(down_ctx.h, api._ptr(u), st.d_pca["u"], C.c_size_t(u.nbytes)))
                    vl = np.empty((st.m_pca, k), order="F")
                    chk(lib.tpg_dev_to_host(down_ctx.h, api._ptr(vl), st.d_pca["v"], C.c_size_t(vl.nbytes)))
                    host["u"], host["v"] = u, vl
                    total[0] += u.nbytes + vl.nbytes
                    stamp("u, v down")
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = threading.Thread(target=downloader)
    th.start()

    def hook(what):
        ctx.sync()  # the kernels that write these results have finished: another stream may read them
        stamp(f"hook {what}")
        q.put(what)

    try:
        st.run(after_per_locus=lambda: hook("per_locus"), after_nn=lambda: hook("nn"))  # (ends with a synchronisation)
        q.put("pca")
    finally:
        q.put(None)
    stamp("step done")
    if trace:
        import faulthandler

        faulthandler.dump_traceback_later(0.025, exit=False, file=sys.stderr)  # where is everybody 25 ms from now?
    th.join()
    if trace:
        faulthandler.cancel_dump_traceback_later()
    stamp("downloader joined")
    down_ctx.close()
    if errors:
        raise errors[0]
    return total[0]


def _e2e_serial(st, path):
    """upload everything, then the step with the downloads beside it (_e2e_run_with_downloads)"""
    tpg, api, lib, ctx, a = st.tpg, st.api, st.lib, st.ctx, st.args
    chk = tpg._lib.check
    n, m, k = a.n, st.m, a.k
    resident = st.X
    try:
        t0 = time.perf_counter()
        st.X = tpg.FBM.open_bk(path, n, m, ctx=ctx, code256=tpg.CODE_012)
        ctx.sync()
        t_up = time.perf_counter()
        host = {}
        down = _e2e_run_with_downloads(st, host)
        t1 = time.perf_counter()
        return {"value": n * m / (t1 - t0), "seconds": t1 - t0, "upload_s": t_up - t0, "step_and_download_s": t1 - t_up,
                "upload_GBps": n * m / (t_up - t0) / 1e9, "bytes_up": n * m, "bytes_down": down}
    finally:
        st.X.free()
        st.X = resident


def _e2e_streamed(st, path, source="bk", budget_bytes=0):
    """The reference's own block loop (R/snp_ibs.R:59-82) as the LIBRARY runs it (tpg_stream_run, csrc/stream.hip): the store
    stays on the host; an uploader thread (its own stream) fills one of two block buffers -- blocks of loci of the .bk, or of
    SNPs of the .bed payload -- while the caller's context packs the block before it (raw and imputed view from one read),
    takes its per-locus statistics and Fst sums and adds its pairwise cross-products and its Gram matrix to the running
    totals; a downloader thread (a third stream) writes the per-locus results of every block into the caller's arrays; after
    the last block the N x N results go down beside the eigen step and the loadings.  Until round 5 this pipeline was Python
    in this file (three threads, three contexts, a queue); now the route is one library call.  budget_bytes = 0: no bound on
    the HBM the store's bytes and views may take (a few large blocks, views kept: the fastest route for a panel that fits)."""
    tpg, a = st.tpg, st.args
    n, m, G, k = a.n, st.m, a.pops, a.k
    t0 = time.perf_counter()
    if source == "bed":
        S = tpg.Stream.open_bed(path, n, m, budget_bytes=budget_bytes, ctx=st.ctx)
    else:
        S = tpg.Stream.open_bk(path, n, m, budget_bytes=budget_bytes, ctx=st.ctx)
    try:
        pca_here = st.has_pca and st.pca_cols is None
        r = S.run(pairwise=("ibs", "king", "grm"), code256=st.code_012, ploidy=st.ploidy, groupIds=st.gid, ngroups=G,
                  alt_freq=True, grouped_alt_freq=True, fst=("Hudson", "WC84"), pairwise_combn=st.pairs.T,
                  k=k if pca_here else 0, code256_pca=st.code_imp)
        rep = dict(r["report"])
        if st.has_pca and not pca_here:  # (monomorphic loci were dropped for the PCA: its own selection, its own sweep)
            r2 = S.run(None, st.pca_cols, k=k, code256_pca=st.code_imp)
            r.update({key: r2[key] for key in ("d", "u", "v", "center", "scale", "square_frobenius")})
            for key in ("bytes_up", "bytes_down"):
                rep[key] += r2["report"][key]
        t1 = time.perf_counter()
    finally:
        S.close()
    # the pipeline must give what the resident step gives
    check = {"fst_hudson_max_rel_diff": float(np.nanmax(np.abs(r["fst_tot"]["Hudson"] / st.fst["Hudson"] - 1))),
             "fst_wc84_max_rel_diff": float(np.nanmax(np.abs(r["fst_tot"]["WC84"] / st.fst["WC84"] - 1))),
             "pca_d_max_rel_diff": float(np.max(np.abs(r["d"] / st.pca_d - 1))) if st.has_pca else None,
             "frobenius_rel_diff": abs(r["square_frobenius"] / st.pca_fro.value - 1) if st.has_pca else None}
    return {"value": n * m / (t1 - t0), "seconds": t1 - t0, "last_block_in_HBM_s": rep["seconds_first_sweep"],
            "tail_s": (t1 - t0) - rep["seconds_first_sweep"], "blocks": rep["blocks"], "block_loci": rep["block_loci"],
            "bytes_up": rep["bytes_up"], "bytes_down": rep["bytes_down"], "views_kept": bool(rep["views_kept"]),
            "sweeps": rep["sweeps"], "budget_bytes": budget_bytes, "planned_bytes": rep["planned_bytes"],
            "state_bytes": rep["state_bytes"], "peak_device_bytes_growth": rep["peak_device_bytes"],
            "entry_point": "tpg_stream_run (csrc/stream.hip)", "agreement_with_resident_step": check}


def end_to_end(st):
    """Host backing file -> HBM -> every result of the step back in host memory, on rank 0's panel at N = 1: what an R
    caller holding a bigstatsr .bk file pays, PCIe included (never `value`).  Two ways: serial (upload, step,
    download) and the library's block pipeline (_e2e_streamed = tpg_stream_run)."""
    fst_results(st)  # of the resident step: what the pipelines are compared with
    path = _e2e_file(st)
    if path is None:
        return {"skipped": "no room for the backing file"}
    bed_path = None
    def throttled():
        """(periods this cgroup was throttled in, microseconds it stood still): the GPU boxes give a job 16 cores' worth of CPU
        time per 100 ms, and a route whose thread teams exceed it stands still until the period ends"""
        try:
            kv = dict(line.split() for line in open("/sys/fs/cgroup/cpu.stat"))
            return int(kv.get("nr_throttled", 0)), int(kv.get("throttled_usec", 0))
        except (OSError, ValueError):
            return 0, 0

    def median_of(fn, *a, reps=3):
        """the run with the median time of `reps` (transfers over PCIe from a shared host vary from run to run: on the
        driver's box of round 3 the pipelined route took 0.336 s once where it takes 0.175 s)"""
        th0 = throttled()
        runs = sorted((fn(*a) for _ in range(reps)), key=lambda r: r["seconds"])
        th1 = throttled()
        mid = dict(runs[len(runs) // 2])
        mid["seconds_all_runs"] = [r["seconds"] for r in runs]
        mid["cpu_quota_throttling_over_all_runs"] = {"periods": th1[0] - th0[0], "stood_still_ms": (th1[1] - th0[1]) / 1e3}
        return mid

    try:
        ser = median_of(_e2e_serial, st, path)
        d_bk = st.pca_d.copy()
        ovl = median_of(_e2e_streamed, st, path)
        routes = {"serial": ("bigstatsr .bk (1 byte per genotype, warm page cache) -> HBM in one upload -> the step, its "
                             "results going down to host memory beside it", ser),
                  "overlapped": ("bigstatsr .bk (1 byte per genotype, warm page cache) -> tpg_stream_run: HBM in 8 locus blocks uploaded by "
                                 "the library's uploader thread / stream beside pack + accumulate, per-locus results down block by "
                                 "block on a third -> all results in host memory", ovl)}
        best = min(routes, key=lambda k_: routes[k_][1]["seconds"])
        out = {"value": routes[best][1]["value"], "unit": "SNP-genotypes/s", "seconds": routes[best][1]["seconds"],
               "route": routes[best][0], "best_bk_route": best, "statistic": "median of 3 runs per route; value = the faster .bk route",
               "overlapped": ovl, "serial": ser}
        try:  # the same call when the panel may NOT stay: 1 / 8 of its bytes as the budget (a second sweep for the loadings)
            tight = _e2e_streamed(st, path, budget_bytes=st.args.n * st.m // 8)
            tight["route"] = ("the same .bk through tpg_stream_run with budget_bytes = 1 / 8 of the panel: the store's bytes and views "
                              "never take more HBM than that; the loadings stream the file a second time")
            out["out_of_core"] = tight
        except Exception as e:  # noqa: BLE001
            out["out_of_core"] = {"failed": f"{type(e).__name__}: {e}"}
        if not st.args.no_dropin:
            try:
                out["dropin"] = dropin(st, path)
            except Exception as e:  # noqa: BLE001 -- the leg must not take the bench line down with it
                out["dropin"] = {"failed": f"{type(e).__name__}: {e}"}
        os.remove(path)  # room for the .bed
        try:
            bed_path = _e2e_bed_file(st, os.path.dirname(path))
            bed = median_of(_e2e_bed, st, bed_path)
            # the .bed holds the imputed genotypes, so its PCA is the PCA of the .bk route (the pairwise statistics see
            # no missing genotype there, which is a different input: not compared)
            bed["pca_d_max_rel_diff_vs_bk_route"] = float(np.max(np.abs(st.pca_d / d_bk - 1))) if st.has_pca else None
            bed["route"] = ("PLINK .bed of the imputed panel (2 bits per genotype, warm page cache) -> HBM as it is through pinned "
                            "staging -> pack from the .bed bytes -> the step, its results going down to host memory beside it")
            # the same file through the block pipeline (what the pipeline is compared with: the .bed's own resident step)
            fst_results(st)
            # (blocks: TPG_STREAM_BLOCKS; measured in round 5: 2 blocks 75.5 ms, 3: 80.7, 4: 80.0, 8: 98 -- per-block fixed costs)
            bed_ovl = median_of(lambda st_, p_: _e2e_streamed(st_, p_, source="bed"), st, bed_path)
            bed_ovl["route"] = (f"PLINK .bed of the imputed panel -> tpg_stream_run: HBM in {bed_ovl['blocks']} blocks of SNPs uploaded through "
                                "pinned staging by the library's uploader thread / stream beside pack + accumulate, per-locus results down "
                                "block by block on a third -> all results in host memory")
            out["bed"] = dict(bed_ovl if bed_ovl["seconds"] < bed["seconds"] else bed)
            out["bed"]["serial"], out["bed"]["overlapped"] = bed, bed_ovl
        except (OSError, MemoryError) as e:
            out["bed"] = {"skipped": f"{type(e).__name__}: {e}"}
        return out
    finally:
        for p_ in (path, bed_path):
            try:
                if p_:
                    os.remove(p_)
            except OSError:
                pass


def standalone(st):
    """The three pairwise analyses called ON THEIR OWN on the resident panel -- what `pairwise_grm()`, `snp_king()`,
    `snp_ibs()` cost when a session asks for one of them -- and BASELINE config 2's literal workload (KING + GRM at
    1 000 x 650 000).  Each accumulates only the cross-products it needs (tpg_pairwise_accumulate_products: 2 / 4 / 3 of
    the 5) and `frac` prices the kernel on exactly those (2 / 5 / 6 N^2 M ops for AS / KING / IBS in the
    reference's own algebra; here the kernels' real 2 / 4 / 3 N^2 M, the smaller figures).  `ms` = view pack + kernel +
    epilogue, outputs left in HBM."""
    tpg, api, lib, ctx, a = st.tpg, st.api, st.lib, st.ctx, st.args
    chk = tpg._lib.check
    out = {}

    def one(name, X, n, m, products, ops_per, key, epilogue, note):
        pw = api.Pairwise(ctx, n)
        d = [ctx.dev_alloc(8 * n * n) for _ in range(2)]
        best = None
        for _ in range(3):
            ctx.prof_reset()
            ctx.sync()
            t0 = time.perf_counter()
            v = api.View(X, None, None, code256=None)
            pw.zero()
            pw.accumulate(v, products=products)
            epilogue(pw, d, m)
            v.free()
            ctx.sync()
            ms = (time.perf_counter() - t0) * 1e3
            prof = ctx.prof_dump()
            k_ms = prof.get(key, (0, 0.0))[1]
            if best is None or ms < best[0]:
                best = (ms, k_ms, {k_: round(v_[1], 4) for k_, v_ in sorted(prof.items())})
        for p_ in d:
            ctx.dev_free(p_)
        pw.free()
        ops = ops_per * n * n * m
        out[name] = {"workload": f"{n} x {m}", "ms": best[0], "kernel_ms": best[1], "kernel": key,
                     "products": note, "algorithmic_ops": ops, "achieved_TOPs": ops / (best[1] * 1e-3) / 1e12 if best[1] else None,
                     "peak_TOPs": 10000.0, "frac": ops / (best[1] * 1e-3) / 1e12 / 10000.0 if best[1] else None,
                     "kernel_ms_all": best[2]}

    n, m = a.n, st.m
    ctx.prof_enable(True)
    one("pairwise_grm", st.X, n, m, api.PW_FOR_AS, 2.0, "pairwise_mfma_as",
        lambda pw, d, m_: chk(lib.tpg_pairwise_grm(ctx.h, pw.h, d[0])), "V, D (2 of 5): src/snp_as.cpp:64-65")
    one("snp_king", st.X, n, m, api.PW_FOR_KING, 4.0, "pairwise_mfma_king",
        lambda pw, d, m_: chk(lib.tpg_pairwise_king(ctx.h, pw.h, d[0])), "V, D, A, A' (4 of 5): src/snp_king.cpp:70-72")
    one("snp_ibs", st.X, n, m, api.PW_FOR_IBS_ALONE, 3.0, "pairwise_mfma_ibs1",
        lambda pw, d, m_: chk(lib.tpg_pairwise_ibs(ctx.h, pw.h, C.c_int(0), C.c_int64(m_), d[0])),
        "V and D + H (three of the five rank-1 products, the last two into one sum: TPG_PW_DH): src/snp_ibs.cpp:67-72")
    one("snp_ibs_with_allele_sharing", st.X, n, m, api.PW_FOR_IBS, 3.0, "pairwise_mfma_ibs",
        lambda pw, d, m_: chk(lib.tpg_pairwise_ibs(ctx.h, pw.h, C.c_int(0), C.c_int64(m_), d[0])),
        "V, D, H apart (3 of 5), for callers that want allele sharing / GRM from the same pass")
    # BASELINE config 2, literally: pairwise_king + pairwise_grm of an HGDP-like 1 000 x 650 000 panel on one MI355X
    n2, m2 = 1000, 650000
    X2 = tpg.FBM.synth(2, n2, m2, npop=a.pops, miss=0.02, imputed_bytes=True, ctx=ctx, code256=tpg.CODE_012)
    one("config2_king_plus_grm", X2, n2, m2, api.PW_FOR_KING, 4.0, "pairwise_mfma_king",
        lambda pw, d, m_: chk(lib.tpg_pairwise_epilogues(ctx.h, pw.h, C.c_int(0), C.c_int64(m_), C.c_void_p(None), d[0],
                                                         C.c_void_p(None), d[1])),
        "V, D, A, A' (4 of 5) serve both KING and GRM")
    X2.free()
    ctx.prof_enable(False)
    return out


def dropin(st, path):
    """What an UNMODIFIED tidypopgen session pays for `snp_ibs()` (R/snp_ibs.R:59-95) when its native symbols are this
    library's: the compiled shim (shim/tpg_rshim.c) driven through tests/rmock (a stand-in for R's C API: R is not in the
    image) exactly as the R driver drives it -- blocks of bigstatsr::block_size(n) loci, `_tidypopgen_increment_ibs_counts`
    per block on the genotype .bk and two file-backed N x N double FBMs, default (non-deferred) mode: per block an upload of
    its columns, pack, the {V, D, H} kernel, and K / K2 incremented in the caller's mapping before the call returns.  Beside
    it the opt-in deferred mode (one download at tpg_flush) and the whole-analysis entry point the shim adds
    (`_tidypopgen_tpg_snp_pairwise`: tpg_multi_pairwise on the host mapping, which = ibs)."""
    import shutil
    import tempfile

    from tests import rmock

    api, a = st.api, st.args
    n, m = a.n, st.m
    tmp = tempfile.mkdtemp(prefix="tpg_dropin_", dir=os.path.dirname(path))
    out = {"route": "rmock -> shim/tpg_rshim.c -> libtpg_hip.so; genotype .bk warm in the page cache; R absent from the image"}
    saved = {k_: os.environ.get(k_) for k_ in ("TPG_RSHIM_DEFERRED", "TPG_DEVICES", "TPG_RSHIM_CACHE")}
    try:
        rows = np.arange(1, n + 1, dtype=np.int32)
        cols = np.arange(1, m + 1, dtype=np.int32)
        block = api.block_size(n)
        lo, up = api.cut_by_size(m, block)

        def session(deferred):
            os.environ.pop("TPG_RSHIM_CACHE", None)
            os.environ["TPG_DEVICES"] = "1"
            if deferred:
                os.environ["TPG_RSHIM_DEFERRED"] = "1"
            else:
                os.environ.pop("TPG_RSHIM_DEFERRED", None)
            lib = rmock.build(tmp)
            return lib, rmock.Session(lib)

        def accumulators(r, tag):
            files = []
            for nm in ("k", "k2"):
                f = os.path.join(tmp, f"{tag}_{nm}.bk")
                np.zeros(n * n).tofile(f)  # bigstatsr::FBM(n, n, init = 0)
                files.append(f)
            return files, [r.fbm(f, n, n) for f in files]

        for mode, deferred in (("block_loop_default", False), ("block_loop_deferred", True)):
            lib, r = session(deferred)
            BM = r.fbm(path, n, m, st.code_012)
            files, (K, K2) = accumulators(r, mode)
            t0 = time.perf_counter()
            rmock.driver_loop(r, "ibs", BM, K, K2, rows, cols, lo, up, scratch_width=1)
            if deferred:
                r.call("tpg_flush")
            dt = time.perf_counter() - t0
            k = np.fromfile(files[0], dtype=np.float64, count=2 * n).reshape(2, n)  # first two columns of K
            out[mode] = {"seconds": dt, "blocks": int(len(lo)), "block_loci": int(block), "value": n * m / dt,
                         "K_first_entries": k[0, :3].tolist()}
            lib.R_unload_tpgshim(None)
            lib.rmock_reset()
            for f in files:
                os.remove(f)
        lib, r = session(False)
        BM = r.fbm(path, n, m, st.code_012)
        t0 = time.perf_counter()
        res = r.call("tpg_snp_pairwise", BM, r.int(rows), r.int(cols), r.lib.rmock_lgl(0), r.int([1]))
        dt = time.perf_counter() - t0
        ibs = r.list_elt(res, 0, (n, n))
        out["tpg_snp_pairwise_ibs"] = {"seconds": dt, "value": n * m / dt, "ibs_first_entries": ibs[0, :3].tolist()}
        # the three routes computed the same matrix: proportion = K / K2 (R/snp_ibs.R:88-95) for the first entries
        lib.R_unload_tpgshim(None)
        lib.rmock_reset()
        out["unit"] = "seconds per snp_ibs() of the whole panel; value = SNP-genotypes/s"
    finally:
        for k_, v_ in saved.items():
            if v_ is None:
                os.environ.pop(k_, None)
            else:
                os.environ[k_] = v_
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def cpu_baseline(args, st=None):
    """The oracle's "as the reference does it" path (oracle/oracle.py: dense FP64 one-hot blocks + BLAS
    products for IBS/KING/AS, C loops for the per-locus statistics and Fst, numpy Gram for PCA), timed on
    this host's cores over a bounded sample of the same workload.  With `st` (the resident step's context) the GPU then
    computes the same analyses on the same sample and `parity` reports max |delta| against the oracle's results: the second
    half of BASELINE.json's metric, in the one leg of bench.py that may call the oracle (as the checker, after the timing)."""
    from oracle import oracle as orc

    n, G = args.n, args.pops
    B = args.cpu_sample_loci or max(1024, args.m // 20)  # M / 20, extrapolated linearly in M
    fbm = orc.synth_fbm(3, n, B, npop=G, miss=0.02, imputed_bytes=True)
    r = np.arange(1, n + 1, dtype=np.int32)
    gid = (np.arange(n) % G).astype(np.int32)
    ploidy = np.full(n, 2.0)
    blk = orc.block_size_default(n)  # the reference's own block size, bigstatsr::block_size(n)
    t0 = time.time()
    K = [np.zeros((n, n)) for _ in range(6)]
    for a in range(0, B, blk):
        c = np.arange(a + 1, min(B, a + blk) + 1, dtype=np.int32)
        orc.blas_increment_ibs(K[0], K[1], fbm, r, c)
        orc.blas_increment_king(K[2], K[3], fbm, r, c)
        orc.blas_increment_as(K[4], K[5], fbm, r, c)
    c = np.arange(1, B + 1, dtype=np.int32)
    ref = {"king": orc.king_epilogue(K[2], K[3])}
    ref["grm"] = orc.pairwise_grm(orc.as_epilogue(K[4], K[5]))
    ref["freq"] = orc.alt_freq_dip_pseudo_cpp(fbm, r, c, ploidy)
    ref["gfreq"] = orc.grouped_alt_freq_dip_pseudo_cpp(fbm, r, c, gid, G, ploidy)
    with np.errstate(invalid="ignore", divide="ignore"):
        ref["Hudson"] = orc.pairwise_pop_fst(fbm, r, c, gid, G, method="Hudson")["fst_tot"]
        ref["WC84"] = orc.pairwise_pop_fst(fbm, r, c, gid, G, method="WC84")["fst_tot"]
    # PCA Gram of the sample (K = Z Z' through BLAS), as bigstatsr::big_SVD accumulates it per block
    Kp = np.zeros((n, n))
    for a in range(0, B, blk):
        X = orc.CODE_IMPUTE_PRED[fbm[:, a:a + blk]]
        center = X.mean(axis=0)
        p = center / 2
        scale = np.sqrt(2 * p * (1 - p))
        keep = scale > 0
        Z = (X[:, keep] - center[keep]) / scale[keep]
        Kp += Z @ Z.T
    dt = time.time() - t0
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    try:  # the threads the BLAS products actually ran on (OpenBLAS caps them at its build maximum)
        from threadpoolctl import threadpool_info

        blas = [int(t["num_threads"]) for t in threadpool_info() if t.get("user_api") == "blas"]
        if blas:
            cores = min(cores, max(blas))
    except ImportError:
        pass
    out = {"value": n * B / dt, "unit": "SNP-genotypes/s", "cores": cores, "kind": "port",
           "sample": f"{n} x {B} loci (M / {args.m // B if B else 0}) of the same synthetic panel, extrapolated linearly in M: "
                     f"IBS+KING+AS via numpy/BLAS FP64 one-hot products "
                     f"(reference's 6/4/2 products per block of {blk} loci, multi-threaded), per-locus + Fst (Hudson, WC84) C loops "
                     f"(OpenMP), PCA Gram via BLAS; {dt:.1f} s; eigen step excluded"}
    if st is not None:
        try:
            out["parity"] = _parity_vs_oracle(st, fbm, K, ref, Kp, B)
        except Exception as e:  # noqa: BLE001 -- the check must not take the bench line down with it
            out["parity"] = {"failed": f"{type(e).__name__}: {e}"}
    return out


def _parity_vs_oracle(st, fbm, K, ref, Kp, B):
    """max |delta| of the HIP path against the oracle's results on the cpu_baseline sample (the first B loci of the bench panel:
    the device generator and the oracle's are the same pure function of (seed, individual, locus), checked first)"""
    tpg, api, a = st.tpg, st.api, st.args
    n, G, k = a.n, a.pops, a.k
    ctx = st.ctx
    X = tpg.FBM.synth(3, n, B, npop=G, miss=0.02, imputed_bytes=True, ctx=ctx, code256=tpg.CODE_012)
    out = {"sample": f"{n} x {B}", "same_input_bytes": bool(np.array_equal(X.to_numpy(), fbm))}
    v = api.View(X, None, None, code256=None)
    pw = api.Pairwise(ctx, n)
    pw.accumulate(v)
    cnt = pw.counts()
    out["counts_max_abs"] = float(max(np.abs(cnt[name] - K[i]).max() for i, name in
                                      enumerate(("ibs", "ibs_valid", "king_num", "n_Aa_i", "as_num", "as_den"))))
    ep = pw.epilogues(which=("ibs", "king", "grm"))

    def max_rel(x, y):
        both = np.isfinite(x) & np.isfinite(y)
        if not np.array_equal(np.isfinite(x), np.isfinite(y)):
            return float("inf")
        den = np.maximum(np.abs(y[both]), 1e-300)
        return float((np.abs(x[both] - y[both]) / den).max()) if both.any() else 0.0

    with np.errstate(invalid="ignore", divide="ignore"):
        out["ibs_max_rel"] = max_rel(ep["ibs"], K[0] / K[1])  # R/snp_ibs.R:88-95
    out["king_max_rel"] = max_rel(ep["king"], ref["king"])
    # GRM = 2 (M - mb) / (1 - mb) passes through zero: relative to the largest entry
    out["grm_max_rel_of_max"] = float(np.nanmax(np.abs(ep["grm"] - ref["grm"])) / np.nanmax(np.abs(ref["grm"])))
    pw.free()
    v.free()
    f = tpg.loci_alt_freq(X)
    out["alt_freq_max_abs"] = float(np.abs(f - ref["freq"][:, 0]).max()) if f.ndim == 1 else float(np.abs(f - ref["freq"]).max())
    gid = (np.arange(n) % G).astype(np.int32)
    vv = api.View(X, None, None, code256=tpg.CODE_012)
    gf = np.zeros((B, 2 * G), order="F")
    pl = np.full(n, 2.0)  # kept alive across the call (a temporary's buffer may be gone by the time the library reads it)
    tpg._lib.check(st.lib.tpg_grouped_alt_freq_dip_pseudo(ctx.h, vv.h, api._ptr(gid), C.c_int(G), api._ptr(pl),
                                                          C.c_int(0), api._ptr(gf)))
    vv.free()
    out["grouped_alt_freq_max_abs"] = float(np.nanmax(np.abs(gf - ref["gfreq"])))
    fst_rel = 0.0
    for method in ("Hudson", "WC84"):
        t = tpg.pairwise_pop_fst(X, None, None, gid, G, method=method)["fst_tot"]
        fst_rel = max(fst_rel, max_rel(np.asarray(t), np.asarray(ref[method])))
    out["fst_max_rel"] = fst_rel
    # PCA: d of the polymorphic loci of the sample against sqrt of the top eigenvalues of the oracle's BLAS Gram (LAPACK)
    dec = np.where(fbm > 3, fbm - 4, fbm).astype(np.int64)
    alt = dec.sum(axis=0)
    pc = (np.where((alt > 0) & (alt < 2 * n))[0] + 1).astype(np.int32)
    t = tpg.gt_pca_partialSVD(X, None, pc, k=k)
    from scipy.linalg import eigh

    # d against the top eigenvalues
    # ... and the SCORES u d (what BASELINE's metric names) against the eigenvectors of the same matrix: an eigenvector is
    # determined up to (difference of the two Gram matrices, ~1e-10 lambda_1) / (gap to its neighbours), so the figure is
    # reported beside the bound that gap allows (tests/test_gpu_oracle_at_scale.py asserts the same at full size)
    lam_top, U_top = eigh(Kp, subset_by_index=[max(0, n - k - 1), n - 1])
    lam_all, U_all = lam_top[::-1], U_top[:, ::-1]
    lam, U = lam_all[:k], U_all[:, :k]
    out["pca_d_max_rel"] = float(np.max(np.abs(t["d"] / np.sqrt(lam) - 1)))
    sign = np.sign((U * t["u"]).sum(axis=0))
    sign[sign == 0] = 1
    s_ref, s_dev = U * sign * np.sqrt(lam), t["u"] * t["d"]
    rel = np.abs(s_dev - s_ref).max(axis=0) / np.abs(s_ref).max(axis=0)
    below = np.abs(np.diff(lam_all[:k + 1])) if len(lam_all) > k else np.abs(np.diff(np.append(lam, 0.0)))
    gaps = np.minimum(below, np.abs(np.diff(np.concatenate([[np.inf], lam]))))
    bound = np.maximum(1e-6, 1e-10 * lam[0] / gaps * np.sqrt(n))
    out["pca_scores_max_rel"] = float(rel.max())
    out["pca_scores_max_rel_over_bound"] = float((rel / bound).max())
    out["pca_scores_note"] = ("max over the k components of max_i |u_ik d_k - ref| / max_i |ref|, sign-aligned, against LAPACK eigh of the "
                              "oracle's FP64 BLAS Gram matrix; _over_bound divides by max(1e-6, 1e-10 lambda_1 / gap_k sqrt(n)): <= 1 "
                              "means every component is inside what its spectral gap allows")
    X.free()
    return out


def launch_ranks(args):
    """`python bench.py --gpus N` without a launcher around it: start N fresh rank processes through
    torch.distributed.run (one per GPU) and hand on rank 0's JSON line and the children's exit code.  This process never
    touches the GPU (counting devices does not initialise HIP); the ranks are new processes, not a re-exec."""
    import socket
    import subprocess

    n = args.gpus
    if os.environ.get("TPG_BENCH_SHARE_GPU") not in ("1", "rccl"):  # rehearsal modes put every rank on device 0
        import torch

        have = torch.cuda.device_count()
        if have < n:
            sys.stderr.write(f"[bench] --gpus {n} asked for, {have} HIP device(s) visible: refusing to report a "
                             f"{n}-GPU line from fewer GPUs (TPG_BENCH_SHARE_GPU=1 rehearses the sharded path on one)\n")
            return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: what RCCL needs between processes on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // n)))
    return subprocess.call(cmd, env=env)


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1:
            sys.exit(launch_ranks(args))
    elif int(os.environ["WORLD_SIZE"]) != args.gpus:
        sys.stderr.write(f"[bench] --gpus {args.gpus} but the launcher started WORLD_SIZE={os.environ['WORLD_SIZE']} ranks\n")
        sys.exit(2)
    # stdout carries exactly one JSON line: libraries that print to fd 1 (RCCL's version banner on communicator
    # creation, for one) are sent to stderr for the whole run, the result goes to the saved descriptor
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        import torch.distributed as dist

        dist.init_process_group("gloo")  # control plane only: RCCL id, barriers, the max over ranks of the time
    # one process per GPU: each rank stays on the host NUMA node of its GPU (tpg_host_bind_near_device, what a launcher's
    # `numactl --cpunodebind` does) -- the host-side legs (end_to_end, dropin) run 20 - 25 % faster with their teams and
    # buffers on one socket; the GPU-resident step does not care.  --no-numa-bind: leave the scheduler alone.
    numa_node = None
    if not args.no_numa_bind:
        import tidypopgen_amd as _tpg

        try:
            numa_node = _tpg.bind_host_near_device(local_rank % max(1, _tpg.device_count()))
        except Exception as e:  # (an optimisation of the host-side legs: never a reason to lose the line)
            sys.stderr.write(f"[bench] rank {rank}: not bound to a NUMA node: {e}\n")
    st = Step(args, rank, world, local_rank)
    st.numa_node = numa_node
    from tidypopgen_amd import sharding

    for _ in range(args.warmup):
        st.run()
    # The timed region brackets only the MFMA kernels the roofline prices with HIP events (on the stream they run on): two
    # event records around a launch cost ~5 us of idle GPU each, and a step has 70 - 170 launches.  The per-kernel table
    # (kernel_ms_per_step, roofline_other_kernels) comes from a second, untimed pass with every launch bracketed (--full).
    # With several ranks the class exchange's all-to-all is bracketed too: config.pca_gram_path names the path by it.
    ROOF_KEYS = ["pairwise_mfma", "pca_gram_mfma", "pca_gram_classes"]
    st.ctx.prof_enable(True)
    st.ctx.prof_only(ROOF_KEYS + (["gclx_alltoall"] if world > 1 else []))
    st.ctx.prof_reset()
    st.barrier_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        st.run()
    st.barrier_sync()
    dt = time.perf_counter() - t0
    if world > 1:
        dt = float(sharding.all_reduce_numpy(np.array([dt]), op="max")[0])
    prof_timed = st.ctx.prof_dump()
    if args.dump_outputs:
        dump_outputs(st, args.dump_outputs)
    prof = dict(prof_timed)
    table_steps = ms_per_step_all_events = None
    if args.full:
        table_steps = max(2, min(args.steps, 10))
        st.ctx.prof_only(None)
        st.ctx.prof_reset()
        st.barrier_sync()
        t1 = time.perf_counter()
        for _ in range(table_steps):
            st.run()
        st.barrier_sync()
        ms_per_step_all_events = (time.perf_counter() - t1) / table_steps * 1e3
        prof_table = st.ctx.prof_dump()
        # one dictionary, per `args.steps` steps: the roofline kernels from the timed region, the others scaled from the table pass
        prof = {k_: (v_[0] * args.steps / table_steps, v_[1] * args.steps / table_steps) for k_, v_ in prof_table.items()}
        prof.update(prof_timed)
    st.ctx.prof_enable(False)
    dig = digest(st) if args.digest else None
    if rank == 0 and args.digest:
        with open(args.digest, "w") as f:
            json.dump(dig, f)
    if rank == 0:
        n, m = args.n, st.m  # m: this rank's loci (what one launch of a kernel processes)
        total_genotypes = n * st.m_total
        ms_per_step = dt / args.steps * 1e3
        traffic_src = os.path.join(ROOT, "profiles", "traffic.json")
        TRAFFIC, TRAFFIC_META = {}, {}
        if (n, m, args.pops, args.k) == (5000, 1000000, 51, 20):
            try:
                with open(traffic_src) as f:
                    TRAFFIC_META = json.load(f)
                TRAFFIC = TRAFFIC_META["hbm_bytes_per_launch"]
            except (OSError, KeyError, ValueError):
                TRAFFIC, TRAFFIC_META = {}, {}

        def avg(key):
            cnt, ms = prof.get(key, (0, 0.0))
            return (ms / cnt) if cnt else None

        # MFMA-bound kernels, priced on ALGORITHMIC ops per launch against the dense peak of the
        # MFMA they issue: 5 POP/s int8 (v_mfma_i32_32x32x32_i8), 10 PFLOP/s FP4 (v_mfma_scale_f32_32x32x64_f8f6f4)
        def mfma_roof(key, kernel, ops, note, peak=5000.0):
            t = avg(key)
            if t is None:
                return None
            achieved = ops / (t * 1e-3) / 1e12
            return {"bound": "mfma", "kernel": kernel, "achieved": achieved, "peak": peak, "unit": "TOP/s",
                    "frac": achieved / peak, "traffic": TRAFFIC.get(key),
                    "traffic_from": (f"STORED profile, not measured in this run: profiles/traffic.json <- {TRAFFIC_META.get('source')} "
                                     f"(rocprofv3 --pmc passes of this workload, {TRAFFIC_META.get('date', 'date not recorded')}, commit "
                                     f"{TRAFFIC_META.get('commit', 'not recorded')})") if TRAFFIC.get(key) else None,
                    "avg_launch_ms": t, "algorithmic_ops_per_launch": ops, "note": note}

        m_pca = st.m_pca if st.has_pca else m
        G, P, k = args.pops, st.P, args.k
        Cpad = 32 * -(-G // 32)
        roofs = [
            mfma_roof("pairwise_mfma", "tpg_pairwise_kernel (v_mfma_scale_f32_32x32x64_f8f6f4, FP4 operands)", 5.0 * n * n * m,
                      "fused IBS+KING+AS/GRM: 3 symmetric + 1 general product = 2.5 N^2 M MACs on exact FP4 planes "
                      "(0.5 / 1 / +-2 with block scales, integer sums in FP32 below 2^24); peak = dense FP4 at 2.4 GHz; the MFMA pipe is "
                      "89 % busy at the 1.87 - 2.05 GHz the chip holds under this kernel (profiles/r05_pmc_one_step.json); that clock is a "
                      "POWER limit that depends on the operand data: the same kernel on constant genotypes runs at 0.76 - 0.78 of the peak, "
                      "the rate of the bare instruction loop on constant registers (7.7 POP/s, tools/ubench_mfma_fp4.hip), at a measured "
                      "2.1 - 2.2 GHz instead of 1.83 - 1.89 (profiles/r05_pairwise_experiments.txt, DESIGN.md 3.1)",
                      peak=10000.0),
            mfma_roof("pca_gram_mfma", "tpg_pca_gram_kernel (v_mfma_i32_32x32x32_i8)", 4.0 * n * n * m_pca,
                      "PCA Gram: 4 weight digits x symmetric int8 product = 4 * N^2 M / 2 MACs"),
            mfma_roof("pca_gram_classes", "tpg_gcls_gram2_kernel / tpg_gcls_gram_kernel (v_mfma_scale_f32_32x32x64_f8f6f4, FP4 "
                      "dosages from 2-bit codes)", 1.0 * n * n * m_pca,
                      "PCA Gram by weight classes: ONE unweighted symmetric product = N^2 M / 2 MACs on exact FP4 dosages "
                      "(2-bit codes over the L2 -> CU path, made FP4 operand words by one v_and_b32 each: the odd block of a "
                      "block pair is stored as centred dosages in the high halves of the nibbles, 4 VALU per MFMA); a class "
                      "end is 8 v_pk_fma_f32 per 32 x 32 tile (small weight differences of a group of neighbouring classes, "
                      "summation by parts), a group end the FP64 fold; 64 x 64 wave tiles, two waves per SIMD; each wave waits "
                      "for its own instruction stream and its dependencies (MFMA pipe 42 % busy, 8.4 VALU-class instructions per MFMA, "
                      "s_waitcnt 27 %: profiles/r05_pmc_one_step.json)",
                      peak=10000.0),
        ]
        roofs = [r for r in roofs if r]
        roofs.sort(key=lambda r: -r["avg_launch_ms"])
        roof = roofs[0] if roofs else None

        # the HBM-bound kernels of the path, priced on their algorithmic bytes
        def hbm_roof(key, kernel, nbytes, note):
            t = avg(key)
            if t is None:
                return None
            achieved = nbytes / (t * 1e-3) / 1e9
            return {"bound": "hbm", "kernel": kernel, "achieved": achieved, "peak": 8000.0, "unit": "GB/s",
                    "frac": achieved / 8000.0, "traffic": None, "avg_launch_ms": t,
                    "algorithmic_bytes_per_launch": nbytes, "note": note}

        def valu_roof(key, kernel, flop, note):  # FP64 VALU: 256 CUs x 4 SIMDs x 16 lanes x 2 (FMA) x 2.4 GHz = 78.6 TFLOP/s
            t = avg(key)
            if t is None:
                return None
            achieved = flop / (t * 1e-3) / 1e12
            return {"bound": "fp64-valu", "kernel": kernel, "achieved": achieved, "peak": 78.6, "unit": "TFLOP/s",
                    "frac": achieved / 78.6, "traffic": None, "avg_launch_ms": t, "algorithmic_flop_per_launch": flop,
                    "note": note}

        others = [
            hbm_roof("pack", "tpg_pack_fast_kernel<1>", 1.5 * n * m, "FBM bytes -> two 2-bit layouts: N M read + N M / 2 written"),
            hbm_roof("pack2", "tpg_pack_fast_kernel<2>", 2.0 * n * m,
                     "FBM bytes -> the raw AND the imputed view from one read: N M read + N M written (L of both views, "
                     "N M / 4 each, + the FP4 operand layout T4 of the raw view, N M / 2); FETCH_SIZE of the kernel alone = the algorithmic 5.0 GB; a "
                     "plain device-to-device copy of 5 GB gets 4.5 TB/s on this part (tools/copy_probe.py), a pure read 6.0"),
            hbm_roof("t4_expand", "tpg_t4_expand_kernel", 0.75 * n * m,
                     "2-bit T layout -> FP4 operand nibbles of the pairwise kernel: N M / 4 read + N M / 2 written"),
            hbm_roof("gcls_gather", "tpg_gcls_gather_kernel", 0.5 * n * m_pca,
                     "class-sorted 2-bit operand layout of the PCA Gram: N M / 4 read (128 contiguous bytes per locus of the "
                     "locus-major copy, loci in class order) + N M / 4 written; 16 x 16 tiles of 2-bit codes transposed in registers"),
            hbm_roof("loci_counts", "tpg_loci_counts_sum_kernel", 4.0 * ((((n + 127) // 128) + 1) // 2) * m + 16.0 * m,
                     "per-locus genotype counts from the dwords the pack kernel leaves per chunk of 256 individuals and locus "
                     "(4 B x chunks per locus read + 16 B written; the N M / 4 bytes of the L layout are not read again)"),
            hbm_roof("grouped_counts", "tpg_grouped_counts_kernel (FP4 MFMA one-hot contraction)",
                     0.25 * n * m + 12.0 * Cpad * m,
                     "grouped counts: N M / 4 read once + 3 int32 count planes of Cpad classes per locus written "
                     "(the 3*2*N*Cpad ops per locus run on the FP4 matrix cores with the 2-bit code as the operand: 0.2 ms of "
                     "MFMA time at C4)"),
            hbm_roof("grouped_finalize", "tpg_grouped_finalize_kernel", (12.0 * Cpad + 16.0 * G) * m,
                     "counts -> the m x 2G doubles grouped_alt_freq returns: 12 Cpad B read + 16 G B written per locus"),
            valu_roof("fst_hudson", "tpg_fst_hudson_gemm_kernel (totals as three masked G x M x G products on v_mfma_f64_16x16x4_f64)",
                      12.0 * P * m,
                      "priced at SURVEY.md 8d's ~12 flop per pair-locus against the FP64 VALU peak (the FP64 MFMA has the same rate on "
                      "this part); the kernel itself does 3 * 2 * 64^2 flop per locus (16-wide tiles pad 51 populations to 64)"),
            valu_roof("fst_wc84", "tpg_fst_wc84_tile_kernel (totals, 3 x 2 tiles of populations per thread, reciprocals tabulated by "
                      "valid-allele count)", 45.0 * P * m,
                      "priced at SURVEY.md 8d's ~45 flop per pair-locus; the kernel issues 22 FP64 (27 VALU) instructions and 3.67 "
                      "16-byte LDS reads per pair-locus: LDS bandwidth and VALU issue within 10 % of each other"),
            mfma_roof("loadings_mfma", "tpg_loadings_mfma_kernel (v = Z'u/d)", 2.0 * n * m_pca * 6 * k,
                      "u split into 6 int8 digits: 2 N M 6k ops; HBM side N M / 4 + 4 * 32 ceil(6k/32) B per locus"),
            hbm_roof("pairwise_epilogue", "tpg_pairwise_epilogue_kernel", (20.0 * n * (n + 64) / 2 + 24.0 * n * n) / max(1, world),
                     "5 int32 planes of this rank's band of the triangle read, 3 N x N double outputs written"),
        ]
        analyses = ["pack", "loci_alt_freq", "grouped_alt_freq", "fst_hudson", "fst_wc84", "ibs", "king", "grm"]
        if st.has_pca:
            analyses.append(f"pca_partialSVD_k{args.k}")
        if args.scaling == "strong":
            wl = (f"{n} individuals x {st.m_total} SNPs cut into {world} SNP-block shard(s) of ~{st.m_total // world} loci, "
                  f"51 populations, 2% missing (imputed bytes), seed 3 [BASELINE configs 2-4]")
        else:
            wl = (f"{n} individuals x {args.m} SNPs per GPU ({world} GPU, panel of {st.m_total}), 51 populations, 2% missing "
                  f"(imputed bytes), seed 3 [BASELINE configs 2-4]")
        out = {
            "metric": "SNP-genotypes/s (N x M) for IBS+KING+GRM+Fst+PCA; max |delta| vs CPU ref (cpu_baseline.parity)",
            "value": total_genotypes / (dt / args.steps),
            "unit": "SNP-genotypes/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "fp4-e2m1 operands (exact integers, f32 accumulate) for the cross-products, the PCA Gram and the grouped counts, int8 (int32 accumulate) for the loadings, f64 for statistics",
            "data": "synthetic",
            "host_numa_node": getattr(st, "numa_node", None),  # rank 0 bound to its GPU's node (-1 / null: not bound)
            "config": {"workload": wl, "analyses": analyses, "pca_included": bool(st.has_pca),
                       "pca_gram_path": ("whole weight classes per rank (packed columns by one all-to-all)" if "gclx_alltoall" in prof
                                         else "this rank's loci, weight classes" if "pca_gram_classes" in prof
                                         else "this rank's loci, int8 weight digits"),
                       "collectives": (f"library-owned, transport {getattr(st, 'transport', 'host (gloo) rehearsal')}: reduce-scatter of int32 pairwise "
                                       "slabs, all-reduce of Fst sums and of the FP64 Gram (upper triangle), all-to-all of the packed columns "
                                       "(whole weight classes per rank) when the PCA's cost model takes it")
                       if world > 1 else "none (one rank)"},
            "roofline": roof,
            "roofline_other_kernels": roofs[1:] + [r for r in others if r],
            "kernel_ms_from": (f"HIP events; {', '.join(k_ for k_ in ROOF_KEYS if k_ in prof_timed)} inside the timed region, the other "
                               f"kernels in a second pass of {table_steps} steps with every launch bracketed "
                               f"({ms_per_step_all_events:.3f} ms per step with all the events in the stream)" if args.full else
                               f"HIP events; {', '.join(k_ for k_ in ROOF_KEYS if k_ in prof_timed)} inside the timed region "
                               f"(the other kernels: --full)"),
            "kernel_ms_per_step": {k_: round(v_[1] / args.steps, 4) for k_, v_ in sorted(prof.items())},
            "kernel_launches_per_step": {k_: v_[0] / args.steps for k_, v_ in sorted(prof.items())},
        }
        # the secondary legs (--full) must not take the contract line down with them
        if world == 1 and args.full and not args.no_standalone:
            try:
                out["standalone"] = standalone(st)
            except Exception as e:  # noqa: BLE001
                out["standalone"] = {"failed": f"{type(e).__name__}: {e}"}
        if world == 1 and args.full and not args.no_end_to_end:
            try:
                out["end_to_end"] = end_to_end(st)
            except Exception as e:  # noqa: BLE001
                out["end_to_end"] = {"failed": f"{type(e).__name__}: {e}"}
            if "dropin" in out["end_to_end"]:
                out["dropin"] = out["end_to_end"].pop("dropin")
        # cpu_baseline is MEASURED at N = 1 only (rank 0, this host's cores).  It is a property of the host and the panel shape, not
        # of the GPU count, so an N > 1 line carries the figure of the N = 1 run of the same shape on this host when there is one
        # (the driver runs N = 1, 2, 4, 8 back to back), else the committed figure of an earlier round -- labelled as such, never
        # re-timed beside RCCL ranks that own the cores.
        cache = os.path.join(tempfile.gettempdir(), f"tpg_cpu_baseline_{args.n}x{args.m}_G{args.pops}_k{args.k}.json")
        if args.full and not args.no_cpu_baseline and world == 1:
            try:
                out["cpu_baseline"] = cpu_baseline(args, st)
            except Exception as e:  # noqa: BLE001 -- (its parity block already guards itself; this is for the CPU timing)
                out["cpu_baseline"] = {"failed": f"{type(e).__name__}: {e}"}
            try:
                with open(cache, "w") as f:
                    json.dump({"measured_unix_time": time.time(), "host": os.uname().nodename, "cpu_baseline": out["cpu_baseline"]}, f)
            except OSError:
                pass
        elif args.full and not args.no_cpu_baseline:
            cb = None
            try:
                with open(cache) as f:
                    c = json.load(f)
                cb = dict(c["cpu_baseline"])
                cb["cached_from"] = (f"the N = 1 run of this shape on this host ({c.get('host')}), "
                                     f"{time.time() - c['measured_unix_time']:.0f} s before this line: not re-timed at N = {world}")
            except (OSError, KeyError, ValueError):
                try:
                    with open(os.path.join(ROOT, "profiles", "cpu_baseline_reference.json")) as f:
                        c = json.load(f)
                    if c.get("shape") == [args.n, args.m if args.scaling == "weak" else st.m_total, args.pops, args.k]:
                        cb = dict(c["cpu_baseline"])
                        cb["cached_from"] = f"profiles/cpu_baseline_reference.json ({c.get('origin')}): ANOTHER host, not re-timed at N = {world}"
                except (OSError, KeyError, ValueError):
                    cb = None
            if cb is not None:
                cb.pop("parity", None)  # the parity block belongs to the run that computed it
                out["cpu_baseline"] = cb
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        st.comm.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
