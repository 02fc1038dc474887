#!/usr/bin/env python3
"""Site frequency spectra (include/tpg.h "site frequency spectra") at the sizes they are for, from a packed view of a synthetic
5 000 x 1 000 000 panel (51 populations, 2 % missing; individual i belongs to group i mod G):

  1. 51 groups projected to 20 alleles each (W = 1 071), one block
  2. 3 groups projected to 200 each (W = 603), one block
  3. shape 2 in 1 000 equal blocks (jsfs, 2.9 GB, stays in device memory; the other outputs come to the host)

Per shape: one warm-up call, then RUNS timed calls (a host clock around a call that ends in a stream synchronise; median and
range), then ONE further call with HIP events around every launch for the kernel-level split.  The Gram kernel's FP64 rate is
the flops it issues -- 2 x 4096 per staged locus and 64 x 64 tile of the upper triangle of the (W + 1)-wide operand -- over its
kernel time; beside it the rate of pcr_gram_kernel (pcrelate.hip: 3 n^2 m flops over its kernel time) measured IN THE SAME JOB
on a 5 000 x 200 000 panel: existing code, the yardstick.  The numpy float route (tests/sfs_ref.py) is timed once on a slice
of 2 000 loci on this host and EXTRAPOLATED by the number of loci -- marked as such.  Every step is a child process under its
own time limit and a step that fails ends the probe.  For the record: no figure here is a pass criterion.

    python tools/sfs_probe.py          writes profiles/sfs_probe.txt"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

N, M = 5000, 1000000
SHAPES = {"1": (51, 20, 1), "2": (3, 200, 1), "3": (3, 200, 1000)}
PCR = (5000, 200000, 10)
SLICE = 2000
RUNS = 3
LIMIT_S = 420
OUT = os.path.join("profiles", "sfs_probe.txt")


def emit(text):
    print(text, flush=True)
    with open(OUT, "a") as f:
        f.write(text + "\n")


def step_sfs(which):
    import tidypopgen_amd as tpg

    G, pj, nb = SHAPES[which]
    lib, check = tpg._lib.lib, tpg._lib.check
    ctx = tpg.default_context()
    small = tpg.View(tpg.FBM.synth(3, 64, 512, npop=4, miss=0.02))
    tpg.sfs_blocks(small, np.arange(64) % 2, 2, [0], [512], proj=4)  # warm-up: code objects, the pool
    v = tpg.View(tpg.FBM.synth(7, N, M, npop=51, miss=0.02))
    gid = np.ascontiguousarray(np.arange(N) % G, dtype=np.int32)
    proj = np.full(G, pj, dtype=np.int32)
    W = G * (pj + 1)
    edges = np.linspace(0, M, nb + 1).astype(np.int64)
    lo, hi = np.ascontiguousarray(edges[:-1]), np.ascontiguousarray(edges[1:])
    sfs, n1 = np.zeros((W, nb), order="F"), np.zeros((G, nb), dtype=np.int64, order="F")
    n2 = np.zeros((G, G, nb), dtype=np.int64, order="F")
    on_device = nb > 1
    jbytes = W * W * nb * 8
    J = None if on_device else np.zeros((W, W, nb), order="F")
    dJ = ctx.dev_alloc(jbytes) if on_device else None
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def call():
        check(lib.tpg_sfs_blocks(ctx.h, v.h, ptr(gid), G, None, ptr(proj), None, None, ptr(lo), ptr(hi), nb, ptr(sfs), ptr(n1),
                                 dJ if on_device else ptr(J), ptr(n2)))
        ctx.sync()

    call()  # warm-up at this shape: the count table of the view, the pool blocks
    walls = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t0)
    ctx.prof_enable(True)
    ctx.prof_reset()
    call()
    kern = ctx.prof_dump()
    ctx.prof_enable(False)
    nt = -(-(W + 1) // 64)
    tiles = nt * (nt + 1) // 2
    flops = 2.0 * 4096 * tiles * float((hi - lo).sum())
    gram_n, gram_ms = kern.get("sfs_gram", (0, float("nan")))
    segs = [tpg.sfs_segments(int(b - a), W) for a, b in zip(lo[:1], hi[:1])][0]
    emit("\n".join([
        f"shape {which}: {N} x {M}, {G} groups projected to {pj} (W = {W}, {tiles} tiles), {nb} block(s) of {int(hi[0] - lo[0])} loci, "
        f"{segs} segment(s) each; scratch {tpg.sfs_scratch_bytes(M, G, W, nb) / 2 ** 20:.0f} MiB; jsfs {'in device memory' if on_device else 'to the host'}",
        f"  tpg_sfs_blocks, {RUNS} runs after a warm-up: median {np.median(walls):.3f} s wall (min {min(walls):.3f}, max {max(walls):.3f}) "
        f"from the packed view to the outputs; n_used1 {int(n1.min())} .. {int(n1.max())} per block, sum of sfs {sfs.sum():.6g}",
        f"  kernels, ONE further run (HIP events): sfs_gram {gram_ms:.1f} ms in {gram_n} launches = {flops / gram_ms / 1e9:.1f} TFLOP/s FP64 "
        f"issued ({flops:.3g} flops); all: " + ", ".join(f"{k} {ms:.1f} ms x{cnt}" for k, (cnt, ms) in sorted(kern.items()))]))
    if on_device:
        ctx.dev_free(dJ)
    return 0


def step_pcrelate():
    import tidypopgen_amd as tpg

    n, m, K = PCR
    ctx = tpg.default_context()
    rng = np.random.default_rng(1)
    pop = np.arange(n) % 4
    cols = [(pop == g).astype(float) - 0.25 for g in range(3)] + [rng.standard_normal(n) for _ in range(K - 3)]
    V = np.asfortranarray(np.column_stack(cols) * np.sqrt(float(m)))
    v = tpg.View(tpg.FBM.synth(7, n, m, npop=4, miss=0.05), code256=None)
    tpg.pcrelate(v, V, return_counts=False)  # warm-up
    ctx.prof_enable(True)
    ctx.prof_reset()
    tpg.pcrelate(v, V, return_counts=False)
    kern = ctx.prof_dump()
    ctx.prof_enable(False)
    cnt, ms = kern.get("pcrelate_gram", (0, float("nan")))
    flops = 3.0 * n * n * m
    emit(f"yardstick, same job: pcr_gram_kernel at {n} x {m}, K = {K}, ONE run after a warm-up: {ms:.1f} ms in {cnt} launches = "
         f"{flops / ms / 1e9:.1f} TFLOP/s FP64 from 3 n^2 m = {flops:.3g} flops")
    return 0


def step_model():
    from tests import sfs_ref as sr

    rng = np.random.default_rng(5)
    codes = rng.binomial(2, rng.uniform(0.05, 0.95, size=SLICE)[None, :], size=(N, SLICE)).astype(np.uint8)
    codes[rng.random((N, SLICE)) < 0.02] = sr.MISSING
    lines = []
    for which in ("1", "2"):
        G, pj, _ = SHAPES[which]
        gid = np.arange(N) % G
        t0 = time.perf_counter()
        x, v = sr.group_tables(codes, gid, G)
        n = sr.proj_sizes(gid, G, np.full(G, pj))
        H = sr.weights_float(x, v, n, sr.usable(v, n))
        sr.blocks_float(H, [0], [SLICE])
        t = time.perf_counter() - t0
        lines.append(f"numpy float route (tests/sfs_ref.py) for shape {which} on a slice of {SLICE} loci, one run on this host: {t:.2f} s; "
                     f"EXTRAPOLATED by the number of loci to {M}: {t * M / SLICE:.0f} s (not measured)")
    emit("\n".join(lines))
    return 0


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--sfs":
        return step_sfs(sys.argv[2])
    if len(sys.argv) == 2 and sys.argv[1] == "--pcrelate":
        return step_pcrelate()
    if len(sys.argv) == 2 and sys.argv[1] == "--model":
        return step_model()
    os.makedirs("profiles", exist_ok=True)
    with open(OUT, "w") as f:
        f.write("tools/sfs_probe.py: tpg_sfs_blocks on a synthetic panel; timed runs and one profiled run per shape\n")
    # every step that uses the GPU runs as a child under its own time limit; nothing follows a step that failed
    for args in [["--sfs", "1"], ["--sfs", "2"], ["--sfs", "3"], ["--pcrelate"], ["--model"]]:
        try:
            r = subprocess.run([sys.executable, __file__, *args], timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"no result within {LIMIT_S} s", flush=True)
            return 1
        if r.returncode != 0:
            print(f"exit status {r.returncode}", flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
