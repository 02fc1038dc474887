#!/usr/bin/env python3
"""Runs of homozygosity (tpg_roh_detect) on a synthetic 5 000 x 1 000 000 panel with 1 % missing, at window sizes 15, 50 and
512: HIP-event times of every ROH kernel (medians of three after a warm-up, one job) and the wall clock of the call, beside the
project's kernel of the same traffic class, tpg_impute_view_kernel in mode "mode" (reads n m / 4 bytes, writes n m / 4), timed
in the same job.  The status stage reads n m / 4 bytes (plus the halo) and writes n m / 8.

    python tools/roh_probe.py [n m]"""
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import tidypopgen_amd as tpg

REPS = 3
KERNELS = ("roh_status", "roh_seg_count", "roh_row_scan", "roh_seg_emit", "roh_filter", "roh_keep_scan", "roh_compact")
ctx = tpg.default_context()
ctx.prof_enable(True)


def med_prof(fn, names):
    rows, walls = [], []
    for rep in range(REPS + 1):
        ctx.sync(); ctx.prof_reset()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        wall = time.perf_counter() - t0
        prof = ctx.prof_dump()
        if rep:
            rows.append([prof.get(k, (0, 0.0))[1] for k in names])
            walls.append(wall)
        if rep < REPS and hasattr(out, "free"):
            out.free()
    return [statistics.median(c) for c in zip(*rows)], walls, out


def probe(n, m):
    X = tpg.FBM.synth(9, n, m, npop=8, miss=0.01)
    v = tpg.View(X)
    rng = np.random.default_rng(9)
    pos = 1000 + np.cumsum(rng.integers(1, 3000, m)).astype(np.int64)
    chrom = (np.arange(m) * 22 // m).astype(np.int32)
    print(f"panel {n} x {m}, synthetic, 1 % missing, 22 chromosomes; medians of {REPS} after a warm-up; "
          f"n m / 4 = {n * m / 4 / 1e9:.3f} GB")
    (imp,), _, vi = med_prof(lambda: v.impute("mode"), ("impute_view",))
    vi.free()
    print(f"  impute_view (mode)  {imp:9.3f} ms   the yardstick: n m / 4 read + n m / 4 written")
    status = {}
    for W in (15, 50, 512):
        med, walls, r = med_prof(lambda: tpg.Roh(v, chrom, pos, window_size=W), KERNELS)
        status[W] = med[0]
        print(f"  W = {W}: {r.count} runs")
        for k, t in zip(KERNELS, med):
            extra = f"   {t / imp:.2f} x impute_view" if k == "roh_status" else ""
            print(f"    {k:14s} {t:9.3f} ms{extra}")
        print(f"    tpg_roh_detect wall {statistics.median(walls) * 1e3:9.3f} ms   (all runs: {', '.join(f'{w * 1e3:.1f}' for w in walls)})")
        t0 = time.perf_counter()
        lc = r.locus_counts()
        n_runs, _ = r.indiv_summary()
        print(f"    locus_counts + indiv_summary wall {(time.perf_counter() - t0) * 1e3:.3f} ms; max locus count {int(lc.max())}, "
              f"runs per individual {n_runs.mean():.1f}")
        r.free()
    print(f"  roh_status at W = 512 against W = 15: {status[512] / status[15]:.2f} x  "
          f"(blocks read per chunk of 16: {16 + 2 * 4} against {16 + 2 * 1})")
    v.free(); X.free()


if len(sys.argv) >= 3:
    probe(int(sys.argv[1]), int(sys.argv[2]))
else:
    probe(5000, 1_000_000)
