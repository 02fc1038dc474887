#!/usr/bin/env python3
"""LD clumping (tpg_ld_clump) at 5 000 x 1 000 000 with a 500-SNP window, and at the HGDP-like BASELINE size 1 000 x 650 000:
HIP-event kernel times of the band kernel and of the resolution (medians of three after a warm-up, one job), the fraction of the
10 POP/s FP4 peak the band kernel reaches on its algorithmic work 2 n sum_j (hi[j] - j), and the wall clock of the call.

The two large panels: columns of the synthetic store without missing genotypes, each repeated RUN times in a row -- r^2 = 1
inside a run, independent across runs.  The band kernel's time does not depend on the data (every tile of the band is
computed); the resolution's does: there every locus has RUN - 1 links and a run settles in two rounds.  So a third panel,
5 000 x 200 000 made on the host with decaying LD (a haplotype copies the locus before with probability 0.97, as
tests/ld_ref.py's generator does), prices the resolution rounds of a panel that takes more than two.

    python tools/ld_clump_probe.py [n m window run]"""
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import tidypopgen_amd as tpg

REPS = 3
PEAK = 10e15
ctx = tpg.default_context()
ctx.prof_enable(True)


def ld_store(n, m, rho, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, size=m)
    G = np.empty((n, m), dtype=np.uint8, order="F")
    prev = (rng.random(2 * n) < p[0]).astype(np.uint8)
    for j0 in range(0, m, 2000):
        j1 = min(m, j0 + 2000)
        own = (rng.random((2 * n, j1 - j0)) < p[None, j0:j1]).astype(np.uint8)
        copy = rng.random((2 * n, j1 - j0)) < rho
        hap = np.empty((2 * n, j1 - j0), dtype=np.uint8)
        for j in range(j1 - j0):
            if j0 + j > 0:
                prev = np.where(copy[:, j], prev, own[:, j])
            hap[:, j] = prev
        G[:, j0:j1] = hap[:n] + hap[n:]
    return G


def probe(n, m, win, run, thr=0.2, rho=None):
    if rho is None:
        mc = -(-m // run)
        X = tpg.FBM.synth(5, n, mc, npop=8, miss=0.0)
        cols = (np.arange(m) // run + 1).astype(np.int32)
        v = tpg.View(X, None, cols)
        what = f"runs of {run}"
    else:
        X = tpg.FBM.from_numpy(ld_store(n, m, rho, 21), code256=tpg.CODE_012)
        v = tpg.View(X)
        what = f"host panel with decaying LD, rho {rho}"
    hi = np.minimum(np.arange(m, dtype=np.int64) + win, m - 1)
    ops = 2.0 * n * float((hi - np.arange(m)).sum())
    rows = []
    for rep in range(REPS + 1):
        ctx.sync(); ctx.prof_reset()
        t0 = time.perf_counter()
        keep, r = tpg.ld_clump(v, hi, thr, return_report=True)
        wall = time.perf_counter() - t0
        prof = ctx.prof_dump()
        if rep:
            ms = lambda k: prof.get(k, (0, 0.0))[1]
            rows.append((ms("ld_band"), ms("ld_round") + ms("ld_finish"), ms("ld_sort") + ms("ld_key") + ms("ld_rank"),
                         ms("loci_counts") + ms("ld_prep"), wall))
    med = [statistics.median(c) for c in zip(*rows)]
    print(f"panel {n} x {m}, window {win} loci, {what}, thr_r2 {thr}; medians of {REPS} after a warm-up")
    print(f"  report: {r}")
    print(f"  ld_band            {med[0]:9.3f} ms   {ops / (med[0] * 1e-3) / PEAK:.4f} of the 10 POP/s FP4 peak on {ops:.3e} ops")
    print(f"  resolution         {med[1]:9.3f} ms   ({r['rounds']} rounds, {r['finish_loci']} loci left to the walk)")
    print(f"  key + sort + rank  {med[2]:9.3f} ms")
    print(f"  counts + prep      {med[3]:9.3f} ms")
    print(f"  tpg_ld_clump wall  {med[4] * 1e3:9.3f} ms   (all runs: {', '.join(f'{x[4] * 1e3:.2f}' for x in rows)})")
    v.free(); X.free()


if len(sys.argv) >= 5:
    probe(*(int(x) for x in sys.argv[1:5]))
else:
    probe(5000, 1_000_000, 500, 64)
    probe(1000, 650_000, 500, 64)
    probe(5000, 200_000, 500, 0, rho=0.97)
