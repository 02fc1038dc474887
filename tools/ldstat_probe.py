#!/usr/bin/env python3
"""LD statistics (tpg_ld_stats) at 5 000 x 1 000 000 and at the HGDP-like BASELINE size 1 000 x 650 000, window 500 loci -- the
panels of tools/ld_clump_probe.py -- next to the band kernel of LD clumping (ld_band, through tpg_ld_clump) in the same job:
HIP-event kernel times, medians of three after a warm-up, and the ratio of the two.  Both kernels contract the same band
(tpg_band_contract); what differs is the epilogue, so the ratio prices one FP64 division, two conversions, three LDS atomics and
the row and column sums per pair against one comparison and a ballot.

The variants: both output groups with index distances (bins of one locus), each group alone, and both groups with positions
200 apart in bins of 1 000, where the pairs of a wave instruction fall in one or two bins.

    python tools/ldstat_probe.py [n m window run]"""
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import tidypopgen_amd as tpg

REPS = 3
ctx = tpg.default_context()
ctx.prof_enable(True)


def timed(call, keys):
    rows = []
    for rep in range(REPS + 1):
        ctx.sync(); ctx.prof_reset()
        t0 = time.perf_counter()
        out = call()
        wall = time.perf_counter() - t0
        prof = ctx.prof_dump()
        if rep:
            rows.append([sum(prof.get(k, (0, 0.0))[1] for k in ks) for ks in keys] + [wall * 1e3])
    return out, [statistics.median(c) for c in zip(*rows)]


def probe(n, m, win, run):
    X = tpg.FBM.synth(5, n, -(-m // run), npop=8, miss=0.0)
    v = tpg.View(X, None, (np.arange(m) // run + 1).astype(np.int32))
    hi = np.minimum(np.arange(m, dtype=np.int64) + win, m - 1)
    pos = np.arange(m, dtype=np.int64) * 200
    pairs = float((hi - np.arange(m)).sum())
    print(f"panel {n} x {m}, window {win} loci, runs of {run}; {pairs:.3e} pairs; medians of {REPS} after a warm-up")
    _, (band, wall) = timed(lambda: tpg.ld_clump(v, hi, 0.2), [("ld_band",)])
    print(f"  ld_band (tpg_ld_clump)                   {band:9.3f} ms")
    variants = [("scores + decay, index distances", dict(n_bins=win + 1)),
                ("scores alone", dict(n_bins=0)),
                ("decay alone, index distances", dict(n_bins=win + 1, scores=False)),
                ("scores + decay, positions, bins of 1000", dict(position=pos, bin_size=1000, n_bins=win // 5 + 1))]
    for name, kw in variants:
        r, (k, prep, wall) = timed(lambda: tpg.ld_stats(v, hi, **kw), [("ldstat_band",), ("loci_counts", "ldstat_prep")])
        print(f"  ldstat_band, {name:40s} {k:9.3f} ms   {k / band:5.2f} x ld_band   {k * 1e9 / pairs:6.2f} ps per pair"
              f"   (counts + prep {prep:.3f} ms, tpg_ld_stats wall {wall:.2f} ms)")
    rep = r["report"]
    print(f"  report: {rep}; tiles contracted hold {rep['band_tiles'] * 1024 / max(rep['pairs'], 1):.3f} x the pairs")
    v.free(); X.free()


if len(sys.argv) >= 5:
    probe(*(int(x) for x in sys.argv[1:5]))
else:
    probe(5000, 1_000_000, 500, 64)
    probe(1000, 650_000, 500, 64)
