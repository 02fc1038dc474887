#!/usr/bin/env python3
"""LD-kNN imputation (View.impute_knn, include/tpg.h "LD-kNN imputation") at 5 000 x 1 000 000 with 2 % missing, l = 10,
k = 8 and an index window of 100 loci: HIP-event times per kernel and the wall clock of the call (medians of three after a
warm-up, one job).  For scale, on the same panel in the same job: View.impute("mode"), and the numpy restatement
(tests/knn_impute_ref.py) on a slice of 2 000 loci, extrapolated to the panel and labelled as such.

    python tools/knn_impute_probe.py [n m width l k slice]"""
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import tidypopgen_amd as tpg
from tests import knn_impute_ref as kr

REPS = 3
KERNELS = ("impute_view", "loci_counts", "knn_prep", "knn_band", "knn_select", "knn_list", "knn_vote")


def probe(n=5000, m=1_000_000, width=100, l=10, k=8, nslice=2000, miss=0.02):
    ctx = tpg.default_context()
    ctx.prof_enable(True)
    X = tpg.FBM.synth(5, n, m, npop=8, miss=miss)
    v = tpg.View(X, code256=None)
    hi = np.minimum(np.arange(m, dtype=np.int64) + width, m - 1)
    rows, mode_wall = [], []
    rep_d = None
    for rep in range(REPS + 1):
        ctx.sync(); ctx.prof_reset()
        t0 = time.perf_counter()
        f = v.impute_knn(hi, l, k)
        ctx.sync()
        wall = time.perf_counter() - t0
        prof = ctx.prof_dump()
        rep_d = f.impute_report
        f.free()
        t0 = time.perf_counter()
        w = v.impute("mode")
        ctx.sync()
        mw = time.perf_counter() - t0
        w.free()
        if rep:
            rows.append([prof.get(kn, (0, 0.0))[1] for kn in KERNELS] + [wall * 1e3])
            mode_wall.append(mw * 1e3)
    med = [statistics.median(c) for c in zip(*rows)]
    print(f"panel {n} x {m}, {miss:.0%} missing, l = {l}, k = {k}, window {width} loci; medians of {REPS} after a warm-up")
    print(f"  report: {rep_d}")
    print(f"  planned scratch (tpg_knn_impute_scratch_bytes): {tpg.knn_impute_scratch_bytes(n, m, width, l) / 2 ** 20:.0f} MiB")
    for kn, x in zip(KERNELS, med):
        print(f"  {kn:<20s} {x:10.3f} ms")
    print(f"  View.impute_knn wall {med[-1]:10.3f} ms   (all runs: {', '.join(f'{r[-1]:.1f}' for r in rows)})")
    print(f"  View.impute('mode') wall {statistics.median(mode_wall):8.3f} ms")
    pairs = float(rep_d["imputed"] + rep_d["entries_left"]) * n
    print(f"  pairs of individuals in the vote: {pairs:.3e}; {pairs / (med[KERNELS.index('knn_vote')] * 1e-3):.3e} pairs / s")
    # the numpy restatement on a slice, once
    ns = min(nslice, m)
    if ns < 1:
        return
    codes =tpg.View(X, None, np.arange(1, ns + 1, dtype=np.int32), code256=None).unpack()
    t0 = time.perf_counter()
    kr.impute(codes, np.minimum(np.arange(ns, dtype=np.int64) + width, ns - 1), l, k)
    t = time.perf_counter() - t0
    print(f"  numpy restatement on {ns} loci: {t:.2f} s; EXTRAPOLATED to {m} loci: {t * m / ns:.0f} s")
    v.free(); X.free()


if __name__ == "__main__":
    probe(*(int(x) for x in sys.argv[1:7]))
