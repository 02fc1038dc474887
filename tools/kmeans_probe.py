#!/usr/bin/env python3
"""The cluster sweep of gt_cluster_pca (include/tpg.h "k-means on PCA scores") on synthetic PCA scores: n points in d dimensions
drawn around `blobs` centres, n_start runs per k, all runs of all k in one tpg_kmeans_batch call.  Wall clock of the sweep for
k = 1 .. 50 and for the reference's default k = 1 .. n / 10 (after a small warm-up call), the iteration counts, the HIP-event time
per kernel of the large sweep, and -- for k = 1 .. 10 only -- the numpy restatement (tests/kmeans_ref.py) on the CPU beside the
device.  For the record: no figure here is a pass criterion.

    python tools/kmeans_probe.py [n d n_start blobs]     default 5000 20 10 8; writes profiles/kmeans_probe.txt"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")

FP64_VECTOR_TFLOPS = 78.6  # MI355X datasheet


def main():
    import tidypopgen_amd as tpg
    from tests import kmeans_ref as kr

    args = [int(a) for a in sys.argv[1:5]]
    n, d, n_start, blobs = args + [5000, 20, 10, 8][len(args):]
    ctx = tpg.default_context()
    rng = np.random.default_rng(1)
    scores = np.asfortranarray(rng.normal(size=(blobs, d))[rng.integers(0, blobs, size=n)] * 3.0 + rng.normal(size=(n, d)))
    dd = np.sqrt((scores ** 2).sum(axis=0))
    pca = dict(u=np.asfortranarray(scores / dd[None, :]), d=dd)
    lines = [f"scores {n} x {d}, {blobs} Gaussian blobs, n_start = {n_start}, max_iter = 100000, one tpg_kmeans_batch call per sweep"]
    tpg.gt_cluster_pca(pca, k_clusters=(1, 3), n_start=2)  # warm-up: code objects, the pool
    ctx.sync()
    for kmax in (50, max(int(round(n / 10)), 1)):
        t0 = time.perf_counter()
        cl = tpg.gt_cluster_pca(pca, k_clusters=(1, kmax), n_start=n_start, seed=0)["clusters"]
        ctx.sync()
        wall = time.perf_counter() - t0
        runs = 1 + (kmax - 1) * n_start
        it = np.array(cl["n_iter"])
        lines.append(f"k = 1 .. {kmax}: {runs} runs, wall {wall * 1e3:.0f} ms; iterations of the winning runs min / median / max = "
                     f"{it.min()} / {int(np.median(it))} / {it.max()}; not converged {int((~np.array(cl['converged'])).sum())}; "
                     f"winners with an empty centre {int((np.array(cl['n_empty']) > 0).sum())}; BIC minimum at k = {int(np.argmin(cl['BIC'])) + 1}")
    # the large sweep again with every launch bracketed by HIP events, all runs visible
    ks = [1] + [k for k in range(2, kmax + 1) for _ in range(n_start)]
    seeds = [tpg.kmeans_run_seed(0, k, t) for k in range(1, kmax + 1) for t in range(1 if k == 1 else n_start)]
    t0 = time.perf_counter()
    start_rows = [tpg.kmeans_start(s, n, k) for k, s in zip(ks[::max(len(ks) // 50, 1)], seeds[::max(len(ks) // 50, 1)])]
    t_start = (time.perf_counter() - t0) / len(start_rows) * len(ks)
    ctx.prof_enable(True)
    ctx.prof_reset()
    t0 = time.perf_counter()
    r = tpg.kmeans_batch(scores, ks, seeds, return_centers=False)
    wall = time.perf_counter() - t0
    prof = ctx.prof_dump()
    ctx.prof_enable(False)
    it = r["n_iter"].astype(np.int64)
    terms = float((it * np.array(ks, dtype=np.int64)).sum()) * n * d
    lines.append(f"all {len(ks)} runs of k = 1 .. {kmax} (events on): wall {wall * 1e3:.0f} ms; iterations min / median / max = {it.min()} / "
                 f"{int(np.median(it))} / {it.max()}, {int(it.sum())} run-iterations in {int(it.max())} rounds of launches")
    lines.append(f"  start rows on the host (one partial sort of n keys per run): about {t_start * 1e3:.0f} ms of that")
    kern = 0.0
    for name, (cnt, ms) in sorted(prof.items()):
        if name.startswith("km_"):
            lines.append(f"  {name:14s} {ms:10.2f} ms in {cnt} launches")
            kern += ms
    lines.append(f"  kernels together {kern:.1f} ms")
    if "km_assign" in prof:
        ms = prof["km_assign"][1]
        lines.append(f"  assign: {terms:.3e} distance terms (subtract + fused multiply-add) = {3 * terms / ms / 1e9:.2f} TFLOP/s FP64 over "
                     f"{ms:.1f} ms, of {FP64_VECTOR_TFLOPS} vector peak")
    # the numpy restatement beside the device, k = 1 .. 10 only
    t0 = time.perf_counter()
    dev = tpg.gt_cluster_pca(pca, k_clusters=(1, 10), n_start=n_start, seed=0)["clusters"]
    ctx.sync()
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = kr.cluster_pca((pca["u"] * dd[None, :])[:, :d], range(1, 11), n_start=n_start, seed=0)
    t_ref = time.perf_counter() - t0
    same = all(np.array_equal(dev["groups"][k], ref["groups"][k]) for k in range(1, 11))
    lines.append(f"k = 1 .. 10: device {t_dev * 1e3:.0f} ms, numpy restatement on the CPU {t_ref * 1e3:.0f} ms; groups equal: {same}; "
                 f"max |WSS - WSS_ref| / WSS_ref = {np.max(np.abs(dev['WSS'] - ref['WSS']) / ref['WSS']):.2e}")
    text = "\n".join(lines)
    print(text)
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "kmeans_probe.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
