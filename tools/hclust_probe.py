#!/usr/bin/env python3
"""The Ward route of gt_cluster_pca_ward (include/tpg.h "Ward clustering on PCA scores") on synthetic PCA scores: n points in d
dimensions drawn around `blobs` centres.  Wall clock of the tree (3 (n - 1) + 3 launches queued back to back), of the cuts at
k = 1 .. n / 10 on the host and of the one tpg_cluster_wss call; the wall clock per merge step, which at these sizes is the cost
of three launches; the mean and the maximum length of the recompute list per step; the HIP-event time per kernel of a second
run; and scipy.cluster.hierarchy.linkage on the same host for the same scores where scipy imports.  For the record: no figure
here is a pass criterion.

    python tools/hclust_probe.py [n d blobs [n2]]     default 5000 20 8 16000; writes profiles/hclust_probe.txt"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")


def probe(tpg, ctx, n, d, blobs, lines, with_events):
    rng = np.random.default_rng(1)
    scores = np.asfortranarray(rng.normal(size=(blobs, d))[rng.integers(0, blobs, size=n)] * 3.0 + rng.normal(size=(n, d)))
    kmax = min(max(int(round(n / 10)), 1), 1024)  # (tpg_cluster_wss takes k up to TPG_KMEANS_MAX_K)
    ks = list(range(1, kmax + 1))
    lines.append(f"scores {n} x {d}, {blobs} Gaussian blobs; S is {8 * n * n / 2 ** 20:.0f} MiB")
    for power, name in ((2, "reference (d^4)"), (1, "ward (d^2)")):
        ctx.sync()
        t0 = time.perf_counter()
        tree = tpg.hclust_ward(scores, power=power, return_list_len=True)
        t_tree = time.perf_counter() - t0
        t0 = time.perf_counter()
        labels = tpg.hclust_cut(tree, ks)
        t_cut = time.perf_counter() - t0
        t0 = time.perf_counter()
        wss = tpg.cluster_wss(scores, labels, ks)
        t_wss = time.perf_counter() - t0
        ll = tree["list_len"][1:]  # (entry 0 is the first fill, all n rows)
        lines.append(f"  {name}: tree {t_tree * 1e3:.0f} ms = {t_tree / (n - 1) * 1e6:.1f} us per merge step of 3 launches; cuts at k = 1 .. "
                     f"{kmax} {t_cut * 1e3:.0f} ms (host); one tpg_cluster_wss call for {kmax} labellings {t_wss * 1e3:.0f} ms")
        lines.append(f"    recompute list per step: mean {ll.mean():.2f}, max {int(ll.max())} of n = {n}; heights that fall below "
                     f"their predecessor: {int((np.diff(tree['height']) < 0).sum())}; WSS(1) {wss[0]:.6e}, WSS({kmax}) {wss[-1]:.6e}")
    if with_events:
        ctx.prof_enable(True)
        ctx.prof_reset()
        t0 = time.perf_counter()
        tpg.hclust_ward(scores, power=2)
        wall = time.perf_counter() - t0
        prof = ctx.prof_dump()
        ctx.prof_enable(False)
        lines.append(f"  reference again with every launch bracketed by HIP events: wall {wall * 1e3:.0f} ms")
        for kname, (cnt, ms) in sorted(prof.items()):
            if kname.startswith("hc_"):
                lines.append(f"    {kname:10s} {ms:10.2f} ms in {cnt} launches = {ms / cnt * 1e3:.1f} us each")
    try:
        from scipy.cluster.hierarchy import linkage
        from scipy.spatial.distance import pdist
    except ImportError:
        lines.append("  scipy does not import on this host: no CPU figure")
        return
    t0 = time.perf_counter()
    y = pdist(scores) ** 2
    t_dist = time.perf_counter() - t0
    t0 = time.perf_counter()
    Z = linkage(y, "ward")
    t_link = time.perf_counter() - t0
    ours = np.sort(np.sqrt(tpg.hclust_ward(scores, power=2)["height"]))
    lines.append(f"  scipy on this host, one tree: pdist^2 {t_dist * 1e3:.0f} ms + linkage(., 'ward') {t_link * 1e3:.0f} ms (the reference "
                 f"builds {kmax} such trees, one per k); sorted heights agree to {np.max(np.abs(ours - np.sort(Z[:, 2])) / np.sort(Z[:, 2])):.1e}")


def main():
    import tidypopgen_amd as tpg

    args = [int(a) for a in sys.argv[1:5]]
    n, d, blobs, n2 = args + [5000, 20, 8, 16000][len(args):]
    ctx = tpg.default_context()
    tpg.hclust_ward(np.asfortranarray(np.random.default_rng(0).normal(size=(300, d))))  # warm-up: code objects, the pool
    lines = []
    probe(tpg, ctx, n, d, blobs, lines, True)
    probe(tpg, ctx, n2, d, blobs, lines, False)
    lines.append("worst case of the recompute list: a star (every row's nearest later neighbour is one point) sends all live rows to the "
                 "list in one step, n row scans; tests/test_gpu_hclust.py builds one on 129 points")
    text = "\n".join(lines)
    print(text)
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "hclust_probe.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
