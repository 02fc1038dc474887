#!/usr/bin/env python3
"""Trees from a pairwise matrix (include/tpg.h "Trees from a pairwise matrix") on the Euclidean distance matrix of n synthetic
points drawn around `blobs` centres, kept in HBM as a DeviceMatrix: wall clock per tree and per step of complete and average
linkage (3 (n - 1) launches queued back to back) and of neighbour-joining (3 (n - 2) launches), the best and the median of
`reps` runs after one warm-up run; the HIP-event time per kernel of one further run at the first size; the bytes the neighbour-joining row scan
reads, counted from the join list, over the event time of that kernel; and scipy.cluster.hierarchy.linkage on the same host for
the same matrix where scipy imports.  For the record: no figure here is a pass criterion.

    python tools/tree_probe.py [n reps [n2 reps2]]     default 5000 5 16000 2; writes profiles/tree_probe.txt"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")


def matrix(n, d=20, blobs=8):
    rng = np.random.default_rng(1)
    x = rng.normal(size=(blobs, d))[rng.integers(0, blobs, size=n)] * 3.0 + rng.normal(size=(n, d))
    sq = (x * x).sum(axis=1)
    D = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * (x @ x.T), 0.0))
    D = np.tril(D, -1)
    return np.asfortranarray(D + D.T)


def timed(ctx, reps, f):
    f()  # warm-up: code objects, the pool's blocks of this size
    ts = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return out, min(ts), float(np.median(ts))


def scan_bytes(n, join_b):
    """what nj_rowmin reads of S: for every live row i the n - 1 - i doubles right of its diagonal, at every join"""
    per_join, total = 8 * (n * (n - 1) // 2), 0
    for b in join_b.tolist():
        total += per_join
        per_join -= 8 * (n - 1 - b)
    return total


def events(tpg, ctx, f, prefixes):
    ctx.prof_enable(True)
    ctx.prof_reset()
    t0 = time.perf_counter()
    f()
    wall = time.perf_counter() - t0
    prof = ctx.prof_dump()
    ctx.prof_enable(False)
    return wall, {k: v for k, v in sorted(prof.items()) if k.startswith(prefixes)}


def probe(tpg, ctx, n, reps, lines, with_events):
    D = matrix(n)
    M = tpg.DeviceMatrix.from_numpy(D, ctx)
    lines.append(f"n = {n}: Euclidean distances of {n} points in 20 dimensions around 8 centres; D and S are {8 * n * n / 2 ** 20:.0f} MiB each; "
                 f"1 warm-up run, then {reps} timed runs (best / median), D in HBM")
    trees = {}
    for method in ("complete", "average"):
        tree, best, med = timed(ctx, reps, lambda: tpg.hclust_dist(M, method))
        trees[method] = tree
        lines.append(f"  hclust_dist {method:8s}: tree {best * 1e3:.1f} / {med * 1e3:.1f} ms = {best / (n - 1) * 1e6:.1f} us per merge step of 3 launches "
                     f"(Ward on scores: 21 us, profiles/hclust_probe.txt); heights that fall: {int((np.diff(tree['height']) < 0).sum())}")
    nj, best, med = timed(ctx, reps, lambda: tpg.nj(M))
    nbytes = scan_bytes(n, nj["join_b"])
    lines.append(f"  nj: tree {best * 1e3:.1f} / {med * 1e3:.1f} ms = {best / (n - 2) * 1e6:.1f} us per join of 3 launches; the row scan reads "
                 f"{nbytes / 1e9:.1f} GB of S over the tree (first join {8 * (n * (n - 1) // 2) / 1e6:.0f} MB) = {nbytes / best / 1e12:.2f} TB/s over the wall clock "
                 f"of the whole tree; negative branch lengths: {int((nj['len_a'] < 0).sum() + (nj['len_b'] < 0).sum())}")
    runs = (("hclust_dist complete", lambda: tpg.hclust_dist(M, "complete"), ("hc_", "tr_")), ("nj", lambda: tpg.nj(M), ("nj_", "tr_")))
    for name, f, prefixes in runs if with_events else ():
        wall, prof = events(tpg, ctx, f, prefixes)
        lines.append(f"  {name} again with every launch bracketed by HIP events: wall {wall * 1e3:.0f} ms")
        for kname, (cnt, ms) in prof.items():
            extra = f"; {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s of S" if kname == "nj_rowmin" else ""
            lines.append(f"    {kname:10s} {ms:10.2f} ms in {cnt} launches = {ms / cnt * 1e3:.1f} us each{extra}")
    M.free()
    try:
        from scipy.cluster.hierarchy import linkage
        from scipy.spatial.distance import squareform
    except ImportError:
        lines.append("  scipy does not import on this host: no CPU figure")
        return
    y = squareform(D, checks=False)
    for method in ("complete", "average"):
        t0 = time.perf_counter()
        Z = linkage(y, method)
        t_link = time.perf_counter() - t0
        ours = np.sort(trees[method]["height"])
        lines.append(f"  scipy on this host, linkage(., '{method}') once: {t_link * 1e3:.0f} ms; sorted heights agree to "
                     f"{np.max(np.abs(ours - np.sort(Z[:, 2]))):.1e} absolute")


def main():
    import tidypopgen_amd as tpg

    args = [int(a) for a in sys.argv[1:5]]
    n, reps, n2, reps2 = args + [5000, 5, 16000, 2][len(args):]
    ctx = tpg.default_context()
    lines = []
    probe(tpg, ctx, n, reps, lines, True)
    probe(tpg, ctx, n2, reps2, lines, False)
    text = "\n".join(lines)
    print(text)
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "tree_probe.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
