#!/usr/bin/env python3
"""The least-squares projection (include/tpg.h "least-squares projection") at the sizes it is for, beside the route it does not
replace: predict_gt_pca_lsq (one device call: the MFMA sweep, the reduce, the batched Cholesky solve) and
predict_gt_pca(project_method="least_squares") (the host table of pair products, two generic sweeps, numpy solves row by row)
in the same job on the same synthetic panel and the same loadings.  Per shape: the wall time of each call from host arrays to
host arrays (both pack their own view of the store; the calls end synchronised), new - old - new so that a drift shows; the new
call's kernels by HIP events in a further call (lsq_sweep, lsq_reduce, lsq_solve apart); the sweep's FP64 rate from
2 n m (P + L + 1) flops over its kernel time; and the largest difference between the two results.  Every shape is one step, run
as a child process under its own time limit, and a step that fails ends the probe.  For the record: no figure here is a pass
criterion.

    python tools/lsq_probe.py          writes profiles/lsq_probe.txt"""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

SHAPES = [(5000, 1000000, 2), (5000, 1000000, 10), (5000, 1000000, 20), (100000, 100000, 10)]
LIMIT_S = 420
OUT = os.path.join("profiles", "lsq_probe.txt")


def step(n, m, L):
    import tidypopgen_amd as tpg

    ctx = tpg.default_context()
    rng = np.random.default_rng(L)
    V = np.asfortranarray(np.linalg.qr(rng.standard_normal((m, L)))[0])
    p = rng.uniform(0.05, 0.95, m)
    pca = dict(v=V, center=2.0 * p, scale=np.sqrt(2.0 * p * (1.0 - p)))
    pcs = tuple(range(1, L + 1))
    small = tpg.FBM.synth(3, 64, 256, npop=4, miss=0.05)
    sp = dict(v=V[:256], center=pca["center"][:256], scale=pca["scale"][:256])
    tpg.predict_gt_pca_lsq(sp, small, lsq_pcs=pcs)  # warm-up: code objects, the pool
    tpg.predict_gt_pca(sp, small, project_method="least_squares", lsq_pcs=pcs)
    X = tpg.FBM.synth(7, n, m, npop=4, miss=0.05)
    ctx.sync()

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        return time.perf_counter() - t0, out

    t_new1, (x, sing) = timed(lambda: tpg.predict_gt_pca_lsq(pca, X, lsq_pcs=pcs, return_singular=True))
    print(f"{n} x {m}, L = {L}: new {t_new1:.3f} s", flush=True)
    t_old, y = timed(lambda: tpg.predict_gt_pca(pca, X, project_method="least_squares", lsq_pcs=pcs))
    print(f"  old {t_old:.3f} s", flush=True)
    t_new2, (x2, _) = timed(lambda: tpg.predict_gt_pca_lsq(pca, X, lsq_pcs=pcs, return_singular=True))
    same = np.array_equal(x.view(np.uint64), x2.view(np.uint64))
    ctx.prof_enable(True)
    ctx.prof_reset()
    tpg.predict_gt_pca_lsq(pca, X, lsq_pcs=pcs)
    kern = {name: ms for name, (cnt, ms) in ctx.prof_dump().items()}
    ctx.prof_enable(False)
    P = L * (L + 1) // 2
    flops = 2.0 * n * m * (P + L + 1)
    sweep = kern.get("lsq_sweep", float("nan"))
    diff = np.abs(x - y).max() / np.abs(y).max()
    t_new = min(t_new1, t_new2)
    lines = [f"{n} x {m} loci, L = {L} ({P + L + 1} columns), 5% missing, {sing} singular rows",
             f"  predict_gt_pca_lsq: {t_new1:.3f} s and {t_new2:.3f} s wall (same bits: {same}); "
             f"predict_gt_pca(least_squares): {t_old:.3f} s wall; old / new = {t_old / t_new:.1f}",
             f"  kernels of the new call: lsq_sweep {sweep:.2f} ms ({flops / sweep / 1e9:.2f} TFLOP/s FP64 from 2 n m (P + L + 1) = "
             f"{flops:.3g} flops), lsq_reduce {kern.get('lsq_reduce', float('nan')):.2f} ms, lsq_solve "
             f"{kern.get('lsq_solve', float('nan')):.2f} ms; all: " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(kern.items())),
             f"  largest |new - old| / max |old|: {diff:.2e}"]
    text = "\n".join(lines)
    print(text, flush=True)
    with open(OUT, "a") as f:
        f.write(text + "\n")
    return 0


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--step":
        return step(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    os.makedirs("profiles", exist_ok=True)
    with open(OUT, "w") as f:
        f.write("tools/lsq_probe.py: predict_gt_pca_lsq beside predict_gt_pca(project_method=\"least_squares\"), one job, one panel per shape\n")
    # every step that uses the GPU runs as a child under its own time limit; nothing follows a step that failed
    for n, m, L in SHAPES:
        try:
            r = subprocess.run([sys.executable, __file__, "--step", str(n), str(m), str(L)], timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"no result within {LIMIT_S} s", flush=True)
            return 1
        if r.returncode != 0:
            print(f"exit status {r.returncode}", flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
