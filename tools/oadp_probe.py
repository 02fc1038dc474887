#!/usr/bin/env python3
"""The OADP projection (include/tpg.h "OADP projection") at the size it is for: n new individuals against a PCA of K components.
HIP-event time of the projection kernel at K = 20 and K = 10 on synthetic (XV, X_norm, d); the same kernel beside the sweep that
feeds it (tpg_predict_oadp on a synthetic n x m panel, loadings drawn at random); and the numpy restatement (tests/oadp_ref.py),
row by row and on stacks, on this machine's host for n_host individuals.  The measurement is one step, run as a child process
under its own time limit.  For the record: no figure here is a pass criterion.

    python tools/oadp_probe.py [n m n_host]     default 100000 100000 10000; writes profiles/oadp_probe.txt"""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

LIMIT_S = 480


def kernel_ms(ctx, fn, reps=3):
    """fn() `reps` times with every launch bracketed by HIP events -> (the smallest time per launch of each kernel, the result)"""
    best, out = {}, None
    for _ in range(reps):
        ctx.prof_reset()
        out = fn()
        for name, (cnt, ms) in ctx.prof_dump().items():
            best[name] = min(best.get(name, np.inf), ms)
    return best, out


def step(n, m, n_host):
    import tidypopgen_amd as tpg
    from tests import oadp_ref as oref

    ctx = tpg.default_context()
    lines = [f"{n} new individuals; one launch of the projection kernel (one wave per workgroup, 64 / G individuals per wave)"]
    tpg.oadp_proj(*oref.grid_case(0, 64, 3, 10.0))  # warm-up: code objects, the pool
    ctx.sync()
    ctx.prof_enable(True)
    cases = {}
    for K in (20, 10):
        XV, nrm, d = oref.grid_case(K, n, K, 10.0)
        cases[K] = (XV, nrm, d)
        t0 = time.perf_counter()
        best, (out, deg) = kernel_ms(ctx, lambda: tpg.oadp_proj(XV, nrm, d, return_degenerate=True))
        wall = (time.perf_counter() - t0) / 3
        lines.append(f"K = {K}: kernel {best['oadp']:.2f} ms ({best['oadp'] * 1e3 / n:.3f} us per individual), the finite check "
                     f"{best['km_finite']:.2f} ms, the call from host arrays {wall * 1e3:.0f} ms; degenerate rows {deg}")
    # beside the sweep: a synthetic panel, loadings at random with orthonormal columns, d above the norms so that no row is degenerate
    K = 20
    X = tpg.FBM.synth(7, n, m, npop=4)
    rng = np.random.default_rng(2)
    V = np.asfortranarray(np.linalg.qr(rng.standard_normal((m, K)))[0])
    pca = dict(v=V, center=np.full(m, 0.9), scale=np.full(m, 0.7), d=np.linspace(3.0, 1.0, K) * np.sqrt(4.0 * m))
    tpg.predict_gt_pca_oadp(pca, X)  # warm-up (every call packs its own view of X; only kernels are timed below)
    best, (out, deg) = kernel_ms(ctx, lambda: tpg.predict_gt_pca_oadp(pca, X, return_degenerate=True), reps=2)
    sweep = sum(ms for name, ms in best.items() if name.startswith("sweep_"))
    lines.append(f"predict_gt_pca_oadp, {n} x {m} loci, K = {K}: sweep kernels {sweep:.1f} ms, projection kernel {best['oadp']:.2f} ms; "
                 f"degenerate rows {deg}; all kernels of the call: "
                 + ", ".join(f"{name} {ms:.2f}" for name, ms in sorted(best.items())))
    ctx.prof_enable(False)
    # the restatement on the host
    for K in (20, 10):
        XV, nrm, d = cases[K][0][:n_host], cases[K][1][:n_host], cases[K][2]
        t0 = time.perf_counter()
        rows = np.array([oref.oadp_row(XV[i], nrm[i], d)[0] for i in range(len(XV))])
        t_loop = time.perf_counter() - t0
        t0 = time.perf_counter()
        stacked, _ = oref.oadp_proj(XV, nrm, d)
        t_stack = time.perf_counter() - t0
        dev = tpg.oadp_proj(np.asfortranarray(XV), nrm, d)
        bnd = np.array([oref.bound(XV[i], nrm[i], d) for i in range(len(XV))])
        lines.append(f"host, K = {K}, {len(XV)} individuals: numpy row by row {t_loop * 1e3:.0f} ms, on stacks {t_stack * 1e3:.0f} ms "
                     f"({os.cpu_count()} CPUs visible, LAPACK's own threading); device against it: largest ratio to the bound "
                     f"{(np.abs(dev - rows).max(axis=1) / bnd).max():.2e}")
    text = "\n".join(lines)
    print(text)
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "oadp_probe.txt"), "w") as f:
        f.write(text + "\n")
    return 0


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--step":
        return step(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    args = [int(a) for a in sys.argv[1:4]]
    sizes = args + [100000, 100000, 10000][len(args):]
    # the one step that uses the GPU runs as a child under its own time limit; nothing follows it
    try:
        r = subprocess.run([sys.executable, __file__, "--step"] + [str(s) for s in sizes], timeout=LIMIT_S)
    except subprocess.TimeoutExpired:
        print(f"no result within {LIMIT_S} s", flush=True)
        return 1
    if r.returncode != 0:
        print(f"exit status {r.returncode}", flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
