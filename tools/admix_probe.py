#!/usr/bin/env python3
"""Admixture EM (include/tpg.h "admixture") on a synthetic panel (FBM.synth, 2 % missing): milliseconds per iteration and per
sweep, beside the roofline of DESIGN.md 3.10.  One process, one view; a short run warms up, then `iters` iterations with
tol = 0 (no early stop) are timed by the wall clock around a call that ends synchronised, and again with the kernels bracketed
by HIP events (tpg_prof_get) for the per-sweep split.  The per-iteration wall figure divides the whole call, start and final
likelihood pass included, by iters.

    python tools/admix_probe.py [n m K iters]     default 5000 1000000 8 10; writes profiles/admix_probe.txt"""
import os
import sys
import time

sys.path.insert(0, ".")

FP64_VECTOR_TFLOPS = 78.6  # MI355X datasheet: half the FP32 vector rate of 157.3
HBM_TBS = 6.29             # measured float4 copy


def main():
    import tidypopgen_amd as tpg

    args = [int(a) for a in sys.argv[1:5]]
    n, m, K, iters = args + [5000, 1_000_000, 8, 10][len(args):]
    ctx = tpg.default_context()
    X = tpg.FBM.synth(9, n, m, npop=max(K, 2), miss=0.02)
    v = tpg.View(X)
    lines = [f"panel {n} x {m}, synthetic, 2 % missing, K = {K}, {iters} iterations, tol = 0"]
    tpg.admix_em(v, K, seed=1, max_iter=2, tol=0.0)  # warm-up: code objects, the T layout, the pool
    ctx.sync()
    t0 = time.perf_counter()
    r = tpg.admix_em(v, K, seed=1, max_iter=iters, tol=0.0, return_trace=True)
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e3
    assert r["n_iter"] == iters
    lines.append(f"wall {wall:.1f} ms for the call = {wall / iters:.2f} ms per iteration; loglik {r['trace'][0]:.6e} -> {r['loglik']:.6e}")
    ctx.prof_enable(True)
    ctx.prof_reset()
    tpg.admix_em(v, K, seed=1, max_iter=iters, tol=0.0)
    prof = ctx.prof_dump()
    ctx.prof_enable(False)
    for name, (cnt, ms) in sorted(prof.items()):
        if name.startswith("admix_"):
            lines.append(f"  {name:18s} {ms / cnt:10.3f} ms per launch x {cnt}")
    flop = 2.0 * n * m * (6 * K + 10)
    byts = 2.0 * n * m / 4
    lines.append(f"roofline per iteration: {flop / 1e9:.1f} GFLOP FP64 / {FP64_VECTOR_TFLOPS} TFLOP/s = {flop / FP64_VECTOR_TFLOPS / 1e9:.2f} ms; "
                 f"{byts / 1e6:.0f} MB of packed panel / {HBM_TBS} TB/s = {byts / HBM_TBS / 1e9:.3f} ms")
    sweeps = sum(ms / cnt for name, (cnt, ms) in prof.items() if name in ("admix_f_sweep", "admix_q_sweep", "admix_q_combine", "admix_ll_sum"))
    if sweeps > 0:
        lines.append(f"kernels of one iteration {sweeps:.2f} ms = {flop / sweeps / 1e9:.2f} TFLOP/s of the model's count, "
                     f"{100 * flop / FP64_VECTOR_TFLOPS / 1e9 / sweeps:.1f} % of the FP64 vector rate")
    text = "\n".join(lines)
    print(text)
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "admix_probe.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
