#!/usr/bin/env python3
"""sNMF (include/tpg.h "sNMF") on a synthetic panel (FBM.synth, 2 % missing): milliseconds per iteration and per kernel, beside
the arithmetic of DESIGN.md 3.13.  One process, one view; a short run warms up, then `iters` iterations with tol = 0 are timed by
the wall clock around a call that ends synchronised, and again with the kernels bracketed by HIP events (tpg_prof_get) for the
per-kernel split.  The per-iteration wall figure divides the whole call, start and store included, by iters.

    python tools/snmf_probe.py [n m K iters]     default 5000 1000000 8 10; writes profiles/snmf_probe.txt"""
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
    lines = [f"panel {n} x {m}, synthetic, 2 % missing, K = {K}, alpha = 10, {iters} iterations, tol = 0"]
    tpg.snmf(v, K, seed=1, max_iter=2, tol=0.0)  # warm-up: code objects, the T layout, the pool
    ctx.sync()
    t0 = time.perf_counter()
    r = tpg.snmf(v, K, seed=1, max_iter=iters, tol=0.0, return_trace=True)
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e3
    tr = r["trace"]
    lines.append(f"wall {wall:.1f} ms for the call = {wall / iters:.2f} ms per iteration; {r['n_iter']} iterations; "
                 f"ls {tr[0]:.6e} -> {r['ls']:.6e}; unsolved systems {r['n_unsolved']}")
    ctx.prof_enable(True)
    ctx.prof_reset()
    tpg.snmf(v, K, seed=1, max_iter=iters, tol=0.0)
    prof = ctx.prof_dump()
    ctx.prof_enable(False)
    per_iter = 0.0
    for name, (cnt, ms) in sorted(prof.items()):
        if name.startswith("snmf_"):
            lines.append(f"  {name:18s} {ms / cnt:10.3f} ms per launch x {cnt}")
            if name not in ("snmf_start", "snmf_store"):
                per_iter += ms / max(r["n_iter"], 1)
    adds = 1.0 * n * m * K
    byts = n * m / 4
    lines.append(f"each right-hand-side sweep: {adds / 1e9:.1f} G additions FP64 / {FP64_VECTOR_TFLOPS / 2} T add/s = "
                 f"{adds / (FP64_VECTOR_TFLOPS / 2) / 1e9:.2f} ms; {byts / 1e6:.0f} MB of packed panel / {HBM_TBS} TB/s = "
                 f"{byts / HBM_TBS / 1e9:.3f} ms")
    lines.append(f"systems per iteration: {3 * m} (G step) + {n} (Q step), one {K} x {K} matrix each step")
    for name in ("snmf_nnls_g", "snmf_nnls_q"):
        if name in prof:
            cnt, ms = prof[name]
            systems = 3 * m if name == "snmf_nnls_g" else n
            lines.append(f"  {name}: {1e6 * ms / cnt / systems:.2f} ns per system")
    lines.append(f"kernels of one iteration {per_iter:.2f} ms")
    text = "\n".join(lines)
    print(text)
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "snmf_probe.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
