#!/usr/bin/env python3
"""The pcadapt scan (include/tpg.h "pcadapt") on a synthetic panel without missing genotypes (FBM.synth): wall clock of
tpg_pcadapt and the HIP-event time of every kernel family it launches, for K = 2, 10 and 20, beside the traffic model of
DESIGN.md 3.11 (operand reads of the selection kernel).  U is an orthonormal basis of random columns: the cost does not depend
on what the columns mean.  One process, one view; a call at K = 2 warms up (code objects, the pool), then every K is timed by
the wall clock around a call that ends synchronised, and once more with the kernels bracketed by HIP events (tpg_prof_get).

    python tools/pcadapt_probe.py [n m]     default 5000 1000000; writes profiles/pcadapt_probe.txt"""
import os
import sys
import time

sys.path.insert(0, ".")

FAMILIES = ("pcadapt_select", "sweep_rowscale", "sweep_reduce", "pcadapt_rotate", "pcadapt_scale", "pcadapt_mask", "pcadapt_dist",
            "pcadapt_finalize", "pcadapt_mean", "pcadapt_log10p")


def main():
    import numpy as np

    import tidypopgen_amd as tpg
    from tidypopgen_amd import api

    args = [int(a) for a in sys.argv[1:3]]
    n, m = args + [5000, 1_000_000][len(args):]
    ctx = tpg.default_context()
    X = tpg.FBM.synth(9, n, m, npop=5, miss=0.0)
    v = tpg.View(X)
    rng = np.random.default_rng(1)
    lines = [f"panel {n} x {m}, synthetic, no missing genotypes"]
    api.pcadapt(v, np.linalg.qr(rng.standard_normal((n, 2)))[0])  # warm-up
    for K in (2, 10, 20):
        U = np.asfortranarray(np.linalg.qr(rng.standard_normal((n, K)))[0])
        ctx.sync()
        t0 = time.perf_counter()
        r = api.pcadapt(v, U)
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        ctx.prof_enable(True)
        ctx.prof_reset()
        api.pcadapt(v, U)
        prof = ctx.prof_dump()
        ctx.prof_enable(False)
        nsel = 2 * (2 * (K + K * (K - 1)) + K) + 1  # virtual columns selected: (K + K (K - 1)) medians and MADs twice, the final K, dist
        lines.append(f"K = {K}: wall {wall:.1f} ms, n_valid {r['n_valid']}, gc_lambda {r['gc_lambda']:.4f}, {nsel} selections")
        total = 0.0
        for name in FAMILIES:
            if name in prof:
                cnt, ms = prof[name]
                total += ms
                lines.append(f"  {name:18s} {ms:10.3f} ms in {cnt} launches")
        lines.append(f"  kernels together   {total:10.3f} ms")
        if "pcadapt_select" in prof:
            # two reads of each operand column per selection is the floor of the traffic model; pair columns read two
            npair = 4 * K * (K - 1)
            byts = 2.0 * 8 * m * ((nsel - npair) + 2 * npair)
            lines.append(f"  selection floor: 2 reads x {byts / 2 / 8 / m:.0f} operand columns = {byts / 1e9:.2f} GB "
                         f"-> {byts / prof['pcadapt_select'][1] / 1e9:.2f} TB/s of model traffic")
    text = "\n".join(lines)
    print(text)
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "pcadapt_probe.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
