#!/usr/bin/env python3
"""Accelerated admixture (include/tpg.h "admixture, accelerated") on a synthetic panel (FBM.synth, 2 % missing): HIP-event time
per launch of the two kernels the extrapolation adds (admix_sq_norms with its one-workgroup combine, admix_sq_extrap) beside one EM
step (admix_f_sweep + admix_q_sweep + admix_q_combine + admix_ll_sum) of the same run; then the plain EM against the accelerated
one from the same seeded start, tol = 1e-4, both capped at `cap` EM steps: EM steps, wall clock, final loglik, and the EM step at
which the accelerated run first reaches the plain run's final likelihood.  One process, one view; a short run warms up (code
objects, the pool).

    python tools/admix_squarem_probe.py [n m K cap]     default 5000 1000000 8 150; writes profiles/admix_squarem_probe.txt"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")

HBM_TBS = 6.29  # measured float4 copy


def main():
    import tidypopgen_amd as tpg

    args = [int(a) for a in sys.argv[1:5]]
    n, m, K, cap = args + [5000, 1_000_000, 8, 150][len(args):]
    KT = K if K <= 4 else 8 if K <= 8 else 16 if K <= 16 else 32
    ctx = tpg.default_context()
    X = tpg.FBM.synth(9, n, m, npop=max(K, 2), miss=0.02)
    v = tpg.View(X)
    lines = [f"panel {n} x {m}, synthetic, 2 % missing, K = {K} (dispatch width {KT}), seeded start 1, tol = 1e-4, cap {cap} EM steps"]
    tpg.admix_em(v, K, seed=1, max_iter=4, tol=0.0, accel="squarem")  # warm-up
    tpg.admix_em(v, K, seed=1, max_iter=2, tol=0.0)
    ctx.sync()
    # the kernels, under the profiler: two whole cycles
    ctx.prof_enable(True)
    ctx.prof_reset()
    tpg.admix_em(v, K, seed=1, max_iter=6, tol=0.0, accel="squarem")
    prof = ctx.prof_dump()
    ctx.prof_enable(False)
    per = {}
    for name, (cnt, ms) in sorted(prof.items()):
        if name.startswith("admix_"):
            per[name] = ms / cnt
            lines.append(f"  {name:20s} {ms / cnt:10.3f} ms per launch x {cnt}")
    it = sum(per.get(k, 0.0) for k in ("admix_f_sweep", "admix_q_sweep", "admix_q_combine", "admix_ll_sum"))
    # norms: Q and F launched apiece (two launches per cycle) + the combine; extrap: likewise two launches per cycle
    extra = 2 * per.get("admix_sq_norms", 0.0) + per.get("admix_sq_combine", 0.0) + 2 * per.get("admix_sq_extrap", 0.0)
    state = (n + m) * KT * 8.0
    lines.append(f"arithmetic: a padded state is {state / 1e6:.0f} MB; the norms read three ({3 * state / HBM_TBS / 1e9:.3f} ms at "
                 f"{HBM_TBS} TB/s), the extrapolation reads three and writes one ({4 * state / HBM_TBS / 1e9:.3f} ms)")
    if it > 0:
        lines.append(f"measured: one EM step {it:.3f} ms; the extrapolation of one cycle (norms of Q and F, combine, theta' of Q and F) "
                     f"{extra:.3f} ms = {extra / (3 * it):.4f} of the cycle's three EM steps")
    # plain against accelerated, the same job, the same start
    runs = {}
    for name, accel in (("plain", None), ("accelerated", "squarem")):
        ctx.sync()
        t0 = time.perf_counter()
        r = tpg.admix_em(v, K, seed=1, max_iter=cap, tol=1e-4, accel=accel, return_trace=True)
        ctx.sync()
        runs[name] = (r, time.perf_counter() - t0)
        extra_txt = f", {r['n_cycles']} cycles, {r['n_rejected']} rejected, smallest alpha {r['alpha'].min():.2f}" if accel else ""
        lines.append(f"{name:12s} EM steps {r['n_iter']:5d}, converged {r['converged']}, wall {runs[name][1]:8.2f} s "
                     f"({runs[name][1] / max(r['n_iter'], 1) * 1e3:.2f} ms per EM step), loglik {r['loglik']:.4f}{extra_txt}")
    p, a = runs["plain"][0], runs["accelerated"][0]
    lines.append(f"loglik accelerated - plain = {a['loglik'] - p['loglik']:.4f}")
    tr = a["trace"][:-1]
    starts = np.arange(0, len(tr), 3)  # the likelihoods at the starts of the cycles
    hit = [int(t) for t in starts if tr[t] >= p["loglik"]]
    if hit:
        lines.append(f"the accelerated run starts a cycle at or above the plain run's final loglik after {hit[0]} EM steps "
                     f"(plain: {p['n_iter']}): {hit[0] / max(p['n_iter'], 1):.2f} of the plain run's steps")
    else:
        lines.append("the accelerated run starts no cycle at or above the plain run's final loglik within the cap")
    text = "\n".join(lines)
    print(text)
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "admix_squarem_probe.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
