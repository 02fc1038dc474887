#!/usr/bin/env python3
"""Admixture cross-validation (include/tpg.h "admixture cross-validation") on a synthetic panel (FBM.synth, 2 % missing): HIP-event
time per launch of the hold-out view kernel and of the hold-out sweep, beside one EM iteration (admix_f_sweep + admix_q_sweep +
admix_q_combine + admix_ll_sum) of the same run, and the ratio "mask + hold-out sums per fold : one EM iteration" that DESIGN.md
3.10 quotes.  One process, one view; a short run warms up (code objects, the pool), then tpg_admix_cv runs `iters` iterations per
fold with tol = 0 under the profiler (tpg_prof_get), and once more without it for the wall clock.

    python tools/admix_cv_probe.py [n m K folds iters]     default 5000 1000000 8 5 2; writes profiles/admix_cv_probe.txt"""
import os
import sys
import time

sys.path.insert(0, ".")

HBM_TBS = 6.29  # measured float4 copy


def main():
    import tidypopgen_amd as tpg

    args = [int(a) for a in sys.argv[1:6]]
    n, m, K, folds, iters = args + [5000, 1_000_000, 8, 5, 2][len(args):]
    ctx = tpg.default_context()
    X = tpg.FBM.synth(9, n, m, npop=max(K, 2), miss=0.02)
    v = tpg.View(X)
    lines = [f"panel {n} x {m}, synthetic, 2 % missing, K = {K}, {folds} folds, {iters} iterations per fold, tol = 0"]
    tpg.admix_cv(v, K, folds=2, cv_seed=1, seed=1, max_iter=1, tol=0.0)  # warm-up
    ctx.sync()
    ctx.prof_enable(True)
    ctx.prof_reset()
    r = tpg.admix_cv(v, K, folds=folds, cv_seed=1, seed=1, max_iter=iters, tol=0.0)
    prof = ctx.prof_dump()
    ctx.prof_enable(False)
    t0 = time.perf_counter()
    tpg.admix_cv(v, K, folds=folds, cv_seed=1, seed=1, max_iter=iters, tol=0.0)
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e3
    lines.append(f"cv error {r['cv_error']:.6f}; held-out entries per fold {r['fold_count'].tolist()}")
    lines.append(f"wall {wall:.1f} ms for the call = {wall / folds:.1f} ms per fold")
    per = {}
    for name, (cnt, ms) in sorted(prof.items()):
        if name.startswith("admix_") or name == "l2t":
            per[name] = ms / cnt
            lines.append(f"  {name:20s} {ms / cnt:10.3f} ms per launch x {cnt}")
    byts = 2.0 * n * m / 4
    lines.append(f"the mask and the hold-out sweep each move {byts / 1e6:.0f} MB of packed panel: {byts / HBM_TBS / 1e9:.3f} ms at {HBM_TBS} TB/s")
    it = sum(per.get(k, 0.0) for k in ("admix_f_sweep", "admix_q_sweep", "admix_q_combine", "admix_ll_sum"))
    cv = per.get("admix_holdout_view", 0.0) + per.get("admix_holdout_sweep", 0.0)
    if it > 0:
        lines.append(f"one EM iteration {it:.3f} ms; mask + hold-out sums per fold {cv:.3f} ms = {cv / it:.3f} of an iteration")
        if "admix_loglik" in per:
            lines.append(f"hold-out sweep : likelihood-only pass = {per.get('admix_holdout_sweep', 0.0) / per['admix_loglik']:.3f}")
    text = "\n".join(lines)
    print(text)
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "admix_cv_probe.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
