#!/usr/bin/env python3
"""autoSVD (include/tpg.h "autoSVD") on a synthetic panel without missing genotypes (FBM.synth), 20 chromosomes of equal
length, clumping in a window of 500 loci: wall clock of tpg_pca_auto_svd and the HIP-event time of every stage -- clumping,
the SVDs, the OGK distance, the rolling mean, the sort, the medcouple, the gather of the sub-view -- and the medcouple on its
own at 1e5 and 1e6 values.  The synthetic loci are independent, so the loop converges after one detection pass: the stages are
timed once each, at the size of the whole panel, which is what the question "do the new stages cost less than one SVD" needs.
One process; a call on a small panel warms up (code objects, the pool).

    python tools/autosvd_probe.py [n m]     default 5000 1000000; writes profiles/autosvd_probe.txt"""
import os
import sys
import time

sys.path.insert(0, ".")

NEW = {"gather": ("autosvd_gather",), "rollmean": ("autosvd_rollmean",), "sort": ("autosvd_keys", "autosvd_sort", "autosvd_stats"),
       "medcouple": ("autosvd_mc_step", "autosvd_mc_final"),
       "other new": ("autosvd_mac", "autosvd_start", "autosvd_sqrt", "autosvd_seg", "autosvd_fence", "autosvd_compact", "autosvd_check_idx")}


def stage_times(prof):
    """HIP-event milliseconds by stage: the new kernels by name, ld_* = clumping, pcadapt_* = OGK, everything else = the SVD"""
    out = {k: sum(prof[n][1] for n in names if n in prof) for k, names in NEW.items()}
    known = {n for names in NEW.values() for n in names}
    out["clump"] = sum(ms for n, (_, ms) in prof.items() if n.startswith("ld_"))
    out["OGK"] = sum(ms for n, (_, ms) in prof.items() if n.startswith("pcadapt_"))
    out["SVD"] = sum(ms for n, (_, ms) in prof.items() if n not in known and not n.startswith(("ld_", "pcadapt_")))
    return out


def main():
    import numpy as np

    import tidypopgen_amd as tpg
    from tidypopgen_amd import api

    args = [int(a) for a in sys.argv[1:3]]
    n, m = args + [5000, 1_000_000][len(args):]
    k, roll, window = 10, 50, 500
    ctx = tpg.default_context()
    lines = [f"panel {n} x {m}, synthetic, no missing genotypes, 20 chromosomes, k = {k}, roll_size = {roll}, window {window} loci"]

    def run(nn, mm):
        X = tpg.FBM.synth(9, nn, mm, npop=5, miss=0.0)
        v = tpg.View(X, code256=tpg.CODE_IMPUTE_PRED)
        chrom = (np.arange(mm) * 20 // mm).astype(np.int32)
        hi = api.ld_window_hi(chrom, None, window, use_positions=False)
        ctx.sync()
        t0 = time.perf_counter()
        r = api.pca_auto_svd(v, chrom, hi, k=k, thr_r2=0.2, roll_size=roll)
        ctx.sync()
        return r, (time.perf_counter() - t0) * 1e3, (v, chrom, hi)

    run(500, 20000)  # warm-up
    r, wall, (v, chrom, hi) = run(n, m)
    lines.append(f"wall {wall:.1f} ms; {r['n_iter']} SVD(s), converged {r['converged']}, kept {len(r['idx0'])} of {m}, "
                 f"outliers per pass {[h['n_outliers'] for h in r['history']]}")
    ctx.prof_enable(True)
    ctx.prof_reset()
    r = api.pca_auto_svd(v, chrom, hi, k=k, thr_r2=0.2, roll_size=roll)
    st = stage_times(ctx.prof_dump())
    ctx.prof_enable(False)
    for name in ("clump", "SVD", "OGK", "gather", "rollmean", "sort", "medcouple", "other new"):
        lines.append(f"  {name:10s} {st[name]:10.3f} ms")
    new = sum(st[name] for name in NEW)
    lines.append(f"  new stages together {new:.3f} ms against {st['SVD'] / max(r['n_iter'], 1):.3f} ms per SVD; "
                 f"V crosses PCIe twice per pass: {2 * 8 * len(r['idx0']) * k / 1e6:.1f} MB")
    rng = np.random.default_rng(1)
    for c in (100_000, 1_000_000):
        x = rng.exponential(size=c)
        api.medcouple(x)
        ctx.sync()
        t0 = time.perf_counter()
        mc = api.medcouple(x)
        wall = (time.perf_counter() - t0) * 1e3
        ctx.prof_enable(True)
        ctx.prof_reset()
        api.medcouple(x)
        st = stage_times(ctx.prof_dump())
        ctx.prof_enable(False)
        lines.append(f"medcouple alone, c = {c}: {mc:.6f}, wall {wall:.2f} ms (upload included); sort {st['sort']:.3f} ms, "
                     f"63 bisection steps {st['medcouple']:.3f} ms")
    text = "\n".join(lines)
    print(text)
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "autosvd_probe.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
