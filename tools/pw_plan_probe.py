#!/usr/bin/env python3
"""The five-product pairwise kernel under forced dealing plans (TPG_PW_PLAN, A/B only): one line per plan with the best and the
mean of `reps` launches after one warm-up (HIP events inside the library).
  tools/pw_plan_probe.py [n m reps] [plan ...]     plan = "S[,c[,nblk]]", "-" = the library's own choice;
                                                   default plans: S = 1 2 3 4 5 7 10 14 with the tail cut, then "10,1" and "-"
  tools/pw_plan_probe.py --table <dir>             after rocprofv3 --pmc passes of the line above into <dir>/<pass>/ (their
                                                   stdout in <dir>/<pass>.log): ms, FETCH_SIZE, clock and MFMA busy per plan
With TPG_LIB_PATH another build of the library runs (a parent build ignores the plan: every line is then its own S)."""
import collections
import csv
import glob
import os
import re
import sys

PLANS = ["1", "2", "3", "4", "5", "7", "10", "14", "10,1", "-"]


def table(src):
    ms = collections.defaultdict(dict)
    for log in sorted(glob.glob(os.path.join(src, "*.log"))):
        for ln in open(log):
            g = re.match(r"plan (\S+)\s.*mean (\S+) ms", ln)
            if g:
                ms[os.path.basename(log)[:-4]][g.group(1)] = float(g.group(2))
    rows = collections.defaultdict(dict)
    for f in glob.glob(os.path.join(src, "*", "*", "*_counter_collection.csv")):
        tag = os.path.relpath(f, src).split(os.sep)[0]
        per = collections.defaultdict(lambda: collections.defaultdict(float))
        for r in csv.DictReader(open(f)):
            if "tpg_pairwise_kernel" in r["Kernel_Name"]:
                per[int(r["Dispatch_Id"])][r["Counter_Name"]] += float(r["Counter_Value"])
        ids = sorted(per)
        plans = list(ms[tag])
        if not plans or len(ids) % len(plans):
            print(f"# {tag}: {len(ids)} dispatches do not divide over {len(plans)} plans", file=sys.stderr)
            continue
        k = len(ids) // len(plans)
        for i, p in enumerate(plans):
            mine = ids[i * k + 1:(i + 1) * k]  # without the warm-up launch
            for name in per[mine[0]]:
                rows[p][name] = sum(per[d][name] for d in mine) / len(mine)
                rows[p]["ms:" + name] = ms[tag][p]  # the time of the pass this counter came from
    print("plan     ms (pmc passes)   L2-miss GB/launch (2 x 1024 x FETCH_SIZE)   clock GHz   MFMA pipe busy")
    for p, c in rows.items():
        cyc = c.get("GRBM_GUI_ACTIVE", 0.0) / 8
        t = c.get("ms:GRBM_GUI_ACTIVE", 0.0)
        print(f"{p:8s} {t:8.3f}          {c.get('FETCH_SIZE', 0.0) * 2048 / 1e9:8.2f}"
              f"                                  {cyc / (t * 1e6) if t else 0:6.3f}      "
              f"{c.get('SQ_VALU_MFMA_BUSY_CYCLES', 0.0) / 1024 / cyc if cyc else 0:6.3f}")


def main():
    sys.path.insert(0, ".")
    import numpy as np
    import tidypopgen_amd as tpg

    a = sys.argv[1:]
    n, m, reps = (int(a[0]), int(a[1]), int(a[2])) if len(a) >= 3 else (5000, 1000000, 3)
    plans = a[3:] or PLANS
    ctx = tpg.default_context()
    ctx.prof_enable(True)
    X = tpg.FBM.synth(3, n, m, npop=51, imputed_bytes=True)
    v = tpg.View(X, code256=None)
    pw = tpg.Pairwise(ctx, n)
    for p in plans:
        if p == "-":
            os.environ.pop("TPG_PW_PLAN", None)
        else:
            os.environ["TPG_PW_PLAN"] = p
        t = []
        for rep in range(reps + 1):
            ctx.prof_reset()
            pw.zero(); pw.accumulate(v); ctx.sync()
            t.append(ctx.prof_dump()["pairwise_mfma"][1])
        t = np.array(t[1:])
        print(f"plan {p:6s} best {t.min():.3f} mean {t.mean():.3f} ms   std {t.std(ddof=1) if reps > 1 else 0:.3f}   "
              f"{5.0 * n * n * m / t.min() / 1e13:.3f} of the FP4 peak", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--table":
        table(sys.argv[2])
    else:
        main()
