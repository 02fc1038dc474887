#!/usr/bin/env python3
"""The streamed PCA (k = 20) of the bench panel with impute="mode" on a raw store (2 % missing as byte 3) against the same run
on a pre-imputed store (the same panel with the missing entries as imputed bytes), five repeats each: the difference should
be the impute kernel's time per block, within the spread of the unimputed runs."""
import sys
import time
sys.path.insert(0, ".")
import numpy as np
import tidypopgen_amd as tpg
n, m, k = 5000, 1000000, 20
ctx = tpg.default_context()


def runs(st, **kw):
    out = []
    for rep in range(6):
        ctx.sync()
        t0 = time.perf_counter()
        r = st.run(k=k, total_var=False, **kw)
        out.append((time.perf_counter() - t0) * 1e3)
    return np.array(out[1:]), r  # the first run warms pools and pinned buffers


pre = tpg.Stream.synth(3, n, m, npop=51, imputed_bytes=True)
a, ra = runs(pre)
pre.close()
raw = tpg.Stream.synth(3, n, m, npop=51, imputed_bytes=False)
b, rb = runs(raw, impute="mode")
ctx.prof_enable(True); ctx.prof_reset()
raw.run(k=k, total_var=False, impute="mode"); ctx.sync()
d = ctx.prof_dump()
raw.close()
print("pre-imputed store  ms:", np.round(a, 2), "median %.2f spread %.2f" % (np.median(a), a.max() - a.min()), "blocks", ra["report"]["blocks"])
print("raw + impute=mode  ms:", np.round(b, 2), "median %.2f spread %.2f" % (np.median(b), b.max() - b.min()), "blocks", rb["report"]["blocks"])
print("difference of medians %.2f ms; impute_view kernels of one run: %d launches, %.3f ms; pack kernels: %s" % (
    np.median(b) - np.median(a), d["impute_view"][0], d["impute_view"][1], {k_: (v[0], round(v[1], 3)) for k_, v in d.items() if k_.startswith("pack")}))
