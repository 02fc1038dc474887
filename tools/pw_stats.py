#!/usr/bin/env python3
"""Launch-to-launch statistics of the pairwise kernels (HIP events inside the library): mean, standard deviation, min and max
over 12 launches of the five-product kernel and of every product-set kernel at 5 000 x 1 000 000 -- what an A/B of two builds
in one GPU job compares (TPG_LIB_PATH picks the build; tools/pw_only.py prints the best of three instead).   tools/pw_stats.py"""
import sys
sys.path.insert(0, ".")
import numpy as np
import tidypopgen_amd as tpg

n, m, L = 5000, 1000000, 12
ctx = tpg.default_context()
ctx.prof_enable(True)
X = tpg.FBM.synth(3, n, m, npop=51, imputed_bytes=True)
v = tpg.View(X, code256=None)
pw = tpg.Pairwise(ctx, n)
sets = (("all", None, "pairwise_mfma"), ("as", tpg.PW_FOR_AS, "pairwise_mfma_as"), ("ibs", tpg.PW_FOR_IBS, "pairwise_mfma_ibs"),
        ("ibs1", tpg.PW_FOR_IBS_ALONE, "pairwise_mfma_ibs1"), ("king", tpg.PW_FOR_KING, "pairwise_mfma_king"))
for name, products, key in sets:
    t = []
    for rep in range(L + 2):
        ctx.prof_reset()
        pw.zero(); pw.accumulate(v, products=products); ctx.sync()
        t.append(ctx.prof_dump()[key][1])
    t = np.array(t[2:])
    print(f"{name:5s} mean {t.mean():.3f} std {t.std(ddof=1):.3f} min {t.min():.3f} max {t.max():.3f} ms over {L} launches", flush=True)
