#!/usr/bin/env python3
"""Time the imputation kernels alone on the bench panel (5 000 x 1 000 000 bytes, 2 % missing), next to the pack kernel that
streams the same bytes: the store kernel in its three launch shapes (TPG_IMPUTE_WPL: waves per locus), and the view kernel
against the pack of the view it reads."""
import os
import sys
sys.path.insert(0, ".")
import numpy as np
import tidypopgen_amd as tpg
from oracle import oracle as orc
n, m = 5000, 1000000
ctx = tpg.default_context(); ctx.prof_enable(True)
# 16-byte pieces that hold a missing byte (what the store kernel writes back), from a slice of the same panel on the host
host = orc.synth_fbm(3, n, 2048, npop=51, imputed_bytes=False)
flat = host.ravel(order="F")
frac = float((flat[: flat.size // 16 * 16].reshape(-1, 16) == 3).any(axis=1).mean())
moved = n * m * (1.0 + frac)
print(f"pieces with a missing byte: {frac:.4f}  bytes moved per call: {moved/1e9:.3f} GB")
for method in ("mode", "random"):
    for wpl in ("1", "4", "16"):
        os.environ["TPG_IMPUTE_WPL"] = wpl
        best = []
        for rep in range(3):
            X = tpg.FBM.synth(3, n, m, npop=51, imputed_bytes=False)
            ctx.sync(); ctx.prof_reset()
            r = X.impute_simple(method, 1); ctx.sync()
            best.append(ctx.prof_dump()["impute_store"][1])
            X.free()
        ms = min(best)
        print(f"impute_store {method:6s} wpl={wpl:2s} {ms:.3f} ms (runs {['%.3f' % b for b in best]}) = {moved/ms/1e9:.2f} TB/s  imputed {r['imputed']}")
os.environ.pop("TPG_IMPUTE_WPL")
X = tpg.FBM.synth(3, n, m, npop=51, imputed_bytes=False)
c012 = np.ascontiguousarray(tpg.CODE_012)
for rep in range(3):
    ctx.prof_reset()
    v = tpg.View(X, None, None, code256=c012); ctx.sync()
    pack_ms = ctx.prof_dump()["pack"][1]
    for method in ("mode", "random"):
        ctx.prof_reset()
        w = v.impute(method, 1); ctx.sync()
        ms = ctx.prof_dump()["impute_view"][1]
        w.free()
        if rep == 2:
            print(f"impute_view {method:6s} {ms:.3f} ms = {2 * n * m / 4 / ms / 1e9:.2f} TB/s (L read + L written; the second read is L2's)")
    v.free()
print(f"pack  {pack_ms:.3f} ms = {7.5e9/pack_ms/1e9:.2f} TB/s (store read + L and T written)")
