#!/usr/bin/env python3
"""The streamed QC pass at the BASELINE panel (5 000 x 1 000 000 synthetic, 51 populations), from host bytes:
  (a) Stream.qc with every output (loci_counts, loci_hwe, grouped_genotype_counts, gt_grouped_hwe, indiv_counts);
  (b) the route the library offered before it for the same answers: FBM.from_numpy (the whole store uploaded) + one view +
      the five resident calls.
Wall times, a warm-up and then REPS runs each: median and range.  Separately the accumulate kernel of the per-individual
counts (loci.hip: indiv_accumulate) from tpg_prof_get, in a run that asks for that output alone, next to its HBM floor
(n / 4 bytes per locus read once from L) and next to what the resident tpg_indiv_counts spends (the T layout built from L,
then its count kernel).

    python tools/stream_qc_probe.py [n m G]"""
import ctypes as C
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import tidypopgen_amd as tpg

n, m, G = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (5000, 1000000, 51)
REPS = 3
ALL = dict(loci_counts=True, hwe=True, grouped_counts=True, grouped_hwe=True, indiv_counts=True)


def spread(xs):
    return f"median {statistics.median(xs):8.3f}  (min {min(xs):8.3f}, max {max(xs):8.3f})"


ctx = tpg.default_context()
fbm = tpg.FBM.synth(3, n, m, npop=G).to_numpy()  # (the device copy is gone when this line ends)
gid = (np.arange(n) % G).astype(np.int32)
print(f"panel {n} x {m} host bytes, {G} groups, mid-p; a warm-up, then {REPS} runs")

# (a) one streamed pass
st = tpg.Stream.from_numpy(fbm)
ts, s = [], None
for rep in range(REPS + 1):
    ctx.sync()
    t0 = time.perf_counter()
    s = st.qc(groupIds=gid, ngroups=G, **ALL)
    if rep:
        ts.append(time.perf_counter() - t0)
r = s["report"]
print(f"(a) Stream.qc, all outputs            wall s: {spread(ts)}   blocks {r['blocks']} of {r['block_loci']} loci, "
      f"up {r['bytes_up'] / 1e6:.0f} MB, down {r['bytes_down'] / 1e6:.0f} MB, peak HBM {r['peak_device_bytes'] / 1e6:.0f} MB")

# (b) upload the store, then the resident entry points
tb, parts, res = [], [], None
for rep in range(REPS + 1):
    ctx.sync()
    t0 = time.perf_counter()
    X = tpg.FBM.from_numpy(fbm)
    t1 = time.perf_counter()
    v = tpg.View(X)
    p1 = np.zeros(m)
    tpg._lib.check(tpg._lib.lib.tpg_loci_hwe(ctx.h, v.h, C.c_int(1), p1.ctypes.data))
    res = dict(loci_counts=tpg.loci_counts(v), loci_hwe=p1, grouped_genotype_counts=tpg.grouped_genotype_counts(v, gid, G),
               gt_grouped_hwe=tpg.gt_grouped_hwe(v, gid, G), indiv_counts=tpg.indiv_counts(v))
    t2 = time.perf_counter()
    if rep:
        tb.append(t2 - t0)
        parts.append((t1 - t0, t2 - t1))
    v.free()
    X.free()
print(f"(b) FBM.from_numpy + 5 resident calls wall s: {spread(tb)}   of which upload {statistics.median([p[0] for p in parts]):.3f}, "
      f"view + calls {statistics.median([p[1] for p in parts]):.3f}")
same = all(np.array_equal(s[k], res[k]) for k in res)
print(f"(a) equals (b) bit for bit: {same}")

# the accumulate kernel alone, against its floor
ctx.prof_enable(True)
ctx.prof_only(["indiv_accumulate", "indiv_finish"])
ka, launches = [], 0
for rep in range(REPS + 1):
    ctx.sync(); ctx.prof_reset()
    st.qc(indiv_counts=True)
    ms, launches = ctx.prof_get("indiv_accumulate")
    if rep:
        ka.append(ms)
gb = n / 4 * m / 1e9
print(f"indiv_accumulate, {launches} launches (one per block): ms {spread(ka)}   reads {gb:.2f} GB of L -> "
      f"{gb / (statistics.median(ka) / 1e3):.0f} GB/s")
ctx.prof_only(None)
X = tpg.FBM.from_numpy(fbm)
kt = []
for rep in range(REPS + 1):
    v = tpg.View.pair(X, code256_a=tpg.CODE_012, code256_b=tpg.CODE_IMPUTE_PRED)[0]  # a view that carries L only: T is made on demand
    ctx.sync(); ctx.prof_reset()
    tpg.indiv_counts(v)
    prof = ctx.prof_dump()
    if rep:
        kt.append(sum(t for name, (_, t) in prof.items()))
    if rep == REPS:
        print("resident tpg_indiv_counts on a view without T, kernels:", {k: round(t, 3) for k, (_, t) in prof.items()})
    v.free()
print(f"resident tpg_indiv_counts (T from L + count kernel): ms {spread(kt)}")
st.close()
