#!/usr/bin/env python3
"""Hardy-Weinberg exact tests at the BASELINE panel (5 000 x 1 000 000 synthetic, 51 populations): what the device path costs,
kernel by kernel and end to end, next to what the library offered before it -- the genotype table downloaded
(tpg_grouped_genotype_counts) and a host loop over it (the same recurrence, csrc/host/host_hwe.h, compiled here with gcc
-O2 -fopenmp; one thread and 16).  Medians of three runs after a warm-up; every run packs a fresh view, so the grouped
counts are swept each time (a view caches them).  Also printed: how evenly the trip counts of the test kernel fill a wave
(the bound min(hom1, hom2) + het / 2 per lane against the largest of its wave, in the kernel's own mapping).

    python tools/hwe_probe.py [n m G]"""
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, ".")
import numpy as np

import tidypopgen_amd as tpg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
n, m, G = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (5000, 1000000, 51)
REPS = 3

HOST_SRC = r"""
#include <stdint.h>
#include "host_hwe.h"
/* tab = three m x G int32 matrices (k = 0, 1, 2 alternate alleles), p = m x G */
void hwe_host_loop(const int32_t* tab, int64_t total, int midp, int threads, double* p) {
#pragma omp parallel for schedule(static, 4096) num_threads(threads)
  for (int64_t i = 0; i < total; i++) p[i] = tpg_hwe_exact(tab[i], tab[total + i], tab[2 * total + i], midp);
}
"""


def host_lib(d):
    src, so = os.path.join(d, "hwe_host.c"), os.path.join(d, "libhwe_host.so")
    with open(src, "w") as f:
        f.write(HOST_SRC)
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-fopenmp", "-shared", "-fPIC",
                           "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc", "host"), src, "-o", so])
    lib = C.CDLL(so)
    lib.hwe_host_loop.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]
    lib.hwe_host_loop.restype = None
    return lib


def med(xs):
    return statistics.median(xs)


ctx = tpg.default_context()
ctx.prof_enable(True)
X = tpg.FBM.synth(3, n, m, npop=G)
gid = (np.arange(n) % G).astype(np.int32)
print(f"panel {n} x {m}, {G} groups, mid-p; medians of {REPS} after a warm-up")

# (a) the device path
rows = {"grouped": [], "loci": []}
p_dev = None
for rep in range(REPS + 1):
    v = tpg.View(X)
    ctx.sync(); ctx.prof_reset()
    t0 = time.perf_counter()
    p_dev = tpg.gt_grouped_hwe(v, gid, G)
    wall = time.perf_counter() - t0
    prof = ctx.prof_dump()
    if rep:
        rows["grouped"].append((wall, prof["onehot"][1] + prof["grouped_counts"][1], prof["hwe_grouped"][1]))
    v.free()
    ctx.sync(); ctx.prof_reset()
    t0 = time.perf_counter()
    q = tpg.loci_hwe(X)  # packs its own view: timed apart below through the kernels
    wall = time.perf_counter() - t0
    prof = ctx.prof_dump()
    if rep:
        rows["loci"].append((wall, prof["loci_counts"][1], prof["hwe_loci"][1], prof["pack"][1]))
g = rows["grouped"]
print(f"(a) tpg_gt_grouped_hwe   wall {med([r[0] for r in g]):8.3f} s   count sweep (onehot + grouped_counts) {med([r[1] for r in g]):8.3f} ms   "
      f"test kernel hwe_grouped {med([r[2] for r in g]):8.3f} ms   ({m * G / 1e6:.1f} M tests, {m * G * 8 / 1e6:.0f} MB of p-values downloaded)")
g = rows["loci"]
print(f"(a) loci_hwe (pack + tpg_loci_hwe) wall {med([r[0] for r in g]):8.3f} s   pack {med([r[3] for r in g]):8.3f} ms   loci_counts {med([r[1] for r in g]):8.3f} ms   "
      f"test kernel hwe_loci {med([r[2] for r in g]):8.3f} ms")

# (b) before: the table downloaded, the loop on the host
with tempfile.TemporaryDirectory() as d:
    hl = host_lib(d)
    dl, tab = [], None
    for rep in range(REPS + 1):
        v = tpg.View(X)
        ctx.sync()
        t0 = time.perf_counter()
        tab3 = np.zeros((3, G, m), dtype=np.int32)
        tpg._lib.check(tpg._lib.lib.tpg_grouped_genotype_counts(ctx.h, v.h, C.c_void_p(gid.ctypes.data), C.c_int(G), C.c_void_p(tab3.ctypes.data)))
        if rep:
            dl.append(time.perf_counter() - t0)
        v.free()
    p_host = np.zeros(m * G)
    loops = {}
    for threads in (16, 1):
        ts = []
        for rep in range(REPS + 1):
            t0 = time.perf_counter()
            hl.hwe_host_loop(tab3.ctypes.data, m * G, 1, threads, p_host.ctypes.data)
            if rep:
                ts.append(time.perf_counter() - t0)
        loops[threads] = med(ts)
    print(f"(b) tpg_grouped_genotype_counts + download of {tab3.nbytes / 1e6:.0f} MB: wall {med(dl):8.3f} s;   host loop 16 threads {loops[16]:8.3f} s,"
          f" 1 thread {loops[1]:8.3f} s   -> end to end {med(dl) + loops[16]:8.3f} s (16 threads), {med(dl) + loops[1]:8.3f} s (1 thread)")
    dev = p_dev.ravel(order="F")
    rel = np.abs(dev - p_host) / np.maximum(p_host, 1e-300)
    print(f"device against host loop: largest relative difference {rel.max():.3e} over {dev.size} tests")

# lane utilisation of the test kernel: a wave = 64 consecutive loci of one group
bound = np.minimum(tab3[0], tab3[2]).astype(np.int64) + tab3[1] // 2  # (G, m)
mw = (m // 64) * 64
waves = bound[:, :mw].reshape(G, mw // 64, 64)
print(f"trip-count bound per lane: mean {bound.mean():.2f}, mean of the wave maxima {waves.max(axis=2).mean():.2f} "
      f"-> lanes busy {waves.sum() / (64.0 * waves.max(axis=2).sum()):.3f} of the time a wave spends in the walks")
