#!/usr/bin/env python3
"""IBD segments (tpg_ibd_segments) on a synthetic panel with planted relatives, 2 % missing, 22 chromosomes, at the default
parameters, for kind 1 and kind 2: HIP-event times PER LAUNCH of the kernels (count walk, pair scan, emit walk, mirror) with
their launches per call, and the wall clock, of the C call with room for every segment, of the Python wrapper at its default
cap and of the wrapper with arrays that are too short, which repeats the call (medians of REPS after a warm-up, one job);
pair-words per second of the count walk, the share of the device time that goes into emission, snp_king on the same panel
in the same job as the yardstick, and the vectorised numpy restatement (tests/ibdseg_ref.py) timed on a sample of pairs and
EXTRAPOLATED to all pairs.

The relatives: the last 4 * FAMILIES rows are replaced by families made from rows of the panel -- two parents as they are and
two full sibs, each one recombinant gamete per parent (the parents' heterozygous loci phased at random, two crossovers per
chromosome) -- so parent - offspring pairs share IBD1 everywhere and the sibs have IBD0 / 1 / 2 stretches.

    python tools/ibdseg_probe.py [n m]"""
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import ctypes as C

import tidypopgen_amd as tpg
from tidypopgen_amd._lib import check, lib
from tidypopgen_amd.api import _ptr
from tests import ibdseg_ref as ir

REPS = 2
FAMILIES = 10
NCHROM = 22
SAMPLE_PAIRS = 24
ctx = tpg.default_context()
ctx.prof_enable(True)


def plant_families(G, chrom, rng):
    n, m = G.shape
    truth = []
    for f in range(FAMILIES):
        pa, pb, c0, c1 = (n - 4 * FAMILIES + 4 * f + k for k in range(4))
        haps = []
        for p in (pa, pb):
            g = np.ascontiguousarray(G[p])
            g = np.where(g == 3, 0, g)
            first = np.where(g == 1, rng.integers(0, 2, m), g // 2).astype(np.uint8)
            haps.append(np.stack([first, (g - first).astype(np.uint8)]))
        for c in (c0, c1):
            child = np.zeros(m, dtype=np.uint8)
            for h in haps:
                which = np.empty(m, dtype=np.int64)
                for ch in range(NCHROM):
                    idx = np.flatnonzero(chrom == ch)
                    cuts = np.sort(rng.choice(np.arange(1, len(idx)), 2, replace=False))
                    which[idx] = (int(rng.integers(0, 2)) + np.searchsorted(cuts, np.arange(len(idx)), side="right")) % 2
                child += h[which, np.arange(m)]
            child[rng.random(m) < 0.02] = 3
            G[c] = child
        truth.append((pa, pb, c0, c1))
    return truth


def med_prof(fn, names):
    """fn once as a warm-up, then REPS times -> (median ms PER LAUNCH of every name, launches per run of every name, walls, result)"""
    rows, launches, walls, out = [], [], [], None
    for rep in range(REPS + 1):
        ctx.sync(); ctx.prof_reset()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        wall = time.perf_counter() - t0
        prof = ctx.prof_dump()
        if rep:
            cnt = [prof.get(k, (0, 0.0))[0] for k in names]
            rows.append([prof.get(k, (0, 0.0))[1] / max(c, 1) for k, c in zip(names, cnt)])
            launches = cnt
            walls.append(wall)
    return [statistics.median(c) for c in zip(*rows)], launches, walls, out


def c_call(v, chrom, pos, kind, cap, seg, n_seg, total):
    """tpg_ibd_segments itself at the default parameters -> count"""
    count = C.c_int64()
    check(lib.tpg_ibd_segments(v.ctx.h, v.h, _ptr(chrom), _ptr(pos), kind, 200, 0, 10**6, 50, -1, cap,
                               *(_ptr(a) if cap else None for a in seg), C.byref(count), _ptr(n_seg), _ptr(total)))
    return int(count.value)


def probe(n, m):
    rng = np.random.default_rng(9)
    t0 = time.perf_counter()
    X0 = tpg.FBM.synth(9, n, m, npop=8, miss=0.02)
    G = X0.to_numpy()
    X0.free()
    pos = 1000 + np.cumsum(rng.integers(1, 3000, m)).astype(np.int64)
    chrom = (np.arange(m) * NCHROM // m).astype(np.int32)
    truth = plant_families(G, chrom, rng)
    X = tpg.FBM.from_numpy(G, code256=tpg.CODE_012)
    v = tpg.View(X)
    npairs, nwords = n * (n - 1) // 2, -(-m // 32)
    print(f"panel {n} x {m}, synthetic (8 populations), 2 % missing, {NCHROM} chromosomes, {FAMILIES} planted families of two parents and "
          f"two full sibs; built in {time.perf_counter() - t0:.1f} s")
    print(f"  {npairs} pairs x {nwords} words = {npairs * nwords:.3e} pair-words; default parameters (min_snp 200, bridge_min_snp 50, "
          f"max_gap 1e6); medians of {REPS} runs after a warm-up")
    _, _, kw, _ = med_prof(lambda: tpg.snp_king(X), ())
    prof = ctx.prof_dump()
    print(f"  snp_king wall {statistics.median(kw) * 1e3:10.1f} ms   (the yardstick; its launches: "
          f"{', '.join(f'{k} {t:.1f} ms' for k, (_, t) in sorted(prof.items()))})")
    chrom_c, pos_c = np.ascontiguousarray(chrom, dtype=np.int32), np.ascontiguousarray(pos, dtype=np.int64)
    n_seg, total = np.zeros((n, n), dtype=np.int32), np.zeros((n, n), dtype=np.int64)
    for kind in (1, 2):
        names = (f"ibd_count_{kind}", "ibd_pair_scan", f"ibd_emit_{kind}", "ibd_mirror")
        count = c_call(v, chrom_c, pos_c, kind, 0, [None] * 6, n_seg, total)  # the counting call
        seg = [np.empty(count, dtype=np.int32 if k in (0, 1, 4, 5) else np.int64) for k in range(6)]
        med, launches, walls, _ = med_prof(lambda: c_call(v, chrom_c, pos_c, kind, count, seg, n_seg, total), names)
        dev = sum(t * c for t, c in zip(med, launches))
        print(f"  kind {kind}: {count} segments in {int((n_seg > 0).sum()) // 2} pairs, {int((seg[5] > 0).sum())} bridged")
        print(f"    tpg_ibd_segments with room for all (cap = count), per launch:")
        for k, t, c in zip(names, med, launches):
            print(f"      {k:14s} {t:10.3f} ms   x {c} launch(es) per call")
        print(f"      count walk: {npairs * nwords / (med[0] * 1e-3):.3e} pair-words / s; emission (emit walk) {100 * med[2] * launches[2] / dev:.1f} % of "
              f"the device time {dev:.1f} ms")
        print(f"      wall of the C call {statistics.median(walls) * 1e3:10.1f} ms   (all runs: {', '.join(f'{w * 1e3:.1f}' for w in walls)}); "
              f"{statistics.median(walls) / statistics.median(kw):.2f} x snp_king")
        _, wl, ww, s = med_prof(lambda: tpg.ibd_segments(v, chrom, pos, kind=kind), names)
        print(f"    ibd_segments (the wrapper, default cap): wall {statistics.median(ww) * 1e3:10.1f} ms   (all runs: "
              f"{', '.join(f'{w * 1e3:.1f}' for w in ww)}); launches per call: {', '.join(f'{k} {c}' for k, c in zip(names, wl))}")
        _, wl, ww, _ = med_prof(lambda: tpg.ibd_segments(v, chrom, pos, kind=kind, cap=1), names)
        print(f"    ibd_segments with arrays too short (cap = 1: the call is repeated): wall {statistics.median(ww) * 1e3:10.1f} ms; launches "
              f"per call: {', '.join(f'{k} {c}' for k, c in zip(names, wl))}")
        for pa, pb, c0, c1 in truth[:2]:
            L = s["sum_length"]
            print(f"    family rows {pa}..{c1}: sum_length parent-child {int(L[pa, c0])}, {int(L[pb, c1])}; sibs {int(L[c0, c1])}; "
                  f"parents {int(L[pa, pb])}")
        # the numpy restatement on a sample: the planted sibs and random pairs
        pairs = sorted({(t[2], t[3]) for t in truth[:4]} | {tuple(sorted(rng.choice(n, 2, replace=False).tolist())) for _ in range(SAMPLE_PAIRS - 4)})
        rows = sorted({i for p in pairs for i in p})
        sub = np.ascontiguousarray(G[rows])
        local = [(rows.index(a), rows.index(b)) for a, b in pairs]
        t1 = time.perf_counter()
        want = ir.segments_vec(sub, chrom, pos, pairs=local, kind=kind)
        t_np = time.perf_counter() - t1
        got = {(a, b, f, l) for a, b, f, l in zip(s["ind_a"].tolist(), s["ind_b"].tolist(), s["first"].tolist(), s["last"].tolist())
               if (a, b) in set(pairs)}
        ref = {(rows[a], rows[b], f, l) for a, b, f, l in zip(want["ind_a"].tolist(), want["ind_b"].tolist(), want["first"].tolist(),
                                                             want["last"].tolist())}
        print(f"    numpy route, {len(pairs)} pairs: {t_np:.2f} s, same segments as the device: {got == ref}; EXTRAPOLATED to {npairs} pairs: "
              f"{t_np / len(pairs) * npairs / 3600:.1f} h on one core")
    print(f"  genome length {tpg.ibd_genome_length(chrom, pos)}")
    v.free(); X.free()


if len(sys.argv) >= 3:
    probe(int(sys.argv[1]), int(sys.argv[2]))
else:
    probe(1000, 650_000)
    probe(5000, 1_000_000)
