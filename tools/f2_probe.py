#!/usr/bin/env python3
"""Blocked f2 at the benchmark's panel size (5 000 x 1 000 000 synthetic, 51 groups, ~700 jackknife blocks) beside the Hudson
totals of tpg_pairwise_pop_fst_sums on the same view: the same count sweep and the same kind of FP64 matrix products, which is
the yardstick.  Every leg runs in a process of its own under its own time limit, on a view packed in that process: `first` is
the call on a fresh view (the count sweep included), `again` the same call on the same view (the view keeps its count table),
both wall clock around a call that ends synchronised; kernel times are HIP-event times of the `again` call.

    python tools/f2_probe.py [n m]             all legs
    python tools/f2_probe.py --leg NAME n m     one leg (what the driver starts)"""
import subprocess
import sys
import time

sys.path.insert(0, ".")

G = 51
NB = 700
LEGS = ("f2_default", "f2_without_ap", "f2_one_weight", "hudson_sums")
LIMIT_S = 300


def _wall(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    out = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, out


def leg(name, n, m):
    import ctypes as C

    import numpy as np

    import tidypopgen_amd as tpg

    ctx = tpg.default_context()
    X = tpg.FBM.synth(9, n, m, npop=G, miss=0.02)
    v = tpg.View(X)
    gid = (np.arange(n) * G // n).astype(np.int32)
    edges = np.linspace(0, m, NB + 1).astype(np.int64)
    lo, hi = edges[:-1].copy(), edges[1:].copy()
    ctx.prof_enable(True)
    if name == "hudson_sums":
        pairs = np.ascontiguousarray(tpg.combn2(G).T.astype(np.int32))  # (P, 2), 1-based
        P = len(pairs)
        num, den = np.zeros(P), np.zeros(P)
        call = lambda: tpg._lib.check(tpg._lib.lib.tpg_pairwise_pop_fst_sums(  # noqa: E731
            ctx.h, v.h, C.c_void_p(gid.ctypes.data), C.c_int(G), None, C.c_int(tpg.FST_METHODS["Hudson"]),
            C.c_void_p(pairs.ctypes.data), C.c_int(P), C.c_void_p(num.ctypes.data), C.c_void_p(den.ctypes.data)))
        down = 16 * P
    else:
        kw = dict(f2_default=dict(), f2_without_ap=dict(afprod=False), f2_one_weight=dict(poly_only=("f2", "ap")))[name]
        call = lambda: tpg.f2_blocks(v, gid, G, lo, hi, **kw)  # noqa: E731
        down = G * G * NB * (12 if name == "f2_without_ap" else 24) + 8 * NB
    first, _ = _wall(ctx, call)
    ctx.prof_reset()
    again, _ = _wall(ctx, call)
    prof = ctx.prof_dump()
    kern = ", ".join(f"{k} {ms:.3f} ms x{cnt}" for k, (cnt, ms) in sorted(prof.items()) if k.startswith(("f2_", "fst_", "grouped_")))
    print(f"{name:16s} first {first:9.2f} ms   again {again:9.2f} ms   bytes to the host {down:>12,d}")
    print(f"{'':16s} kernels of `again`: {kern or 'none'}", flush=True)


def main():
    if len(sys.argv) >= 5 and sys.argv[1] == "--leg":
        leg(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
        return 0
    n, m = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) >= 3 else (5000, 1_000_000)
    print(f"panel {n} x {m}, synthetic, 2 % missing, {G} groups, {NB} blocks; one call each, wall clock in ms", flush=True)
    for name in LEGS:
        try:
            r = subprocess.run([sys.executable, __file__, "--leg", name, str(n), str(m)], timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {LIMIT_S} s; stopping here", flush=True)
            return 1
        if r.returncode != 0:  # nothing more is started on the GPU after a failure
            print(f"{name}: exit status {r.returncode}; stopping here", flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
