#!/usr/bin/env python3
"""Windowed pairwise Fst at the benchmark's Fst shape (5 000 x 1 000 000 synthetic, 51 groups, 1 275 pairs) with two window
lists (1 000 SNPs step 1 000, and 1 000 SNPs step 100): the staged route (tpg_pairwise_pop_fst(return_num_dem = 1) into two
m x P device matrices, then tpg_window_stats over each) beside the fused route (tpg_windows_pairwise_pop_fst) on the same view.
Every leg runs once in a process of its own under its own time limit, on a view packed in that process: `cold` is the call on
a fresh view (the count sweep included), `warm` the same call on the same view (the view keeps its count table), both wall
clock around a call that ends synchronised; kernel times are HIP-event times (tpg_prof_dump) of the `warm` call; `device
growth` is the growth of the device memory in use (hipMemGetInfo) over the cold call, in a pool that keeps what it allocated.
The staged route is Hudson only (what windows_pairwise_pop_fst computes); its WC84 leg runs the same two steps by hand.

    python tools/winfst_probe.py [n m]           all legs
    python tools/winfst_probe.py --leg NAME n m   one leg (what the driver starts)"""
import ctypes as C
import subprocess
import sys
import time

sys.path.insert(0, ".")

G = 51
LEGS = tuple(f"{route}_{method}_step{step}" for step in (1000, 100) for method in ("Hudson", "WC84") for route in ("staged", "fused"))
LIMIT_S = 400


def _used(hip):
    fr, tot = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
    return tot.value - fr.value


def _wall(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    out = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, out


def leg(name, n, m):
    import numpy as np

    import tidypopgen_amd as tpg
    from tidypopgen_amd.api import FST_METHODS, _ptr, _window_stats, check, lib

    route, method, step = name.split("_")
    step = int(step[4:])
    hip = C.CDLL("libamdhip64.so.7")
    ctx = tpg.default_context()
    X = tpg.FBM.synth(9, n, m, npop=G, miss=0.02)
    v = tpg.View(X)
    gid = (np.arange(n) * G // n).astype(np.int32)
    wr = tpg.window_index_ranges(np.ones(m, dtype=np.int32), None, 1000, step)
    nw = len(wr["lo"])
    pairs_c = np.ascontiguousarray(tpg.combn2(G).T)
    P = len(pairs_c)
    pl = np.full(n, 2.0)

    def staged():
        d_num, d_den = ctx.dev_alloc(8 * m * P), ctx.dev_alloc(8 * m * P)
        try:
            check(lib.tpg_pairwise_pop_fst(ctx.h, v.h, _ptr(gid), G, _ptr(pl), FST_METHODS[method], _ptr(pairs_c), P, 1, 1, None,
                                           d_num, d_den))
            num, _ = _window_stats(ctx, d_num, m, P, wr, 0, 1)
            den, _ = _window_stats(ctx, d_den, m, P, wr, 0, 1)
        finally:
            ctx.dev_free(d_num)
            ctx.dev_free(d_den)
        with np.errstate(invalid="ignore", divide="ignore"):
            return num / den

    def fused():
        return tpg.windows_fst(v, gid, G, wr["lo"], wr["hi"], wr["pad_na"], 1, pl, method)["fst"]

    call = staged if route == "staged" else fused
    ctx.prof_enable(True)
    ctx.sync()
    before = _used(hip)
    cold, a = _wall(ctx, call)
    growth = _used(hip) - before
    ctx.prof_reset()
    warm, b = _wall(ctx, call)
    prof = ctx.prof_dump()
    kern = ", ".join(f"{k} {ms:.3f} ms x{cnt}" for k, (cnt, ms) in sorted(prof.items()))
    same = "same bits" if a.tobytes() == b.tobytes() else "BITS DIFFER between the two calls"
    print(f"{name:26s} cold {cold:9.2f} ms   warm {warm:9.2f} ms   device growth {growth / 1e6:10.1f} MB   {nw} windows x {P} pairs"
          f"   scratch by the header {tpg.windows_fst_scratch_bytes(m, G, P, nw) / 1e6:.1f} MB   {same}")
    print(f"{'':26s} kernels of `warm`: {kern}   winfst_ total {ctx.prof_get('winfst_')[0]:.3f} ms", flush=True)


def main():
    if len(sys.argv) >= 5 and sys.argv[1] == "--leg":
        leg(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
        return 0
    n, m = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) >= 3 else (5000, 1_000_000)
    print(f"panel {n} x {m}, synthetic, 2 % missing, {G} groups; windows of 1 000 SNPs; one call each, wall clock in ms", flush=True)
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
