#!/usr/bin/env python3
"""Tajima's D at the benchmark's panel size (5 000 x 1 000 000 synthetic, 10 groups) with two window lists (1 000 SNPs step
1 000, and 1 000 SNPs step 100): the whole-view call and the windowed call, beside what the library offered before them for
the same answer -- gt_grouped_pi_diploid to the host (16 m G bytes) and a numpy finish.  Every leg runs once in a process of
its own under its own time limit, on a view packed in that process: `first` is the call on a fresh view (the count sweep
included), `again` the same call on the same view (the view keeps its count table), both wall clock around a call that ends
synchronised; kernel times are HIP-event times from tpg_prof_get("tajima_") of the `again` call.

    python tools/tajima_probe.py [n m]          all legs
    python tools/tajima_probe.py --leg NAME n m  one leg (what the driver starts)"""
import subprocess
import sys
import time

sys.path.insert(0, ".")

G = 10
LEGS = ("whole", "windows_step1000", "windows_step100", "parent_whole", "parent_windows_step1000", "parent_windows_step100")
LIMIT_S = 300


def _wall(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    out = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, out


def leg(name, n, m):
    import numpy as np

    import tidypopgen_amd as tpg

    ctx = tpg.default_context()
    X = tpg.FBM.synth(9, n, m, npop=G, miss=0.02)
    v = tpg.View(X)
    gid = (np.arange(n) * G // n).astype(np.int32)
    step = 100 if name.endswith("step100") else 1000
    wr = tpg.window_index_ranges(np.ones(m, dtype=np.int32), None, 1000, step)
    nw = len(wr["lo"])
    ctx.prof_enable(True)
    if name == "whole":
        # the public function packs a view per call; time the C entry point on ONE view so that `again` finds the count table
        import ctypes as C

        d, seg, k = np.zeros(G), np.zeros(G, dtype=np.int64), np.zeros(G)
        call = lambda: tpg._lib.check(tpg._lib.lib.tpg_pop_tajimas_d(  # noqa: E731
            ctx.h, v.h, C.c_void_p(gid.ctypes.data), C.c_int(G), None, C.c_void_p(d.ctypes.data), C.c_void_p(seg.ctypes.data),
            C.c_void_p(k.ctypes.data)))
        down = 3 * 8 * G
    elif name.startswith("windows"):
        call = lambda: tpg.tajima_windows(v, gid, G, wr["lo"], wr["hi"], wr["pad_na"], 1)  # noqa: E731
        down = nw * G * (8 + 8 + 8 + 4)
    else:
        def call():
            r = tpg.gt_grouped_pi_diploid(v, gid, G)  # pi and n, m x G doubles each, to the host
            t0 = time.perf_counter()
            pi = r["pi"]
            if name == "parent_whole":
                seg = ((pi > 0) & (pi < 1)).sum(axis=0)
                out = [tpg.tajimas_d_from_sums(2 * int((gid == g).sum()), int(seg[g]), float(pi[:, g].sum())) for g in range(G)]
            else:
                out = np.empty((nw, G))
                sizes = np.bincount(gid, minlength=G)
                for w in range(nw):
                    sl = pi[wr["lo"][w]:wr["hi"][w]]
                    seg, kh = ((sl > 0) & (sl < 1)).sum(axis=0), sl.sum(axis=0)
                    out[w] = [tpg.tajimas_d_from_sums(2 * int(sizes[g]), int(seg[g]), float(kh[g])) for g in range(G)]
            call.finish_ms = (time.perf_counter() - t0) * 1e3
            return out
        down = 16 * m * G
    first, _ = _wall(ctx, call)
    extra = f" (numpy finish {call.finish_ms:.1f})" if name.startswith("parent") else ""
    ctx.prof_reset()
    again, _ = _wall(ctx, call)
    extra2 = f" (numpy finish {call.finish_ms:.1f})" if name.startswith("parent") else ""
    prof = ctx.prof_dump()
    kern = ", ".join(f"{k} {ms:.3f} ms x{cnt}" for k, (cnt, ms) in sorted(prof.items()) if k.startswith(("tajima_", "grouped_")))
    windows = f", {nw} windows" if "windows" in name else ""
    print(f"{name:26s} first {first:9.2f} ms{extra}   again {again:9.2f} ms{extra2}   bytes to the host {down:>12,d}{windows}")
    print(f"{'':26s} kernels of `again`: {kern or 'none of tajima_ / grouped_'}   tajima_ total {ctx.prof_get('tajima_')[0]:.3f} ms")


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
