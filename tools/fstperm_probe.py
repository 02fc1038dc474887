#!/usr/bin/env python3
"""Fst under relabelings (include/tpg.h "Fst under relabelings") at the size it is for, on a synthetic 5 000 x 1 000 000 panel
(FBM.synth, 10 populations, 2 % missing, packed once per step; NO real panel is measured):

  fused     tpg_fst_relabel_sums, 1 024 rows of the pairwise scheme (two groups per row: the rows r = 1, 2, ... of the 45 pairs in
            turn), Hudson, WC84 and Nei87; and 128 rows of the global scheme with ten groups, Hudson, all 45 pairs.
  loop      the route there was before: one tpg_pairwise_pop_fst_sums call per relabeling on that ONE view, the relabeling's
            labels as groupIds0 (for the two-group rows the individuals outside go into a third group that no pair names), run
            from ANOTHER BUILD of the library -- the parent commit's, given as FSTPERM_BASELINE_LIB -- over the first LOOP_ROWS
            rows of the same label matrices.
  test      one pairwise_pop_fst_test at 10 populations, n_perm = 999: 45 000 relabelings, wall time with the host's share.

Device time is the sum of the HIP-event times around every launch of the call(s) (the library's profiler), per relabeling;
beside it the wall time of the same calls.  Every figure says how many runs are behind it.  Every step is a child process under
its own time limit and a step that fails ends the probe.

    FSTPERM_BASELINE_LIB=/path/to/parent/libtpg_hip.so python tools/fstperm_probe.py      writes profiles/fstperm_probe.txt"""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

N, M, NPOP = 5000, 1000000, 10
R2, RG = 1024, 128
LOOP_ROWS = 24
RUNS = 3
LIMIT_S = 400
OUT = os.path.join("profiles", "fstperm_probe.txt")


def emit(text):
    print(text, flush=True)
    with open(OUT, "a") as f:
        f.write(text + "\n")


def _panel(tpg):
    small = tpg.View(tpg.FBM.synth(3, 64, 512, npop=4, miss=0.02))
    tpg.pairwise_pop_fst(small.X, None, None, np.arange(64) % 3, 3, sums=True)  # warm-up: code objects, the pool
    X = tpg.FBM.synth(7, N, M, npop=NPOP, miss=0.02)
    return X, tpg.View(X), np.ascontiguousarray(np.arange(N) % NPOP, dtype=np.int32)


def _rows2(tpg, gid, count):
    pairs = tpg.combn2(NPOP)
    return np.stack([tpg.fst_perm_labels(N, gid, NPOP, 0, int(pairs[0, k % 45]) - 1, int(pairs[1, k % 45]) - 1, 11, 1 + k // 45)
                     for k in range(count)])


def _rowsg(tpg, gid, count):
    return np.stack([tpg.fst_perm_labels(N, gid, NPOP, 1, 0, 0, 11, 1 + k) for k in range(count)])


def _timed(ctx, call, runs):
    call()  # warm-up at this shape
    walls = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        ctx.sync()
        walls.append(time.perf_counter() - t0)
    ctx.prof_enable(True)
    ctx.prof_reset()
    call()
    kern = ctx.prof_dump()
    ctx.prof_enable(False)
    return walls, kern


def _kern_text(kern):
    return ", ".join(f"{k} {ms:.2f} ms x{cnt}" for k, (cnt, ms) in sorted(kern.items()))


def step_fused():
    import tidypopgen_amd as tpg

    ctx = tpg.default_context()
    X, v, gid = _panel(tpg)
    one = np.array([[1], [2]], dtype=np.int32)
    lab2, labg = _rows2(tpg, gid, R2), _rowsg(tpg, gid, RG)
    emit(f"fused: {N} x {M}, scratch bound {tpg._lib.lib.tpg_fst_relabel_scratch_bytes(N, M, 2, 1) / 2 ** 20:.0f} MiB (two groups, one pair), "
         f"{tpg._lib.lib.tpg_fst_relabel_scratch_bytes(N, M, NPOP, 45) / 2 ** 20:.0f} MiB (ten groups, 45 pairs)")
    for method in ("Hudson", "WC84", "Nei87"):
        walls, kern = _timed(ctx, lambda: tpg.fst_relabel_sums(v, lab2, 2, one, method), RUNS)
        dev = sum(ms for _, ms in kern.values())
        emit(f"  pairwise scheme, {R2} rows, {method}: device {dev / R2 * 1e3:.2f} us per relabeling (ONE profiled run: {_kern_text(kern)}); "
             f"wall {np.median(walls) / R2 * 1e6:.2f} us per relabeling (median of {RUNS} runs after a warm-up, min {min(walls):.3f} s, max {max(walls):.3f} s per call)")
    walls, kern = _timed(ctx, lambda: tpg.fst_relabel_sums(v, labg, NPOP, None, "Hudson"), RUNS)
    dev = sum(ms for _, ms in kern.values())
    emit(f"  global scheme, {RG} rows of {NPOP} groups, 45 pairs, Hudson: device {dev / RG * 1e3:.1f} us per relabeling (ONE profiled run: "
         f"{_kern_text(kern)}); wall {np.median(walls) / RG * 1e6:.1f} us per relabeling (median of {RUNS} runs, min {min(walls):.3f} s, max {max(walls):.3f} s)")
    return 0


def step_loop():
    import tidypopgen_amd as tpg

    assert not hasattr(tpg._lib.lib, "tpg_fst_relabel_sums"), "the baseline must be a build without the code under test"
    ctx = tpg.default_context()
    X, v, gid = _panel(tpg)
    # the labels come from the restatement (this build of the library has no tpg_fst_perm_labels)
    from tests import fstperm_ref as fr

    pairs = tpg.combn2(NPOP)
    lab2 = np.stack([fr.perm_labels(N, gid, NPOP, 0, int(pairs[0, k % 45]) - 1, int(pairs[1, k % 45]) - 1, 11, 1 + k // 45)
                     for k in range(LOOP_ROWS)])
    lab2 = np.where(lab2 < 0, 2, lab2).astype(np.int32)  # the individuals outside: a third group that no pair names
    labg = np.stack([fr.perm_labels(N, gid, NPOP, 1, 0, 0, 11, 1 + k) for k in range(LOOP_ROWS)])
    one = np.array([[1], [2]], dtype=np.int32)
    for what, lab, G, prs in (("pairwise scheme (three groups, the pair (1, 2))", lab2, 3, one), (f"global scheme ({NPOP} groups, 45 pairs)", labg, NPOP, None)):
        for method in (("Hudson", "WC84", "Nei87") if G == 3 else ("Hudson",)):
            # ONE view for every call: pairwise_pop_fst packs a view per call, so the loop goes through the C entry point
            def call_view(G=G, prs=prs, method=method, lab=lab):
                import ctypes as C

                pc = np.ascontiguousarray((tpg.combn2(G) if prs is None else prs).T)
                sn, sd = np.zeros(pc.shape[0]), np.zeros(pc.shape[0])
                pl = np.full(N, 2.0)
                for row in lab:
                    row = np.ascontiguousarray(row, dtype=np.int32)
                    tpg._lib.check(tpg._lib.lib.tpg_pairwise_pop_fst_sums(ctx.h, v.h, C.c_void_p(row.ctypes.data), G, C.c_void_p(pl.ctypes.data),
                                                                          tpg.api.FST_METHODS[method], C.c_void_p(pc.ctypes.data), pc.shape[0],
                                                                          C.c_void_p(sn.ctypes.data), C.c_void_p(sd.ctypes.data)))

            walls, kern = _timed(ctx, call_view, RUNS)
            dev = sum(ms for _, ms in kern.values())
            emit(f"loop (parent build), {what}, {method}: device {dev / len(lab) * 1e3:.1f} us per relabeling (ONE profiled run of {len(lab)} calls: "
                 f"{_kern_text(kern)}); wall {np.median(walls) / len(lab) * 1e6:.1f} us per relabeling (median of {RUNS} runs of {len(lab)} calls)")
    return 0


def step_test():
    import tidypopgen_amd as tpg

    ctx = tpg.default_context()
    X, v, gid = _panel(tpg)
    t0 = time.perf_counter()
    out = tpg.pairwise_pop_fst_test(X, None, None, gid, NPOP, method="Hudson", n_perm=999, seed=1)
    ctx.sync()
    t = time.perf_counter() - t0
    emit(f"pairwise_pop_fst_test, {NPOP} populations, n_perm = 999 (45 000 relabelings), Hudson, ONE run: {t:.1f} s wall, the packing of the view, "
         f"the host's label rows and argument checks included; p in [{out['p_value'].min():.3f}, {out['p_value'].max():.3f}], n_valid "
         f"{int(out['n_valid'].min())} .. {int(out['n_valid'].max())}.  A synthetic panel: no real panel was measured.")
    return 0


def main():
    if len(sys.argv) == 2 and sys.argv[1] in ("--fused", "--loop", "--test"):
        return {"--fused": step_fused, "--loop": step_loop, "--test": step_test}[sys.argv[1]]()
    base = os.environ.get("FSTPERM_BASELINE_LIB")
    if not base or not os.path.exists(base):
        print("FSTPERM_BASELINE_LIB must name a build of the parent commit's library", flush=True)
        return 2
    os.makedirs("profiles", exist_ok=True)
    with open(OUT, "w") as f:
        f.write("tools/fstperm_probe.py: relabelled Fst sums, the fused call against a loop of tpg_pairwise_pop_fst_sums calls, same job\n")
    for arg in ("--fused", "--loop", "--test"):
        env = dict(os.environ)
        env.pop("TPG_LIB_PATH", None)
        if arg == "--loop":
            env["TPG_LIB_PATH"] = base
        try:
            r = subprocess.run([sys.executable, __file__, arg], timeout=LIMIT_S, env=env)
        except subprocess.TimeoutExpired:
            print(f"no result within {LIMIT_S} s", flush=True)
            return 1
        if r.returncode != 0:
            print(f"exit status {r.returncode}", flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
