#!/usr/bin/env python3
"""AMOVA (include/tpg.h "AMOVA") at the sizes it is for, on synthetic panels (FBM.synth, ten populations in five regions, 2 %
missing; NO real panel is measured):

  n5000     5 000 individuals x 100 000 loci.  The squared distance stays in HBM.  class_sums with the labelings gt_amova issues
            at n_perm = 999: the all-zero row, 1 + 2 x 999 population rows, 1 + 2 x 999 region rows.  Device time from the
            library's profiler (HIP events around every launch), cells per second of the partial kernel (a cell = one (i, j,
            labeling)), and the two estimates of DESIGN 3.25 beside it: VALU issue (10 cycles per wave and cell column: a
            compare and two selects at 2 cycles each on the 32-wide SIMD, an FP64 add at 4) and the re-read of A once per batch
            of labelings.  Then one whole gt_amova call from the FBM, and the share of the pairwise pass in it.
  numpy     the comparison: the numpy restatement of the ordered sum (tests/amova_ref.py) on the same machine, on the same
            5 000 x 5 000 matrix, NUMPY_ROWS labelings, which it finishes; its rows equal the device's bit for bit.  The time
            for all the labelings is EXTRAPOLATED from that (the restatement is linear in the number of rows).
  n20000    20 000 individuals x 20 000 loci, N20_ROWS population rows.

Every figure says how many runs are behind it.  Every step is a child process under its own time limit and a step that fails ends
the probe.

    python tools/amova_probe.py      writes profiles/amova_probe.txt"""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

NPOP, NREG, N_PERM = 10, 5, 999
N5, M5 = 5000, 100000
N20, M20, N20_ROWS = 20000, 20000, 512
NUMPY_ROWS = 32
RUNS = 3
LIMIT_S = 420
CLOCK_HZ, SIMDS, CYCLES_PER_CELL_COLUMN = 2.4e9, 1024, 10
OUT = os.path.join("profiles", "amova_probe.txt")


def emit(text):
    print(text, flush=True)
    with open(OUT, "a") as f:
        f.write(text + "\n")


def _design(n):
    return np.ascontiguousarray(np.arange(n) % NPOP, dtype=np.int32), np.ascontiguousarray(np.arange(NPOP) // 2, dtype=np.int32)


def _rows(tpg, n, pop, reg, scheme, count, regions=False):
    out = []
    for r in range(1, count + 1):
        p, g = tpg.amova_perm_labels(n, pop, NPOP, reg, NREG, scheme, 11, r)
        out.append(g[p] if regions else p)
    return out


def _profiled(ctx, call):
    ctx.prof_enable(True)
    ctx.prof_reset()
    call()
    kern = ctx.prof_dump()
    ctx.prof_enable(False)
    return kern


def _kern_text(kern):
    return ", ".join(f"{k} {ms:.2f} ms x{cnt}" for k, (cnt, ms) in sorted(kern.items()))


def _class_sums_report(tpg, ctx, A, n, lab, k, what):
    B = int(tpg._lib.lib.tpg_classsum_batch())
    tpg.class_sums(A, lab[:B], k)  # warm-up: code objects, the pool
    walls = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        tpg.class_sums(A, lab, k)
        walls.append(time.perf_counter() - t0)
    kern = _profiled(ctx, lambda: tpg.class_sums(A, lab, k))
    R = len(lab)
    part = kern["classsum_partial"][1] * 1e-3
    cells = R * n * n
    padded = -(-R // B) * B * n * n  # what the kernel computes: whole batches
    issue = padded / 64 * CYCLES_PER_CELL_COLUMN / (SIMDS * CLOCK_HZ)
    reread = -(-R // B) * n * n * 8
    emit(f"  {what}: {R} labelings, {k} classes: device {sum(ms for _, ms in kern.values()):.2f} ms (ONE profiled run: {_kern_text(kern)}); "
         f"wall {np.median(walls) * 1e3:.1f} ms (median of {RUNS} runs after a warm-up, min {min(walls) * 1e3:.1f}, max {max(walls) * 1e3:.1f}: "
         f"the host's checks, label table and transfers included)")
    emit(f"    partial kernel: {cells / part:.3e} cells/s; the VALU-issue estimate gives {issue * 1e3:.2f} ms for its {padded:.3e} computed cells "
         f"({part / issue:.2f} x the estimate); A is re-read once per batch of {B}: {reread / 2 ** 30:.1f} GiB, {reread / part / 1e12:.2f} TB/s if none of it "
         f"were shared through a cache")
    return kern


def step_n5000():
    import tidypopgen_amd as tpg

    ctx = tpg.default_context()
    pop, reg = _design(N5)
    X = tpg.FBM.synth(7, N5, M5, npop=NPOP, miss=0.02)
    tpg.pairwise_sqdist(tpg.FBM.synth(3, 64, 512, npop=4), device=True)  # warm-up
    t0 = time.perf_counter()
    A = tpg.pairwise_sqdist(X, device=True)
    ctx.sync()
    t_dist = time.perf_counter() - t0
    emit(f"n = {N5}, {M5} loci: the squared distance (view packed, one pairwise pass with the KING products, epilogue; stays in HBM): "
         f"{t_dist * 1e3:.0f} ms wall, ONE run after a warm-up at another size; scratch bound of class_sums "
         f"{tpg._lib.lib.tpg_class_sums_scratch_bytes(N5, 10 ** 9, NPOP) / 2 ** 20:.0f} MiB for any number of labelings")
    t0 = time.perf_counter()
    st, sc = _rows(tpg, N5, pop, reg, 0, N_PERM), _rows(tpg, N5, pop, reg, 1, N_PERM)
    lab_pop = np.stack([pop] + st + sc)
    lab_reg = np.stack([reg[pop]] + [reg[p] for p in st] + _rows(tpg, N5, pop, reg, 2, N_PERM, regions=True))
    emit(f"  the {3 * N_PERM} relabelings on the host (tpg_amova_perm_labels): {time.perf_counter() - t0:.2f} s, ONE run")
    _class_sums_report(tpg, ctx, A, N5, np.zeros((1, N5), dtype=np.int32), 1, "the all-zero row (T)")
    _class_sums_report(tpg, ctx, A, N5, lab_pop, NPOP, "population rows")
    _class_sums_report(tpg, ctx, A, N5, lab_reg, NREG, "region rows")
    t0 = time.perf_counter()
    out = tpg.gt_amova(X, pop=pop, npop=NPOP, region_of_pop=reg, n_perm=N_PERM, seed=11)
    ctx.sync()
    t = time.perf_counter() - t0
    emit(f"gt_amova from the FBM, n_perm = {N_PERM} ({1 + 2 * (1 + 2 * N_PERM)} labelings), ONE run: {t:.2f} s wall, of which the distance "
         f"(pack + pairwise pass + epilogue) took about {t_dist:.2f} s ({100 * t_dist / t:.0f} %) when measured alone above; the rest is the host's "
         f"relabelings, label tables, checks and {3 * N_PERM + 1} finisher calls around the kernels.  phi (CT, SC, ST) = "
         f"{np.array2string(out['phi'], precision=4)}, p = {out['p_value']}")
    # the comparison: the numpy restatement on the same matrix
    from tests import amova_ref as ar

    host = A.to_numpy()
    C = ar.constants()[0]
    t0 = time.perf_counter()
    want = ar.ordered_class_sums(host, lab_pop[:NUMPY_ROWS], NPOP, C)
    t_np = time.perf_counter() - t0
    got = tpg.class_sums(A, lab_pop[:NUMPY_ROWS], NPOP)
    total = len(lab_pop) + len(lab_reg) + 1
    emit(f"numpy restatement (tests/amova_ref.py, vectorised over rows and labelings), same machine, same {N5} x {N5} matrix in host memory: "
         f"{NUMPY_ROWS} population rows in {t_np:.2f} s, ONE run; equal to the device's rows bit for bit: {ar.same_values(got, want)}.  "
         f"EXTRAPOLATED linearly to the {total} labelings of the call: {t_np / NUMPY_ROWS * total:.0f} s, without the {host.nbytes / 2 ** 20:.0f} MiB "
         f"download it would need first")
    return 0


def step_n20000():
    import tidypopgen_amd as tpg

    ctx = tpg.default_context()
    pop, reg = _design(N20)
    X = tpg.FBM.synth(9, N20, M20, npop=NPOP, miss=0.02)
    t0 = time.perf_counter()
    A = tpg.pairwise_sqdist(X, device=True)
    ctx.sync()
    emit(f"n = {N20}, {M20} loci: the squared distance: {(time.perf_counter() - t0) * 1e3:.0f} ms wall, ONE cold run; the matrix is "
         f"{8 * N20 * N20 / 2 ** 30:.1f} GiB (beyond the Infinity Cache); scratch bound of class_sums "
         f"{tpg._lib.lib.tpg_class_sums_scratch_bytes(N20, 10 ** 9, NPOP) / 2 ** 20:.0f} MiB")
    lab = np.stack([pop] + _rows(tpg, N20, pop, reg, 0, N20_ROWS - 1))
    _class_sums_report(tpg, ctx, A, N20, lab, NPOP, "population rows")
    return 0


def main():
    steps = {"--n5000": step_n5000, "--n20000": step_n20000}
    if len(sys.argv) == 2 and sys.argv[1] in steps:
        return steps[sys.argv[1]]()
    os.makedirs("profiles", exist_ok=True)
    with open(OUT, "w") as f:
        f.write("tools/amova_probe.py: class sums under batches of labelings and gt_amova on one MI355X, synthetic panels only\n")
    for arg in steps:
        try:
            r = subprocess.run([sys.executable, __file__, arg], timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"no result within {LIMIT_S} s", flush=True)
            return 1
        if r.returncode != 0:
            print(f"exit status {r.returncode}", flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
