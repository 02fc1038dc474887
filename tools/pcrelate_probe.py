#!/usr/bin/env python3
"""PC-Relate (include/tpg.h "PC-Relate") at the sizes it is for: one timed tpg.pcrelate call per shape on a synthetic panel of
four populations with 5 % missing genotypes (the view is packed before the clock starts; the call ends with kin, f and n_snp
in host memory), then ONE further call with HIP events around every launch for the kernel-level split, and the FP64 rate of the
Gram kernel from 3 n^2 m flops (three chains over the lower triangle) over its kernel time.  The only comparison is with the
numpy restatement (tests/pcrelate_ref.py), timed once at a small size on this host and EXTRAPOLATED by n^2 m -- marked as such
in the output.  Every shape is one step, run as a child process under its own time limit, and a step that fails ends the probe.
For the record: no figure here is a pass criterion.

    python tools/pcrelate_probe.py          writes profiles/pcrelate_probe.txt"""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

SHAPES = [(5000, 1000000, 10), (20000, 100000, 10)]
SMALL = (1000, 20000, 10)  # the restatement's timed size
LIMIT_S = 420
OUT = os.path.join("profiles", "pcrelate_probe.txt")


def scores(n, K, m, seed):
    """population contrasts of the synthetic panel (individual i belongs to population i mod 4), then independent columns"""
    rng = np.random.default_rng(seed)
    pop = np.arange(n) % 4
    cols = [(pop == g).astype(float) - 0.25 for g in range(3)][:K]
    cols += [rng.standard_normal(n) for _ in range(K - len(cols))]
    return np.asfortranarray(np.column_stack(cols) * np.sqrt(float(m)))


def emit(text):
    print(text, flush=True)
    with open(OUT, "a") as f:
        f.write(text + "\n")


def step_model():
    from oracle import oracle as orc
    from tests import pcrelate_ref as pr

    n, m, K = SMALL
    codes = orc.synth_fbm(7, n, m, npop=4, miss=0.05)
    V = scores(n, K, m, 1)
    t0 = time.perf_counter()
    pr.pcrelate(codes, V)
    t = time.perf_counter() - t0
    lines = [f"numpy restatement (tests/pcrelate_ref.py: pcrelate) at {n} x {m}, K = {K}, one run on this host: {t:.2f} s"]
    for nn, mm, _ in SHAPES:
        lines.append(f"  EXTRAPOLATED by n^2 m to {nn} x {mm}: {t * (nn / n) ** 2 * (mm / m):.0f} s (not measured)")
    emit("\n".join(lines))
    return 0


def step(n, m, K):
    import tidypopgen_amd as tpg

    ctx = tpg.default_context()
    small = tpg.View(tpg.FBM.synth(3, 64, 256, npop=4, miss=0.05), code256=None)
    tpg.pcrelate(small, scores(64, K, 256, 0))  # warm-up: code objects, the pool
    X = tpg.FBM.synth(7, n, m, npop=4, miss=0.05)
    v = tpg.View(X, code256=None)
    V = scores(n, K, m, 1)
    ctx.sync()
    t0 = time.perf_counter()
    r = tpg.pcrelate(v, V)
    ctx.sync()
    wall = time.perf_counter() - t0
    kin = r["kin"]
    off = kin[~np.eye(n, dtype=bool)] if n <= 5000 else kin[np.triu_indices(n, 1)]
    stats = f"n_snp {int(r['n_snp'].min())} .. {int(r['n_snp'].max())}, off-diagonal kin mean {off.mean():.2e} sd {off.std():.2e}, " \
            f"f mean {r['inbreeding'].mean():.2e}"
    del r, kin, off
    ctx.prof_enable(True)
    ctx.prof_reset()
    tpg.pcrelate(v, V, return_counts=False)
    kern = ctx.prof_dump()
    ctx.prof_enable(False)
    gram_n, gram_ms = kern.get("pcrelate_gram", (0, float("nan")))
    op_n, op_ms = kern.get("pcrelate_operands", (0, float("nan")))
    flops = 3.0 * n * n * m
    B = tpg.pcrelate_block_loci(n)
    emit("\n".join([
        f"{n} x {m} loci, K = {K}, 5% missing; operand block B = {B} loci, operand scratch {tpg.pcrelate_scratch_bytes(n, m, K) / 2 ** 20:.0f} MiB",
        f"  tpg.pcrelate, ONE run: {wall:.3f} s wall from the packed view to kin, f and n_snp in host memory ({stats})",
        f"  kernels, ONE further run (HIP events, no n_snp): pcrelate_gram {gram_ms:.1f} ms in {gram_n} launches "
        f"({flops / gram_ms / 1e9:.1f} TFLOP/s FP64 from 3 n^2 m = {flops:.3g} flops), pcrelate_operands {op_ms:.1f} ms in {op_n} launches; "
        f"all: " + ", ".join(f"{k} {ms:.1f}" for k, (cnt, ms) in sorted(kern.items()))]))
    return 0


def main():
    if len(sys.argv) == 2 and sys.argv[1] == "--model":
        return step_model()
    if len(sys.argv) == 5 and sys.argv[1] == "--step":
        return step(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    os.makedirs("profiles", exist_ok=True)
    with open(OUT, "w") as f:
        f.write("tools/pcrelate_probe.py: tpg.pcrelate on a synthetic panel, one timed run and one profiled run per shape\n")
    # every step that uses the GPU runs as a child under its own time limit; nothing follows a step that failed
    for args in [["--step", str(n), str(m), str(K)] for n, m, K in SHAPES] + [["--model"]]:
        try:
            r = subprocess.run([sys.executable, __file__, *args], timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"no result within {LIMIT_S} s", flush=True)
            return 1
        if r.returncode != 0:
            print(f"exit status {r.returncode}", flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
