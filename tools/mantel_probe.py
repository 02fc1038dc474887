#!/usr/bin/env python3
"""Mantel tests (include/tpg.h "Mantel tests") at the sizes they are for, on synthetic panels (FBM.synth, ten populations, 2 %
missing, coordinates drawn uniformly; NO real panel is measured):

  n5000     5 000 individuals x 100 000 loci.  The squared distance stays in HBM, y = great-circle distances, z = those of a second
            coordinate set.  mantel_sums with R = 1 000 permutations, Q = 1 and Q = 2: device time of the product kernel and of the
            reduce kernel from the library's profiler (HIP events around every launch), wall time of the call, cells per second
            (a cell = one (r, i, j): R n^2 / t) and the implied re-read rate of A (R n^2 8 B / t), to set beside the Infinity
            Cache and L2 figures.  Then one whole gt_mantel (n_perm = 999), split into distance, permutations, kernels and host,
            and Spearman's form, whose ranks are host work.
  numpy     the comparison: (A[np.ix_(p, p)] * B)[off].sum() on the same machine and the same matrices in host memory, NUMPY_PERMS
            permutations, which it finishes; the time for all of them is EXTRAPOLATED from that.
  n16384    16 384 individuals (the largest n: a column of A fills 128 KiB of LDS), R = 128, Q = 1.

Every figure says how many runs are behind it.  Every step is a child process under its own time limit and a step that fails ends
the probe.

    python tools/mantel_probe.py      writes profiles/mantel_probe.txt"""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

N5, M5, R5 = 5000, 100000, 1000
N16, M16, R16 = 16384, 4096, 128
NUMPY_PERMS = 8
RUNS = 3
LIMIT_S = 420
OUT = os.path.join("profiles", "mantel_probe.txt")


def emit(text):
    print(text, flush=True)
    with open(OUT, "a") as f:
        f.write(text + "\n")


def _profiled(ctx, call):
    ctx.prof_enable(True)
    ctx.prof_reset()
    out = call()
    kern = ctx.prof_dump()
    ctx.prof_enable(False)
    return kern, out


def _kern_text(kern):
    return ", ".join(f"{k} {ms:.2f} ms x{cnt}" for k, (cnt, ms) in sorted(kern.items()))


def _coords(seed, n):
    rng = np.random.default_rng(seed)
    return rng.uniform(-20, 40, size=n), rng.uniform(30, 65, size=n)


def _sums_report(tpg, ctx, A, Bs, perms, what):
    n, R, Q = A.n, len(perms), len(Bs)
    tpg.mantel_sums(A, Bs, perms[:32])  # warm-up: code objects, the pool
    walls = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        tpg.mantel_sums(A, Bs, perms)
        walls.append(time.perf_counter() - t0)
    kern, _ = _profiled(ctx, lambda: tpg.mantel_sums(A, Bs, perms))
    prod = kern["mantel_product"][1] * 1e-3
    cells = R * n * n
    emit(f"  {what}: n = {n}, R = {R}, Q = {Q}: device {sum(ms for _, ms in kern.values()):.2f} ms (ONE profiled run: {_kern_text(kern)}); wall "
         f"{np.median(walls) * 1e3:.1f} ms (median of {RUNS} runs after a warm-up, min {min(walls) * 1e3:.1f}, max {max(walls) * 1e3:.1f}: the "
         f"host's bijection check, inverses and transfers included)")
    emit(f"    product kernel: {cells / prod:.3e} cells/s ({cells:.3e} cells, one LDS gather each, {Q} product(s) and add(s)); A is re-read "
         f"once per batch of 32 permutations: {cells / 32 * 8 / 2 ** 30:.1f} GiB = {cells / 32 * 8 / prod / 1e12:.3f} TB/s; the streamed reads "
         f"(4 B of permutation and {8 * Q} B of B per cell) are {cells * (4 + 8 * Q) / 2 ** 30:.0f} GiB = {cells * (4 + 8 * Q) / prod / 1e12:.2f} TB/s "
         f"from L2 / Infinity Cache; R n^2 8 B / t = {cells * 8 / prod / 1e12:.2f} TB/s (the rate at which a kernel that staged a column "
         f"of A per permutation would have to re-read A to keep up)")
    return kern


def step_n5000():
    import tidypopgen_amd as tpg

    ctx = tpg.default_context()
    X = tpg.FBM.synth(7, N5, M5, npop=10, miss=0.02)
    tpg.pairwise_sqdist(tpg.FBM.synth(3, 64, 512, npop=4), device=True)  # warm-up
    t0 = time.perf_counter()
    A = tpg.pairwise_sqdist(X, device=True)
    ctx.sync()
    t_dist = time.perf_counter() - t0
    emit(f"n = {N5}, {M5} loci: the squared distance (stays in HBM): {t_dist * 1e3:.0f} ms wall, ONE run after a warm-up at another size; "
         f"scratch bound of mantel_sums {tpg.mantel_scratch_bytes(N5, 10 ** 9, 2) / 2 ** 20:.0f} MiB for any number of permutations (Q = 2)")
    t0 = time.perf_counter()
    y, z = tpg.great_circle_dist(*_coords(1, N5)), tpg.great_circle_dist(*_coords(2, N5))
    emit(f"  two great-circle matrices on the host (numpy): {time.perf_counter() - t0:.2f} s, ONE run")
    times = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        perms = tpg.mantel_perms(N5, 11, 0, R5)
        times.append(time.perf_counter() - t0)
    emit(f"  the {R5} permutations on the host (ONE tpg_mantel_perms call): {np.median(times) * 1e3:.0f} ms (median of {RUNS} runs)")
    # centred operands, as the driver forms them
    mats = []
    for M in (A, tpg.DeviceMatrix.from_numpy(y), tpg.DeviceMatrix.from_numpy(z)):
        S, _ = tpg.offdiag_moments(M)
        mats.append(tpg.offdiag_center(M, S / (N5 * (N5 - 1.0))))
    _sums_report(tpg, ctx, mats[0], mats[1:2], perms, "Mantel")
    _sums_report(tpg, ctx, mats[0], mats[1:3], perms, "partial Mantel")
    # the whole driver, y and z as host matrices (their upload is part of the call).  The parts are timed INSIDE the call: a host
    # clock around every library call gt_mantel makes, the stream drained before each reading; what is left is Python and numpy
    tpg.gt_mantel(X, y=y, n_perm=31, seed=11)  # warm-up
    api, acc = tpg.api, {}

    def timed(owner, name, label):
        inner = getattr(owner, name)

        def outer(*args, **kw):
            ctx.sync()
            t0 = time.perf_counter()
            out = inner(*args, **kw)
            ctx.sync()
            acc[label] = acc.get(label, 0.0) + time.perf_counter() - t0
            return out

        setattr(owner, name, outer)
        return inner

    parts = (("pairwise_sqdist", "distance"), ("mantel_perms", "permutations"), ("mantel_sums", "mantel_sums"),
             ("offdiag_moments", "moments + centring"), ("offdiag_center", "moments + centring"))
    kept = [(api, name, timed(api, name, label)) for name, label in parts]
    upload = api.DeviceMatrix.from_numpy.__func__

    def from_numpy(cls, A_, ctx_=None):
        ctx.sync()
        t0 = time.perf_counter()
        out = upload(cls, A_, ctx_)
        ctx.sync()
        acc["uploads"] = acc.get("uploads", 0.0) + time.perf_counter() - t0
        return out

    api.DeviceMatrix.from_numpy = classmethod(from_numpy)
    for what, kw in (("gt_mantel", dict(y=y)), ("gt_mantel, partial", dict(y=y, z=z))):
        acc.clear()
        t0 = time.perf_counter()
        out = tpg.gt_mantel(X, n_perm=R5 - 1, seed=11, **kw)
        ctx.sync()
        t = time.perf_counter() - t0
        emit(f"{what} from the FBM, n_perm = {R5 - 1}, ONE run, every library call inside it timed by a host clock with the stream drained: "
             f"{t * 1e3:.1f} ms wall = " + " + ".join(f"{k} {v * 1e3:.1f}" for k, v in acc.items())
             + f" + the rest {(t - sum(acc.values())) * 1e3:.1f} (Python, numpy's finisher and p-value).  mantel_sums includes the host's bijection "
             f"check, the inverses and the transfers of the permutations; uploads are y and z, {8 * N5 * N5 / 2 ** 20:.0f} MiB each, from pageable "
             f"memory.  r = {out['statistic']:.4f}, p = {out['p_value']:.3f}")
    for owner, name, inner in kept:
        setattr(owner, name, inner)
    api.DeviceMatrix.from_numpy = classmethod(upload)
    # Spearman's form: the ranks are host work
    t0 = time.perf_counter()
    tpg.offdiag_midranks(y)
    t_rank = time.perf_counter() - t0
    t0 = time.perf_counter()
    out = tpg.gt_mantel(X, y=y, method="spearman", n_perm=R5 - 1, seed=11)
    t = time.perf_counter() - t0
    emit(f"gt_mantel(method='spearman') from the FBM, n_perm = {R5 - 1}, ONE run: {t:.2f} s wall; the mid-ranks of ONE {N5} x {N5} matrix on the host "
         f"(numpy: one stable argsort of {N5 * (N5 - 1) // 2} entries) {t_rank:.2f} s, ONE run, and the call ranks two, after a "
         f"{8 * N5 * N5 / 2 ** 20:.0f} MiB download of the distances.  r = {out['statistic']:.4f}, p = {out['p_value']:.3f}")
    # the comparison: vectorised numpy on the same matrices
    hA, hB = mats[0].to_numpy(), mats[1].to_numpy()
    off = ~np.eye(N5, dtype=bool)
    t0 = time.perf_counter()
    got = [float((hA[np.ix_(p, p)] * hB)[off].sum()) for p in perms[:NUMPY_PERMS]]
    t_np = time.perf_counter() - t0
    dev_sums = tpg.mantel_sums(mats[0], mats[1:2], perms[:NUMPY_PERMS])[:, 0]
    rel = max(abs(a - b) / max(abs(b), 1e-300) for a, b in zip(got, dev_sums))
    emit(f"numpy, (A[np.ix_(p, p)] * B)[off].sum(), same machine, same {N5} x {N5} matrices in host memory: {NUMPY_PERMS} permutations in "
         f"{t_np:.2f} s ({t_np / NUMPY_PERMS:.3f} s each), ONE run; largest relative difference from the device's sums {rel:.1e} (numpy adds "
         f"pairwise, in another order).  EXTRAPOLATED linearly to the {R5} permutations: {t_np / NUMPY_PERMS * R5:.0f} s, without the two "
         f"{hA.nbytes / 2 ** 20:.0f} MiB downloads it would need first")
    return 0


def step_n16384():
    import tidypopgen_amd as tpg

    ctx = tpg.default_context()
    t0 = time.perf_counter()
    A = tpg.pairwise_sqdist(tpg.FBM.synth(9, N16, M16, npop=10, miss=0.02), device=True)
    B = tpg.pairwise_sqdist(tpg.FBM.synth(10, N16, M16, npop=10, miss=0.02), device=True)  # a second matrix of that size, for the timing alone
    ctx.sync()
    emit(f"n = {N16} (TPG_MANTEL_MAX_N), {M16} loci: two squared-distance matrices of {8 * N16 * N16 / 2 ** 30:.1f} GiB each (beyond the "
         f"Infinity Cache; synthesis on the device, one pairwise pass of {N16 * N16 * M16:.2e} products and the epilogue each): "
         f"{(time.perf_counter() - t0) * 1e3:.0f} ms wall, ONE cold run; scratch bound of mantel_sums "
         f"{tpg.mantel_scratch_bytes(N16, 10 ** 9, 1) / 2 ** 20:.0f} MiB (Q = 1)")
    t0 = time.perf_counter()
    perms = tpg.mantel_perms(N16, 11, 0, R16)
    emit(f"  the {R16} permutations on the host: {(time.perf_counter() - t0) * 1e3:.0f} ms, ONE run")
    _sums_report(tpg, ctx, A, [B], perms, "Mantel")
    return 0


def main():
    steps = {"--n5000": step_n5000, "--n16384": step_n16384}
    if len(sys.argv) == 2 and sys.argv[1] in steps:
        return steps[sys.argv[1]]()
    os.makedirs("profiles", exist_ok=True)
    with open(OUT, "w") as f:
        f.write("tools/mantel_probe.py: Mantel cross sums under batches of permutations and gt_mantel on one MI355X, synthetic panels only\n")
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
