#!/usr/bin/env python3
"""PCA by operator products (include/tpg.h) at the sizes it is for.  For the record: no figure here is a pass criterion.

  halves N M     the two int8 halves W = Z'Q, Y = Z W on a synthetic N x M panel with the operands in device memory: HIP-event
                 time of every kernel (the smallest of three calls) and the wall time of a half at b = 12, 32, 64; beside them
                 at b = 32 the same two products by the FP64 sweeps (tpg_sweep_loci_rowscale -- internal, reached by its
                 C++ symbol -- and tpg_fbm256_prod_and_rowSumsSq), and the operator's relative error against those sweeps,
                 |(A_mfma - A_fp64) q|_F / |A_fp64 q|_F for A = Z Z' and 32 random columns q, from which the floor of tol is read:
                 100 times it, rounded up to a power of ten, not below 1e-8.
  route R N M K  gt_pca_randomSVD(route = R, tol = 1e-4) on a synthetic N x M panel: wall time of a cold and of a warm call (each
                 packs its view), n_apply, the growth of the device memory in use over the cold call (hipMemGetInfo; the pool
                 keeps what a call allocated) and the leading singular values.

Every leg runs in a process of its own under its own time limit, and nothing is started after a leg that failed.

    python tools/pcaop_probe.py [plan]     plan = default | small; writes profiles/pcaop_probe.txt"""
import ctypes as C
import math
import os
import subprocess
import sys
import time

sys.path.insert(0, ".")

LIMIT_S = 360
OUT = os.path.join("profiles", "pcaop_probe.txt")
PLANS = {
    # the benchmark's panel; a tall panel for both routes (8 n^2 = 12.8 GB); the tall panel of the issue for the operator route
    # alone: its Gram matrix would take 80 GB of a shared device
    "default": [("halves", 5000, 1000000), ("route", "operator", 5000, 1000000, 20), ("route", "gram", 5000, 1000000, 20),
                ("halves", 100000, 100000), ("route", "operator", 40000, 100000, 20), ("route", "gram", 40000, 100000, 20),
                ("route", "operator", 100000, 100000, 20)],
    "small": [("halves", 600, 20000), ("route", "operator", 600, 20000, 8), ("route", "gram", 600, 20000, 8)],
}
ROWSCALE = "_Z23tpg_sweep_loci_rowscaleP7tpg_ctxPK8tpg_viewPKdS5_S5_iPd"


def _used(hip):
    fr, tot = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
    return tot.value - fr.value


def _panel(tpg, n, m):
    import numpy as np

    X = tpg.FBM.synth(3, n, m, npop=51, imputed_bytes=True)
    return X, np.ascontiguousarray(tpg.CODE_IMPUTE_PRED)


def halves(n, m):
    import numpy as np
    import torch

    import tidypopgen_amd as tpg
    from tidypopgen_amd.api import check, lib

    ctx = tpg.default_context()
    X, code = _panel(tpg, n, m)
    v = tpg.View(X, None, None, code256=code)
    center, scale = tpg.pca_center_scale(v)
    dev = torch.device("cuda")
    f64 = torch.float64
    d_center, d_scale = torch.as_tensor(center, device=dev), torch.as_tensor(scale, device=dev)
    d_inv = 1.0 / d_scale
    gen = torch.Generator(device=dev).manual_seed(1)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def zt(Q, W):
        check(lib.tpg_pca_zt_prod(ctx.h, v.h, p(d_center), p(d_scale), p(Q), Q.shape[0], p(W)))

    def z(W, Y):
        check(lib.tpg_pca_z_prod(ctx.h, v.h, p(d_center), p(d_scale), p(W), W.shape[0], p(Y)))

    def timed(fn, reps=3):
        best, wall = {}, math.inf
        for _ in range(reps):
            ctx.prof_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            wall = min(wall, (time.perf_counter() - t0) * 1e3)
            for name, (cnt, ms) in ctx.prof_dump().items():
                best[name] = (cnt, min(best.get(name, (0, math.inf))[1], ms))
        return wall, best

    def show(best, prefix):
        return ", ".join(f"{k} {ms:.3f} ms x{cnt}" for k, (cnt, ms) in sorted(best.items()) if k.startswith(prefix))

    _say(f"panel {n} x {m}, synthetic, 51 populations; operands in device memory (column-major: a tensor of b rows of length n or m); "
          f"kernel times are HIP-event times, the smallest of three calls; wall = the call, synchronised")
    ctx.prof_enable(True)
    keep = {}
    for b in (12, 32, 64):
        Q = torch.randn((b, n), generator=gen, device=dev, dtype=f64)   # row c = column c of the n x b block
        W = torch.empty((b, m), device=dev, dtype=f64)
        Y = torch.empty((b, n), device=dev, dtype=f64)
        torch.cuda.synchronize()
        zt(Q, W)
        z(W, Y)  # warm-up: code objects, the pool, the view's second layout
        wall_zt, k_zt = timed(lambda: zt(Q, W))
        wall_z, k_z = timed(lambda: z(W, Y))
        _say(f"b = {b:2d}: zt wall {wall_zt:8.3f} ms  [{show(k_zt, 'pcaop_zt')}]")
        _say(f"        z  wall {wall_z:8.3f} ms  [{show(k_z, 'pcaop_z_')}]")
        if b == 32:
            keep = dict(Q=Q, W=W.clone(), Y=Y.clone())
    # the same products by the FP64 sweeps at b = 32
    b = 32
    Q, W_op, Y_op = keep["Q"], keep["W"], keep["Y"]
    W64 = torch.empty((b, m), device=dev, dtype=f64)
    Y64 = torch.empty((b, n), device=dev, dtype=f64)
    rss = torch.empty((n,), device=dev, dtype=f64)
    rowscale = getattr(lib, ROWSCALE, None)

    def z64(Win, Yout):
        check(lib.tpg_fbm256_prod_and_rowSumsSq(ctx.h, v.h, p(d_center), p(d_scale), p(Win), b, p(Yout), p(rss)))

    if rowscale is None:
        _say("tpg_sweep_loci_rowscale not found under its symbol: the FP64 side of zt is not measured")
        return 1
    rowscale.restype = C.c_int
    rowscale.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p]

    def zt64(Qin, Wout):
        check(rowscale(ctx.h, v.h, p(d_center), p(d_inv), p(Qin), b, p(Wout)))

    torch.cuda.synchronize()
    zt64(Q, W64)
    z64(W64, Y64)
    wall_zt64, k_zt64 = timed(lambda: zt64(Q, W64))
    wall_z64, k_z64 = timed(lambda: z64(W64, Y64))
    _say(f"FP64 sweeps, b = 32: Z'Q wall {wall_zt64:8.3f} ms  [{show(k_zt64, 'sweep_')}]")
    _say(f"                     Z W wall {wall_z64:8.3f} ms  [{show(k_z64, 'sweep_')}]")
    ctx.prof_enable(False)
    torch.cuda.synchronize()
    nrm = lambda t: float(torch.linalg.norm(t))  # noqa: E731
    e_zt = nrm(W_op - W64) / nrm(W64)
    Yx = torch.empty_like(Y64)
    z(W64, Yx)  # the z half alone, on the FP64 operand
    ctx.sync()
    e_z = nrm(Yx - Y64) / nrm(Y64)
    e_op = nrm(Y_op - Y64) / nrm(Y64)
    floor = max(1e-8, 10.0 ** math.ceil(math.log10(100.0 * e_op)))
    _say(f"relative error in norm against the FP64 sweeps, b = 32: Z'Q {e_zt:.3e}, Z W {e_z:.3e}, the operator Z (Z'q) {e_op:.3e}")
    _say(f"floor of tol: 100 x {e_op:.3e} rounded up to a power of ten, not below 1e-8 -> {floor:g} "
          f"(PCA_OP_TOL_FLOOR of the library: {tpg.PCA_OP_TOL_FLOOR:g})")
    return 0


def route(name, n, m, k):
    import numpy as np

    import tidypopgen_amd as tpg

    hip = C.CDLL("libamdhip64.so.7")
    ctx = tpg.default_context()
    X, code = _panel(tpg, n, m)
    ctx.sync()
    before = _used(hip)
    t0 = time.perf_counter()
    r = tpg.gt_pca_randomSVD(X, k=k, tol=1e-4, code256=code, route=name)
    ctx.sync()
    cold = time.perf_counter() - t0
    growth = _used(hip) - before
    t0 = time.perf_counter()
    r2 = tpg.gt_pca_randomSVD(X, k=k, tol=1e-4, code256=code, route=name)
    ctx.sync()
    warm = time.perf_counter() - t0
    same = all(r[key].tobytes() == r2[key].tobytes() for key in ("d", "u", "v"))
    extra = f"n_apply {r['n_apply']}, scratch by the header {tpg.pca_op_scratch_bytes(n, m, k) / 1e6:.0f} MB" if name == "operator" \
        else f"Gram matrix 8 n^2 = {8 * n * n / 1e6:.0f} MB"
    _say(f"route {name:8s} {n} x {m}, k = {k}, tol 1e-4: cold {cold * 1e3:9.1f} ms, warm {warm * 1e3:9.1f} ms, device growth "
          f"{growth / 1e6:9.1f} MB (view layouts included), {extra}; d[:4] = {np.array2string(r['d'][:4], precision=9)}; "
          f"{'same bits twice' if same else 'BITS DIFFER between the two calls'}")
    return 0


def _say(text):
    """to the output and to profiles/pcaop_probe.txt (the driver emptied it)"""
    print(text, flush=True)
    with open(OUT, "a") as f:
        f.write(text + "\n")


def main():
    if len(sys.argv) >= 2 and sys.argv[1] == "--leg":
        kind = sys.argv[2]
        if kind == "halves":
            return halves(int(sys.argv[3]), int(sys.argv[4]))
        return route(sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]))
    plan = PLANS[sys.argv[1] if len(sys.argv) > 1 else "default"]
    os.makedirs("profiles", exist_ok=True)
    open(OUT, "w").close()
    for leg in plan:
        args = [str(a) for a in leg]
        try:
            r = subprocess.run([sys.executable, __file__, "--leg"] + args, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            _say(f"{' '.join(args)}: no result within {LIMIT_S} s; stopping here")
            return 1
        if r.returncode != 0:  # nothing more is started on the GPU after a failure
            _say(f"{' '.join(args)}: exit status {r.returncode}; stopping here")
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
