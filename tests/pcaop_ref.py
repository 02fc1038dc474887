"""Fixed-point model, exact route and derived bounds for the PCA operator halves (csrc/pcaop.hip, include/tpg.h "PCA by
operator products").

    zt:  W = Z'Q  (m x b)      W[j,c] = ( sum_i g_ij q~_ic  -  c_j sum_i q~_ic ) / s_j
    z:   Y = Z W  (n x b)      Y[i,c] =   sum_j g_ij w~'_jc  -  sum_j c_j w~'_jc ,     w'_jc = fl(W[j,c] / s_j)

with Z = (G - 1c')S^-1 and G the n x m dosages 0 / 1 / 2.

The model (model_zt, model_z) restates what the device does, step by step: ONE binary exponent per column c, ex_c with
amax_c = max |x_ic| < 2^ex_c (frexp), FU_c = 7 TU - 2 - ex_c fractional bits, x~ = rint(x 2^FU_c) (half to even) -- TU = 6
balanced base-128 digits hold it, digits() shows that --, the integer sums exact, the column sums of the correction term
taken of the ROUNDED operand, one rounding of the exact integer to FP64, then the FP64 expressions of the finalize kernels
in their stated order.  TU and per_column are arguments so that tests/test_pcaop_host.py can show that a model with one digit
fewer, or with one exponent for the whole block, leaves the bounds.

The exact route (exact_zt, exact_z) is integer arithmetic on the doubles' own bits (every double is an integer times a power
of two; the n x m integer contraction runs on 24-bit limbs in int64, the rest on Python integers) and rounds ONCE, correctly,
at the end.

The bounds (bound_zt, bound_z, bound_apply) are DERIVED; no constant in them is fitted to an observed error.  U = 2^-52 is
twice the unit roundoff u = 2^-53, which absorbs the (1 + u)^k factors of the few roundings that follow each other.

  zt.  |q~ - q| <= 2^-41 2^ex_c <= 2^-40 amax_c per entry and |g - c_j| <= 2, so the integer part is off by at most
       2 n 2^-40 amax_c, and W by that over s_j: the LEADING term.  FP64: gu = fl(exact integer) 2^-FU (u |gu|),
       qsum = fl(exact sum) (u |qsum|), p = fl(c_j qsum) (so p is within 2u |p|), d = fl(gu - p), W = fl(d / s_j) (each
       u |W|).  Together  ( U (|gu| + 2 |p|) ) / s_j + 3 U |W|.
  z.   The same with m terms: 2 m 2^-40 amax_c, amax_c of w'.  w' itself is fl(W / s): u |w'| per entry, 2 m u amax_c in the
       sum.  FP64: gu as above; csum_c = sum_j fl(c_j w~'_jc) by 256 * 64 strided partial sums of ceil(m / 16384) terms
       each, an 8-level pairwise tree inside a workgroup and a 6-level one over the 64 workgroups: at most
       ceil(m / 16384) + 14 additions and one product rounding on any path, (ceil(m / 16384) + 15) u sum_j |c_j w~'_jc|;
       Y = fl(gu - csum): u |Y|.
  apply.  Z (Z'Q) by the two halves against numpy's FP64 Z @ (Z.T @ Q): the z bound at the W that went in, the zt bound carried
       through |Z|, and numpy's own rounding, (n + m + 4) U |Z| (|Z'| |Q|) for two products of inner lengths n and m.
"""
import numpy as np

TU = 6
BMAX = 64
U = 2.0 ** -52
SHAPES = ((33, 130), (128, 128), (129, 257), (200, 1000))  # partial row tiles; one and two chunks; chunk edges
BS = (1, 5, 6, 22, 64)  # 6, 30, 36, 132, 384 int8 columns: inside a tile, two tiles, a 4 + 1 launch split, three full launches
KINDS = ("normal", "two_mag", "zero_col", "neg_col")


# ---------------------------------------------------------------------------------------------------------------------
# inputs
def panel(seed, n, m, npop=3):
    """the panels of the tests: orc.synth_fbm(..., miss=0.0), monomorphic loci dropped -> (G int64 n x m', kept columns)"""
    from oracle import oracle as orc

    fbm = orc.synth_fbm(seed, n, m, npop=npop, miss=0.0)
    keep = np.where((fbm.sum(axis=0) > 0) & (fbm.sum(axis=0) < 2 * n))[0]
    return fbm[:, keep].astype(np.int64), keep


def center_scale(G):
    """bigsnpr::snp_scaleBinom from the counts, as tpg_pca_center_scale computes it"""
    n = G.shape[0]
    mean = G.sum(axis=0).astype(np.float64) / float(n)
    p = mean / 2
    return mean, np.sqrt(2 * p * (1 - p))


def operand(kind, rows, b, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rows, b))
    if kind == "two_mag":  # columns of magnitude 1 and 1e-7 side by side: what a common exponent cannot hold
        X[:, 1::2] *= 1e-7
        if b == 1:
            X *= 1e-7
    elif kind == "zero_col":
        X[:, b // 2] = 0.0
    elif kind == "neg_col":
        X[:, 0] = -np.abs(X[:, 0]) - 0.25
    else:
        assert kind == "normal"
    return np.asfortranarray(X)


# ---------------------------------------------------------------------------------------------------------------------
# the fixed-point model
def exponents(X, tu=TU, per_column=True):
    """amax[c], FU[c] of an operand block (a zero column: FU 0)"""
    amax = np.abs(X).max(axis=0)
    ref = amax if per_column else np.full_like(amax, amax.max())
    _, ex = np.frexp(ref)  # ref = mant 2^ex, mant in [1/2, 1)
    FU = np.where(ref > 0, 7 * tu - 2 - ex, 0).astype(np.int64)
    return amax, FU


def fixed(X, FU):
    """rint(x 2^FU_c), int64 (|.| <= 2^(7 TU - 2))"""
    return np.rint(np.ldexp(X, FU[None, :].astype(np.int32))).astype(np.int64)


def digits(Wint, tu=TU):
    """the balanced base-128 digits (tu, ...) of the fixed-point integers, each in [-64, 63]; sum_t d_t 128^t == Wint"""
    W = Wint.astype(np.int64).copy()
    out = []
    for _ in range(tu):
        d = W & 127
        d = np.where(d >= 64, d - 128, d)
        out.append(d)
        W = (W - d) >> 7
    assert np.all(W == 0), "the fixed-point integer does not fit its digits"
    return np.stack(out)


def _gu(S, FU):
    # the exact integer (|S| < 2^63 at the tests' sizes: int64 holds it), rounded once, times 2^-FU
    return np.ldexp(S.astype(np.float64), (-FU[None, :]).astype(np.int32))


def model_zt(G, center, scale, Q, tu=TU, per_column=True, parts=False):
    amax, FU = exponents(Q, tu, per_column)
    Qi = fixed(Q, FU)
    for c in range(Q.shape[1]):
        if amax[c] > 0:
            digits(Qi[:, c], tu)
    gu = _gu(G.T @ Qi, FU)
    qsum = np.ldexp(Qi.sum(axis=0).astype(np.float64), (-FU).astype(np.int32))
    p = center[:, None] * qsum[None, :]
    W = (gu - p) / scale[:, None]
    W[:, amax == 0] = 0.0
    return (W, gu, p, amax) if parts else W


NG = 64  # OP_NG of csrc/pcaop.hip: workgroups per column in the correction sums


def _csum(center, wt):
    """sum_j fl(center_j wt_jc) in the order of tpg_pcaop_colsum_kernel / tpg_pcaop_colsum2_kernel: thread t of workgroup g adds
    j = 256 g + t, + 256 NG, ... ascending; the 256 sums of a workgroup pairwise (t with t + 128, t + 64, ...); then the NG
    workgroups' sums pairwise (g with g + 32, ...)"""
    m, b = wt.shape
    prod = center[:, None] * wt
    T = 256 * NG
    rows = -(-m // T)
    pad = np.zeros((rows * T, b))
    pad[:m] = prod
    acc = np.zeros((T, b))
    for r in range(rows):
        acc = acc + pad[T * r:T * (r + 1)]
    acc = acc.reshape(NG, 256, b)
    w = 128
    while w > 0:
        acc[:, :w] = acc[:, :w] + acc[:, w:2 * w]
        w >>= 1
    acc = acc[:, 0].copy()
    w = NG // 2
    while w > 0:
        acc[:w] = acc[:w] + acc[w:2 * w]
        w >>= 1
    return acc[0]


def model_z(G, center, scale, W, tu=TU, per_column=True, parts=False):
    Wp = W / scale[:, None]
    amax, FU = exponents(Wp, tu, per_column)
    Wi = fixed(Wp, FU)
    for c in range(W.shape[1]):
        if amax[c] > 0:
            digits(Wi[:, c], tu)
    gu = _gu(G @ Wi, FU)
    wt = np.ldexp(Wi.astype(np.float64), (-FU[None, :]).astype(np.int32))
    csum = _csum(center, wt)
    Y = gu - csum[None, :]
    Y[:, amax == 0] = 0.0
    cabs = (np.abs(center)[:, None] * np.abs(wt)).sum(axis=0)
    return (Y, gu, cabs, amax) if parts else Y


# ---------------------------------------------------------------------------------------------------------------------
# the exact route
def _as_int(X):
    """X (float64 array) = I 2^e with I an object array of Python integers and one e for the whole array"""
    mant, ex = np.frexp(X)
    M = np.ldexp(mant, 53).astype(np.int64)  # exact: 53-bit integers
    e = ex.astype(np.int64) - 53
    nz = M != 0
    emin = int(e[nz].min()) if nz.any() else 0
    sh = np.where(nz, e - emin, 0)
    I = np.array([int(a) << int(s) for a, s in zip(M.ravel(), sh.ravel())], dtype=object).reshape(X.shape)
    return I, emin


def _int_matmul(A, I):
    """A (int64, small entries) @ I (object integers), exact: 24-bit limbs of |I| with its sign, int64 products, recombined"""
    sign = np.array([(x > 0) - (x < 0) for x in I.ravel()], dtype=np.int64).reshape(I.shape)
    mag = np.array([abs(x) for x in I.ravel()], dtype=object).reshape(I.shape)
    bits = max((int(x).bit_length() for x in mag.ravel()), default=1)
    out = np.zeros((A.shape[0], I.shape[1]), dtype=object)
    for l in range(-(-max(bits, 1) // 24)):
        limb = np.array([(int(x) >> (24 * l)) & 0xFFFFFF for x in mag.ravel()], dtype=np.int64).reshape(I.shape) * sign
        out = out + (A @ limb).astype(object) * (1 << (24 * l))
    return out


def _ldexp_obj(F, e):
    return np.ldexp(np.array(F, dtype=np.float64), np.asarray(e, dtype=np.int64).astype(np.int32))


def exact_zt(G, center, scale, Q):
    """(sum_i (g_ij - c_j) q_ic) / s_j, exact, rounded once"""
    Qi, eq = _as_int(Q)
    Ci, ec = _as_int(center)
    A = _int_matmul(G.T.copy(), Qi)                     # m x b, times 2^eq
    B = Qi.sum(axis=0)                                  # b,     times 2^eq
    sh = max(-ec, 0)
    N = A * (1 << sh) - (Ci[:, None] * B[None, :]) * (1 << max(ec, 0))  # times 2^(eq + min(ec, 0))
    smant, sex = np.frexp(scale)
    Si = np.array([int(x) for x in np.ldexp(smant, 53).astype(np.int64)], dtype=object)
    quo = np.array([[n_ / s_ for n_ in row] for row, s_ in zip(N, Si)], dtype=np.float64)  # int / int: correctly rounded
    return _ldexp_obj(quo, (eq + min(ec, 0)) - (sex.astype(np.int64) - 53)[:, None])


def exact_z(G, center, scale, W):
    """sum_j (g_ij - c_j) w'_jc with w' = fl(W / s) (the operand the device rounds), exact, rounded once"""
    Wp = W / scale[:, None]
    Wi, ew = _as_int(Wp)
    Ci, ec = _as_int(center)
    A = _int_matmul(G, Wi)                              # n x b, times 2^ew
    D = (Ci[:, None] * Wi).sum(axis=0)                  # b,     times 2^(ew + ec)
    N = A * (1 << max(-ec, 0)) - D[None, :] * (1 << max(ec, 0))
    F = np.array([[float(x) for x in row] for row in N], dtype=np.float64)  # float(int): correctly rounded
    return _ldexp_obj(F, ew + min(ec, 0))


# ---------------------------------------------------------------------------------------------------------------------
# the bounds
def bound_zt(G, center, scale, Q, tu=TU):
    n = G.shape[0]
    W, gu, p, amax = model_zt(G, center, scale, Q, parts=True)
    lead = 2.0 * n * 2.0 ** -(7 * tu - 2) * amax[None, :]
    return (lead + U * (np.abs(gu) + 2 * np.abs(p))) / scale[:, None] + 3 * U * np.abs(W)


def bound_z(G, center, scale, W, tu=TU):
    m = G.shape[1]
    Y, gu, cabs, amax = model_z(G, center, scale, W, parts=True)
    lead = 2.0 * m * (2.0 ** -(7 * tu - 2) + U) * amax[None, :]
    return lead + U * (np.abs(gu) + (-(-m // (256 * NG)) + 15) * cabs[None, :]) + 2 * U * np.abs(Y)


def scaled(G, center, scale):
    return (G.astype(np.float64) - center[None, :]) / scale[None, :]


def bound_apply(G, center, scale, Q, W=None):
    """elementwise bound on | z(zt(Q)) - Z @ (Z.T @ Q) |, the reference in numpy FP64; W: what zt returned (default: the model's)"""
    n, m = G.shape
    if W is None:
        W = model_zt(G, center, scale, Q)
    Za = np.abs(scaled(G, center, scale))
    return bound_z(G, center, scale, W) + Za @ bound_zt(G, center, scale, Q) + (n + m + 4) * U * (Za @ (Za.T @ np.abs(Q)))


def op_error_norm(G, center, scale, u):
    """E of the SVD tests: the 2-norm of bound_apply for one vector u"""
    return float(np.linalg.norm(bound_apply(G, center, scale, np.asfortranarray(u.reshape(-1, 1)))))
