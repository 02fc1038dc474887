"""Weights, launch plan, exact reference, derived bounds and a numpy model for the digit-split Gram route of csrc/pca.hip
(tpg_pca_digits_kernel, tpg_pca_gram_kernel<TD>, tpg_gram_locate / tpg_pca_assemble_kernel, the plan in pca_gram_device).

The route is integer arithmetic.  With w_j = 1.0 / (s_j * s_j), the weight of locus j is the integer
W_j = llrint(ldexp(w_j, F)), cut into T balanced base-128 digits (-64 .. 63); the kernel sums g_ij g_kj digit_t(W_j) in int32 per
digit on the int8 matrix cores, adds them shifted into int64 slabs, and the assemble kernel returns ldexp((double)S_ik, -F).  With
center = 0 the call therefore returns K0 = ldexp((double)S, -F), S = sum_j g_ij g_kj W_j, and nothing is rounded as long as
|S| < 2^53.  pca_gram takes any per-locus scale, so a test can PRESCRIBE W digit by digit (weights(), scale_of()), the launch
plan is restated for any CU count (plan()), exact_S() is the integer matrix, model() runs the device's order of work in numpy
and takes a fault=, and CASES is the table tests/test_gpu_gramdig.py runs on the device, every case asserting on the restated
plan the arm it was built for.  tests/test_gramdig_host.py shows on the CPU that the model equals exact_S() and that every
fault of FAULTS leaves it on the cases named for the fault.

Two limits of the arithmetic, besides the int64 overflow the overflow section deals with.  T digits of -64 .. 63 reach
63 (128^T - 1) / 127, which is 1 / 127 short of the 2^(7 T - 1) that F = 7 T - 1 - wbits lets the largest weight come to.  A
largest weight in the top 1 / 127 of its binade (w = 127; w = n + 1/2 of a singleton under the binomial scaling for
n = 4 064 .. 4 095) would lose the carry out of its top digit and come out 2^(7 T - F) too small.  pca_gram_device gives up one
fractional bit where F > 22 and adds a digit otherwise, up to eight (digit_plan() restates it; the cases "top_carry_*" sit there).  For the
same reason the issue's pattern W = 2^(7 T - 1) - 1 cannot arise (wbits = ceil(log2(wmax + 1)) keeps w <= 2^wbits - 1): the
largest weight a panel can hold is the all-63 pattern for wbits >= 7 and (2^wbits - 1) 2^F below, and those are used.

Bounds (u = 2^-53; every one derived here, none fitted)
* center = 0, |S_ik| < 2^53: K_ik == ldexp(S_ik, -F) in every bit (check_K0).
* center = 0, 2^53 <= |S_ik| < 2^62: within one unit in the last place of float(S_ik) 2^-F: the int64 -> double conversion
  rounds once and the contract does not say how.  Every T = 8 case is of this kind (a weight of 55 bits on the diagonal), and
  T = 7 "wide" is the one case the issue asks for.  No bit-for-bit case with |S| < 2^53 exists at T = 8.
* against the true weights (bound_true): |K_ik - sum_j g g / s_j^2| <= sum_j g_ij g_kj (2^-(F+1) + 3 u w_j) + u |K_ik|.
  W_j is w_j 2^F rounded to an integer: 2^-(F+1) per unit of g g.  w_j = fl(1 / fl(s s)) is within 2 u (1 + u) of 1 / s^2
  and the long-double reference is rounded to double for the comparison: 3 u w_j per term as the issue states it.  u |K| is
  the conversion of S where |S| >= 2^53 (zero below).
* center = the column mean (bound_mean): S' is exact, so gramcls_ref.bound_centred with rel = 0: n 2^-52 max |S'|, against
  the exact rational double centring of the integer S (centred_exact).  bound_centred derives the centring's own roundings
  as 49 u max |S'| for n <= 512 and states them as n 2^-52; for n < 25 that is smaller than derived, and the only such case
  here is n = 1, where K = ((S - S) - S) + S = 0 exactly.
* a general center (bound_general): K_ik = val - r_i - r_k + Cc with val = S'_ik exact, r_i the RAW sweep of
  wc_j = fl(what_j c_j) over the m loci and Cc the sum of fl(wc_j c_j) over 512 x 256 threads, a tree of 8 levels and 512
  partial sums in long double.  With A_i = sum_j what_j |c_j| g_ij and B = sum_j what_j c_j^2:
    |r^_i - r_i| <= (m + 8) u (1 + u) A_i + u A_i <= (m + 10) u A_i         (sweep_ref: (N + 8) u; wc's own rounding)
    |Cc^ - C|   <= (d + 12) u B,  d = ceil(m / 131072)                       (two roundings per product, d serial additions
                                                                            per thread, 8 tree levels, one long double -> double)
    the roundings of val - r_i - r_k + Cc (the issue counts four with val's conversion, exact here): each at most u of a
    partial sum no larger than M_ik = |val| + A_i + A_k + B: 4 u M_ik, the fourth covering the second-order terms
  bound_ik = (m + 10) u (A_i + A_k) + (d + 12) u B + 4 u M_ik, against sum_j what_j (g_ij - c_j)(g_kj - c_j) in long double
  (reference error m 2^-64 M_ik, counted in by the slack of (m + 10) over the first-order m + 9).

The overflow.  S_ik = sum_j g_ij g_kj W_j <= 4 sum_j W_j, so 4 sum_j W_j < 2^63 is sufficient for no sum and no partial sum
to wrap (terms are non-negative; the per-digit int64 adds of a slab are partial sums of a rearrangement with signed digits,
each bounded by the same 4 sum_j |digits| 128^t <= 4 * 128/127 sum W, which is why the cases keep a factor two of room and why
the library's guard is on 4 sum W rather than on the pair).  The library cannot see sum W before the digits exist; it has
sum_j w_j from the reduction that finds the smallest scale, and W_j <= 2^F w_j + 1/2: guard() restates
4 (2^F (1 + 2^-20) sum w + m / 2) < 2^63.  Outside it the class route runs whatever its cost model says (FP64 for any
weights), and where that is not available (TPG_GRAM_DIGITS, m >= 2^31 - 64) the call is refused with TPG_ENUMERIC.
OVERFLOW_CASES are the two panels of the issue and one whose largest weight would need a ninth digit (T = 8, F = 22, the
top 1 / 127: the same fall-back); for their single weight class the mixed fold's deviation term is zero, so
its full fold rounds exactly as the FP64 fold does and gramcls_ref.rel_fold64 is the bound of either kernel.
"""
import math

import numpy as np

from tests.gramcls_ref import LD, bound_centred, centre  # noqa: F401  (centre: re-exported for the tests)

FBITS = 22
U = 2.0 ** -53
PCA_TB = 4
OOB = -(2 ** 62) - 12345  # what the model returns where a faulty index leaves the slabs


# ---------------------------------------------------------------------------------------------------------------------
# weights
def top_of(T):
    """largest value T balanced digits hold"""
    return 63 * (128 ** T - 1) // 127


def digit_plan(scale):
    """(wbits, T, F) as pca_gram_device takes them from the smallest scale, for pca_digit_fbits = 22"""
    smin = float(np.min(scale))
    wmax = 1.0 / (smin * smin)
    lg = math.log2(wmax + 1.0)
    assert lg == round(lg) or abs(lg - round(lg)) > 1e-9  # (no case sits where two libm's could disagree on the ceiling)
    wbits = int(math.ceil(lg))
    T = max(4, (wbits + FBITS + 1 + 6) // 7)
    F = 7 * T - 1 - wbits
    assert T <= 8
    if int(np.rint(np.ldexp(wmax, F))) > top_of(T):
        if F > 22:
            F -= 1
        else:
            T += 1  # (T = 9: no such kernel; the library takes the class route, as outside the overflow guard)
    return wbits, T, F


def weights(scale, F):
    """W_j = llrint(ldexp(1.0 / (s_j * s_j), F)) as int64 (at most 55 bits)"""
    scale = np.asarray(scale, dtype=np.float64)
    return np.rint(np.ldexp(1.0 / (scale * scale), F)).astype(np.int64)


def digits(W, T, fault=None):
    """(T, m) balanced digits as tpg_pca_digits_kernel cuts them, and what is left of W after T digits (0 if it fits)"""
    W = np.array(W, dtype=np.int64)
    out = np.zeros((T, len(W)), dtype=np.int64)
    for t in range(T):
        dig = W & 127
        neg = dig >= 64
        dig = np.where(neg, dig - 128, dig)
        W = (W >> 7) if fault == "borrow_lost" else ((W - dig) >> 7)
        out[t] = dig
    if fault == "digit0_dropped":
        out[0] = 0
    return out, W


def passes(T):
    """[(t0, td)]: 4 + (T - 4)"""
    return [(t0, min(4, T - t0)) for t0 in range(0, T, 4)]


def from_digits(ds):
    return sum(int(d) * 128 ** t for t, d in enumerate(ds))


def scale_of(W, F):
    """a scale whose restated weight is W, checked with 1 / s^2 moved by up to 4 units in the last place either way"""
    W = np.asarray(W, dtype=np.int64)
    assert W.min() >= 1 and W.max() < 2 ** 50
    s = np.sqrt(np.ldexp(1.0, F) / W.astype(np.float64))
    w = 1.0 / (s * s)
    lo, hi = w.copy(), w.copy()
    for _ in range(4):
        lo, hi = np.nextafter(lo, 0.0), np.nextafter(hi, np.inf)
    for x in (lo, w, hi):
        assert np.array_equal(np.rint(np.ldexp(x, F)).astype(np.int64), W)
    return s


def guard(scale, F):
    """pca_gram_device's overflow guard: True = the digit route may run"""
    scale = np.asarray(scale, dtype=np.float64)
    wsum = float(np.sum(1.0 / (scale * scale)))
    return 4.0 * (math.ldexp(wsum * (1.0 + 2.0 ** -20), F) + 0.5 * len(scale)) < 2.0 ** 63


def safe(W):
    """the sufficient condition itself, in integers"""
    return 4 * sum(int(x) for x in W) < 2 ** 63


# ---------------------------------------------------------------------------------------------------------------------
# exact reference
def exact_S(g, W, wide=False):
    """sum_j g_ij g_kj W_j.  W in pieces of 26 bits, each piece's matrix by float64 BLAS (entries below 4 m 2^26 < 2^53 for
    m < 2^25: exact in any order), recombined in int64 -- or in Python integers (object array) with wide=True, for the
    panels whose sums pass 2^63."""
    g = np.asarray(g)
    m = g.shape[1]
    assert m < 2 ** 25 and g.max() <= 2
    gf = g.astype(np.float64)
    Wi = np.asarray(W, dtype=np.int64)
    assert Wi.min() >= 0
    S = None
    for p in range(3):
        piece = (Wi >> (26 * p)) & ((1 << 26) - 1)
        if not piece.any():
            continue
        P = (gf * piece.astype(np.float64)[None, :]) @ gf.T
        assert P.max() < 2.0 ** 53
        P = P.astype(np.int64)
        if wide:
            P = P.astype(object) * (1 << (26 * p))
        else:
            assert P.max() < 2 ** (62 - 26 * p)
            P = P << (26 * p)
        S = P if S is None else S + P
    if S is None:
        S = np.zeros((g.shape[0], g.shape[0]), dtype=np.int64)
    if not wide:
        assert S.min() >= 0  # nothing wrapped on the way
    return S


def exact_K0(S, F):
    return np.ldexp(np.asarray(S, dtype=np.int64).astype(np.float64), -F)


def check_K0(K, S, F):
    """(ok, n_exact, n_wide): bit equality where |S| < 2^53, one unit in the last place of float(S) 2^-F above"""
    ref = exact_K0(S, F)
    small = np.abs(S) < 2 ** 53
    ok = np.array_equal(K[small], ref[small])
    wide = ~small
    if wide.any():
        ok = ok and bool(np.all(np.abs(K[wide] - ref[wide]) <= np.spacing(ref[wide])))
    return ok, int(small.sum()), int(wide.sum())


def _ld_of_ints(N):
    """object array of Python integers below 2^93 -> long double, one rounding"""
    hi = (N >> 40).astype(np.float64)
    lo = (N & ((1 << 40) - 1)).astype(np.float64)
    return hi.astype(LD) * LD(2.0 ** 40) + lo.astype(LD)


def centred_exact(S, F):
    """H S H 2^-F, H = I - 11'/n, from the integer n^2 S_ik - n rowsum_i - n rowsum_k + total, rounded once to long double"""
    So = np.asarray(S).astype(object)
    n = So.shape[0]
    rows = So.sum(axis=1)
    N = So * (n * n) - (rows * n)[:, None] - (rows * n)[None, :] + rows.sum()
    return _ld_of_ints(N) / LD(n * n) * LD(2.0 ** -F)


def true_K0(g, scale):
    """sum_j g_ij g_kj w_j with w_j = 1 / s_j^2 in long double (s_j^2 and the quotient both long double)"""
    s = np.asarray(scale, dtype=np.float64).astype(LD)
    w = LD(1) / (s * s)
    gl = np.asarray(g).astype(LD)
    return (gl * w[None, :]) @ gl.T


def bound_true(g, scale, F, K):
    s = np.asarray(scale, dtype=np.float64)
    w = 1.0 / (s * s)
    gf = np.asarray(g).astype(np.float64)
    gg = gf @ gf.T
    return (2.0 ** -(F + 1) * gg + 3 * U * ((gf * w[None, :]) @ gf.T)) * (1 + 2.0 ** -40) + U * np.abs(K)


def bound_mean(S, F, n):
    return bound_centred(0.0, exact_K0(S, F), n)


def asym_mean(S, F):
    """bound of |K_ik - K_ki| for center = the column mean: both are ((S'_ik - a) - b) + C of the SAME device values r^_i, r^_k,
    C^ with a, b in the two orders; each is three roundings of partial sums no larger than |S'_ik| + |r^_i| + |r^_k| + |C^|
    <= 4 max |S'| (1 + n u) away from the exact combination, so the two differ by at most 6 u * 4 max |S'| (1 + 2^-30)"""
    return 24 * U * float(np.abs(exact_K0(S, F)).max()) * (1 + 2.0 ** -30)


def asym_general(g, W, F, center, S):
    """the same for a general center, elementwise: 6 u M_ik (1 + 2^-30), M_ik of bound_general (|r^_i| <= A_i (1 + (m + 10) u))"""
    what = np.ldexp(np.asarray(W, dtype=np.float64), -F)
    c = np.asarray(center, dtype=np.float64)
    A = np.asarray(g).astype(np.float64) @ (what * np.abs(c))
    M = np.abs(exact_K0(S, F)) + A[:, None] + A[None, :] + float(np.sum(what * c * c))
    return 6 * U * M * (1 + 2.0 ** -30)


def general_exact(g, W, F, center):
    what = np.ldexp(np.asarray(W, dtype=np.float64), -F).astype(LD)
    z = np.asarray(g).astype(LD) - np.asarray(center, dtype=np.float64).astype(LD)[None, :]
    return (z * what[None, :]) @ z.T


def bound_general(g, W, F, center, S):
    what = np.ldexp(np.asarray(W, dtype=np.float64), -F)
    c = np.asarray(center, dtype=np.float64)
    m = len(c)
    A = np.asarray(g).astype(np.float64) @ (what * np.abs(c))
    B = float(np.sum(what * c * c))
    d = -(-m // 131072)
    M = np.abs(exact_K0(S, F)) + A[:, None] + A[None, :] + B
    return ((m + 10) * U * (A[:, None] + A[None, :]) + (d + 12) * U * B + 4 * U * M) * (1 + 2.0 ** -40)


# ---------------------------------------------------------------------------------------------------------------------
# launch plan
class Plan:
    pass


def plan(n, m, num_cu=256, fault=None):
    """pca_gram_device's units, their order and lut, the K split of the cost model and its ranges"""
    p = Plan()
    p.n, p.m, p.KG = n, m, -(-m // 128)
    p.Q = -(-n // 128)
    p.nrt = 4 * p.Q
    p.nrtv = -(-n // 32)
    p.nsbf = p.nrtv // PCA_TB
    p.rem = p.nrtv - PCA_TB * p.nsbf
    order, p.patches = [], 0
    for pj in range(-(-p.nsbf // 8)):
        j1 = min(p.nsbf, pj * 8 + 8)
        p.patches += 1
        for a in range(j1):
            for jb in range(max(pj * 8, a), j1):
                for r in range(PCA_TB):
                    if fault == "patch2_first_missing" and pj == 1 and a == 0 and jb == 8 and r == 0:
                        continue
                    order.append((PCA_TB * a + r, jb))
    if p.rem > 0:
        for jb in range(p.nsbf + 1):
            for r in range(p.rem):
                order.append((PCA_TB * p.nsbf + r, jb))
    p.order = order
    p.nun = len(order)
    p.lut = np.full((p.nrt, p.nsbf + 1), -1, dtype=np.int64)
    for u, (ia, jb) in enumerate(order):
        p.lut[ia, jb] = u
    nblk = max(num_cu // 8 * 8, 8)
    p.waves = 4 * nblk
    maxS = min(p.KG // 8, 96) if p.KG // 8 > 0 else 1
    best, bestS = -1.0, 1
    for S in range(1, maxS + 1):
        rounds = -(-p.nun * S // p.waves)
        cost = float(rounds) * (float(-(-p.KG // S)) * 1.17 + 65.0)
        if best < 0 or cost < best * 0.995:
            best, bestS = cost, S
    p.S = bestS
    p.ranges = [(p.KG * ks // p.S, p.KG * (ks + 1) // p.S) for ks in range(p.S)]
    return p


def longest_range_loci(n, m, num_cu=256):
    p = plan(n, m, num_cu)
    return 128 * max(k1 - k0 for k0, k1 in p.ranges)


def locate(nsbf, i, k, fault=None):
    """tpg_gram_locate on index arrays: (ia, jb, tb, row, col)"""
    i, k = np.array(i, dtype=np.int64), np.array(k, dtype=np.int64)
    F4 = 4 * nsbf
    ti, tk = i >> 5, k >> 5
    full = (ti < F4) & (tk < F4)
    corner = (ti >= F4) & (tk >= F4)
    swap = np.where(full, (tk >> 2) < (ti >> 2), np.where(corner, False, ti < F4))
    i, k = np.where(swap, k, i), np.where(swap, i, k)
    ti, tk = i >> 5, k >> 5
    ia = ti
    jb = np.where(corner, nsbf, tk >> 2)
    tb = np.where(corner, tk - F4, tk & 3)
    if fault == "corner_tb_no_F4":
        tb = np.where(corner, tk, tb)
    if fault == "rem_full_next_slab":
        jb = np.where(~full & ~corner, jb + 1, jb)
    return ia, jb, tb, i & 31, k & 31


# ---------------------------------------------------------------------------------------------------------------------
# the model
FAULTS = ("digit0_dropped", "borrow_lost", "planes_swapped", "pass2_shift", "pass2_base0", "last_group_dropped",
          "dead_unmasked", "dead1_kg", "boundary_up", "rem_full_next_slab", "corner_tb_no_F4", "patch2_first_missing",
          "pad_loci_digits")


def misread_pass2(D, td):
    """the td digit planes a second pass finds at the START of the digit table (pass_base = 0), which the first pass laid out
    with 4 digits per 16-locus slot: chunk c = slot * td + t of its own stride is digit c % 4 of slot c // 4 there"""
    mpad = D.shape[1]
    Dp = np.zeros((td, mpad), dtype=np.int64)
    for t in range(td):
        c = (np.arange(mpad) // 16) * td + t
        Dp[t] = D[c % 4, (c // 4) * 16 + np.arange(mpad) % 16]
    return Dp


def _i32(x):
    assert np.abs(x).max(initial=0.0) < 2.0 ** 31  # the kernel's accumulators are int32
    return x.astype(np.int64)


def model(g, W, T, num_cu=256, fault=None):
    """S as the device forms it: per K range and pass, the int32 sums of every digit over the range's loci (A side: the
    digit plane D for dosage 1, 2 D for dosage 2, zero for the padding code 3; B side: the code itself), shifted by 7 t
    inside the pass and by 7 t0 for the pass, added into the int64 slab of every unit [tb][row][col] (wrapping, as int64
    does), then read back through locate() and the lut.  Individuals past n and loci past m carry code 3; the digits of a
    locus past m are zero.  Returns the n x n int64 matrix, OOB where a faulty index points outside the slabs."""
    assert fault is None or fault in FAULTS
    g = np.asarray(g)
    n, m = g.shape
    p = plan(n, m, num_cu, fault)
    KG, npad, mpad = p.KG, 128 * p.Q, 128 * p.KG
    code = np.full((npad, mpad), 3, dtype=np.int64)
    code[:n, :m] = g
    dg, left = digits(W, T, fault)
    assert fault == "borrow_lost" or not left.any()
    D = np.zeros((T, mpad), dtype=np.int64)
    D[:, :m] = dg
    if fault == "pad_loci_digits":
        D[:, m:] = dg[:, m - 1:m]
    # A-side byte for (code, digit): v_perm picks D, 2 D or the constant 0
    one, two = (2, 1) if fault == "planes_swapped" else (1, 2)
    amul = np.zeros(4, dtype=np.int64)
    amul[1], amul[2] = one, two
    Amul = amul[code].astype(np.float64)
    Bf = code.astype(np.float64)
    slabs = np.zeros((p.nun, PCA_TB, 32, 32), dtype=np.int64)
    for pi, (t0, td) in enumerate(passes(T)):
        if pi == 1 and fault == "pass2_base0":
            # the second pass reads from the start of the table, which the first pass laid out with 4 digits per 16-locus
            # slot: chunk c = slot * td + t of its own stride is digit c % 4 of slot c // 4 there
            Dp = misread_pass2(D, td)
        else:
            Dp = D[t0:t0 + td]
        shift0 = 7 * (t0 - 1) if (pi == 1 and fault == "pass2_shift") else 7 * t0
        for ks, (k0, k1) in enumerate(p.ranges):
            if fault == "boundary_up" and ks + 1 < p.S:
                k1 = -(-KG * (ks + 1) // p.S)  # this range's end rounded up, the next one's start as it was
            if k0 >= k1:
                continue
            loci = [np.arange(128 * k0, 128 * (k1 - (1 if fault == "last_group_dropped" else 0)))]
            ndead = (-(k1 - k0)) % 3
            if fault == "dead_unmasked":  # steps 1 .. 3 of every dead group run on the clamped prefetch: the last group again
                loci += [np.arange(128 * (k1 - 1) + 32, 128 * k1)] * ndead
            if fault == "dead1_kg" and ndead:  # step 0 of the first dead group, decoded inside the last live one
                loci.append(np.arange(128 * (k1 - 1), 128 * (k1 - 1) + 32))
            jj = np.concatenate(loci)
            if len(jj) == 0:
                continue
            c = np.zeros((npad, npad), dtype=np.int64)
            for t in range(td):
                At = Amul[:, jj] * Dp[t, jj].astype(np.float64)[None, :]
                c += _i32(At @ Bf[:, jj].T) << (7 * t)
            c = c << shift0
            for u, (ia, jb) in enumerate(p.order):
                for tb in range(PCA_TB):
                    tile = PCA_TB * jb + tb
                    slabs[u, tb] += c[32 * ia:32 * ia + 32, 32 * tile:32 * tile + 32]
    ii, kk = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    ia, jb, tb, row, col = locate(p.nsbf, ii, kk, fault)
    u = np.where(jb <= p.nsbf, p.lut[ia, np.minimum(jb, p.nsbf)], -1)
    flat = ((u * PCA_TB + tb) * 32 + row) * 32 + col
    inside = (u >= 0) & (flat >= 0) & (flat < slabs.size)
    out = np.where(inside, slabs.reshape(-1)[np.where(inside, flat, 0)], OOB)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# panels
def dense_panel(n, m, seed):
    """dosages 0 / 1 / 2 at allele frequency one half, no missing value"""
    bits = np.random.default_rng(seed).integers(0, 4, size=(n, m), dtype=np.uint8)
    return np.asfortranarray((bits & 1) + (bits >> 1))


def tile_pairs(n):
    """one pair of individuals per (row tile, row tile) block, the diagonal blocks and the corner included, at a position
    inside the block that changes from block to block"""
    nt = -(-n // 32)
    out = []
    for ta in range(nt):
        for tb in range(ta, nt):
            q = len(out)
            a = min(32 * ta + (5 * q + 3) % 32, n - 1)
            b = min(32 * tb + (11 * q + 7) % 32, n - 1)
            out.append((a, b))
    return out


def pair_panel(n, m):
    """locus j is non-zero for the individuals of its pairs only.  The pairs: tile_pairs(n), then all pairs (a <= b) in a
    strided order, until there are at least m and every locus has one; pair q goes to locus q % m with dosages
    1 + q % 2 and 1 + (q // 2) % 2 (a pair (a, a) takes the first).  Returns (g, pairs)."""
    pairs = tile_pairs(n)
    total = n * (n + 1) // 2
    stride = next(s for s in range(max(2, int(0.38 * total)), total + 2) if math.gcd(s, total) == 1) if total > 1 else 1
    q = 0
    while len(pairs) < m:
        r = (q * stride) % total
        # r-th pair of the triangle a <= b, row by row
        a = int((2 * n + 1 - math.sqrt((2 * n + 1) ** 2 - 8 * r)) // 2)
        while a * (2 * n - a + 1) // 2 > r:
            a -= 1
        while (a + 1) * (2 * n - a) // 2 <= r:
            a += 1
        pairs.append((a, a + r - a * (2 * n - a + 1) // 2))
        q += 1
    g = np.zeros((n, m), dtype=np.uint8, order="F")
    for q, (a, b) in enumerate(pairs):
        j = q % m
        g[a, j] = 1 + q % 2
        if b != a:
            g[b, j] = 1 + (q // 2) % 2
    return g, pairs


def onehot_panel(n, m):
    """locus j is typed non-zero in individual j % n only, dosage 1 + (j // n) % 2: K[a, a] reads the weights back"""
    g = np.zeros((n, m), dtype=np.uint8, order="F")
    j = np.arange(m)
    g[j % n, j] = 1 + (j // n) % 2
    return g


# ---------------------------------------------------------------------------------------------------------------------
# weight patterns
T_WBITS = {4: 5, 5: 7, 6: 13, 7: 20, 8: 27}  # the wbits a "digits" case of T digits is built on: F = 22, 27, 28, 28, 28


def patterns(T):
    """the prescribed W of a "digits" case with T <= 7 digits, the anchor (largest weight, which sets wbits) first"""
    wbits = T_WBITS[T]
    F = 7 * T - 1 - wbits
    # the largest weight a panel can hold: all digits 63 where wbits >= 7, (2^wbits - 1) 2^F below (module docstring)
    anchor = top_of(T) if wbits >= 7 else ((1 << wbits) - 1) << F
    cap = anchor // 128 ** (T - 1) - (1 if wbits < 7 else 0)  # largest top digit that stays below the anchor with any lower digits
    out = [anchor, 1]
    out.append(from_digits([63] * (T - 1) + [cap]))                      # every digit +63
    out.append(from_digits([-64] * (T - 1) + [1]))                       # every digit -64 below a positive top digit
    out.append(from_digits([-64] * (T - 1) + [cap]))
    for t in range(T):                                                   # one non-zero digit at each position
        out.append(from_digits([0] * t + [1]))
        out.append(from_digits([0] * t + [63 if t < T - 1 else cap]))
        if t < T - 1:
            out.append(from_digits([0] * t + [-64] + [0] * (T - 2 - t) + [1]))
    # borrow chains: unsigned base-128 digits 0x40 (a borrow out of every digit) and 0x3F / 0x40 alternating, under a top
    # digit small enough for the dense panel's sums to stay below 2^53
    for low in ([0x40] * (T - 1), [0x3F, 0x40] * T, [0x40, 0x3F] * T, [0x7F] * (T - 1)):
        for top in (0x0E, 0):
            v = sum(d << (7 * t) for t, d in enumerate(low[:T - 1])) + (top << (7 * (T - 1)))
            out.append(v)
    assert max(out) == anchor and min(out) >= 1
    return out, wbits, F


def fill_weights(pats, m, limit):
    """m weights: the patterns once each, then the patterns below `limit` again and again"""
    small = [v for v in pats if v < limit]
    assert len(pats) <= m and small
    return np.array(pats + [small[i % len(small)] for i in range(m - len(pats))], dtype=np.int64)


def lcg_weights(m, T, seed):
    """the all-63 anchor (T >= 5, wbits = 7 T - 28 ... any wbits >= 7), then m - 1 weights with every digit in use"""
    x = np.random.default_rng(seed).integers(1, top_of(T), size=m, dtype=np.int64)
    x[0] = top_of(T)
    return x


def scales26(m, seed, nbig=12):
    """T = 8: scales of at most 26 significant bits (s s is exact, 1 / (s s) one correctly rounded division); the anchor
    w = 0.97 * 2^27, nbig - 1 more weights of 54 .. 55 bits, the others spread from 2^-10 to 2^10"""
    rng = np.random.default_rng(seed)
    ka = int(round(2.0 ** 25.5 / math.sqrt(0.97)))
    k = rng.integers(1 << 25, 1 << 26, size=m, dtype=np.int64)
    e = rng.integers(-31, -20, size=m)
    pos = rng.permutation(m)[:nbig]
    k[pos] = rng.integers(ka, 1 << 26, size=nbig)
    e[pos] = -39
    k[pos[0]] = ka
    s = np.ldexp(k.astype(np.float64), e)
    assert np.all(np.ldexp(np.rint(np.ldexp(s, -e)), e) == s)
    return s


# ---------------------------------------------------------------------------------------------------------------------
# cases
class Case:
    """name, family, n, m, scale, W, (wbits, T, F), the panels by kind ("pair", "dense", "onehot"), kind of the S bound
    ("exact": |S| < 2^53 everywhere, "wide": 2^53 <= max |S| < 2^62), arm(plan): the assertions on the restated plan"""

    def __init__(self, name, family, n, m, scale, kinds, arm, expect_T, size="exact", seed=1):
        self.name, self.family, self.n, self.m, self.kinds, self.arm, self.size, self.seed = name, family, n, m, kinds, arm, size, seed
        self.scale = np.ascontiguousarray(scale, dtype=np.float64)
        assert len(self.scale) == m
        self.wbits, self.T, self.F = digit_plan(self.scale)
        assert self.T == expect_T <= 8, (name, self.T, expect_T)
        self.W = weights(self.scale, self.F)
        assert self.W.min() >= 0 and self.W.max() <= top_of(self.T) and not digits(self.W, self.T)[1].any()
        assert safe(self.W) and guard(self.scale, self.F), name
        self._built = {}

    def panel(self, kind):
        """(g, S) of one of the case's panels, built once and left unchanged"""
        if kind not in self._built:
            g = {"pair": lambda: pair_panel(self.n, self.m)[0], "dense": lambda: dense_panel(self.n, self.m, self.seed),
                 "onehot": lambda: onehot_panel(self.n, self.m)}[kind]()
            S = exact_S(g, self.W)
            mx = int(S.max())
            assert 8 * sum(int(x) for x in self.W) < 2 ** 63  # (a factor two of room for the signed partial sums)
            if self.size == "exact":
                assert mx < 2 ** 53, (self.name, kind, math.log2(mx))
            elif kind == "dense":
                assert 2 ** 53 <= mx < 2 ** 62, (self.name, kind, math.log2(mx))
            g.setflags(write=False)
            S.setflags(write=False)
            self._built[kind] = (g, S)
        return self._built[kind]

    def check_arm(self, num_cu=256):
        p = plan(self.n, self.m, num_cu)
        self.arm(self, p)
        return p


CASES = []


def tds(T):
    return [td for _, td in passes(T)]


def _digit_cases():
    n, m = 97, 300
    for T in (4, 5, 6, 7):
        pats, wbits, F = patterns(T)

        def arm(c, p, T=T, wbits=wbits, F=F):
            assert (c.wbits, c.T, c.F) == (wbits, T, F) and tds(T) == ([4] if T == 4 else [4, T - 4])
            assert p.S == 1 and p.KG == 3 and (p.nsbf, p.rem) == (1, 0)
            d = digits(c.W, T)[0]
            for t in range(T - 1):  # every digit position sees both ends of its range, and so a borrow
                assert d[t].max() == 63 and d[t].min() == -64
            assert d[T - 1].max() == (63 if T > 4 else 62) and d[T - 1].min() == 0
            assert 1 in c.W and c.W.max() == (top_of(T) if T > 4 else 31 << 22)

        W = fill_weights(pats, m, 1 << 36)
        CASES.append(Case(f"digits_T{T}", "digits", n, m, scale_of(W, F), ("onehot", "pair", "dense"), arm, T))
    # 2^53 <= |S| < 2^62 at T = 7: the same patterns with the large ones repeated
    pats, wbits, F = patterns(7)
    W = fill_weights(pats, m, 1 << 49)
    CASES.append(Case("digits_T7_wide", "digits", n, m, scale_of(W, F), ("pair", "dense"),
                      lambda c, p: None, 7, size="wide"))

    def arm8(c, p):
        assert (c.wbits, c.T, c.F) == (27, 8, 28) and tds(8) == [4, 4]
        d = digits(c.W, 8)[0]
        assert all(d[t].max() > 0 and d[t].min() < 0 for t in range(7)) and d[7].max() == 62 and d[7].min() == 0
        assert all(d[t].max() >= 60 and d[t].min() <= -60 for t in range(4))  # (the upper ones: twelve large weights' worth)

    CASES.append(Case("digits_T8", "digits", n, m, scales26(m, 8), ("onehot", "pair", "dense"), arm8, 8, size="wide"))
    # the carry out of the top digit (module docstring): w = 127 and w = 4095 exactly, among ordinary weights
    for name, wtop, T, F in (("top_carry_F", 127.0, 5, 26), ("top_carry_T", 4095.0, 6, 22)):
        w = np.concatenate([[wtop, wtop * (1 - 2.0 ** -9)], np.random.default_rng(3).uniform(0.5, 40.0, size=m - 2)])
        sc = 1.0 / np.sqrt(w)
        sc[0] = np.float64(1.0) / np.sqrt(np.float64(wtop))

        def arm(c, p, T=T, F=F, wtop=wtop):
            assert 1.0 / (c.scale[0] * c.scale[0]) == wtop or abs(1.0 / (c.scale[0] * c.scale[0]) - wtop) < 1e-9 * wtop
            assert (c.T, c.F) == (T, F)
            w0 = int(np.rint(np.ldexp(1.0 / (c.scale.min() ** 2), 7 * c.T - 1 - c.wbits)))
            assert w0 > top_of((c.wbits + 29) // 7)  # it is in the top 1 / 127: the plain rule would lose the carry

        CASES.append(Case(name, "digits", n, m, sc, ("onehot", "dense"), arm, T))


def _t5_scale(m, seed):
    return scale_of(lcg_weights(m, 5, seed), 27)


def _k_cases():
    n = 130
    for KG in (1, 2, 3, 4, 5, 7):
        for m in (128 * (KG - 1) + 1, 128 * KG):  # one locus in the last group, and the group full
            def arm(c, p, KG=KG):
                assert p.KG == KG and p.S == 1 and (p.nsbf, p.rem) == (1, 1) and c.m % 128 in (0, 1)
                assert [k1 - k0 for k0, k1 in p.ranges] == [KG]

            CASES.append(Case(f"k_{KG}_{m}", "K ranges", n, m, _t5_scale(m, m), ("pair", "dense"), arm, 5))
    for KG, at256 in ((16, [8, 8]), (17, [8, 9]), (19, [9, 10]), (24, [8, 8, 8]), (25, [8, 8, 9])):
        m = 128 * KG - 59

        def arm(c, p, KG=KG, at256=at256):
            assert p.KG == KG and (p.nsbf, p.rem) == (1, 1) and c.m % 128 != 0
            if p.waves == 1024:
                assert [k1 - k0 for k0, k1 in p.ranges] == at256
            assert p.S >= 2  # six units: one round at any CU count (at least 32 waves), the flush is paid once and S > 1 wins

        CASES.append(Case(f"k_{KG}", "K ranges", n, m, _t5_scale(m, m), ("pair", "dense"), arm, 5))


TILE_N = (1, 31, 32, 33, 64, 96, 97, 127, 128, 129, 160, 192, 224, 256, 289)
TILE_ARMS = {1: (0, 1), 31: (0, 1), 32: (0, 1), 33: (0, 2), 64: (0, 2), 96: (0, 3), 97: (1, 0), 127: (1, 0), 128: (1, 0),
             129: (1, 1), 160: (1, 1), 192: (1, 2), 224: (1, 3), 256: (2, 0), 289: (2, 2)}


def _tile_cases():
    m = 300
    for n in TILE_N:
        def arm(c, p, n=n):
            assert (p.nsbf, p.rem) == TILE_ARMS[n] and p.S == 1 and p.patches == (1 if p.nsbf else 0)
            pairs = pair_panel(c.n, c.m)[1]
            nt = p.nrtv
            assert {(a >> 5, b >> 5) for a, b in pairs} >= {(x, y) for x in range(nt) for y in range(x, nt)}

        CASES.append(Case(f"tiles_{n}", "row tiles", n, m, _t5_scale(m, 1000 + n), ("pair", "dense"), arm, 5))
    assert {TILE_ARMS[n] for n in TILE_N} >= {(0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 2)}


def _patch_case():
    def arm(c, p):
        assert (p.nrtv, p.nsbf, p.rem, p.patches) == (38, 9, 2, 2) and p.S == 1 and p.KG == 2
        assert p.order.index((0, 8)) == 4 * 36  # the second patch starts behind the 36 super-tile pairs of the first
        pairs = pair_panel(c.n, c.m)[1]
        assert len({(a >> 5, b >> 5) for a, b in pairs}) == 38 * 39 // 2

    CASES.append(Case("patches_1185", "two patches", 1185, 256, _t5_scale(256, 77), ("pair", "dense"), arm, 5))


_digit_cases()
_k_cases()
_tile_cases()
_patch_case()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def names(family):
    return [c.name for c in CASES if c.family == family]


# the overflow: (name, n, m, scale, dosage) -- outside the sufficient condition, and their sums do pass 2^63
# ninth_digit: w = 2^33 (1 - 2^-9) with wbits = 33, T = 8, F = 22: in the top 1 / 127, no spare bit and no ninth digit
OVERFLOW_CASES = {"scale_1e-3": (130, 12000, 1e-3, "twos"), "scale_1e-4": (97, 300, 1e-4, "dense"),
                  "ninth_digit": (97, 3, float(1.0 / np.sqrt(2.0 ** 33 * (1 - 2.0 ** -9))), "dense")}


def overflow_case(name):
    n, m, s, kind = OVERFLOW_CASES[name]
    g = np.full((n, m), 2, dtype=np.uint8, order="F") if kind == "twos" else dense_panel(n, m, 5)
    return g, np.full(m, s)
