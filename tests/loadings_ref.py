"""Quantiser, integer reference, derived bound, restated launch plan and fault models for the int8 loadings
(csrc/pca.hip: tpg_u_digits_kernel, tpg_uq_colsum_kernel, tpg_loadings_mfma_kernel, tpg_loadings_finalize_kernel).

    v_jk = ( sum_i g_ij u_ik  -  c_j sum_i u_ik ) / (s_j d_k)

The device rounds u ONCE to fixed point, with one exponent for the whole n x k block: amax = max |u| < 2^ex (frexp),
FU = 7 TU - 2 - ex = 40 - ex, W = rint(u 2^FU) half to even (llrint of ldexp; numpy's rint of ldexp is the same), |W| <= 2^40.
Everything from there to the last four FP64 operations is integers:

    S_jk   = sum_i g_ij W_ik        what the six int32 digit planes recombine to; |S| <= 2 n 2^40 < 2^53 for n <= 2048
    Wsum_k = sum_i W_ik             |Wsum| <= n 2^40: the FP64 sum of the W_ik 2^-FU is exact in any order
    gu = S 2^-FU, usum = Wsum 2^-FU both doubles, no rounding
    p = fl(c_j usum_k);  t = fl(gu - p)  or, fused,  t = fl(gu - c_j usum_k);  D' = fl(s_j d_k);  v = fl(t / D')

EXACT tier (exact_loadings, compared with np.array_equal).  With c_j in {0, 1/2, 1, 2} and s_j, d_k powers of two, c_j usum_k is
Wsum_k times a power of two (or 0): a double.  gu - c usum = (2 S - (2 c) Wsum) 2^-(FU + 1) with |2 S - 2 c Wsum| =
2 |sum_i (g - c) W| <= 4 n 2^40 < 2^53: a double, fused or not.  s d and the quotient only move exponents.  No operation rounds,
so the result does not depend on contraction, and tests/test_loadings_host.py checks every claim of this paragraph in integers
on every exact panel.

GENERAL tier (rational_loadings, bound).  N = gu - c usum exactly (a rational; c is any double), D = s d exactly.  With
u = 2^-53 and |e_i| <= u:  p = c usum (1 + e1),  t = (gu - p)(1 + e2) = (N - c usum e1)(1 + e2),  D' = D (1 + e3),
v = t / D' (1 + e4).  To first order  |v - N / D| <= u (|c usum| + 3 |N|) / |D|; the bound is stated with 4 |N|, and that fourth
u |N| takes the second-order terms (all of them <= 4 u^2 (|N| + |c usum|)) wherever |N| >= 2^-50 |c usum|.  Where gu and c usum
cancel more deeply than that, the second-order share of u |c usum| -- 2^-51 of the bound -- is the one thing the statement leaves
out.  Fused, e1 = 0 and the bound holds with room.  Nothing in it is measured.

The restated launch plan (launches, pipeline, lm_lane_map, model_sums) follows the kernel's index arithmetic line by line and gives
S again -- the host test holds it to quantised_sums -- and the FAULTS are single knobs on that restatement.
"""
from fractions import Fraction

import numpy as np

TU = 6
LD_D = 4    # genotype register slots of tpg_loadings_mfma_kernel
LD_NLT = 2  # 32-locus tiles per wave
UNIT = Fraction(1, 2 ** 53)

KS = (1, 5, 6, 11, 16, 17, 22, 27, 33, 43, 64)  # tests/test_gpu_loadings.py: every arm of the launch chain
N_ROWS = (1, 127, 128, 129, 257, 385, 512, 513, 641, 897, 1025, 1152)  # Q = 1 1 1 2 3 4 4 5 6 8 9 9
N_LM = (8, 128, 136, 264, 384, 512, 520, 904, 1032)                    # Q = 1 1 2 3 3 4 5 8 9
M_EDGES = (1, 32, 33, 128, 129, 256, 257, 289)
N_EDGE = {"rows": (127, 257, 513), "locus_major": (128, 264, 520)}     # Q = 1, 3, 5: the depths the m and k lists are run at


def chunks(n):
    return -(-n // 128)


# ---------------------------------------------------------------------------------------------------------------------
# the quantiser
def exponent(U):
    """(amax, FU) of the whole block"""
    amax = float(np.abs(U).max())
    assert 0 < amax < 1e300
    _, ex = np.frexp(amax)  # amax = mant 2^ex, mant in [1/2, 1)
    return amax, 7 * TU - 2 - int(ex)


def fixed(U, FU):
    """rint(u 2^FU), int64"""
    return np.rint(np.ldexp(np.asarray(U, dtype=np.float64), np.int32(FU))).astype(np.int64)


def digits(W):
    """the balanced base-128 digits (TU, ...) of W, each in [-64, 63]; sum_t d_t 128^t == W"""
    W = W.astype(np.int64).copy()
    out = []
    for _ in range(TU):
        d = W & 127
        d = np.where(d >= 64, d - 128, d)
        out.append(d)
        W = (W - d) >> 7
    assert np.all(W == 0), "the fixed-point integer does not fit its digits"
    return np.stack(out)


def quantised_sums(G, U):
    """(S m x k, Wsum k, FU), int64"""
    _, FU = exponent(U)
    W = fixed(U, FU)
    assert np.abs(W).max() <= 2 ** 40 and G.shape[0] <= 2048
    return G.astype(np.int64).T @ W, W.sum(axis=0), FU


def _scaled(I, FU):
    return np.ldexp(I.astype(np.float64), np.int32(-FU))


def finalize(S, Wsum, FU, center, scale, d, fused=False):
    """the last four operations of tpg_loadings_finalize_kernel in FP64; fused: the subtraction as one fma, emulated in rationals
    (slow: the host test alone asks for it)"""
    gu, usum = _scaled(S, FU), _scaled(Wsum, FU)
    if fused:
        t = np.array([[float(Fraction(g) - Fraction(c) * Fraction(us)) for g, us in zip(row, usum)] for row, c in zip(gu, center)])
        t = t.reshape(gu.shape)
    else:
        t = gu - center[:, None] * usum[None, :]
    return np.asfortranarray(t / (scale[:, None] * d[None, :]))


def exact_loadings(G, U, center, scale, d):
    """the exact tier's reference: no operation of it rounds when center, scale and d are the exact tier's"""
    assert np.isin(center, (0.0, 0.5, 1.0, 2.0)).all()
    for x in (scale, d):
        assert (np.frexp(x)[0] == 0.5).all(), "powers of two"
    S, Wsum, FU = quantised_sums(G, U)
    return finalize(S, Wsum, FU, center, scale, d)


def _frac(x):
    return np.array([Fraction(float(v)) for v in np.ravel(x)], dtype=object).reshape(np.shape(x))


def rational_loadings(G, U, center, scale, d):
    """(N, D, P): N = gu - c usum, D = s d, P = c usum, exact, as object arrays of Fractions (m x k)"""
    S, Wsum, FU = quantised_sums(G, U)
    two = Fraction(2) ** (-FU)
    c, s, dd = _frac(center), _frac(scale), _frac(d)
    P = c[:, None] * (Wsum.astype(object) * two)[None, :]
    N = S.astype(object) * two - P
    return N, s[:, None] * dd[None, :], P


def bound(N, D, P):
    """|v - N / D| <= 2^-53 (|c usum| + 4 |N|) / |D|, element by element (Fractions)"""
    return UNIT * (abs(P) + 4 * abs(N)) / abs(D)


def error_over_bound(got, N, D, P):
    """max over the cells of |got - N / D| / bound (a cell with bound 0 must be hit exactly: inf otherwise)"""
    err = abs(_frac(got) - N / D)
    b = bound(N, D, P)
    worst = 0.0
    for e, bb in zip(err.ravel(), b.ravel()):
        worst = max(worst, float(e / bb) if bb else (0.0 if e == 0 else float("inf")))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# panels
class Panel:
    def __init__(self, name, G, U, center, scale, d):
        self.name, self.G, self.U = name, G, np.asfortranarray(U, dtype=np.float64)
        self.center, self.scale, self.d = center, scale, d
        self.n, self.m = G.shape
        self.k = U.shape[1]
        for a in (self.G, self.U, self.center, self.scale, self.d):
            a.setflags(write=False)

    def args(self):
        return self.G, self.U, self.center, self.scale, self.d

    def bytes(self):
        return np.asfortranarray(self.G.astype(np.uint8))


def genotypes(n, m, seed):
    """dosages 0 / 1 / 2 with a frequency of their own per locus, none missing; a monomorphic locus may occur (scale is the
    caller's on this route)"""
    rng = np.random.default_rng([seed, n, m])
    f = rng.uniform(0.05, 0.95, m)
    return (rng.random((n, m)) < f).astype(np.int64) + (rng.random((n, m)) < f).astype(np.int64)


def single_entry_genotypes(n, m):
    """locus j holds one 1 or 2 (in turn, two loci each) at individual rows[j] and 0 elsewhere: S_jk is one entry of W, so a
    piece that went to the wrong lane or chunk names itself.  rows: the first chunk's individuals on the even loci, the last
    chunk's on the odd ones -- with m >= 256 every byte position of every K step of both"""
    Q = chunks(n)
    first, last = np.arange(min(n, 128)), np.arange(128 * (Q - 1), n)
    rows = np.empty(m, dtype=np.int64)
    rows[0::2] = first[np.arange(len(rows[0::2])) % len(first)]
    rows[1::2] = last[np.arange(len(rows[1::2])) % len(last)]
    G = np.zeros((n, m), dtype=np.int64)
    G[rows, np.arange(m)] = 1 + (np.arange(m) // 2) % 2
    return G, rows


def full_W(n, k, seed):
    """u = W 2^-40 with W drawn from all 40 bits and one entry +-(2^40 - 1), so that FU = 40 and fixed(u) is W again"""
    rng = np.random.default_rng([seed, n, k, 40])
    W = rng.integers(-(2 ** 40 - 1), 2 ** 40, size=(n, k))
    W[(7 * k) % n, k // 2] = (2 ** 40 - 1) * (1 if k % 2 else -1)
    return np.ldexp(W.astype(np.float64), -40)


def gaussian_U(n, k, seed=0):
    """orthonormal columns of a Gaussian matrix, off the fixed-point grid (k > n: there are no k orthonormal columns, and they are
    Gaussian columns of norm 1)"""
    rng = np.random.default_rng([seed, n, k, 7])
    B = rng.standard_normal((n, k))
    if k > n:
        return B / np.linalg.norm(B, axis=0)
    U, _ = np.linalg.qr(B)
    return U


def spike_U(n, k):
    """tests/test_gpu_loadings.py's U: a constant column, a near-spike that sets the digit scale, the rest ~ n^-1/2 in the low
    digits"""
    rng = np.random.default_rng(100 + k)
    B = rng.standard_normal((n, k))
    B[:, 0] = 1.0 / np.sqrt(n)
    if k > 1:
        B[:, 1] = 0.0
        B[min(7, n - 1), 1] = 1.0
    U, _ = np.linalg.qr(B)
    return U


def exact_csd(m, k):
    """center in {0, 1/2, 1, 2}, scale and d powers of two, all of them changing along their axis with periods that share no
    factor with 32 or 6 (a transposed, shifted or tile-wrapped index shows)"""
    j, kk = np.arange(m), np.arange(k)
    center = np.array([0.0, 0.5, 1.0, 2.0])[(j * 3 + j // 5) % 4]
    return center, np.ldexp(1.0, (j % 7) - 3), np.ldexp(1.0, 4 - (kk % 5))


def exact_panel(n, m, k, kind="full", seed=1):
    """kind: "full" (40-bit W), "gauss" (orthonormal Gaussian, k <= n), "spike", "onehot<part>" or a name of PRESCRIBED;
    "single:<kind>" puts the single-entry genotypes under that U"""
    single = kind.startswith("single:")
    ukind = kind.split(":", 1)[1] if single else kind
    if ukind == "full":
        U = full_W(n, k, seed)
    elif ukind == "gauss":
        U = gaussian_U(n, k, seed)
    elif ukind == "spike":
        U = spike_U(n, k)
    elif ukind.startswith("onehot"):
        U = one_hot_U(n, k, int(ukind[6:]))
    else:
        U = PRESCRIBED[ukind](n, k)
    G = single_entry_genotypes(n, m)[0] if single else genotypes(n, m, seed)
    return Panel(f"{kind}-{n}x{m}x{k}", G, U, *exact_csd(m, k))


def general_panel(n, m, k, seed=2):
    """column means, binomial scales (a monomorphic locus is given one 0 and one 2 first; at n = 1, where every locus is
    monomorphic, scale 1), d = linspace(9, 2, k), Gaussian orthonormal U"""
    G = genotypes(n, m, seed)
    if n >= 2:
        mono = (G.sum(0) == 0) | (G.sum(0) == 2 * n)
        G[0, mono], G[1, mono] = 0, 2
    mean = G.sum(axis=0).astype(np.float64) / float(n)
    p = mean / 2
    scale = np.sqrt(2 * p * (1 - p)) if n >= 2 else np.ones(m)
    return Panel(f"general-{n}x{m}x{k}", G, gaussian_U(n, k, seed), mean, scale, np.linspace(9.0, 2.0, k))


# --- prescribed digits: W written down, u = W 2^(e - 40); every builder checks that the quantiser gives its W back
def _from_W(W):
    U = np.ldexp(W.astype(np.float64), -40)
    _, FU = exponent(U)
    assert FU == 40 and np.array_equal(fixed(U, FU), W)
    return U


def _cycle(values, n, k, anchor):
    """W[i, c] = values[(i + 3 c) mod len]: every value meets every byte position and K step within len * 16 rows or so; one entry
    is the anchor that pins FU = 40"""
    v = np.array(values, dtype=np.int64)
    i, c = np.meshgrid(np.arange(n), np.arange(k), indexing="ij")
    W = v[(i + 3 * c) % len(v)]
    W[n // 2, k - 1] = anchor
    return W


LOW5 = sum(128 ** t for t in range(5))  # 1 in each of the five low positions


def w_digits_min_max(n, k):
    """the five low digits all -64 or all 63 under every top digit that keeps |W| < 2^40 (the top digit itself cannot leave
    [-32, 32]: |W| <= 2^40 = 32 * 128^5), and single positions at -64 / 63"""
    vals = [top * 128 ** 5 + lo * LOW5 for top in (-31, -1, 0, 1, 31) for lo in (-64, 63)]
    vals += [lo * 128 ** t for t in range(5) for lo in (-64, 63)]
    return _from_W(_cycle(vals, n, k, 2 ** 40 - 1))


def w_carries(n, k):
    """64 and -65 in every position: 64 is written -64 carry 1, -65 is written 63 borrow 1, and with every position at it the
    carry runs through all six digits; also alone in each position"""
    vals = [top * 128 ** 5 + lo * LOW5 for top in (-30, 0, 30) for lo in (64, -65)]
    vals += [lo * 128 ** t for t in range(5) for lo in (64, -65)]
    vals += [2 ** 35 - 1, -(2 ** 35), 2 ** 35 - 64, -(2 ** 35) + 63]  # 127 in every low position: a carry chain of another kind
    return _from_W(_cycle(vals, n, k, -(2 ** 40 - 1)))


def w_pm_full(n, k):
    return _from_W(_cycle([2 ** 40 - 1, -(2 ** 40 - 1), 2 ** 40 - 2, 1, -1, 0], n, k, 2 ** 40 - 1))


def w_pow2(n, k):
    """amax = 1/2 exactly: frexp gives ex = 0, FU = 40, W = 2^39, the smallest W an amax can have"""
    U = _from_W(_cycle([2 ** 39 - 1, -(2 ** 39) + 1, 12345678901, -1, 3 * 2 ** 37], n, k, 2 ** 39))
    assert exponent(U) == (0.5, 40)
    return U


def w_below_pow2(n, k):
    """amax one ulp below 1/2: ex = -1, FU = 41, and rint(amax 2^41) = 2^40 -- the largest W there is, top digit 32"""
    U = w_pow2(n, k).copy()
    U[np.abs(U) == 0.5] = np.nextafter(0.5, 0.0)
    _, FU = exponent(U)
    assert FU == 41 and fixed(U, FU).max() == 2 ** 40
    return U


def _gauss_scaled(amax):
    def build(n, k):
        U = np.random.default_rng([n, k, 200]).standard_normal((n, k))
        return U * (amax / np.abs(U).max())
    return build


def one_hot_U(n, k, part):
    """column c is zero but for ONE individual: number 64 part + c of the first chunk's 128 followed by the last chunk's 128 (n a
    multiple of 128, k = 64: four parts name every byte position of every K step of both chunks).  Its W is 2^40 - 1 - 12345 c,
    signs in turn, so that S_jc = g_ij W_c says which individual and which column reached the sum"""
    assert n % 128 == 0 and n >= 256 and k == 64 and 0 <= part < 4
    who = np.concatenate([np.arange(128), np.arange(n - 128, n)])[64 * part:64 * part + 64]
    W = np.zeros((n, k), dtype=np.int64)
    c = np.arange(k)
    W[who, c] = (2 ** 40 - 1 - 12345 * c) * np.where(c % 2 == 0, 1, -1)
    return _from_W(W)


PRESCRIBED = {"digits_min_max": w_digits_min_max, "carries": w_carries, "pm_full": w_pm_full, "pow2": w_pow2,
              "below_pow2": w_below_pow2, "spike": spike_U, "tiny": _gauss_scaled(1e-200), "huge": _gauss_scaled(1e200)}


def _exact_cases():
    """(layout, n, m, k, kind): the exact tier's grid.  Depths at k = 7 (two column tiles, a straddling component) and m = 67;
    locus edges and column arms at Q = 1, 3, 5 / 3, 5, not their product with the depths; the prescribed digits at Q = 3 or 4;
    one nonzero individual per column at every position of the first and last chunk; the single-entry genotypes at m = 256"""
    out = []
    for layout, ns in (("rows", N_ROWS), ("locus_major", N_LM)):
        out += [(layout, n, 67, 7, "full") for n in ns]
        out += [(layout, n, m, 3, "full") for n in N_EDGE[layout] for m in M_EDGES]
        out += [(layout, n, 45, k, "spike") for n in N_EDGE[layout][1:] for k in KS]
        out += [(layout, 385 if layout == "rows" else 264, 40, 3, kind) for kind in PRESCRIBED]
        out += [(layout, 640, 40, 64, f"onehot{part}") for part in range(4)]
    out += [("rows", 641, 256, 2, "single:full"), ("locus_major", 520, 256, 2, "single:full"),
            ("locus_major", 264, 256, 2, "single:carries"), ("rows", 129, 256, 2, "single:digits_min_max")]
    return out


EXACT_CASES = _exact_cases()


def case_id(case):
    return "-".join(str(x) for x in case)


# ---------------------------------------------------------------------------------------------------------------------
# the launch plan, restated
def launches(k):
    """[(ct0, width)]: CT = ceil(6 k / 32) column tiles, four a launch while four are left, then one launch of 3, 2 or 1"""
    CT = -(-TU * k // 32)
    out, ct0 = [], 0
    while ct0 < CT:
        w = min(CT - ct0, 4)
        out.append((ct0, w))
        ct0 += w
    return CT, out


def grid(m):
    """(n_lt, workgroups, idle): n_lt = 4 KG tiles of 32 loci (KG groups of 128), a wave owns LD_NLT tiles, a workgroup four waves;
    idle = the waves (workgroup, wave) whose tiles lie past n_lt -- they fetch tile 0 again, serve the LDS, and store nothing"""
    n_lt = 4 * -(-m // 128)
    wgs = -(-n_lt // (4 * LD_NLT))
    idle = [(b, w) for b in range(wgs) for w in range(4) if (4 * b + w) * LD_NLT >= n_lt]
    return n_lt, wgs, idle


def pipeline(Q, lm, frag_clamp=None, stale_slot=False, extra_odd=False):
    """For the groups the loop runs, in order: (genotype chunk in the slot used -- rows -- or (pair base in the slots used, dq) -- LM --,
    group whose digit fragments are in the LDS buffer read).  Slot and buffer contents are tracked as the kernel assigns them.
    Knobs: frag_clamp (the clamp of the fragment look-ahead, Q - 1 in the kernel), stale_slot (a genotype slot is not refilled),
    extra_odd (LM, Q odd: the loop runs the second half of the last pair too)"""
    fc = Q - 1 if frag_clamp is None else max(frag_clamp, 0)
    AR = [None] * LD_D
    if lm:
        AR[0] = AR[1] = 0  # the pair (0, 1): base 0
    else:
        for dd in range(LD_D - 1):
            AR[dd] = min(dd, Q - 1)
    ubuf, un = [0, None], [None, min(1, fc)]
    used = []
    for q in range(Q + (1 if extra_odd and lm and Q % 2 == 1 else 0)):
        C = q % LD_D
        M = (C + LD_D - 1) % LD_D
        qa, qu, cur = min(q + LD_D - 1, Q - 1), min(q + 2, fc), q & 1
        if not lm:
            if not (stale_slot and qa >= LD_D):
                AR[M] = qa
        elif C % 2 == 0:
            qb = min(q + 2, Q - 1)
            if not (stale_slot and qb >= LD_D):
                AR[(C + 2) % LD_D] = AR[M] = qb
        un[C & 1] = qu
        used.append(((AR[C & ~1], C & 1) if lm else AR[C], ubuf[cur]))
        ubuf[cur ^ 1] = un[(C & 1) ^ 1]
    return used


def lm_lane_map(Q, base, dq, swap=False, untraded=()):
    """LM: the piece (chunk, locus in the tile, h) that lane (r, h) = lane r + 32 h holds in dword s of `av` for the group that
    uses the pair fetched at `base`, half dq: arrays [s, lane] -> chunk, locus, h.
    Load X of the pair: lane i fetches tpg_lm_piece(16 X + (i >> 2), Q, min(base + ldq, Q - 1), i & 1), ldq = (i >> 1) & 1.
    turn(): bs = load 1's register from lane i ^ 2 (quad_perm [2, 3, 0, 1]); the lane keeps a (load 0) if ldq == dq, else bs;
    ds_bpermute: lane L reads lane lm_src(L) / 4 ^ (dq ? 2 : 0), lm_src / 4 = (L & 15) 4 + ((L >> 4) & 1) 2 + (L >> 5).
    Knobs: swap (dq inverted), untraded (dwords that keep what the lane itself fetched in load 0)"""
    i = np.arange(64)
    ldq = (i >> 1) & 1
    chunk = np.minimum(base + ldq, Q - 1)
    load = [(chunk, 16 * X + (i >> 2), i & 1) for X in (0, 1)]
    if swap:
        dq ^= 1
    bs = tuple(a[i ^ 2] for a in load[1])
    sel = tuple(np.where(ldq == dq, a, b) for a, b in zip(load[0], bs))
    src = ((i & 15) * 4 + ((i >> 4) & 1) * 2 + (i >> 5)) ^ (2 if dq else 0)
    out = tuple(np.stack([load[0][x] if s in untraded else sel[x][src] for s in range(4)]) for x in range(3))
    return out


def model_sums(G, W, lm, frag_clamp=None, stale_slot=False, extra_odd=False, swap=False, untraded=(), ct0_lost=False,
               straddle_one_tile=False, idle_stored=False, reversed_digits=False, dg=None):
    """S by the kernel's route: digit planes in column tiles, launches, the pipeline's slots, LM's lane trade, int accumulators per
    (locus, digit column), recombination.  With every knob at rest this is G' W (the host test asserts it)."""
    n, m = G.shape
    k = W.shape[1]
    Q = chunks(n)
    CT, chain = launches(k)
    n_lt, _, idle = grid(m)
    # the A operand is the packed codes themselves, and the pack kernels write code 3 for individuals past n and loci past m:
    # harmless against the zero digits of those individuals, and only against them
    Gp = np.full((128 * Q, 32 * n_lt), 3, dtype=np.int64)
    Gp[:n, :m] = G
    dg = digits(W) if dg is None else dg
    UD = np.zeros((128 * Q, 32 * CT), dtype=np.int64)  # column 6 kk + t: digit t of component kk
    for t in range(TU):
        UD[:n, t:TU * k:TU] = dg[t]
    acc = np.zeros((32 * n_lt, 32 * CT), dtype=np.int64)
    e = np.arange(16)
    Gp3 = Gp.reshape(128 * Q, n_lt, 32)
    groups = []  # (the 128 x loci operand a group multiplies, the group whose digits it meets)
    for slot, uq in pipeline(Q, lm, frag_clamp, stale_slot, extra_odd):
        if not lm:
            A = Gp[128 * slot:128 * slot + 128]
        else:
            chunk, locus, hh = lm_lane_map(Q, slot[0], slot[1], swap, untraded)  # [s, lane]
            A3 = np.zeros((128, n_lt, 32), dtype=np.int64)
            for s in range(4):
                for h in range(2):
                    ln = np.arange(32) + 32 * h  # the lanes (r, h) of the operand: 16 individuals each in this K step
                    rows = 128 * chunk[s, ln] + 32 * s + 16 * hh[s, ln]
                    got = Gp3[rows[None, :] + e[:, None], :, locus[s, ln][None, :]]  # [e, r, tile]
                    A3[32 * s + 16 * h:32 * s + 16 * h + 16] = got.transpose(0, 2, 1)
            A = A3.reshape(128, 32 * n_lt)
        groups.append((A, uq))
    for li, (ct0, w) in enumerate(chain):
        src0 = 0 if (ct0_lost and li > 0) else ct0
        B = UD[:, 32 * src0:32 * (src0 + w)]
        part = np.zeros((32 * n_lt, 32 * w), dtype=np.int64)
        for A, uq in groups:
            part += A.T @ B[128 * uq:128 * uq + 128]
        acc[:, 32 * ct0:32 * (ct0 + w)] = part
    if idle_stored:  # an idle wave holds the sums of the tile it fetched (tile 0) and stores them where its own index wraps to
        for b, wv in idle:
            for t in range(LD_NLT):
                lt = ((4 * b + wv) * LD_NLT + t) % n_lt
                acc[32 * lt:32 * lt + 32] = acc[0:32]
    S = np.zeros((m, k), dtype=np.int64)
    for kk in range(k):
        for t in range(TU):
            col = TU * kk + t
            if straddle_one_tile:  # the tile of the component's first digit serves all six
                col = 32 * ((TU * kk) // 32) + col % 32
            S[:, kk] += acc[:m, col] * 128 ** (TU - 1 - t if reversed_digits else t)
    return S


# ---------------------------------------------------------------------------------------------------------------------
# fault models: one knob each
class NotApplicable(Exception):
    pass


def _need(cond, reason):
    if not cond:
        raise NotApplicable(reason)


PIECE = np.arange(48, 64)  # the 16 individuals of one lane's piece in one K step: chunk 0, s = 1, h = 1


def _piece(n):
    return PIECE[PIECE < n] if n > 48 else np.arange(min(n, 16))


def _with_digits(p, lm, dg):
    W = fixed(p.U, exponent(p.U)[1])
    return model_sums(p.G, W, lm, dg=dg), W.sum(axis=0)


def digit_unsigned(p, lm):
    """the lowest digit in one byte position of one lane's piece reaches the MFMA without its sign: d & 0xFF"""
    W = fixed(p.U, exponent(p.U)[1])
    dg = digits(W)
    rows = _piece(p.n)[5:6]
    _need((dg[0][rows] < 0).any(), "no negative lowest digit in that byte")
    dg[0][rows] &= 0xFF
    return _with_digits(p, lm, dg)


def _carry_fault(p, lm, edge):
    W = fixed(p.U, exponent(p.U)[1])
    dg = digits(W)
    rows = _piece(p.n)
    # the lowest digit sits at the edge: the carry (64 -> -64, +1) or the borrow (-65 -> 63, -1) into digit 1 is lost
    hit = (dg[0][rows] == -64) if edge == 64 else (dg[0][rows] == 63) & (W[rows] < 0)
    _need(hit.any(), "no lowest digit at the edge in the piece")
    sub = dg[1][rows]
    sub[hit] += -1 if edge == 64 else 1
    dg[1][rows] = sub
    return _with_digits(p, lm, dg)


def carry_dropped_63_64(p, lm):
    """a W whose lowest base-128 digit is 64: written -64, and the carry into the next digit is dropped"""
    return _carry_fault(p, lm, 64)


def carry_dropped_m64_m65(p, lm):
    """a negative W whose lowest digit wraps from -65 to 63: the borrow from the next digit is dropped"""
    return _carry_fault(p, lm, -65)


def _knob(**kw):
    def run(p, lm):
        W = fixed(p.U, exponent(p.U)[1])
        return model_sums(p.G, W, lm, **kw), W.sum(axis=0)
    return run


def digits_reversed(p, lm):
    """the finalize kernel recombines with the digit order reversed"""
    return _knob(reversed_digits=True)(p, lm)


def usum_unrounded(p, lm):
    """usum from u itself, not from the rounded values the contraction sees (returns Wsum as a float array in units of 2^-FU)"""
    _, FU = exponent(p.U)
    W = fixed(p.U, FU)
    raw = np.ldexp(p.U.sum(axis=0), np.int32(FU))
    _need((p.center != 0).any(), "every center is 0")
    _need(not np.array_equal(raw, W.sum(axis=0).astype(np.float64)), "u lies on the fixed-point grid")
    return model_sums(p.G, W, lm), raw


def ct0_lost(p, lm):
    """the launches after the first read their digit fragments from column tile 0 on"""
    _need(launches(p.k)[0] > 4, "CT <= 4: one launch")
    return _knob(ct0_lost=True)(p, lm)


def straddle_read_from_one_tile(p, lm):
    """a component whose six digits lie in two column tiles has all six read from the first"""
    _need(any((TU * kk) // 32 != (TU * kk + TU - 1) // 32 for kk in range(p.k)), "k <= 5: no component straddles two tiles")
    return _knob(straddle_one_tile=True)(p, lm)


def last_fragments_from_Qm2(p, lm):
    """the fragment look-ahead clamps at Q - 2: the last group meets the digits of the group before it"""
    _need(chunks(p.n) >= 2, "Q = 1: one group")
    return _knob(frag_clamp=chunks(p.n) - 2)(p, lm)


def slot_not_refilled(p, lm):
    """the genotype slot of group q + 4 still holds group q"""
    _need(chunks(p.n) > LD_D, "Q <= 4: no slot is used twice")
    return _knob(stale_slot=True)(p, lm)


def lm_clamped_chunk_added(p, lm):
    """LM, Q odd: the second half of the last pair -- the last chunk again -- is multiplied too"""
    _need(lm, "rows layout: no pairs")
    _need(chunks(p.n) % 2 == 1, "Q even: no clamped half pair")
    return _knob(extra_odd=True)(p, lm)


def lm_pair_swapped(p, lm):
    """LM: the two chunks of a pair trade places"""
    _need(lm, "rows layout: no pairs")
    _need(chunks(p.n) >= 2, "Q = 1: the pair is one chunk twice")
    return _knob(swap=True)(p, lm)


def lm_trade_first_dword_only(p, lm):
    """LM: the lane trade is done for dword 0; dwords 1 .. 3 stay in the lanes that fetched them"""
    _need(lm, "rows layout: no lane trade")
    return _knob(untraded=(1, 2, 3))(p, lm)


def idle_wave_stored(p, lm):
    """an idle wave stores the tile it holds"""
    _need(grid(p.m)[2], "no idle wave: the tiles fill their workgroups")
    _need(p.m > 32, "one tile of loci: the idle waves' copy of tile 0 lands on padding alone")
    return _knob(idle_stored=True)(p, lm)


FAULTS = [digit_unsigned, carry_dropped_63_64, carry_dropped_m64_m65, digits_reversed, usum_unrounded, ct0_lost,
          straddle_read_from_one_tile, last_fragments_from_Qm2, slot_not_refilled, lm_clamped_chunk_added, lm_pair_swapped,
          lm_trade_first_dword_only, idle_wave_stored]


def faulty_loadings(fault, p, lm):
    """the loadings the finalize kernel would give from the fault's sums (unfused)"""
    _, FU = exponent(p.U)
    S, Wsum = fault(p, lm)
    return finalize(S, Wsum, FU, p.center, p.scale, p.d)
