"""Builder, exact reference, derived bounds and a numpy model for the class Gram kernels (csrc/gramcls.hip).

S' = sum_c w_c G_c: the panel's loci sorted into classes of equal weight w = 1 / scale^2, every class padded to 64-locus
blocks, the integer class matrices G_c = g_c g_c' folded into FP64 either class by class (tpg_gcls_gram_kernel) or group by
group with the small weight differences inside a group summed in FP32 (tpg_gcls_gram2_kernel).  pca_gram takes any
per-locus scale, so a test can PRESCRIBE the class table: build() makes a panel from a list of (weight, loci) pairs,
describe() restates the table the device will make of it (classes, blocks, fold flags of both kernels), exact() is
sum_c w_c G_c with exact integer G_c and long-double sums, the rel_* / bound_* functions are error bounds DERIVED from the
arithmetic the kernels do (no constant in them is fitted to an observed error), and model() runs the two folding schemes
in numpy over the restated table for any cut into K ranges -- tests/test_gramcls_host.py shows with it that the bounds
hold for a right kernel and that every slip on its list of mutations leaves them.  CASES is the table of structures that
tests/test_gpu_gramcls.py runs on the device; every case names the edge it was built for and asserts it on the table.
"""
import numpy as np

GCLS_GQ = 6          # a group: same exponent and leading GCLS_GQ mantissa bits
GCLS_GMAX = 64       # ... and at most this many classes (absolute run index)
GCLS_GRUN = 16384    # blocks between two full folds of the mixed kernel
GCLS_MAX_RUN = 65536  # blocks between two folds of the FP64-fold kernel
W_MAX = 4096.0       # pca_gram_device checks the digit range of 1 / scale^2 before the class path runs

LD = np.longdouble


# ---------------------------------------------------------------------------------------------------------------------
# the class table
class Meta:
    """The device's class table for a vector of scales (tpg_gcls_keys_kernel ... tpg_gcls_block_table2_kernel).

    w[j]          1.0 / (scale[j] * scale[j]), float64
    key[r], wkey[r], count[r], nblk[r], blk_start[r]     per class, in key order
    src[64 b + l] locus on slot l of block b (-1: padding); a class's loci keep their order (the radix sort is stable)
    cls[b]        class of block b
    flag64[b]     1: the FP64-fold kernel folds after block b
    flag2[b]      1: class end inside a group, 2: full fold after block b (mixed kernel)
    delta[b]      float32(w_c - w_{c+1}) where flag2 == 1
    group[r]      index of the group of class r (a new group after every class-end full fold)
    F64, F2       fold events in the two tables
    """

    def ranges(self, S):
        return [((self.npairs * ks) // S, (self.npairs * (ks + 1)) // S) for ks in range(S)]

    @property
    def fold64_by_default(self):  # gcls_fold64 without TPG_GRAM_FOLD64
        return float(self.nruns) < 0.15 * float(self.nblocks)


def describe(scale, w_max=W_MAX):
    """w_max: the largest weight the caller expects (the overflow cases of tests/gramdig_ref.py reach the class route with
    weights of 1e6 and more; nothing in the table depends on it)"""
    scale = np.ascontiguousarray(scale, dtype=np.float64)
    me = Meta()
    me.w = 1.0 / (scale * scale)
    assert np.all(me.w > 0) and me.w.max() <= w_max
    bits = me.w.view(np.uint64)
    key = (bits + np.uint64(16)) & ~np.uint64(31)
    order = np.argsort(key, kind="stable")
    me.key, start, count = np.unique(key[order], return_index=True, return_counts=True)
    me.wkey = me.key.view(np.float64)
    nr = me.nruns = len(me.key)
    me.count, me.start = count.astype(np.int64), start.astype(np.int64)
    me.nblk = (me.count + 63) // 64
    me.blk_start = np.concatenate([[0], np.cumsum(me.nblk)[:-1]]).astype(np.int64)
    nb = me.nblocks = int(me.nblk.sum())
    me.npairs = (nb + 1) // 2
    me.cls = np.repeat(np.arange(nr), me.nblk)
    off = np.arange(nb) - me.blk_start[me.cls]
    class_end = off + 1 == me.nblk[me.cls]
    me.flag64 = (class_end | (off % GCLS_MAX_RUN == GCLS_MAX_RUN - 1)).astype(np.int8)
    bucket = me.key >> np.uint64(52 - GCLS_GQ)
    r = np.arange(nr)
    ce_full = r == nr - 1
    ce_full[:-1] |= bucket[:-1] != bucket[1:]
    ce_full |= r % GCLS_GMAX == GCLS_GMAX - 1
    ce_full |= me.blk_start // GCLS_GRUN != (me.blk_start + me.nblk) // GCLS_GRUN
    full = (off % GCLS_GRUN == GCLS_GRUN - 1) | (class_end & ce_full[me.cls])
    me.flag2 = np.where(full, 2, np.where(class_end, 1, 0)).astype(np.int8)
    nxt = np.minimum(me.cls + 1, nr - 1)
    me.delta = np.where(me.flag2 == 1, (me.wkey[me.cls] - me.wkey[nxt]).astype(np.float32), np.float32(0))
    me.group = np.concatenate([[0], np.cumsum(ce_full[:-1])]).astype(np.int64)
    me.order = order
    pos = me.blk_start[np.repeat(r, me.count)] * 64 + (np.arange(len(scale)) - np.repeat(me.start, me.count))
    me.src = np.full(nb * 64, -1, dtype=np.int64)
    me.src[pos] = order
    me.F64, me.F2 = int(me.flag64.sum()), int((me.flag2 == 2).sum())
    return me


def build(structure, n, seed):
    """(g, scale, meta) for a list of (w_target, n_loci) pairs: n x m dosages 0 / 1 / 2 without a missing value and with
    every column polymorphic (two different dosages; one individual alone is a heterozygote), scale = 1 / sqrt(w_target),
    the classes' loci interleaved in a seeded random column order.  Both alleles at frequency one half, so that all
    entries of S' lie within a small factor of each other (about 1 : 1.5 between off-diagonal and diagonal)."""
    rng = np.random.default_rng(seed)
    wt = np.repeat(np.array([s[0] for s in structure], dtype=np.float64), [s[1] for s in structure])
    m = len(wt)
    scale = np.empty(m)
    scale[rng.permutation(m)] = 1.0 / np.sqrt(wt)
    bits = rng.integers(0, 4, size=(n, m), dtype=np.uint8)
    g = np.asfortranarray((bits & 1) + (bits >> 1))
    del bits
    if n == 1:
        g[:] = 1
    else:
        flat = (g == g[0]).all(axis=0)
        g[0, flat] = (g[0, flat] + 1) % 3
    return g, scale, describe(scale)


# ---------------------------------------------------------------------------------------------------------------------
# the exact reference
def _int_gram(gc):
    """g_c g_c' in float64, exact: float32 products of at most 2^15 loci (sums below 2^17), added in float64 (below 2^53)"""
    n = gc.shape[0]
    G = np.zeros((n, n))
    for s in range(0, gc.shape[1], 32768):
        a = gc[:, s:s + 32768].astype(np.float32)
        G += (a @ a.T).astype(np.float64)
    return G


def exact(g, scale):
    """R = sum over the distinct float64 weights w of w * G_w, G_w the integer Gram matrix of the loci of that weight:
    long-double products and sums of exact terms (no Z Z' anywhere).  2^-64 per operation: far below every bound here."""
    scale = np.asarray(scale, dtype=np.float64)
    w = 1.0 / (scale * scale)
    wu, inv = np.unique(w, return_inverse=True)
    order = np.argsort(inv, kind="stable")
    ends = np.cumsum(np.bincount(inv, minlength=len(wu)))
    n = g.shape[0]
    R = np.zeros((n, n), dtype=LD)
    s = 0
    for c, e in enumerate(ends):
        R += LD(wu[c]) * _int_gram(g[:, order[s:e]]).astype(LD)
        s = e
    return R


def centre(R):
    """H R H in long double"""
    R = np.asarray(R, dtype=LD)
    return R - R.mean(axis=0, keepdims=True) - R.mean(axis=1, keepdims=True) + R.mean()


def centred_majorant(g, meta):
    """max over the pairs of M_ik = sum_j w_j |term_j|, term_j what the centred-operand kernel adds for locus j: g_i g_k
    on the even blocks of the sorted list, (g_i - 1)(g_k - 1) on the odd ones.  Every partial sum of that kernel is at
    most M in magnitude, which is what bound_centred needs in place of S' (see there)."""
    slot = np.empty(g.shape[1], dtype=np.int64)
    slot[meta.src[meta.src >= 0]] = np.nonzero(meta.src >= 0)[0]
    odd = (slot // 64) % 2 == 1
    M = np.zeros((g.shape[0], g.shape[0]))
    for s in range(0, g.shape[1], 65536):
        gm = g[:, s:s + 65536].astype(np.float64)
        gm[:, odd[s:s + 65536]] = np.abs(gm[:, odd[s:s + 65536]] - 1.0)
        M += (gm * meta.w[None, s:s + 65536]) @ gm.T
    return float(M.max())


# ---------------------------------------------------------------------------------------------------------------------
# bounds
U = 2.0 ** -53


def rel_fold64(meta):
    """Elementwise relative bound of tpg_gcls_gram_kernel + tpg_gcls_assemble_kernel with center = 0 (K = S'):
        |K_ik - R_ik| <= (2^-47 + (F + 34) 2^-53) R_ik,   F = fold events of the table (meta.F64).

    The FP4 products and their FP32 sums are exact integers: a class is folded at its end and after GCLS_MAX_RUN blocks
    at the latest (256 * 2^16 = 2^24).  What is rounded:
    * the weight: a class is folded with its KEY, (bits + 16) & ~31 read as a double, at most 16 units in the last place
      = 2^-48 away from the weight of any of its loci.  2^-47 is kept as the issue states it; the spare 2^-48 also covers
      a device reciprocal that is one unit off numpy's.
    * the folds o = fma(acc, w, o): one rounding each, 2^-53 of a partial sum of non-negative terms, i.e. of at most the
      slab's final value.  Range ks does F_ks of the table's folds and one more at its end (b == bl): together at most
      sum_ks (F_ks + 1) 2^-53 slab_ks <= (F + 1) 2^-53 R_ik.
    * the assemble kernel adds S <= 32 slabs in order, the first one to zero: at most 31 roundings of a partial sum <= R.
    First order (F + 32) 2^-53; (1 + u)^(F + 32) - 1 <= (F + 34) u as long as (F + 32)^2 u <= 2, which is asserted."""
    F = meta.F64
    assert (F + 32) ** 2 * U <= 2.0
    return 2.0 ** -47 + (F + 34) * U


C32 = GCLS_GMAX * 2.0 ** -24 * (1 + 2.0 ** -17) * 2.0 ** -GCLS_GQ  # = 2^-24 (1 + 2^-17) = 5.96e-8


def rel_mixed(meta):
    """Elementwise relative bound of tpg_gcls_gram2_kernel<false> + assemble with center = 0:
        |K_ik - R_ik| <= (2^-47 + (2 F + 66)(1 + 2^-6) 2^-53 + C32) R_ik,   F = full folds of the table (meta.F2),
        C32 = GCLS_GMAX 2^-24 (1 + 2^-17) 2^-GCLS_GQ = 5.96e-8.

    One K range's piece of one group holds classes 1 .. L (L <= GCLS_GMAX: a group ends where the absolute run index is
    GCLS_GMAX - 1 mod GCLS_GMAX) with keys w_1 < ... < w_L in one bucket, w_L - w_1 < 2^-GQ w_1.  With P_c the running
    integer sums from the start of the piece (exact: a group has fewer than 2^15 blocks, 256 * 2^15 = 2^23),
        sum_c w_c G_c = w_L P_L + sum_{c < L} d_c P_c,   d_c = w_c - w_{c+1} < 0       (summation by parts, exact)
    holds for ANY starting point with zero sums and any last class, so a range that starts or ends inside a group computes
    its own share T of the group by the same identity with no more terms than the whole group has: it does not enlarge
    anything below.  (The class end pending at a range end is folded with w_c itself, which is the identity with L = c.)
    * FP32 part.  sum_c |d_c| P_c <= (w_L - w_1) P_L <= 2^-GQ w_1 P_L <= 2^-GQ T elementwise (G_c >= 0).  d_c is an exact
      double (two keys of one binade), rounded once to float (a normal float: |d_c| >= 2^-47 w, and w >= 2^-60 is
      asserted below); every term then goes through at most L - 1 <= GMAX - 1 roundings of the
      FP32 FMA chain: at most GMAX factors (1 + e), |e| <= 2^-24, so the FP32 sum is off by at most
      ((1 + 2^-24)^GMAX - 1) 2^-GQ T <= GMAX 2^-24 (1 + 2^-17) 2^-GQ T.  Summed over pieces: C32 R_ik.
    * FP64 part.  A full fold is o = fma(acc, w, o) + (double)dev: two roundings, of partial sums that exceed the true
      (non-negative, growing) partial sum by at most |dev| <= 2^-GQ of it.  Each range does its share of the F full folds
      and one at its end; then the assemble sums as in rel_fold64: (2 (F + 1) + 31)(1 + 2^-6) 2^-53, and 2 F + 66 covers
      the second-order terms as there.
    * the key: 2^-47, as in rel_fold64."""
    F = meta.F2
    assert (2 * F + 64) ** 2 * U <= 2.0 and meta.w.min() >= 2.0 ** -60
    return 2.0 ** -47 + (2 * F + 66) * (1 + 2.0 ** -GCLS_GQ) * U + C32


def rel_mixed_table(meta):
    """rel_mixed with the FP32 part taken from THIS table instead of the worst table there is: the same derivation gives,
    for a group g of L_g classes whose keys span s_g = (w_last - w_first) / w_first, an FP32 error of at most
    L_g 2^-24 (1 + 2^-17) s_g T, so that C32 becomes max_g L_g s_g 2^-24 (1 + 2^-17) (<= C32: L_g <= GMAX, s_g < 2^-GQ; a
    K range's or a mid-class fold's piece of a group has no more classes and no wider span than the group).  Five classes
    2^-9 apart give 3e-9 where C32 is 6e-8: this is the bound a subtly wrong FP32 term meets first."""
    first = np.concatenate([[0], np.nonzero(np.diff(meta.group))[0] + 1])
    last = np.concatenate([first[1:] - 1, [meta.nruns - 1]])
    c32 = float(((last - first + 1) * (meta.wkey[last] - meta.wkey[first]) / meta.wkey[first]).max()) * 2.0 ** -24 * (1 + 2.0 ** -17)
    assert c32 <= C32
    return rel_mixed(meta) - C32 + c32


def bound_centred(rel, R, n, majorant=None):
    """Bound of max |K - H R H| for the centred call (center = column mean: K = H S' H, formed on the device):
        4 max_ab (rel R_ab) + n 2^-52 max |R|.

    * H E H of an elementwise error E: the rows of |H| = |I - 11'/n| sum to 2 (1 - 1/n) < 2, so |H E H|_ik <= 4 max |E|.
    * The centred-operand kernel (tpg_gcls_gram2_kernel<true>) sums (g_i - 1)(g_k - 1) on the odd blocks; what that
      leaves out is r_i + r_k + const, which H removes exactly.  Its partial sums are no longer non-negative, but bounded
      by the majorant M of centred_majorant(), so every step of rel_mixed's derivation holds with max M in place of R_ik;
      the bound is stated against max R and REQUIRES max M <= max R, asserted here when the majorant is given (the
      builder's dosages give E M_ik <= 1.0 against E R_ii = 1.5 per locus and unit weight).
    * The double centring itself (tpg_colmean_kernel, tpg_mean_kernel, tpg_double_center_kernel): a column mean is
      ceil(n / 256) - 1 serial additions, 8 tree levels and a division, d + 1 <= 10 roundings for n <= 512, each at most
      2^-53 max|S'|; the grand mean inherits that and adds as much; K - r_i - r_k + C carries those 4 (d + 1) and three
      roundings of sums up to 2, 3 and 4 max|S'|: at most 49 * 2^-53 = 24.5 * 2^-52 of max |R|.  The issue states this
      term as n 2^-52 max |R|; for n < 25 the difference is covered by the 4 * 2^-48 that rel leaves unused in its key
      term (64 * 2^-52).  n <= 512 is asserted."""
    assert n <= 512
    mx = float(np.abs(R).max())
    if majorant is not None:
        assert majorant <= mx * (1 + 2.0 ** -30), (majorant, mx)  # (M is summed in float64; equal where every block is even)
    return 4.0 * float((rel * np.abs(R)).max()) + n * 2.0 ** -52 * mx


# ---------------------------------------------------------------------------------------------------------------------
# the model
def _fma(acc, w, o):
    return (acc.astype(LD) * LD(w) + o.astype(LD)).astype(np.float64)


MUTATIONS = ("drop_last_locus_of_class", "drop_first_locus_of_block", "pad_read_as_one", "neighbour_weight", "omit_delta",
             "delta_one_block_late", "range_end_next_weight", "pair_in_both", "pair_in_neither", "pad_block_flagged",
             "pad_block_takes_flag", "omit_grun_fold")


def model(g, meta, kernel, S, mut=None, at=None):
    """K = S' as the FP64-fold kernel (kernel = "fold64") or the mixed-fold kernel ("mixed") and the assemble kernel
    compute it over meta's block table, the block-pair list cut into S ranges [npairs ks / S, npairs (ks + 1) / S).
    Integer sums are carried exactly (and asserted to fit FP32), FP32 and FP64 roundings are numpy's; an FMA is a
    long-double product and sum rounded to double.  mut names one slip (MUTATIONS), `at` where: a class, a block or a
    range index."""
    assert kernel in ("fold64", "mixed") and (mut is None or mut in MUTATIONS)
    n = g.shape[0]
    nb, npairs, nr = meta.nblocks, meta.npairs, meta.nruns
    T = np.zeros((2 * npairs * 64, n), dtype=np.float32)
    ok = meta.src >= 0
    T[:nb * 64][ok] = g[:, meta.src[ok]].T
    if mut == "drop_last_locus_of_class":
        T[meta.blk_start[at] * 64 + meta.count[at] - 1] = 0
    elif mut == "drop_first_locus_of_block":
        T[at * 64] = 0
    elif mut == "pad_read_as_one":
        assert at % 2 == 0 and meta.src[at * 64 + 63] < 0
        T[at * 64 + 63] = 1
    T = T.reshape(2 * npairs, 64, n)
    cum = np.zeros((2 * npairs + 1, n, n))
    np.cumsum(np.einsum("bli,blk->bik", T, T).astype(np.float64), axis=0, out=cum[1:])
    # per-block table, padded to whole pairs: the padding entry is the last class's, flagless
    npad = 2 * npairs - nb
    cls = np.concatenate([meta.cls, np.full(npad, nr - 1)])
    wb = meta.wkey[cls].copy()
    flag = np.concatenate([meta.flag64 if kernel == "fold64" else meta.flag2, np.zeros(npad, dtype=np.int8)])
    delta = np.concatenate([meta.delta, np.zeros(npad, dtype=np.float32)])
    if mut == "neighbour_weight":
        wb[cls == at] = meta.wkey[at + 1]
    elif mut == "pad_block_flagged":
        assert npad == 1
        flag[nb] = flag[nb - 1]
    elif mut == "pad_block_takes_flag":
        assert npad == 1
        flag[nb], flag[nb - 1] = flag[nb - 1], 0
    elif mut == "omit_grun_fold":
        off = np.arange(nb) - meta.blk_start[meta.cls]
        flag[:nb][(off + 1 != meta.nblk[meta.cls]) & (flag[:nb] == 2)] = 0
    top = 2.0 ** 24

    def sums(b_from, b_to):  # integer sums of blocks [b_from, b_to)
        a = cum[b_to] - cum[b_from]
        if mut == "omit_grun_fold":
            return np.minimum(a, top)  # the FP32 accumulators stop counting
        assert a.max(initial=0.0) <= top
        return a

    K = np.zeros((n, n))
    for ks, (p0, p1) in enumerate(meta.ranges(S)):
        if mut == "pair_in_both" and ks == at - 1:
            p1 += 1
        if mut == "pair_in_neither" and ks == at:
            p0 += 1
        o = np.zeros((n, n))
        if p0 < p1:
            if kernel == "fold64":
                b0, b1 = 2 * p0, min(2 * p1, nb)
                since = b0
                for b in b0 + np.nonzero(flag[b0:b1])[0]:
                    o = _fma(sums(since, b + 1), wb[b], o)
                    since = b + 1
                if since < b1:
                    o = _fma(sums(since, b1), wb[b1 - 1], o)
            else:
                b0, b1 = 2 * p0, 2 * p1
                since = b0
                dev = np.zeros((n, n), dtype=np.float32)
                for b in b0 + np.nonzero(flag[b0:b1])[0]:
                    if flag[b] == 2:
                        o = _fma(sums(since, b + 1), wb[b], o) + dev.astype(np.float64)
                        since = b + 1
                        dev[:] = 0
                    elif b + 1 < b1 and not (mut == "omit_delta" and cls[b] == at):
                        # the class end is applied in front of the next block of the range, to the sums as they are then
                        upto = b + 2 if mut == "delta_one_block_late" and cls[b] == at else b + 1
                        dev = (np.float64(delta[b]) * sums(since, upto) + dev.astype(np.float64)).astype(np.float32)
                w = wb[b1 - 1]
                if mut == "range_end_next_weight" and flag[b1 - 1] == 1:
                    w = meta.wkey[cls[b1 - 1] + 1]
                o = _fma(sums(since, b1), w, o) + dev.astype(np.float64)
        K = K + o
    return K


# ---------------------------------------------------------------------------------------------------------------------
# the case table
def _jitter(w, k):
    """w (1 + x 2^-16), 0 <= x < 1 from the golden ratio: a weight with all its mantissa bits in use, so that its key is
    rounded, its difference to a neighbour is rounded to float and the FP32 products are (weights such as 1 + k 2^-10 pass
    through the FP32 sums of the mixed fold without one rounding)"""
    return w * (1.0 + ((k + 1) * 0.6180339887498949 % 1.0) * 2.0 ** -16)


def _bucket_w(e, q, i, step=2.0 ** -9):
    """weight i of bucket (exponent e, leading mantissa bits q): 2^e (1 + q / 64 + (i + 1) step) (1 + jitter),
    (i + 2) step + 2^-15 < 2^-6"""
    assert 0 <= q < 64 and (i + 2) * step + 2.0 ** -15 < 2.0 ** -6
    return _jitter(2.0 ** e * (1.0 + q / 64.0 + (i + 1) * step), 64 * i + q + e)


class Case:
    def __init__(self, name, family, structure, n, edge, seed=1):
        self.name, self.family, self.structure, self.n, self.edge, self.seed = name, family, structure, n, edge, seed

    def build(self, n=None):
        g, scale, meta = build(self.structure, self.n if n is None else n, self.seed)
        self.edge(meta)
        return g, scale, meta


def _ngroups(meta):
    return int(meta.group[-1]) + 1


CASES = []
BLOCK_LENGTHS = [1, 63, 64, 65, 127, 128, 129]


def _block_edges():
    for grouping in ("group", "bucket"):
        for parity in ("even", "odd"):
            lens = BLOCK_LENGTHS + ([64] if parity == "odd" else [])
            ws = [_bucket_w(0, 3, i, 2.0 ** -10) if grouping == "group" else _bucket_w(0, 3 + i, 0) for i in range(len(lens))]

            def edge(meta, lens=lens, grouping=grouping, parity=parity):
                assert sorted(meta.count.tolist()) == sorted(lens) and meta.count.tolist()[:7] == BLOCK_LENGTHS
                assert meta.nblk.tolist()[:7] == [1, 1, 1, 2, 2, 2, 3]
                assert meta.nblocks % 2 == (1 if parity == "odd" else 0)
                assert _ngroups(meta) == (1 if grouping == "group" else meta.nruns)
                assert meta.F2 == _ngroups(meta) and int((meta.flag2 == 1).sum()) == meta.nruns - _ngroups(meta)

            CASES.append(Case(f"blocks_{grouping}_{parity}", "block edges", list(zip(ws, lens)), 40, edge))
    for m in (1, 64, 65):
        def edge(meta, m=m):
            assert meta.nruns == 1 and meta.nblocks == (m + 63) // 64 and meta.npairs == 1
            assert meta.ranges(2)[0] == (0, 0)  # S = 2 on one pair: the first K range is empty

        CASES.append(Case(f"one_class_{m}", "block edges", [(1.0 / 0.42, m)], 40, edge))


def _group_structure(ncl, e=0, q=5):
    # ncl classes of 1, 2, 3 blocks inside one bucket: 2^e (1 + q / 64 + (i + 1) 2^-14) (1 + jitter 2^-16), 131 * 2^-14 < 2^-6
    return [(_jitter(2.0 ** e * (1.0 + q / 64.0 + (i + 1) * 2.0 ** -14), i), (40, 100, 150)[i % 3]) for i in range(ncl)]


def _group_edges():
    for ncl in (63, 64, 65, 129):
        def edge(meta, ncl=ncl):
            assert meta.nruns == ncl and len(set((meta.key >> np.uint64(46)).tolist())) == 1
            assert set(meta.nblk.tolist()) == {1, 2, 3}
            assert _ngroups(meta) == (ncl + GCLS_GMAX - 1) // GCLS_GMAX  # cut by GCLS_GMAX alone
            assert np.bincount(meta.group).max() == min(ncl, GCLS_GMAX)

        CASES.append(Case(f"group_{ncl}", "group edges", _group_structure(ncl), 40, edge))

    def edge(meta):  # neighbours 2^-11 apart on the two sides of a 2^-6 bucket edge, and a group on either side
        assert meta.nruns == 8 and _ngroups(meta) == 2 and meta.group.tolist() == [0] * 4 + [1] * 4
        assert meta.wkey[4] - meta.wkey[3] < 2.0 ** -10 * meta.wkey[3]

    b = 1.0 + 9 / 64.0
    CASES.append(Case("bucket_edge", "group edges",
                      [(_jitter(b - (i + 1) * 2.0 ** -12, i), 70 + 30 * i) for i in range(4)] + [(_jitter(b + (i + 1) * 2.0 ** -12, 4 + i), 90 + 30 * i) for i in range(4)],
                      40, edge))

    def edge(meta):  # the exponent changes between two neighbours 2^-11 apart
        assert meta.nruns == 8 and _ngroups(meta) == 2 and meta.group.tolist() == [0] * 4 + [1] * 4
        assert meta.wkey[3] < 2.0 <= meta.wkey[4] and (meta.key[3] >> np.uint64(52)) + np.uint64(1) == meta.key[4] >> np.uint64(52)

    CASES.append(Case("power_of_two", "group edges",
                      [(_jitter(2.0 * (1 - (i + 1) * 2.0 ** -12), i), 70 + 30 * i) for i in range(4)] + [(_jitter(2.0 * (1 + (i + 1) * 2.0 ** -12), 4 + i), 90 + 30 * i) for i in range(4)],
                      40, edge))

    def edge(meta):  # a key that carries into the exponent: the weight just below 4 rounds to the key 4.0 exactly
        assert meta.nruns == 3 and meta.wkey[1] == 4.0 and meta.w.max() > 4.0 and np.sum(meta.w < 4.0) == 200 + 130

    CASES.append(Case("key_carry", "group edges", [(4.0 * (1 - 2.0 ** -50), 130), (4.0 * (1 + 2.0 ** -9), 77), (3.5, 200)], 40, edge))

    spread = [(_bucket_w(e, (7 * e) % 64, i), 50 + 17 * ((e + i) % 9)) for e in range(-10, 12) for i in range(3)]

    def edge(meta):
        # 22 buckets, and the three-class bucket of runs 63 .. 65 is cut after run 63: GCLS_GMAX counts absolute runs
        assert meta.nruns == 66 and _ngroups(meta) == 23 and np.bincount(meta.group).tolist() == [3] * 21 + [1, 2]
        assert 2.0 ** -10 <= meta.w.min() < 2.0 ** -9 and 2.0 ** 11 < meta.w.max() <= W_MAX

    CASES.append(Case("spread", "group edges", spread, 40, edge))
    for name, per, f64 in (("ratio_below", 10, True), ("ratio_above", 5, False)):
        def edge(meta, per=per, f64=f64):  # 20 classes in 200 or 100 blocks: 0.10 and 0.20 classes per block
            assert meta.nruns == 20 and meta.nblocks == 20 * per and meta.fold64_by_default == f64
            assert _ngroups(meta) == 4

        CASES.append(Case(name, "group edges", [(_bucket_w(1, 11 + i // 5, i % 5), 64 * per - 3 * i) for i in range(20)], 40, edge))


def ranges_structure(nblocks):
    """classes of 1, 1, 2, 1, 3, 2, ... blocks up to nblocks blocks in all, the last block of every class partly filled,
    five classes to a bucket and at least 2^-9 of their weight apart inside it (w < 1.26 * 2^e, step 1.3 * 2^-9 * 2^e):
    these are the structures of the difference-term mutations"""
    out, left, i = [], nblocks, 0
    while left > 0:
        k = min((1, 1, 2, 1, 3, 2)[i % 6], left)
        out.append((_bucket_w((i // 5) % 4 - 1, (i // 5 * 5) % 16, i % 5, 1.3 * 2.0 ** -9), 64 * k - 1 - 3 * (i % 7)))
        left -= k
        i += 1
    return out


def cost_model_S(meta, fold64, n=40, nwaves=2048):
    """gcls_cost_classes: the number of K ranges the library takes (nwaves = 8 waves on each of 256 CUs)"""
    nrt = (n + 31) // 32
    nI = (nrt + 1) // 2
    nun = sum(1 for I in range(nI) for J in range(nI) if 2 * J + 1 >= 2 * I)
    t_class, t_block = (0.136, 0.079) if fold64 else (0.045, 0.067)
    best, bestS = -1.0, 2
    for S in range(2, 33, 2):
        if meta.nblocks // S < 4 and S > 2:
            break
        rounds = -(-nun * S // nwaves)
        per = (meta.nruns / S + 1.0) * 4 * t_class + (-(-meta.nblocks // S)) * 4 * t_block + 6.0
        cost = rounds * per + S * nun * 8.5e-3
        if best < 0 or cost < best * 0.995:
            best, bestS = cost, S
    return bestS


def _k_ranges():
    for nblocks in (1, 2, 3, 7, 8, 9, 25, 33, 49, 127, 128, 129):  # (25, 33, 49: S = 6, 8, 12, between the 2 and the 26 .. 32 of the others)
        st = ranges_structure(nblocks)

        def edge(meta, nblocks=nblocks, st=st):
            assert meta.nblocks == nblocks and meta.nruns == len(st) <= 200
            same = meta.group[1:] == meta.group[:-1]
            assert not same.any() or (np.diff(meta.wkey)[same] / meta.wkey[1:][same]).min() >= 2.0 ** -9 * (1 - 2.0 ** -20)
            seen = set()
            for S in {cost_model_S(meta, True), cost_model_S(meta, False)}:
                assert S == 2 or nblocks // S >= 4
                for p0, p1 in meta.ranges(S):
                    if p0 == p1:
                        seen.add("empty")
                    elif p0 == 0:
                        continue
                    elif meta.cls[2 * p0] == meta.cls[2 * p0 - 1]:
                        seen.add("in class")
                    else:
                        seen.add({1: "in group", 2: "on group end"}[int(meta.flag2[2 * p0 - 1])])
                if nblocks % 2:
                    assert meta.ranges(S)[-1][1] * 2 == nblocks + 1  # the last range ends on the padding block
            if nblocks == 1:
                assert seen == {"empty"}
            if nblocks >= 127:
                assert seen == {"in class", "in group", "on group end"}, seen

        CASES.append(Case(f"ranges_{nblocks}", "K ranges", st, 40, edge))


TILE_N = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 257]
TILE_STRUCTURE = [(_bucket_w(i // 5 % 3, (11 * (i // 5)) % 64, i % 5), 100 + ((37 * i) % 71) - 35) for i in range(40)]


def _tile_edges():
    def edge(meta):
        assert meta.nruns == 40 and 3800 <= len(meta.w) <= 4200 and _ngroups(meta) == 8

    for n in TILE_N:
        CASES.append(Case(f"tiles_{n}", "tile edges", TILE_STRUCTURE, n, edge, seed=100 + n))
    CASES.append(Case("tiles_store", "tile edges", TILE_STRUCTURE + [(_bucket_w(0, 40, i), 80) for i in range(5)], 150,
                      lambda meta: None, seed=99))


def _long_run():
    lo = [(_bucket_w(-2, (3 * (i // 6)) % 64, i % 6), 64 + (i * 29) % 150) for i in range(300)]
    hi = [(_bucket_w(2, (3 * (i // 6)) % 64, i % 6), 64 + (i * 31) % 150) for i in range(60)]
    nlo = sum((c + 63) // 64 for _, c in lo)
    lo.append((0.25 * (1 + 22 / 64.0 + 2.0 ** -9), 64 * (1 - nlo % 2)))  # the long class starts on an odd block
    lo = [s for s in lo if s[1] > 0]
    long_blocks = GCLS_GRUN + 2100

    def edge(meta):
        r = int(np.argmax(meta.nblk))
        assert meta.nblk[r] == long_blocks > GCLS_GRUN and r == len(lo) and meta.nruns == len(st)
        assert meta.blk_start[r] % 2 == 1 and 0 < meta.blk_start[r] < GCLS_GRUN < meta.blk_start[r] + meta.nblk[r]
        mid = meta.blk_start[r] + GCLS_GRUN - 1
        assert meta.flag2[mid] == 2 and meta.flag64[mid] == 0  # the mid-class fold of the mixed kernel only
        last = meta.blk_start[r] + meta.nblk[r] - 1
        assert meta.flag2[last] == 2 and meta.group[r + 1] == meta.group[r] + 1  # the forced group end ...
        assert meta.key[r] >> np.uint64(46) == meta.key[r + 1] >> np.uint64(46) and r % GCLS_GMAX != GCLS_GMAX - 1  # ... and nothing else ends it
        assert 1.1e6 < len(meta.w) < 1.3e6

    # the first class after the long one shares its bucket, so that only the crossing of a multiple of GCLS_GRUN ends the group
    st = lo + [(1.0 + 2.0 ** -9, 64 * long_blocks - 17), (1.0 + 2.0 ** -8, 70)] + hi
    CASES.append(Case("long_run", "long runs", st, 40, edge, seed=7))


_block_edges()
_group_edges()
_k_ranges()
_tile_edges()
_long_run()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
