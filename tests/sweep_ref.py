"""Panels, an exact reference, a derived bound and fault models for the FP64 sweeps of csrc/pca.hip (tpg_sweep_kernel,
run_sweep):  out[row][k] = sum_col z(row, col) Tab[col][k] (/ d[k]),  rss[row] = sum_col z(row, col)^2,  z = (g - center) / scale
for a typed genotype and 0 for a missing one ("colscale": center / scale belong to the column, rows = individuals; "rowscale":
they belong to the row, rows = loci, the Z'U / d of the loadings; "valid": z = 1 for a typed genotype).

Exact panels.  center is a multiple of 1/4 in [0, 2], scale one of 1/4, 1/2, 1, 2, 4, Tab holds integers with |t| <= 2^20 and d
powers of two.  The device forms inv = 1.0 / scale (a power of two: exact), g - center (a multiple of 1/4, |.| <= 2: exact) and
z = (g - center) inv (a multiple of 2^-4, |z| <= 8: exact).  Every product z t is then an integer multiple of 2^-4 below 2^24
<= 2^26, and a sum of at most 2^15 of them -- in any order, over any cut into splits, with or without fused multiply-adds -- stays
an integer multiple of 2^-4 below 2^41 < 2^53 2^-4: every partial sum is a double, no addition rounds.  z^2 is a multiple of 2^-8
no larger than 2^6 < 2^8 and a sum of 2^15 of them stays below 2^23 = 2^31 2^-8.  The division by a power of two is exact as
well.  So whatever order the device adds in, its result equals sweep_exact() in every bit, and a kernel that drops, doubles or
misplaces one term cannot hide behind a tolerance.  tests/test_sweep_host.py shows both halves on the host: three orders of
float64 addition give sweep_exact() bit for bit, and every entry of FAULTS moves some element.

General panels.  Real center / scale (the binomial scaling of the panel), Gaussian Tab, d from linspace.  sweep_bound() is
derived, not measured: with u = 2^-53 the device's z carries three roundings (g - center, 1 / scale, their product), a term z t
one more, the N - 1 additions of a row (the two halves of a row and the splits included: they are additions of the same sum)
at most (N - 1) u of sum |z t| to first order, the division by d one: (N + 4) u, and N + 8 leaves room for the second-order
terms.  For rss, z^2 carries 2 * 3 + 1 roundings: (N + 6) u, again within N + 8.  sweep_fraction() is the reference there: the
same sums in rational arithmetic, rounded once.

run_sweep's launch rule is restated in splits() / split_bounds(): the column blocks of 128 are cut into S ranges
[nblocks s / S, nblocks (s + 1) / S) (integer division: unequal lengths); S starts at 1 and doubles while
ceil(nrowtiles / 4) S < 4 CUs, 2 S <= nblocks and S < 64.  The K columns go in passes of KC = 4 (K <= 4) or 20.
"""
from fractions import Fraction

import numpy as np

KC_LARGE = 20
MODES = ("colscale", "rowscale", "valid")
SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)
KMAX = 64


# ---------------------------------------------------------------------------------------------------------------------
# run_sweep's launch rule
def dims(mode, n, m):
    """(nrowtiles, nblocks, nrows, ncols) of the sweep for a view of n individuals and m loci"""
    Q, KG = -(-n // 128), -(-m // 128)
    return (4 * KG, Q, m, n) if mode == "rowscale" else (4 * Q, KG, n, m)


def splits(mode, n, m, num_cu=256):
    nrowtiles, nblocks, _, _ = dims(mode, n, m)
    row_blocks = -(-nrowtiles // 4)
    S = 1
    while row_blocks * S < 4 * num_cu and S * 2 <= nblocks and S < 64:
        S *= 2
    return S


def split_bounds(nblocks, S):
    return [(nblocks * s // S, nblocks * (s + 1) // S) for s in range(S)]


def passes(K):
    KC = 4 if K <= 4 else KC_LARGE
    return [(k0, min(KC, K - k0)) for k0 in range(0, K, KC)]


# ---------------------------------------------------------------------------------------------------------------------
class Panel:
    """G (n x m, codes 0 1 2 and 3 = missing), center / scale (m: per locus, the column of "colscale" and the row of
    "rowscale"), V (m x KMAX: the Tab of the T-layout modes), U (n x KMAX: the Tab of "rowscale"), d (KMAX)"""

    def __init__(self, G, center, scale, V, U, d):
        self.G, self.center, self.scale, self.V, self.U, self.d = G, center, scale, V, U, d
        self.n, self.m = G.shape
        for a in (G, center, scale, V, U, d):
            a.setflags(write=False)

    def args(self, mode, K):
        """(G, center, scale, Tab, d) of one sweep: what sweep_exact, sweep_model and the faults take"""
        if mode == "rowscale":
            return self.G, self.center, self.scale, np.asfortranarray(self.U[:, :K]), self.d[:K]
        return self.G, self.center, self.scale, np.asfortranarray(self.V[:, :K]), None


def _plant_missing(rng, G, miss):
    n, m = G.shape
    if miss <= 0:
        return
    G[rng.random((n, m)) < miss] = 3
    i, j = np.arange(n), np.arange(m)
    # both sides of every boundary of a 128-block and of a 32-tile, along both axes (either axis is the rows of some mode)
    for step in (32, 128):
        for b in range(step, m, step):
            G[i % 3 == 0, b - 1] = 3
            G[i % 3 == 1, b] = 3
        for b in range(step, n, step):
            G[b - 1, j % 3 == 0] = 3
            G[b, j % 3 == 1] = 3
    if n >= 3 and m >= 3:
        G[n - 1, j % 5 == 2] = 3  # the last row and the last column: some, not all
        G[i % 5 == 2, m - 1] = 3
        G[n - 1, m - 1] = rng.integers(0, 3)  # (the corner stays typed: the last row meets the last column's Tab entries)
        G[n // 2, :] = 3  # typed nowhere
        G[:, m // 3] = 3
        assert n // 2 != n - 1 and m // 3 != m - 1


def _tables(rng, n, m):
    k = np.arange(KMAX)
    out = []
    for rows in (m, n):
        base = rng.integers(-2 ** 13, 2 ** 13, rows)
        T = (k[None, :] + 1) * base[:, None] + k[None, :]  # column k = (k + 1) base + k: no two columns alike
        T[rows - 1] = 2 ** 19 + 17 * k + 1  # the last valid row: large and odd one out, so that losing it shows everywhere
        assert np.abs(T).max() <= 2 ** 20
        out.append(np.asfortranarray(T.astype(np.float64)))
    return out


def exact_panel(seed, n, m, miss):
    """see the module docstring.  n or m below 3 leave out the planted rows and columns (a 1 x 1 panel is one typed genotype)"""
    rng = np.random.default_rng([seed, n, m])
    G = rng.integers(0, 3, (n, m)).astype(np.uint8)
    _plant_missing(rng, G, miss)
    center = rng.integers(0, 9, m) / 4.0
    scale = np.array(SCALES)[rng.integers(0, len(SCALES), m)]
    V, U = _tables(rng, n, m)
    d = np.exp2(((7 * np.arange(KMAX)) % 11 - 5).astype(np.float64))  # d[k], d[k - 20], d[k - 40], d[k - 60] all differ
    return Panel(G, center, scale, V, U, d)


def general_panel(seed, n, m, miss):
    rng = np.random.default_rng([seed, n, m, 1])
    p = rng.uniform(0.05, 0.95, m)
    G = rng.binomial(2, p[None, :], (n, m)).astype(np.uint8)
    _plant_missing(rng, G, miss)
    typed = G != 3
    # snp_scaleBinom on the typed genotypes; a locus it cannot scale (typed nowhere, or one allele only) gets p = 1/2
    cnt = np.maximum(typed.sum(0), 1)
    center = np.where(typed, G, 0).sum(0) / cnt
    center = np.where((center > 0) & (center < 2), center, 1.0)
    scale = np.sqrt(2 * (center / 2) * (1 - center / 2))
    V = np.asfortranarray(rng.standard_normal((m, KMAX)))
    U = np.asfortranarray(rng.standard_normal((n, KMAX)))
    d = np.linspace(9.0, 2.0, KMAX)
    return Panel(G, center, scale, V, U, d)


# ---------------------------------------------------------------------------------------------------------------------
def _is_pow2(x):
    mant, _ = np.frexp(x)
    return bool(np.all(mant == 0.5))


def sweep_exact(mode, G, center, scale, Tab, d=None):
    """(out, rss) of an exact panel from integer sums: z 2^4 and Tab are integers, the sums are taken in int64 (checked
    against overflow by their majorant) and converted once.  rss is None outside "colscale" (the device returns none)."""
    assert mode in MODES
    Gi = np.asarray(G).astype(np.int64)
    typed = Gi != 3
    assert Gi.min() >= 0 and Gi.max() <= 3
    Ti = np.asarray(Tab).astype(np.int64)
    assert np.array_equal(Ti.astype(np.float64), Tab) and np.abs(Ti).max() <= 2 ** 20, "Tab is not on the exact grid"
    if mode == "valid":
        Z, shift = typed.astype(np.int64), 0
    else:
        c4 = np.asarray(center * 4).astype(np.int64)
        i4 = np.asarray(4.0 / scale).astype(np.int64)
        assert np.array_equal(c4 / 4.0, center) and c4.min() >= 0 and c4.max() <= 8, "center is not on the exact grid"
        assert np.array_equal(4.0 / i4, scale) and set(scale.tolist()) <= set(SCALES), "scale is not on the exact grid"
        Z, shift = np.where(typed, (4 * Gi - c4[None, :]) * i4[None, :], 0), 4  # 16 z
        if mode == "rowscale":
            Z = np.ascontiguousarray(Z.T)
    assert Z.shape[1] == Ti.shape[0]
    assert Z.shape[1] * int(np.abs(Z).max()) * int(np.abs(Ti).max()) < 2 ** 53  # no int64 overflow, and a double holds it
    sums = Z @ Ti  # integer arithmetic
    out = np.ldexp(sums.astype(np.float64), -shift)
    if d is not None:
        assert _is_pow2(d), "d is not on the exact grid"
        out = out / np.asarray(d)[None, :]  # a power of two: exact
    rss = np.ldexp((Z * Z).sum(axis=1).astype(np.float64), -2 * shift) if mode == "colscale" else None
    return np.asfortranarray(out), rss


def _fr(x):
    return Fraction(float(x))


def sweep_fraction(mode, G, center, scale, Tab, d=None):
    """(out, rss) in rational arithmetic from the doubles as they are (z = (g - center) / scale, no rounded reciprocal),
    rounded once at the end: the reference of the general panels"""
    assert mode in MODES
    G = np.asarray(G)
    n, m = G.shape
    nrows, ncols = (m, n) if mode == "rowscale" else (n, m)
    K = Tab.shape[1]
    T = [[_fr(Tab[c, k]) for k in range(K)] for c in range(ncols)]
    cF, sF = [_fr(c) for c in center], [_fr(s) for s in scale]
    out = np.zeros((nrows, K), order="F")
    rss = np.zeros(nrows) if mode == "colscale" else None
    for r in range(nrows):
        z = []
        for c in range(ncols):
            g, j = (G[c, r], r) if mode == "rowscale" else (G[r, c], c)
            z.append(Fraction(0) if g == 3 else Fraction(1) if mode == "valid" else (int(g) - cF[j]) / sF[j])
        for k in range(K):
            s = sum((z[c] * T[c][k] for c in range(ncols) if z[c]), Fraction(0))
            out[r, k] = float(s / _fr(d[k])) if d is not None else float(s)
        if rss is not None:
            rss[r] = float(sum((zc * zc for zc in z), Fraction(0)))
    return out, rss


def _zmat(mode, G, center, scale, missing_as_3=False, neighbour=False):
    """z as the device forms it (float64: inv = 1 / scale, then (code - center) inv), rows x columns of the sweep"""
    G = np.asarray(G)
    code = G.astype(np.float64)
    if mode == "valid":
        Z = np.ones(G.shape)
    else:
        c, inv = np.asarray(center, dtype=np.float64), 1.0 / np.asarray(scale, dtype=np.float64)
        if neighbour:  # locus j reads the center and scale of locus j - 1 (locus 0 keeps its own)
            idx = np.maximum(np.arange(len(c)) - 1, 0)
            c, inv = c[idx], inv[idx]
        Z = (code - c[None, :]) * inv[None, :]
    if not missing_as_3:
        Z = np.where(G == 3, 0.0, Z)
    return np.ascontiguousarray(Z.T) if mode == "rowscale" else Z


def sweep_bound(mode, G, center, scale, Tab, d=None):
    """(bound of out, bound of rss), elementwise: (N + 8) 2^-53 sum |z t| (/ |d|) and (N + 8) 2^-53 sum z^2, N the columns"""
    Z = _zmat(mode, G, center, scale)
    f = (Z.shape[1] + 8) * 2.0 ** -53
    b = f * (np.abs(Z) @ np.abs(Tab))
    if d is not None:
        b = b / np.abs(d)[None, :]
    return b, (f * (Z * Z).sum(axis=1) if mode == "colscale" else None)


def excess(got, ref, bound):
    """largest |got - ref| / bound over the elements of out and of rss (where there is one): <= 1 = inside the bound.  Where
    the bound is 0 (a row typed nowhere: every term is 0) any error at all counts as infinite."""
    worst = 0.0
    for g, r, b in zip(got, ref, bound):
        if r is None:
            continue
        assert g is not None and g.shape == r.shape == b.shape
        err = np.abs(g - r)
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
        worst = max(worst, float(ratio.max()))
    return worst


def sweep_model(mode, G, center, scale, Tab, d=None, order="forward", S=1):
    """the same sums in float64, one column after the other: "forward", "reversed", or "split": the blocks of 128 columns cut
    into run_sweep's S ranges, each summed forward, the ranges then added in turn (the reduce kernel)"""
    Z = _zmat(mode, G, center, scale)
    nrows, ncols = Z.shape
    K = Tab.shape[1]

    def run(cols):
        acc, rs = np.zeros((nrows, K)), np.zeros(nrows)
        for c in cols:
            acc += Z[:, c, None] * Tab[c][None, :]
            rs += Z[:, c] * Z[:, c]
        return acc, rs

    if order == "split":
        nblocks = -(-ncols // 128)
        acc, rs = np.zeros((nrows, K)), np.zeros(nrows)
        for b0, b1 in split_bounds(nblocks, S):
            a, r = run(range(128 * b0, min(128 * b1, ncols)))
            acc += a
            rs += r
    else:
        acc, rs = run(range(ncols) if order == "forward" else range(ncols - 1, -1, -1))
    if d is not None:
        acc = acc / np.asarray(d)[None, :]
    return acc, (rs if mode == "colscale" else None)


# ---------------------------------------------------------------------------------------------------------------------
# Fault models: what one specific wrong kernel or launcher would return.  f(mode, G, center, scale, Tab, d, S) -> (out, rss);
# NotApplicable(reason) where the wrong code would run no differently from the right one.
class NotApplicable(Exception):
    pass


def _finish(mode, Z, Tab, d):
    out = Z @ Tab
    if d is not None:
        out = out / np.asarray(d)[None, :]
    return out, ((Z * Z).sum(axis=1) if mode == "colscale" else None)


def last_column_dropped(mode, G, center, scale, Tab, d, S):
    Z = _zmat(mode, G, center, scale)
    Z[:, -1] = 0
    return _finish(mode, Z, Tab, d)


def last_block_dropped(mode, G, center, scale, Tab, d, S):
    Z = _zmat(mode, G, center, scale)
    Z[:, 128 * ((Z.shape[1] - 1) // 128):] = 0
    return _finish(mode, Z, Tab, d)


def split_off_by_one_block(mode, G, center, scale, Tab, d, S):
    """the second range starts one block late: block nblocks / S (integer division) belongs to nobody"""
    if S < 2:
        raise NotApplicable("one range: there is no boundary between ranges")
    Z = _zmat(mode, G, center, scale)
    b = split_bounds(-(-Z.shape[1] // 128), S)[1][0]
    Z[:, 128 * b:128 * (b + 1)] = 0
    return _finish(mode, Z, Tab, d)


def _needs_second_pass(Tab):
    if Tab.shape[1] <= KC_LARGE:
        raise NotApplicable("K <= 20: one pass")


def pass_reads_tab_of_pass_0(mode, G, center, scale, Tab, d, S):
    _needs_second_pass(Tab)
    Z = _zmat(mode, G, center, scale)
    return _finish(mode, Z, Tab[:, np.arange(Tab.shape[1]) % KC_LARGE], d)


def rss_from_last_pass(mode, G, center, scale, Tab, d, S):
    """The kernel forms z again in every pass and z does not depend on Tab: the rss of the last pass is the rss of the first,
    the same additions in the same order.  A launcher that took it from the last pass would return the right bits (and spend a
    buffer write per extra pass); no test can or need tell it apart.  What CAN go wrong with rss over passes is
    rss_added_in_every_pass below."""
    raise NotApplicable("z does not depend on the pass: every pass would give the same rss")


def rss_added_in_every_pass(mode, G, center, scale, Tab, d, S):
    """every pass adds its rss to the output, not the first alone"""
    if mode != "colscale":
        raise NotApplicable("no rss is returned in this mode")
    _needs_second_pass(Tab)
    out, rss = _finish(mode, _zmat(mode, G, center, scale), Tab, d)
    return out, rss * len(passes(Tab.shape[1]))


def missing_counted_as_3(mode, G, center, scale, Tab, d, S):
    if not (np.asarray(G) == 3).any():
        raise NotApplicable("no missing genotype in the panel")
    return _finish(mode, _zmat(mode, G, center, scale, missing_as_3=True), Tab, d)


def center_scale_of_neighbour(mode, G, center, scale, Tab, d, S):
    if mode == "valid":
        raise NotApplicable("no center or scale in this mode")
    if len(center) < 2:
        raise NotApplicable("one locus: no neighbour")
    return _finish(mode, _zmat(mode, G, center, scale, neighbour=True), Tab, d)


def padded_rows_one_up(mode, G, center, scale, Tab, d, S):
    """the rows of the last 32-tile past the end (padding: code 3, z = 0, sums 0) land one row up: on the last valid row"""
    Z = _zmat(mode, G, center, scale)
    if Z.shape[0] % 32 == 0:
        raise NotApplicable("the rows fill their last 32-tile: no padded row")
    out, rss = _finish(mode, Z, Tab, d)
    out[-1] = 0
    if rss is not None:
        rss[-1] = 0
    return out, rss


def col_div_of_pass_0(mode, G, center, scale, Tab, d, S):
    if d is None:
        raise NotApplicable("no col_div in this mode")
    _needs_second_pass(Tab)
    return _finish(mode, _zmat(mode, G, center, scale), Tab, np.asarray(d)[np.arange(len(d)) % KC_LARGE])


FAULTS = [last_column_dropped, last_block_dropped, split_off_by_one_block, pass_reads_tab_of_pass_0, rss_from_last_pass,
          rss_added_in_every_pass, missing_counted_as_3, center_scale_of_neighbour, padded_rows_one_up, col_div_of_pass_0]


# ---------------------------------------------------------------------------------------------------------------------
# The grid of tests/test_gpu_sweep.py (and of the host proofs in tests/test_sweep_host.py).  S is for 256 CUs.
# 769 loci are SEVEN blocks (6 * 128 = 768), cut 1 / 2 / 2 / 2 by S = 4; 767 loci are the six blocks cut 1 / 2 / 1 / 2.
T_SHAPES = {(1, 1): 1, (31, 127): 1, (32, 128): 1, (33, 129): 2, (129, 130): 2, (130, 769): 4, (130, 12805): 64, (260, 1153): 8,
            (130, 767): 4}
L_SHAPES = {(5, 40): 1, (128, 129): 1, (130, 257): 2, (643, 300): 4, (136, 289): 2}
KS = (1, 4, 5, 20, 21, 40, 41, 64)
# every shape at K = 4 and 21; every K on a shape with S > 1 and on a ragged one (every shape but (32, 128) is ragged)
T_EXTRA = {1: [(33, 129), (130, 12805)], 5: [(129, 130), (130, 767)], 20: [(130, 769), (260, 1153)], 40: [(260, 1153), (33, 129)],
           41: [(130, 12805), (130, 767)], 64: [(130, 769), (33, 129)]}
L_EXTRA = {1: [(130, 257)], 5: [(643, 300)], 20: [(136, 289)], 40: [(130, 257)], 41: [(643, 300)], 64: [(136, 289)]}
MISS = 0.03
SEED = 7


def grid(shapes, extra):
    cases = [(n, m, K) for (n, m) in shapes for K in (4, 21)]
    cases += [(n, m, K) for K, nm in extra.items() for (n, m) in nm]
    return cases


T_CASES = grid(T_SHAPES, T_EXTRA)
L_CASES = grid(L_SHAPES, L_EXTRA)
GENERAL = {"colscale": (33, 129), "valid": (33, 129), "rowscale": (130, 257)}  # ragged, S = 2; K = 21

_panels = {}


def panel(kind, n, m, miss=MISS):
    key = (kind, n, m, miss)
    if key not in _panels:
        _panels[key] = (exact_panel if kind == "exact" else general_panel)(SEED, n, m, miss)
    return _panels[key]
