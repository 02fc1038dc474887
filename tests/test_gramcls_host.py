"""CPU: the bounds of tests/gramcls_ref.py have teeth, and its class table is the device's.

tests/test_gpu_gramcls.py holds the class Gram kernels to elementwise bounds derived from their arithmetic.  Here, without a
GPU: every structure of its case table shows the edge it was built for (Case.build asserts it on the restated table); a numpy
model of the two folding schemes stays inside the bound of its kernel for every cut into K ranges; the same model with ONE
slip -- a locus, a flag, a weight, a difference term, a block pair -- leaves the bound at some element of the structure
named beside it; and the table agrees with a second, loop-by-loop computation of sort, group and cut.
"""
import collections
import struct

import numpy as np
import pytest

from tests import gramcls_ref as gr

N_MODEL = 12  # individuals of the model runs: the class table does not depend on it

_cache = {}


def _case(name, n=N_MODEL):
    if (name, n) not in _cache:
        c = gr.BY_NAME[name]
        g, scale, meta = c.build(n=min(c.n, n))
        _cache[(name, n)] = (g, scale, meta, gr.exact(g, scale))
    return _cache[(name, n)]


def _rel(meta, kernel, table=False):
    return gr.rel_fold64(meta) if kernel == "fold64" else gr.rel_mixed_table(meta) if table else gr.rel_mixed(meta)


def _excess(K, R, rel):
    """largest |K - R| - rel R over the elements, in units of max R: positive = some element has left the bound"""
    return float((np.abs(K.astype(gr.LD) - R) - gr.LD(rel) * R).max() / R.max())


@pytest.mark.parametrize("name", [c.name for c in gr.CASES])
def test_every_case_shows_its_edge(name):
    c = gr.BY_NAME[name]
    g, scale, meta = c.build(n=min(c.n, 3))  # (asserts the edge)
    assert g.shape[1] == len(scale) == sum(s[1] for s in c.structure) and g.max() <= 2
    assert np.all(g.min(axis=0) != g.max(axis=0)) if g.shape[0] > 1 else np.all(g == 1)
    assert np.allclose(np.sort(1.0 / (scale * scale)), np.sort(np.repeat([s[0] for s in c.structure], [s[1] for s in c.structure])), rtol=1e-15)


_distinct = {}
for _c in gr.CASES:
    if _c.family != "long runs":
        _distinct.setdefault(id(_c.structure), _c.name)


@pytest.mark.parametrize("name", list(_distinct.values()))
def test_model_stays_inside_the_bounds(name):
    g, scale, meta, R = _case(name)
    assert meta.nruns <= 300
    for kernel in ("fold64", "mixed"):
        rel = _rel(meta, kernel, table=True)  # (the sharper bound of the mixed kernel, which the GPU file uses)
        assert rel <= _rel(meta, kernel)
        for S in (2, 4, 32):
            if S > max(2, meta.nblocks // 4):
                continue
            K = gr.model(g, meta, kernel, S)
            assert np.array_equal(K, K.T)
            assert _excess(K, R, rel) <= 0, (name, kernel, S, _excess(K, R, rel))
            # the centred call: H K H against H R H, without the device's own rounding of the centring
            Kc = np.asarray(gr.centre(K), dtype=np.float64)
            assert np.abs(Kc - gr.centre(R)).max() <= gr.bound_centred(rel, R, g.shape[0], gr.centred_majorant(g, meta))


def _first(meta, flag):
    return int(np.nonzero(meta.flag2 == flag)[0][0])


def _site_class_end_in_group(meta):
    """a class that ends inside a group (flag 1) with the next block in the same K range for S = 2"""
    b = [b for b in np.nonzero(meta.flag2 == 1)[0] if b + 2 < 2 * (meta.npairs // 2)]
    return int(meta.cls[b[len(b) // 2]])


def _S_range_end_on_class_end(meta):
    """an S whose range ends fall on a class end inside a group"""
    for S in range(2, 33, 2):
        if any(0 < p1 < meta.npairs and p0 < p1 and meta.flag2[2 * p1 - 1] == 1 for p0, p1 in meta.ranges(S)):
            return S
    raise AssertionError("no K range of this structure ends on a class end inside a group")


# mutation, structure built for it, kernels, S, site
MUTANTS = [
    ("drop_last_locus_of_class", "blocks_group_odd", ("fold64", "mixed"), 2, lambda me: 4),       # the class of 127 loci
    ("drop_first_locus_of_block", "blocks_bucket_even", ("fold64", "mixed"), 2, lambda me: 10),   # the middle block of 129 loci
    ("pad_read_as_one", "blocks_group_even", ("fold64", "mixed"), 2, lambda me: 0),               # the class of one locus
    ("neighbour_weight", "ranges_9", ("fold64", "mixed"), 2, lambda me: int(me.cls[_first(me, 2)])),  # the first group's last class
    ("omit_delta", "ranges_129", ("mixed",), 2, _site_class_end_in_group),
    ("delta_one_block_late", "ranges_129", ("mixed",), 2, _site_class_end_in_group),
    ("range_end_next_weight", "ranges_127", ("mixed",), None, lambda me: None),
    ("pair_in_both", "ranges_8", ("fold64", "mixed"), 2, lambda me: 1),
    ("pair_in_neither", "ranges_8", ("fold64", "mixed"), 2, lambda me: 1),
]


@pytest.mark.parametrize("mut,name,kernels,S,site", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_each_mutation_leaves_the_bound(mut, name, kernels, S, site):
    g, scale, meta, R = _case(name)
    if S is None:
        S = _S_range_end_on_class_end(meta)
    at = site(meta)
    for kernel in kernels:
        rel = _rel(meta, kernel)
        assert _excess(gr.model(g, meta, kernel, S), R, rel) <= 0
        ex = _excess(gr.model(g, meta, kernel, S, mut, at), R, rel)
        # out of the bound, and not by a hair: the smallest slip here is a weight step of 2^-9 on one block of 129,
        # 2^-9 / 129 = 1.5e-5 of an element against a bound of 6e-8
        assert ex > 10 * rel, (mut, name, kernel, S, at, ex, rel)


def test_difference_term_structures_are_spaced():
    """what makes one wrong FP32 term visible over rel_mixed's 6e-8: in-group weights 2^-9 apart, at most 200 classes"""
    for name in ("ranges_127", "ranges_129"):
        _, _, meta, _ = _case(name)
        same = meta.group[1:] == meta.group[:-1]
        assert meta.nruns <= 200 and (np.diff(meta.wkey)[same] / meta.wkey[1:][same]).min() >= 2.0 ** -9 * (1 - 2.0 ** -20)


def test_flag_on_the_padding_block_changes_nothing():
    """The entry that pads an odd block list carries no flag.  A flag there -- the last class's, copied or moved from the
    last real block -- CANNOT leave a bound, and the model shows why: the padding block is empty, the last real block of the
    list is always a full fold (r == nr - 1), and the fold after the loop takes the key of the padding entry, which is the
    last class's: with the flag copied the extra fold adds zero sums, with the flag moved the same sums are folded with the
    same key one (empty) block later.  So this pins bitwise invariance, on the odd structure built for the padding entry; what
    a wrong padding entry can break -- its KEY, or a non-empty padding block -- is caught by pad_read_as_one and by the
    GPU cases with an odd block count."""
    g, scale, meta, R = _case("blocks_group_odd")
    assert meta.nblocks % 2 == 1
    for S in (2, 4):
        K = gr.model(g, meta, "mixed", S)
        for mut in ("pad_block_flagged", "pad_block_takes_flag"):
            assert np.array_equal(gr.model(g, meta, "mixed", S, mut), K)


def test_omitted_mid_class_fold_saturates():
    """One class of more than 2 * 2^16 blocks in which individual 0 is homozygous throughout: each of the two K ranges adds
    256 per block to its FP32 sum of the pair (0, 0).  With the folds every GCLS_GRUN blocks the sums stay below 2^22; without
    them they pass 2^24, where an FP32 accumulator stops counting (modelled as saturation)."""
    blocks = 2 * gr.GCLS_MAX_RUN + 700
    m = 64 * blocks - 5
    g = np.empty((2, m), dtype=np.uint8, order="F")
    g[0], g[1] = 2, 1
    scale = np.full(m, 0.7)
    meta = gr.describe(scale)
    assert meta.nruns == 1 and meta.nblocks == blocks and meta.F2 == blocks // gr.GCLS_GRUN + 1
    R = gr.exact(g, scale)
    rel = gr.rel_mixed(meta)
    assert _excess(gr.model(g, meta, "mixed", 2), R, rel) <= 0
    assert _excess(gr.model(g, meta, "mixed", 2, "omit_grun_fold"), R, rel) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------
def _brute_table(scale):
    """sort, group, cut: the class table once more, locus by locus and block by block in Python integers"""
    keys = []
    for sc in scale:
        w = 1.0 / (float(sc) * float(sc))
        bits = struct.unpack("<Q", struct.pack("<d", w))[0]
        keys.append((bits + 16) & ~31)
    counts = collections.Counter(keys)
    uk = sorted(counts)
    flag64, flag2, delta, cls = [], [], [], []
    start = 0
    for r, k in enumerate(uk):
        nblk = -(-counts[k] // 64)
        ends_group = (r == len(uk) - 1 or (k >> 46) != (uk[r + 1] >> 46) or r % 64 == 63 or start // 16384 != (start + nblk) // 16384)
        for o in range(nblk):
            last = o == nblk - 1
            flag64.append(1 if last or o % 65536 == 65535 else 0)
            full = o % 16384 == 16383 or (last and ends_group)
            flag2.append(2 if full else 1 if last else 0)
            d = 0.0
            if last and not full:
                d = struct.unpack("<d", struct.pack("<Q", k))[0] - struct.unpack("<d", struct.pack("<Q", uk[r + 1]))[0]
            delta.append(np.float32(d))
            cls.append(r)
        start += nblk
    by_key = collections.defaultdict(list)
    for j, k in enumerate(keys):
        by_key[k].append(j)
    src = []
    for k in uk:
        src += by_key[k] + [-1] * (-len(by_key[k]) % 64)
    return uk, [counts[k] for k in uk], flag64, flag2, delta, cls, src


def _same_table(scale):
    meta = gr.describe(scale)
    uk, counts, flag64, flag2, delta, cls, src = _brute_table(scale)
    assert meta.key.tolist() == uk and meta.count.tolist() == counts
    assert meta.flag64.tolist() == flag64 and meta.flag2.tolist() == flag2 and meta.cls.tolist() == cls
    assert np.array_equal(meta.delta, np.array(delta, dtype=np.float32))
    assert meta.src.tolist() == src
    return meta


@pytest.mark.parametrize("seed", range(6))
def test_table_against_brute_force_random(seed):
    rng = np.random.default_rng(seed)
    nw = int(rng.integers(1, 150))
    w = np.exp2(rng.uniform(-10, 12, nw))
    w[: nw // 3] = 2.0 + rng.integers(0, 40, nw // 3) * 2.0 ** -11  # many classes in and around one bucket
    m = int(rng.integers(nw, 6000))
    scale = 1.0 / np.sqrt(w[rng.integers(0, nw, m)])
    _same_table(scale)


def test_table_key_rounding():
    """keys that carry into the exponent; weights closer than 2^-47 are one class, further apart than 2^-46 two"""
    def scale_of(bits):  # a scale whose float64 weight 1 / scale^2 has exactly these bits (searched for among its neighbours)
        w = struct.unpack("<d", struct.pack("<Q", bits))[0]
        lo = hi = 1.0 / np.sqrt(w)
        for _ in range(6):
            for s in (lo, hi):
                if 1.0 / (s * s) == w:
                    return s
            lo, hi = np.nextafter(lo, 0.0), np.nextafter(hi, np.inf)
        return None

    four = struct.unpack("<Q", struct.pack("<d", 4.0))[0]
    got = {}
    for d in range(-40, 41):  # not every double is 1 / s^2 for some double s: take those that are
        s = scale_of(four + d)
        if s is not None:
            got[d] = s
    below = [d for d in got if -16 <= d < 0]
    assert below, "no weight within 16 units below 4.0"
    meta = _same_table(np.array([got[below[0]]] * 70 + [got[max(d for d in got if d > 16)]] * 3))
    assert meta.wkey[0] == 4.0 and meta.w.min() < 4.0  # the key carried into the exponent
    one = struct.unpack("<Q", struct.pack("<d", 1.0))[0]
    got = {d: scale_of(one + d) for d in range(0, 200)}
    got = {d: s for d, s in got.items() if s is not None}
    # just above 1.0 a unit in the last place is 2^-52 of the weight: 2^-47 is 32 units, 2^-46 is 64.  A class is a cell of 32
    # units around a multiple of 32, so two weights less than 2^-47 apart share a class when no cell edge lies between them
    # (the pair is chosen so), and two weights more than 2^-46 apart never do
    close = [(a, b) for a in got for b in got if 0 < b - a < 32 and (a + 16) // 32 == (b + 16) // 32]
    far = [(a, b) for a in got for b in got if b - a > 64 + 1]
    assert close and far
    a, b = max(close, key=lambda ab: ab[1] - ab[0])
    assert _same_table(np.array([got[a], got[b]] * 50)).nruns == 1
    a, b = min(far, key=lambda ab: ab[1] - ab[0])
    assert _same_table(np.array([got[a], got[b]] * 50)).nruns == 2


def test_table_against_brute_force_long_run():
    c = gr.BY_NAME["long_run"]
    _, scale, _ = c.build(n=2)
    meta = _same_table(scale)
    assert meta.F2 > meta.group[-1] + 1  # a fold that is no group end: the one inside the long class
