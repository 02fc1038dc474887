"""GPU: the three class Gram kernels of csrc/gramcls.hip on PRESCRIBED weight-class structures (tests/gramcls_ref.py).

pca_gram takes any per-locus scale, and w = 1 / scale^2 is the class table: so the classes, groups, blocks and K ranges
that a kernel meets are chosen here instead of being whatever the binomial scaling of a random panel gives.  Every case of
gramcls_ref.CASES names its edge and asserts it on the restated table (on the CPU too: tests/test_gramcls_host.py) -- class
lengths around 64 and 128, one class in one block (an empty K range), groups of GCLS_GMAX - 1 .. GCLS_GMAX + 1 classes,
a cut at a 2^-6 bucket edge, at a power of two and at a key that carries into the exponent, K ranges that start inside a
class, inside a group, on a group end and end on the padding block, row tiles around 32, 64 and 128 individuals, and a class
of more than GCLS_GRUN blocks behind a run of short ones.

Every case runs tpg_gcls_gram_kernel (TPG_GRAM_FOLD64=1), tpg_gcls_gram2_kernel<false> (=0, center = 0) and
tpg_gcls_gram2_kernel<true> (=0, center = the column mean, which the library recognises) with the prescribed scale.  With
center = 0 the call returns S' itself, a sum of non-negative terms, held ELEMENTWISE to rel_fold64 / rel_mixed_table of the
exact reference (integer class matrices, long-double sums; rel_mixed_table is rel_mixed with the FP32 term of the case's own
table, which is smaller); the centred calls to bound_centred.  The bounds are derived in gramcls_ref, none is fitted; the host
file shows that one wrong term, flag or block leaves them.  Besides: K is exactly symmetric, a second call returns the same
bits, and so does every TPG_GATHER_QW.
"""
import os

import numpy as np
import pytest

from tests import gramcls_ref as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_built = {}


def _case(name):
    """(g, scale, meta) of a named case, built once per module and left unchanged"""
    if name not in _built:
        g, scale, meta = gr.BY_NAME[name].build()
        g.setflags(write=False)
        scale.setflags(write=False)
        _built[name] = (g, scale, meta)
    return _built[name]


def _check(tpg, label, v, g, scale, meta, fold64_left_alone=False):
    """the three kernels on view v, whose genotypes are g, against the exact reference and the bound of each"""
    n = g.shape[0]
    R = gr.exact(g, scale)
    Rc = gr.centre(R)
    major = gr.centred_majorant(g, meta)
    zero, mean = np.zeros(g.shape[1]), tpg.pca_center_scale(v)[0]
    assert np.array_equal(mean, g.sum(axis=0, dtype=np.int64) / n)
    rel64, rel2 = gr.rel_fold64(meta), gr.rel_mixed_table(meta)  # (the sharper of the two mixed bounds: it implies rel_mixed)
    runs = [("fold64", "1", zero, rel64), ("fold64 centred", "1", mean, rel64), ("mixed", "0", zero, rel2),
            ("mixed centred", "0", mean, rel2)]
    if fold64_left_alone:  # the library's own choice between the two folds, by classes per block
        runs = [("own choice", None, zero, rel64 if meta.fold64_by_default else rel2)]
    for kernel, fold64, center, rel in runs:
        with _env(TPG_GRAM_CLASSES="1", TPG_GRAM_DIGITS=None, TPG_GRAM_FOLD64=fold64, TPG_GATHER_QW=None):
            K = tpg.pca_gram(v, center, scale)
            again = tpg.pca_gram(v, center, scale)
            by_qw = []
            for qw in ("1", "2", "4"):
                with _env(TPG_GATHER_QW=qw):
                    by_qw.append(tpg.pca_gram(v, center, scale))
        if center is zero:  # K = S': elementwise
            err = np.abs(K.astype(gr.LD) - R)
            bound = gr.LD(rel) * R
            worst = float((err / np.where(bound > 0, bound, 1)).max())
            inside = bool(np.all(err <= bound))
        else:
            err = float(np.abs(K.astype(gr.LD) - Rc).max())
            bound = gr.bound_centred(rel, R, n, major)
            worst, inside = err / bound, err <= bound
        print(f"gramcls {label:24s} {kernel:15s} error / bound = {worst:.3g}")
        assert np.array_equal(K, K.T), (label, kernel)
        assert inside, (label, kernel, worst)
        assert np.array_equal(again, K), (label, kernel)
        for qw, Kq in zip("124", by_qw):
            assert np.array_equal(Kq, K), (label, kernel, "TPG_GATHER_QW", qw)


def _run(tpg, name, **kw):
    g, scale, meta = _case(name)
    _check(tpg, name, tpg.View(tpg.FBM.from_numpy(g)), g, scale, meta, **kw)


def _names(family):
    return [c.name for c in gr.CASES if c.family == family]


@pytest.mark.parametrize("name", _names("block edges"))
def test_block_edges(tpg, name):
    """classes of 1, 63, 64, 65, 127, 128, 129 loci in one group and in a bucket each, an even and an odd number of blocks;
    the whole panel one class of 1, 64, 65 loci: one block pair, two K ranges, the first one empty"""
    _run(tpg, name)


@pytest.mark.parametrize("name", [n for n in _names("group edges") if not n.startswith("ratio")])
def test_group_edges(tpg, name):
    """63, 64, 65, 129 classes in one bucket (cut by GCLS_GMAX alone, on the absolute run index); neighbours on the two sides
    of a bucket edge and of a power of two; a key that carries into the exponent; weights from 2^-10 to 2^11"""
    _run(tpg, name)


@pytest.mark.parametrize("name", ["ratio_below", "ratio_above"])
def test_fold_choice_on_both_sides_of_the_threshold(tpg, name):
    """0.10 and 0.20 classes per block around gcls_fold64's 0.15, TPG_GRAM_FOLD64 unset: the result must meet the bound of the
    kernel the library is to pick -- 1e-14 below the threshold, which the mixed fold of these groups would not -- and then the
    bounds of both kernels when they are forced"""
    _run(tpg, name, fold64_left_alone=True)
    _run(tpg, name)


@pytest.mark.parametrize("name", _names("K ranges"))
def test_k_ranges(tpg, name):
    """1 .. 129 blocks: S = 2 with an empty or a one-pair range up to S = 32, with range starts inside a class, inside a group,
    on a group end, and the last range ending on the padding block (the assertions do not depend on the S taken)"""
    _run(tpg, name)


@pytest.mark.parametrize("name", [n for n in _names("tile edges") if n != "tiles_store"])
def test_tile_edges(tpg, name):
    """n = 1 .. 257: clamped row tiles past the data, the `tk < ti` skip of the assemble kernel, units on the diagonal"""
    _run(tpg, name)


@pytest.mark.parametrize("which", ["rows", "cols"])
def test_tile_edges_subset_views(tpg, which):
    """130 of the 150 individuals, and 4 000 of the loci in an order of their own, as views of one larger store"""
    g, scale, _ = _case("tiles_store")
    rng = np.random.default_rng(5)
    X = tpg.FBM.from_numpy(g)
    if which == "rows":
        rows = np.sort(rng.permutation(g.shape[0])[:130])
        gs, ss = g[rows], scale
        v = tpg.View(X, (rows + 1).astype(np.int32))
    else:
        rows = np.sort(rng.permutation(g.shape[0])[:130])
        cols = rng.permutation(g.shape[1])[:4000]
        gs, ss = g[np.ix_(rows, cols)], scale[cols]
        v = tpg.View(X, (rows + 1).astype(np.int32), (cols + 1).astype(np.int32))
    assert v.n == 130 and v.m == gs.shape[1]
    _check(tpg, f"tiles_store/{which}", v, np.asfortranarray(gs), np.ascontiguousarray(ss), gr.describe(ss))


def test_long_run(tpg):
    """n = 40, 1.2 million loci: 300 short classes, then one class of GCLS_GRUN + 2 100 blocks that starts on an odd block and
    crosses block GCLS_GRUN of the list -- the mid-class fold of the mixed kernel and the group end forced after it -- then
    short classes again"""
    _run(tpg, "long_run")
