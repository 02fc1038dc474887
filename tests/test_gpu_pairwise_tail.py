"""GPU: the pairwise kernels under forced dealing plans (TPG_PW_PLAN = "S,c,nblk", host/host_pwplan.h): all six integer matrices
of Pairwise.counts() equal the sums formed on the CPU from the genotype bytes -- float32 products of the 0/1 planes, exact below
2^24 loci.  nblk = 8 workgroups are 32 wave slots, so tiny panels run full rounds and tails.

Five-product kernel, units = sum over the 32-column tiles jt of (jt // 3 + 1): 2 at n = 33, 7 at n = 130, 18 at n = 257, 45 at 449.
  n    S   plan on 32 slots                what it pins
  33   1   R = 0, L = 2                    no full round, everything is tail
  130  3   R = 0, L = 21, c = 1            no full round, a tail too full to be cut
  130  5   R = 1, L = 3, c up to 10        a full round plus a tail with c > 1
  130  8   R = 1, L = 24 > W / 2, c = 1    a tail that cannot be cut
  257  4   R = 2, L = 8, c up to 4         two cuts of the K range inside the tail (wave-units 64 .. 71 span ks = 3 only)
  257  7   R = 3, L = 30, c = 1
  449  1   R = 1, L = 13, c up to 2        more units than slots
each at three m: every tail piece exactly 8 groups (m = 128 * 8 S (W // L)); the same plus 5 groups and 37 loci (ragged pieces, a
partial last group); 1 024 loci (c capped by the 8-group minimum), and at 2 % and 50 % missing.  The plan each case names is
asserted on the restatement (tests/pwplan_ref.py) AND read back from the library's TPG_DEBUG line."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

from tests import pwplan_ref as pr

pytestmark = pytest.mark.gpu

NAMES = ("ibs", "ibs_valid", "king_num", "n_Aa_i", "as_num", "as_den")
NBLK = 8
CASES = [(33, 1), (130, 3), (130, 5), (130, 8), (257, 4), (257, 7), (449, 1)]


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


@pytest.fixture(scope="module")
def cus():
    hip, n = C.CDLL("libamdhip64.so.7"), C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(n), 63, 0) == 0 and n.value > 0  # hipDeviceAttributeMultiprocessorCount
    return n.value


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


class _stderr:
    """what the library writes to file descriptor 2 inside the block -> .text"""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode()
        self.tmp.close()


_panels = {}


def _panel(n, m, miss):
    """genotype bytes (3 = missing) and the six matrices from float32 products of the 0/1 planes (every sum <= 2 m < 2^24)"""
    key = (n, m, miss)
    if key not in _panels:
        assert 2 * m < 1 << 24
        rng = np.random.default_rng(1000 * n + m + int(100 * miss))
        g = rng.integers(0, 3, size=(n, m), dtype=np.uint8)
        g[rng.random((n, m)) < miss] = 3
        g0, g1, g2 = ((g == k).astype(np.float32) for k in range(3))
        v, d, hom = g0 + g1 + g2, g2 - g0, g0 + g2
        i64 = lambda x: np.rint(x).astype(np.int64)
        vv = i64(v @ v.T)
        ref = {"ibs_valid": 2 * vv, "as_den": vv, "as_num": i64(d @ d.T), "n_Aa_i": i64(g1 @ v.T),
               "ibs": 2 * i64(g0 @ g0.T) + 2 * i64(g1 @ g1.T) + 2 * i64(g2 @ g2.T) + i64(g1 @ hom.T) + i64(hom @ g1.T),
               "king_num": i64(g1 @ g1.T) - 2 * (i64(g0 @ g2.T) + i64(g2 @ g0.T))}
        for r in ref.values():
            r.setflags(write=False)
        _panels[key] = (np.asfortranarray(g), ref)
    return _panels[key]


def _run(tpg, g, plan=None, products=None, variant=None, times=1, pw=None):
    """accumulate under TPG_PW_PLAN = plan -> (the Pairwise, the [tpg] lines of the launches)"""
    X = tpg.FBM.from_numpy(g)
    v = tpg.View(X, code256=None)
    pw = pw or tpg.Pairwise(X.ctx, g.shape[0])
    with _env(TPG_PW_PLAN=plan, TPG_DEBUG="1", TPG_PW_VARIANT=variant), _stderr() as err:
        for _ in range(times):
            pw.accumulate(v, products=products)
        X.ctx.sync()
    return pw, [ln for ln in err.text.splitlines() if ln.startswith("[tpg] pairwise") and "units, S =" in ln]


def _equal(pw, ref, names=NAMES, times=1):
    c = pw.counts(names)
    for k in names:
        assert np.array_equal(c[k], times * ref[k]), k


def _ms(n, S):
    """the three m of a case: every tail piece 8 groups; plus 5 groups and 37 loci; 1 024 loci"""
    nun, W = pr.units_all(n), 4 * NBLK
    L = nun * S % W
    kgs = 8 * S * (W // L)
    return (128 * kgs, 128 * (kgs + 5) + 37, 1024)


@pytest.mark.parametrize("miss", [0.02, 0.5])
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("n,S", CASES)
def test_five_products_under_forced_plans(tpg, n, S, which, miss):
    m = _ms(n, S)[which]
    p = pr.launch_plan(pr.units_all(n), m, S=S, nblk=NBLK)
    R, fit = p.full // p.W, p.W // p.L
    assert p.W == 32 and p.L > 0
    assert (R, p.L) == {(33, 1): (0, 2), (130, 3): (0, 21), (130, 5): (1, 3), (130, 8): (1, 24), (257, 4): (2, 8), (257, 7): (3, 30),
                        (449, 1): (1, 13)}[(n, S)]
    if which == 2:
        assert p.c == max(1, min(fit, (8 // S) // 8))  # 8 groups in all: only S = 1 leaves a piece to cut, and not in two
        assert p.c == 1
    else:
        assert p.c == fit  # 16, 1, 10, 1, 4, 1, 2
        if which == 0:
            t = np.arange(p.full, p.total)
            _, k0, k1 = pr.pieces(p)
            assert np.all((k1 - k0)[t] == 8)
    g, ref = _panel(n, m, miss)
    pw, lines = _run(tpg, g, plan=f"{S},0,{NBLK}")
    assert len(lines) == 1 and lines[0].endswith(pr.debug_line(p)), (lines, pr.debug_line(p))
    _equal(pw, ref)


def _first_cut_S(nun, m, W, ksteps):
    """the smallest S whose plan on W slots has a full round and a tail of c > 1"""
    for S in range(1, 15):
        p = pr.launch_plan(nun, m, per_wg=W // NBLK, ksteps=ksteps, S=S, nblk=NBLK)
        if p.full and p.L and p.c > 1:
            return S, p
    raise AssertionError("no such S")


SETS = {  # products, TPG_PW_VARIANT, units, takers per workgroup, what counts() may be asked for
    "V,D": ("PW_FOR_AS", None, (4, 2), 4, ("as_num", "as_den")),
    "V|D+H": ("PW_FOR_IBS_ALONE", None, (4, 2), 4, ("ibs", "ibs_valid")),
    "V,D,H": ("PW_FOR_IBS", None, (2, 2), 4, ("ibs", "ibs_valid", "as_num", "as_den")),
    "KING": ("PW_FOR_KING", None, (2, 2), 4, ("king_num", "n_Aa_i", "as_num", "as_den")),
    "workgroup": ("PW_FOR_AS", "14", (8, 4), 1, ("as_num", "as_den")),
}


@pytest.mark.parametrize("name", list(SETS))
def test_product_sets_and_the_workgroup_form(tpg, name):
    """n = 257, m = 128 * 133 + 37 (a partial last group): the first S with a full round and a cut tail on 8 workgroups"""
    products, variant, (RA, RB), per_wg, names = SETS[name]
    n, m = 257, 128 * 133 + 37
    S, p = _first_cut_S(pr.units_set(n, RA, RB), m, per_wg * NBLK, 2)
    g, ref = _panel(n, m, 0.02)
    pw, lines = _run(tpg, g, plan=f"{S},0,{NBLK}", products=getattr(tpg, products), variant=variant)
    assert len(lines) == 1 and lines[0].endswith(pr.debug_line(p)), (lines, pr.debug_line(p))
    if name == "workgroup":
        assert "workgroups of" in lines[0]
    _equal(pw, ref, names)
    # c capped at 1: the same sums without the tail cut
    pw1, lines1 = _run(tpg, g, plan=f"{S},1,{NBLK}", products=getattr(tpg, products), variant=variant)
    assert lines1[0].endswith(f"tail {p.L} x 1")
    _equal(pw1, ref, names)


def test_two_plans_into_the_same_accumulators_add_up(tpg):
    n, m = 257, 128 * 133 + 37
    g, ref = _panel(n, m, 0.02)
    pw, a = _run(tpg, g, plan=f"4,0,{NBLK}")
    pw, b = _run(tpg, g, plan=f"7,1,{NBLK}", pw=pw)
    pw, c = _run(tpg, g, plan="2,3,16", pw=pw)
    assert "S = 4" in a[0] and "S = 7" in b[0] and "S = 2" in c[0] and a[0] != b[0] != c[0]
    _equal(pw, ref, times=3)


def test_default_plan_is_the_one_restated_from_the_cu_count(tpg, cus):
    n, m = 257, 4096
    g, ref = _panel(n, m, 0.02)
    p = pr.launch_plan(pr.units_all(n), m, num_cu=cus)
    assert p.W == 4 * (cus // 8 * 8) and p.nun == 18
    pw, lines = _run(tpg, g)
    assert len(lines) == 1 and lines[0].endswith(pr.debug_line(p)), (lines, pr.debug_line(p))
    _equal(pw, ref)


def test_bad_knobs_are_refused(tpg):
    g, _ = _panel(33, 1024, 0.02)
    for bad in ("0", "x", "3,-1", "3,1,12", "3,1,4", "97", "1,1,100000"):
        with pytest.raises(Exception):
            _run(tpg, g, plan=bad)
