"""CPU: the dealing of the pairwise kernels, tidypopgen_amd/csrc/host/host_pwplan.h, compiled as a stand-alone program under the
host sanitizers (tests/host/pwplan_main.cpp) and run over the grid
    nun in {1, 3, 92, 117, 392, 4134}  x  S in 1 .. 14  x  W in {32, 1024}  x  kgs in {1, 7, 8, 9, 144, 208, 977, 7813}.
Per plan, on what the header's own functions return:
  * every (unit, group) is covered exactly once;
  * there are R W + L c indices, R = floor(nun S / W), L = nun S - R W, and the tail L c is at most W;
  * c is the largest integer with L c <= W whose pieces keep 8 groups (1 where there is none);
  * every tail piece is at least min(8, its parent range) groups long, and no piece exceeds 2^17 groups;
  * with c capped at 1, and wherever L = 0, the decode is the one the kernels had before, index for index;
  * the tail is ordered piece-outer: tail index t is piece t // L of wave-unit R W + t % L.  So the takers of one piece are
    one run of L consecutive indices over consecutive wave-units -- 128 consecutive indices share one piece unless they
    cross a multiple of L, where they pass into the NEXT piece of the same range (never more than two pieces when L >= 128).
    "One sub-range for any 128 consecutive indices" cannot hold together with an unpadded tail of L c indices when 128 does
    not divide L; what is asserted is the order that statement was meant to secure.
  * the header and the numpy restatement (tests/pwplan_ref.py) agree index for index.
The K split under the cost model keeps every piece within 2^17 groups on a range of 2^20 groups."""
import shutil

import numpy as np
import pytest

from tests import pwplan_ref as pr

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")

NUN = (1, 3, 92, 117, 392, 4134)
SS = tuple(range(1, 15))
WS = (32, 1024)
KGS = (1, 7, 8, 9, 144, 208, 977, 7813)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return pr.build_host_program(str(tmp_path_factory.mktemp("pwplan") / "pwplan_main"))


def _covered_once(unit, k0, k1, nun, kgs):
    """the pieces of every unit, sorted, tile [0, kgs) without gap or overlap"""
    o = np.lexsort((k1, k0, unit))
    u, a, b = unit[o], k0[o], k1[o]
    assert np.all(a <= b) and u[0] == 0 and u[-1] == nun - 1
    first = np.r_[True, u[1:] != u[:-1]]
    last = np.r_[first[1:], True]
    assert np.all(np.diff(u) <= 1) and first.sum() == nun  # every unit is there
    assert np.all(a[first] == 0) and np.all(b[last] == kgs)
    assert np.all(a[1:][~first[1:]] == b[:-1][~first[1:]])


@pytest.mark.parametrize("nun", NUN)
def test_grid(exe, tmp_path, nun):
    grid = [(S, W, kgs, cmax) for S in SS for W in WS for kgs in KGS for cmax in (0, 1)]
    res = pr.run_host_program(exe, tmp_path, [f"plan {nun} {S} {W} {kgs} {pr.MIN_GROUPS} {cmax}" for S, W, kgs, cmax in grid])
    cut = 0
    for (S, W, kgs, cmax), (head, rows) in zip(grid, res):
        what = (nun, S, W, kgs, cmax)
        p = pr.Plan(*(int(x) for x in head))
        unit, k0, k1 = (rows[:, i].astype(np.int64) for i in range(3))
        R, L = nun * S // W, nun * S - nun * S // W * W
        assert (p.nun, p.S, p.W, p.kgs, p.full, p.L) == (nun, S, W, kgs, R * W, L), what
        assert p.total == R * W + L * p.c == len(rows) and L * p.c <= W and p.c >= 1, what
        if cmax == 1 or L == 0:
            assert p.c == 1, what
            b = pr.before(nun, S, kgs)
            assert all(np.array_equal(x, y) for x, y in zip((unit, k0, k1), b)), what
            continue
        # c: the largest that fits the round and keeps 8 groups in the shortest piece of the shortest range, floor(kgs / S)
        fits = [c for c in range(1, W + 1) if L * c <= W and (kgs // S) // c >= pr.MIN_GROUPS]
        assert p.c == (max(fits) if fits else 1), what
        cut += p.c > 1
        _covered_once(unit, k0, k1, nun, kgs)
        assert np.all(k1 - k0 <= 1 << 17), what
        # the full rounds are the old decode
        b = pr.before(nun, S, kgs)
        assert all(np.array_equal(x[:p.full], y[:p.full]) for x, y in zip((unit, k0, k1), b)), what
        # the tail: piece t // L of wave-unit R W + t % L, each piece at least min(8, parent) groups
        t = np.arange(L * p.c)
        wu = p.full + t % L
        assert np.array_equal(unit[p.full:], wu % nun), what
        lo, hi = kgs * (wu // nun) // S, kgs * (wu // nun + 1) // S
        tk0, tk1 = k0[p.full:], k1[p.full:]
        assert np.all(tk1 - tk0 >= np.minimum(pr.MIN_GROUPS, hi - lo)), what
        assert np.all((tk0 >= lo) & (tk1 <= hi)), what
        sub = t // L
        assert np.array_equal(tk0, lo + (hi - lo) * sub // p.c) and np.array_equal(tk1, lo + (hi - lo) * (sub + 1) // p.c), what
        if L >= 128:  # 128 consecutive indices: one piece, or two neighbouring ones across a multiple of L
            w = np.lib.stride_tricks.sliding_window_view(sub, 128)
            assert np.all(w[:, -1] - w[:, 0] <= 1), what
            inside = (t[:len(w)] % L) + 128 <= L
            assert np.all(w[inside, -1] == w[inside, 0]), what
        # the restatement
        assert p == pr.make(nun, S, W, kgs) and all(np.array_equal(x, y) for x, y in zip((unit, k0, k1), pr.pieces(p))), what
    assert cut >= 10, (nun, cut)  # the grid holds cut tails for every nun


def test_named_plans(exe, tmp_path):
    """the bench panel (4134 units, 7813 groups, 1024 waves): 40.37 rounds at S = 10 become 40 and a tail of 380 x 2; a call of
    26 624 loci: 4.04 rounds at S = 1 become 4 and a tail of 38 x 26"""
    res = pr.run_host_program(exe, tmp_path, ["plan 4134 10 1024 7813 8 0", "plan 4134 1 1024 208 8 0", "plan 4134 5 1024 7813 8 0",
                                              "plan 33 1 32 8 8 0", "plan 4134 2 2048 15626 16 0"])
    heads = [tuple(int(x) for x in h) for h, _ in res]
    assert heads[0] == (4134, 10, 1024, 7813, 40 * 1024, 380, 2, 40 * 1024 + 760)
    assert heads[1] == (4134, 1, 1024, 208, 4 * 1024, 38, 26, 4 * 1024 + 38 * 26)
    assert heads[2] == (4134, 5, 1024, 7813, 20 * 1024, 190, 5, 20 * 1024 + 950)
    assert heads[3] == (33, 1, 32, 8, 32, 1, 1, 33)
    assert heads[4][4:] == (4 * 2048, 76, 26, 4 * 2048 + 76 * 26)  # K in blocks of 64 loci: a piece keeps 16 of them


def test_ksplit(exe, tmp_path):
    """the header's K split equals the restatement; on 2^20 groups (minS = 8) no piece exceeds 2^17 groups"""
    qs = [(nun, kgs, 8, -(-kgs // pr.MAX_GROUPS), W, ts, tf)
          for nun in (1, 92, 392, 4134, 16471) for kgs in (8, 208, 977, 7813, 1 << 20) for W in (32, 1024)
          for ts, tf in ((0.55, 12.0), (0.3, 4.8))]
    res = pr.run_host_program(exe, tmp_path, ["ksplit " + " ".join(str(x) for x in q) for q in qs])
    for q, (head, _) in zip(qs, res):
        S = int(head[0])
        assert S == pr.ksplit(*q) and S >= q[3], q
        p = pr.make(q[0], S, q[4], q[1])
        assert -(-q[1] // S) <= 1 << 17 and p.L * p.c <= max(q[4], p.L), q
