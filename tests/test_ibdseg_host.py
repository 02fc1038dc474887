"""CPU-only: the definition of include/tpg.h "IBD segments" in its two numpy restatements (tests/ibdseg_ref.py), a toy with its
segments spelled out, the conditions the panels of the GPU grid must meet, csrc/host/host_ibdseg.h under the host sanitizers,
and a simulated pedigree whose true IBD regions the segments must cover."""
import shutil

import numpy as np
import pytest

from tests import ibdseg_ref as ir

C = ir.CHUNK
LOOP_LOCI = 30000  # pair-loci the literal route walks per panel and configuration


def _sample_pairs(n, m, seed):
    """all pairs of a small panel; of a larger one the planted pairs (0, 1), (2, 3) and a random sample, in (a, b) order"""
    ia, ib = np.triu_indices(n, 1)
    P = len(ia)
    want = max(3, LOOP_LOCI // max(m, 1))
    if P <= want:
        return np.stack([ia, ib], axis=1)
    rng = np.random.default_rng([seed, n, m])
    pick = set(rng.choice(P, want, replace=False).tolist())
    pick |= {k for k in range(P) if (ia[k], ib[k]) in ((0, 1), (2, 3))}
    idx = np.array(sorted(pick))
    return np.stack([ia[idx], ib[idx]], axis=1)


def _loop_on(G, chrom, pos, pairs, **kw):
    p = ir.params(**kw)
    brk = ir.breaks(chrom, pos, p["max_gap"])
    rows = []
    for a, b in pairs:
        bad, typed = ir.bad_typed(G[a], G[b], p["kind"])
        rows += [(a, b) + s for s in ir.pair_segments_loop(bad, typed, brk, np.asarray(pos), p)]
    return ir._table(rows)


@pytest.mark.parametrize("n", ir.NS[1:])
def test_the_two_routes_agree_on_the_grid(n):
    for m in ir.MS:
        if (n, m) not in ir.GRID:
            continue
        G, chrom, pos = ir.grid_case(n, m)
        pairs = _sample_pairs(n, m, 3)
        for kind, bridge in ir.CONFIGS:
            kw = dict(ir.GRID_PARAMS, kind=kind, bridge_min_snp=bridge)
            assert ir.same_segments(ir.segments_vec(G, chrom, pos, pairs=pairs, **kw), _loop_on(G, chrom, pos, pairs, **kw)), (m, kind, bridge)
    G, chrom, pos = ir.grid_case(n, 1000)
    for kind, min_snp, bridge in ir.LONG_CONFIGS:  # the long thresholds report something too
        kw = dict(ir.GRID_PARAMS, kind=kind, min_snp=min_snp, bridge_min_snp=bridge)
        pairs = _sample_pairs(n, 1000, 5)
        want = ir.segments_vec(G, chrom, pos, pairs=pairs, **kw)
        assert len(want["first"]) > 0 and ir.same_segments(want, _loop_on(G, chrom, pos, pairs, **kw))
    G, chrom, pos = ir.grid_case(n, 129)
    if n <= 33:  # and the route over all pairs is the route over a list of all pairs
        kw = dict(ir.GRID_PARAMS, kind=1, bridge_min_snp=ir.GRID_BRIDGE)
        assert ir.same_segments(ir.segments_vec(G, chrom, pos, **kw), ir.segments_loop(G, chrom, pos, **kw))


def _toy():
    m = 48
    g0 = np.zeros(m, dtype=np.uint8)
    g1 = g0.copy()
    g1[[10, 20, 21, 30, 36, 38]] = 2  # opposite homozygotes: bad for either kind
    g0[5] = 3
    G = np.stack([g0, g1, np.full(m, 3, dtype=np.uint8), g1])  # 2: wholly missing; 3: a duplicate of 1
    chrom = np.ones(m, dtype=np.int32)
    pos = 100 * np.arange(m, dtype=np.int64)
    pos[30:] += 5000  # brk[29]
    return G, chrom, pos


TOY_PARAMS = dict(min_snp=3, min_length=0, max_gap=1000, bridge_min_snp=3, max_err=-1)
# (first, last, n_typed, n_err) of the pair (0, 1): [0, 9] + [11, 19] bridged over locus 10 (locus 5 is missing in 0); 20 and 21 are
# two bad loci in a row: no bridge; the break behind 29 lies next to the bad locus 30: no bridge; [37, 37] has one locus: no
# bridge on either side of it, and it falls to min_snp; the last segment ends at m - 1
TOY_01 = [(0, 19, 19, 1), (22, 29, 8, 0), (31, 35, 5, 0), (39, 47, 9, 0)]
TOY_13 = [(0, 29, 30, 0), (30, 47, 18, 0)]  # the duplicate: one segment per break-free region


def _toy_want(kind):
    rows = [(0, 1) + s for s in TOY_01] + [(0, 3) + s for s in TOY_01] + [(1, 3) + s for s in TOY_13]
    return ir._table(rows)


@pytest.mark.parametrize("kind", [1, 2])
def test_toy(kind):
    G, chrom, pos = _toy()
    for route in (ir.segments_loop, ir.segments_vec):
        got = route(G, chrom, pos, kind=kind, **TOY_PARAMS)
        assert ir.same_segments(got, _toy_want(kind)), route.__name__
    n_seg, total = ir.summary(_toy_want(kind), 4, pos)
    assert n_seg[0, 1] == n_seg[1, 0] == 4 and n_seg[1, 3] == 2 and not n_seg[2].any() and not np.diag(n_seg).any()
    assert total[1, 3] == ir.genome_length(chrom, pos, 1000) == 2900 + 1700
    off = ir.segments_vec(G, chrom, pos, kind=kind, **dict(TOY_PARAMS, bridge_min_snp=0))
    assert (0, 1, 0, 9, 9, 0) in ir.seg_set(off) and (0, 1, 11, 19, 9, 0) in ir.seg_set(off) and not off["n_err"].any()


def test_parameter_checks_and_order():
    G, chrom, pos = _toy()
    for bad in (dict(min_snp=0), dict(min_length=-1), dict(max_gap=-1), dict(bridge_min_snp=-1), dict(kind=3), dict(kind=0)):
        with pytest.raises(ValueError):
            ir.segments_vec(G, chrom, pos, **bad)
    back = pos.copy()
    back[20] = back[19] - 1
    with pytest.raises(ValueError, match="not ordered"):
        ir.segments_vec(G, chrom, back)
    assert len(ir.segments_vec(G[:1], chrom, pos)["first"]) == 0  # one individual: no pair


TEETH = (("min_snp", dict(min_snp=60)), ("min_length", dict(min_length=40000)), ("max_gap", dict(max_gap=1980)),
         ("bridge_min_snp", dict(bridge_min_snp=0)), ("max_err", dict(max_err=0)))


@pytest.mark.parametrize("kind", [1, 2])
def test_every_parameter_has_teeth(kind):
    G, chrom, pos = ir.grid_case(33, 1000)
    base = dict(ir.GRID_PARAMS, kind=kind, bridge_min_snp=ir.GRID_BRIDGE)
    want = ir.seg_set(ir.segments_vec(G, chrom, pos, **base))
    assert want
    for name, over in TEETH:
        got = ir.seg_set(ir.segments_vec(G, chrom, pos, **dict(base, **over)))
        assert got and got != want, name


def test_the_grid_panels_hold_what_the_gpu_tests_need():
    for n, m in ir.GRID:
        if n < 2:
            continue
        G, chrom, pos = ir.grid_case(n, m)
        brk = ir.breaks(chrom, pos, ir.GRID_PARAMS["max_gap"])
        segs = {kind: ir.segments_vec(G, chrom, pos, **dict(ir.GRID_PARAMS, kind=kind, bridge_min_snp=ir.GRID_BRIDGE)) for kind in (1, 2)}
        if m >= 128:
            assert len(segs[1]["first"]) and len(segs[2]["first"]), (n, m)
            assert segs[1]["n_err"].any() or segs[2]["n_err"].any(), (n, m)
        if m >= 64:
            assert any(brk[31::32]), (n, m)  # a break on a word border
        if C < m < 2 * C:
            assert brk[C - 1]  # and on a chunk border
        # the planted bad locus on the last bit of a word / a chunk, typed stretches on either side: bridged in the pair (0, 1)
        for e in (63, C - 1):
            if m // 4 + 8 < e < m - 8:
                bad, typed = ir.bad_typed(G[0], G[1], 1)
                assert bad[e] and typed[e - 2:e + 3].all() and not bad[e - 2:e].any() and not bad[e + 1:e + 3].any(), (n, m, e)
        if m >= 2 * C:  # a segment across three chunks
            s = segs[2]
            assert any(a == 0 and b == 1 and f < C and l >= 2 * C for a, b, f, l in zip(s["ind_a"], s["ind_b"], s["first"], s["last"])), n


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert shutil.which("g++") is not None, "the host sanitizer run needs g++"
    return ir.build_host_program(str(tmp_path_factory.mktemp("ibdseg") / "ibdseg_san"), sanitize=True)


def test_host_state_machine_under_the_sanitizers(exe, tmp_path):
    cases = [ir.grid_case(n, m) for n, m in ((3, 129), (33, 1000), (2, 2 * C + 5), (32, 33), (31, 1), (3, C + 1))] + [_toy()]
    for G, chrom, pos in cases:
        n = G.shape[0]
        pairs = list(zip(*(x.tolist() for x in np.triu_indices(n, 1))))
        for kind, min_snp, bridge in [(k, None, b) for k, b in ir.CONFIGS + [(1, 3)]] + ir.LONG_CONFIGS:
            kw = dict(TOY_PARAMS if n == 4 else ir.GRID_PARAMS, kind=kind, bridge_min_snp=bridge)
            if min_snp is not None:
                kw["min_snp"] = min_snp
            got, length = ir.run_host_program(exe, tmp_path / "in.txt", G, chrom, pos, pairs, **kw)
            assert ir.same_segments(got, ir.segments_vec(G, chrom, pos, **kw)), (G.shape, kind, bridge)
            assert length == ir.genome_length(chrom, pos, kw["max_gap"])
    G, chrom, pos = _toy()
    got, _ = ir.run_host_program(exe, tmp_path / "in.txt", G, chrom, pos, [(0, 1), (1, 3)], kind=2, max_err=0, **{
        k: v for k, v in TOY_PARAMS.items() if k != "max_err"})
    assert ir.seg_set(got) == {(0, 1) + s for s in TOY_01[1:]} | {(1, 3) + s for s in TOY_13}


def test_pedigree_true_regions_lie_inside_reported_segments():
    G, chrom, pos, A = ir.pedigree(1)
    n = G.shape[0]
    P = ir.PED_PARAMS
    brk = ir.breaks(chrom, pos, P["max_gap"])
    segs = {kind: ir.segments_vec(G, chrom, pos, kind=kind, **P) for kind in (1, 2)}
    covered = 0
    for a in range(n):
        for b in range(a + 1, n):
            state = ir.true_ibd(A, a, b)
            _, typed = ir.bad_typed(G[a], G[b], 1)
            for kind in (1, 2):
                s = segs[kind]
                mine = [(f, l) for x, y, f, l in zip(s["ind_a"], s["ind_b"], s["first"], s["last"]) if (x, y) == (a, b)]
                for lo, hi in ir.true_regions(state, kind, brk):
                    if typed[lo:hi + 1].sum() >= P["min_snp"]:
                        assert any(f <= lo and hi <= l for f, l in mine), (a, b, kind, lo, hi)
                        covered += 1
            if a < ir.PED_N_FOUNDERS and b < ir.PED_N_FOUNDERS:  # unrelated founders report nothing
                assert not state.any()
                assert not any((x, y) == (a, b) for kind in (1, 2) for x, y in zip(segs[kind]["ind_a"], segs[kind]["ind_b"]))
    assert covered >= 20
    Lg = ir.genome_length(chrom, pos, P["max_gap"])
    L1, L2 = ir.summary(segs[1], n, pos)[1], ir.summary(segs[2], n, pos)[1]
    for child, (pa, pb) in enumerate(ir.PED_CHILDREN, start=ir.PED_N_FOUNDERS):
        for par in (pa, pb):  # parent - offspring: IBD1 everywhere, IBD2 nowhere
            assert L1[par, child] == Lg and L2[par, child] == 0
    sibs = [(6, 7), (6, 8), (7, 8)]
    assert all(0 < L2[a, b] < L1[a, b] <= Lg for a, b in sibs)
    kin = (L1 + L2) / (4.0 * Lg)
    assert all(kin[a, b] > 0.0884 for a, b in sibs) and kin[0, 6] == 0.25 and kin[4, 5] == 0 and kin[0, 9] == 0
