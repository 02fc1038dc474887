"""IBD segments as include/tpg.h defines them ("IBD segments"), restated in numpy in two forms: a literal one that walks the
loci of every pair (clean stretches, then joints, then chains), and a vectorised one over all pairs at once.  Everything is an
integer.  Also the panels, the locus tables and the simulated pedigree of the tests, and the stand-alone host program."""
import os
import subprocess

import numpy as np

from tests.roh_ref import breaks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(kind=1, min_snp=200, min_length=0, max_gap=10**6, bridge_min_snp=50, max_err=-1)
KEYS = ("ind_a", "ind_b", "first", "last", "n_typed", "n_err")
CHUNK = 1024  # TPG_IBD_CHUNK_LOCI: the panels plant their seam cases by it (tests/test_gpu_ibdseg.py checks the library agrees)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def check_params(p):
    if p["min_snp"] < 1 or p["min_length"] < 0 or p["max_gap"] < 0 or p["bridge_min_snp"] < 0 or p["kind"] not in (1, 2):
        raise ValueError("parameter outside its range")


def bad_typed(ga, gb, kind):
    ga, gb = np.asarray(ga).astype(np.int64), np.asarray(gb).astype(np.int64)
    typed = (ga != 3) & (gb != 3)
    bad = typed & ((np.abs(ga - gb) == 2) if kind == 1 else (ga != gb))
    return bad, typed


def _table(rows):
    a = np.array(rows, dtype=np.int64).reshape(-1, 6)
    return {k: a[:, i] for i, k in enumerate(KEYS)}


def _reported(n_typed, length, n_err, p):
    return n_typed >= p["min_snp"] and length >= p["min_length"] and (p["max_err"] < 0 or n_err <= p["max_err"])


def pair_segments_loop(bad, typed, brk, pos, p):
    """steps 2 - 4 for one pair, literally -> [(first, last, n_typed, n_err)]"""
    m, B = len(bad), p["bridge_min_snp"]
    stretches, s = [], None
    for j in range(m):  # step 2
        if bad[j]:
            continue
        if s is None:
            s = j
        if j == m - 1 or bad[j + 1] or brk[j]:
            stretches.append((s, j, int(typed[s:j + 1].sum())))
            s = None
    chains = []
    for k, (s2, e2, c2) in enumerate(stretches):  # step 3
        joined = False
        if k > 0 and B > 0:
            s1, e1, c1 = stretches[k - 1]
            joined = s2 == e1 + 2 and not brk[e1] and not brk[e1 + 1] and c1 >= B and c2 >= B
        if joined:
            chains[-1] = (chains[-1][0], e2, chains[-1][2] + 1)
        else:
            chains.append((s2, e2, 0))
    out = []
    for first, last, n_err in chains:  # step 4
        n_typed = int(typed[first:last + 1].sum())
        if _reported(n_typed, int(pos[last] - pos[first]), n_err, p):
            out.append((first, last, n_typed, n_err))
    return out


def segments_loop(G, chrom, pos, **kw):
    p = params(**kw)
    check_params(p)
    G, pos = np.asarray(G), np.asarray(pos, dtype=np.int64)
    n = G.shape[0]
    brk = breaks(chrom, pos, p["max_gap"])
    rows = []
    for a in range(n):
        for b in range(a + 1, n):
            bad, typed = bad_typed(G[a], G[b], p["kind"])
            rows += [(a, b) + seg for seg in pair_segments_loop(bad, typed, brk, pos, p)]
    return _table(rows)


def segments_vec(G, chrom, pos, pairs=None, **kw):
    """all pairs at once (or the rows of `pairs`, (P, 2) with a < b, in (a, b) order)"""
    p = params(**kw)
    check_params(p)
    G, pos = np.asarray(G), np.asarray(pos, dtype=np.int64)
    n, m = G.shape
    brk = breaks(chrom, pos, p["max_gap"])
    if pairs is None:
        ia, ib = np.triu_indices(n, 1)
    else:
        ia, ib = np.asarray(pairs)[:, 0], np.asarray(pairs)[:, 1]
    if len(ia) == 0:
        return _table([])
    out, step = [], max(1, (1 << 25) // max(m, 1))
    for lo in range(0, len(ia), step):  # (blocks of pairs: the boolean planes stay small)
        out.append(_segments_block(G, ia[lo:lo + step], ib[lo:lo + step], brk, pos, p))
    return {k: np.concatenate([o[k] for o in out]) for k in KEYS}


def _segments_block(G, ia, ib, brk, pos, p):
    m, B = G.shape[1], p["bridge_min_snp"]
    bad, typed = bad_typed(G[ia], G[ib], p["kind"])
    P = len(ia)
    cut_before = np.concatenate([[True], brk])  # a stretch cannot continue into locus j from j - 1
    cut_after = np.concatenate([brk, [True]])
    prev_bad = np.concatenate([np.ones((P, 1), dtype=bool), bad[:, :-1]], axis=1)
    next_bad = np.concatenate([bad[:, 1:], np.ones((P, 1), dtype=bool)], axis=1)
    sp, sj = np.nonzero(~bad & (prev_bad | cut_before[None, :]))
    ep, ej = np.nonzero(~bad & (next_bad | cut_after[None, :]))
    assert np.array_equal(sp, ep) and np.all(ej >= sj)
    ct = np.concatenate([np.zeros((P, 1), dtype=np.int64), np.cumsum(typed, axis=1, dtype=np.int64)], axis=1)
    c = ct[sp, ej + 1] - ct[sp, sj]
    K = len(sj)
    joined = np.zeros(K, dtype=bool)  # stretch k is joined to stretch k - 1
    if B > 0 and K > 1:
        e1 = ej[:-1]
        ok = (sp[1:] == sp[:-1]) & (sj[1:] == e1 + 2) & (c[:-1] >= B) & (c[1:] >= B)
        e1c = np.minimum(e1, m - 3)  # (where the joint can hold, e1 + 1 <= m - 2: the clamp only keeps the index inside)
        ok &= ~brk[e1c] & ~brk[e1c + 1] if m >= 3 else False
        joined[1:] = ok
    chain = np.cumsum(~joined) - 1
    head = np.flatnonzero(~joined)
    tail = np.concatenate([head[1:] - 1, [K - 1]]) if K else head
    first, last, pr = sj[head], ej[tail], sp[head]
    n_err = np.bincount(chain, weights=joined, minlength=len(head)).astype(np.int64) if K else np.zeros(0, dtype=np.int64)
    n_typed = ct[pr, last + 1] - ct[pr, first]
    keep = (n_typed >= p["min_snp"]) & (pos[last] - pos[first] >= p["min_length"])
    if p["max_err"] >= 0:
        keep &= n_err <= p["max_err"]
    return dict(ind_a=ia[pr][keep].astype(np.int64), ind_b=ib[pr][keep].astype(np.int64), first=first[keep], last=last[keep],
                n_typed=n_typed[keep], n_err=n_err[keep])


def same_segments(a, b):
    return all(np.array_equal(np.asarray(a[k], dtype=np.int64), np.asarray(b[k], dtype=np.int64)) for k in KEYS)


def seg_set(s):
    return set(zip(*(np.asarray(s[k]).tolist() for k in KEYS)))


def summary(segs, n, pos):
    """-> (n_seg (n, n) int32, sum_length (n, n) int64), symmetric with a zero diagonal"""
    pos = np.asarray(pos, dtype=np.int64)
    n_seg, total = np.zeros((n, n), dtype=np.int32), np.zeros((n, n), dtype=np.int64)
    a, b = np.asarray(segs["ind_a"], dtype=np.int64), np.asarray(segs["ind_b"], dtype=np.int64)
    length = pos[segs["last"]] - pos[segs["first"]]
    np.add.at(n_seg, (a, b), 1)
    np.add.at(total, (a, b), length)
    return n_seg + n_seg.T, total + total.T


def genome_length(chrom, pos, max_gap):
    pos = np.asarray(pos, dtype=np.int64)
    m = len(pos)
    if m == 0:
        return 0
    brk = breaks(chrom, pos, max_gap)
    starts = np.concatenate([[0], np.flatnonzero(brk) + 1])
    ends = np.concatenate([np.flatnonzero(brk), [m - 1]])
    return int((pos[ends] - pos[starts]).sum())


# ---- panels -------------------------------------------------------------------------------------------------------------
GRID_PARAMS = dict(min_snp=20, min_length=0, max_gap=10**6, max_err=-1)  # of the grid tests; bridging: 8 loci, or off
GRID_BRIDGE = 8
NS = (1, 2, 3, 31, 32, 33, 65, 130)
MS = (1, 31, 32, 33, 127, 128, 129, 1000, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5)
GRID = [(n, m) for n in NS for m in MS if n < 130 or m <= 1000]  # (the pair tile is 32 x 32: its edges are in NS)
CONFIGS = [(kind, bridge) for kind in (1, 2) for bridge in (GRID_BRIDGE, 0)]
# (kind, min_snp, bridge_min_snp) around the thresholds of 33 loci from which the library skips the stretches inside a word
# (csrc/host/host_ibdseg.h: host_ibd_skip_short): on, on, and off by one locus
LONG_CONFIGS = [(kind, 33, bridge) for kind in (1, 2) for bridge in (33, 0, 32)]


def grid_case(n, m):
    """the panel and the loci of one grid point"""
    chrom, pos = ibd_loci(100 + n, m)
    return ibd_panel(100 + n, n, m), chrom, pos


def ibd_loci(seed, m, max_gap=10**6):
    """chrom (int32) and pos (int64) of m ordered loci: spacings of up to 2000, a tenth of them zero (equal positions); a
    chromosome change on a word border (m >= 64), one on the chunk border (CHUNK < m < 2 CHUNK), and one gap above max_gap.
    With m >= 2 CHUNK everything behind locus CHUNK / 2 is one break-free region: room for a segment across three chunks."""
    rng = np.random.default_rng([seed, m, 11])
    sp = (1 + rng.integers(0, 2000, m)).astype(np.int64)
    sp[rng.random(m) < 0.1] = 0
    cuts = []
    if m >= 64:
        cuts.append(96 if m >= 2 * CHUNK else 32 * max(1, (m // 3) // 32))
    if CHUNK < m < 2 * CHUNK:
        cuts.append(CHUNK)
    chrom = (np.searchsorted(np.array(cuts, dtype=np.int64), np.arange(m), side="right") + 1).astype(np.int32)
    if m >= 12:
        sp[CHUNK // 2 if m >= 2 * CHUNK else (3 * m) // 4 + 3] = max_gap + 1 + int(rng.integers(0, 1000))
    pos = np.empty(m, dtype=np.int64)
    for c in np.unique(chrom):
        idx = np.flatnonzero(chrom == c)
        pos[idx] = 1000 + np.cumsum(sp[idx])
    return chrom, pos


def ibd_panel(seed, n, m, nfounder=4, miss=0.05, flip=0.004):
    """mosaics of a few founder haplotypes with crossovers (so that pairs share stretches by descent), every odd individual a
    copy of its predecessor over a long stretch (IBD2; individual 1 from locus m / 4 up to the last, individual 3 from the
    first), a small rate of homozygote flips (bridgeable errors), about 5 % missing.  The pair (0, 1) has planted errors only:
    opposite homozygotes every 150 loci, and on the last bit of a word and of a chunk, with typed stretches on either side.  Codes 0, 1, 2 and 3 = missing."""
    rng = np.random.default_rng([seed, n, m, 5])
    f = 0.1 + 0.8 * rng.random(m)
    H = (rng.random((nfounder, m)) < f[None, :]).astype(np.uint8)
    L = max(24, m // 4)

    def mosaic():
        cross = np.concatenate([[True], rng.random(m - 1) < 1.0 / L])
        return H[rng.integers(0, nfounder, int(cross.sum()))[np.cumsum(cross) - 1], np.arange(m)]

    G = np.stack([mosaic() + mosaic() for _ in range(n)]).astype(np.uint8)
    a1 = m // 4
    for i in range(3, n, 2):
        if i == 3:
            a, b = 0, max(1, (2 * m) // 3)
        else:
            ln = int(rng.integers(max(1, m // 3), m + 1))
            a = int(rng.integers(0, m - ln + 1))
            b = a + ln
        G[i, a:b] = G[i - 1, a:b]
    hom = (G != 1) & (rng.random((n, m)) < flip)
    G[hom] = 2 - G[hom]
    if n >= 2:
        G[1, a1:] = G[0, a1:]  # (behind the flips: the errors of this pair are the planted ones below)
    G[rng.random((n, m)) < miss] = 3
    if n >= 2:
        for e in [63, CHUNK - 1] + list(range(a1 + 157, m, 150)):
            if a1 + 8 < e < m - 8:
                G[0, e - 2:e + 3] = G[1, e - 2:e + 3] = np.where(G[0, e - 2:e + 3] == 3, 0, G[0, e - 2:e + 3])
                G[0, e], G[1, e] = 0, 2
    return G


# ---- a simulated pedigree: founders, parent - offspring, full sibs, unrelated; crossovers recorded, no genotype errors ------
PED_N_FOUNDERS = 6
# (parents) of the non-founders 6 .. 9: three full sibs of founders 0 and 1, one child of founders 2 and 3; 4 and 5 are unrelated
PED_CHILDREN = ((0, 1), (0, 1), (0, 1), (2, 3))
PED_PARAMS = dict(min_snp=150, min_length=0, max_gap=10**6, bridge_min_snp=50, max_err=-1)


def pedigree(seed, m_chrom=(1500, 1300)):
    """-> G (10, m), chrom, pos, A (10, 2, m): the founder haplotype (2 f, 2 f + 1 of founder f) every haplotype copies at
    every locus"""
    rng = np.random.default_rng([seed, 23])
    m = int(sum(m_chrom))
    chrom = np.repeat(np.arange(1, len(m_chrom) + 1), m_chrom).astype(np.int32)
    pos = np.empty(m, dtype=np.int64)
    for c in np.unique(chrom):
        idx = np.flatnonzero(chrom == c)
        pos[idx] = 5000 + np.cumsum(1 + rng.integers(0, 3000, len(idx)))
    f = 0.2 + 0.6 * rng.random(m)
    H = (rng.random((2 * PED_N_FOUNDERS, m)) < f[None, :]).astype(np.uint8)
    A = [np.stack([np.full(m, 2 * k), np.full(m, 2 * k + 1)]) for k in range(PED_N_FOUNDERS)]

    def gamete(parent):
        out = np.empty(m, dtype=np.int64)
        for c in np.unique(chrom):
            idx = np.flatnonzero(chrom == c)
            nx = int(rng.integers(1, 3))  # one or two crossovers per chromosome
            cuts = np.sort(rng.choice(np.arange(1, len(idx)), nx, replace=False))
            which = (int(rng.integers(0, 2)) + np.searchsorted(cuts, np.arange(len(idx)), side="right")) % 2
            out[idx] = A[parent][which, idx]
        return out

    for pa, pb in PED_CHILDREN:
        A.append(np.stack([gamete(pa), gamete(pb)]))
    A = np.stack(A)
    G = (H[A[:, 0], np.arange(m)[None, :]] + H[A[:, 1], np.arange(m)[None, :]]).astype(np.uint8)
    G[rng.random(G.shape) < 0.02] = 3
    return G, chrom, pos, A


def true_ibd(A, a, b):
    """IBD state 0, 1 or 2 of the pair at every locus, from the recorded ancestry"""
    x, y = A[a], A[b]
    both = ((x[0] == y[0]) & (x[1] == y[1])) | ((x[0] == y[1]) & (x[1] == y[0]))
    one = (x[0] == y[0]) | (x[0] == y[1]) | (x[1] == y[0]) | (x[1] == y[1])
    return np.where(both, 2, np.where(one, 1, 0))


def true_regions(state, level, brk):
    """maximal [s, e] with state >= level throughout and no brk inside"""
    on = state >= level
    m = len(on)
    out, s = [], None
    for j in range(m):
        if on[j] and s is None:
            s = j
        if s is not None and (j == m - 1 or not on[j + 1] or brk[j]):
            if on[j]:
                out.append((s, j))
            s = None
    return out


# ---- csrc/host/host_ibdseg.h through the stand-alone program tests/host/ibdseg_san.cpp ----------------------------------------
def build_host_program(exe, sanitize=True):
    san = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", *san, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-function",
           "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc"), os.path.join(ROOT, "tests", "host", "ibdseg_san.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_host_program(exe, path, G, chrom, pos, pairs, **kw):
    """the segments of the given pairs as the program prints them, as a table; also the genome length it prints"""
    p = params(**kw)
    G = np.asarray(G)
    m = G.shape[1]
    lines = [f"{m} {len(pairs)} {p['kind']} {p['min_snp']} {p['min_length']} {p['max_gap']} {p['bridge_min_snp']} {p['max_err']}",
             " ".join(str(int(c)) for c in chrom), " ".join(str(int(x)) for x in pos)]
    for a, b in pairs:
        lines.append("".join(str(int(g)) for g in G[a]) + " " + "".join(str(int(g)) for g in G[b]))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stderr[-4000:])
    rows, length = [], None
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "L":
            length = int(w[1])
        else:
            k = int(w[0])
            rows.append((pairs[k][0], pairs[k][1]) + tuple(int(x) for x in w[1:]))
    return _table(rows), length
