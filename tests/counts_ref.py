"""Panels, class vectors, exact references, restated launch plans and fault models for the integer count sweeps:
tpg_loci_counts_kernel / tpg_loci_counts_sum_kernel / tpg_indiv_accumulate_kernel / tpg_grouped_counts_kernel (csrc/loci.hip)
and the per-chunk partial counts of tpg_pack_fast_kernel (csrc/pack.hip).  numpy only: no GPU, no library import.

Every output is an integer and the reference is (g == c).sum(): no tolerance anywhere.  A panel holds the codes 0, 1, 2 and
3 = missing as bytes (what CODE_012 and CODE_IMPUTE_PRED both read them as), Fortran order.

Panels are prescribed, not drawn: const() saturates every packed counter, rows_alternate() puts a saturated individual next to
one whose count must stay 0 (a carry out of any packed field lands there), stripes() changes code at the periods of the layouts
(element 4, dword 16, half block 32 / 64, block 128 along the individuals; 1, 3, 15 and 30 locus tiles = 32, 96, 480, 960 along
the loci), slots() names the element slot of a 128-individual block by the locus at which its count appears.  control() is the
one random panel.

Plans restate the launch rules so that a case can name the edge it was chosen for (tests/test_counts_host.py asserts each):
  Q = ceil(n / 128), KG = ceil(m / 128); the loci kernel walks its Q (as tpg_indiv_counts: KG) blocks in passes of 4 and a
  remainder loop, and takes npad = Q 128 - n (KG 128 - m) off the missing count afterwards;
  the fast pack kernel (n % 8 == 0, no row subset) leaves one partial per chunk of 256 individuals, a thread holds 16
  individuals and masks its halves by i0 + 8 <= n, i0 + 16 <= n;
  tpg_indiv_accumulate_kernel: gx = ceil(Q / 4) workgroups of four 128-individual groups, n_lt = ceil(m / 32) locus tiles in
  gy = ceil(n_lt / tiles) pieces, tiles = clamp(ceil(ceil(n_lt / ceil(4 CU / gx)) / 15) 15, 30, 255);
  tpg_grouped_counts_kernel: GT = ceil(nclass / 32) class tiles launched as <2>, <2>, ..., <1>, Q groups in passes of 4.

Fault models are numpy restatements of one kernel's arithmetic with one knob turned (FAULTS): tests/test_counts_host.py shows that
each one moves a count on a named case of the tables below, i.e. that tests/test_gpu_counts.py would see it.
"""
import numpy as np

CU_COUNTS = (8, 64, 256, 304)


def _cdiv(a, b):
    return -(-a // b)


def _f(a):
    a = np.asfortranarray(a, dtype=np.uint8)
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------------------------------
# panels: uint8 codes 0..3, Fortran order
def const(n, m, c):
    return _f(np.full((n, m), c))


def rows_alternate(n, m, a, b):
    """individual i is all `a` if i is even, else all `b`"""
    return _f(np.where((np.arange(n) % 2 == 0)[:, None], a, b) * np.ones((1, m), dtype=np.int64))


def cols_alternate(n, m, a, b):
    """locus j is all `a` if j is even, else all `b`"""
    return _f(np.ones((n, 1), dtype=np.int64) * np.where(np.arange(m) % 2 == 0, a, b)[None, :])


def stripes(n, m, pi, pj):
    return _f((np.arange(n)[:, None] // pi + np.arange(m)[None, :] // pj) % 4)


def slots(n, m):
    """g[i, j] = 1 + (i // 128) % 2 where j % 128 == i % 128, else 0: the count at locus j names slot j % 128 of a block"""
    assert m >= 128
    i, j = np.arange(n)[:, None], np.arange(m)[None, :]
    return _f(np.where(j % 128 == i % 128, 1 + (i // 128) % 2, 0))


CONTROL_P = (0.45, 0.3, 0.15, 0.1)


def control(n, m, seed=0):
    return _f(np.random.default_rng([seed, n, m]).choice(4, size=(n, m), p=CONTROL_P))


_MAKERS = {"const": const, "rows_alternate": rows_alternate, "cols_alternate": cols_alternate, "stripes": stripes, "slots": slots,
           "control": control}


def panel(n, m, spec):
    """spec = (maker name, further arguments...)"""
    return _MAKERS[spec[0]](n, m, *spec[1:])


def name(spec):
    return spec[0] + "(" + ", ".join(str(a) for a in spec[1:]) + ")"


# ---------------------------------------------------------------------------------------------------------------------
# class vectors: (gid int32, G, ploidy or None)
def blocks(n, G):
    """contiguous runs of individuals: most class tiles of a 128-individual group are empty"""
    return (np.arange(n) * G // n).astype(np.int32), G, None


def round_robin(n, G):
    return (np.arange(n) % G).astype(np.int32), G, None


def last_only(n, G):
    return np.full(n, G - 1, dtype=np.int32), G, None


def singletons(n, G):
    assert G == n
    return np.arange(n, dtype=np.int32), G, None


def edge(n, G):
    """individuals on the two sides of the 32- and 64-class tile boundaries and in the last class, nowhere else"""
    assert G >= 65
    where = np.array(sorted({0, 31, 32, 63, 64, G - 1}), dtype=np.int32)
    return where[np.arange(n) % len(where)], G, None


def hap(n, G):
    """round_robin ids, ploidy alternating 2 / 1 (in steps of G individuals, so that every group has both where n allows)"""
    return (np.arange(n) % G).astype(np.int32), G, np.where((np.arange(n) // G) % 2 == 0, 2.0, 1.0)


CLASS_BUILDERS = {"blocks": blocks, "round_robin": round_robin, "last_only": last_only, "singletons": singletons, "edge": edge,
                  "hap": hap}


def pseudohaploid(g, ploidy):
    """the panel as a store holds it: pseudohaploid individuals are 0 / 2, a 1 is rewritten to 2"""
    g = np.array(g, order="F")
    rows = np.asarray(ploidy) == 1.0
    sub = g[rows]
    sub[sub == 1] = 2
    g[rows] = sub
    return _f(g)


def class_plan_ids(gid, G, ploidy):
    """(cls, nclass) as make_class_plan builds them: 2 g + hap with 2 G classes as soon as one individual is pseudohaploid"""
    if ploidy is None or not (np.asarray(ploidy) == 1.0).any():
        return np.asarray(gid, dtype=np.int32), G
    return (2 * np.asarray(gid) + (np.asarray(ploidy) == 1.0)).astype(np.int32), 2 * G


# ---------------------------------------------------------------------------------------------------------------------
# references, each twice: vectorised and as a plain loop
def loci_counts(g):
    return np.stack([(g == c).sum(axis=0) for c in range(4)], axis=1).astype(np.int32)


def loci_counts_loop(g):
    n, m = g.shape
    out = np.zeros((m, 4), dtype=np.int32)
    for j in range(m):
        for i in range(n):
            out[j, g[i, j]] += 1
    return out


def indiv_counts(g):
    return np.stack([(g == c).sum(axis=1) for c in range(4)], axis=1).astype(np.int32)


def indiv_counts_loop(g):
    n, m = g.shape
    out = np.zeros((n, 4), dtype=np.int32)
    for i in range(n):
        for j in range(m):
            out[i, g[i, j]] += 1
    return out


def _onehot(ids, ncol):
    oh = np.zeros((len(ids), ncol), dtype=np.int64)
    ok = ids >= 0
    oh[np.nonzero(ok)[0], ids[ok]] = 1
    return oh


def class_counts(g, gid, G):
    """(3, m, G): [k, j, c] = individuals of class c with k alternate alleles at locus j"""
    oh = _onehot(np.asarray(gid), G)
    return np.stack([(g == k).astype(np.int64).T @ oh for k in range(3)]).astype(np.int32)


def class_counts_loop(g, gid, G):
    n, m = g.shape
    out = np.zeros((3, m, G), dtype=np.int32)
    for i in range(n):
        for j in range(m):
            if g[i, j] < 3:
                out[g[i, j], j, gid[i]] += 1
    return out


def class_missing(g, gid, G):
    """(m, G): missing genotypes of class c at locus j"""
    return ((g == 3).astype(np.int64).T @ _onehot(np.asarray(gid), G)).astype(np.int32)


def class_missing_loop(g, gid, G):
    n, m = g.shape
    out = np.zeros((m, G), dtype=np.int32)
    for i in range(n):
        for j in range(m):
            out[j, gid[i]] += g[i, j] == 3
    return out


def hap_table(g, gid, G, ploidy, swapped=False):
    """(m, 2 G) doubles, the as_counts table of the grouped allele frequencies restated from the class counts as tpg_group_vals
    reads them: alt = n1d + 2 n2d + (n1h + 2 n2h) / 2, valid = 2 nvd + nvh.  swapped: the 2 g + hap interleave the wrong way."""
    h = (np.asarray(ploidy) == 1.0).astype(np.int64)
    cls = 2 * np.asarray(gid, dtype=np.int64) + (1 - h if swapped else h)
    c = class_counts(g, cls, 2 * G).astype(np.int64)
    nv = c.sum(axis=0)
    d, hp = slice(0, 2 * G, 2), slice(1, 2 * G, 2)
    alt = (c[1][:, d] + 2 * c[2][:, d]) + 0.5 * (c[1][:, hp] + 2 * c[2][:, hp])
    valid = 2.0 * nv[:, d] + nv[:, hp]
    return np.asfortranarray(np.concatenate([alt, valid], axis=1))


def hap_table_loop(g, gid, G, ploidy):
    """the same table the way the reference sums it: x / (3 - ploidy) and ploidy per typed genotype"""
    n, m = g.shape
    out = np.zeros((m, 2 * G), order="F")
    for i in range(n):
        for j in range(m):
            if g[i, j] < 3:
                out[j, gid[i]] += g[i, j] / (3.0 - ploidy[i])
                out[j, G + gid[i]] += ploidy[i]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# restated plans
def loci_plan(n, m):
    """tpg_loci_counts over L, and what the fast pack kernel leaves beside the layouts"""
    Q, KG = _cdiv(n, 128), _cdiv(m, 128)
    fast = n % 8 == 0
    chunks = _cdiv(Q, 2) if fast else 0
    return dict(Q=Q, KG=KG, npad=Q * 128 - n, full_passes=Q // 4, remainder=Q % 4, fast_pack=fast, chunks=chunks,
                last_chunk_rows=n - 256 * (chunks - 1) if fast else 0, half_thread=n % 16 == 8, last_tile_loci=m - 32 * (_cdiv(m, 32) - 1))


def indiv_plan(n, m):
    """tpg_indiv_counts: the loci kernel on T, KG in the place of Q"""
    Q, KG = _cdiv(n, 128), _cdiv(m, 128)
    return dict(Q=Q, KG=KG, pad=KG * 128 - m, full_passes=KG // 4, remainder=KG % 4,
                origins=3 if n % 8 == 0 else 1)  # (a panel the fast pack kernel does not take is packed with T for every view)


def accumulate_plan(n, m, num_cu=256):
    """tpg_launch_indiv_accumulate"""
    Q, n_lt = _cdiv(n, 128), _cdiv(m, 32)
    gx = _cdiv(Q, 4)
    tiles = _cdiv(_cdiv(n_lt, _cdiv(4 * num_cu, gx)), 15) * 15
    tiles = 30 if tiles < 30 else 255 if tiles > 255 else tiles
    gy = _cdiv(n_lt, tiles)
    last = n_lt - (gy - 1) * tiles
    return dict(Q=Q, gx=gx, idle_waves=4 * gx - Q, n_lt=n_lt, tiles=tiles, gy=gy, last_piece_tiles=last,
                last_piece_steps=_cdiv(last, 15), last_tile_loci=m - 32 * (n_lt - 1))


def chain(GT):
    return [2] * (GT // 2) + [1] * (GT % 2)


def grouped_plan(n, m, nclass):
    """tpg_grouped_counts"""
    Q, GT = _cdiv(n, 128), _cdiv(nclass, 32)
    return dict(Q=Q, KG=_cdiv(m, 128), full_passes=Q // 4, remainder=Q % 4, GT=GT, chain=chain(GT), npad=Q * 128 - n)


def empty_class_tiles(cls, nclass):
    """the (128-individual group, class tile) pairs without one individual"""
    cls = np.asarray(cls)
    Q, GT = _cdiv(len(cls), 128), _cdiv(nclass, 32)
    seen = {(i // 128, int(c) // 32) for i, c in enumerate(cls)}
    return [(q, t) for q in range(Q) for t in range(GT) if (q, t) not in seen]


# ---------------------------------------------------------------------------------------------------------------------
# the kernels restated, with their knobs
def _pad_rows(g, rows, fill=3):
    out = np.full((rows, g.shape[1]), fill, dtype=np.uint8)
    out[: g.shape[0]] = g
    return out


def loci_kernel_model(g, npad_kept=False, npad_off_n0=False, remainder_dropped=False):
    """tpg_loci_counts_kernel: blocks of 128 individuals, padded with the missing code, four at a time and a remainder loop;
    the padding comes off the missing count afterwards"""
    n, m = g.shape
    Q = _cdiv(n, 128)
    gp = _pad_rows(g, Q * 128).astype(np.int64)
    c_lo, c_hi, c_both = (np.zeros(m, dtype=np.int64) for _ in range(3))

    def acc(q):
        blk = gp[128 * q: 128 * q + 128]
        c_lo[:] += (blk & 1).sum(axis=0)
        c_hi[:] += ((blk >> 1) & 1).sum(axis=0)
        c_both[:] += ((blk & 1) & (blk >> 1)).sum(axis=0)

    q = 0
    while q + 4 <= Q:
        for k in range(4):
            acc(q + k)
        q += 4
    if not remainder_dropped:
        while q < Q:
            acc(q)
            q += 1
    n3, n1, n2 = c_both, c_lo - c_both, c_hi - c_both
    npad = Q * 128 - n
    n0 = Q * 128 - n1 - n2 - n3
    if npad_kept:
        return np.stack([n0, n1, n2, n3], axis=1).astype(np.int32)
    if npad_off_n0:
        return np.stack([n0 - npad, n1, n2, n3], axis=1).astype(np.int32)
    return np.stack([n0, n1, n2, n3 - npad], axis=1).astype(np.int32)


def indiv_kernel_model(g, pad_kept=False):
    """tpg_indiv_counts: the same code on T, the roles of n and m swapped"""
    return loci_kernel_model(np.ascontiguousarray(g.T), npad_kept=pad_kept)


def pack_partials_model(g, wraps_at_256=False, half_mask_off=False):
    """the fast pack kernel's partial counts + tpg_loci_counts_sum_kernel: per chunk of 256 individuals and locus three fields
    {bit 0 set, bit 1 set, both} of ten bits; a thread holds 16 individuals from i0 = 16 t, counts all of them if i0 + 16 <= n,
    the first eight if i0 + 8 <= n, none otherwise (what it did not load it packed as the missing code)"""
    n, m = g.shape
    assert n % 8 == 0
    chunks = _cdiv(n, 256)
    gp = _pad_rows(g, chunks * 256).astype(np.int64)
    i = np.arange(chunks * 256)
    i0 = i // 16 * 16
    counted = np.where(i - i0 < 8, i0 + 8 <= n, i0 + 8 <= n if half_mask_off else i0 + 16 <= n)
    field = 255 if wraps_at_256 else 1023
    lo, hi, both = (np.zeros(m, dtype=np.int64) for _ in range(3))
    for c in range(chunks):
        rows = slice(256 * c, 256 * c + 256)
        blk = gp[rows] * counted[rows, None]  # (a row not counted adds to no field)
        lo += (blk & 1).sum(axis=0) & field
        hi += ((blk >> 1) & 1).sum(axis=0) & field
        both += ((blk & 1) & (blk >> 1)).sum(axis=0) & field
    n1, n2 = lo - both, hi - both
    return np.stack([n - n1 - n2 - both, n1, n2, both], axis=1).astype(np.int32)


def indiv_accumulate_model(g, num_cu=256, loci_per_field2=3, groups_per_field4=5, mask=True, piece_start=0):
    """tpg_indiv_accumulate_kernel + tpg_indiv_finish_kernel, literally in the packed fields of a lane: a dword holds the codes of 16
    individuals at one locus; `loci_per_field2` loci are added in the sixteen 2-bit fields, `groups_per_field4` such groups in
    eight 4-bit fields, the steps of a piece in bytes, the 32 lanes of a tile in 16-bit fields, all as uint32 additions that
    wrap and carry as the device's do.  Element e sits at bits 8 (e & 3) + 2 (e >> 2) as on the device (tpg_elem_shift), so a carry
    falls into the same neighbour: out of a saturated even individual into an odd one in one field in four, two and one.
    piece_start: -1 = a piece after the first counts the tile before it again, +1 = it skips its first tile."""
    n, m = g.shape
    p = accumulate_plan(n, m, num_cu)
    Q, n_lt, tiles, gy = p["Q"], p["n_lt"], p["tiles"], p["gy"]
    gp = np.full((Q * 128, n_lt * 32), 3, dtype=np.uint32)
    gp[:n, :m] = g
    e = np.arange(16, dtype=np.uint32).reshape(1, 1, 1, 16, 1, 1)
    W = (gp.reshape(Q, 4, 2, 16, n_lt, 32) << (8 * (e & 3) + 2 * (e >> 2))).sum(axis=3, dtype=np.uint32)  # [q, s, h, lt, r]
    W = np.ascontiguousarray(W.transpose(3, 0, 1, 2, 4))  # [lt][q, s, h, r]
    r = np.arange(32)
    u32 = np.uint32
    acc = np.zeros((3, Q * 128), dtype=np.int64)
    step = loci_per_field2 * groups_per_field4
    for by in range(gy):
        lt0, lt1 = by * tiles, min(by * tiles + tiles, n_lt)
        if by > 0:
            lt0 += piece_start
        a8 = np.zeros((3, 4) + W.shape[1:], dtype=np.uint32)  # [plane][k]: byte b = element 4 k + b
        for base in range(lt0, lt1, step):
            a4 = np.zeros((3, 2) + W.shape[1:], dtype=np.uint32)
            for gq in range(groups_per_field4):
                a2 = np.zeros((3,) + W.shape[1:], dtype=np.uint32)
                for u in range(loci_per_field2):
                    lt = base + loci_per_field2 * gq + u
                    if lt >= lt1:
                        continue
                    w = W[lt]
                    if mask:
                        w = np.where(lt * 32 + r < m, w, u32(0))
                    lo, hi = w & u32(0x55555555), (w >> u32(1)) & u32(0x55555555)
                    a2[0] += lo
                    a2[1] += hi
                    a2[2] += lo & hi
                a4[:, 0] += a2 & u32(0x33333333)
                a4[:, 1] += (a2 >> u32(2)) & u32(0x33333333)
            for k in range(2):
                a8[:, k] += a4[:, k] & u32(0x0F0F0F0F)
                a8[:, 2 + k] += (a4[:, k] >> u32(4)) & u32(0x0F0F0F0F)
        ev = (a8 & u32(0x00FF00FF)).sum(axis=-1, dtype=np.uint32)  # over the 32 lanes of a tile, in 16-bit fields
        od = ((a8 >> u32(8)) & u32(0x00FF00FF)).sum(axis=-1, dtype=np.uint32)
        c = np.stack([ev & u32(0xFFFF), od & u32(0xFFFF), ev >> u32(16), od >> u32(16)])  # [b][plane][k][q, s, h]
        acc += c.transpose(1, 3, 4, 5, 2, 0).reshape(3, Q * 128)  # individual 128 q + 32 s + 16 h + 4 k + b
    acc = acc[:, :n]  # rows past n are not written
    n1, n2 = acc[0] - acc[2], acc[1] - acc[2]
    return np.stack([m - n1 - n2 - acc[2], n1, n2, acc[2]], axis=1).astype(np.int32)


def grouped_kernel_model(g, cls, nclass, tile_mod32=False, last_group_twice=False, last_group_dropped=False,
                         second_step_dropped=False, csize_padded=False):
    """tpg_onehot_kernel + tpg_grouped_counts_kernel: per 128-individual group two steps of 64 individuals, the planes {bit 0,
    bit 1, both} against the one-hot class matrix; het = Y - W, hom-alt = Z - W, valid = class size - W.  Returns
    (counts (3, m, nclass) as tpg_grouped_genotype_counts reads them, missing (m, nclass) = class size - valid)."""
    n, m = g.shape
    cls = np.asarray(cls, dtype=np.int64)
    Q, GT = _cdiv(n, 128), _cdiv(nclass, 32)
    Cpad = 32 * GT
    gp = _pad_rows(g, Q * 128).astype(np.int64)
    cp = np.full(Q * 128, -1, dtype=np.int64)
    cp[:n] = cls % 32 if tile_mod32 else cls
    groups = list(range(Q))
    if last_group_twice:
        groups.append(Q - 1)
    if last_group_dropped:
        groups.pop()
    sums = np.zeros((3, m, Cpad), dtype=np.int64)
    for q in groups:
        for S in range(1 if second_step_dropped else 2):
            rows = slice(128 * q + 64 * S, 128 * q + 64 * S + 64)
            x, oh = gp[rows], _onehot(cp[rows], Cpad)
            y, z = x & 1, (x >> 1) & 1
            sums[0] += y.T @ oh
            sums[1] += z.T @ oh
            sums[2] += (y & z).T @ oh
    csize = np.bincount(cls, minlength=Cpad)
    true_size = csize.copy()
    if csize_padded:
        csize[0] += Q * 128 - n
    het, hom, valid = sums[0] - sums[2], sums[1] - sums[2], csize[None, :] - sums[2]
    counts = np.stack([valid - het - hom, het, hom])[:, :, :nclass].astype(np.int32)
    return counts, (true_size[None, :] - valid)[:, :nclass].astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# the case tables of tests/test_gpu_counts.py: shape, then the edge the case is there for as values of its restated plan

# per-locus counts: (n, m, edge of loci_plan)
LOCI_PANELS = [("const", 3), ("const", 1), ("rows_alternate", 3, 0), ("stripes", 4, 1), ("stripes", 128, 32), ("control",)]
LOCI_CASES = [
    (1, 1, dict(Q=1, npad=127, fast_pack=False, last_tile_loci=1)),
    (8, 31, dict(Q=1, fast_pack=True, chunks=1, last_chunk_rows=8, half_thread=True)),
    (127, 32, dict(Q=1, npad=1, fast_pack=False, last_tile_loci=32)),
    (128, 33, dict(Q=1, npad=0, chunks=1, last_chunk_rows=128, half_thread=False, last_tile_loci=1)),
    (129, 128, dict(Q=2, npad=127, remainder=2, fast_pack=False, KG=1)),
    (248, 129, dict(Q=2, chunks=1, last_chunk_rows=248, half_thread=True, KG=2)),
    (256, 1000, dict(Q=2, npad=0, chunks=1, last_chunk_rows=256, half_thread=False)),
    (264, 1, dict(Q=3, remainder=3, chunks=2, last_chunk_rows=8, half_thread=True)),
    (264, 1000, dict(Q=3, chunks=2, last_chunk_rows=8, half_thread=True, KG=8)),
    (385, 33, dict(Q=4, full_passes=1, remainder=0, npad=127, fast_pack=False)),
    (512, 129, dict(Q=4, full_passes=1, remainder=0, npad=0, chunks=2, last_chunk_rows=256)),
    (520, 1000, dict(Q=5, full_passes=1, remainder=1, chunks=3, last_chunk_rows=8, half_thread=True)),
    (640, 32, dict(Q=5, full_passes=1, remainder=1, npad=0, chunks=3, last_chunk_rows=128, half_thread=False)),
    (1025, 31, dict(Q=9, full_passes=2, remainder=1, npad=127, fast_pack=False)),
    (1025, 128, dict(Q=9, full_passes=2, remainder=1, fast_pack=False, KG=1, last_tile_loci=32)),
]

# per-individual counts from T: (n, m, edge of indiv_plan)
T_PANELS = [("const", 3), ("const", 1), ("const", 0), ("cols_alternate", 3, 0), ("stripes", 16, 32), ("stripes", 4, 1), ("control",)]
T_CASES = [
    (1, 127, dict(KG=1, pad=1, origins=1)),
    (33, 1, dict(KG=1, pad=127, origins=1)),
    (130, 128, dict(KG=1, pad=0, Q=2, origins=1)),
    (136, 129, dict(KG=2, pad=127, remainder=2, origins=3)),
    (264, 511, dict(KG=4, pad=1, full_passes=1, remainder=0, origins=3)),
    (136, 513, dict(KG=5, pad=127, full_passes=1, remainder=1, origins=3)),
    (33, 513, dict(KG=5, full_passes=1, remainder=1, origins=1)),
    (264, 1153, dict(KG=10, pad=127, full_passes=2, remainder=2, origins=3)),
    (130, 1153, dict(KG=10, full_passes=2, remainder=2, origins=1)),
]

# per-individual counts from L: (n, m, edge of accumulate_plan); tiles = 30 at every one of them, for any CU count from 8 up
ACC_PANELS = [("const", c) for c in range(4)] + [("rows_alternate", a, b) for a, b in ((3, 0), (0, 3), (1, 0), (2, 0))] + [
    ("stripes", 16, 32), ("stripes", 4, 96), ("stripes", 32, 480), ("stripes", 128, 960), ("control",)]
ACC_CASES = [
    (1, 1, dict(n_lt=1, gy=1, last_tile_loci=1, idle_waves=3)),
    (127, 31, dict(n_lt=1, last_tile_loci=31, Q=1, idle_waves=3)),
    (129, 33, dict(n_lt=2, last_tile_loci=1, Q=2, idle_waves=2)),
    (385, 479, dict(n_lt=15, last_piece_steps=1, last_tile_loci=31, idle_waves=0)),
    (129, 480, dict(n_lt=15, last_piece_steps=1, last_tile_loci=32, idle_waves=2)),
    (513, 480, dict(n_lt=15, last_piece_steps=1, last_tile_loci=32, Q=5, gx=2, idle_waves=3)),
    (640, 481, dict(n_lt=16, last_piece_steps=2, last_tile_loci=1, gx=2, idle_waves=3)),
    (1, 959, dict(n_lt=30, gy=1, last_piece_tiles=30, last_tile_loci=31)),
    (127, 960, dict(n_lt=30, gy=1, last_piece_tiles=30, last_tile_loci=32)),
    (513, 960, dict(n_lt=30, gy=1, last_piece_tiles=30, gx=2, idle_waves=3)),
    (129, 961, dict(n_lt=31, gy=2, last_piece_tiles=1, last_tile_loci=1)),
    (385, 961, dict(n_lt=31, gy=2, last_piece_tiles=1, last_tile_loci=1, idle_waves=0)),
    (385, 1921, dict(n_lt=61, gy=3, last_piece_tiles=1, last_tile_loci=1)),
    (640, 1921, dict(n_lt=61, gy=3, last_piece_tiles=1, gx=2, idle_waves=3)),
]
ACC_BLOCK_LOCI = 128  # the streamed pass under a budget: blocks of 128 loci, at least three with a narrower last one from m = 479 up

# per-class counts: (n, m, class builder, G, edge of grouped_plan + "empty": some class tile of some 128-group has nobody)
CLASS_PANELS = [("const", 3), ("const", 1), ("slots",), ("stripes", 16, 1), ("stripes", 64, 32), ("stripes", 128, 96), ("control",)]
CLASS_CASES = [
    (1, 1, "round_robin", 1, dict(Q=1, GT=1, chain=[1], npad=127)),
    (1, 33, "last_only", 31, dict(Q=1, GT=1, chain=[1])),
    (127, 129, "singletons", 127, dict(Q=1, GT=4, chain=[2, 2], npad=1)),
    (129, 33, "singletons", 129, dict(Q=2, GT=5, chain=[2, 2, 1], empty=True)),
    (127, 500, "blocks", 32, dict(Q=1, GT=1, chain=[1], KG=4)),
    (129, 1, "round_robin", 33, dict(Q=2, remainder=2, GT=2, chain=[2])),
    (257, 129, "blocks", 64, dict(Q=3, remainder=3, GT=2, chain=[2], empty=True)),
    (385, 33, "edge", 65, dict(Q=4, full_passes=1, remainder=0, GT=3, chain=[2, 1])),
    (513, 500, "round_robin", 96, dict(Q=5, full_passes=1, remainder=1, GT=3, chain=[2, 1])),
    (641, 129, "edge", 97, dict(Q=6, full_passes=1, remainder=2, GT=4, chain=[2, 2])),
    (769, 33, "blocks", 129, dict(Q=7, full_passes=1, remainder=3, GT=5, chain=[2, 2, 1], empty=True)),
    (897, 129, "round_robin", 160, dict(Q=8, full_passes=2, remainder=0, GT=5, chain=[2, 2, 1])),
    (897, 1, "last_only", 64, dict(Q=8, GT=2, chain=[2], empty=True)),
    (1025, 33, "last_only", 160, dict(Q=9, full_passes=2, remainder=1, GT=5, chain=[2, 2, 1], empty=True)),
    (1153, 500, "edge", 160, dict(Q=10, full_passes=2, remainder=2, GT=5, chain=[2, 2, 1], empty=True)),
    (1153, 129, "blocks", 31, dict(Q=10, full_passes=2, remainder=2, GT=1, chain=[1])),
    (129, 33, "hap", 16, dict(Q=2, GT=1, chain=[1])),
    (641, 129, "hap", 17, dict(Q=6, remainder=2, GT=2, chain=[2])),
    (1025, 500, "hap", 33, dict(Q=9, full_passes=2, remainder=1, GT=3, chain=[2, 1])),
]
CLASS_NS = (1, 127, 129, 257, 385, 513, 641, 769, 897, 1025, 1153)
CLASS_GS = (1, 31, 32, 33, 64, 65, 96, 97, 129, 160)


def class_case(n, builder, G):
    """(gid, G, ploidy, cls, nclass) of a case"""
    gid, G, ploidy = CLASS_BUILDERS[builder](n, G)
    cls, nclass = class_plan_ids(gid, G, ploidy)
    return gid, G, ploidy, cls, nclass


def class_panels(m):
    return [s for s in CLASS_PANELS if s[0] != "slots" or m >= 128]


# ---------------------------------------------------------------------------------------------------------------------
# fault models: name -> (family, function of a panel (and a class case) giving what the faulted kernel would return)
def _grouped_fault(**knob):
    def run(g, gid, G, ploidy):
        cls, nclass = class_plan_ids(gid, G, ploidy)
        return grouped_kernel_model(g, cls, nclass, **knob)
    return run


FAULTS = {
    "loci_npad_kept": ("loci", lambda g: loci_kernel_model(g, npad_kept=True)),
    "loci_npad_off_n0": ("loci", lambda g: loci_kernel_model(g, npad_off_n0=True)),
    "loci_remainder_dropped": ("loci", lambda g: loci_kernel_model(g, remainder_dropped=True)),
    "indiv_pad_kept": ("indiv", lambda g: indiv_kernel_model(g, pad_kept=True)),
    "acc_four_loci_per_2bit_field": ("acc", lambda g: indiv_accumulate_model(g, loci_per_field2=4)),
    "acc_six_groups_per_4bit_field": ("acc", lambda g: indiv_accumulate_model(g, groups_per_field4=6)),
    "acc_locus_mask_off": ("acc", lambda g: indiv_accumulate_model(g, mask=False)),
    "acc_piece_counts_its_first_tile_twice": ("acc", lambda g: indiv_accumulate_model(g, piece_start=-1)),
    "acc_piece_skips_its_first_tile": ("acc", lambda g: indiv_accumulate_model(g, piece_start=1)),
    "grouped_class_in_tile_c_mod_32": ("grouped", _grouped_fault(tile_mod32=True)),
    "grouped_last_group_twice": ("grouped", _grouped_fault(last_group_twice=True)),
    "grouped_last_group_dropped": ("grouped", _grouped_fault(last_group_dropped=True)),
    "grouped_second_step_dropped": ("grouped", _grouped_fault(second_step_dropped=True)),
    "grouped_csize_over_padded_count": ("grouped", _grouped_fault(csize_padded=True)),
    "grouped_hap_interleave_swapped": ("hap", lambda g, gid, G, ploidy: hap_table(g, gid, G, ploidy, swapped=True)),
    "pack_field_wraps_at_256": ("pack", lambda g: pack_partials_model(g, wraps_at_256=True)),
    "pack_half_thread_mask_off": ("pack", lambda g: pack_partials_model(g, half_mask_off=True)),
}
