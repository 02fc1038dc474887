"""numpy restatement of simple imputation (include/tpg.h: TPG_IMPUTE_MODE / _MEAN0 / _RANDOM), integers only.

`codes` is an n x m array of genotype codes 0, 1, 2 and 3 = missing: the rows / columns of the object being imputed
(a whole store, or the kept rows and columns of a view).  Every function returns the filled codes (0, 1, 2; 3 only where
a locus has nobody typed); `store_bytes` turns raw store bytes into what tpg_fbm_impute_simple leaves (3 -> 4 + fill).
"""
import numpy as np

METHODS = ("mode", "mean0", "random")
_M64 = (1 << 64) - 1


def mix64(x):
    """tpg_mix64 (csrc/synth_common.h): the splitmix64 finaliser, on uint64 arrays (wraps modulo 2^64)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def mix64_int(x: int) -> int:
    """the same on one Python int (the arithmetic written out, as a cross-check of the array form)"""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def counts(codes):
    codes = np.asarray(codes)
    return [np.sum(codes == g, axis=0, dtype=np.int64) for g in (0, 1, 2)]


def fill_mode(c0, c1, c2):
    """most frequent genotype, the smaller one on a tie (which.max)"""
    return np.argmax(np.stack([c0, c1, c2]), axis=0)  # argmax returns the first maximum


def fill_mean0(c0, c1, c2):
    """round(s / t) half to even, decided in integers: 0.5 -> 0, 1.5 -> 2"""
    t, s2 = c0 + c1 + c2, 2 * (c1 + 2 * c2)
    return np.where(s2 <= t, 0, np.where(s2 < 3 * t, 1, 2))


def draws(seed: int, n: int, m: int, c0, c1, c2, row0: int = 0, col0: int = 0):
    """the `random` fill of EVERY entry (i, j) of an n x m object, were it missing"""
    t, s = c0 + c1 + c2, c1 + 2 * c2
    thr = np.array([(int(sj) << 31) // int(tj) if tj > 0 else 0 for sj, tj in zip(s, t)], dtype=np.uint64)
    key = mix64(np.uint64(seed) ^ mix64(np.arange(col0, col0 + m, dtype=np.uint64)))
    h = mix64(key[None, :] ^ mix64(np.arange(row0, row0 + n, dtype=np.uint64))[:, None])
    u1, u2 = h >> np.uint64(32), h & np.uint64(0xFFFFFFFF)
    return (u1 < thr[None, :]).astype(np.uint8) + (u2 < thr[None, :]).astype(np.uint8)


def impute_codes(codes, method: str, seed: int = 0):
    codes = np.asarray(codes, dtype=np.uint8)
    n, m = codes.shape
    c0, c1, c2 = counts(codes)
    typed = (c0 + c1 + c2) > 0
    if method == "mode":
        fill = np.broadcast_to(fill_mode(c0, c1, c2).astype(np.uint8), (n, m))
    elif method == "mean0":
        fill = np.broadcast_to(fill_mean0(c0, c1, c2).astype(np.uint8), (n, m))
    elif method == "random":
        fill = draws(seed, n, m, c0, c1, c2)
    else:
        raise ValueError(method)
    out = codes.copy()
    where = (codes == 3) & typed[None, :]
    out[where] = fill[where]
    return out


def report(codes):
    codes = np.asarray(codes)
    c0, c1, c2 = counts(codes)
    typed = (c0 + c1 + c2) > 0
    return {"imputed": int(np.sum((codes == 3) & typed[None, :])), "loci_all_missing": int(np.sum(~typed))}


def store_bytes(raw, method: str, seed: int = 0):
    """raw CODE_012 store bytes (0, 1, 2, 3) -> the bytes after tpg_fbm_impute_simple: a filled entry is 4 + fill"""
    raw = np.asarray(raw, dtype=np.uint8)
    assert raw.max(initial=0) <= 3
    filled = impute_codes(raw, method, seed)
    out = raw.copy()
    where = (raw == 3) & (filled != 3)
    out[where] = 4 + filled[where]
    return out


def decode_imputed(store):
    """store bytes through CODE_IMPUTE_PRED as 2-bit codes: 0..2 and 4..6 -> genotype, everything else 3"""
    store = np.asarray(store, dtype=np.uint8)
    out = np.full(store.shape, 3, dtype=np.uint8)
    out[store < 3] = store[store < 3]
    hi = (store >= 4) & (store <= 6)
    out[hi] = store[hi] - 4
    return out
