"""Run by tests/test_host_sanitizers.py in a child process whose LD_PRELOAD is the ASan runtime: drives the sanitizer build
of shim/tpg_rshim.c + tests/rmock/rmock.c + tests/host/tpg_stub.c (a host stand-in for libtpg_hip.so) the way the R drivers
drive the shim: the table of mapped files, the cache, the per-call uploads, and then every reference symbol under the mock's
GC torture and strict arguments, with integer and double indices, and with each of its allocations failing in turn.
usage: drive_shim_san.py <lib.so> <tmpdir>"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import rmock  # noqa: E402

so, tmp = sys.argv[1], sys.argv[2]
lib = rmock.bind(C.CDLL(so))
r = rmock.Session(lib)
counter = lambda name: C.c_int.in_dll(lib, name).value  # noqa: E731

rng = np.random.default_rng(7)
n_all, m_all = 37, 900
fbm = rng.integers(0, 4, size=(n_all, m_all)).astype(np.uint8)
bk = os.path.join(tmp, "geno.bk")
fbm.T.tofile(bk)
code = np.full(256, np.nan)
code[:3] = [0, 1, 2]
rows = (rng.permutation(n_all)[:29] + 1).astype(np.int32)
ploidy = np.full(len(rows), 2.0)


def expect(cols):
    sub = fbm[np.ix_(rows - 1, cols - 1)].astype(float)
    sub[sub == 3] = np.nan
    return np.stack([np.nansum(sub, axis=0), 2.0 * np.sum(~np.isnan(sub), axis=0)], axis=1)


def alt_freq(BM, cols):
    out = r.call("alt_freq_dip_pseudo_cpp", BM, r.int(rows), r.int(cols), r.real(ploidy), r.int([1]), lib.rmock_lgl(1))
    return r.as_numpy(out, (len(cols), 2))


for cache in (False, True):
    os.environ.pop("TPG_RSHIM_CACHE", None)
    if cache:
        os.environ["TPG_RSHIM_CACHE"] = "1"
    BM = r.fbm(bk, n_all, m_all, code)
    up0 = counter("g_stub_uploads")
    # the big_apply blocks of the R driver (contiguous), a reversed block, a scattered colInd (gathered upload), one column
    for cols in (np.arange(1, 301), np.arange(301, 901), np.arange(600, 100, -1), np.arange(1, 901, 13), np.array([900])):
        cols = cols.astype(np.int32)
        assert np.array_equal(alt_freq(BM, cols), expect(cols)), (cache, cols[:4])
    if cache:
        assert counter("g_stub_uploads") == up0 + 1, "the cached FBM was uploaded more than once"
        r.call("tpg_invalidate", BM)
        assert counter("g_stub_fbm_alive") == 0
        assert np.array_equal(alt_freq(BM, np.arange(1, 11, dtype=np.int32)), expect(np.arange(1, 11)))
        assert counter("g_stub_uploads") == up0 + 2
    else:
        assert counter("g_stub_uploads") == up0 + 5 and counter("g_stub_fbm_alive") == 0, "a per-call upload outlived its call"
    assert counter("g_stub_view_alive") == 0
    # an out-of-range colInd is an R error, and nothing leaks on the way out
    try:
        alt_freq(BM, np.array([m_all + 1], dtype=np.int32))
        raise SystemExit("out-of-range colInd accepted")
    except RuntimeError:
        pass
    assert counter("g_stub_view_alive") == 0
    r.call("tpg_release")
    assert counter("g_stub_fbm_alive") == 0

# the block loops of three analyses one after the other on file-backed accumulators: the table of mapped files grows,
# entries are forgotten (swap-compaction) while others are in use, pointers handed out stay valid
os.environ.pop("TPG_RSHIM_CACHE", None)
BM = r.fbm(bk, n_all, m_all, code)
n = len(rows)
cols = np.arange(1, m_all + 1, dtype=np.int32)
for which in ("ibs", "king", "as", "ibs"):
    files = []
    for nm in ("k", "k2"):
        f = os.path.join(tmp, f"{which}_{nm}_{len(files)}_{np.random.randint(1 << 30)}.bk")
        np.zeros(n * n).tofile(f)
        files.append(f)
    K, K2 = r.fbm(files[0], n, n), r.fbm(files[1], n, n)
    lo, up = np.array([1, 241, 481, 722]), np.array([240, 480, 721, 900])
    rmock.driver_loop(r, which, BM, K, K2, rows, cols, lo, up, scratch_width=1)
    k = np.fromfile(files[0]).reshape(n, n, order="F")
    k2 = np.fromfile(files[1]).reshape(n, n, order="F")
    assert k[0, 0] == m_all and k2[n - 1, n - 1] == 4 * n and k.sum() == m_all, which
maps = open("/proc/self/maps").read()
assert maps.count("_k_") + maps.count("_k2_") <= 2, "accumulators of earlier analyses are still mapped"
r.call("tpg_release")
maps = open("/proc/self/maps").read()
assert "_k_" not in maps and "_k2_" not in maps and "geno.bk" not in maps

# the whole-analysis entry point with a `which` mask: NULL for what was not asked, bad masks refused
BM = r.fbm(bk, n_all, m_all, code)
out = r.call("tpg_snp_pairwise", BM, r.int(rows), r.int(cols), lib.rmock_lgl(0), r.int([2 | 8]))
assert lib.TYPEOF(lib.VECTOR_ELT(out, 0)) == 0 and lib.TYPEOF(lib.VECTOR_ELT(out, 2)) == 0
assert np.all(r.list_elt(out, 1, (n, n)) == 2.0 * m_all) and np.all(r.list_elt(out, 3, (n, n)) == 4.0 * m_all)
for bad in (0, 16):
    try:
        r.call("tpg_snp_pairwise", BM, r.int(rows), r.int(cols), lib.rmock_lgl(0), r.int([bad]))
        raise SystemExit("bad which mask accepted")
    except RuntimeError:
        pass
# ---- every reference symbol, under GC torture and with its arguments checked for writes, with integer and with double
# indices; then each one with its k-th allocation failing, k = 1, 2, ... until the call goes through ----
os.environ.pop("TPG_RSHIM_CACHE", None)
BM = r.fbm(bk, n_all, m_all, code)
G = 3
gid = (np.arange(len(rows)) % G).astype(np.int32)
cols = np.array([5, 9, 1, 400, 77, 78, 79, 900], dtype=np.int32)
m = len(cols)
fa_in = rng.uniform(0.1, 0.9, size=(m, G))
S = dict(n=np.full((m, G), 20.0), fa=fa_in, fr=1 - fa_in, het=rng.uniform(0, 0.5, size=(m, G)))
S["n"][2, 1] = rmock.na_real()
pairs = np.array([[2, 1], [3, 3], [1, 2]], dtype=np.int32).T  # 2 x P, unsorted
V = rng.standard_normal((m, 3))


def entry_calls(double):
    """{symbol: (argument builder, check of the result)} for the 14 reference symbols"""
    ix = lambda v: r.index(v, double)  # noqa: E731
    gids = lambda: r.index(gid, double)  # noqa: E731
    ng = lambda: r.index([G], double)  # noqa: E731
    pl = lambda: r.real(ploidy)  # noqa: E731
    lg = lib.rmock_lgl
    scratch = lambda: r.matrix(np.zeros((len(rows), 1)))  # noqa: E731

    def fst_args(first):
        pc = r.int_matrix(pairs) if not double else r.matrix(pairs.astype(float))
        return lambda bl, nd: (pc, r.matrix(S["n"]), *first(), lg(bl), lg(nd))

    def acc(name):
        f = os.path.join(tmp, f"acc_{name}_{np.random.randint(1 << 30)}.bk")
        np.zeros(len(rows) ** 2).tofile(f)
        return r.fbm(f, len(rows), len(rows))

    return {
        "alt_freq_dip_pseudo_cpp": (lambda: (BM, ix(rows), ix(cols), pl(), r.int([1]), lg(0)), ("matrix", (m, 2), 14)),
        "grouped_alt_freq_dip_pseudo_cpp": (lambda: (BM, ix(rows), ix(cols), gids(), ng(), pl(), r.int([1]), lg(1)),
                                            ("matrix", (m, 2 * G), 14)),
        "grouped_missingness_cpp": (lambda: (BM, ix(rows), ix(cols), gids(), ng(), r.int([1])), ("matrix", (m, G), 14)),
        "grouped_summaries_dip_pseudo_cpp": (lambda: (BM, ix(rows), ix(cols), gids(), ng(), pl(), r.int([1])),
                                             ("list", ["freq_alt", "freq_ref", "n", "het_obs"], (m, G))),
        "gt_ind_hetero": (lambda: (BM, ix(rows), ix(cols), r.int([1])), ("matrix", (2, len(rows)), 13)),
        "gt_pi_diploid": (lambda: (BM, ix(rows), ix(cols), r.int([1])), ("vector", m, 14)),
        "gt_grouped_pi_diploid": (lambda: (BM, ix(rows), ix(cols), gids(), ng(), r.int([1])), ("list", ["pi", "n"], (m, G))),
        "pairwise_fst_hudson_loop": (lambda: fst_args(lambda: (r.matrix(S["fa"]), r.matrix(S["fr"])))(1, 0),
                                     ("list", ["fst_locus", "fst_tot"], None)),
        "pairwise_fst_wc84_loop": (lambda: fst_args(lambda: (r.matrix(S["fa"]), r.matrix(S["het"])))(1, 1),
                                   ("list", ["Fst_by_locus_num", "Fst_by_locus_den"], (m, 3))),
        "pairwise_fst_nei87_loop": (lambda: fst_args(lambda: (r.matrix(S["het"]), r.matrix(S["fa"]), r.matrix(S["fr"])))(0, 0),
                                    ("list", ["fst_locus", "fst_tot"], None)),
        "fbm256_prod_and_rowSumsSq": (lambda: (BM, ix(rows), ix(cols), r.real(np.full(m, 0.9)), r.real(np.full(m, 0.7)),
                                               r.matrix(V)), ("pca", None, None)),
        "increment_ibs_counts": (lambda: (acc("k"), acc("k2"), scratch(), scratch(), scratch(), BM, ix(rows), ix(cols)),
                                 ("nil", None, None)),
        "increment_king_numerator": (lambda: (acc("k"), acc("k2"), scratch(), scratch(), scratch(), scratch(), BM, ix(rows),
                                              ix(cols)), ("nil", None, None)),
        "increment_as_counts": (lambda: (acc("k"), acc("k2"), scratch(), scratch(), BM, ix(rows), ix(cols)), ("nil", None, None)),
    }


def check(name, out, want):
    kind, a, b = want
    if kind == "nil":
        assert lib.TYPEOF(out) == 0, name
    elif kind == "matrix":
        assert lib.TYPEOF(out) == b and r.dim(out) == a, (name, lib.TYPEOF(out), r.dim(out))
    elif kind == "vector":
        assert lib.TYPEOF(out) == b and lib.XLENGTH(out) == a and r.dim(out) is None, name
    elif kind == "pca":
        assert lib.TYPEOF(out) == 19 and lib.XLENGTH(out) == 2 and r.names(out) is None, name
        assert r.dim(lib.VECTOR_ELT(out, 0)) == (len(rows), 3) and lib.XLENGTH(lib.VECTOR_ELT(out, 1)) == len(rows), name
    else:
        assert lib.TYPEOF(out) == 19 and r.names(out) == a, (name, r.names(out))
        if b is not None:
            for k in range(len(a)):
                assert lib.TYPEOF(lib.VECTOR_ELT(out, k)) == 14 and r.dim(lib.VECTOR_ELT(out, k)) == b, (name, k)


def value(out):
    t = lib.TYPEOF(out)
    if t == 19:
        return [value(lib.VECTOR_ELT(out, k)) for k in range(lib.XLENGTH(out))]
    return None if t == 0 else r.as_numpy(out).tobytes()


lib.rmock_gctorture(1)
lib.rmock_strict(1)
failures = []
for double in (False, True):
    for name, (args, want) in entry_calls(double).items():
        depth = r.depth()
        try:
            out = r.call(name, *args())
        except RuntimeError as e:
            failures.append(f"{name} ({'double' if double else 'integer'} indices): {e}")
            continue
        assert r.depth() == depth
        check(name, out, want)
        if double:  # the same call with integer indices gives the same bytes
            ref = r.call(name, *entry_calls(False)[name][0]())
            assert value(out) == value(ref), name
assert not failures, "\n".join(failures)
assert counter("g_stub_view_alive") == 0

for name, (args, want) in entry_calls(True).items():
    for k in range(1, 100):
        a = args()
        alive = counter("g_stub_fbm_alive")
        depth = r.depth()
        lib.rmock_fail_alloc_at(k)
        try:
            out = r.call(name, *a)
        except RuntimeError as e:
            assert str(e).startswith("cannot allocate vector"), (name, k, str(e))
            assert counter("g_stub_view_alive") == 0, f"{name}: a device view leaked when allocation {k} failed"
            assert counter("g_stub_fbm_alive") == alive, f"{name}: an uploaded FBM leaked when allocation {k} failed"
            assert r.depth() == depth, (name, k)
            continue
        check(name, out, want)
        break
    else:
        raise SystemExit(f"{name}: never went through")
lib.rmock_fail_alloc_at(0)
lib.rmock_gctorture(0)
lib.rmock_strict(0)
r.call("tpg_release")

lib.R_unload_tpgshim(None)
lib.rmock_reset()
print("ok shim under sanitizers")
