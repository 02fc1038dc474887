"""Host side of Tajima's D: the numpy restatement tests/tajima_ref.py against itself (float route = exact route), the closed
forms of the constants, tpg_tajimas_d_from_sums (host arithmetic in the library: loading it needs no GPU), the declarations in
the header and the binding, and the R shim's registration.  No GPU."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import rmock
from tests import tajima_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("tpg_tajimas_d_from_sums", "tpg_pop_tajimas_d", "tpg_windows_pop_tajimas_d")


def test_closed_forms_of_the_constants():
    assert tr.consts(2) == (1.0, 1.0, 0.0, 0.0)  # n = 2: e1 = e2 = 0 exactly, so vd = 0
    a1, a2, e1, e2 = tr.consts(4)
    assert a1 == 1.0 + 0.5 + 1.0 / 3.0 and abs(Fraction(a1) - Fraction(11, 6)) <= Fraction(1, 2 ** 52)
    assert abs(Fraction(a2) - Fraction(49, 36)) <= Fraction(1, 2 ** 52)
    for n in (4, 20):
        a1, a2, e1, e2 = tr.consts(n)
        A1, A2 = tr.a1_exact(n), sum((Fraction(1, i * i) for i in range(1, n)), Fraction(0))
        E1 = (Fraction(n + 1, 3 * (n - 1)) - 1 / A1) / A1
        E2 = (Fraction(2 * (n * n + n + 3), 9 * n * (n - 1)) - Fraction(n + 2, n) / A1 + A2 / A1 ** 2) / (A1 ** 2 + A2)
        # e1 and e2 are differences of terms of size <= 1: a few roundings of 2^-53 each
        assert abs(Fraction(a1) - A1) <= 2 * n * Fraction(1, 2 ** 53) and abs(Fraction(a2) - A2) <= 2 * n * Fraction(1, 2 ** 53)
        assert abs(Fraction(e1) - E1) <= 4 * n * Fraction(1, 2 ** 53) and abs(Fraction(e2) - E2) <= 4 * n * Fraction(1, 2 ** 53)


@pytest.mark.parametrize("n,G", [(13, 1), (13, 3), (13, 33), (65, 33)])
def test_float_route_equals_exact_route_on_the_planted_panel(n, G):
    m = 300
    codes, gid = tr.panel(5, n, m, G)
    x, v = tr.group_counts(codes, gid, G)
    size = tr.group_sizes(n, gid, G)
    pi = tr.pi_float(x, v)
    # the planted columns are there
    assert np.isnan(pi[m // 3, 0]) and (v[m // 3, 0] == 0)
    last = 0 if gid is None else int(gid.max())
    if G > 1:
        assert size[last] == 1 and pi[m // 2, last] == 1.0
        assert (size == 0).any() == (G > n)
    assert np.all(pi[m // 4:m // 4 + 70][~np.isnan(pi[m // 4:m // 4 + 70])] == 0.0)
    assert 0.05 < np.mean(codes == tr.MISSING) < 0.15
    # windows of 65 loci, the whole panel, the planted heterozygote alone (k_hat = 1, S = 0: +Inf), the monomorphic stretch
    lo = np.r_[np.arange(0, m - 64, 7), 0, m // 2, m // 4]
    hi = np.r_[np.arange(0, m - 64, 7) + 65, m, m // 2 + 1, m // 4 + 64]
    ref = tr.windows_ref(codes, gid, G, lo, hi)
    assert np.isnan(ref["tajimas_d"][-1]).all() and (ref["seg"][-1] == 0).all()  # S = 0 and k_hat = 0: 0 / 0
    kinds = set()
    for g in range(G):
        n_all = 2 * int(size[g])
        for w in range(len(lo)):
            L = int(hi[w] - lo[w])
            seg, k = tr.sums_exact(x[lo[w]:hi[w], g], v[lo[w]:hi[w], g])
            assert seg == ref["seg"][w, g]
            assert (k is None) == bool(np.isnan(ref["k_hat"][w, g]))
            if k is None:
                assert np.isnan(ref["tajimas_d"][w, g])
                kinds.add("nan")
                continue
            kf = float(ref["k_hat"][w, g])
            assert abs(Fraction(kf) - k) <= L * Fraction(1, 2 ** 52) * k
            num = (Fraction(kf) - Fraction(seg) / Fraction(tr.consts(n_all)[0]))
            assert abs(num - tr.numerator_exact(n_all, seg, k)) <= Fraction(1, 2 ** 50) * (L * k + Fraction(seg) / tr.a1_exact(n_all))
            d = ref["tajimas_d"][w, g]
            kinds.add("nan" if np.isnan(d) else "inf" if np.isinf(d) else "finite")
            if n_all == 2:
                assert not np.isfinite(d)  # vd = 0
    assert "nan" in kinds and (G == 1 or "inf" in kinds) and "finite" in kinds


def _from_sums(lib, n, seg, k):
    d = C.c_double()
    rc = lib.tpg_tajimas_d_from_sums(C.c_int64(n), C.c_int64(seg), C.c_double(k), C.byref(d))
    return rc, d.value


def test_from_sums_equals_the_float_route_to_4_ulp():
    from tidypopgen_amd import _lib

    seen = set()
    for n in (2, 4, 6, 20, 10000):
        for seg in (0, 1, 2, 1000):
            for k in (0.0, 0.4, seg / tr.consts(n)[0], 0.37 * seg + 0.125, 250.0, np.nan):
                rc, got = _from_sums(_lib.lib, n, seg, k)
                assert rc == 0
                want = float(tr.d_from_sums(n, seg, k))
                assert tr.max_ulp([got], [want]) <= 4, (n, seg, k, got, want)
                seen.add("nan" if np.isnan(got) else "inf" if np.isinf(got) else "finite")
    assert seen == {"nan", "inf", "finite"}
    assert np.isnan(_from_sums(_lib.lib, 20, 0, 0.0)[1]) and _from_sums(_lib.lib, 20, 0, 1.0)[1] == np.inf  # S = 0
    for n, seg in ((1, 3), (0, 3), (-4, 3), (20, -1)):
        assert _from_sums(_lib.lib, n, seg, 1.0)[0] != 0
    from tidypopgen_amd import api

    assert api.tajimas_d_from_sums(20, 7, 2.5) == float(tr.d_from_sums(20, 7, 2.5))
    with pytest.raises(_lib.TpgError):
        api.tajimas_d_from_sums(1, 7, 2.5)
    assert api.TAJIMA_CHUNK_LOCI > 0


def test_header_and_binding_declare_the_functions():
    from tidypopgen_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "tpg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for f in FUNCTIONS:
        assert re.search(r"\bint " + f + r"\s*\(", code), f
        assert f in _lib.SYMBOLS and hasattr(_lib.lib, f) and getattr(_lib.lib, f).argtypes is not None
    assert "Tajima's D" in hdr
    import tidypopgen_amd as tpg

    for f in ("tajimas_d_from_sums", "pop_tajimas_d", "windows_pop_tajimas_d"):
        assert callable(getattr(tpg, f))


def _table(lib, symbol):
    """a NULL-terminated registration table of the shim, whatever its length: {name: (function pointer, arity)}"""
    row = C.cast(C.addressof(rmock.Entry.in_dll(lib, symbol)), C.POINTER(rmock.Entry))
    out, k = {}, 0
    while row[k].name:
        out[row[k].name.decode()] = (row[k].fun, row[k].numArgs)
        k += 1
    return out


def test_shim_registers_the_two_entries_once(tmp_path):
    for extra in ((), ("-DTPG_RSHIM_STANDALONE",)):
        r = rmock.compile_only(extra)
        assert r.returncode == 0, r.stderr[-4000:]
    lib = rmock.build(tmp_path)  # links against libtpg_hip.so; loading it needs no GPU
    got = _table(lib, "tpg_rshim_entries_tajima")
    assert {k: v[1] for k, v in got.items()} == {"_tidypopgen_tpg_pop_tajimas_d": 5, "_tidypopgen_tpg_windows_pop_tajimas_d": 9}
    for name, (fun, _) in got.items():
        assert fun == C.cast(getattr(lib, name), C.c_void_p).value
    src = open(os.path.join(ROOT, "shim", "tpg_rshim.c")).read()
    tables = set(re.findall(r"const R_CallMethodDef (tpg_rshim_entries\w*)\[\]", src)) - {"tpg_rshim_entries_tajima"}
    assert {"tpg_rshim_entries", "tpg_rshim_entries_roh"} <= tables
    for tab in tables:  # no name shared with any other table
        assert not set(got) & set(_table(lib, tab)), tab
