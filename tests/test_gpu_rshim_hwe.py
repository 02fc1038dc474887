"""GPU: the four Hardy-Weinberg rows of shim/tpg_rshim.c (tpg_rshim_entries_hwe[]) through the strict R mock: results against
the exact-arithmetic reference (tests/hwe_ref.py, tolerance and input condition as in tests/test_gpu_hwe.py), arguments
unmodified (the mock's strict mode checks that), protect stack balanced."""
import numpy as np
import pytest

from tests import hwe_ref as hr
from tests import rmock

pytestmark = pytest.mark.gpu

CODE_012 = np.r_[0.0, 1.0, 2.0, np.full(253, np.nan)]


def _hwe_entries(lib):
    tab = (rmock.Entry * 8).in_dll(lib, "tpg_rshim_entries_hwe")
    out = {}
    for e in tab:
        if not e.name:
            break
        out[e.name.decode()] = (e.fun, e.numArgs)
    return out


@pytest.fixture(scope="module")
def r(tmp_path_factory):
    lib = rmock.build(tmp_path_factory.mktemp("rshim_hwe"))
    lib.rmock_gctorture(1)
    lib.rmock_strict(1)
    s = rmock.Session(lib)
    s.ent = {**s.ent, **_hwe_entries(lib)}
    yield s
    lib.rmock_gctorture(0)
    lib.rmock_strict(0)
    lib.R_unload_tpgshim(None)
    lib.rmock_reset()


def _panel(n, m, seed):
    rng = np.random.default_rng(seed)
    g = rng.binomial(2, rng.random(m)[None, :], size=(n, m)).astype(np.uint8)
    g[rng.random((n, m)) < 0.05] = 3
    g[:, m // 3] = 3
    return np.asfortranarray(g)


def _check(got, tabs, midp):
    assert len(got) == len(tabs)
    left_out = 0
    for p, (a, h, b) in zip(got, tabs):
        res = hr.exact(a, h, b)
        if not hr.comparable(res):
            left_out += 1
            continue
        assert hr.close(float(p), res.p_mid if midp else res.p, a + h + b), (a, h, b, midp, float(p))
    assert left_out <= len(tabs) // 1000


def _tables(codes, gid, G):
    out = []
    for g in range(G):
        sub = codes[gid == g]
        out.extend((int((sub[:, j] == 0).sum()), int((sub[:, j] == 1).sum()), int((sub[:, j] == 2).sum()))
                   for j in range(codes.shape[1]))
    return out


def test_table_rows_and_arities(r):
    ent = _hwe_entries(r.lib)
    assert {k: v[1] for k, v in ent.items()} == {"_tidypopgen_SNPHWE2_R": 4, "_tidypopgen_hwe_on_matrix": 2,
                                                 "_tidypopgen_gt_grouped_hwe": 6, "_tidypopgen_tpg_loci_hwe": 4}
    assert not set(ent) & set(rmock.entries(r.lib))


@pytest.mark.parametrize("midp", [0, 1])
def test_scalar_and_matrix_forms(r, midp):
    depth = r.depth()
    tabs = [t for t in hr.all_tables(12)] + [(120, 300, 80), (0, 0, 0), (2500, 0, 2500)]
    for a, h, b in tabs[::7]:
        p = r.as_numpy(r.call("SNPHWE2_R", r.int([h]), r.int([a]), r.int([b]), r.lib.rmock_lgl(midp)))
        _check(p, [(a, h, b)], midp)
    # a 4-row big_counts matrix (0 / 1 / 2 / NA counts) and a plain 3-row one, integer and double storage
    c4 = np.array([[a, h, b, 5] for a, h, b in tabs], dtype=np.int32).T
    for mat in (r.int_matrix(c4), r.int_matrix(c4[:3]), r.matrix(c4.astype(np.float64))):
        p = r.as_numpy(r.call("hwe_on_matrix", mat, r.lib.rmock_lgl(midp)))
        _check(p, tabs, midp)
    assert r.depth() == depth
    with pytest.raises(RuntimeError, match="negative"):
        r.call("hwe_on_matrix", r.int_matrix(np.array([[1], [-2], [3]], dtype=np.int32)), r.lib.rmock_lgl(midp))
    assert r.depth() == depth


@pytest.mark.parametrize("n,m,G", [(12, 40, 1), (65, 129, 3), (301, 500, 51)])
def test_store_rows(r, tmp_path, n, m, G):
    raw = _panel(n, m, 10 * n + G)
    path = tmp_path / "geno.bk"
    path.write_bytes(raw.tobytes(order="F"))
    BM = r.fbm(path, n, m, CODE_012)
    rng = np.random.default_rng(n)
    rows = np.sort(rng.permutation(n)[: max(2, (3 * n) // 4)]) + 1
    cols = np.arange(3, m - 2)
    gid = rng.integers(0, G, size=len(rows)).astype(np.int32)
    if G > 1:
        gid[gid == 1] = 0  # an empty group
    sub = raw[np.ix_(rows - 1, cols - 1)]
    depth = r.depth()
    for midp in (0, 1):
        p = r.as_numpy(r.call("tpg_loci_hwe", BM, r.int(rows), r.int(cols), r.lib.rmock_lgl(midp)))
        _check(p, _tables(sub, np.zeros(len(rows), dtype=np.int32), 1), midp)
        # index vectors and group ids as doubles, ngroups as a double: what R code passes
        q = r.as_numpy(r.call("gt_grouped_hwe", BM, r.index(rows, double=True), r.index(cols, double=True),
                              r.real(gid.astype(np.float64)), r.real([float(G)]), r.lib.rmock_lgl(midp)), (len(cols), G))
        _check(q.ravel(order="F"), _tables(sub, gid, G), midp)
        if G > 1:
            assert np.all(q[:, 1] == (0.5 if midp else 1.0))
    assert r.depth() == depth
    assert np.array_equal(np.frombuffer(path.read_bytes(), dtype=np.uint8), raw.ravel(order="F"))
    with pytest.raises(RuntimeError, match="Not implemented for a single individual"):
        r.call("tpg_loci_hwe", BM, r.int([1]), r.int(cols), r.lib.rmock_lgl(1))
    with pytest.raises(RuntimeError, match="groupIds"):
        r.call("gt_grouped_hwe", BM, r.int(rows), r.int(cols), r.int(np.full(len(rows), G)), r.int([G]), r.lib.rmock_lgl(1))
    assert r.depth() == depth
