"""GPU: tpg_sym_eig_topk (csrc/pca.hip: eig_topk, eig_topk_any) on matrices with a prescribed spectrum and known eigenvectors
(tests/eig_ref.py, pinned to LAPACK by tests/test_eig_host.py).

The rest of the suite only hands the solver Gram matrices of population panels, where a handful of large eigenvalues
dominate whatever an edge lane reads.  Here every eigenvector is dense, the spectra are chosen (geometric, linear, spikes
over a flat bulk, a triple and a 1e-10 cluster, rank below the block, identity, zero), and the sizes walk the edges of the
kernels: n = 0, 1, 15, 16, 17, 63 (mod 64) for tpg_symm_apply_kernel's clamped last chunk, its `kb + 16 <= n` branch and
its 8-byte-aligned row loads at odd n; n = 0, 1, 15 (mod 16) for tpg_deflate_kernel; 4096 | 4097 for the rows_per_chunk
switch of the small Gram products; k > 52 for the batched route, down to a last batch of one pair; and K scaled by
2^-600 ... 2^600.  Every bound is `eig_ref.check`'s.
"""
import numpy as np
import pytest

from tests import eig_ref as er

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tpg():
    import tidypopgen_amd as t

    t.default_context()
    return t


_built = {}


def _case(name, n):
    """(K, lam, Q) of a named spectrum, built once per module and left unchanged (the two n ~ 4096 matrices are not kept)"""
    key = (name if isinstance(name, str) else name.__name__, n)
    if n > 1000:
        return er.build(name, n)
    if key not in _built:
        K, lam, Q = er.build(name, n)
        for a in (K, lam, Q):
            a.setflags(write=False)
        _built[key] = (K, lam, Q)
    return _built[key]


def _solve(tpg, K, k):
    return tpg.sym_eig_topk(K.T, k)  # (K is symmetric to the bit: its transpose is the column-major array the ABI takes)


def _run(tpg, name, n, k, undetermined=False, rank=None):
    K, lam, Q = _case(name, n)
    lh, U = _solve(tpg, K, k)
    label = f"{name if isinstance(name, str) else name.__name__}/{n}/{k}"
    er.check(K, lam, Q, lh, U, k, subspace_undetermined=undetermined, label=label)
    if rank is not None and k > rank:
        past = float(np.abs(lh[rank:]).max() / lam[0])
        assert past <= 1e-9, (label, past)
    return lh, U


EDGE_N = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193, 255, 257, 1000]
EDGE = [(n, k) for n in EDGE_N for k in (1, 2, 10, 26, 52) if k <= n] + [(4096, 10), (4097, 10), (53, 52), (66, 26), (70, 52)]


@pytest.mark.parametrize("n,k", EDGE)
def test_edge_shapes(tpg, n, k):
    """geometric spectrum 0.9^j: every pair is separated from the next by a tenth of itself, so a wrong element read by one
    lane of the last chunk shows in the residual instead of vanishing under a dominant direction"""
    _run(tpg, "geo", n, k)


SPECTRA = [("spikes", 3, False, None), ("spikes", 10, False, None), ("triple", 8, False, None), ("cluster", 8, False, None),
           ("identity", 5, True, None), ("zero", 3, True, None), (er.rank(5), 5, False, 5), (er.rank(5), 10, True, 5),
           (er.rank(20), 10, False, 20)]
SPECTRA_CASES = [(300,) + s for s in SPECTRA] + [(193,) + s for s in SPECTRA if s[0] in ("spikes", "triple", "cluster")]


@pytest.mark.parametrize("n,name,k,undetermined,rank", SPECTRA_CASES,
                         ids=lambda v: getattr(v, "__name__", None) or str(v))
def test_spectra(tpg, n, name, k, undetermined, rank):
    """wanted pairs next to a flat bulk, repeated and clustered eigenvalues inside the wanted set (the subspace is what is
    defined, and what is compared), and matrices whose rank is below k or below the block of 2 k + 12 vectors"""
    _run(tpg, name, n, k, undetermined, rank)


@pytest.mark.parametrize("name,n,k", [("lin", 64, 53), ("lin", 65, 60), ("lin", 100, 79), ("lin", 129, 104), ("lin", 257, 105),
                                      ("lin", 130, 130), ("geo", 100, 79), ("geo", 129, 104)])
def test_batched_route_full_rank(tpg, name, n, k):
    """k > 52: batches of 26 with explicit deflation; 53 and 79 end in a batch of one pair, 130 of 130 takes everything"""
    _run(tpg, name, n, k)


@pytest.mark.parametrize("r", [40, 59])
def test_batched_route_rank_deficient(tpg, r):
    """the rank ends inside the second (40) and the third (59) batch: the pairs past it are zeros, orthonormal to the rest"""
    _run(tpg, er.rank(r), 200, 60, undetermined=True, rank=r)


_scale0 = {}


@pytest.mark.parametrize("p", [0, -600, -300, -40, 40, 300, 600])
def test_scale(tpg, p):
    """2^p K has the eigenvectors of K and 2^p times its eigenvalues, exactly: the contract holds at every p relative to that
    matrix's own lam_1, and the eigenvalues agree with those at p = 0 after scaling back"""
    n, k = 193, 5
    K, lam, Q = _case("geo", n)
    Kp, lamp = np.ldexp(K, p), np.ldexp(lam, p)
    lh, U = _solve(tpg, Kp, k)
    er.check(Kp, lamp, Q, lh, U, k, label=f"geo*2^{p}/{n}/{k}")
    if p == 0:
        _scale0["lam"] = lh
    elif "lam" in _scale0:
        drift = float(np.abs(np.ldexp(lh, -p) - _scale0["lam"]).max() / lam[0])
        assert drift <= 1e-12, (p, drift)
    else:
        lh0, _ = _solve(tpg, K, k)
        assert np.abs(np.ldexp(lh, -p) - lh0).max() <= 1e-12 * lam[0]


def test_block_override(tpg, monkeypatch):
    """TPG_EIG_BLOCK: a block of 14 for two pairs over a flat bulk, where the default would be 16.  This pins the contract
    UNDER the override, not the override itself: a block of 16 meets the same bounds, so the test cannot tell whether the
    switch was honoured."""
    monkeypatch.setenv("TPG_EIG_BLOCK", "14")
    _run(tpg, "spikes", 129, 2)
