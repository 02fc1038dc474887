"""CPU: include/tpg.h "least-squares projection" restated in numpy (tests/lsq_ref.py) against its exact route within the bounds
derived there; the teeth of those bounds; the singular rule at its thresholds; and the routine the kernel runs
(csrc/host/host_lsq.h) as a stand-alone program under the host sanitizers, bit for bit against the Python restatement."""
import shutil

import numpy as np
import pytest

from tests import lsq_ref as lref

# (seed, n, m, L, typed fraction): m from 33 to 700, L from 2 to 32, typed fractions from 1.0 down to 0.02; the sparse fractions go
# with few components, so that t_i >= L for most rows (a row with t_i < L is singular by the rule and is checked as such)
GRID = [(1, 6, 33, 2, 1.0), (2, 4, 33, 32, 1.0), (3, 6, 33, 2, 0.5), (4, 6, 100, 10, 0.5), (5, 6, 129, 17, 0.5),
        (6, 6, 200, 10, 0.3), (7, 4, 700, 20, 0.3), (8, 6, 700, 3, 0.05), (9, 6, 700, 2, 0.02), (10, 3, 300, 32, 1.0),
        (11, 3, 700, 32, 0.5), (12, 6, 128, 16, 0.3), (13, 6, 400, 5, 0.05),
        # few typed loci per component: the ill-conditioned rows
        (14, 8, 700, 10, 0.03), (15, 8, 700, 20, 0.05), (16, 8, 400, 10, 0.05), (17, 8, 100, 16, 0.3)]

_cache = {}


def _case(spec):
    """a grid case with its float64 sums, its exact route and the per-row numbers, computed once"""
    if spec not in _cache:
        seed, n, m, L, frac = spec
        codes, center, scale, V = lref.grid_case(seed, n, m, L, frac)
        Af, bf, nt = lref.normal_float(codes, center, scale, V)
        ex = lref.normal_exact(codes, center, scale, V)
        bA, bb = lref.bound_A(ex), lref.bound_b(ex)
        xf, sing = lref.solve_restated(Af, bf, nt)
        rows = {}
        for i in range(n):
            if np.isnan(xf[i]).any():
                continue
            xe = lref.solve_exact_row(lref.unpack(ex["A"][i], L), ex["b"][i])
            rows[i] = (xe, lref.row_numbers(ex["A"][i], ex["b"][i], bA[i], bb[i], L))
        _cache[spec] = dict(L=L, n=n, Af=Af, bf=bf, nt=nt, ex=ex, bA=bA, bb=bb, xf=xf, sing=sing, rows=rows)
    return _cache[spec]


def test_restatement_agrees_with_the_exact_route_within_the_bounds():
    worst = dict(A=0.0, b=0.0, solve=0.0, chain=0.0, kappa=0.0)
    left_out = 0
    for spec in GRID:
        c = _case(spec)
        L, ex = c["L"], c["ex"]
        assert np.array_equal(c["nt"], ex["n_typed"])
        typed = c["nt"] > 0
        rA = np.abs(c["Af"].astype(lref.LD) - ex["A"]).astype(np.float64)[typed] / c["bA"][typed]
        rb = np.abs(c["bf"].astype(lref.LD) - ex["b"]).astype(np.float64)[typed] / np.maximum(c["bb"][typed], 1e-300)
        worst["A"], worst["b"] = max(worst["A"], rA.max()), max(worst["b"], rb.max())
        assert rA.max() <= lref.REF_SLACK and rb.max() <= lref.REF_SLACK, (spec, rA.max(), rb.max())
        # the rule and the count agree: the singular rows are exactly the rows with t < L on this grid
        assert c["sing"] == int((c["nt"] < L).sum()) and sorted(c["rows"]) == [i for i in range(c["n"]) if c["nt"][i] >= L]
        for i, (xe, (kap, eA, eb, ec)) in c["rows"].items():
            if not lref.held(kap, eA, ec):
                left_out += 1
                continue
            xn = float(np.linalg.norm(xe.astype(np.float64)))
            err = float(np.linalg.norm((c["xf"][i].astype(lref.LD) - xe).astype(np.float64)))
            worst["chain"] = max(worst["chain"], err / lref.chain_bound(kap, eA, eb, ec, xn))
            worst["kappa"] = max(worst["kappa"], kap)
            assert err <= lref.REF_SLACK * lref.chain_bound(kap, eA, eb, ec, xn), (spec, i, err, kap)
            # the solve alone: from the float64 (A, b), against the exact solve of those very numbers
            xs = lref.solve_exact_row(lref.unpack(c["Af"][i], L), c["bf"][i])
            errs = float(np.linalg.norm((c["xf"][i].astype(lref.LD) - xs).astype(np.float64)))
            xsn = float(np.linalg.norm(xs.astype(np.float64)))
            worst["solve"] = max(worst["solve"], errs / lref.solve_bound(kap, ec, xsn))
            assert errs <= lref.REF_SLACK * lref.solve_bound(kap, ec, xsn), (spec, i, errs, kap)
    print("largest ratios to the bounds:", worst)
    assert left_out == 0


def test_teeth_single_precision_and_a_perturbed_entry():
    seen = 0
    for spec in GRID:
        c = _case(spec)
        L = c["L"]
        x32, _ = lref.solve_restated(c["Af"], c["bf"], c["nt"], cast=np.float32)
        for i, (xe, (kap, eA, eb, ec)) in c["rows"].items():
            if kap <= 10.0:
                continue
            seen += 1
            xn = float(np.linalg.norm(xe.astype(np.float64)))
            err = float(np.linalg.norm((x32[i].astype(lref.LD) - xe).astype(np.float64)))
            print(f"{spec} row {i}: kappa {kap:.3g}, single precision at {err / lref.chain_bound(kap, eA, eb, ec, xn):.3g} of the chain bound")
            assert not err <= lref.chain_bound(kap, eA, eb, ec, xn), (spec, i, err, kap)
        # a relative perturbation of 1e-9 in one (diagonal) entry of A_packed leaves the A bound
        i = next(iter(c["rows"]))
        p = lref.pidx(L, L - 1, L - 1)
        pert = c["Af"][i, p] * (1.0 + 1e-9)
        assert abs(float(lref.LD(pert) - c["ex"]["A"][i, p])) > c["bA"][i, p]
    assert seen >= 20


def _codes_with_typed(m, typed):
    row = np.full(m, 3, dtype=np.uint8)
    row[list(typed)] = 1
    return row


def _singular_cases():
    """(name, A_packed rows, b rows, n_typed, expected singular flags): each threshold with the row just above it"""
    out = []
    # t = L - 1 and t = L on generic loadings; t = 0 (and t = 1 for one component)
    for L in (1, 3, 10):
        codes, center, scale, V = lref.grid_case(50 + L, 1, 64, L, 1.0)
        rows = np.stack([_codes_with_typed(64, range(L - 1)), _codes_with_typed(64, range(L)), _codes_with_typed(64, [])])
        A, b, nt = lref.normal_float(rows, center, scale, V)
        out.append((f"typed counts, L = {L}", A, b, nt, [True, False, True]))
    # two identical loading columns, in numbers that make every pivot exact: pivots 1, 1, 0; beside it an orthogonal third column
    h = 0.5
    Vd = np.array([[h, h, h], [h, -h, -h], [h, h, h], [h, -h, -h]])
    Vo = np.array([[h, h, h], [h, -h, -h], [h, h, -h], [h, -h, h]])
    full = np.ones((1, 4), dtype=np.uint8)
    for name, VV, flag in (("identical columns", Vd, True), ("orthogonal columns", Vo, False)):
        A, b, nt = lref.normal_float(full, np.zeros(4), np.ones(4), np.asfortranarray(VV))
        out.append((name, A, b, nt, [flag]))
    # t = L = 2 with a rank-deficient selection: typed rows (2, 3), (0, 0) -> pivots 4, 0; (2, 3), (0, 1) -> pivots 4, 1
    for name, VV, flag in (("rank-deficient selection", [[2.0, 3.0], [0.0, 0.0], [5.0, 1.0]], True),
                           ("full-rank selection", [[2.0, 3.0], [0.0, 1.0], [5.0, 1.0]], False)):
        A, b, nt = lref.normal_float(np.array([[1, 1, 3]], dtype=np.uint8), np.zeros(3), np.ones(3), np.asfortranarray(VV))
        assert nt[0] == 2
        out.append((name, A, b, nt, [flag]))
    # the pivot threshold itself, L = 2, A = [[1, c], [c, 1]]: c = 1 - 2^-52 gives the pivot 2^-51 = L 2^-52 A[1,1] exactly (not
    # above it: singular), c = 1 - 2^-51 the pivot 2^-50
    for c, flag in ((1.0 - 2.0 ** -52, True), (1.0 - 2.0 ** -51, False)):
        out.append((f"pivot threshold, c = 1 - {1.0 - c:g}", np.array([[1.0, c, 1.0]]), np.array([[1.0, 0.5]]), np.array([5]), [flag]))
    return out


def test_singular_rule_at_its_thresholds():
    for name, A, b, nt, flags in _singular_cases():
        x, sing = lref.solve_restated(A, b, nt)
        assert sing == sum(flags), name
        for i, flag in enumerate(flags):
            assert np.isnan(x[i]).all() if flag else np.isfinite(x[i]).all(), (name, i)
    # the exact pivots of the constructed cases
    A, b, nt = next((A, b, nt) for name, A, b, nt, _ in _singular_cases() if name == "full-rank selection")
    assert np.array_equal(A[0], [4.0, 6.0, 10.0])
    assert np.array_equal(b[0], [2.0, 4.0]) and np.array_equal(lref.solve_restated(A, b, nt)[0][0], [-1.0, 1.0])  # every step exact


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_library_routine_stand_alone_under_address_and_undefined_sanitizers(tmp_path):
    exe = lref.build_host_program(str(tmp_path / "lsq_san"), sanitize=True)
    for seed, (L, m, frac) in enumerate([(1, 40, 0.5), (2, 64, 0.5), (3, 33, 0.3), (10, 200, 0.3), (31, 300, 0.5), (32, 300, 0.5)]):
        codes, center, scale, V = lref.grid_case(100 + seed, 5, m, L, frac)
        codes[4, :] = 3  # a fully missing individual inside the batch
        A, b, nt = lref.normal_float(codes, center, scale, V)
        rc, got, sing = lref.run_host_program(exe, tmp_path, A, b, nt)
        want, wsing = lref.solve_restated(A, b, nt)
        assert rc == 0 and sing == wsing >= 1
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), L
    for name, A, b, nt, flags in _singular_cases():
        rc, got, sing = lref.run_host_program(exe, tmp_path, A, b, nt)
        want, _ = lref.solve_restated(A, b, nt)
        assert rc == 0 and sing == sum(flags), name
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
    # the argument checks
    A, b, nt = np.ones((2, 3)), np.ones((2, 2)), np.array([4, 4])
    assert lref.run_host_program(exe, tmp_path, A, b, nt, L=0)[0] == 2
    assert lref.run_host_program(exe, tmp_path, A, b, nt, L=33)[0] == 2
    bad = A.copy()
    bad[1, 2] = np.nan
    assert lref.run_host_program(exe, tmp_path, bad, b, nt)[0] == 1
    bad = b.copy()
    bad[0, 1] = np.inf
    assert lref.run_host_program(exe, tmp_path, A, bad, nt)[0] == 1
    assert lref.run_host_program(exe, tmp_path, np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0, dtype=np.int64))[0] == 0
