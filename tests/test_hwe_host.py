"""Hardy-Weinberg exact tests without a GPU: the exact-arithmetic reference (tests/hwe_ref.py) against PLINK's own results
and closed forms, the host restatement of the FP64 recurrence (csrc/host/host_hwe.h, what SNPHWE2_R of the R shim runs and
what the kernels of csrc/hwe.hip run per lane) against that reference on every table of up to 40 individuals, and the
shim's third registration table."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import pytest

from tests import hwe_ref as hr
from tests import rmock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "related")
HOST = os.path.join(ROOT, "tidypopgen_amd", "csrc", "host")


@pytest.mark.parametrize("name,midp", [("families_hwe.hwe", False), ("families_hwe_midp.hwe", True)])
def test_reference_against_plink(name, midp):
    rows = hr.read_plink_hwe(os.path.join(GOLDEN, name))
    assert len(rows) == 10
    for snp, (a, h, b), p in rows:
        assert abs(float(hr.p_value(a, h, b, midp)) - p) <= 5e-5, (name, snp, (a, h, b))


def test_reference_closed_forms():
    assert hr.exact(0, 0, 0)[:3] == (1, Fraction(1, 2), 1)
    for n in (1, 7, 40):  # monomorphic
        assert hr.exact(n, 0, 0)[:3] == (1, Fraction(1, 2), 1)
        assert hr.exact(0, 0, n)[:3] == (1, Fraction(1, 2), 1)
    r = hr.exact(0, 4, 2)  # 2 and 4 heterozygotes are equally likely
    assert (r.p, r.p_mid, r.ties) == (1, Fraction(17, 33), 2)
    assert hr.exact(1, 0, 1)[:2] == (Fraction(1, 3), Fraction(1, 6))  # {0: 1, 2: 2} ways
    for a, h, b in ((3, 5, 11), (0, 9, 4), (20, 1, 19)):
        assert hr.exact(a, h, b) == hr.exact(b, h, a)
    with pytest.raises(ValueError):
        hr.exact(1, -1, 1)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("hwe_host")
    src = d / "drive.c"
    src.write_text('#include <stdio.h>\n#include "host_hwe.h"\n'
                   "int main(void) {\n  long a, h, b;\n  int midp;\n"
                   '  while (scanf("%ld %ld %ld %d", &a, &h, &b, &midp) == 4) printf("%a\\n", tpg_hwe_exact(a, h, b, midp));\n'
                   "  return 0;\n}\n")
    exe = str(d / "drive")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + HOST, str(src), "-o", exe])

    def run(cases):
        out = subprocess.run([exe], input="".join("%d %d %d %d\n" % c for c in cases), capture_output=True, text=True,
                             check=True).stdout.split()
        assert len(out) == len(cases)
        return [float.fromhex(v) for v in out]

    return run


def test_host_recurrence_on_every_small_table(driver):
    tabs = hr.all_tables(40)
    assert len(tabs) == 12341  # sum over n <= 40 of (n + 1)(n + 2) / 2
    cases = [(a, h, b, midp) for a, h, b in tabs for midp in (0, 1)]
    got = driver(cases)
    left_out = 0
    for k, (a, h, b) in enumerate(tabs):
        r = hr.exact(a, h, b)
        if not hr.comparable(r):
            left_out += 1
            continue
        assert hr.close(got[2 * k], r.p, a + h + b), (a, h, b, got[2 * k], float(r.p))
        assert hr.close(got[2 * k + 1], r.p_mid, a + h + b), (a, h, b, got[2 * k + 1], float(r.p_mid))
    assert left_out == 0


def test_host_recurrence_large_tables(driver):
    # n = 5 000 in the bulk and in both tails; n = 40 000 with too many and too few heterozygotes (int64 products; p < 1e-300)
    tabs = [(1200, 2500, 1300), (2000, 1000, 2000), (100, 4800, 100), (4990, 10, 0), (0, 3, 4997),
            (7000, 26000, 7000), (13000, 14000, 13000), (9000, 22000, 9000), (10000, 20000, 10000), (39990, 10, 0)]
    got = driver([(a, h, b, midp) for a, h, b in tabs for midp in (0, 1)])
    for k, (a, h, b) in enumerate(tabs):
        r = hr.exact(a, h, b)
        assert hr.comparable(r), (a, h, b)
        assert hr.close(got[2 * k], r.p, a + h + b), (a, h, b, got[2 * k], float(r.p))
        assert hr.close(got[2 * k + 1], r.p_mid, a + h + b), (a, h, b, got[2 * k + 1], float(r.p_mid))
    for a, h, b in ((7000, 26000, 7000), (13000, 14000, 13000)):
        assert hr.exact(a, h, b).p < Fraction(1, 10 ** 300)


def test_shim_compiles_and_has_the_hwe_table(tmp_path):
    for extra in ((), ("-DTPG_RSHIM_STANDALONE",)):
        r = rmock.compile_only(extra)
        assert r.returncode == 0, r.stderr[-4000:]
    lib = rmock.build(tmp_path)  # links against libtpg_hip.so; loading it needs no GPU
    tab = (rmock.Entry * 8).in_dll(lib, "tpg_rshim_entries_hwe")
    got = {}
    for e in tab:
        if not e.name:
            break
        got[e.name.decode()] = (e.fun, e.numArgs)
    assert {k: v[1] for k, v in got.items()} == {"_tidypopgen_SNPHWE2_R": 4, "_tidypopgen_hwe_on_matrix": 2,
                                                 "_tidypopgen_gt_grouped_hwe": 6, "_tidypopgen_tpg_loci_hwe": 4}
    for name, (fun, _) in got.items():
        assert fun == C.cast(getattr(lib, name), C.c_void_p).value, name
    assert not set(got) & set(rmock.entries(lib))  # the main table is as it was: a name is registered once
    # one table through the shim's host path (no device): the heterozygotes come first
    lib.rmock_strict(1)
    try:
        s = rmock.Session(lib)
        s.ent = {**s.ent, **got}
        depth = lib.rmock_protect_depth()
        for het, hom1, hom2, midp in ((4, 0, 2, 1), (4, 0, 2, 0), (0, 0, 0, 1), (25, 10, 12, 1)):
            p = s.as_numpy(s.call("SNPHWE2_R", s.int([het]), s.int([hom1]), s.int([hom2]), lib.rmock_lgl(midp)))
            assert p.shape == (1,) and hr.close(float(p[0]), hr.p_value(hom1, het, hom2, midp), het + hom1 + hom2)
        assert lib.rmock_protect_depth() == depth
        with pytest.raises(RuntimeError, match="non-negative"):
            s.call("SNPHWE2_R", s.int([-1]), s.int([1]), s.int([1]), lib.rmock_lgl(1))
    finally:
        lib.rmock_strict(0)
        lib.rmock_reset()
