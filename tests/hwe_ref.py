"""The Hardy-Weinberg exact test in exact arithmetic: the reference of tests/test_hwe_host.py, tests/test_gpu_hwe.py and
tests/test_gpu_rshim_hwe.py.  Written from the definition (Wigginton, Cutler, Abecasis 2005; mid-p: Graffelman, Moreno
2013), Python integers and fractions.Fraction throughout, nothing rounded before the last conversion to a double.

A table (hom1, het, hom2) of n individuals has r = 2 min(hom1, hom2) + het copies of the rarer allele.  Given r and n the
number of heterozygotes x runs over r mod 2, r mod 2 + 2, ..., r and the number of samples with x heterozygotes is

    W(x) = n! 2^x / (((r - x) / 2)! x! ((2 n - r - x) / 2)!)           (an integer; P(x) = W(x) / sum W)

eps = 2^-44: T = {x : W(x) < W(het) (1 + eps)}, ties = |{x in T : W(x) > W(het) (1 - eps)}|,
p = sum_T W / sum W, p_mid = (sum_T W - ties W(het) / 2) / sum W."""
from collections import namedtuple
from fractions import Fraction
from math import comb

EPS_BITS = 44
Result = namedtuple("Result", "p p_mid ties nearest")


def weights(hom1: int, het: int, hom2: int):
    """{x: W(x)} for every possible heterozygote count of the table's margins"""
    n = hom1 + het + hom2
    r = 2 * min(hom1, hom2) + het
    x = r % 2
    a, b = (r - x) // 2, (2 * n - r - x) // 2
    w = comb(n, a) * comb(n - a, x) * 2 ** x  # n! / (a! x! b!) * 2^x
    out = {}
    while True:
        out[x] = w
        if x + 2 > r:
            return out
        num, den = 4 * a * b, (x + 2) * (x + 1)
        assert (w * num) % den == 0
        w = w * num // den
        x, a, b = x + 2, a - 1, b - 1


def exact(hom1: int, het: int, hom2: int) -> Result:
    if min(hom1, het, hom2) < 0:
        raise ValueError("negative count")
    W = weights(hom1, het, hom2)
    wh, total = W[het], sum(W.values())
    one = 1 << EPS_BITS
    T = [w for w in W.values() if w * one < wh * (one + 1)]
    ties = sum(1 for w in T if w * one > wh * (one - 1))
    tail = sum(T)
    others = [abs(w - wh) for w in W.values() if w != wh]
    return Result(Fraction(tail, total), Fraction(2 * tail - ties * wh, 2 * total), ties,
                  Fraction(min(others), wh) if others else None)


def p_value(hom1: int, het: int, hom2: int, midp) -> Fraction:
    r = exact(hom1, het, hom2)
    return r.p_mid if midp else r.p


NEAREST_MIN = Fraction(1, 1 << 30)  # a case is compared only if no other count is almost, but not exactly, as likely


def comparable(res: Result) -> bool:
    return res.nearest is None or res.nearest >= NEAREST_MIN


def tolerance(n: int) -> float:
    """relative bound of an FP64 recurrence from the observed count against the exact value: every step two roundings, at
    most n / 2 + 1 steps, one rounding per term in each running sum, the quotient, the mid-p subtraction at most doubling
    it: <= ~3.5 n units of 2^-53, rounded up to 8 max(n, 8)"""
    return 8.0 * max(n, 8) * 2.0 ** -53


def close(got: float, want: Fraction, n: int) -> bool:
    """the comparison every test makes: relative `tolerance(n)`, absolute 1e-300 where the exact value is below that"""
    if want < Fraction(1, 10 ** 300):
        return 0.0 <= got <= 1e-300
    return abs(Fraction(got) - want) <= Fraction(tolerance(n)) * want


def all_tables(nmax: int):
    """every (hom1, het, hom2) with hom1 + het + hom2 <= nmax, n = 0 and both orders of the homozygotes included"""
    return [(a, h, n - a - h) for n in range(nmax + 1) for a in range(n + 1) for h in range(n - a + 1)]


def read_plink_hwe(path):
    """rows of a PLINK .hwe file: (snp, (hom1, het, hom2), p)"""
    out = []
    with open(path) as f:
        head = f.readline().split()
        for line in f:
            rec = dict(zip(head, line.split()))
            a, h, b = (int(v) for v in rec["GENO"].split("/"))
            out.append((rec["SNP"], (a, h, b), float(rec["P"])))
    return out
