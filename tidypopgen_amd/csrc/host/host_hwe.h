/* host_hwe.h -- the Hardy-Weinberg exact test of one genotype table, for host and device code (plain C99 / C++ / HIP).
 *
 * Written from the published definition (Wigginton, Cutler, Abecasis 2005; mid-p: Graffelman, Moreno 2013):
 * a table (hom1, het, hom2) of n individuals carries r = 2 min(hom1, hom2) + het copies of the rarer allele and
 * c = 2 n - r of the other.  Given r and n, the heterozygote count x runs over r mod 2, r mod 2 + 2, ..., r with
 *
 *     w(x + 2) / w(x) = (r - x) (c - x) / ((x + 2) (x + 1))            P(x) = w(x) / sum w
 *
 * With eps = 2^-44 ("equally likely" up to that relative width), T = { x : w(x) < w(het) (1 + eps) } and
 * ties = |{ x in T : w(x) > w(het) (1 - eps) }| (het itself is one of them):
 *
 *     p = sum_T w / sum w                    p_mid = (sum_T w - ties w(het) / 2) / sum w
 *
 * Everything is relative to w(het) = 1: two walks outward from the observed count, each step one exact integer
 * numerator, one exact integer denominator, one division and one multiplication.  Every term lands in the total; a term
 * lands in the tail sum when it is in T.  The weights are unimodal in x, so once a term is too small to move the tail
 * sum (which is at least 1) every later term of that walk is smaller still and the walk ends.  Relative error against
 * the exact value: at most ~3.5 n units of 2^-53 (tests/test_hwe_host.py holds it to 8 max(n, 8)).
 * A total that overflows FP64 means p < 1e-300: 0 is returned.  n = 0 (and any monomorphic table) gives 1, mid-p 0.5.
 * The products of counts are int64 and must stay exact in FP64: n < 2^26 (TPG_HWE_MAX_N). */
#ifndef TPG_HOST_HWE_H
#define TPG_HOST_HWE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define TPG_HWE_FN __host__ __device__ static inline
#else
#define TPG_HWE_FN static inline
#endif

#define TPG_HWE_MAX_N ((int64_t)1 << 26)

/* upper bound of the steps the two walks take together: the number of possible heterozygote counts besides the observed one */
TPG_HWE_FN int64_t tpg_hwe_max_steps(int64_t hom1, int64_t het, int64_t hom2) {
  return (hom1 < hom2 ? hom1 : hom2) + het / 2;
}

TPG_HWE_FN double tpg_hwe_exact(int64_t hom1, int64_t het, int64_t hom2, int midp) {
  const int64_t n = hom1 + het + hom2;
  const int64_t r = 2 * (hom1 < hom2 ? hom1 : hom2) + het;
  const int64_t c = 2 * n - r;
  const double above = 1.0 + 0x1p-44, below = 1.0 - 0x1p-44, finite = 1.7976931348623157e308;
  double total = 1.0, tail = 1.0, w = 1.0;
  int64_t ties = 1;
  for (int64_t x = het; x < r; x += 2) { /* more heterozygotes */
    w *= (double)((r - x) * (c - x)) / (double)((x + 2) * (x + 1));
    if (!(w <= finite)) return 0.0;
    if (tail + w == tail) break;
    total += w;
    if (w < above) {
      tail += w;
      if (w > below) ties++;
    }
  }
  w = 1.0;
  for (int64_t x = het; x >= 2; x -= 2) { /* fewer heterozygotes */
    w *= (double)(x * (x - 1)) / (double)((r - x + 2) * (c - x + 2));
    if (!(w <= finite)) return 0.0;
    if (tail + w == tail) break;
    total += w;
    if (w < above) {
      tail += w;
      if (w > below) ties++;
    }
  }
  if (!(total <= finite)) return 0.0;
  return midp ? (tail - 0.5 * (double)ties) / total : tail / total;
}

#endif
