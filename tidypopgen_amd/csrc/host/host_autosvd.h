// host_autosvd.h -- the scalar pieces of include/tpg.h "autoSVD" that live on the host, or that host and device share: the
// upper normal quantile by bisection, the Gaussian weights of the rolling mean, the closed-form tie terms of the medcouple
// count, g(r), the Tukey fence from the sorted statistics, and the finder of consecutive outlier runs.
// Plain C++ with no HIP in it, so that tests/host/autosvd_san.cpp can build it with -fsanitize=address,undefined.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__HIPCC__)
#define TPG_AUTOSVD_HD __host__ __device__
#else
#define TPG_AUTOSVD_HD
#endif

#define TPG_AUTOSVD_BITS_ONE 0x3FF0000000000000ull  // the bit pattern of 1.0
#define TPG_AUTOSVD_BITS_INF 0x7FF0000000000000ull  // ... of +inf: patterns of non-negative doubles order as integers

// the upper tail of the standard normal: 0.5 erfc(x / sqrt(2)), sqrt(2) as the double 1.4142135623730951
static inline double host_pnorm_upper(double x) { return 0.5 * erfc(x / 1.4142135623730951); }

// the root x of host_pnorm_upper(x) = p, 0 < p < 1, by bisection on [-40, 40] until the two ends are neighbouring doubles; the
// upper end is returned (the tail there is <= p)
static inline double host_qnorm_upper(double p) {
  double lo = -40.0, hi = 40.0;
  for (;;) {
    const double mid = lo + (hi - lo) / 2;
    if (!(mid > lo && mid < hi)) break;
    if (host_pnorm_upper(mid) > p) lo = mid;
    else hi = mid;
  }
  return hi;
}

// w[2 radius + 1]: the normal density at len equally spaced points between the -L and L of include/tpg.h "autoSVD" step 4;
// radius 0: the single weight 1
static inline void host_rollmean_weights(int radius, double* w) {
  const int len = 2 * radius + 1;
  if (radius == 0) {
    w[0] = 1.0;
    return;
  }
  const double a = len <= 10 ? 3.0 / 8.0 : 0.5;
  const double p1 = (1.0 - a) / ((double)len + 1.0 - 2.0 * a);
  const double L = host_qnorm_upper(p1);
  const double step = (2.0 * L) / (double)(len - 1);
  for (int i = 0; i < len; i++) {
    const double t = -L + (double)i * step;
    w[i] = exp(-(t * t) / 2.0) / 2.5066282746310002;  // sqrt(2 pi) as a double
  }
}

// Medcouple, the ratios that are not a division: with k values equal to the median and nB = |B| (the k zeros included), how
// many of the k (nB - k) + k k tie ratios are <= the ratio whose bit pattern is `cand`:
//   k (k - 1) / 2 zeros always, k ones from 1.0 on, k (k - 1) / 2 + k (nB - k) times +inf from +inf on
TPG_AUTOSVD_HD static inline uint64_t tpg_mc_tie_count(uint64_t k, uint64_t nB, uint64_t cand) {
  const uint64_t half = k * (k - (k ? 1 : 0)) / 2;
  uint64_t c = half;
  if (cand >= TPG_AUTOSVD_BITS_ONE) c += k;
  if (cand >= TPG_AUTOSVD_BITS_INF) c += half + k * (nB - k);
  return c;
}

// g(r) = (1 - r) / (1 + r), g(+inf) = -1: the medcouple kernel value h = (a - b) / (a + b) of the ratio r = b / a
static inline double host_mc_g(double r) { return r > 1.79769313486231570815e308 ? -1.0 : (1.0 - r) / (1.0 + r); }

static inline double host_mc_from_ratio_bits(uint64_t lo_bits, uint64_t hi_bits) {
  double lo, hi;
  memcpy(&lo, &lo_bits, sizeof lo);
  memcpy(&hi, &hi_bits, sizeof hi);
  return (host_mc_g(lo) + host_mc_g(hi)) / 2;
}

// coef and thr of step 5 from c, the quartiles and the medcouple, in the order the header states
static inline void host_tukey_fence(double c, double q1, double q3, double mc, double alpha, double* coef, double* thr) {
  const double z75 = host_qnorm_upper(0.25);
  *coef = (host_qnorm_upper(alpha / c) - z75) / (2.0 * z75);
  const double e = mc >= 0.0 ? exp(3.0 * mc) : exp(4.0 * mc);
  *thr = q3 + *coef * (q3 - q1) * e;
}

// Runs of outliers: pos[count] ascending positions in one iteration's kept list, chrom_of[count] the chromosome of each.  A
// run is a maximal stretch of consecutive positions on one chromosome; those of at least min_size entries are reported as
// (index of the first entry, index of the last) into pos.
static inline void host_outlier_runs(const int64_t* pos, const int32_t* chrom_of, int64_t count, int64_t min_size,
                                     std::vector<int64_t>& first, std::vector<int64_t>& last) {
  first.clear();
  last.clear();
  int64_t a = 0;
  for (int64_t i = 1; i <= count; i++) {
    if (i < count && pos[i] == pos[i - 1] + 1 && chrom_of[i] == chrom_of[i - 1]) continue;
    if (i - a >= min_size) {
      first.push_back(a);
      last.push_back(i - 1);
    }
    a = i;
  }
}
