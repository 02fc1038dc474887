// host_pcadapt.h -- the scalar pieces of include/tpg.h "pcadapt" that host and device share, and the host glue of the OGK
// step: log Q(a, x) of the regularised upper incomplete gamma function (series / modified Lentz, one function for both
// sides), the chi-square median by bisection, the K x K matrix R of one OGK iteration from the scales of the sum and
// difference columns, and the map of the final location / scatter back to the coordinates of the input.
// Plain C++ with no HIP in it, so that tests/host/pcadapt_san.cpp can build it with -fsanitize=address,undefined.
#pragma once
#include <math.h>
#include <stddef.h>

#include <vector>

#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wunused-function"  // host_eig.h also holds the Cholesky pieces of the eigen solver
#include "host_eig.h"
#pragma GCC diagnostic pop

#if defined(__HIPCC__)
#define TPG_PCADAPT_HD __host__ __device__
#else
#define TPG_PCADAPT_HD
#endif

#define TPG_PCADAPT_MAD_SCALE 1.4826

// log Q(a, x), a > 0 with lga = lgamma(a) from the host (a = df / 2 is one value per call; device and host then differ by
// their log / exp / log1p alone).  x < a + 1: the series of P, log1p(-P); otherwise the continued fraction by modified Lentz,
// -x + a ln x - lgamma(a) + ln(cf): finite where Q itself underflows.  x = 0: 0; x = +inf: -inf; x < 0 or NaN: NaN.
TPG_PCADAPT_HD static inline double tpg_logq(double a, double lga, double x) {
  if (!(x >= 0.0)) return NAN;
  if (x == 0.0) return 0.0;
  if (x > 1.79769313486231570815e308) return -INFINITY;
  if (x < a + 1.0) {
    double ap = a, del = 1.0 / a, sum = del;
    for (int it = 0; it < 10000; it++) {
      ap += 1.0;
      del *= x / ap;
      sum += del;
      if (del < sum * 1e-17) break;
    }
    const double P = sum * exp(a * log(x) - x - lga);
    return log1p(-P);
  }
  const double tiny = 1e-300;
  double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
  for (int i = 1; i <= 10000; i++) {
    const double an = -(double)i * ((double)i - a);
    b += 2.0;
    d = an * d + b;
    if (fabs(d) < tiny) d = tiny;
    c = b + an / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) < 1e-16) break;
  }
  return -x + a * log(x) - lga + log(h);
}

// log Q(df / 2, x / 2) for an integer df by the finite sums (the form tests/pcadapt_ref.py: logq_ref restates, operation by
// operation): h = x / 2; even df: -h + log(sum_{i < df/2} h^i / i!); odd df: log(erfc(sqrt h) + e^-h sum_{i < (df-1)/2}
// h^(i + 1/2) / Gamma(i + 3/2)).  Sums of positive terms: good to a few ulps around the median, which is all the bisection
// below asks of it (far in the tail the odd form underflows: that is tpg_logq's ground)
static inline double host_logq_chisq_finite(int df, double x) {
  const double h = x / 2;
  if (df % 2 == 0) {
    double term = 1.0, sum = 1.0;
    for (int i = 1; i < df / 2; i++) {
      term = term * h / (double)i;
      sum += term;
    }
    return -h + log(sum);
  }
  const double r = sqrt(h);
  double term = r / 0.886226925452758013649,  // Gamma(3/2) = sqrt(pi) / 2
      sum = 0.0;
  for (int i = 0; i < (df - 1) / 2; i++) {
    if (i > 0) term = term * h / ((double)i + 0.5);
    sum += term;
  }
  return log(erfc(r) + exp(-h) * sum);
}

// the median of chi-square(df): the root of log Q(df/2, x/2) = log(1/2) by bisection on [0, 2 df + 8] until the two ends are
// neighbouring doubles; the upper end is returned (log Q there is <= log(1/2))
static inline double host_qchisq_median(int df) {
  const double target = log(0.5);
  double lo = 0.0, hi = 2.0 * df + 8.0;
  for (;;) {
    const double mid = lo + (hi - lo) / 2;
    if (!(mid > lo && mid < hi)) break;
    if (host_logq_chisq_finite(df, mid) > target) lo = mid;
    else hi = mid;
  }
  return hi;
}

// One OGK iteration on the host: mad_sum / mad_diff hold MAD(Y_a + Y_b) and MAD(Y_a - Y_b) for the pairs a < b in the order
// (0,1), (0,2), ..., (0,K-1), (1,2), ...; R (K x K, column-major) and its eigenvectors E (columns, eigenvalues descending).
// false: a scale that is zero or not finite
static inline bool host_ogk_corr(int K, const double* mad_sum, const double* mad_diff, std::vector<double>& R,
                                 std::vector<double>& E) {
  R.assign((size_t)K * K, 0.0);
  size_t p = 0;
  for (int a = 0; a < K; a++) {
    R[a + (size_t)a * K] = 1.0;
    for (int b = a + 1; b < K; b++, p++) {
      const double sp = TPG_PCADAPT_MAD_SCALE * mad_sum[p], sm = TPG_PCADAPT_MAD_SCALE * mad_diff[p];
      if (!(sp > 0.0 && sp <= 1.79769313486231570815e308 && sm > 0.0 && sm <= 1.79769313486231570815e308)) return false;
      const double r = (sp * sp - sm * sm) / 4;
      R[a + (size_t)b * K] = r;
      R[b + (size_t)a * K] = r;
    }
  }
  std::vector<double> theta;
  host_sym_eig(R, K, theta, E);
  return true;
}

// Back to the coordinates of the input: a row of Z is x = B w with B = (D1 E1)(D2 E2), D_t = diag(s_t), so
// center = B nu and cov = B diag(Gamma) B'.  Plain loops in the order written:
//   A_t[i][l] = s_t[i] * E_t[i][l];  B[i][j] = sum_l A_1[i][l] * A_2[l][j] (l ascending);
//   center[i] = sum_k B[i][k] * nu[k];  cov[i][j] = sum_k (B[i][k] * Gamma[k]) * B[j][k]   (k ascending)
static inline void host_ogk_backmap(int K, const double* s1, const double* E1, const double* s2, const double* E2, const double* nu,
                                    const double* gamma, double* center, double* cov) {
  std::vector<double> B((size_t)K * K);
  for (int i = 0; i < K; i++)
    for (int j = 0; j < K; j++) {
      double acc = 0.0;
      for (int l = 0; l < K; l++) {
        const double a1 = s1[i] * E1[i + (size_t)l * K], a2 = s2[l] * E2[l + (size_t)j * K];
        acc += a1 * a2;
      }
      B[i + (size_t)j * K] = acc;
    }
  for (int i = 0; i < K; i++) {
    double acc = 0.0;
    for (int k = 0; k < K; k++) acc += B[i + (size_t)k * K] * nu[k];
    center[i] = acc;
    for (int j = 0; j < K; j++) {
      double c = 0.0;
      for (int k = 0; k < K; k++) c += (B[i + (size_t)k * K] * gamma[k]) * B[j + (size_t)k * K];
      cov[i + (size_t)j * K] = c;
    }
  }
}
