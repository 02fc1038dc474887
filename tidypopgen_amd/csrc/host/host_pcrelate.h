// host_pcrelate.h -- the host half of include/tpg.h "PC-Relate": step 0 (the orthonormal basis Q of span[1, V]) and, written once
// for the host and the device, the pinned expressions of step 2 (the individual-specific allele frequency and the three
// operands) and of step 4 (the epilogue).  Compile with -ffp-contract=off: every product below is rounded before it is added.
//
// Basis.  Q is n x L column-major, L = K + 1.  Column 0 is 1 / sqrt(n).  Column j = 1 .. K starts as w = V[, j - 1] with
// nb = sqrt(sum_i w_i^2); then TWICE, for p = 0 .. j - 1 in turn: d = sum_i Q_ip w_i, w_i = w_i - d Q_ip (modified Gram-Schmidt,
// every sum ascending in i from +0); na = sqrt(sum_i w_i^2) and Q_ij = w_i / na.  The design is rank deficient -- the call
// refuses it -- when na > n 2^-52 nb fails (a NaN or an infinity in V fails it too).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TPG_PCR_FN __host__ __device__ static inline
#else
#define TPG_PCR_FN static inline
#endif

#define HOST_PCRELATE_MAX_K 32
#define HOST_PCRELATE_EPS 2.220446049250313e-16  // 2^-52

// 0, or 1 (the arguments: K outside [0, 32], n < L + 1), or 2 (a column that the columns before it explain: rank deficient)
static inline int host_pcrelate_basis(const double* V, int64_t n, int K, double* Q) {
  if (K < 0 || K > HOST_PCRELATE_MAX_K || n < (int64_t)K + 2) return 1;
  const double q0 = 1.0 / sqrt((double)n);
  for (int64_t i = 0; i < n; i++) Q[i] = q0;
  for (int j = 1; j <= K; j++) {
    double* w = Q + (int64_t)j * n;
    const double* v = V + (int64_t)(j - 1) * n;
    double s = 0.0;
    for (int64_t i = 0; i < n; i++) {
      w[i] = v[i];
      s += w[i] * w[i];
    }
    const double nb = sqrt(s);
    for (int pass = 0; pass < 2; pass++) {
      for (int p = 0; p < j; p++) {
        const double* q = Q + (int64_t)p * n;
        double d = 0.0;
        for (int64_t i = 0; i < n; i++) d += q[i] * w[i];
        for (int64_t i = 0; i < n; i++) w[i] = w[i] - d * q[i];
      }
    }
    s = 0.0;
    for (int64_t i = 0; i < n; i++) s += w[i] * w[i];
    const double na = sqrt(s);
    if (!(na > (double)n * HOST_PCRELATE_EPS * nb)) return 2;
    for (int64_t i = 0; i < n; i++) w[i] = w[i] / na;
  }
  return 0;
}

// step 2: twice the frequency, a = mean + sum_k q[k qs] c[k cs] with k ascending and every product rounded on its own; mu = 0.5 a
TPG_PCR_FN double host_pcrelate_mu(double mean, const double* q, int64_t qs, const double* c, int64_t cs, int L) {
  double a = mean;
  for (int k = 0; k < L; k++) a = a + q[k * qs] * c[k * cs];
  return 0.5 * a;
}
// valid = typed and thr <= mu <= hi, hi = 1 - thr rounded once by the caller
TPG_PCR_FN bool host_pcrelate_valid(int code, double mu, double thr, double hi) { return code != 3 && mu >= thr && mu <= hi; }
// the operands of a VALID cell: R = g - 2 mu (2 mu is exact), S = sqrt(mu (1 - mu)); an invalid cell is 0 in both
TPG_PCR_FN double host_pcrelate_r(int code, double mu) { return (double)code - 2.0 * mu; }
TPG_PCR_FN double host_pcrelate_s(double mu) { return sqrt(mu * (1.0 - mu)); }
// step 4
TPG_PCR_FN double host_pcrelate_kin(double num, double den) { return num / (4.0 * den); }
TPG_PCR_FN double host_pcrelate_f(double kin_ii) { return 2.0 * kin_ii - 1.0; }
