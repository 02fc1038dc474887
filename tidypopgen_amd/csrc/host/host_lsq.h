// host_lsq.h -- the per-individual solve of include/tpg.h "least-squares projection", written once for the host and the device.
// A TEAM works on one individual: the host's team is one thread (LsqSolo below), the device's a group of lanes of one wave
// (lsq.hip).  The team shares one workspace of P + 2 L doubles, P = L (L + 1) / 2 -- the packed upper triangle of A, which
// becomes the Cholesky factor R (A = R'R) in place, then y and x -- in host memory or in LDS.  Every floating-point sum is
// formed by ONE member in ascending index order, starting from 0, and is subtracted once, so the result does not depend on the
// size of the team: the stand-alone program of tests/host/lsq_san.cpp runs the very arithmetic the kernel runs.  Compile with
// -ffp-contract=off.
//
// Packed order: (a, b), a <= b, a-major: row a of the upper triangle is contiguous and starts at host_lsq_idx(L, a, a).
//   Cholesky, row by row: p_k = A[k,k] - sum_{c<k} R[c,k]^2 (every member forms it: the same bits, no exchange), R[k,k] = sqrt(p_k),
//     R[k,b] = (A[k,b] - sum_{c<k} R[c,k] R[c,b]) / R[k,k] for b > k, one member per b.
//   R'y = b:  y_k = (b_k - sum_{c<k} R[c,k] y_c) / R[k,k], k ascending, member k mod size.
//   R x = y:  x_k = (y_k - sum_{c>k} R[k,c] x_c) / R[k,k], k descending, member k mod size.
// Singular rule (include/tpg.h): t < L, or a pivot that fails p_k > L 2^-52 A[k,k] (A[k,k] as given, before it is overwritten),
// or is not finite.  The arithmetic of a singular row runs to its end all the same -- the barriers of a team stay whole -- and
// its result is replaced by NaN.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TPG_LSQ_FN __host__ __device__ static inline
#else
#define TPG_LSQ_FN static inline
#endif

#define HOST_LSQ_MAX_L 32
#define HOST_LSQ_EPS 2.220446049250313e-16  // 2^-52
#define HOST_LSQ_DBL_MAX 1.79769313486231570815e308

TPG_LSQ_FN int host_lsq_pairs(int L) { return L * (L + 1) / 2; }
// packed index of (a, b), a <= b
TPG_LSQ_FN int host_lsq_idx(int L, int a, int b) { return a * L - a * (a - 1) / 2 + (b - a); }
// doubles of one individual's workspace
TPG_LSQ_FN int host_lsq_ws_doubles(int L) { return host_lsq_pairs(L) + 2 * L; }

// the team of one: the host
struct LsqSolo {
  int lane() const { return 0; }
  int size() const { return 1; }
  void sync() const {}
};

// One individual.  A: its P packed sums, entries lda apart (NULL: the filler of a workgroup's last teams, a row of zeros with
// t = 0); b: its L right-hand sides, entries ldb apart; t: its typed loci; ws: host_lsq_ws_doubles(L) doubles shared by the
// team; out: the L results, entries ldo apart (NULL: nothing is stored).  Returns 1 when the row is singular (it is then NaN),
// the same value in every member.
template <class Team>
TPG_LSQ_FN int host_lsq_solve_row(const Team& tm, int L, const double* A, int64_t lda, const double* b, int64_t ldb, int64_t t, double* ws,
                                  double* out, int64_t ldo) {
  const int P = host_lsq_pairs(L);
  double* R = ws;
  double* y = ws + P;
  double* x = ws + P + L;
  for (int p = tm.lane(); p < P; p += tm.size()) R[p] = A ? A[(int64_t)p * lda] : 0.0;
  for (int k = tm.lane(); k < L; k += tm.size()) y[k] = A ? b[(int64_t)k * ldb] : 0.0;
  tm.sync();
  int singular = (!A || t < (int64_t)L) ? 1 : 0;
  const double tol = (double)L * HOST_LSQ_EPS;
  for (int k = 0; k < L; k++) {
    const int kk = host_lsq_idx(L, k, k);
    const double akk = R[kk];
    double s = 0.0;
    for (int c = 0; c < k; c++) {
      const double r = R[host_lsq_idx(L, c, k)];
      s += r * r;
    }
    const double piv = akk - s;
    if (!(piv > tol * akk) || !(piv <= HOST_LSQ_DBL_MAX)) singular = 1;
    const double rkk = sqrt(piv);
    tm.sync();  // every member has read A[k,k]
    for (int bcol = k + tm.lane(); bcol < L; bcol += tm.size()) {
      if (bcol == k) {
        R[kk] = rkk;
        continue;
      }
      double q = 0.0;
      for (int c = 0; c < k; c++) q += R[host_lsq_idx(L, c, k)] * R[host_lsq_idx(L, c, bcol)];
      R[kk + (bcol - k)] = (R[kk + (bcol - k)] - q) / rkk;
    }
    tm.sync();
  }
  for (int k = 0; k < L; k++) {
    if (k % tm.size() == tm.lane()) {
      double q = 0.0;
      for (int c = 0; c < k; c++) q += R[host_lsq_idx(L, c, k)] * y[c];
      y[k] = (y[k] - q) / R[host_lsq_idx(L, k, k)];
    }
    tm.sync();
  }
  for (int k = L - 1; k >= 0; k--) {
    if (k % tm.size() == tm.lane()) {
      const int kk = host_lsq_idx(L, k, k);
      double q = 0.0;
      for (int c = k + 1; c < L; c++) q += R[kk + (c - k)] * x[c];
      x[k] = (y[k] - q) / R[kk];
    }
    tm.sync();
  }
  if (out)
    for (int k = tm.lane(); k < L; k += tm.size()) out[(int64_t)k * ldo] = singular ? (double)NAN : x[k];
  tm.sync();
  return singular;
}

// Argument check of A (n x P) and b (n x L): 1 when a value is not finite, else 0
static inline int host_lsq_check(const double* A, const double* b, int64_t n, int L) {
  const int64_t P = host_lsq_pairs(L);
  for (int64_t i = 0; i < n * P; i++)
    if (!(fabs(A[i]) <= HOST_LSQ_DBL_MAX)) return 1;
  for (int64_t i = 0; i < n * L; i++)
    if (!(fabs(b[i]) <= HOST_LSQ_DBL_MAX)) return 1;
  return 0;
}

// Every individual on the host: A n x P, b n x L and out n x L column-major; ws: host_lsq_ws_doubles(L) doubles.  Returns the
// count of singular rows.
static inline int64_t host_lsq_all(const double* A, const double* b, const int64_t* nt, int64_t n, int L, double* ws, double* out) {
  int64_t sing = 0;
  const LsqSolo solo;
  for (int64_t i = 0; i < n; i++) sing += host_lsq_solve_row(solo, L, A + i, n, b + i, n, nt[i], ws, out + i, n);
  return sing;
}
