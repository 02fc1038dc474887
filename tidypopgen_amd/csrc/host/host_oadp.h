// host_oadp.h -- the per-individual arithmetic of include/tpg.h "OADP projection", written once for the host and the device.
// A TEAM works on one individual: the host's team is one thread (OadpSolo below), the device's a group of lanes of one wave
// (oadp.hip).  The team shares one workspace -- the (K+1) x (K+1) matrix, column-major with an odd leading dimension, and K+1
// doubles -- in host memory or in LDS.  Every floating-point sum is formed by ONE member in ascending index order and every
// column pair of a Jacobi round belongs to one member, so the result does not depend on the size of the team: the stand-alone
// program of tests/host/oadp_san.cpp runs the very arithmetic the kernel runs.  Compile with -ffp-contract=off.
//
// The two decompositions are one routine, a one-sided (Hestenes) Jacobi iteration on the columns of A in the fixed round-robin
// order of the circle method: A J = W with orthogonal columns, so W = (left vectors)(singular values) and J the right vectors.
//   M (K+1 x K+1): W = A S; its column of smallest norm goes last, the top K x K block of the rest is W1 = A1 S_K and the
//     last row w = a S_K.  No vectors are accumulated.
//   C = S_K A1' D = W1' D is never transposed: the iteration runs on C' = D W1 (the rows of W1 scaled in place), C' J = Z with
//     J = P and Z = W Sigma, so R = P W' = J Sigma^-1 Z' and the output c (w J) Sigma^-1 Z'.  The row w sits under C' and takes
//     every rotation, which is all of J that is needed; sigma_j is the norm of column j of Z.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TPG_OADP_FN __host__ __device__ static inline
#else
#define TPG_OADP_FN static inline
#endif

#define HOST_OADP_KMAX 32
#define HOST_OADP_MAX_SWEEPS 30
#define HOST_OADP_EPS 2.220446049250313e-16           // 2^-52: a pair with |a_i . a_j| <= eps |a_i| |a_j| is left alone
#define HOST_OADP_DEGENERATE 9.094947017729282e-13    // 2^-40: sigma_min(C) <= this times sigma_max(C) -> R is not unique

// leading dimension of the workspace matrix: odd, so that the columns a team's members read in one round lie in different banks
TPG_OADP_FN int host_oadp_ld(int K) { return (K + 1) | 1; }
// doubles of one individual's workspace
TPG_OADP_FN int host_oadp_ws_doubles(int K) { return host_oadp_ld(K) * (K + 1) + (K + 1) + ((K + 1) & 1); }

// the team of one: the host
struct OadpSolo {
  int lane() const { return 0; }
  int size() const { return 1; }
  void sync() const {}
  bool any(bool b) const { return b; }
};

// Columns 0 .. nc-1 of A (column-major, leading dimension ld) are rotated until they are orthogonal over rows 0 .. nd-1; every
// rotation is applied to rows 0 .. nr-1 (nr >= nd).  Round-robin: with m = nc or nc - 1, whichever is odd, round s pairs
// (s + p) mod m with (s - p) mod m for p = 1 .. (m-1)/2, and column s with column nc-1 when nc is even.  A sweep is m rounds;
// the iteration ends after a sweep without a rotation (any() may extend that to the teams that share a workgroup: a sweep over
// converged columns rotates nothing and changes no bit), or after HOST_OADP_MAX_SWEEPS.
template <class Team>
TPG_OADP_FN void host_oadp_jacobi(const Team& t, double* A, int ld, int nd, int nr, int nc) {
  const int odd = nc & 1, np = (nc + 1) / 2, m = nc - 1 + odd;
  for (int sweep = 0; sweep < HOST_OADP_MAX_SWEEPS; sweep++) {
    bool rotated = false;
    for (int s = 0; s < m; s++) {
      for (int p = t.lane() + odd; p < np; p += t.size()) {
        int i = p == 0 ? s : (s + p) % m, j = p == 0 ? nc - 1 : (s + m - p) % m;
        if (i > j) { const int h = i; i = j; j = h; }
        double* ai = A + (size_t)i * ld;
        double* aj = A + (size_t)j * ld;
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int r = 0; r < nd; r++) {
          const double x = ai[r], y = aj[r];
          al += x * x;
          be += y * y;
          ga += x * y;
        }
        if (fabs(ga) > HOST_OADP_EPS * sqrt(al * be)) {
          rotated = true;
          const double zeta = (be - al) / (2.0 * ga);
          const double tn = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
          for (int r = 0; r < nr; r++) {
            const double x = ai[r], y = aj[r];
            ai[r] = cs * x - sn * y;
            aj[r] = sn * x + cs * y;
          }
        }
      }
      t.sync();
    }
    if (!t.any(rotated)) break;
  }
}

// One individual.  l: its row of XV, entries ldl apart (NULL: a row of zeros with s = 0, the filler of a workgroup's last
// teams); s: its squared norm; d: the K singular values (readable by every member); ws: host_oadp_ws_doubles(K) doubles shared
// by the team; out: the K results, entries ldo apart (NULL: nothing is stored).  Returns 1 when the row is degenerate (it is
// then NaN), the same value in every member.
template <class Team>
TPG_OADP_FN int host_oadp_project(const Team& t, int K, const double* l, int64_t ldl, double s, const double* d, double* ws,
                                  double* out, int64_t ldo) {
  const int n = K + 1, ld = host_oadp_ld(K);
  double* A = ws;
  double* w = ws + (size_t)ld * n;
  // M: diag(d), the last row (l, rho), rho^2 = max(s - |l|^2, 0)
  double ssq = 0.0;
  if (l)
    for (int k = 0; k < K; k++) ssq += l[(int64_t)k * ldl] * l[(int64_t)k * ldl];
  else
    s = 0.0;
  const double rho2 = s - ssq;
  for (int idx = t.lane(); idx < n * n; idx += t.size()) {
    const int r = idx % n, c = idx / n;
    double v = 0.0;
    if (r == c) v = r < K ? d[r] : (rho2 > 0.0 ? sqrt(rho2) : 0.0);
    else if (r == K && l) v = l[(int64_t)c * ldl];
    A[r + (size_t)c * ld] = v;
  }
  t.sync();
  host_oadp_jacobi(t, A, ld, n, n, n);
  // the column of smallest norm (the last of equals) goes to position K
  for (int c = t.lane(); c < n; c += t.size()) {
    double q = 0.0;
    for (int r = 0; r < n; r++) q += A[r + (size_t)c * ld] * A[r + (size_t)c * ld];
    w[c] = q;
  }
  t.sync();
  int jmin = 0;
  for (int c = 1; c < n; c++)
    if (w[c] <= w[jmin]) jmin = c;
  t.sync();
  if (jmin != K)
    for (int r = t.lane(); r < n; r += t.size()) {
      const double x = A[r + (size_t)jmin * ld];
      A[r + (size_t)jmin * ld] = A[r + (size_t)K * ld];
      A[r + (size_t)K * ld] = x;
    }
  t.sync();
  // |W1|_F^2 column by column, and C' = D W1 in place
  for (int c = t.lane(); c < K; c += t.size()) {
    double q = 0.0;
    for (int r = 0; r < K; r++) {
      const double x = A[r + (size_t)c * ld];
      q += x * x;
      A[r + (size_t)c * ld] = d[r] * x;
    }
    w[c] = q;
  }
  t.sync();
  double fro = 0.0;
  for (int c = 0; c < K; c++) fro += w[c];
  t.sync();
  host_oadp_jacobi(t, A, ld, K, n, K);
  for (int c = t.lane(); c < K; c += t.size()) {
    double q = 0.0;
    for (int r = 0; r < K; r++) q += A[r + (size_t)c * ld] * A[r + (size_t)c * ld];
    w[c] = sqrt(q);
  }
  t.sync();
  double smax = w[0], smin = w[0], tr = 0.0;
  for (int c = 0; c < K; c++) {
    tr += w[c];
    if (w[c] > smax) smax = w[c];
    if (w[c] < smin) smin = w[c];
  }
  const int degenerate = !(smin > HOST_OADP_DEGENERATE * smax) || !(fro > 0.0);  // (a NaN anywhere lands here too)
  for (int c = t.lane(); c < K; c += t.size()) A[K + (size_t)c * ld] = A[K + (size_t)c * ld] / w[c];
  t.sync();
  const double coef = tr / fro;
  if (out)
    for (int i = t.lane(); i < K; i += t.size()) {
      double y = 0.0;
      for (int c = 0; c < K; c++) y += A[K + (size_t)c * ld] * A[i + (size_t)c * ld];
      out[(int64_t)i * ldo] = degenerate ? (double)NAN : coef * y;
    }
  t.sync();
  return degenerate;
}

// Argument check of the singular values: 0 fine, 1 not finite, 2 not positive or not descending
static inline int host_oadp_check_sval(const double* d, int K) {
  for (int k = 0; k < K; k++)
    if (!(fabs(d[k]) <= 1.79769313486231570815e308)) return 1;
  for (int k = 0; k < K; k++)
    if (!(d[k] > 0.0) || (k > 0 && d[k] > d[k - 1])) return 2;
  return 0;
}

// Every individual on the host: XV n x K and out n x K column-major; ws: host_oadp_ws_doubles(K) doubles.  Returns the count of
// degenerate rows.
static inline int64_t host_oadp_all(const double* XV, const double* X_norm, int64_t n, int K, const double* d, double* ws, double* out) {
  int64_t deg = 0;
  const OadpSolo solo;
  for (int64_t i = 0; i < n; i++) deg += host_oadp_project(solo, K, XV + i, n, X_norm[i], d, ws, out + i, n);
  return deg;
}
