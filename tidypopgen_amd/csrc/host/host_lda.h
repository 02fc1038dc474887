// host_lda.h -- the discriminant analysis of include/tpg.h "DAPC" on the host: n x d scores with d <= 64, so everything is a
// handful of d x d matrices.  The Cholesky factor, the triangular inverse and the symmetric eigen-decomposition are those of
// host_eig.h.  Plain C++ with no HIP in it: kmeans.hip exports it as tpg_lda and tests/host/lda_san.cpp builds the same text
// under the host sanitizers.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "host_eig.h"

#define HOST_LDA_OK 0
#define HOST_LDA_EINVAL 1
#define HOST_LDA_ENUMERIC 4

// Outputs as tpg_lda documents them (column-major; Lmax = min(d, G - 1)).  *why names the refusal.
static inline int host_lda(const double* X, int64_t n, int d, const int32_t* grp, int G, int n_da_asked, double* prior, double* means,
                           double* mu_out, double* scaling, double* svd, int32_t* n_lda, int32_t* n_da_out, double* ind_coord,
                           double* grp_coord, double* posterior, int32_t* assign, const char** why) {
  *why = "";
  if (d < 1 || d > 64) { *why = "d outside [1, 64]"; return HOST_LDA_EINVAL; }
  if (G < 2) { *why = "fewer than two groups"; return HOST_LDA_EINVAL; }
  if (n <= G) { *why = "n <= G: no within-group degrees of freedom"; return HOST_LDA_EINVAL; }
  if (n_da_asked < 1) { *why = "n_da < 1"; return HOST_LDA_EINVAL; }
  const size_t D = (size_t)d, N = (size_t)n, Gs = (size_t)G;
  std::vector<int64_t> cnt(Gs, 0);
  for (size_t i = 0; i < N; i++) {
    if (grp[i] < 0 || grp[i] >= G) { *why = "a group label outside [0, G)"; return HOST_LDA_EINVAL; }
    cnt[(size_t)grp[i]]++;
  }
  for (size_t g = 0; g < Gs; g++)
    if (cnt[g] == 0) { *why = "an empty group"; return HOST_LDA_EINVAL; }
  for (size_t t = 0; t < N * D; t++)
    if (!std::isfinite(X[t])) { *why = "a score that is not finite"; return HOST_LDA_ENUMERIC; }

  // group means (sums in ascending i), priors, the grand mean
  std::vector<double> mg(Gs * D, 0.0), mu(D, 0.0), pi(Gs);
  for (size_t j = 0; j < D; j++)
    for (size_t i = 0; i < N; i++) mg[(size_t)grp[i] + j * Gs] += X[i + j * N];
  for (size_t g = 0; g < Gs; g++) {
    pi[g] = (double)cnt[g] / (double)n;
    for (size_t j = 0; j < D; j++) mg[g + j * Gs] /= (double)cnt[g];
  }
  for (size_t j = 0; j < D; j++)
    for (size_t g = 0; g < Gs; g++) mu[j] += pi[g] * mg[g + j * Gs];

  // W and B
  std::vector<double> W(D * D, 0.0), B(D * D, 0.0), r(D);
  for (size_t i = 0; i < N; i++) {
    const size_t g = (size_t)grp[i];
    for (size_t j = 0; j < D; j++) r[j] = X[i + j * N] - mg[g + j * Gs];
    for (size_t b = 0; b < D; b++)
      for (size_t a = 0; a < D; a++) W[a + b * D] += r[a] * r[b];
  }
  for (double& w : W) w /= (double)(n - G);
  for (size_t g = 0; g < Gs; g++) {
    for (size_t j = 0; j < D; j++) r[j] = mg[g + j * Gs] - mu[j];
    for (size_t b = 0; b < D; b++)
      for (size_t a = 0; a < D; a++) B[a + b * D] += (double)cnt[g] * r[a] * r[b];
  }
  for (double& b : B) b /= (double)(G - 1);

  // W = R'R; a pivot that is nothing beside the variable's total variance: singular within the groups
  std::vector<double> R = W, Ri, tv(D, 0.0);
  for (size_t j = 0; j < D; j++) {
    for (size_t i = 0; i < N; i++) tv[j] += (X[i + j * N] - mu[j]) * (X[i + j * N] - mu[j]);
    tv[j] /= (double)(n - 1);
  }
  const bool factored = host_cholesky_upper(R, d);
  for (size_t j = 0; j < D; j++)
    if (!factored || !(R[j + j * D] * R[j + j * D] > ldexp(tv[j], -40))) {
      *why = "W is singular: a variable is constant, or a combination of the others, within the groups";
      return HOST_LDA_ENUMERIC;
    }
  host_upper_inverse(R, d, Ri);
  // M = Ri' B Ri
  std::vector<double> T(D * D, 0.0), M(D * D, 0.0);
  for (size_t b = 0; b < D; b++)
    for (size_t a = 0; a < D; a++) {
      double s = 0;
      for (size_t k = 0; k < D; k++) s += B[a + k * D] * Ri[k + b * D];
      T[a + b * D] = s;
    }
  for (size_t b = 0; b < D; b++)
    for (size_t a = 0; a < D; a++) {
      double s = 0;
      for (size_t k = 0; k < D; k++) s += Ri[k + a * D] * T[k + b * D];
      M[a + b * D] = s;
    }
  std::vector<double> lambda, E;
  host_sym_eig(M, d, lambda, E);
  const size_t Lmax = (size_t)(d < G - 1 ? d : G - 1);
  size_t L = 0;
  while (L < Lmax && lambda[L] > 1e-10) L++;
  std::vector<double> S(D * Lmax, 0.0);
  for (size_t a = 0; a < L; a++) {
    for (size_t j = 0; j < D; j++) {
      double s = 0;
      for (size_t k = 0; k < D; k++) s += Ri[j + k * D] * E[k + a * D];
      S[j + a * D] = s;
    }
    size_t big = 0;
    for (size_t j = 1; j < D; j++)
      if (fabs(S[j + a * D]) > fabs(S[big + a * D])) big = j;
    if (S[big + a * D] < 0)
      for (size_t j = 0; j < D; j++) S[j + a * D] = -S[j + a * D];
  }
  size_t nda = (size_t)n_da_asked;
  if (nda > Lmax) nda = Lmax;
  if (nda > L) nda = L;
  if (nda < 1) { *why = "no discriminant function separates the groups"; return HOST_LDA_ENUMERIC; }

  for (size_t g = 0; g < Gs; g++) prior[g] = pi[g];
  for (size_t t = 0; t < Gs * D; t++) means[t] = mg[t];
  if (mu_out)
    for (size_t j = 0; j < D; j++) mu_out[j] = mu[j];
  for (size_t t = 0; t < D * Lmax; t++) scaling[t] = S[t];
  for (size_t a = 0; a < Lmax; a++) svd[a] = a < L ? sqrt(lambda[a] > 0 ? lambda[a] : 0.0) : 0.0;
  *n_lda = (int32_t)L;
  *n_da_out = (int32_t)nda;

  // coordinates, their group means, the group centres m_g
  std::vector<double> mgc(Gs * nda, 0.0);
  for (size_t a = 0; a < nda; a++) {
    for (size_t i = 0; i < N; i++) {
      double s = 0;
      for (size_t j = 0; j < D; j++) s += (X[i + j * N] - mu[j]) * S[j + a * D];
      ind_coord[i + a * N] = s;
    }
    for (size_t g = 0; g < Gs; g++) grp_coord[g + a * Gs] = 0.0;
    for (size_t i = 0; i < N; i++) grp_coord[(size_t)grp[i] + a * Gs] += ind_coord[i + a * N];
    for (size_t g = 0; g < Gs; g++) {
      grp_coord[g + a * Gs] /= (double)cnt[g];
      double s = 0;
      for (size_t j = 0; j < D; j++) s += (mg[g + j * Gs] - mu[j]) * S[j + a * D];
      mgc[g + a * Gs] = s;
    }
  }
  std::vector<double> q(Gs);
  for (size_t i = 0; i < N; i++) {
    size_t best = 0;
    for (size_t g = 0; g < Gs; g++) {
      double s = 0;
      for (size_t a = 0; a < nda; a++) {
        const double t = ind_coord[i + a * N] - mgc[g + a * Gs];
        s += t * t;
      }
      q[g] = 0.5 * s - log(pi[g]);
      if (q[g] < q[best]) best = g;
    }
    double tot = 0;
    for (size_t g = 0; g < Gs; g++) {
      posterior[i + g * N] = exp(-(q[g] - q[best]));
      tot += posterior[i + g * N];
    }
    for (size_t g = 0; g < Gs; g++) posterior[i + g * N] /= tot;
    assign[i] = (int32_t)best;
  }
  return HOST_LDA_OK;
}
