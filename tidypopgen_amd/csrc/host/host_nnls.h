// host_nnls.h -- the non-negative least squares solver of include/tpg.h "sNMF", one system per call: Lawson and Hanson's active-set
// method on the normal equations with a KT-bit passive mask.  An inner solve is a fully unrolled KT x KT Cholesky factorisation of
// the masked matrix (identity rows for the inactive k, so every index is a compile-time constant and the factor can live in
// registers) followed by one step of iterative refinement.  Plain C++ with fma(): snmf.hip runs it one thread per system with
// the matrix in LDS; tests/host/nnls_san.cpp builds the same text for the host.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../../include/tpg.h"

#if defined(__HIPCC__)
#define TPG_NNLS_FN __host__ __device__ __forceinline__
#else
#define TPG_NNLS_FN inline
#endif

// Cholesky factor of the masked matrix: row i, column j <= i at i (i + 1) / 2 + j; the diagonal holds 1 / l(i, i)
template <int KT>
struct SnmfChol {
  double L[KT * (KT + 1) / 2];

  TPG_NNLS_FN void factor(const double* __restrict__ A, uint32_t P) {
#pragma unroll
    for (int j = 0; j < KT; j++) {
      const bool pj = (P >> j) & 1u;
      double d = pj ? A[j * KT + j] : 1.0;
#pragma unroll
      for (int p = 0; p < j; p++) d = fma(-L[j * (j + 1) / 2 + p], L[j * (j + 1) / 2 + p], d);
      const double inv = 1.0 / sqrt(d);
      L[j * (j + 1) / 2 + j] = inv;
#pragma unroll
      for (int i = j + 1; i < KT; i++) {
        double a = pj && ((P >> i) & 1u) ? A[i * KT + j] : 0.0;
#pragma unroll
        for (int p = 0; p < j; p++) a = fma(-L[i * (i + 1) / 2 + p], L[j * (j + 1) / 2 + p], a);
        L[i * (i + 1) / 2 + j] = a * inv;
      }
    }
  }

  TPG_NNLS_FN void solve(const double (&rhs)[KT], double (&x)[KT]) const {
#pragma unroll
    for (int i = 0; i < KT; i++) {
      double y = rhs[i];
#pragma unroll
      for (int p = 0; p < i; p++) y = fma(-L[i * (i + 1) / 2 + p], x[p], y);
      x[i] = y * L[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = KT - 1; i >= 0; i--) {
      double y = x[i];
#pragma unroll
      for (int p = i + 1; p < KT; p++) y = fma(-L[p * (p + 1) / 2 + i], x[p], y);
      x[i] = y * L[i * (i + 1) / 2 + i];
    }
  }
};

// s = the solution of the system restricted to the passive set P (0 elsewhere), one step of iterative refinement
template <int KT>
TPG_NNLS_FN void snmf_passive_solve(const double* __restrict__ A, uint32_t P, const double (&b)[KT], double (&s)[KT]) {
  SnmfChol<KT> ch;
  ch.factor(A, P);
  double r[KT], d[KT];
#pragma unroll
  for (int k = 0; k < KT; k++) r[k] = (P >> k) & 1u ? b[k] : 0.0;
  ch.solve(r, s);
#pragma unroll
  for (int k = 0; k < KT; k++) {
    double t = b[k];
#pragma unroll
    for (int l = 0; l < KT; l++) t = fma(-A[k * KT + l], s[l], t);
    r[k] = (P >> k) & 1u ? t : 0.0;
  }
  ch.solve(r, d);
#pragma unroll
  for (int k = 0; k < KT; k++) s[k] += d[k];
}

// x = NNLS(A, b) of include/tpg.h; A: KT x KT in LDS.  -> whether x meets the contract
template <int KT>
TPG_NNLS_FN bool snmf_nnls(const double* __restrict__ A, const double (&b)[KT], double (&x)[KT]) {
  double bmax = 0.0;
#pragma unroll
  for (int k = 0; k < KT; k++) {
    bmax = fmax(bmax, fabs(b[k]));
    x[k] = 0.0;
  }
  const double tol = TPG_SNMF_KKT_TOL * bmax;
  uint32_t P = 0, tabu = 0;  // tabu: candidates whose own solution was not positive; cleared whenever x moves
  for (int outer = 0; outer < 3 * KT + 4; outer++) {
    // the candidate with the largest gradient w = b - A x
    double wbest = 0.5 * tol;
    int kb = -1;
#pragma unroll
    for (int k = 0; k < KT; k++) {
      double wk = b[k];
#pragma unroll
      for (int l = 0; l < KT; l++) wk = fma(-A[k * KT + l], x[l], wk);
      if (!(((P | tabu) >> k) & 1u) && wk > wbest) {
        wbest = wk;
        kb = k;
      }
    }
    if (kb < 0) break;
    P |= 1u << kb;
    for (int inner = 0; inner <= KT; inner++) {
      double s[KT];
      snmf_passive_solve<KT>(A, P, b, s);
      if (inner == 0) {
        double skb = 0.0;
#pragma unroll
        for (int k = 0; k < KT; k++) skb = k == kb ? s[k] : skb;
        if (!(skb > 0.0)) {  // rounding only: the candidate leaves again and is not tried until x moves
          P &= ~(1u << kb);
          tabu |= 1u << kb;
          break;
        }
      }
      double alpha = 2.0;
#pragma unroll
      for (int k = 0; k < KT; k++)
        if (((P >> k) & 1u) && !(s[k] > 0.0)) alpha = fmin(alpha, x[k] / (x[k] - s[k]));
      tabu = 0;
      if (alpha > 1.0) {  // feasible: accept
#pragma unroll
        for (int k = 0; k < KT; k++) x[k] = (P >> k) & 1u ? s[k] : 0.0;
        break;
      }
      // towards s as far as x >= 0 allows; whoever reaches 0 leaves the passive set
#pragma unroll
      for (int k = 0; k < KT; k++) {
        if (!((P >> k) & 1u)) continue;
        const bool leaves = !(s[k] > 0.0) && x[k] / (x[k] - s[k]) <= alpha;
        const double xn = x[k] + alpha * (s[k] - x[k]);
        if (leaves || !(xn > 0.0)) {
          x[k] = 0.0;
          P &= ~(1u << k);
        } else {
          x[k] = xn;
        }
      }
    }
  }
  bool ok = true;
#pragma unroll
  for (int k = 0; k < KT; k++) x[k] = x[k] > 0.0 ? x[k] : 0.0;
#pragma unroll
  for (int k = 0; k < KT; k++) {
    double wk = b[k];
#pragma unroll
    for (int l = 0; l < KT; l++) wk = fma(-A[k * KT + l], x[l], wk);
    ok &= x[k] > 0.0 ? fabs(wk) <= tol : wk <= tol;
  }
  return ok;
}
