// fst_terms.h -- the per-locus, per-pair Fst terms shared by fst.hip (whole-view and by-locus Fst) and winfst.hip (windowed
// Fst): the reference's arithmetic statement for statement.  Include it only from files compiled with -ffp-contract=off.
#pragma once
#include <math.h>

#include "common.h"
#include "devfrag.h"


// e1 / e2: the per-(locus, population) term staged once per locus chunk -- Hudson: p q / (n - 1), hoisted out of
// the pair loop with its operation order unchanged (src/pairwise_fst_hudson_loop.cpp:28-29), so values stay
// bit-identical.  FAST (only when no by-locus output is requested): WC84 with 3 divisions instead of 8
// (reciprocals reused); the ratio of sums moves by ~1e-15 relative.
// 1 / x to ~1 ulp: v_rcp_f64 (about 2^-23 relative) and two Newton steps.  x = 0 or inf gives NaN, callers guard.
__device__ __forceinline__ double fst_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  double e = fma(-x, r, 1.0);
  r = fma(e, r, r);
  e = fma(-x, r, 1.0);
  return fma(e, r, r);
}

template <int METHOD, bool FAST>
__device__ __forceinline__ void fst_terms(double n1, double p1, double h1, double e1, double n2, double p2, double h2,
                                          double e2, double& num, double& den) {
  if (METHOD == TPG_FST_HUDSON) {
    // src/pairwise_fst_hudson_loop.cpp:27-32
    const double q1 = 1 - p1, q2 = 1 - p2;  // freq_ref = 1 - freq_alt (grouped_summaries :53)
    const double d = p1 - p2;
    num = d * d - e1 - e2;
    den = p1 * q2 + p2 * q1;
  } else if (METHOD == TPG_FST_WC84 && FAST) {
    // Sums only (no per-locus output): the same estimator with the two-population algebra done by hand.
    // Staged per (locus, population): n1 = individuals (allele count / 2), h1 = het_obs * individuals, e1 = 1 /
    // individuals.  With r = 2:  n_c = 2 n1 n2 / nt,  s2 = 2 d^2 n1 n2 / nt^2  (d = p1 - p2), so
    // n_bar / n_c * s2 = d^2 / 2 and n_bar / n_c = nt^2 / (4 n1 n2): two reciprocals per pair and locus (by
    // v_rcp_f64 + two Newton steps) instead of three IEEE divisions, ~50 FP64 instructions instead of ~100.
    // Differs from the statement-order path by rounding only (tests: <= 1e-12 relative on the sums).
    const double nt = n1 + n2;
    const double inv_nt = fst_rcp(nt);
    const double nb1 = 0.5 * nt - 1.0;
    double inv_nb1 = fst_rcp(nb1);
    if (nb1 == 0.0) inv_nb1 = HUGE_VAL;  // one individual per population (nb1 = +0): the reference's 1 / 0 = +inf
    const double p_bar = (p1 * n1 + p2 * n2) * inv_nt, h_bar = (h1 + h2) * inv_nt;
    const double d = p1 - p2, hd2 = 0.5 * (d * d);
    const double half_s2 = (2.0 * hd2) * (n1 * n2) * (inv_nt * inv_nt);
    const double core = p_bar * (1.0 - p_bar) - half_s2;
    const double X = (0.25 * (nt * nt)) * (e1 * e2) * inv_nb1;
    const double a = hd2 - X * (core - 0.25 * h_bar);
    const double b = (0.5 * nt) * inv_nb1 * (core - (0.5 * (nt - 1.0)) * inv_nt * h_bar);
    num = a;
    den = a + b + 0.5 * h_bar;
  } else if (METHOD == TPG_FST_WC84) {
    // src/pairwise_fst_wc84_loop.cpp:41-99 with r = 2
    const double r = 2.0;
    const double ni1 = n1 / 2.0, ni2 = n2 / 2.0;
    double sum_n = 0.0, sum_sq = 0.0;
    sum_n += ni1; sum_sq += ni1 * ni1;
    sum_n += ni2; sum_sq += ni2 * ni2;
    const double n_total = sum_n, n_bar = sum_n / 2;
    const double n_c = (sum_n - sum_sq / sum_n) / (2 - 1);
    double sum_pn = 0.0, sum_h = 0.0;
    sum_pn += p1 * ni1; sum_h += h1 * ni1;
    sum_pn += p2 * ni2; sum_h += h2 * ni2;
    const double p_bar = sum_pn / n_total, h_bar = sum_h / n_total;
    double sum_sq_diff = 0.0;
    sum_sq_diff += (p1 - p_bar) * (p1 - p_bar) * ni1;
    sum_sq_diff += (p2 - p_bar) * (p2 - p_bar) * ni2;
    const double s2 = sum_sq_diff / (n_bar * (2 - 1));
    const double a = n_bar / n_c * (s2 - (1.0 / (n_bar - 1.0)) * (p_bar * (1 - p_bar) - ((r - 1.0) / r) * s2 - h_bar / 4.0));
    const double b = n_bar / (n_bar - 1.0) *
                     (p_bar * (1 - p_bar) - ((r - 1.0) / r) * s2 - ((2 * n_bar - 1.0) / (4.0 * n_bar)) * h_bar);
    const double c = h_bar / 2.0;
    num = a;
    den = a + b + c;
  } else {
    // src/pairwise_fst_nei87_loop.cpp:45-80
    const double q1 = 1 - p1, q2 = 1 - p2;
    const double np1 = n1 / 2.0, np2 = n2 / 2.0;
    int valid = 0;
    double nsum = 0.0, inv_nsum = 0.0, ho_sum = 0.0;
    if (np1 == np1) { valid++; ho_sum += h1; nsum += 1.0; inv_nsum += 1.0 / np1; }
    if (np2 == np2) { valid++; ho_sum += h2; nsum += 1.0; inv_nsum += 1.0 / np2; }
    const double np = valid;
    const double mn = (inv_nsum > 0) ? nsum / inv_nsum : TPG_QNAN;
    const double mHo = ho_sum / valid;
    const double sp2a = p1 * p1 + p2 * p2;
    const double sp2r = q1 * q1 + q2 * q2;
    const double sp2 = sp2a + sp2r;
    const double msp2 = sp2 / 2.0;
    const double fAm = (p1 + p2) / 2.0, fRm = (q1 + q2) / 2.0;
    const double mp2 = fAm * fAm + fRm * fRm;
    const double mHs = mn / (mn - 1.0) * (1.0 - msp2 - mHo / (2.0 * mn));
    const double Ht = 1.0 - mp2 + mHs / (mn * np) - mHo / (2.0 * mn * np);
    const double Dst = Ht - mHs;
    const double Dstp = (np / (np - 1.0)) * Dst;
    num = Dstp;
    den = mHs + Dstp;
  }
}

struct FstSrc {
  // either class counts (fused path) ...
  const int32_t* cnt;
  int64_t Mpad;
  int Cpad;
  int has_hap;
  // ... or the reference's m x G matrices (loop mirror)
  const double* n;
  const double* p;
  const double* q;  // freq_ref; only used to honour a caller-supplied matrix in the mirror
  const double* h;
};

// n (valid alleles), freq_alt and het_obs of population g at locus j, as grouped_summaries_dip_pseudo_cpp forms them
// (src/grouped_summaries_dip_pseudo_cpp.cpp:40-56), from the class counts of the fused path or from the caller's matrices
__device__ __forceinline__ void fst_stage(const FstSrc& src, int64_t m, int64_t j, int g, double& vn, double& vp, double& vh) {
  if (src.cnt) {
    const int64_t plane = src.Mpad * src.Cpad;
    if (!src.has_hap) {
      const int64_t o = j * src.Cpad + g;
      const int n1 = src.cnt[o], n2 = src.cnt[plane + o], nv = src.cnt[2 * plane + o];
      vn = (double)(2 * nv);
      vp = (double)(n1 + 2 * n2) / vn;
      vh = (double)(2 * n1) / vn;
    } else {
      const int64_t o = j * src.Cpad + 2 * g;
      const int n1d = src.cnt[o], n2d = src.cnt[plane + o], nvd = src.cnt[2 * plane + o];
      const int n1h = src.cnt[o + 1], n2h = src.cnt[plane + o + 1], nvh = src.cnt[2 * plane + o + 1];
      vn = (double)(2 * nvd + nvh);
      vp = ((double)(n1d + 2 * n2d) + 0.5 * (double)(n1h + 2 * n2h)) / vn;
      vh = (double)(2 * (n1d + n1h)) / vn;
    }
  } else {
    vn = src.n[j + (int64_t)g * m];
    vp = src.p[j + (int64_t)g * m];
    vh = src.h ? src.h[j + (int64_t)g * m] : 0.0;
  }
}
