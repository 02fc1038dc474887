// host_sfs.h -- the projection row of include/tpg.h "site frequency spectra", written once for the host and the device: the
// hypergeometric weights h(k) = C(x,k) C(v-x,n-k) / C(v,n), k = 0 .. n.  sfs_operands_kernel (sfs.hip) calls this very function
// once per (locus, group); tpg_sfs_project_row and the stand-alone program of tests/host/sfs_san.cpp run it on the host.
// Whoever includes this header compiles without FMA contraction (-ffp-contract=off).
//
// Evaluation order (pinned; the bound below counts its roundings, u = 2^-53):
//   support   kmin = max(0, n - (v - x)), kmax = min(n, x); every k outside it gets the double +0.0.
//   mode      k0 = floor((x + 1)(n + 1) / (v + 2)) clamped to the support; w(k0) = 1.0.
//   upwards   w(k + 1) = w(k) * ((double)((x - k)(n - k)) / (double)((k + 1)(v - x - n + k + 1))),  k = k0 .. kmax - 1
//   downwards w(k - 1) = w(k) * ((double)(k (v - x - n + k)) / (double)((x - k + 1)(n - k + 1))),  k = k0 .. kmin + 1
//             the integer products are formed in int64 (x, v < 2^31: below 2^62, exact) and converted once each.
//   sum       s = w(kmin) + w(kmin + 1) + ... + w(kmax), added in ascending k from +0.0.
//   result    h(k) = w(k) / s.
// w(k0) = 1 is the largest weight (the ratios are those of neighbouring hypergeometric terms, and k0 is a mode), so every w is
// in (0, 1], 1 <= s <= n + 1, nothing overflows, and s is never an underflowed value.  With v = n the support is the single
// k = x: w = 1, s = 1, h(x) = 1.0 with no rounding -- the row is exactly the indicator.
// Bound.  A step of a recurrence is at most four roundings (two conversions, the division, the product): w(k) carries at most
// 4 |k - k0| <= 4 n.  s is a sum of at most n + 1 non-negative terms, each within 4 n roundings, through at most n additions:
// 5 n.  The last division adds one.  So where the exact h(k) is at least 2^-1000,
//     |h(k) - exact| <= HOST_SFS_ENTRY_ROUNDINGS(n) u exact,    HOST_SFS_ENTRY_ROUNDINGS(n) = 9 n + 4
// (9 n + 1 roundings; the three spare ones cover the second-order terms for every n <= 2^30).  Below 2^-1000 the weights of the
// recurrence may have passed through the subnormal range, where a rounding is absolute (2^-1075): such an entry is a
// non-negative double below 2^-999, possibly +0.0, and has no relative bound.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TPG_SFS_FN __host__ __device__ static inline
#else
#define TPG_SFS_FN static inline
#endif

#define HOST_SFS_ENTRY_ROUNDINGS(n) (9 * (int64_t)(n) + 4)

// at(k) is the place of h(k), k = 0 .. n: a plain array on the host (HostSfsArray), a fragment address on the device.
// 0 <= x <= v, 1 <= n <= v, v < 2^31.
struct HostSfsArray {
  double* p;
#if defined(__HIPCC__)
  __host__ __device__
#endif
  double& operator()(int64_t k) const { return p[k]; }
};
template <class At>
TPG_SFS_FN void host_sfs_row(int64_t x, int64_t v, int64_t n, const At& at) {
  const int64_t y = v - x;
  const int64_t kmin = n - y > 0 ? n - y : 0, kmax = n < x ? n : x;
  for (int64_t k = 0; k < kmin; k++) at(k) = 0.0;
  for (int64_t k = kmax + 1; k <= n; k++) at(k) = 0.0;
  int64_t k0 = ((x + 1) * (n + 1)) / (v + 2);
  k0 = k0 < kmin ? kmin : k0 > kmax ? kmax : k0;
  at(k0) = 1.0;
  double w = 1.0;
  for (int64_t k = k0; k < kmax; k++) {
    const double num = (double)((x - k) * (n - k)), den = (double)((k + 1) * (y - n + k + 1));
    const double r = num / den;
    w = w * r;
    at((k + 1)) = w;
  }
  w = 1.0;
  for (int64_t k = k0; k > kmin; k--) {
    const double num = (double)(k * (y - n + k)), den = (double)((x - k + 1) * (n - k + 1));
    const double r = num / den;
    w = w * r;
    at((k - 1)) = w;
  }
  double s = 0.0;
  for (int64_t k = kmin; k <= kmax; k++) s = s + at(k);
  for (int64_t k = kmin; k <= kmax; k++) at(k) = at(k) / s;
}
