// host_ldstat.h -- the per-pair pieces of include/tpg.h "LD statistics", written once for the host and the device: r2 of a pair
// of loci from its integer sums, the fixed-point value q every sum of r2 is made of, and the distance bin.  The epilogue of
// tpg_ldstat_kernel (ldstat.hip) calls these very functions; the stand-alone program of tests/host/ldstat_san.cpp runs them
// under the host sanitizers.  Whoever includes this header compiles without FMA contraction (-ffp-contract=off).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TPG_LDSTAT_FN __host__ __device__ static inline
#else
#define TPG_LDSTAT_FN static inline
#endif

#define HOST_LDSTAT_ONE 1073741824.0  // 2^30
#define HOST_LDSTAT_MAX_BINS 4096

// r2 = (dn * dn) / (d_j * d_k) with dn = (double)(n Sxy - Sx_j Sx_k): three IEEE double operations in this order, the
// expression of "LD-kNN imputation", step 1.  n < 2^22, so n, Sxy <= 4 n and Sx <= 2 n are 32-bit values and num is two
// 32 x 32 -> 64 bit products.  The caller has seen d_j > 0 and d_k > 0.
TPG_LDSTAT_FN double host_ldstat_r2(int32_t n, int32_t sxy, int32_t sxj, int32_t sxk, double dj, double dk) {
  const int64_t num = (int64_t)n * sxy - (int64_t)sxj * sxk;
  const double dn = (double)num;
  const double sq = dn * dn;
  const double den = dj * dk;
  return sq / den;
}

// q = floor(r2 * 2^30 + 0.5): the product is exact, the sum is one IEEE addition.  num^2 <= d_j d_k (Cauchy-Schwarz), so r2 is
// at most 1 up to its roundings and the sum lies below 2^31: its floor is the conversion to a 32-bit unsigned integer.
TPG_LDSTAT_FN uint64_t host_ldstat_q(double r2) {
  const double x = r2 * HOST_LDSTAT_ONE;
  const double y = x + 0.5;
  return (uint64_t)(uint32_t)y;
}

// The bin of a pair: dist / bin_size by integer division if that is below nbins, else nbins ("beyond"); dist >= 0, bin_size >= 1,
// 1 <= nbins <= HOST_LDSTAT_MAX_BINS.  One 32-bit division where both fit.  Otherwise the quotient is built from its bit 12
// downwards by subtraction, which leaves min(quotient, 8191): no product that could overflow, and no 64-bit division, which is
// a routine of some 150 instructions on the device at each of the 64 places the epilogue would inline it.
TPG_LDSTAT_FN int host_ldstat_bin(int64_t dist, int64_t bin_size, int nbins) {
  if ((((uint64_t)dist | (uint64_t)bin_size) >> 32) == 0) {
    const uint32_t b = (uint32_t)dist / (uint32_t)bin_size;
    return b < (uint32_t)nbins ? (int)b : nbins;
  }
  int64_t rem = dist;
  int b = 0;
#pragma nounroll
  for (int s = 12; s >= 0; s--) {
    if (bin_size > (INT64_MAX >> s)) continue;  // bin_size << s is beyond every distance
    const int64_t step = bin_size << s;
    if (rem >= step) {
      rem -= step;
      b += 1 << s;
    }
  }
  return b < nbins ? b : nbins;
}
