// host_knnimp.h -- the integer pieces of include/tpg.h "LD-kNN imputation" that the vote kernel (knnimp.hip) runs per pair of
// individuals and per missing entry, written once for the host and the device: the stand-alone program of
// tests/host/knnimp_san.cpp runs the very functions the kernel calls.
//
// Profile of an individual over the l_j <= 32 neighbour loci of a locus: a 64-bit THERMOMETER word (locus t in bits 2 t and
// 2 t + 1: genotype 0 -> 00, 1 -> 01, 2 -> 11, missing -> 00) and a 32-bit MISSING mask (bit t).  For two typed genotypes
// |x - y| is the number of thermometer bits that differ; a locus where either is missing costs 1.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TPG_KNN_FN __host__ __device__ static inline
#else
#define TPG_KNN_FN static inline
#endif

#define HOST_KNN_MAX_L 32
#define HOST_KNN_DISTS (2 * HOST_KNN_MAX_L + 1)  // distances 0 .. 64
#define HOST_KNN_HIST (3 * HOST_KNN_DISTS)       // hist[dist * 3 + g]
#define HOST_KNN_WEIGHT_ONE (1ll << 24)

// bit t of the 16-bit m -> bits 2 t and 2 t + 1
TPG_KNN_FN uint32_t host_knn_spread16(uint32_t x) {
  x = (x | (x << 8)) & 0x00FF00FFu;
  x = (x | (x << 4)) & 0x0F0F0F0Fu;
  x = (x | (x << 2)) & 0x33333333u;
  x = (x | (x << 1)) & 0x55555555u;
  return x | (x << 1);
}
// the same for 32 bits, as two halves: 32-bit shifts only (a 64-bit shift runs at a quarter of the rate on the device)
TPG_KNN_FN uint64_t host_knn_spread(uint32_t m) {
  return ((uint64_t)host_knn_spread16(m >> 16) << 32) | host_knn_spread16(m & 0xFFFFu);
}

// code (0, 1, 2, 3 = missing) of neighbour locus t goes into the profile
TPG_KNN_FN void host_knn_profile_add(uint64_t* th, uint32_t* ms, int t, int code) {
  if (code == 3) *ms |= (uint32_t)1 << t;
  else *th |= (uint64_t)(code | (code >> 1)) << (2 * t);
}

// D = sum_t c(x_t, y_t), c = |x - y| if both are typed, else 1
TPG_KNN_FN int host_knn_dist(uint64_t th_a, uint32_t ms_a, uint64_t th_b, uint32_t ms_b) {
  const uint32_t M = ms_a | ms_b;
  return __builtin_popcountll((th_a ^ th_b) & ~host_knn_spread(M)) + __builtin_popcount(M);
}

// The walk over hist[dist * 3 + g], dist < ndist: T voters in all (the caller's sum of hist; T = 0 leaves the entry missing:
// 3).  d* = the smallest distance at which min(k, T) voters are reached, the whole boundary distance takes part; genotype g
// scores s_g = sum_{dist <= d*} hist[dist][g] * (2^24 / (1 + dist)) (integer division, int64); the largest score wins, the
// smaller genotype on a tie.
TPG_KNN_FN int host_knn_vote(const int32_t* hist, int ndist, int64_t k, int64_t T) {
  if (T <= 0) return 3;
  const int64_t need = k < T ? k : T;
  int64_t cum = 0, s[3] = {0, 0, 0};
  for (int d = 0; d < ndist; d++) {
    const int64_t w = HOST_KNN_WEIGHT_ONE / (1 + d);
    for (int g = 0; g < 3; g++) {
      cum += hist[3 * d + g];
      s[g] += (int64_t)hist[3 * d + g] * w;
    }
    if (cum >= need) break;
  }
  int best = 0;
  if (s[1] > s[best]) best = 1;
  if (s[2] > s[best]) best = 2;
  return best;
}
