// host_kmeans.h -- the start rows of include/tpg.h "k-means on PCA scores": the k rows with the smallest (h_i, i),
// h_i = M(seed ^ M(i)), in that order.  Plain C++ with no HIP in it: kmeans.hip calls it once per run of a batch and
// tests/host/kmeans_san.cpp builds the same text under the host sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../synth_common.h"

// idx[0 .. k-1]; 1 <= k <= n.  `keys` is scratch the caller may keep between calls (one allocation per batch, not per run)
static inline void host_kmeans_start(uint64_t seed, int64_t n, int k, int32_t* idx, std::vector<std::pair<uint64_t, int32_t>>& keys) {
  keys.resize((size_t)n);
  for (int64_t i = 0; i < n; i++) keys[(size_t)i] = {tpg_mix64(seed ^ tpg_mix64((uint64_t)i)), (int32_t)i};
  // (a pair compares by the hash first, then by the row: the order of the header)
  std::partial_sort(keys.begin(), keys.begin() + k, keys.end());
  for (int c = 0; c < k; c++) idx[c] = keys[(size_t)c].second;
}
