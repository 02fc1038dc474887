// host_fstperm.h -- the host pieces of include/tpg.h "Fst under relabelings": the r-th relabeling of tpg_fst_perm_labels, the
// argument checks of tpg_fst_relabel_sums, and the packing of a batch of label rows into the class columns of the fused kernel
// (fstperm.hip).  Plain C++ with no HIP in it: fstperm.hip calls these very functions, and tests/host/fstperm_san.cpp builds
// the same text under the host sanitizers.
//
// Class packing.  A workgroup of the fused kernel owns HOST_FSTPERM_TILE = 64 class columns (two 32-column MFMA tiles).  A
// relabeling with G groups takes G consecutive columns, a "slot"; a workgroup holds 64 / G slots and the columns behind the
// last whole slot stay empty, so the classes of one relabeling never lie in two workgroups.  Row b of a batch sits in class
// group b / slots, slot b % slots; label l of that row is column slot * G + l of the group.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../synth_common.h"

#define HOST_FSTPERM_MAX_GROUPS 64
#define HOST_FSTPERM_TILE 64

static inline int host_fstperm_slots(int G) { return HOST_FSTPERM_TILE / G; }
static inline int64_t host_fstperm_class_groups(int64_t rows, int G) {
  const int64_t s = host_fstperm_slots(G);
  return (rows + s - 1) / s;
}
// the class (column of the whole batch) of label l of batch row b
static inline int64_t host_fstperm_class(int64_t b, int l, int G) {
  const int64_t s = host_fstperm_slots(G);
  return (b / s) * HOST_FSTPERM_TILE + (b % s) * G + l;
}

// The argument checks of tpg_fst_relabel_sums that need no device: 0 = fine, 1 = a bad argument described in msg.
static inline int host_fstperm_check(int64_t n, const int32_t* labels, int64_t R, int ngroups, const int32_t* pairs1, int P, char* msg,
                                     size_t cap) {
  if (ngroups < 2) { snprintf(msg, cap, "ngroups = %d: a relabeling needs at least two groups", ngroups); return 1; }
  if (ngroups > HOST_FSTPERM_MAX_GROUPS) {
    snprintf(msg, cap, "ngroups = %d exceeds TPG_FSTPERM_MAX_GROUPS = %d (a relabeling's classes live in one workgroup): relabel pair by pair "
             "with the pairwise scheme (two groups per relabeling)", ngroups, HOST_FSTPERM_MAX_GROUPS);
    return 1;
  }
  if (P < 1 || !pairs1) { snprintf(msg, cap, "no population pairs"); return 1; }
  if (R < 0) { snprintf(msg, cap, "R = %lld is negative", (long long)R); return 1; }
  for (int k = 0; k < P; k++) {
    const int g1 = pairs1[2 * k], g2 = pairs1[2 * k + 1];
    if (g1 < 1 || g1 > ngroups || g2 < 1 || g2 > ngroups) {
      snprintf(msg, cap, "pair %d = (%d, %d) out of [1,%d]", k, g1, g2, ngroups);
      return 1;
    }
    if (g1 == g2) { snprintf(msg, cap, "pair %d names group %d twice", k, g1); return 1; }
  }
  if (R > 0 && !labels) { snprintf(msg, cap, "null argument"); return 1; }
  for (int64_t r = 0; r < R; r++)
    for (int64_t i = 0; i < n; i++) {
      const int32_t l = labels[r * n + i];
      if (l < -1 || l >= ngroups) {
        snprintf(msg, cap, "labels[%lld][%lld] = %d out of [-1,%d)", (long long)r, (long long)i, l, ngroups);
        return 1;
      }
    }
  return 0;
}

// `rows` checked label rows -> lab8 (rows x n bytes, the label as a signed byte) and csize (class_groups x 64 class sizes)
static inline void host_fstperm_pack(int64_t n, const int32_t* labels, int64_t rows, int G, int8_t* lab8, int32_t* csize) {
  const int64_t ncls = host_fstperm_class_groups(rows, G) * HOST_FSTPERM_TILE;
  for (int64_t c = 0; c < ncls; c++) csize[c] = 0;
  for (int64_t b = 0; b < rows; b++)
    for (int64_t i = 0; i < n; i++) {
      const int32_t l = labels[b * n + i];
      lab8[b * n + i] = (int8_t)l;
      if (l >= 0) csize[host_fstperm_class(b, l, G)]++;
    }
}

// The r-th relabeling (include/tpg.h): 0 = fine, 1 = a bad argument described in msg.  a and b are 0-based group ids (scheme 0).
static inline int host_fstperm_labels(int64_t n, const int32_t* groupIds0, int ngroups, int scheme, int a, int b, uint64_t seed, int64_t r,
                                      int32_t* out, char* msg, size_t cap) {
  if (n < 0 || (n > 0 && (!groupIds0 || !out))) { snprintf(msg, cap, "null argument"); return 1; }
  if (ngroups < 1) { snprintf(msg, cap, "ngroups must be positive"); return 1; }
  if (scheme != 0 && scheme != 1) { snprintf(msg, cap, "scheme = %d: 0 (pairwise) or 1 (global)", scheme); return 1; }
  if (r < 0 || r >= ((int64_t)1 << 31)) { snprintf(msg, cap, "r = %lld out of [0, 2^31)", (long long)r); return 1; }
  if (n >= ((int64_t)1 << 31)) { snprintf(msg, cap, "n = %lld: at most 2^31 - 1 individuals", (long long)n); return 1; }
  if (scheme == 0 && (a < 0 || a >= ngroups || b < 0 || b >= ngroups || a == b)) {
    snprintf(msg, cap, "groups a = %d, b = %d: two different ids in [0,%d)", a, b, ngroups);
    return 1;
  }
  for (int64_t i = 0; i < n; i++)
    if (groupIds0[i] < 0 || groupIds0[i] >= ngroups) {
      snprintf(msg, cap, "groupIds[%lld] = %d out of [0,%d)", (long long)i, groupIds0[i], ngroups);
      return 1;
    }
  auto label = [&](int32_t g) -> int32_t { return scheme == 1 ? g : g == a ? 0 : g == b ? 1 : -1; };
  std::vector<std::pair<uint64_t, int64_t>> keys;  // (key, index) of the eligible set, in ascending index
  for (int64_t i = 0; i < n; i++) {
    out[i] = label(groupIds0[i]);
    if (out[i] >= 0 && r > 0) keys.push_back({tpg_mix64(seed ^ tpg_mix64(((uint64_t)r << 32) + (uint64_t)i)), i});
  }
  if (r == 0) return 0;  // the identity, not hashed
  std::vector<int64_t> e(keys.size());
  for (size_t t = 0; t < keys.size(); t++) e[t] = keys[t].second;
  std::sort(keys.begin(), keys.end());  // by key, then by index
  for (size_t t = 0; t < keys.size(); t++) out[keys[t].second] = label(groupIds0[e[t]]);
  return 0;
}
