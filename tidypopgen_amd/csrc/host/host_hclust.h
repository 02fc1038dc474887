// host_hclust.h -- the host side of include/tpg.h "Ward clustering on PCA scores": the cut of a merge list at k clusters and the
// merge matrix in R's convention.  Plain C++ with no HIP in it: hclust.hip wraps it for the C ABI and tests/host/hclust_san.cpp
// builds the same text under the host sanitizers.
#pragma once
#include <stdint.h>

#include <vector>

enum { HOST_HCLUST_OK = 0, HOST_HCLUST_EINVAL = 1 };

// every step names two live slots a < b inside [0, n); b is dead afterwards
static inline int host_hclust_check(int64_t n, const int32_t* merge_a, const int32_t* merge_b, const char** why) {
  std::vector<uint8_t> live((size_t)n, 1);
  for (int64_t s = 0; s + 1 < n; s++) {
    const int64_t a = merge_a[s], b = merge_b[s];
    if (a < 0 || b >= n || a >= b) {
      *why = "a merge step does not name two slots a < b inside [0, n)";
      return HOST_HCLUST_EINVAL;
    }
    if (!live[(size_t)a] || !live[(size_t)b]) {
      *why = "a merge step names a slot that an earlier step has merged away";
      return HOST_HCLUST_EINVAL;
    }
    live[(size_t)b] = 0;
  }
  return HOST_HCLUST_OK;
}

// labels n x R column-major, 0-based: column r applies the first n - k[r] merges and numbers the clusters in the order in which
// they first appear in ascending i (a cluster's slot is its smallest member, so this is the rank of the slot).  Nothing is
// written unless every argument passes.
static inline int host_hclust_cut(int64_t n, const int32_t* merge_a, const int32_t* merge_b, int R, const int32_t* k, int32_t* labels,
                                  const char** why) {
  if (n < 1 || R < 0) {
    *why = "n < 1 or R < 0";
    return HOST_HCLUST_EINVAL;
  }
  for (int r = 0; r < R; r++)
    if (k[r] < 1 || k[r] > n) {
      *why = "a k outside [1, n]";
      return HOST_HCLUST_EINVAL;
    }
  const int rc = host_hclust_check(n, merge_a, merge_b, why);
  if (rc != HOST_HCLUST_OK) return rc;
  std::vector<int32_t> slot((size_t)n), number((size_t)n);
  for (int r = 0; r < R; r++) {
    for (int64_t i = 0; i < n; i++) slot[(size_t)i] = (int32_t)i;
    // b > a always, and a slot only ever points at a smaller one: one ascending pass resolves every chain
    for (int64_t s = 0; s < n - k[r]; s++) slot[(size_t)merge_b[s]] = merge_a[s];
    int32_t next = 0;
    int32_t* out = labels + (size_t)r * (size_t)n;
    for (int64_t i = 0; i < n; i++) {
      if (slot[(size_t)i] == i) number[(size_t)i] = next++;
      else slot[(size_t)i] = slot[(size_t)slot[(size_t)i]];  // (its target is resolved already: it is smaller than i)
      out[i] = number[(size_t)slot[(size_t)i]];
    }
  }
  return HOST_HCLUST_OK;
}

// merge (n - 1) x 2 column-major as R's hclust$merge: -(i + 1) for the point i on its own, the 1-based step that formed it for a
// cluster; a singleton before a cluster; of two singletons the smaller point first, of two clusters the earlier step first.
static inline int host_hclust_r_merge(int64_t n, const int32_t* merge_a, const int32_t* merge_b, int32_t* merge, const char** why) {
  if (n < 1) {
    *why = "n < 1";
    return HOST_HCLUST_EINVAL;
  }
  const int rc = host_hclust_check(n, merge_a, merge_b, why);
  if (rc != HOST_HCLUST_OK) return rc;
  std::vector<int32_t> id((size_t)n);
  for (int64_t i = 0; i < n; i++) id[(size_t)i] = -(int32_t)(i + 1);
  const int64_t rows = n - 1;
  for (int64_t s = 0; s < rows; s++) {
    int32_t u = id[(size_t)merge_a[s]], v = id[(size_t)merge_b[s]];
    if ((u > 0 && v < 0) || (u > 0 && v > 0 && v < u)) {
      const int32_t t = u;
      u = v, v = t;
    }
    merge[s] = u;
    merge[rows + s] = v;
    id[(size_t)merge_a[s]] = (int32_t)(s + 1);
  }
  return HOST_HCLUST_OK;
}

// order[n], 0-based, as R's hclust$order (recalled from hcass2, not pinned): with R's merge matrix above, the leaves of a row are
// the leaves of its first column followed by those of its second, a negative entry is that single point, and order is the leaves
// of the last row.  n = 1 gives [0].  Nothing is written unless the merge list passes host_hclust_check.
static inline int host_hclust_order(int64_t n, const int32_t* merge_a, const int32_t* merge_b, int32_t* order, const char** why) {
  if (n < 1) {
    *why = "n < 1";
    return HOST_HCLUST_EINVAL;
  }
  const int64_t rows = n - 1;
  std::vector<int32_t> merge((size_t)(2 * rows));
  const int rc = host_hclust_r_merge(n, merge_a, merge_b, merge.data(), why);
  if (rc != HOST_HCLUST_OK) return rc;
  if (n == 1) {
    order[0] = 0;
    return HOST_HCLUST_OK;
  }
  // a stack in place of the recursion (a chain of n - 1 merges is n - 1 deep): the second column goes on first, so the first
  // comes off first
  std::vector<int32_t> todo;
  todo.push_back((int32_t)rows);
  int64_t at = 0;
  while (!todo.empty()) {
    const int32_t e = todo.back();
    todo.pop_back();
    if (e < 0) order[at++] = -e - 1;
    else {
      todo.push_back(merge[(size_t)(rows + e - 1)]);
      todo.push_back(merge[(size_t)(e - 1)]);
    }
  }
  return HOST_HCLUST_OK;
}
