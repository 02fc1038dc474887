// host_tree.h -- the host side of include/tpg.h "Trees from a pairwise matrix": the join list of tpg_nj as an edge table in
// ape's phylo layout.  Plain C++ with no HIP in it: tree.hip wraps it for the C ABI and tests/host/tree_san.cpp builds the same
// text under the host sanitizers.
#pragma once
#include <stdint.h>

#include <vector>

enum { HOST_TREE_OK = 0, HOST_TREE_EINVAL = 1 };

// every join names two live slots a < b inside [0, n), b is dead afterwards, and last[0] < last[1] are the two slots left
static inline int host_tree_check_joins(int64_t n, const int32_t* join_a, const int32_t* join_b, const double* last, const char** why) {
  std::vector<uint8_t> live((size_t)n, 1);
  for (int64_t s = 0; s + 2 < n; s++) {
    const int64_t a = join_a[s], b = join_b[s];
    if (a < 0 || b >= n || a >= b) {
      *why = "a join does not name two slots a < b inside [0, n)";
      return HOST_TREE_EINVAL;
    }
    if (!live[(size_t)a] || !live[(size_t)b]) {
      *why = "a join names a slot that an earlier join has taken";
      return HOST_TREE_EINVAL;
    }
    live[(size_t)b] = 0;
  }
  int64_t left[2], found = 0;
  for (int64_t i = 0; i < n; i++)
    if (live[(size_t)i] && found < 2) left[found++] = i;
  if (found != 2 || !(last[0] == (double)left[0]) || !(last[1] == (double)left[1])) {
    *why = "last does not name the two slots that the joins leave";
    return HOST_TREE_EINVAL;
  }
  return HOST_TREE_OK;
}

// edge (2n - 3) x 2 int32 column-major (parent, child) and edge_length[2n - 3], ape's phylo layout (recalled, not pinned): tips
// 1 .. n, the node of join s is 2n - 2 - s, so the last join is the root n + 1 and Nnode = n - 2; the root's children are its
// a-child, its b-child and the node of the other slot left, at length last[2]; preorder from the root, a-child before b-child
// before the third.  n >= 3.  Nothing is written unless every argument passes.
static inline int host_tree_nj_edges(int64_t n, const int32_t* join_a, const int32_t* join_b, const double* len_a, const double* len_b,
                                     const double* last, int32_t* edge, double* edge_length, const char** why) {
  if (n < 3 || n > (int64_t)1 << 29) {
    *why = "n < 3 (a tree of two tips has no join) or too large for int32 node numbers";
    return HOST_TREE_EINVAL;
  }
  const int rc = host_tree_check_joins(n, join_a, join_b, last, why);
  if (rc != HOST_TREE_OK) return rc;
  const int64_t J = n - 2, E = 2 * n - 3;
  // node[slot]: what the slot holds now; kid[2 s], kid[2 s + 1]: the children of join s
  std::vector<int32_t> node((size_t)n), kid((size_t)(2 * J));
  for (int64_t i = 0; i < n; i++) node[(size_t)i] = (int32_t)(i + 1);
  for (int64_t s = 0; s < J; s++) {
    kid[(size_t)(2 * s)] = node[(size_t)join_a[s]];
    kid[(size_t)(2 * s + 1)] = node[(size_t)join_b[s]];
    node[(size_t)join_a[s]] = (int32_t)(2 * n - 2 - s);
  }
  const int64_t x = (int64_t)last[0], y = (int64_t)last[1];
  const int32_t root = (int32_t)(n + 1);
  if (node[(size_t)x] != root && node[(size_t)y] != root) {  // (cannot happen after the check: the last join's slot survives)
    *why = "neither slot left holds the last join";
    return HOST_TREE_EINVAL;
  }
  const int32_t third = node[(size_t)x] == root ? node[(size_t)y] : node[(size_t)x];
  struct Item {
    int32_t parent, child;
    double len;
  };
  // a stack in place of the recursion: children go on in reverse, so the a-child comes off first
  std::vector<Item> todo;
  todo.push_back({root, third, last[2]});
  todo.push_back({root, kid[(size_t)(2 * (J - 1) + 1)], len_b[J - 1]});
  todo.push_back({root, kid[(size_t)(2 * (J - 1))], len_a[J - 1]});
  int64_t at = 0;
  while (!todo.empty()) {
    const Item e = todo.back();
    todo.pop_back();
    edge[at] = e.parent, edge[E + at] = e.child, edge_length[at] = e.len;
    at++;
    if (e.child > n) {
      const int64_t s = 2 * n - 2 - e.child;
      todo.push_back({e.child, kid[(size_t)(2 * s + 1)], len_b[s]});
      todo.push_back({e.child, kid[(size_t)(2 * s)], len_a[s]});
    }
  }
  return HOST_TREE_OK;
}
