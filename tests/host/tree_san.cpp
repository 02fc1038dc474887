// hclust's order (tidypopgen_amd/csrc/host/host_hclust.h) and ape's edge table of a neighbour-joining tree
// (tidypopgen_amd/csrc/host/host_tree.h) as a stand-alone program for the host sanitizers (tests/test_tree_host.py).  Reads cases
// from the file named on the command line: "H n", then n - 1 values of merge_a and n - 1 of merge_b; or "J n", then n - 2 values
// each of join_a, join_b, len_a, len_b and the 3 of last.  Prints per case "refused", or an "order" line, or an "edge" line
// (column-major) and a "length" line, then "ok tree".  Every array is a heap array of exactly the size the header states.
#include <cstdio>
#include <vector>

#include "host/host_hclust.h"
#include "host/host_tree.h"

static bool read_ints(FILE* f, std::vector<int32_t>& v) {
  for (auto& x : v) {
    int t;
    if (fscanf(f, "%d", &t) != 1) return false;
    x = (int32_t)t;
  }
  return true;
}

static bool read_doubles(FILE* f, std::vector<double>& v) {
  for (auto& x : v)
    if (fscanf(f, "%lf", &x) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 3;
  char kind;
  long long n;
  while (fscanf(f, " %c %lld", &kind, &n) == 2) {
    if (n < 1) return 4;
    const char* why = "";
    if (kind == 'H') {
      std::vector<int32_t> ma((size_t)(n - 1)), mb((size_t)(n - 1)), order((size_t)n, -7);
      if (!read_ints(f, ma) || !read_ints(f, mb)) return 5;
      if (host_hclust_order(n, ma.data(), mb.data(), order.data(), &why) != HOST_HCLUST_OK) {
        for (int32_t v : order)
          if (v != -7) return 6;  // a refusal writes nothing
        printf("refused\n");
        continue;
      }
      printf("order");
      for (int32_t v : order) printf(" %d", (int)v);
      printf("\n");
    } else if (kind == 'J') {
      const size_t J = n >= 2 ? (size_t)(n - 2) : 0, E = n >= 2 ? (size_t)(2 * n - 3) : 0;
      std::vector<int32_t> ja(J), jb(J), edge(2 * E, -7);
      std::vector<double> la(J), lb(J), last(3), length(E, -7.0);
      if (!read_ints(f, ja) || !read_ints(f, jb) || !read_doubles(f, la) || !read_doubles(f, lb) || !read_doubles(f, last)) return 5;
      if (host_tree_nj_edges(n, ja.data(), jb.data(), la.data(), lb.data(), last.data(), edge.data(), length.data(), &why) != HOST_TREE_OK) {
        for (int32_t v : edge)
          if (v != -7) return 6;
        for (double v : length)
          if (v != -7.0) return 6;
        printf("refused\n");
        continue;
      }
      printf("edge");
      for (int32_t v : edge) printf(" %d", (int)v);
      printf("\nlength");
      for (double v : length) printf(" %.17g", v);
      printf("\n");
    } else return 7;
  }
  fclose(f);
  printf("ok tree\n");
  return 0;
}
