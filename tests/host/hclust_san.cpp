// The cut and R's merge matrix of the Ward tree (tidypopgen_amd/csrc/host/host_hclust.h) as a stand-alone program for the host
// sanitizers (tests/test_hclust_host.py).  Reads cases from the file named on the command line: "n R", then R values of k, then
// n - 1 values of merge_a, then n - 1 of merge_b.  Prints per case either "refused", or one "labels" line per k and one "merge"
// line (column-major), then "ok hclust".  Every array is a heap array of exactly the size the header states.
#include <cstdio>
#include <vector>

#include "host/host_hclust.h"

static bool read_ints(FILE* f, std::vector<int32_t>& v) {
  for (auto& x : v) {
    int t;
    if (fscanf(f, "%d", &t) != 1) return false;
    x = (int32_t)t;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 3;
  long long n;
  int R;
  while (fscanf(f, "%lld %d", &n, &R) == 2) {
    if (n < 1 || R < 0) return 4;
    std::vector<int32_t> k((size_t)R), ma((size_t)(n - 1)), mb((size_t)(n - 1));
    if (!read_ints(f, k) || !read_ints(f, ma) || !read_ints(f, mb)) return 5;
    std::vector<int32_t> labels((size_t)n * (size_t)R, -7), merge((size_t)(2 * (n - 1)), -7);
    const char* why = "";
    const int rc = host_hclust_cut(n, ma.data(), mb.data(), R, k.data(), labels.data(), &why);
    const int rm = host_hclust_r_merge(n, ma.data(), mb.data(), merge.data(), &why);
    if (rc != HOST_HCLUST_OK || rm != HOST_HCLUST_OK) {
      // a refusal writes nothing
      for (int32_t v : labels)
        if (v != -7) return 6;
      for (int32_t v : merge)
        if (v != -7) return 6;
      printf("refused %d %d\n", rc, rm);
      continue;
    }
    for (int r = 0; r < R; r++) {
      printf("labels");
      for (long long i = 0; i < n; i++) printf(" %d", (int)labels[(size_t)r * (size_t)n + (size_t)i]);
      printf("\n");
    }
    printf("merge");
    for (int32_t v : merge) printf(" %d", (int)v);
    printf("\n");
  }
  fclose(f);
  printf("ok hclust\n");
  return 0;
}
