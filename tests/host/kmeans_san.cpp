// The start rows of the k-means (tidypopgen_amd/csrc/host/host_kmeans.h) as a stand-alone program for the host sanitizers
// (tests/test_kmeans_host.py).  Reads lines "seed n k" (the seed in hexadecimal) from the file named on the command line and
// prints the k rows of each, then "ok kmeans".  The output array is a heap array of exactly k entries.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "host/host_kmeans.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 3;
  uint64_t seed;
  long long n;
  int k;
  std::vector<std::pair<uint64_t, int32_t>> keys;
  while (fscanf(f, "%" SCNx64 " %lld %d", &seed, &n, &k) == 3) {
    if (n < 1 || k < 1 || k > n) return 4;
    std::vector<int32_t> idx((size_t)k);
    host_kmeans_start(seed, n, k, idx.data(), keys);
    printf("start");
    for (int c = 0; c < k; c++) printf(" %d", (int)idx[(size_t)c]);
    printf("\n");
  }
  fclose(f);
  printf("ok kmeans\n");
  return 0;
}
