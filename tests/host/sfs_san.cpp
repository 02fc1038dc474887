// sfs_san.cpp -- the projection row of csrc/host/host_sfs.h, the function sfs_operands_kernel (sfs.hip) calls once per (locus,
// group), as a stand-alone program for the host sanitizers (tests/test_sfs_host.py builds and runs it).  Input: a text file,
// one query "x v n" per line (0 <= x <= v, 1 <= n <= v, v < 2^31, n <= 10^6); output: one line per query, the bits of
// h[0 .. n] as unsigned integers.  The row is written into a heap array of exactly n + 1 doubles, so that a write outside it
// is an error the sanitizer reports.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "host/host_sfs.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  long long x = 0, v = 0, n = 0;
  while (fscanf(f, "%lld %lld %lld", &x, &v, &n) == 3) {
    if (v < 1 || v >= (1ll << 31) || x < 0 || x > v || n < 1 || n > v || n > 1000000) return 3;
    std::vector<double> h((size_t)n + 1, -1.0);
    host_sfs_row((int64_t)x, (int64_t)v, (int64_t)n, HostSfsArray{h.data()});
    for (long long k = 0; k <= n; k++) {
      unsigned long long bits = 0;
      memcpy(&bits, &h[(size_t)k], sizeof(bits));
      printf(k ? " %llu" : "%llu", bits);
    }
    printf("\n");
  }
  fclose(f);
  return 0;
}
