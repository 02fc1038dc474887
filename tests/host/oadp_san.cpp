// The OADP projection (tidypopgen_amd/csrc/host/host_oadp.h) as a stand-alone program for the host sanitizers
// (tests/test_oadp_host.py): the routine the kernel of oadp.hip runs, with a team of one.  Reads "n K", the K singular values,
// the n x K matrix XV (column-major) and the n squared norms, all as hexadecimal bit patterns, from the file named on the
// command line; prints "rc <code>" (the check of the singular values) and, when it passed, "deg <count>" and "out" with the
// n x K results as bit patterns, then "ok oadp".  Every array is a heap array of exactly the documented size.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host/host_oadp.h"

static bool read_doubles(FILE* f, std::vector<double>& a) {
  for (double& x : a) {
    uint64_t u;
    if (fscanf(f, "%" SCNx64, &u) != 1) return false;
    memcpy(&x, &u, sizeof x);
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 3;
  long long n;
  int K;
  if (fscanf(f, "%lld %d", &n, &K) != 2 || n < 0 || K < 1 || K > HOST_OADP_KMAX) return 4;
  std::vector<double> d((size_t)K), XV((size_t)n * K), nrm((size_t)n), out((size_t)n * K), ws((size_t)host_oadp_ws_doubles(K));
  if (!read_doubles(f, d) || !read_doubles(f, XV) || !read_doubles(f, nrm)) return 5;
  fclose(f);
  const int rc = host_oadp_check_sval(d.data(), K);
  printf("rc %d\n", rc);
  if (rc == 0) {
    const int64_t deg = host_oadp_all(XV.data(), nrm.data(), n, K, d.data(), ws.data(), out.data());
    printf("deg %lld\nout", (long long)deg);
    for (double x : out) {
      uint64_t u;
      memcpy(&u, &x, sizeof u);
      printf(" %016" PRIx64, u);
    }
    printf("\n");
  }
  printf("ok oadp\n");
  return 0;
}
