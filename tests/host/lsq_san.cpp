// The solve of the least-squares projection (tidypopgen_amd/csrc/host/host_lsq.h) as a stand-alone program for the host
// sanitizers (tests/test_lsq_host.py): the routine the kernel of lsq.hip runs, with a team of one.  Reads "n L", the n x P packed
// matrix A (P = L (L + 1) / 2) and the n x L matrix b (column-major, hexadecimal bit patterns) and the n typed counts (decimal)
// from the file named on the command line; prints "rc <code>" (2: L outside [1, 32], before anything else is read; 1: a value
// of A or b that is not finite) and, when it is 0, "sing <count>" and "out" with the n x L results as bit patterns, then
// "ok lsq".  Every array is a heap array of exactly the documented size.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host/host_lsq.h"

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
  int L;
  if (fscanf(f, "%lld %d", &n, &L) != 2 || n < 0) return 4;
  if (L < 1 || L > HOST_LSQ_MAX_L) {
    fclose(f);
    printf("rc 2\nok lsq\n");
    return 0;
  }
  const size_t P = (size_t)host_lsq_pairs(L);
  std::vector<double> A((size_t)n * P), b((size_t)n * L), out((size_t)n * L), ws((size_t)host_lsq_ws_doubles(L));
  std::vector<int64_t> nt((size_t)n);
  if (!read_doubles(f, A) || !read_doubles(f, b)) return 5;
  for (int64_t& t : nt) {
    long long v;
    if (fscanf(f, "%lld", &v) != 1) return 6;
    t = v;
  }
  fclose(f);
  const int rc = host_lsq_check(A.data(), b.data(), n, L);
  printf("rc %d\n", rc);
  if (rc == 0) {
    const int64_t sing = host_lsq_all(A.data(), b.data(), nt.data(), n, L, ws.data(), out.data());
    printf("sing %lld\nout", (long long)sing);
    for (double x : out) {
      uint64_t u;
      memcpy(&u, &x, sizeof u);
      printf(" %016" PRIx64, u);
    }
    printf("\n");
  }
  printf("ok lsq\n");
  return 0;
}
