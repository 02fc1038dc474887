// The host half of PC-Relate (tidypopgen_amd/csrc/host/host_pcrelate.h) as a stand-alone program for the host sanitizers
// (tests/test_pcrelate_host.py): the basis of step 0 and the pinned expressions of step 2 that the kernel of pcrelate.hip
// evaluates.  Reads "n K m" and the n x K matrix V (column-major, hexadecimal bit patterns) from the file named on the command
// line; prints "rc <code>" of the basis (1: the arguments, 2: rank deficient) and, when it is 0, "Q" with the n x (K + 1) basis.
// With m > 0 the file goes on with thr, mean[m], c (m x (K + 1)) as bit patterns and the n x m codes (decimal, column-major); the
// program then prints "mu", "valid" (0 / 1), "R" and "S" of every cell, column-major.  The last line is "ok pcrelate".  Every
// array is a heap array of exactly the documented size.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host/host_pcrelate.h"

static bool read_doubles(FILE* f, std::vector<double>& a) {
  for (double& x : a) {
    uint64_t u;
    if (fscanf(f, "%" SCNx64, &u) != 1) return false;
    memcpy(&x, &u, sizeof x);
  }
  return true;
}

static void print_doubles(const char* name, const std::vector<double>& a) {
  printf("%s", name);
  for (double x : a) {
    uint64_t u;
    memcpy(&u, &x, sizeof u);
    printf(" %016" PRIx64, u);
  }
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 3;
  long long n, m;
  int K;
  if (fscanf(f, "%lld %d %lld", &n, &K, &m) != 3 || n < 0 || m < 0) return 4;
  if (K < 0 || K > HOST_PCRELATE_MAX_K || n < K + 2) {
    // the routine refuses these before it reads V: hand it no array at all
    const int rc = host_pcrelate_basis(nullptr, n, K, nullptr);
    fclose(f);
    printf("rc %d\nok pcrelate\n", rc);
    return 0;
  }
  const int L = K + 1;
  std::vector<double> V((size_t)n * K), Q((size_t)n * L);
  if (!read_doubles(f, V)) return 5;
  const int rc = host_pcrelate_basis(V.data(), n, K, Q.data());
  printf("rc %d\n", rc);
  if (rc == 0) {
    print_doubles("Q", Q);
    if (m > 0) {
      std::vector<double> thr(1), mean((size_t)m), c((size_t)m * L);
      std::vector<int> codes((size_t)n * m);
      if (!read_doubles(f, thr) || !read_doubles(f, mean) || !read_doubles(f, c)) return 6;
      for (int& g : codes)
        if (fscanf(f, "%d", &g) != 1 || g < 0 || g > 3) return 7;
      const double hi = 1.0 - thr[0];
      std::vector<double> mu((size_t)n * m), R((size_t)n * m), S((size_t)n * m);
      std::vector<int> valid((size_t)n * m);
      for (long long j = 0; j < m; j++)
        for (long long i = 0; i < n; i++) {
          const size_t at = (size_t)(i + j * n);
          mu[at] = host_pcrelate_mu(mean[(size_t)j], Q.data() + i, n, c.data() + j, m, L);
          valid[at] = host_pcrelate_valid(codes[at], mu[at], thr[0], hi) ? 1 : 0;
          R[at] = valid[at] ? host_pcrelate_r(codes[at], mu[at]) : 0.0;
          S[at] = valid[at] ? host_pcrelate_s(mu[at]) : 0.0;
        }
      print_doubles("mu", mu);
      printf("valid");
      for (int b : valid) printf(" %d", b);
      printf("\n");
      print_doubles("R", R);
      print_doubles("S", S);
    }
  }
  fclose(f);
  printf("ok pcrelate\n");
  return 0;
}
