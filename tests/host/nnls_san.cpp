// The NNLS solver of sNMF (tidypopgen_amd/csrc/host/host_nnls.h) as a stand-alone program for the host sanitizers
// (tests/test_snmf_host.py).  Reads "K nrhs", the K x K matrix (row-major; it is symmetric) and nrhs right-hand sides of K
// doubles, all as hexadecimal bit patterns, from the file named on the command line; pads to the dispatch width of snmf.hip
// (identity in the padding, zero right-hand side); prints per system the contract flag and the bits of x(0 .. K - 1), then
// "ok nnls".  Heap arrays of exactly the sizes read.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host/host_nnls.h"

static double from_bits(uint64_t u) {
  double x;
  memcpy(&x, &u, sizeof x);
  return x;
}
static uint64_t bits(double x) {
  uint64_t u;
  memcpy(&u, &x, sizeof u);
  return u;
}

template <int KT>
static void run(int K, const std::vector<double>& A, const std::vector<double>& B, size_t nrhs) {
  std::vector<double> Ap((size_t)KT * KT);
  for (int k = 0; k < KT; k++)
    for (int l = 0; l < KT; l++) Ap[(size_t)k * KT + l] = k < K && l < K ? A[(size_t)k * K + l] : k == l ? 1.0 : 0.0;
  for (size_t r = 0; r < nrhs; r++) {
    double b[KT], x[KT];
    for (int k = 0; k < KT; k++) b[k] = k < K ? B[r * K + k] : 0.0;
    const bool ok = snmf_nnls<KT>(Ap.data(), b, x);
    printf("x %d", ok ? 1 : 0);
    for (int k = 0; k < K; k++) printf(" %016" PRIx64, bits(x[k]));
    for (int k = K; k < KT; k++)
      if (x[k] != 0.0) printf(" PAD");
    printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 3;
  int K = 0;
  unsigned long long nrhs = 0;
  if (fscanf(f, "%d %llu", &K, &nrhs) != 2 || K < 1 || K > TPG_SNMF_MAX_K) return 4;
  std::vector<double> A((size_t)K * K), B((size_t)nrhs * K);
  uint64_t u;
  for (double& a : A) {
    if (fscanf(f, "%" SCNx64, &u) != 1) return 5;
    a = from_bits(u);
  }
  for (double& b : B) {
    if (fscanf(f, "%" SCNx64, &u) != 1) return 5;
    b = from_bits(u);
  }
  fclose(f);
  const int KT = K <= 4 ? K : K <= 8 ? 8 : 16;
  switch (KT) {
    case 1: run<1>(K, A, B, nrhs); break;
    case 2: run<2>(K, A, B, nrhs); break;
    case 3: run<3>(K, A, B, nrhs); break;
    case 4: run<4>(K, A, B, nrhs); break;
    case 8: run<8>(K, A, B, nrhs); break;
    default: run<16>(K, A, B, nrhs); break;
  }
  printf("ok nnls\n");
  return 0;
}
