// The host pieces of the pcadapt scan (tidypopgen_amd/csrc/host/host_pcadapt.h) as a stand-alone program for the host
// sanitizers (tests/test_pcadapt_host.py): log Q at the points of the test, the chi-square median for every K, and the host glue
// of one OGK step (R from the pairwise MADs, its eigenvectors, the map back) on heap arrays of exactly the sizes the functions
// are told.  Prints the bits of every result for the test to compare, then "ok pcadapt".
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#define TPG_HOST_NO_CLONES 1  // one plain build of the QL (function multiversioning and sanitizers do not mix everywhere)
#include "host/host_pcadapt.h"

static uint64_t bits(double x) {
  uint64_t u;
  memcpy(&u, &x, sizeof u);
  return u;
}

int main() {
  // log Q(K / 2, x / 2): chi-square arguments around both ends and the switch between series and continued fraction
  const int Ks[6] = {1, 3, 21, 2, 20, 64};
  for (int K : Ks) {
    const double sw = (double)K + 2.0;  // x / 2 = a + 1
    std::vector<double> xs = {0.0, 1e-300, 1e-8, (double)K, nextafter(sw, 0.0), sw, nextafter(sw, 1e9), 50.0, 700.0, 1500.0, 1e4, 1e6};
    const double a = 0.5 * K, lga = lgamma(a);
    for (double x : xs) {
      const double v = tpg_logq(a, lga, x / 2);
      if (!(v <= 0.0)) return 1;
      printf("logq %d %016" PRIx64 " %016" PRIx64 "\n", K, bits(x), bits(v));
    }
    if (tpg_logq(a, lga, -1.0) == tpg_logq(a, lga, -1.0)) return 2;       // NaN
    if (tpg_logq(a, lga, NAN) == tpg_logq(a, lga, NAN)) return 3;         // NaN
    if (tpg_logq(a, lga, INFINITY) != -INFINITY) return 4;
  }
  for (int K = 1; K <= 64; K++) printf("q50 %d %016" PRIx64 "\n", K, bits(host_qchisq_median(K)));

  // the OGK glue for K = 1, 3 and 5: pairwise MADs of a made-up correlation structure
  for (int K : {1, 3, 5}) {
    const int P = K * (K - 1) / 2;
    std::vector<double> ms((size_t)P), md((size_t)P), R, E;
    for (int p = 0; p < P; p++) {
      ms[(size_t)p] = (1.0 + 0.07 * (p % 4)) / TPG_PCADAPT_MAD_SCALE;
      md[(size_t)p] = (0.9 - 0.05 * (p % 3)) / TPG_PCADAPT_MAD_SCALE;
    }
    if (!host_ogk_corr(K, ms.data(), md.data(), R, E)) return 5;
    if (R.size() != (size_t)K * K || E.size() != (size_t)K * K) return 6;
    for (int i = 0; i < K * K; i++) printf("ogkR %d %d %016" PRIx64 "\n", K, i, bits(R[(size_t)i]));
    for (int i = 0; i < K * K; i++) printf("ogkE %d %d %016" PRIx64 "\n", K, i, bits(E[(size_t)i]));
    std::vector<double> s1((size_t)K), s2((size_t)K), nu((size_t)K), gm((size_t)K), center((size_t)K), cov((size_t)K * K);
    for (int k = 0; k < K; k++) {
      s1[(size_t)k] = 1.5 + 0.25 * k;
      s2[(size_t)k] = 0.75 + 0.125 * k;
      nu[(size_t)k] = 0.1 * (k - 1);
      gm[(size_t)k] = 1.0 + 0.3 * k;
    }
    host_ogk_backmap(K, s1.data(), E.data(), s2.data(), E.data(), nu.data(), gm.data(), center.data(), cov.data());
    for (int i = 0; i < K; i++) printf("ogkc %d %d %016" PRIx64 "\n", K, i, bits(center[(size_t)i]));
    for (int i = 0; i < K * K; i++) printf("ogkV %d %d %016" PRIx64 "\n", K, i, bits(cov[(size_t)i]));
    if (P > 0) {  // a zero scale and a NaN are refused, nothing is read past P entries
      std::vector<double> bad(ms);
      bad[(size_t)(P - 1)] = 0.0;
      if (host_ogk_corr(K, bad.data(), md.data(), R, E)) return 7;
      bad[(size_t)(P - 1)] = NAN;
      if (host_ogk_corr(K, ms.data(), bad.data(), R, E)) return 8;
    }
  }
  printf("ok pcadapt\n");
  return 0;
}
