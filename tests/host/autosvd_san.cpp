// The host pieces of autoSVD (tidypopgen_amd/csrc/host/host_autosvd.h) as a stand-alone program for the host sanitizers
// (tests/test_autosvd_host.py): the upper normal quantile, the rolling-mean weights on heap arrays of exactly 2 radius + 1
// entries, the closed-form tie counts of the medcouple, g and the fence, and the finder of outlier runs on heap arrays of
// exactly the sizes it is told.  Prints the bits of every result for the test to compare, then "ok autosvd".
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host/host_autosvd.h"

static uint64_t bits(double x) {
  uint64_t u;
  memcpy(&u, &x, sizeof u);
  return u;
}

int main() {
  const double ps[] = {0.25, 0.5, 0.75, 0.025, 1e-3, 2.5e-5, 1e-10, 1e-100, 1e-300, 0.999};
  for (double p : ps) printf("qnorm %016" PRIx64 " %016" PRIx64 "\n", bits(p), bits(host_qnorm_upper(p)));
  for (int radius : {0, 1, 4, 5, 50, 1024}) {
    std::vector<double> w((size_t)(2 * radius + 1));
    host_rollmean_weights(radius, w.data());
    for (size_t i = 0; i < w.size(); i++) printf("w %d %zu %016" PRIx64 "\n", radius, i, bits(w[i]));
  }
  // tie counts: k values at the median among nB entries of B, at candidates below 1, at 1, below +inf, at +inf and beyond
  const uint64_t cands[] = {0, TPG_AUTOSVD_BITS_ONE - 1, TPG_AUTOSVD_BITS_ONE, TPG_AUTOSVD_BITS_INF - 1, TPG_AUTOSVD_BITS_INF,
                            0x7FFFFFFFFFFFFFFFull};
  for (uint64_t k : {0ull, 1ull, 2ull, 5ull, 100000ull})
    for (uint64_t extra : {0ull, 3ull, 3000000000ull})
      for (uint64_t c : cands) printf("tie %" PRIu64 " %" PRIu64 " %016" PRIx64 " %" PRIu64 "\n", k, k + extra, c, tpg_mc_tie_count(k, k + extra, c));
  if (host_mc_g(INFINITY) != -1.0 || host_mc_g(0.0) != 1.0 || host_mc_g(1.0) != 0.0) return 1;
  if (host_mc_from_ratio_bits(0, TPG_AUTOSVD_BITS_INF) != 0.0) return 2;
  double coef, thr;
  host_tukey_fence(2000.0, 1.0, 2.0, 0.1, 0.05, &coef, &thr);
  printf("fence %016" PRIx64 " %016" PRIx64 "\n", bits(coef), bits(thr));
  host_tukey_fence(2000.0, 1.0, 2.0, -0.1, 0.05, &coef, &thr);
  printf("fence %016" PRIx64 " %016" PRIx64 "\n", bits(coef), bits(thr));
  // runs: 18 .. 21 is cut by a chromosome boundary between 19 and 20
  {
    const std::vector<int64_t> pos = {3, 4, 5, 9, 10, 11, 12, 18, 19, 20, 21, 30};
    const std::vector<int32_t> ch = {1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2};
    std::vector<int64_t> first, last;
    for (int64_t min_size : {1, 2, 3, 4, 5}) {
      host_outlier_runs(pos.data(), ch.data(), (int64_t)pos.size(), min_size, first, last);
      if (first.size() != last.size()) return 3;
      for (size_t i = 0; i < first.size(); i++) printf("run %" PRId64 " %" PRId64 " %" PRId64 "\n", min_size, first[i], last[i]);
    }
    host_outlier_runs(pos.data(), ch.data(), 0, 1, first, last);
    if (!first.empty()) return 4;
  }
  printf("ok autosvd\n");
  return 0;
}
