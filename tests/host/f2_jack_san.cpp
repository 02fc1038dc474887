// The f4 block jackknife (tidypopgen_amd/csrc/host/host_f4jack.h) as a stand-alone program for the host sanitizers
// (tests/test_f2_host.py): heap arrays of exactly the sizes the function is told, NaN blocks, empty blocks, 0 / 1 / 2 usable
// blocks and a repeated population.  Prints the bits of one result for the test to compare, then "ok f4jack".
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host/host_f4jack.h"

static uint64_t bits(double x) {
  uint64_t u;
  memcpy(&u, &x, sizeof u);
  return u;
}

int main() {
  const int G = 4;
  const int64_t nb = 9;
  std::vector<double> f2((size_t)G * G * nb);
  std::vector<int64_t> bl((size_t)nb);
  for (int64_t b = 0; b < nb; b++) {
    bl[(size_t)b] = 100 + 37 * b;
    for (int i = 0; i < G; i++)
      for (int j = 0; j < G; j++)
        f2[(size_t)(i + j * G + b * G * G)] = i == j ? 0.0 : 0.01 * (1 + (i + j) % 3) + 0.001 * (double)((7 * b + i * j) % 5);
  }
  f2[(size_t)(0 + 2 * G + 3 * G * G)] = f2[(size_t)(2 + 0 * G + 3 * G * G)] = NAN;
  bl[5] = 0;
  double est, se;
  int32_t used;
  tpg_f4_jackknife_one(f2.data(), G, nb, bl.data(), 0, 1, 2, 3, &est, &se, &used);
  if (used != 7 || !(se > 0)) return 1;
  printf("f4 %016" PRIx64 " %016" PRIx64 " %d\n", bits(est), bits(se), used);
  tpg_f4_jackknife_one(f2.data(), G, nb, bl.data(), 2, 0, 2, 1, &est, &se, &used);  // f3 through the +0.0 diagonal
  if (used != 7 || est != est) return 2;
  tpg_f4_jackknife_one(f2.data(), G, nb, bl.data(), 1, 1, 1, 1, &est, &se, &used);
  if (used != 8 || est != 0.0 || se != 0.0) return 3;
  for (int usable = 0; usable <= 2; usable++) {  // 0, 1 and 2 usable blocks; nb = 0 reads nothing
    std::vector<int64_t> few((size_t)nb, 0);
    for (int k = 0; k < usable; k++) few[(size_t)k] = 50 + k;
    tpg_f4_jackknife_one(f2.data(), G, nb, few.data(), 0, 1, 2, 3, &est, &se, &used);
    if (used != usable || (usable == 0) != (est != est) || (usable < 2) != (se != se)) return 4;
  }
  tpg_f4_jackknife_one(nullptr, G, 0, nullptr, 0, 1, 2, 3, &est, &se, &used);
  if (used != 0 || est == est) return 5;
  printf("ok f4jack\n");
  return 0;
}
