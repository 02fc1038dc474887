// mantel_san.cpp -- the host pieces of csrc/host/host_mantel.h (the permutation list behind tpg_mantel_perms, the finishers behind
// tpg_mantel_from_sums and tpg_mantel_partial, the argument checks, the inverse permutations and the scratch bound of
// tpg_mantel_sums) as a stand-alone program for the host sanitizers (tests/test_mantel_host.py builds and runs it).  Input: a text
// file, one query of integers per line; a double travels as the int64 with its bits:
//   1 n nstrata seed r0 R has_strata strata[n if has_strata]   -> rc, then (rc = 0) the R x n permutations
//   2 N Sa Saa Sb Sbb Sab                                       -> the bits of r
//   3 r_ab r_ac r_bc                                            -> the bits of the partial correlation
//   4 n Q R perms[R * n]                                        -> rc of the checks, then (rc = 0) the inverse permutations
//   5 n R Q                                                     -> the scratch bound
// Every array is a heap block of exactly the size the routine is promised, so that an access outside it is an error the
// sanitizer reports.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "host/host_mantel.h"

static double as_double(long long b) {
  double x;
  memcpy(&x, &b, sizeof(x));
  return x;
}
static long long as_bits(double x) {
  long long b;
  memcpy(&b, &x, sizeof(b));
  return b;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string line;
  char msg[320];
  while (std::getline(f, line)) {
    std::istringstream in(line);
    std::vector<long long> t;
    for (long long x; in >> x;) t.push_back(x);
    if (t.empty()) continue;
    if (t[0] == 1) {
      if (t.size() < 7) return 3;
      const long long n = t[1], nstrata = t[2], r0 = t[4], R = t[5], has = t[6];
      const size_t ns = has && n > 0 ? (size_t)n : 0;
      if (n > 1000000 || R > 100000 || t.size() != 7 + ns) return 3;
      std::vector<int32_t> strata(t.begin() + 7, t.end());
      const size_t cells = R > 0 && n > 0 ? (size_t)(R * n) : 0;
      std::vector<int32_t> out(cells, -7);
      const int rc = host_mantel_perms(n, has ? strata.data() : nullptr, (int)nstrata, (uint64_t)t[3], r0, R, out.data(), msg, sizeof(msg));
      printf("%d", rc);
      for (size_t k = 0; k < out.size(); k++) {
        if (rc == 0) printf(" %d", out[k]);
        else if (out[k] != -7) return 5;  // a refusal writes nothing
      }
      printf("\n");
    } else if (t[0] == 2) {
      if (t.size() != 7) return 3;
      printf("%lld\n", as_bits(host_mantel_from_sums(t[1], as_double(t[2]), as_double(t[3]), as_double(t[4]), as_double(t[5]), as_double(t[6]))));
    } else if (t[0] == 3) {
      if (t.size() != 4) return 3;
      printf("%lld\n", as_bits(host_mantel_partial(as_double(t[1]), as_double(t[2]), as_double(t[3]))));
    } else if (t[0] == 4) {
      if (t.size() < 4) return 3;
      const long long n = t[1], Q = t[2], R = t[3];
      const size_t cells = R > 0 && n > 0 ? (size_t)(R * n) : 0;
      if (t.size() != 4 + cells) return 3;
      std::vector<int32_t> perms(t.begin() + 4, t.end());
      const int rc = host_mantel_check(n, (int)Q, perms.data(), R, msg, sizeof(msg));
      printf("%d", rc);
      if (rc == 0 && R > 0) {
        std::vector<int32_t> inv(cells, -7);
        host_mantel_inverse(n, perms.data(), R, inv.data());
        for (size_t k = 0; k < inv.size(); k++) printf(" %d", inv[k]);
      }
      printf("\n");
    } else if (t[0] == 5) {
      if (t.size() != 4) return 3;
      printf("%lld\n", (long long)host_mantel_scratch_bytes(t[1], t[2], (int)t[3]));
    } else {
      return 3;
    }
  }
  return 0;
}
