// amova_san.cpp -- the host pieces of csrc/host/host_amova.h (the label generator behind tpg_amova_perm_labels, the finisher
// behind tpg_amova_from_sums, the argument checks and the label table of tpg_class_sums) as a stand-alone program for the host
// sanitizers (tests/test_amova_host.py builds and runs it).  Input: a text file, one query of integers per line; a double
// travels as the int64 with its bits:
//   1 n npop nregion scheme seed r pop[n] region_of_pop[npop if nregion > 0]   -> rc, then (rc = 0) pop_out[n], region_of_pop_out[...]
//   2 npop nregion total size[npop] pop_sum[npop] region_of_pop[npop] region_sum[nregion] (the last two if nregion > 0)
//                                                                               -> rc, then (rc = 0) the 21 outputs
//   3 n nclasses R labels[R * n]                                                -> rc of the checks, then (rc = 0) the label table
// Every array is a heap block of exactly the size the routine is promised, so that an access outside it is an error the
// sanitizer reports.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "host/host_amova.h"

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
      const long long n = t[1], npop = t[2], nregion = t[3];
      const size_t nr = nregion > 0 && npop > 0 ? (size_t)npop : 0;
      if (n < 0 || n > 1000000 || npop > 1000000 || t.size() != 7 + (size_t)n + nr) return 3;
      std::vector<int32_t> pop(t.begin() + 7, t.begin() + 7 + (long)n), reg(t.begin() + 7 + (long)n, t.end());
      std::vector<int32_t> pop_out((size_t)n, -7), reg_out(nr, -7);
      const int rc = host_amova_labels(n, pop.data(), (int)npop, nr ? reg.data() : nullptr, (int)nregion, (int)t[4], (uint64_t)t[5], t[6],
                                       pop_out.data(), nr ? reg_out.data() : nullptr, msg, sizeof(msg));
      printf("%d", rc);
      if (rc == 0) {
        for (size_t i = 0; i < pop_out.size(); i++) printf(" %d", pop_out[i]);
        for (size_t p = 0; p < reg_out.size(); p++) printf(" %d", reg_out[p]);
      }
      printf("\n");
    } else if (t[0] == 2) {
      if (t.size() < 4) return 3;
      const long long npop = t[1], nregion = t[2];
      if (npop < 0 || npop > 100000 || nregion < 0 || nregion > 100000) return 3;
      const size_t P = (size_t)npop, G = (size_t)nregion;
      if (t.size() != 4 + 2 * P + (G ? P + G : 0)) return 3;
      std::vector<int64_t> size(t.begin() + 4, t.begin() + 4 + (long)P);
      std::vector<double> pop_sum(P), region_sum(G), out(HOST_AMOVA_OUT, -7.0);
      std::vector<int32_t> reg(G ? P : 0);
      for (size_t p = 0; p < P; p++) pop_sum[p] = as_double(t[4 + P + p]);
      for (size_t p = 0; p < reg.size(); p++) reg[p] = (int32_t)t[4 + 2 * P + p];
      for (size_t g = 0; g < G; g++) region_sum[g] = as_double(t[4 + 3 * P + g]);
      const int rc = host_amova_from_sums((int)npop, size.data(), pop_sum.data(), (int)nregion, G ? reg.data() : nullptr,
                                          G ? region_sum.data() : nullptr, as_double(t[3]), out.data(), msg, sizeof(msg));
      printf("%d", rc);
      for (size_t k = 0; k < out.size(); k++) {
        if (rc == 0) printf(" %lld", as_bits(out[k]));
        else if (out[k] != -7.0) return 5;  // a refusal writes nothing
      }
      printf("\n");
    } else if (t[0] == 3) {
      if (t.size() < 4) return 3;
      const long long n = t[1], nclasses = t[2], R = t[3];
      const size_t nl = R > 0 && n > 0 ? (size_t)(R * n) : 0;
      if (t.size() != 4 + nl) return 3;
      std::vector<int32_t> lab(t.begin() + 4, t.end());
      const int rc = host_classsum_check(n, lab.data(), R, (int)nclasses, msg, sizeof(msg));
      printf("%d", rc);
      if (rc == 0 && R > 0) {
        const long long B = HOST_CLASSSUM_BATCH, nb = (R + B - 1) / B;
        std::vector<int32_t> tab((size_t)(nb * n * B), -7);
        host_classsum_table(n, lab.data(), R, tab.data());
        for (size_t k = 0; k < tab.size(); k++) printf(" %d", tab[k]);
      }
      printf("\n");
    } else {
      return 3;
    }
  }
  return 0;
}
