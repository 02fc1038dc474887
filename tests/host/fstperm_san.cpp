// fstperm_san.cpp -- the host pieces of csrc/host/host_fstperm.h (the label generator behind tpg_fst_perm_labels, the class
// packing and the argument checks of tpg_fst_relabel_sums) as a stand-alone program for the host sanitizers
// (tests/test_fstperm_host.py builds and runs it).  Input: a text file, one query of integers per line:
//   1 n G scheme a b seed r gid[n]         -> rc, then (rc = 0) the n labels of the r-th relabeling
//   2 n G rows labels[rows * n]            -> the class sizes (64 per class group), then the rows * n packed labels
//   3 n G R P pairs[2 P] labels[R * n]     -> rc of the argument checks
// Every array is a heap block of exactly the size the routine is promised, so that an access outside it is an error the
// sanitizer reports.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "host/host_fstperm.h"

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
      if (t.size() < 8) return 3;
      const long long n = t[1];
      if (n < 0 || n > 1000000 || t.size() != 8 + (size_t)n) return 3;
      std::vector<int32_t> gid(t.begin() + 8, t.end()), out((size_t)n, -7);
      const int rc = host_fstperm_labels(n, gid.data(), (int)t[2], (int)t[3], (int)t[4], (int)t[5], (uint64_t)t[6], t[7], out.data(), msg,
                                         sizeof(msg));
      printf("%d", rc);
      if (rc == 0)
        for (long long i = 0; i < n; i++) printf(" %d", out[(size_t)i]);
      printf("\n");
    } else if (t[0] == 2) {
      if (t.size() < 4) return 3;
      const long long n = t[1], G = t[2], rows = t[3];
      if (n < 1 || G < 2 || G > HOST_FSTPERM_MAX_GROUPS || rows < 1 || t.size() != 4 + (size_t)(rows * n)) return 3;
      std::vector<int32_t> lab(t.begin() + 4, t.end());
      if (host_fstperm_check(n, lab.data(), rows, (int)G, std::vector<int32_t>{1, 2}.data(), 1, msg, sizeof(msg))) return 4;
      std::vector<int8_t> lab8((size_t)(rows * n), 99);
      std::vector<int32_t> csize((size_t)(host_fstperm_class_groups(rows, (int)G) * HOST_FSTPERM_TILE), -7);
      host_fstperm_pack(n, lab.data(), rows, (int)G, lab8.data(), csize.data());
      // every labelled individual sits in a class of its own row's slot, inside the class array
      for (long long b = 0; b < rows; b++)
        for (int l = 0; l < (int)G; l++) {
          const int64_t c = host_fstperm_class(b, l, (int)G);
          if (c < 0 || c >= (int64_t)csize.size() || c / HOST_FSTPERM_TILE != b / host_fstperm_slots((int)G)) return 5;
        }
      for (size_t c = 0; c < csize.size(); c++) printf(c ? " %d" : "%d", csize[c]);
      for (size_t i = 0; i < lab8.size(); i++) printf(" %d", (int)lab8[i]);
      printf("\n");
    } else if (t[0] == 3) {
      if (t.size() < 5) return 3;
      const long long n = t[1], G = t[2], R = t[3], P = t[4];
      const size_t np = P > 0 ? (size_t)(2 * P) : 0, nl = R > 0 ? (size_t)(R * n) : 0;
      if (n < 0 || t.size() != 5 + np + nl) return 3;
      std::vector<int32_t> pairs(t.begin() + 5, t.begin() + 5 + (long)np), lab(t.begin() + 5 + (long)np, t.end());
      printf("%d\n", host_fstperm_check(n, lab.data(), R, (int)G, pairs.data(), (int)P, msg, sizeof(msg)));
    } else {
      return 3;
    }
  }
  return 0;
}
