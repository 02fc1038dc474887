// pwplan_main.cpp -- the dealing of the pairwise kernels (tidypopgen_amd/csrc/host/host_pwplan.h: pwplan_make, pwplan_piece,
// pwplan_ksplit, the functions the launcher and the kernels of pairwise.hip call) as a stand-alone host program
// (tests/test_pwplan_host.py builds and runs it).  Input: a text file, one query per line,
//   "plan nun S W kgs min_piece cmax"                      -> int32 {nun, S, W, kgs, full, L, c, total}, then total x {unit, k0, k1}
//   "ksplit nun kgs min_piece minS W t_step t_flush"        -> int32 {S, 0, 0, 0, 0, 0, 0, 0}
// Output: the binary records, one after the other, into the file named second.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "host/host_pwplan.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "wb");
  if (!f || !out) return 2;
  char what[16];
  while (fscanf(f, "%15s", what) == 1) {
    if (!strcmp(what, "plan")) {
      long long nun, S, W, kgs, min_piece, cmax;
      if (fscanf(f, "%lld %lld %lld %lld %lld %lld", &nun, &S, &W, &kgs, &min_piece, &cmax) != 6) return 3;
      if (nun < 1 || S < 1 || W < 1 || kgs < 0 || min_piece < 1 || kgs >= (1ll << 31) || nun * S >= (1ll << 31)) return 3;
      const PwPlan p = pwplan_make(nun, S, W, kgs, min_piece, cmax);
      const int32_t head[8] = {(int32_t)nun, (int32_t)S, (int32_t)W, (int32_t)kgs, (int32_t)p.full, (int32_t)p.L, (int32_t)p.c,
                               (int32_t)p.total};
      fwrite(head, sizeof(int32_t), 8, out);
      std::vector<int32_t> rows((size_t)p.total * 3);
      for (int64_t un = 0; un < p.total; un++) {
        int64_t unit = -1, k0 = -1, k1 = -1;
        pwplan_piece(un, p.nun, p.S, p.full, p.L, p.c, kgs, &unit, &k0, &k1);
        rows[(size_t)un * 3] = (int32_t)unit;
        rows[(size_t)un * 3 + 1] = (int32_t)k0;
        rows[(size_t)un * 3 + 2] = (int32_t)k1;
      }
      fwrite(rows.data(), sizeof(int32_t), rows.size(), out);
    } else if (!strcmp(what, "ksplit")) {
      long long nun, kgs, min_piece, minS, W;
      double t_step, t_flush;
      if (fscanf(f, "%lld %lld %lld %lld %lld %lf %lf", &nun, &kgs, &min_piece, &minS, &W, &t_step, &t_flush) != 7) return 3;
      const int32_t head[8] = {(int32_t)pwplan_ksplit(nun, kgs, min_piece, minS, W, t_step, t_flush), 0, 0, 0, 0, 0, 0, 0};
      fwrite(head, sizeof(int32_t), 8, out);
    } else {
      return 3;
    }
  }
  fclose(f);
  return fclose(out) == 0 ? 0 : 4;
}
