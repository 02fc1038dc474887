// ibdseg_san.cpp -- the per-pair state machine, the breaks and the genome length of csrc/host/host_ibdseg.h, the functions the
// lanes of tpg_ibd_scan_kernel (ibdseg.hip) call, as a stand-alone program for the host sanitizers (tests/test_ibdseg_host.py
// builds and runs it).  Input: a text file
//   m npairs kind min_snp min_length max_gap bridge_min_snp max_err
//   chrom[0] .. chrom[m - 1]
//   pos[0] .. pos[m - 1]
//   npairs lines: the m codes of individual a as one string of the digits 0 - 3, a blank, those of individual b
// Output: "L <genome length>", then one line per reported segment: pair first last n_typed n_err.  Not ordered: exit code 4.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "host/host_ibdseg.h"

struct PrintSink {
  const int64_t* pos;
  long long min_snp, min_length, max_err;
  int pair;
  void operator()(int32_t first, int32_t last, int32_t n_typed, int32_t n_err) {
    if (host_ibd_reported(n_typed, pos[last] - pos[first], n_err, min_snp, min_length, max_err))
      printf("%d %d %d %d %d\n", pair, (int)first, (int)last, (int)n_typed, (int)n_err);
  }
};

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  long long m = 0, npairs = 0, min_snp = 0, min_length = 0, max_gap = 0, bridge = 0, max_err = 0;
  int kind = 0;
  if (fscanf(f, "%lld %lld %d %lld %lld %lld %lld %lld", &m, &npairs, &kind, &min_snp, &min_length, &max_gap, &bridge, &max_err) != 8) return 3;
  if (m < 1 || m > (1 << 24) || npairs < 0 || (kind != 1 && kind != 2) || min_snp < 1 || min_length < 0 || max_gap < 0 || bridge < 0) return 3;
  std::vector<int32_t> chrom((size_t)m);
  std::vector<int64_t> pos((size_t)m);
  for (long long j = 0; j < m; j++) {
    int c = 0;
    if (fscanf(f, "%d", &c) != 1) return 3;
    chrom[(size_t)j] = c;
  }
  for (long long j = 0; j < m; j++) {
    long long x = 0;
    if (fscanf(f, "%lld", &x) != 1) return 3;
    pos[(size_t)j] = x;
  }
  const size_t nwords = (size_t)((m + 31) / 32);
  std::vector<uint32_t> brk(nwords, 0u);
  int64_t length = 0;
  if (host_ibd_breaks(chrom.data(), pos.data(), m, max_gap, brk.data(), &length) >= 0) return 4;
  printf("L %lld\n", (long long)length);
  const int32_t B = (int32_t)(bridge < INT_MAX ? bridge : INT_MAX);
  const bool skip = host_ibd_skip_short(min_snp, bridge);
  std::vector<char> ga((size_t)m + 1), gb((size_t)m + 1);
  char fmt[32];
  snprintf(fmt, sizeof(fmt), "%%%llds %%%llds", m, m);
  for (long long k = 0; k < npairs; k++) {
    if (fscanf(f, fmt, ga.data(), gb.data()) != 2) return 3;
    if ((long long)strlen(ga.data()) != m || (long long)strlen(gb.data()) != m) return 3;
    HostIbdState st;
    PrintSink sink{pos.data(), min_snp, min_length, max_err, (int)k};
    for (size_t w = 0; w < nwords; w++) {
      uint32_t bad = 0, typed = 0;
      for (int b = 0; b < 32; b++) {
        const long long j = (long long)w * 32 + b;
        if (j >= m) break;  // behind the panel: neither bad nor typed
        const int ca = ga[(size_t)j] - '0', cb = gb[(size_t)j] - '0';
        if (ca < 0 || ca > 3 || cb < 0 || cb > 3) return 3;
        bool isbad = false, istyped = false;
        host_ibd_locus_bits(kind, ca, cb, isbad, istyped);
        bad |= (uint32_t)isbad << b;
        typed |= (uint32_t)istyped << b;
      }
      host_ibd_word(st, (int32_t)(w * 32), bad, typed, brk[w], B, skip, sink);
    }
  }
  fclose(f);
  return 0;
}
