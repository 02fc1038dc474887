// ldstat_san.cpp -- r2, its fixed-point value and the distance bin of csrc/host/host_ldstat.h, the functions the epilogue of
// tpg_ldstat_kernel (ldstat.hip) calls, as a stand-alone program for the host sanitizers (tests/test_ldstat_host.py builds and
// runs it).  Input: a text file, one query per line; output: one line per query.
//   R n sxy sxj sxk dj dk      the sums of a valid pair (dj, dk > 0 as integers below 2^53) -> the bits of r2 as an unsigned
//                              integer, and q
//   B dist bin_size nbins      -> the bin, nbins for "beyond"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "host/host_ldstat.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char what;
  while (fscanf(f, " %c", &what) == 1) {
    if (what == 'R') {
      long long n = 0, sxy = 0, sxj = 0, sxk = 0, dj = 0, dk = 0;
      if (fscanf(f, "%lld %lld %lld %lld %lld %lld", &n, &sxy, &sxj, &sxk, &dj, &dk) != 6) return 3;
      if (n < 1 || n >= (1ll << 22) || sxy < 0 || sxy > 4 * n || sxj < 0 || sxj > 2 * n || sxk < 0 || sxk > 2 * n) return 3;
      if (dj < 1 || dk < 1 || dj >= (1ll << 53) || dk >= (1ll << 53)) return 3;
      const long long num = n * sxy - sxj * sxk;
      if ((__int128)num * num > (__int128)dj * dk) return 3;  // not the sums of two loci: q's conversion takes r2 <= 1
      const double r2 = host_ldstat_r2((int32_t)n, (int32_t)sxy, (int32_t)sxj, (int32_t)sxk, (double)dj, (double)dk);
      unsigned long long bits = 0;
      memcpy(&bits, &r2, sizeof(bits));
      printf("%llu %llu\n", bits, (unsigned long long)host_ldstat_q(r2));
    } else if (what == 'B') {
      long long dist = 0, bin_size = 0;
      int nbins = 0;
      if (fscanf(f, "%lld %lld %d", &dist, &bin_size, &nbins) != 3) return 3;
      if (dist < 0 || bin_size < 1 || nbins < 1 || nbins > HOST_LDSTAT_MAX_BINS) return 3;
      printf("%d\n", host_ldstat_bin((int64_t)dist, (int64_t)bin_size, nbins));
    } else {
      return 3;
    }
  }
  fclose(f);
  return 0;
}
