// knnimp_san.cpp -- the distance and the histogram walk of csrc/host/host_knnimp.h, the functions the vote kernel of
// knnimp.hip calls, as a stand-alone program for the host sanitizers (tests/test_knn_impute_host.py builds and runs it).
// Input: a text file, one query per line; output: one integer per query.
//   D L a_0 .. a_{L-1} b_0 .. b_{L-1}   the codes (0..3) of two individuals at L <= 32 loci -> the distance of their profiles
//   V ndist k h_0 .. h_{3 ndist - 1}    hist[dist * 3 + g], ndist <= 65 -> the fill (3: nobody votes)
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "host/host_knnimp.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char what;
  while (fscanf(f, " %c", &what) == 1) {
    if (what == 'D') {
      int L = 0;
      if (fscanf(f, "%d", &L) != 1 || L < 0 || L > HOST_KNN_MAX_L) return 3;
      uint64_t th[2] = {0, 0};
      uint32_t ms[2] = {0, 0};
      for (int s = 0; s < 2; s++)
        for (int t = 0; t < L; t++) {
          int c = 0;
          if (fscanf(f, "%d", &c) != 1 || c < 0 || c > 3) return 3;
          host_knn_profile_add(&th[s], &ms[s], t, c);
        }
      printf("%d\n", host_knn_dist(th[0], ms[0], th[1], ms[1]));
    } else if (what == 'V') {
      int ndist = 0;
      long long k = 0;
      if (fscanf(f, "%d %lld", &ndist, &k) != 2 || ndist < 1 || ndist > HOST_KNN_DISTS) return 3;
      std::vector<int32_t> hist((size_t)3 * ndist);  // exactly the entries the walk may read
      int64_t T = 0;
      for (size_t x = 0; x < hist.size(); x++) {
        int v = 0;
        if (fscanf(f, "%d", &v) != 1 || v < 0) return 3;
        hist[x] = v;
        T += v;
      }
      printf("%d\n", host_knn_vote(hist.data(), ndist, (int64_t)k, T));
    } else {
      return 3;
    }
  }
  fclose(f);
  return 0;
}
