/* host_f4jack.h -- f4 of one quadruple of populations from blocked f2, with the weighted delete-one block jackknife (plain
 * C99 / C++, host only).  include/tpg.h "f2 blocks" states the arithmetic: Busing, Meijer, van der Leeden 1999, "Delete-m
 * jackknife for unequal m", with the block's kept loci as its weight.  Every sum runs in ascending b, in double, in the
 * order written there; build the including file without FMA contraction. */
#ifndef TPG_HOST_F4JACK_H
#define TPG_HOST_F4JACK_H

#include <math.h>
#include <stdint.h>

/* theta_b of quadruple (A, B; C, D) in block b; f2 is G x G x nb column-major */
static inline double tpg_f4_block(const double* f2, int64_t G, int64_t b, int A, int B, int C, int D) {
  const double* f = f2 + b * G * G;
  return 0.5 * (f[A + D * G] + f[B + C * G] - f[A + C * G] - f[B + D * G]);
}

static inline void tpg_f4_jackknife_one(const double* f2, int64_t G, int64_t nb, const int64_t* block_len, int A, int B, int C,
                                        int D, double* est, double* se, int32_t* n_used) {
  double n = 0.0, wsum = 0.0;
  int64_t g = 0;
  for (int64_t b = 0; b < nb; b++) {
    const double th = tpg_f4_block(f2, G, b, A, B, C, D);
    if (th != th || block_len[b] <= 0) continue;
    const double nbk = (double)block_len[b];
    n += nbk;
    wsum += nbk * th;
    g++;
  }
  *n_used = (int32_t)g;
  const double theta = g > 0 ? wsum / n : NAN;
  *est = theta;
  *se = NAN;
  if (g < 2) return;
  double sub = 0.0;
  for (int64_t b = 0; b < nb; b++) {
    const double th = tpg_f4_block(f2, G, b, A, B, C, D);
    if (th != th || block_len[b] <= 0) continue;
    const double nbk = (double)block_len[b];
    const double loo = (n * theta - nbk * th) / (n - nbk);
    sub += (1.0 - nbk / n) * loo;
  }
  const double e = (double)g * theta - sub;
  double var = 0.0;
  for (int64_t b = 0; b < nb; b++) {
    const double th = tpg_f4_block(f2, G, b, A, B, C, D);
    if (th != th || block_len[b] <= 0) continue;
    const double nbk = (double)block_len[b];
    const double loo = (n * theta - nbk * th) / (n - nbk);
    const double h = n / nbk;
    const double tau = h * theta - (h - 1.0) * loo;
    const double dlt = tau - e;
    var += dlt * dlt / (h - 1.0);
  }
  *est = e;
  *se = sqrt(1.0 / (double)g * var);
}

#endif
