// host_pwplan.h -- how the pairwise kernels (pairwise.hip) deal their work, written once for the launcher, the kernels and the
// stand-alone program of tests/host/pwplan_main.cpp (tests/test_pwplan_host.py).  No HIP here beyond the function attributes.
//
// `nun` units (tiles of pairs, in patch order) times S equal cuts of the K range [0, kgs) are nun S wave-units; wave-unit u is
// unit u % nun on cut u / nun, the steps [kgs ks / S, kgs (ks + 1) / S).  W takers (waves, or workgroups) walk them round after
// round: taker slot w of round r has index r W + w.
//   full rounds   R = floor(nun S / W): the indices below R W are the wave-units themselves;
//   the tail      the L = nun S - R W wave-units left over run in ONE more round, each cut once more into c equal pieces,
//                 c the largest integer with L c <= W whose pieces keep at least `min_piece` steps (c = 1: the pieces are
//                 the wave-units, i.e. the dealing without a tail).  Tail index t = sub L + j (piece outer, wave-unit inner)
//                 is piece `sub` of wave-unit R W + j: a run of consecutive takers keeps one K window and one run of units.
// R W + L c indices in all.  Sums over K are integers added with atomics, so every such cut gives the same bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TPG_PWPLAN_FN __host__ __device__ static inline
#else
#define TPG_PWPLAN_FN static inline
#endif

struct PwPlan {
  int64_t nun;    // units
  int64_t S;      // cuts of the K range per unit
  int64_t full;   // R W: the indices of the full rounds
  int64_t L;      // wave-units of the tail round
  int64_t c;      // pieces per wave-unit of the tail (>= 1)
  int64_t total;  // full + L c indices
};

// kgs: steps of the K range; min_piece: the shortest piece a further cut may leave; cmax: a cap on c (<= 0: none)
TPG_PWPLAN_FN PwPlan pwplan_make(int64_t nun, int64_t S, int64_t W, int64_t kgs, int64_t min_piece, int64_t cmax) {
  PwPlan p;
  p.nun = nun;
  p.S = S;
  const int64_t all = nun * S;
  p.full = all / W * W;
  p.L = all - p.full;
  int64_t c = 1;
  if (p.L > 0) {
    c = W / p.L;
    const int64_t by_len = (kgs / S) / min_piece;  // the shortest cut is floor(kgs / S) steps; its shortest piece floor of that / c
    if (c > by_len) c = by_len;
    if (cmax > 0 && c > cmax) c = cmax;
    if (c < 1) c = 1;
  }
  p.c = c;
  p.total = p.full + p.L * c;
  return p;
}

// index un < full + L c  ->  unit and steps [k0, k1) of [0, kgs)
TPG_PWPLAN_FN void pwplan_piece(int64_t un, int64_t nun, int64_t S, int64_t full, int64_t L, int64_t c, int64_t kgs,
                                int64_t* unit, int64_t* k0, int64_t* k1) {
  int64_t u = un, sub = 0, cc = 1;
  if (un >= full) {
    const int64_t t = un - full;
    sub = t / L;
    u = full + (t - sub * L);
    cc = c;
  }
  const int64_t ks = u / nun;
  *unit = u - ks * nun;
  const int64_t lo = (kgs * ks) / S, hi = (kgs * (ks + 1)) / S;
  *k0 = lo + ((hi - lo) * sub) / cc;
  *k1 = lo + ((hi - lo) * (sub + 1)) / cc;
}

// what the cost model of the launcher prices: full rounds of ceil(kgs / S) steps and, where L > 0, one round of ceil(kgs / (S c))
TPG_PWPLAN_FN double pwplan_cost(const PwPlan& p, int64_t W, int64_t kgs, double t_step, double t_flush) {
  const int64_t R = p.full / W;
  double cost = (double)R * ((double)((kgs + p.S - 1) / p.S) * t_step + t_flush);
  if (p.L > 0) cost += (double)((kgs + p.S * p.c - 1) / (p.S * p.c)) * t_step + t_flush;
  return cost;
}

// the K split: the cheapest S in [minS, maxS] under pwplan_cost; a larger S has to win by half a per cent
TPG_PWPLAN_FN int64_t pwplan_ksplit(int64_t nun, int64_t kgs, int64_t min_piece, int64_t minS, int64_t W, double t_step,
                                    double t_flush) {
  int64_t bestS = minS;
  double best = -1;
  const int64_t cap = kgs / min_piece;
  int64_t maxS = cap > 0 ? (cap < 96 ? cap : 96) : 1;
  if (maxS < minS) maxS = minS;
  for (int64_t S = minS; S <= maxS; S++) {
    const PwPlan p = pwplan_make(nun, S, W, kgs, min_piece, 0);
    const double cost = pwplan_cost(p, W, kgs, t_step, t_flush);
    if (best < 0 || cost < best * 0.995) { best = cost; bestS = S; }
  }
  return bestS;
}
