// host_amova.h -- the host pieces of include/tpg.h "AMOVA": the r-th relabeling of tpg_amova_perm_labels (three permutation
// schemes over a two-step hierarchy individual -> population -> region), the finisher tpg_amova_from_sums (sums of squared
// deviations, mean squares, variance components and the three Phi of one relabeling, statement for statement as the header
// gives them) and the argument checks and the label table of tpg_class_sums (amova.hip).  Plain C++ with no HIP in it:
// amova.hip calls these very functions, and tests/host/amova_san.cpp builds the same text under the host sanitizers.  The
// finisher is IEEE double in the order written here: compile without FMA contraction.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../synth_common.h"

#define HOST_CLASSSUM_CHUNK 512         // columns of a chunk partial
#define HOST_CLASSSUM_TILE_ROWS 256     // rows of a workgroup: one row per lane
#define HOST_CLASSSUM_BATCH 32          // labelings a workgroup carries in registers
#define HOST_CLASSSUM_MAX_CLASSES 1024
#define HOST_CLASSSUM_MAX_N (1ll << 20)
#define HOST_CLASSSUM_MAX_ROWS 512      // labelings per internal pass at most ...
#define HOST_CLASSSUM_PART_CAP (256ll << 20)  // ... and bytes of chunk partials at most (unless one batch alone takes more)
#define HOST_AMOVA_OUT 21               // df[4], ssd[4], msd[3], ncoef[3], sigma2[4], phi[3]

// ---- tpg_class_sums: checks, plan, label table ------------------------------------------------------------------------------
// 0 = fine, 1 = a bad argument described in msg
static inline int host_classsum_check(int64_t n, const int32_t* labels, int64_t R, int nclasses, char* msg, size_t cap) {
  if (n < 1) { snprintf(msg, cap, "n = %lld: at least one individual", (long long)n); return 1; }
  if (n > HOST_CLASSSUM_MAX_N) { snprintf(msg, cap, "n = %lld: at most 2^20 individuals", (long long)n); return 1; }
  if (R < 0) { snprintf(msg, cap, "R = %lld is negative", (long long)R); return 1; }
  if (nclasses < 1 || nclasses > HOST_CLASSSUM_MAX_CLASSES) {
    snprintf(msg, cap, "nclasses = %d out of [1, TPG_CLASSSUM_MAX_CLASSES = %d]", nclasses, HOST_CLASSSUM_MAX_CLASSES);
    return 1;
  }
  if (R > 0 && !labels) { snprintf(msg, cap, "null argument"); return 1; }
  for (int64_t r = 0; r < R; r++)
    for (int64_t i = 0; i < n; i++) {
      const int32_t l = labels[r * n + i];
      if (l < -1 || l >= nclasses) {
        snprintf(msg, cap, "labels[%lld][%lld] = %d out of [-1,%d)", (long long)r, (long long)i, l, nclasses);
        return 1;
      }
    }
  return 0;
}

static inline int64_t host_classsum_chunks(int64_t n) { return (n + HOST_CLASSSUM_CHUNK - 1) / HOST_CLASSSUM_CHUNK; }

// the labelings of one internal pass: a multiple of the batch, at most HOST_CLASSSUM_MAX_ROWS, with chunk partials
// (chunks x rows x n doubles) of at most HOST_CLASSSUM_PART_CAP bytes -- but never less than one batch
static inline int64_t host_classsum_pass_rows(int64_t n) {
  const int64_t per_row = host_classsum_chunks(n) * n * 8;
  int64_t rows = std::min<int64_t>(HOST_CLASSSUM_MAX_ROWS, HOST_CLASSSUM_PART_CAP / per_row);
  rows = rows / HOST_CLASSSUM_BATCH * HOST_CLASSSUM_BATCH;
  return std::max<int64_t>(rows, HOST_CLASSSUM_BATCH);
}

// device scratch of a call with R labelings (A itself not counted): the label table, the chunk partials, the row sums t and
// the class sums of one pass.  -1 on a bad size
static inline int64_t host_classsum_scratch_bytes(int64_t n, int64_t R, int nclasses) {
  if (n < 1 || n > HOST_CLASSSUM_MAX_N || R < 0 || nclasses < 1 || nclasses > HOST_CLASSSUM_MAX_CLASSES) return -1;
  const int64_t B = HOST_CLASSSUM_BATCH;
  const int64_t rows = std::min(host_classsum_pass_rows(n), (R + B - 1) / B * B);
  return rows * n * 4 + host_classsum_chunks(n) * rows * n * 8 + rows * n * 8 + rows * (int64_t)nclasses * 8;
}

// `rows` checked label rows -> the table the kernels read: tab[(b n + i) B + q] = the label of individual i under row b B + q
// of the pass, -1 for the rows behind the last one (ceil(rows / B) batches)
static inline void host_classsum_table(int64_t n, const int32_t* labels, int64_t rows, int32_t* tab) {
  const int64_t B = HOST_CLASSSUM_BATCH, nb = (rows + B - 1) / B;
  for (int64_t b = 0; b < nb; b++)
    for (int64_t i = 0; i < n; i++)
      for (int64_t q = 0; q < B; q++) {
        const int64_t r = b * B + q;
        tab[(b * n + i) * B + q] = r < rows ? labels[r * n + i] : -1;
      }
}

// ---- tpg_amova_perm_labels ----------------------------------------------------------------------------------------------------
static inline uint64_t host_amova_key(uint64_t seed, int64_t r, uint64_t u) {
  return tpg_mix64(seed ^ tpg_mix64(((uint64_t)r << 32) + u));
}

// the design: every id in range, no empty population, no empty region.  0 = fine, 1 = described in msg
static inline int host_amova_design(int64_t n, const int32_t* pop0, int npop, const int32_t* region_of_pop0, int nregion, char* msg,
                                    size_t cap) {
  if (n < 0 || n >= ((int64_t)1 << 31) || (n > 0 && !pop0)) { snprintf(msg, cap, "bad n or null argument"); return 1; }
  if (npop < 1) { snprintf(msg, cap, "npop must be positive"); return 1; }
  if (nregion < 0 || nregion > npop) { snprintf(msg, cap, "nregion = %d out of [0, npop = %d]", nregion, npop); return 1; }
  if (nregion > 0 && !region_of_pop0) { snprintf(msg, cap, "null argument"); return 1; }
  std::vector<int64_t> np_((size_t)npop, 0), ng((size_t)nregion, 0);
  for (int64_t i = 0; i < n; i++) {
    if (pop0[i] < -1 || pop0[i] >= npop) {
      snprintf(msg, cap, "pop[%lld] = %d out of [-1,%d)", (long long)i, pop0[i], npop);
      return 1;
    }
    if (pop0[i] >= 0) np_[(size_t)pop0[i]]++;
  }
  for (int p = 0; p < npop; p++) {
    if (np_[(size_t)p] == 0) { snprintf(msg, cap, "population %d is empty", p); return 1; }
    if (nregion > 0) {
      const int32_t g = region_of_pop0[p];
      if (g < 0 || g >= nregion) { snprintf(msg, cap, "region_of_pop[%d] = %d out of [0,%d)", p, g, nregion); return 1; }
      ng[(size_t)g]++;
    }
  }
  for (int g = 0; g < nregion; g++)
    if (ng[(size_t)g] == 0) { snprintf(msg, cap, "region %d is empty", g); return 1; }
  return 0;
}

// The r-th relabeling (include/tpg.h "AMOVA"): 0 = fine, 1 = a bad argument described in msg.  pop_out has n entries;
// region_of_pop_out has npop entries and is written when nregion > 0 (it may be NULL when nregion == 0).
static inline int host_amova_labels(int64_t n, const int32_t* pop0, int npop, const int32_t* region_of_pop0, int nregion, int scheme,
                                    uint64_t seed, int64_t r, int32_t* pop_out, int32_t* region_of_pop_out, char* msg, size_t cap) {
  if (host_amova_design(n, pop0, npop, region_of_pop0, nregion, msg, cap)) return 1;
  if (scheme < 0 || scheme > 2) { snprintf(msg, cap, "scheme = %d: 0 (Phi_ST), 1 (Phi_SC) or 2 (Phi_CT)", scheme); return 1; }
  if (nregion == 0 && scheme != 0) { snprintf(msg, cap, "scheme = %d needs regions", scheme); return 1; }
  if (r < 0 || r >= ((int64_t)1 << 31)) { snprintf(msg, cap, "r = %lld out of [0, 2^31)", (long long)r); return 1; }
  if ((n > 0 && !pop_out) || (nregion > 0 && !region_of_pop_out)) { snprintf(msg, cap, "null output"); return 1; }
  for (int64_t i = 0; i < n; i++) pop_out[i] = pop0[i];
  for (int p = 0; p < npop && nregion > 0; p++) region_of_pop_out[p] = region_of_pop0[p];
  if (r == 0) return 0;  // the identity, not hashed
  typedef std::pair<uint64_t, int64_t> KI;
  // sigma = e sorted by (key, index); unit sigma_t receives what unit e_t held
  auto shuffle = [&](const std::vector<int64_t>& e, const int32_t* from, int32_t* to) {
    std::vector<KI> keys(e.size());
    for (size_t t = 0; t < e.size(); t++) keys[t] = KI(host_amova_key(seed, r, (uint64_t)e[t]), e[t]);
    std::sort(keys.begin(), keys.end());
    for (size_t t = 0; t < e.size(); t++) to[keys[t].second] = from[e[t]];
  };
  if (scheme == 2) {  // the populations are the units: population sigma_t receives the region of population e_t
    std::vector<int64_t> e((size_t)npop);
    for (int p = 0; p < npop; p++) e[(size_t)p] = p;
    shuffle(e, region_of_pop0, region_of_pop_out);
    return 0;
  }
  const int nset = scheme == 1 ? nregion : 1;  // scheme 1: every region on its own; scheme 0: everybody with a population
  std::vector<std::vector<int64_t>> sets((size_t)nset);
  for (int64_t i = 0; i < n; i++)
    if (pop0[i] >= 0) sets[scheme == 1 ? (size_t)region_of_pop0[pop0[i]] : 0].push_back(i);
  for (int g = 0; g < nset; g++) shuffle(sets[(size_t)g], pop0, pop_out);
  return 0;
}

// ---- tpg_amova_from_sums -------------------------------------------------------------------------------------------------------
// One relabeling's class sums -> out[HOST_AMOVA_OUT].  0 = fine, 1 = a bad argument described in msg (nothing written).
static inline int host_amova_from_sums(int npop, const int64_t* pop_size, const double* pop_sum, int nregion, const int32_t* region_of_pop0,
                                       const double* region_sum, double total_sum, double* out, char* msg, size_t cap) {
  if (npop < 1 || !pop_size || !pop_sum || !out) { snprintf(msg, cap, "null argument or npop < 1"); return 1; }
  if (nregion < 0 || nregion > npop || (nregion > 0 && (!region_of_pop0 || !region_sum))) {
    snprintf(msg, cap, "nregion = %d out of [0, npop = %d], or null argument", nregion, npop);
    return 1;
  }
  std::vector<int64_t> Ng((size_t)nregion, 0);
  int64_t N = 0, sq = 0;  // N = sum n_p, sq = sum n_p^2
  for (int p = 0; p < npop; p++) {
    if (pop_size[p] < 1 || pop_size[p] >= ((int64_t)1 << 31)) { snprintf(msg, cap, "population %d has %lld individuals", p, (long long)pop_size[p]); return 1; }
    if (nregion > 0) {
      const int32_t g = region_of_pop0[p];
      if (g < 0 || g >= nregion) { snprintf(msg, cap, "region_of_pop[%d] = %d out of [0,%d)", p, g, nregion); return 1; }
      Ng[(size_t)g] += pop_size[p];
    }
    N += pop_size[p];
    sq += pop_size[p] * pop_size[p];
  }
  for (int g = 0; g < nregion; g++)
    if (Ng[(size_t)g] == 0) { snprintf(msg, cap, "region %d is empty", g); return 1; }
  const double nan = NAN, Nd = (double)N;
  const int P = npop, G = nregion;
  auto over = [&](double x, int64_t d) { return d > 0 ? x / (double)d : nan; };  // a zero df: NaN
  double* df = out;
  double* ssd = out + 4;
  double* msd = out + 8;
  double* nc = out + 11;
  double* s2 = out + 14;
  double* phi = out + 18;
  const double ssd_t = total_sum / (2.0 * Nd);
  double ssd_wp = 0.0;
  for (int p = 0; p < P; p++) ssd_wp += pop_sum[p] / (2.0 * (double)pop_size[p]);
  if (G > 0) {
    double ssd_wr = 0.0, S1 = 0.0;
    int64_t sqg = 0;
    for (int g = 0; g < G; g++) {
      ssd_wr += region_sum[g] / (2.0 * (double)Ng[(size_t)g]);
      sqg += Ng[(size_t)g] * Ng[(size_t)g];
    }
    for (int p = 0; p < P; p++) S1 += (double)(pop_size[p] * pop_size[p]) / (double)Ng[(size_t)region_of_pop0[p]];
    const int64_t d0 = G - 1, d1 = P - G, d2 = N - P;
    df[0] = (double)d0; df[1] = (double)d1; df[2] = (double)d2; df[3] = (double)(N - 1);
    ssd[0] = ssd_t - ssd_wr; ssd[1] = ssd_wr - ssd_wp; ssd[2] = ssd_wp; ssd[3] = ssd_t;
    msd[0] = over(ssd[0], d0); msd[1] = over(ssd[1], d1); msd[2] = over(ssd[2], d2);
    nc[0] = over(Nd - S1, d1);
    nc[1] = over(S1 - (double)sq / Nd, d0);
    nc[2] = over(Nd - (double)sqg / Nd, d0);
    const double sc = msd[2];
    const double sb = (msd[1] - sc) / nc[0];
    double t = msd[0] - sc;
    t = t - nc[1] * sb;
    const double sa = t / nc[2];
    const double sab = sa + sb;
    const double st = sab + sc;
    s2[0] = sa; s2[1] = sb; s2[2] = sc; s2[3] = st;
    phi[0] = sa / st;
    phi[1] = sb / (sb + sc);
    phi[2] = sab / st;
  } else {
    const int64_t d1 = P - 1, d2 = N - P;
    df[0] = nan; df[1] = (double)d1; df[2] = (double)d2; df[3] = (double)(N - 1);
    ssd[0] = nan; ssd[1] = ssd_t - ssd_wp; ssd[2] = ssd_wp; ssd[3] = ssd_t;
    msd[0] = nan; msd[1] = over(ssd[1], d1); msd[2] = over(ssd[2], d2);
    nc[0] = over(Nd - (double)sq / Nd, d1); nc[1] = nan; nc[2] = nan;
    const double sc = msd[2];
    const double sb = (msd[1] - sc) / nc[0];
    const double st = sb + sc;
    s2[0] = nan; s2[1] = sb; s2[2] = sc; s2[3] = st;
    phi[0] = nan; phi[1] = nan;
    phi[2] = sb / st;
  }
  return 0;
}
