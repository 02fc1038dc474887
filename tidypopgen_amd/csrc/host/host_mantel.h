// host_mantel.h -- the host pieces of include/tpg.h "Mantel tests": the permutation list of tpg_mantel_perms (a batch of rows in
// one call, within strata or not), the finishers tpg_mantel_from_sums and tpg_mantel_partial (statement for statement as the
// header gives them) and the argument checks, the inverse permutations and the scratch plan of tpg_mantel_sums (mantel.hip).
// Plain C++ with no HIP in it: mantel.hip calls these very functions, and tests/host/mantel_san.cpp builds the same text under
// the host sanitizers.  The finishers are IEEE double in the order written here: compile without FMA contraction.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <exception>
#include <thread>
#include <utility>
#include <vector>

#include "../synth_common.h"

#define HOST_MANTEL_LANES 256            // partials of a column term: one per thread of a workgroup
#define HOST_MANTEL_MAX_N 16384          // a column of A in LDS: 8 n bytes
#define HOST_MANTEL_MAX_Q 4
#define HOST_MANTEL_BATCH 32             // permutations a workgroup walks with one column of A staged
#define HOST_MANTEL_MAX_ROWS 512         // permutations per internal pass at most ...
#define HOST_MANTEL_TERM_CAP (64ll << 20)  // ... and bytes of column terms at most (never less than one batch)
#define HOST_MANTEL_PERM_THREADS 8       // threads of tpg_mantel_perms at most
#define HOST_MANTEL_STRIDES(Q) ((Q) == 1 ? 8 : 4)  // strides of L rows a thread of the product kernel keeps in flight

// ---- tpg_mantel_sums: checks, plan, inverse permutations -------------------------------------------------------------------------
static inline int host_mantel_size_ok(int64_t n, int64_t R, int Q) {
  return n >= 1 && n <= HOST_MANTEL_MAX_N && R >= 0 && Q >= 1 && Q <= HOST_MANTEL_MAX_Q;
}

// 0 = fine, 1 = a bad argument described in msg.  Every row of perms must be a bijection of 0 .. n-1.
static inline int host_mantel_check(int64_t n, int Q, const int32_t* perms, int64_t R, char* msg, size_t cap) {
  if (n < 1 || n > HOST_MANTEL_MAX_N) { snprintf(msg, cap, "n = %lld out of [1, TPG_MANTEL_MAX_N = %d]", (long long)n, HOST_MANTEL_MAX_N); return 1; }
  if (Q < 1 || Q > HOST_MANTEL_MAX_Q) { snprintf(msg, cap, "Q = %d out of [1, TPG_MANTEL_MAX_Q = %d]", Q, HOST_MANTEL_MAX_Q); return 1; }
  if (R < 0) { snprintf(msg, cap, "R = %lld is negative", (long long)R); return 1; }
  if (R > 0 && !perms) { snprintf(msg, cap, "null argument"); return 1; }
  std::vector<uint8_t> seen((size_t)n);
  for (int64_t r = 0; r < R; r++) {
    std::fill(seen.begin(), seen.end(), (uint8_t)0);
    for (int64_t i = 0; i < n; i++) {
      const int32_t p = perms[r * n + i];
      if (p < 0 || p >= n) { snprintf(msg, cap, "perms[%lld][%lld] = %d out of [0,%lld)", (long long)r, (long long)i, p, (long long)n); return 1; }
      if (seen[(size_t)p]) { snprintf(msg, cap, "perms[%lld]: %d appears twice", (long long)r, p); return 1; }
      seen[(size_t)p] = 1;
    }
  }
  return 0;
}

// the permutations of one internal pass: a multiple of the batch, at most HOST_MANTEL_MAX_ROWS, with column terms (rows x Q x n
// doubles) of at most HOST_MANTEL_TERM_CAP bytes -- but never less than one batch
static inline int64_t host_mantel_pass_rows(int64_t n, int Q) {
  int64_t rows = std::min<int64_t>(HOST_MANTEL_MAX_ROWS, HOST_MANTEL_TERM_CAP / (n * 8 * Q));
  rows = rows / HOST_MANTEL_BATCH * HOST_MANTEL_BATCH;
  return std::max<int64_t>(rows, HOST_MANTEL_BATCH);
}

// device scratch of a call with R permutations (the matrices themselves not counted): the permutations, their inverses, the
// column terms and the sums of one pass.  -1 on a bad size
static inline int64_t host_mantel_scratch_bytes(int64_t n, int64_t R, int Q) {
  if (!host_mantel_size_ok(n, R, Q)) return -1;
  const int64_t rows = std::min(host_mantel_pass_rows(n, Q), std::max<int64_t>(R, 1));
  return rows * n * 4 * 2 + rows * Q * n * 8 + rows * Q * 8;
}

// `rows` checked permutations -> inv[r n + perms[r n + i]] = i
static inline void host_mantel_inverse(int64_t n, const int32_t* perms, int64_t rows, int32_t* inv) {
  for (int64_t r = 0; r < rows; r++)
    for (int64_t i = 0; i < n; i++) inv[r * n + perms[r * n + i]] = (int32_t)i;
}

// ---- tpg_mantel_perms --------------------------------------------------------------------------------------------------------------
// Rows r0 .. r0 + R - 1 of the permutation list (include/tpg.h "Mantel tests"): 0 = fine, 1 = a bad argument described in msg
// (nothing written).  out is R x n.
static inline int host_mantel_perms(int64_t n, const int32_t* strata0, int nstrata, uint64_t seed, int64_t r0, int64_t R, int32_t* out,
                                    char* msg, size_t cap) {
  if (n < 1 || n > HOST_MANTEL_MAX_N) { snprintf(msg, cap, "n = %lld out of [1, TPG_MANTEL_MAX_N = %d]", (long long)n, HOST_MANTEL_MAX_N); return 1; }
  if (R < 0 || r0 < 0 || r0 > ((int64_t)1 << 31) || R > ((int64_t)1 << 31) - r0) {
    snprintf(msg, cap, "rows [%lld, %lld + %lld) out of [0, 2^31)", (long long)r0, (long long)r0, (long long)R);
    return 1;
  }
  if (strata0) {
    if (nstrata < 1) { snprintf(msg, cap, "nstrata must be positive"); return 1; }
    for (int64_t i = 0; i < n; i++)
      if (strata0[i] < 0 || strata0[i] >= nstrata) {
        snprintf(msg, cap, "strata[%lld] = %d out of [0,%d)", (long long)i, strata0[i], nstrata);
        return 1;
      }
  }
  if (R > 0 && !out) { snprintf(msg, cap, "null output"); return 1; }
  // the members of every stratum in ascending order, stratum after stratum
  const int ns = strata0 ? nstrata : 1;
  std::vector<int64_t> start((size_t)ns + 1, 0);
  std::vector<int32_t> member((size_t)n);
  for (int64_t i = 0; i < n; i++) start[(size_t)(strata0 ? strata0[i] : 0) + 1]++;
  for (int s = 0; s < ns; s++) start[(size_t)s + 1] += start[(size_t)s];
  {
    std::vector<int64_t> at(start.begin(), start.end() - 1);
    for (int64_t i = 0; i < n; i++) member[(size_t)at[(size_t)(strata0 ? strata0[i] : 0)]++] = (int32_t)i;
  }
  typedef std::pair<uint64_t, int32_t> KI;
  auto some_rows = [&](int64_t k0, int64_t k1) {
    std::vector<KI> keys((size_t)n);
    for (int64_t k = k0; k < k1; k++) {
      const int64_t r = r0 + k;
      int32_t* pi = out + k * n;
      if (r == 0) {  // the identity, not hashed
        for (int64_t i = 0; i < n; i++) pi[i] = (int32_t)i;
        continue;
      }
      for (int64_t t = 0; t < n; t++) {
        const int32_t e = member[(size_t)t];
        keys[(size_t)t] = KI(tpg_mix64(seed ^ tpg_mix64(((uint64_t)r << 32) + (uint64_t)e)), e);
      }
      for (int s = 0; s < ns; s++) {  // sigma = the members sorted by (key, index); pi(sigma_t) = e_t
        const int64_t a = start[(size_t)s], b = start[(size_t)s + 1];
        std::sort(keys.begin() + a, keys.begin() + b);
        for (int64_t t = a; t < b; t++) pi[keys[(size_t)t].second] = member[(size_t)t];
      }
    }
  };
  // A row is a function of r alone, so the rows are dealt to a few threads when there is enough to sort (a list of 1 000
  // permutations of 5 000 individuals took one thread longer than the device took for their sums)
  int64_t nt = std::min<int64_t>(HOST_MANTEL_PERM_THREADS, std::min<int64_t>(R / 16, (R * n) >> 16));
  nt = std::min<int64_t>(nt, (int64_t)std::thread::hardware_concurrency());
  if (nt < 2) {
    some_rows(0, R);
  } else {
    // a thread that cannot be started (a limit on threads) is no error of the call: the caller does its share of the rows
    std::vector<std::thread> team;
    team.reserve((size_t)nt);
    int64_t done = 0;  // rows handed to a thread
    for (int64_t w = 0; w + 1 < nt; w++) {
      const int64_t k1 = R * (w + 1) / nt;
      try {
        team.emplace_back(some_rows, done, k1);
      } catch (...) {
        break;
      }
      done = k1;
    }
    some_rows(done, R);
    for (auto& th : team) th.join();
  }
  return 0;
}

// ---- the finishers -----------------------------------------------------------------------------------------------------------------
// r = (Sab - Sa Sb / N) / sqrt((Saa - Sa^2 / N)(Sbb - Sb^2 / N)); NaN where a variance is not positive, or N < 1
static inline double host_mantel_from_sums(int64_t N, double Sa, double Saa, double Sb, double Sbb, double Sab) {
  if (N < 1) return NAN;
  const double Nd = (double)N;
  const double mab = Sa * Sb;
  const double cab = Sab - mab / Nd;
  const double maa = Sa * Sa;
  const double va = Saa - maa / Nd;
  const double mbb = Sb * Sb;
  const double vb = Sbb - mbb / Nd;
  if (!(va > 0.0) || !(vb > 0.0)) return NAN;
  const double den = sqrt(va * vb);
  return cab / den;
}

// (r_ab - r_ac r_bc) / sqrt((1 - r_ac^2)(1 - r_bc^2)); NaN where a factor is not positive
static inline double host_mantel_partial(double r_ab, double r_ac, double r_bc) {
  const double fa = 1.0 - r_ac * r_ac;
  const double fb = 1.0 - r_bc * r_bc;
  if (!(fa > 0.0) || !(fb > 0.0)) return NAN;
  const double num = r_ab - r_ac * r_bc;
  const double den = sqrt(fa * fb);
  return num / den;
}
