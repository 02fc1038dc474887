// fstperm.hip -- Fst under relabelings (include/tpg.h "Fst under relabelings"): the sums of the per-locus Fst numerators and
// denominators of R relabelings of the individuals at once, for permutation tests.  The reference has nothing of the kind.
//
//  * fstperm_onehot_kernel: the multi-label one-hot.  The operand layout of tpg_onehot_kernel (loci.hip) with
//    class = class group * 64 + slot * G + label (host/host_fstperm.h): every relabeling is G columns of one 64-column group.
//  * fstperm_fused_kernel: the FP4 MFMA contraction over individuals of tpg_grouped_counts_kernel (planes Y / Z / W of the
//    2-bit code, het = sum Y - sum W, hom-alt = sum Z - sum W, valid = class size - sum W) with the Fst terms in its epilogue.
//    A workgroup owns one class group (64 columns, two MFMA class tiles) and four consecutive spans of FP_S loci, one per
//    wave; the four waves share the one-hot fragments of a 128-individual group through double-buffered LDS as the counts
//    kernel does.  After the contraction of a 32-locus tile a wave turns its accumulators into the integer counts of 16 loci
//    x 64 classes in its own LDS block (twice per tile), and its lanes take (relabeling, pair, unit) tasks: two lanes per
//    (relabeling, pair), one per unit of FP_U = 8 loci.  A lane forms the terms of its unit with fst_stage / fst_terms
//    (fst_terms.h, statement for statement, no FMA contraction) and adds the kept ones in ascending locus order; the even
//    lane adds the two unit sums, lower unit first, to the span sum.  The first 32 (relabeling, pair) items of a workgroup
//    keep their span sums in registers; further ones keep them in the partial array itself (read, add, write: one owner, no
//    atomics).  Only one pair of doubles and one count per (relabeling, pair, span) leave the kernel.
//  * fstperm_reduce_kernel adds the spans in ascending order.
// Nothing here depends on the batch: a relabeling's sums are formed from its own columns in an order fixed by the locus index.
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "devfrag.h"
#include "fst_terms.h"
#include "host/host_fstperm.h"

#define FP_U TPG_FSTPERM_UNIT_LOCI
#define FP_S TPG_FSTPERM_SPAN_LOCI
#define FP_GT 2                      // class tiles of a workgroup
#define FP_PH 16                     // loci staged per epilogue phase: two units
#define FP_CP 65                     // LDS stride of a staged locus (64 classes + 1: the two halves of a wave hit different banks)
#define FP_D 4                       // genotype blocks in flight (GC_D of loci.hip)
#define FP_MAX_ROWS 4096             // relabelings per internal batch at most ...
#define FP_MAX_CLASS_GROUPS 512      // ... class groups at most (the one-hot scratch is 4 Q KiB per class group) ...
#define FP_PART_CAP (256ll << 20)    // ... and bytes of span partials at most (unless one class group alone takes more)
static_assert(32 % FP_U == 0 && FP_S % 128 == 0 && FP_PH == 2 * FP_U && HOST_FSTPERM_TILE == 32 * FP_GT, "the epilogue's task shape");
static_assert(TPG_FSTPERM_MAX_GROUPS == HOST_FSTPERM_MAX_GROUPS, "one limit");

__global__ void fstperm_onehot_kernel(const int8_t* __restrict__ lab8, int64_t n, int64_t Q, int rows, int G, int GT_total,
                                      uint4* __restrict__ OH) {
  const int64_t total = Q * 2 * GT_total * 64;
  const int slots = HOST_FSTPERM_TILE / G;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(idx & 63);
    const int64_t t = idx >> 6;
    const int gt = (int)(t % GT_total);
    const int64_t qS = t / GT_total;
    const int S = (int)(qS & 1);
    const int64_t q = qS >> 1;
    const int c = 32 * gt + (lane & 31), h = lane >> 5;
    const int col = c % HOST_FSTPERM_TILE, slot = col / G, l = col % G;
    const int64_t b = (int64_t)(c / HOST_FSTPERM_TILE) * slots + slot;
    uint32_t w[4] = {0, 0, 0, 0};
    if (slot < slots && b < rows) {
      const int8_t* row = lab8 + b * n;
      for (int d = 0; d < 4; d++)
        for (int j = 0; j < 8; j++) {
          const int e = (j >> 1) + 8 * (j & 1) + 4 * (d & 1);
          const int64_t i = 128 * q + 32 * (2 * S + (d >> 1)) + 16 * h + e;
          if (i < n && row[i] == l) w[d] |= 2u << (4 * j);
        }
    }
    OH[idx] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// the lanes of ONE wave exchange data through LDS: order the accesses, no workgroup barrier
__device__ __forceinline__ void fp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int METHOD>
__global__ __launch_bounds__(256, 2) void fstperm_fused_kernel(const uint4* __restrict__ L, const uint4* __restrict__ OH, int64_t n_lt,
                                                               int64_t Q, int64_t m, int GT_total, const int32_t* __restrict__ csize,
                                                               int G, int rows, const int32_t* __restrict__ pairs0, int P,
                                                               int64_t nspans, double* __restrict__ part_num,
                                                               double* __restrict__ part_den, int32_t* __restrict__ part_cnt) {
  constexpr int GT = FP_GT;
  __shared__ __attribute__((aligned(16))) uint4 ohb[2][2 * GT][64];  // [buffer][step * GT + class tile][lane]
  __shared__ int32_t cnt_s[4][3 * FP_PH * FP_CP];                     // per wave: [plane][locus of the phase][class]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int cg = blockIdx.y, gt0 = GT * cg;
  const int64_t span = (int64_t)blockIdx.x * 4 + wv;
  const bool live = span < nspans;
  const int slots = HOST_FSTPERM_TILE / G;
  const int nrow = rows - cg * slots < slots ? rows - cg * slots : slots;
  const int nitems = nrow * P, nrounds = (2 * nitems + 63) / 64;
  int cs[GT];
#pragma unroll
  for (int g = 0; g < GT; g++) cs[g] = csize[cg * HOST_FSTPERM_TILE + 32 * g + (lane & 31)];
  int32_t* const cnt_w = cnt_s[wv];
  const FstSrc src{cnt_w, FP_PH, FP_CP, 0, nullptr, nullptr, nullptr, nullptr};
  double a_n = 0.0, a_d = 0.0;  // the span sums of item lane >> 1 (round 0), on the even lane
  int a_c = 0;

  const int Qi = (int)Q;
  constexpr int NIT = (2 * GT + 3) / 4;
  const char* po = (const char*)(OH + (int64_t)gt0 * 64);
  auto frag = [&](int q, int it) {
    const int64_t off = ((int64_t)(q * 2 + it / GT) * GT_total + it % GT) * 1024 + lane * 16;
    return *(const uint4*)(po + off);
  };

  for (int ti = 0; ti < FP_S / 32; ti++) {
    // every wave of the workgroup runs every tile step (they meet at the barriers of the one-hot exchange); the workgroup stops
    // when the tile of its FIRST wave lies past the loci, as the other waves' tiles lie further still
    if (((int64_t)blockIdx.x * 4 * (FP_S / 32) + ti) * 32 >= m) break;
    const int64_t lt = span * (FP_S / 32) + ti;
    const bool tile_live = live && lt * 32 < m;
    const int64_t ltu = tpg_uniform64(lt < n_lt ? lt : 0);  // past the end: a copy of tile 0, never used
    const char* pa = (const char*)(L + (ltu * Q) * 64);
    auto LDG = [&](int q) {
      uint32_t off = (uint32_t)lane * 16u + (uint32_t)q * 1024u;
      asm("" : "+v"(off));
      return *(const uint4*)(pa + off);
    };
    v16f acc[3][GT];
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
      for (int g = 0; g < GT; g++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[p][g][r] = 0.f;
    // ---- the contraction over individuals: tpg_grouped_counts_kernel's loop (loci.hip has the account of its staging)
    uint4 R[FP_D], on[2][NIT];
#pragma unroll
    for (int d = 0; d < FP_D - 1; d++) R[d] = LDG(d < Qi ? d : Qi - 1);
#pragma unroll
    for (int j = 0; j < NIT; j++) {
      const int it = wv + 4 * j;
      if (it < 2 * GT) {
        ohb[0][it][lane] = frag(0, it);
        on[1][j] = frag(Qi > 1 ? 1 : 0, it);
      }
    }
    tpg_lds_barrier();
    auto group = [&](auto Cc, auto Mm, int q) {
      constexpr int C = decltype(Cc)::value, M = decltype(Mm)::value;
      static_assert(FP_D % 2 == 0, "the slot of a group's fragments is its parity, known at compile time in the unrolled loop");
      const int qn2 = q + FP_D - 1 < Qi ? q + FP_D - 1 : Qi - 1, qo2 = q + 2 < Qi ? q + 2 : Qi - 1;
      const int cur = q & 1;
      R[M] = LDG(qn2);
#pragma unroll
      for (int j = 0; j < NIT; j++) {
        const int it = wv + 4 * j;
        if (it < 2 * GT) on[C & 1][j] = frag(qo2, it);
      }
#pragma unroll
      for (int S = 0; S < 2; S++) {
        uint32_t fy[4], fz[4], fw[4];
        const uint32_t Pw[2] = {S == 0 ? R[C].x : R[C].z, S == 0 ? R[C].y : R[C].w};
#pragma unroll
        for (int d = 0; d < 4; d++) {
          const uint32_t X = (d & 1) ? (Pw[d >> 1] >> 2) & 0x33333333u : Pw[d >> 1] & 0x33333333u;
          fy[d] = X & 0x11111111u;
          fz[d] = X & 0x22222222u;
          fw[d] = fy[d] & (fz[d] >> 1);
        }
#pragma unroll
        for (int g = 0; g < GT; g++) {
          const uint4 b = ohb[cur][S * GT + g][lane];
          acc[0][g] = tpg_mfma_f4(fy, b, acc[0][g], (int)0x80808080, 0x7F7F7F7F);
          acc[1][g] = tpg_mfma_f4(fz, b, acc[1][g], 0x7F7F7F7F, 0x7F7F7F7F);
          acc[2][g] = tpg_mfma_f4(fw, b, acc[2][g], (int)0x80808080, 0x7F7F7F7F);
        }
      }
      // the other buffer was last read in group q - 1, which every wave left through the barrier below
#pragma unroll
      for (int j = 0; j < NIT; j++) {
        const int it = wv + 4 * j;
        if (it < 2 * GT) ohb[cur ^ 1][it][lane] = on[(C & 1) ^ 1][j];
      }
      tpg_lds_barrier();
    };
    for (int q = 0; q < Qi; q += FP_D)  // Q is the same for every wave: all of them meet every barrier
      tpg_static_for<FP_D>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        if (q + k < Qi) group(std::integral_constant<int, k>{}, std::integral_constant<int, (k + FP_D - 1) % FP_D>{}, q + k);
      });
    if (!tile_live) continue;  // (no workgroup barrier below this line of the step)

    // ---- the epilogue: integer counts of 16 loci x 64 classes at a time, then the terms in unit order
    tpg_static_for<32 / FP_PH>([&](auto phc) {
      constexpr int ph = decltype(phc)::value;
#pragma unroll
      for (int g = 0; g < GT; g++)
#pragma unroll
        for (int rr = 0; rr < 8; rr++) {
          constexpr int plane = FP_PH * FP_CP;
          const int r = 8 * ph + rr;  // tpg_cd_row(r, lane) = 16 ph + row
          const int row = (rr & 3) + 8 * (rr >> 2) + 4 * (lane >> 5);
          const int o = row * FP_CP + 32 * g + (lane & 31);
          const int nmiss = (int)acc[2][g][r];
          cnt_w[o] = (int)acc[0][g][r] - nmiss;
          cnt_w[plane + o] = (int)acc[1][g][r] - nmiss;
          cnt_w[2 * plane + o] = cs[g] - nmiss;
        }
      fp_wave_sync();
      for (int round = 0; round < nrounds; round++) {
        const int tt = lane + 64 * round, it = tt >> 1, half = tt & 1;
        const bool active = it < nitems;
        double un = 0.0, ud = 0.0;  // the unit's sums: kept terms in ascending locus order from 0.0
        int uc = 0;
        int s = 0, p = 0;
        if (active) {
          s = it / P;
          p = it - s * P;
          const int c1 = s * G + pairs0[2 * p], c2 = s * G + pairs0[2 * p + 1];
          const int64_t j0 = lt * 32 + FP_PH * ph + FP_U * half;
#pragma unroll 2
          for (int l = 0; l < FP_U; l++) {
            if (j0 + l >= m) break;
            const int jl = FP_U * half + l;
            double n1, p1, h1, n2, p2, h2, e1 = 0.0, e2 = 0.0, num, den;
            fst_stage(src, 0, jl, c1, n1, p1, h1);
            fst_stage(src, 0, jl, c2, n2, p2, h2);
            if (METHOD == TPG_FST_HUDSON) {  // (p q) / (n - 1), as tpg_fst_kernel stages it
              e1 = (p1 * (1 - p1)) / (n1 - 1);
              e2 = (p2 * (1 - p2)) / (n2 - 1);
            }
            fst_terms<METHOD, false>(n1, p1, h1, e1, n2, p2, h2, e2, num, den);
            if (num == num && den == den) { un += num; ud += den; uc++; }
          }
        }
        // the upper unit's sums come down to the even lane, which adds the two to the span sum, lower unit first
        const double on_ = __shfl_down(un, 1), od_ = __shfl_down(ud, 1);
        const int oc_ = __shfl_down(uc, 1);
        if (active && half == 0) {
          if (round == 0) {
            a_n += un; a_n += on_;
            a_d += ud; a_d += od_;
            a_c += uc + oc_;
          } else {
            const int64_t o = (span * rows + (cg * slots + s)) * (int64_t)P + p;
            const bool first = ti == 0 && ph == 0;
            double xn = first ? 0.0 : part_num[o], xd = first ? 0.0 : part_den[o];
            const int xc = first ? 0 : part_cnt[o];
            xn += un; xn += on_;
            xd += ud; xd += od_;
            part_num[o] = xn;
            part_den[o] = xd;
            part_cnt[o] = xc + uc + oc_;
          }
        }
      }
      fp_wave_sync();  // the next phase writes the block again
    });
  }
  if (live && (lane & 1) == 0 && (lane >> 1) < nitems) {
    const int it = lane >> 1, s = it / P, p = it - s * P;
    const int64_t o = (span * rows + (cg * slots + s)) * (int64_t)P + p;
    part_num[o] = a_n;
    part_den[o] = a_d;
    part_cnt[o] = a_c;
  }
}

// the span sums of a (relabeling, pair) cell in ascending order from 0.0
__global__ void fstperm_reduce_kernel(const double* __restrict__ part_num, const double* __restrict__ part_den,
                                      const int32_t* __restrict__ part_cnt, int64_t nspans, int64_t cells, double* __restrict__ sum_num,
                                      double* __restrict__ sum_den, int64_t* __restrict__ n_kept) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= cells) return;
  double sn = 0.0, sd = 0.0;
  int64_t k = 0;
  for (int64_t s = 0; s < nspans; s++) {
    sn += part_num[s * cells + c];
    sd += part_den[s * cells + c];
    k += part_cnt[s * cells + c];
  }
  sum_num[c] = sn;
  sum_den[c] = sd;
  n_kept[c] = k;
}

// ---------------------------------------------------------------------------
struct FpPlan {
  int64_t rows_max = 0, ncg = 0, nspans = 0;
  size_t b_lab = 0, b_csize = 0, b_oh = 0, b_part = 0, b_out = 0, b_pairs = 0;
  size_t bytes() const { return b_lab + b_csize + b_oh + b_part + b_out + b_pairs; }
};
// the scratch of `rows` relabelings in one batch (rows <= 0: of the largest batch the library forms)
static FpPlan fp_plan(int64_t n, int64_t m, int G, int P, int64_t rows) {
  FpPlan pl;
  const int64_t slots = host_fstperm_slots(G), Q = ceil_div(n, 128);
  pl.nspans = ceil_div(m, FP_S);
  const int64_t per_row = std::max<int64_t>(1, pl.nspans) * P * 20;
  int64_t rmax = std::min<int64_t>(std::min<int64_t>(FP_MAX_ROWS, FP_MAX_CLASS_GROUPS * slots), FP_PART_CAP / per_row);
  rmax = std::max<int64_t>(slots, rmax / slots * slots);
  pl.rows_max = rows > 0 ? std::min(rows, rmax) : rmax;
  pl.ncg = host_fstperm_class_groups(pl.rows_max, G);
  pl.b_lab = (size_t)pl.rows_max * (size_t)n;
  pl.b_csize = sizeof(int32_t) * (size_t)pl.ncg * HOST_FSTPERM_TILE;
  pl.b_oh = sizeof(uint4) * (size_t)Q * 2 * (size_t)(FP_GT * pl.ncg) * 64;
  pl.b_part = (size_t)pl.nspans * (size_t)pl.rows_max * (size_t)P * 20;
  pl.b_out = (size_t)pl.rows_max * (size_t)P * 24;
  pl.b_pairs = sizeof(int32_t) * 2 * (size_t)P;
  return pl;
}

extern "C" int64_t tpg_fstperm_unit_loci(void) { return FP_U; }
extern "C" int64_t tpg_fstperm_span_loci(void) { return FP_S; }

extern "C" int64_t tpg_fst_relabel_scratch_bytes(int64_t n, int64_t m, int ngroups, int P) {
  if (n < 1 || n >= (1 << 24) || m < 0 || ngroups < 2 || ngroups > TPG_FSTPERM_MAX_GROUPS || P < 1) return -1;
  return (int64_t)fp_plan(n, m, ngroups, P, 0).bytes();
}

extern "C" int tpg_fst_perm_labels(int64_t n, const int32_t* groupIds0, int ngroups, int scheme, int a, int b, uint64_t seed, int64_t r,
                                   int32_t* out) {
  char msg[256];
  if (host_fstperm_labels(n, groupIds0, ngroups, scheme, a, b, seed, r, out, msg, sizeof(msg))) {
    tpg_set_error("%s", msg);
    return TPG_EINVAL;
  }
  return TPG_OK;
}

extern "C" int tpg_fst_relabel_sums(tpg_ctx* ctx, const tpg_view* v, const int32_t* labels, int64_t R, int ngroups, int method,
                                    const int32_t* pairs1, int P, double* sum_num, double* sum_den, int64_t* n_kept) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v, TPG_EINVAL, "null argument");
  TPG_REQUIRE(method == TPG_FST_HUDSON || method == TPG_FST_NEI87 || method == TPG_FST_WC84, TPG_EINVAL, "unknown Fst method %d", method);
  char msg[320];
  if (host_fstperm_check(v->n, labels, R, ngroups, pairs1, P, msg, sizeof(msg))) {
    tpg_set_error("%s", msg);
    return TPG_EINVAL;
  }
  if (R == 0) return TPG_OK;
  TPG_REQUIRE(sum_num && sum_den, TPG_EINVAL, "null output");
  TPG_REQUIRE(v->n < (1 << 24), TPG_EUNSUPPORTED, "relabelled counts of more than 2^24 individuals");  // FP32 sums of ones
  TPG_REQUIRE(v->m > 0, TPG_EINVAL, "a view without loci");
  const int G = ngroups;
  const int64_t n = v->n, m = v->m;
  const FpPlan pl = fp_plan(n, m, G, P, R);
  TPG_REQUIRE((int64_t)pl.bytes() <= tpg_fst_relabel_scratch_bytes(n, m, G, P), TPG_EHIP,
              "the scratch of the call (%zu bytes) exceeds what tpg_fst_relabel_scratch_bytes reports", pl.bytes());
  const int64_t cells_max = pl.rows_max * P;
  DevArena sc;
  int8_t* d_lab = nullptr;
  int32_t *d_csize = nullptr, *d_pairs = nullptr, *d_pc = nullptr;
  uint4* d_oh = nullptr;
  double *d_pn = nullptr, *d_pd = nullptr, *d_on = nullptr, *d_od = nullptr;
  int64_t* d_ok = nullptr;
  TPG_TRY(sc.get(&d_lab, pl.b_lab));
  TPG_TRY(sc.get(&d_csize, (size_t)pl.ncg * HOST_FSTPERM_TILE));
  TPG_TRY(sc.get(&d_oh, (size_t)v->Q * 2 * (size_t)(FP_GT * pl.ncg) * 64));
  TPG_TRY(sc.get(&d_pn, (size_t)pl.nspans * (size_t)cells_max));
  TPG_TRY(sc.get(&d_pd, (size_t)pl.nspans * (size_t)cells_max));
  TPG_TRY(sc.get(&d_pc, (size_t)pl.nspans * (size_t)cells_max));
  TPG_TRY(sc.get(&d_on, (size_t)cells_max));
  TPG_TRY(sc.get(&d_od, (size_t)cells_max));
  TPG_TRY(sc.get(&d_ok, (size_t)cells_max));
  TPG_TRY(sc.get(&d_pairs, (size_t)2 * P));
  std::vector<int32_t> p0((size_t)2 * P);
  for (int k = 0; k < 2 * P; k++) p0[(size_t)k] = pairs1[k] - 1;
  TPG_HIP(tpg_h2d_async(ctx, d_pairs, p0.data(), sizeof(int32_t) * p0.size()));
  TPG_TRY(tpg_view_need_L(ctx, v));
  std::vector<int8_t> lab8((size_t)pl.rows_max * (size_t)n);
  std::vector<int32_t> csize((size_t)pl.ncg * HOST_FSTPERM_TILE);
  const int64_t n_lt = v->KG * 4;
  for (int64_t r0 = 0; r0 < R; r0 += pl.rows_max) {
    const int64_t rows = std::min(pl.rows_max, R - r0), ncg = host_fstperm_class_groups(rows, G), cells = rows * P;
    const int GT_total = (int)(FP_GT * ncg);
    host_fstperm_pack(n, labels + r0 * n, rows, G, lab8.data(), csize.data());
    TPG_HIP(tpg_upload(ctx, d_lab, lab8.data(), (size_t)rows * (size_t)n));
    TPG_HIP(tpg_upload(ctx, d_csize, csize.data(), sizeof(int32_t) * (size_t)ncg * HOST_FSTPERM_TILE));
    TPG_LAUNCH(ctx, "fstperm_onehot", fstperm_onehot_kernel, dim3(1024), dim3(256), 0, (const int8_t*)d_lab, n, v->Q, (int)rows, G,
               GT_total, d_oh);
    const dim3 grid((unsigned)ceil_div(pl.nspans, 4), (unsigned)ncg);
#define FP_LAUNCH(M, NAME)                                                                                                          \
  TPG_LAUNCH(ctx, NAME, fstperm_fused_kernel<M>, grid, dim3(256), 0, (const uint4*)v->L, (const uint4*)d_oh, n_lt, v->Q, m, GT_total, \
             (const int32_t*)d_csize, G, (int)rows, (const int32_t*)d_pairs, P, pl.nspans, d_pn, d_pd, d_pc)
    if (method == TPG_FST_HUDSON) FP_LAUNCH(TPG_FST_HUDSON, "fstperm_hudson");
    else if (method == TPG_FST_WC84) FP_LAUNCH(TPG_FST_WC84, "fstperm_wc84");
    else FP_LAUNCH(TPG_FST_NEI87, "fstperm_nei87");
#undef FP_LAUNCH
    TPG_LAUNCH(ctx, "fstperm_reduce", fstperm_reduce_kernel, dim3((unsigned)ceil_div(cells, 256)), dim3(256), 0, (const double*)d_pn,
               (const double*)d_pd, (const int32_t*)d_pc, pl.nspans, cells, d_on, d_od, d_ok);
    TPG_CHECK_LAUNCH();
    // (the downloads wait for the stream: the host staging is free for the next batch, the scratch for its kernels)
    TPG_TRY(tpg_deliver(ctx, sum_num + r0 * P, (const double*)d_on, (size_t)cells));
    TPG_TRY(tpg_deliver(ctx, sum_den + r0 * P, (const double*)d_od, (size_t)cells));
    if (n_kept) TPG_TRY(tpg_deliver(ctx, n_kept + r0 * P, (const int64_t*)d_ok, (size_t)cells));
  }
  TPG_HIP(hipStreamSynchronize(ctx->stream));  // the scratch of this call goes back to the pool at scope exit
  return TPG_OK;
}
