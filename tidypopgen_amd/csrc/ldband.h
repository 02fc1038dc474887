// ldband.h -- the banded L x L' contraction that LD clumping (ld.hip), LD-kNN imputation (knnimp.hip) and the LD statistics
// (ldstat.hip) share; included by those three files only.
//
// Sxy = sum_i x_j x_k of two neighbouring loci is a locus x locus product over the individuals, i.e. over the Q groups of the
// locus-tiled layout L, with L as BOTH operands.  A 2-bit code c in the low bits of a nibble is the FP4 (E2M1) value c / 2, so
// with a block scale of 2 on either side the scaled MFMA adds up the dosage products of 32 x 32 locus pairs and 64 individuals:
// products in {0, 1, 2, 4}, sums of at most 4 n, exact in FP32 below 2^24 for every n < TPG_BAND_MAX_N.  The padding individuals
// of the last group carry code 3: that group's fragments have their 3s cleared before use (tpg_clear3).
//
// A workgroup of four waves owns the 32 loci of row tile jt and walks the column tiles jt .. jt + NT - 1 that meet the band of
// its rows in super-chunks of TPG_BAND_SC; wave wv holds the accumulators of tiles wv, wv + 4, ... of the chunk.  What becomes
// of the sums -- link bits, int32 band entries -- and how many super-chunks there are is the calling kernel's business.
#pragma once
#include "devfrag.h"

#define TPG_BAND_MAX_N (1ll << 22)
#define TPG_BAND_TK 4                    // column tiles per wave and super-chunk (4 x 16 accumulator registers)
#define TPG_BAND_SC (4 * TPG_BAND_TK)    // column tiles per workgroup and super-chunk

// column tiles jt .. jt + NT - 1 meet the band of row tile jt (hi[j]: the last neighbour of locus j)
__device__ __forceinline__ int tpg_band_tiles(const int64_t* __restrict__ hi, int64_t jt, int64_t m) {
  const int64_t j0 = jt * 32, jlast = j0 + 31 < m ? j0 + 31 : m - 1;
  return (int)((hi[jlast] >> 5) - jt) + 1;
}

// Super-chunk sc of row tile jt.  The tiles of wave wv lie at the offsets sc * 4 TK + wv + 4 i from jt, and the first nt of them
// inside the band: the 32 x 32 sums of tile i < nt are added to acc[i], in the MFMA C/D layout (tpg_cd_row); the others are left
// alone.  The CALLER zeroes acc (all TK of them, just before the call): zeroed in here, through the reference, the accumulators
// get copies in the K loop (48 more AGPRs, one wave per SIMD less for tpg_ld_band_kernel).  Returns nt, the same on every lane.
template <int TK>
__device__ __forceinline__ int tpg_band_contract(const uint4* __restrict__ L, int64_t Q, int64_t jt, int NT, int sc, int wv, int lane,
                                                 v16f (&acc)[TK]) {
  const int Qi = (int)Q;
  const char* pa = (const char*)(L + (jt * Q) * 64);
  auto LDG = [&](const char* p, int q) {
    const uint32_t off = (uint32_t)lane * 16u + (uint32_t)q * 1024u;
    return *(const uint4*)(p + off);
  };
  const int t0 = sc * 4 * TK + wv;
  const int nt = __builtin_amdgcn_readfirstlane(NT > t0 ? (NT - t0 + 3) / 4 < TK ? (NT - t0 + 3) / 4 : TK : 0);
  if (nt > 0) {
    const char* pb[TK];
#pragma unroll
    for (int i = 0; i < TK; i++) pb[i] = (const char*)(L + ((jt + t0 + 4 * (i < nt ? i : 0)) * Q) * 64);
    uint4 an = LDG(pa, 0), bn[TK];
#pragma unroll
    for (int i = 0; i < TK; i++)
      if (i < nt) bn[i] = LDG(pb[i], 0);
    for (int q = 0; q < Qi; q++) {
      uint4 a = an;
      uint4 b[TK];
#pragma unroll
      for (int i = 0; i < TK; i++)
        if (i < nt) b[i] = bn[i];
      if (q == Qi - 1) {  // the group with the padding individuals
        tpg_clear3(a);
#pragma unroll
        for (int i = 0; i < TK; i++)
          if (i < nt) tpg_clear3(b[i]);
      }
      const int qn = q + 1 < Qi ? q + 1 : q;
      an = LDG(pa, qn);
#pragma unroll
      for (int i = 0; i < TK; i++)
        if (i < nt) bn[i] = LDG(pb[i], qn);
#pragma unroll
      for (int S = 0; S < 2; S++) {
        uint32_t fa[4];
        tpg_l_halfgroup_operand(a, S, fa);
#pragma unroll
        for (int i = 0; i < TK; i++)
          if (i < nt) {
            uint32_t fb[4];
            tpg_l_halfgroup_operand(b[i], S, fb);
            // FP4 x FP4, both block scales 2^1: (c_j / 2 * 2) * (c_k / 2 * 2)
            acc[i] = tpg_mfma_f4(fa, fb, acc[i], (int)0x80808080, (int)0x80808080);
          }
      }
    }
  }
  return nt;
}
