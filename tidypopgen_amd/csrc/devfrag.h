// devfrag.h -- device-side helpers for the 2-bit fragment layout (see common.h), and the one home of the fragment and wave
// primitives every kernel file shares: the MFMA vector types and the FP4 scaled-MFMA wrapper, the operand words of an L
// fragment, tpg_uniform64, tpg_static_for, tpg_wave_sum, the order-preserving key of a double, TPG_QNAN, the NaN-propagating
// maximum and the team-of-lanes adapter.  A kernel file that needs one of them includes this header; it does not copy it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef double v4d __attribute__((ext_vector_type(4)));

#define TPG_QNAN __longlong_as_double(0x7FF8000000000000ll)

// a wave-uniform value the compiler keeps in SGPRs
__device__ __forceinline__ int64_t tpg_uniform64(int64_t x) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// f(std::integral_constant<int, 0>) ... f(std::integral_constant<int, N - 1>), in ascending order
template <int N, class F>
__device__ __forceinline__ void tpg_static_for(F&& f) {
  if constexpr (N > 0) {
    tpg_static_for<N - 1>(f);
    f(std::integral_constant<int, N - 1>{});
  }
}

// the sum over the 64 lanes of a wave, on every lane: a butterfly over xor 32, 16, 8, 4, 2, 1.  For the integer counts only.
// The 64-bit and FP64 wave sums (pcadapt.hip, autosvd.hip, f2.hip, roh.hip, admix.hip, snmf.hip, admix_common.h) stay written
// out at their sites, in this same order: through a function their kernels came out with reordered instructions, and for the
// FP64 ones the order IS the result (the files built without FMA contraction state their sums by it).
__device__ __forceinline__ int tpg_wave_sum(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// Order-preserving 64-bit key of a double (u = its bits in an lvalue) and the inverse.  -0 and +0 get different keys: a caller
// that wants equal values to have equal keys adds 0.0 first (pcadapt.hip, autosvd.hip) or maps 0 to +0 itself (ld.hip).
// (u & TPG_D_EXP_MASK) == TPG_D_EXP_MASK: not finite.  The forward map is a macro so that its select compiles in place, inside
// whatever test of the mask the call site makes around it.
#define TPG_D_EXP_MASK 0x7FF0000000000000ull
#define TPG_DKEY(u) (((u) >> 63) ? ~(u) : ((u) | 0x8000000000000000ull))
__device__ __forceinline__ double tpg_dunkey(uint64_t key) {
  const uint64_t u = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
  return __longlong_as_double((long long)u);
}

// max(a, b), NaN if either is; and the same over sh[0 .. N - 1] of a workgroup of N threads (N a power of two), left in sh[0]
__device__ __forceinline__ double tpg_nanmax(double a, double b) { return (a != a || b != b) ? TPG_QNAN : (a > b ? a : b); }
template <int N>
__device__ __forceinline__ void tpg_block_nanmax(double* sh) {
  __syncthreads();
  for (int w = N / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] = tpg_nanmax(sh[threadIdx.x], sh[threadIdx.x + w]);
    __syncthreads();
  }
}

// G consecutive lanes of a single-wave workgroup as the team of the row-wise FP64 solvers (host/host_lsq.h, host/host_oadp.h):
// sync() is the workgroup barrier -- of that one wave -- and any() the barrier's OR
template <int G>
struct TpgTeam {
  __device__ int lane() const { return (int)(threadIdx.x % G); }
  __device__ int size() const { return G; }
  __device__ void sync() const { __syncthreads(); }
  __device__ bool any(bool b) const { return __syncthreads_or(b ? 1 : 0) != 0; }
};

// FP4 x FP4 (format code 4) scaled MFMA, 32 x 32 x 64: four operand dwords a side, widened to the eight the instruction
// names, and the two E8M0 block-scale words (one byte per 32 contracted elements; the call sites keep their own constants)
template <class V>
__device__ __forceinline__ v8i tpg_w8(const V& a) { return v8i{(int)a[0], (int)a[1], (int)a[2], (int)a[3], 0, 0, 0, 0}; }
__device__ __forceinline__ v8i tpg_w8(const uint4& a) { return v8i{(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0}; }
template <class A, class B>
__device__ __forceinline__ v16f tpg_mfma_f4(const A& a, const B& b, v16f c, int sa, int sb) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(tpg_w8(a), tpg_w8(b), c, 4, 4, 0, sa, 0, sb);
}

// the four FP4 operand dwords of half-group S (64 individuals) of one L fragment: eight codes each, in the low bits of the
// nibbles (a 2-bit code c there is the FP4 value c / 2).  Which individual lands in which nibble is the same for every locus,
// which is all a product of L with L needs.
__device__ __forceinline__ void tpg_l_halfgroup_operand(const uint4& f, int S, uint32_t (&o)[4]) {
  const uint32_t p0 = S == 0 ? f.x : f.z, p1 = S == 0 ? f.y : f.w;
  o[0] = p0 & 0x33333333u;
  o[1] = (p0 >> 2) & 0x33333333u;
  o[2] = p1 & 0x33333333u;
  o[3] = (p1 >> 2) & 0x33333333u;
}

// code 3 -> 0 in the 16 two-bit codes of a dword (the padding individuals of the last group)
__device__ __forceinline__ uint32_t tpg_clear3(uint32_t w) {
  const uint32_t miss = w & (w >> 1) & 0x55555555u;
  return w & ~(miss * 3u);
}
__device__ __forceinline__ void tpg_clear3(uint4& f) {
  f.x = tpg_clear3(f.x);
  f.y = tpg_clear3(f.y);
  f.z = tpg_clear3(f.z);
  f.w = tpg_clear3(f.w);
}

// v_perm_b32 used as a 4-entry byte lookup: selector bytes 0..3 pick bytes of `lut`.
// LUT byte c = value for code c (0,1,2 = dosage, 3 = missing).
#define TPG_LUT_V 0x00010101u   // valid:        1,1,1,0
#define TPG_LUT_H 0x00000100u   // heterozygous: 0,1,0,0
#define TPG_LUT_E2 0x00010000u  // hom alt:      0,0,1,0
#define TPG_LUT_D 0x000100FFu   // dosage - 1:  -1,0,1,0
#define TPG_LUT_G 0x00020100u   // dosage:       0,1,2,0

__device__ __forceinline__ uint32_t tpg_codes(uint32_t w, int k) { return (w >> (2 * k)) & 0x03030303u; }

__device__ __forceinline__ int tpg_lut(uint32_t lut, uint32_t codes) {
  return (int)__builtin_amdgcn_perm(0u, lut, codes);
}

// FP4 operand nibble of the pairwise kernel (pairwise.hip): one magnitude bit per operand plane -- 0x1 = FP4 0.5, 0x2 = 1.0,
// 0x4 = 2.0 -- for heterozygous (h), MISSING (m) and homozygous (d), bit 3 = the sign of d (dosage 0).  Which plane takes which
// magnitude does not change a single sum (the E8M0 block scales undo it: TPG_T4_SC_*), only the bit patterns the matrix cores
// multiply -- and their clock under the MFMAs is a POWER limit that depends on those (tools/pw_power_probe.py), so the
// assignment is a compile-time choice that was measured (TPG_T4_ENC, tools/enc_ab.py): 0 = h 0.5, m 1, d 2 (rounds 2 - 4).
// For the same reason the plane that three of the five products multiply marks the missing genotypes (a few percent of
// ones), not the typed ones: V = vv' and A = hv' are rebuilt from MM = mm' and HM = hm' by the epilogues (pairwise.hip).
#ifndef TPG_T4_ENC
#define TPG_T4_ENC 0
#endif
#if TPG_T4_ENC == 0
#define TPG_T4_MH 1u
#define TPG_T4_MM 2u
#define TPG_T4_MD 4u
#elif TPG_T4_ENC == 1
#define TPG_T4_MH 1u
#define TPG_T4_MM 4u
#define TPG_T4_MD 2u
#elif TPG_T4_ENC == 2
#define TPG_T4_MH 2u
#define TPG_T4_MM 1u
#define TPG_T4_MD 4u
#elif TPG_T4_ENC == 3
#define TPG_T4_MH 2u
#define TPG_T4_MM 4u
#define TPG_T4_MD 1u
#elif TPG_T4_ENC == 4
#define TPG_T4_MH 4u
#define TPG_T4_MM 1u
#define TPG_T4_MD 2u
#else
#define TPG_T4_MH 4u
#define TPG_T4_MM 2u
#define TPG_T4_MD 1u
#endif
// 2-bit code -> nibble: dosage 0 -> d | sign, 1 -> h, 2 -> d, missing (3) -> m  (0x0204010C for TPG_T4_ENC = 0).  PADDING
// (individuals >= n, loci >= m) is nibble 0: it contributes nothing to any plane.  The 2-bit layouts code padding as 3 like
// a missing genotype, so whoever makes nibbles tells the two apart by position (tpg_t4_keep).
#define TPG_NIB_LUT ((TPG_T4_MD | 8u) | ((TPG_T4_MH) << 8) | ((TPG_T4_MD) << 16) | ((TPG_T4_MM) << 24))
// E8M0 block scale (all four bytes equal) that turns a plane of magnitude bit M into 0 / +-1: 0.5 x 2, 1 x 1, 2 x 0.5
#define TPG_T4_SC(M) ((M) == 1u ? (int)0x80808080 : (M) == 2u ? 0x7f7f7f7f : 0x7e7e7e7e)
// byte mask of the elements 4 k + b (b = 0..3) of a T dword that lie inside the data when `left` elements of the dword do
__device__ __forceinline__ uint32_t tpg_t4_keep(int64_t left, int k) {
  const int64_t c = left - 4 * k;
  return c >= 4 ? 0xFFFFFFFFu : c <= 0 ? 0u : (1u << (8 * (int)c)) - 1u;
}
// one T dword (16 codes) -> two T4 dwords (16 nibbles); `left` = how many of its 16 elements are data (the rest is padding)
__device__ __forceinline__ void tpg_t4_words(uint32_t w, int64_t left, uint32_t& lo, uint32_t& hi) {
  uint32_t nb[4];
#pragma unroll
  for (int k = 0; k < 4; k++) nb[k] = (uint32_t)tpg_lut(TPG_NIB_LUT, tpg_codes(w, k)) & tpg_t4_keep(left, k);
  lo = nb[0] | (nb[1] << 4);
  hi = nb[2] | (nb[3] << 4);
}

// bit position of element e (0..15) inside a packed dword
__host__ __device__ __forceinline__ int tpg_elem_shift(int e) { return 8 * (e & 3) + 2 * (e >> 2); }

// The LM ("locus-major") form of the L layout (common.h): the same 16-byte pieces -- lane (r, h) of block (lt, q) -- with the
// 2 Q pieces of a locus next to each other, q-major then h.  Piece index of locus j = 32 lt + r:
__host__ __device__ __forceinline__ int64_t tpg_lm_piece(int64_t j, int64_t Q, int64_t q, int h) { return (j * Q + q) * 2 + h; }
// One task of the streaming transposition between the two: a workgroup of 256 threads takes the blocks (lt, q0 .. q0 + 3) of
// L, 4 KiB, through uint4 sh[32][8] = [locus in tile][2 (q - q0) + h].  On the L side thread t holds lane t & 63 of block
// q0 + (t >> 6): 1 KiB contiguous per wave; on the LM side piece p = t & 7 of locus r = t >> 3: 128 contiguous bytes per locus.
// Chunks q >= Q do not exist on either side (on = false).
struct TpgLmSide {
  int64_t piece;  // uint4 index in the layout
  int row, col;   // in sh
  bool on;
};
__device__ __forceinline__ int64_t tpg_lm_tasks(int64_t n_lt, int64_t Q) { return n_lt * ((Q + 3) / 4); }
__device__ __forceinline__ void tpg_lm_task(int64_t task, int64_t Q, int tid, TpgLmSide& l, TpgLmSide& lm) {
  const int64_t QG = (Q + 3) / 4, lt = task / QG, q0 = (task % QG) * 4;
  const int lane = tid & 63, wv = tid >> 6, r = tid >> 3, p = tid & 7;
  l = TpgLmSide{(lt * Q + q0 + wv) * 64 + lane, lane & 31, 2 * wv + (lane >> 5), q0 + wv < Q};
  lm = TpgLmSide{tpg_lm_piece(lt * 32 + r, Q, q0, 0) + p, r, p, q0 + (p >> 1) < Q};
}

// MFMA 32x32 C/D register -> row inside the 32x32 tile (col = lane & 31)
__device__ __forceinline__ int tpg_cd_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// Workgroup barrier for data exchanged through LDS only.  __syncthreads() also waits for every global load in
// flight (s_waitcnt vmcnt(0)), i.e. for the prefetch a K loop has just issued for its next iteration: a full memory
// latency per iteration.  The workgroup-scope fences order the LDS accesses (s_waitcnt lgkmcnt(0)) and leave vmcnt alone.
__device__ __forceinline__ void tpg_lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
