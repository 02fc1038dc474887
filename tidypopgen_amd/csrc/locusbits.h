// locusbits.h -- the two-bit codes of T dwords (common.h) as LOCUS-ORDERED bit masks: the fixed shuffle that roh.hip and
// ibdseg.hip read a row of T through (even bits together, then a 4 x 4 bit transpose).  A kernel file that needs it includes
// this header; it does not copy it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// bits 0, 2, .., 30 of x -> bits 0 .. 15
__device__ __forceinline__ uint32_t tpg_lb_even_bits(uint32_t x) {
  x &= 0x55555555u;
  x = (x | (x >> 1)) & 0x33333333u;
  x = (x | (x >> 2)) & 0x0f0f0f0fu;
  x = (x | (x >> 4)) & 0x00ff00ffu;
  x = (x | (x >> 8)) & 0x0000ffffu;
  return x;
}
// in either half: bit 4 b + k -> bit 4 k + b (element e = 4 k + b of a dword sits at bits 8 b + 2 k, common.h)
__device__ __forceinline__ uint32_t tpg_lb_transpose4(uint32_t x) {
  uint32_t t = (x ^ (x >> 3)) & 0x0a0a0a0au;
  x ^= t ^ (t << 3);
  t = (x ^ (x >> 6)) & 0x00cc00ccu;
  x ^= t ^ (t << 6);
  return x;
}
// the 16 codes of two dwords -> locus-ordered masks, dword a in the low half: opposite (code 1; with het: codes 0 and 2)
// and missing (code 3)
__device__ __forceinline__ void tpg_lb_opp_miss(uint32_t a, uint32_t b, int het, uint32_t& opp, uint32_t& miss) {
  const uint32_t la = a & 0x55555555u, ha = (a >> 1) & 0x55555555u;
  const uint32_t lb = b & 0x55555555u, hb = (b >> 1) & 0x55555555u;
  const uint32_t oa = het ? la ^ 0x55555555u : la & ~ha, ob = het ? lb ^ 0x55555555u : lb & ~hb;
  opp = tpg_lb_transpose4(tpg_lb_even_bits(oa) | (tpg_lb_even_bits(ob) << 16));
  miss = tpg_lb_transpose4(tpg_lb_even_bits(la & ha) | (tpg_lb_even_bits(lb & hb) << 16));
}
// the same for the two bit planes of the codes themselves: lo = bit 0 of every code, hi = bit 1
__device__ __forceinline__ void tpg_lb_planes(uint32_t a, uint32_t b, uint32_t& lo, uint32_t& hi) {
  lo = tpg_lb_transpose4(tpg_lb_even_bits(a) | (tpg_lb_even_bits(b) << 16));
  hi = tpg_lb_transpose4(tpg_lb_even_bits(a >> 1) | (tpg_lb_even_bits(b >> 1) << 16));
}
// The masks of lanes r and r + 32 of a fragment block -> the four words (32 loci each) of individual r in that block: a lane
// holds x01 / x23 of its dwords (0, 1) / (2, 3) and p01 / p23 of its partner's (__shfl_xor by 32).  Lane h = 0 makes words 0
// and 1, lane h = 1 words 2 and 3: (w0, w1) below are those two.
__device__ __forceinline__ void tpg_lb_words(int h, uint32_t x01, uint32_t p01, uint32_t x23, uint32_t p23, uint32_t& w0, uint32_t& w1) {
  if (h == 0) {
    w0 = (x01 & 0xffffu) | (p01 << 16);
    w1 = (x01 >> 16) | (p01 & 0xffff0000u);
  } else {
    w0 = (p23 & 0xffffu) | (x23 << 16);
    w1 = (p23 >> 16) | (x23 & 0xffff0000u);
  }
}
