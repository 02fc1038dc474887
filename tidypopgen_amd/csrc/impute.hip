// impute.hip -- simple imputation (gt_impute_simple: mode / mean0 / random), exact in integers.
//
//  * tpg_impute_store_kernel: the byte store in place.  A column (= one locus = nrow contiguous bytes) is cut into the
//    16-byte pieces of the allocation it overlaps; a wave (small nrow) or a workgroup reads them with 16-B loads into
//    registers, counts bytes 1 / 2 / 3 with byte masks + popcount, reduces over the wave (and LDS for a workgroup), decides
//    the fill and writes back ONLY the pieces that held a missing byte: nrow bytes read and at most nrow written per locus,
//    once.  The first and last piece of a column may belong to the neighbouring columns too (nrow is not a multiple of 16):
//    those are read and written byte by byte, so that no lane ever stores a byte of another column.  A column beyond the
//    register budget (8 pieces per thread, 1024 threads: 131 072 rows) is read twice instead.
//    A byte above 3 anywhere makes the call a refusal: the kernel leaves such a column alone and flags it, and the host
//    then turns the bytes 4..6 of all OTHER columns back into 3 (they can only be this call's fills), so that the store is
//    as it was -- without a checking pass over the store in front of every successful call.
//  * tpg_impute_view_kernel: the locus-tiled 2-bit layout L of a view -> the L of a new view.  One wave per 32-locus tile,
//    lane (r, h) owns locus r as in tpg_loci_counts_kernel; the tile's blocks are read twice (count, fill: the second read
//    comes from L2) and written once.  The other layouts of the new view are made from L when somebody asks for them.
//
// The fill of a missing entry under `random` is a pure function of (seed, i, j), the 0-based position in the object being
// imputed: tpg_impute_draw below, restated in include/tpg.h and in tests/impute_ref.py.
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "common.h"
#include "devfrag.h"
#include "synth_common.h"

// ---------------------------------------------------------------------------
// the fill value of a locus with c0 / c1 / c2 typed genotypes (t = c0 + c1 + c2 > 0), mode or mean0
TPG_HD int tpg_impute_fill(int method, int64_t c0, int64_t c1, int64_t c2) {
  if (method == TPG_IMPUTE_MODE) {  // which.max: the smaller genotype wins a tie
    int v = 0;
    int64_t best = c0;
    if (c1 > best) { v = 1; best = c1; }
    if (c2 > best) v = 2;
    return v;
  }
  // mean0: round(s / t) half to even, s / t in [0, 2]: 0.5 -> 0, 1.5 -> 2
  const int64_t t = c0 + c1 + c2, s2 = 2 * (c1 + 2 * c2);
  if (s2 <= t) return 0;
  if (s2 < 3 * t) return 1;
  return 2;
}
TPG_HD uint64_t tpg_impute_locus_key(uint64_t seed, uint64_t j) { return tpg_mix64(seed ^ tpg_mix64(j)); }
// thr = (s << 31) / t = 2^32 s / (2 t); two 32-bit uniforms from one hash
TPG_HD int tpg_impute_draw(uint64_t locus_key, uint64_t i, uint64_t thr) {
  const uint64_t h = tpg_mix64(locus_key ^ tpg_mix64(i));
  return (int)((h >> 32) < thr) + (int)((h & 0xFFFFFFFFull) < thr);
}

// ---------------------------------------------------------------------------
static constexpr int32_t IMP_ALL_MISSING = -1, IMP_REFUSED = -2;  // a locus's entry of stat[]; >= 0: entries filled
static constexpr int IMP_PMAX = 8;  // 16-byte pieces a thread keeps in registers

struct ImpCol {
  uint8_t* bytes;
  int64_t b0, b1, a0;  // the column's bytes [b0, b1), a0 = b0 rounded down to 16
  __device__ __forceinline__ bool full(int64_t p) const { return a0 + 16 * p >= b0 && a0 + 16 * p + 16 <= b1; }
  // piece p; bytes outside the column read as 0 (they count as nothing below)
  __device__ __forceinline__ uint4 load(int64_t p) const {
    const int64_t at = a0 + 16 * p;
    if (full(p)) return *(const uint4*)(bytes + at);
    uint32_t w[4] = {0, 0, 0, 0};
    for (int t = 0; t < 16; t++)
      if (at + t >= b0 && at + t < b1) w[t >> 2] |= (uint32_t)bytes[at + t] << (8 * (t & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
  }
};

__device__ __forceinline__ void imp_count(const uint4& r, int& c1, int& c2, int& c3, uint32_t& bad) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int d = 0; d < 4; d++) {
    bad |= w[d] & 0xFCFCFCFCu;
    const uint32_t lo = w[d] & 0x01010101u, hi = (w[d] >> 1) & 0x01010101u;
    c1 += __popc(lo & ~hi);
    c2 += __popc(hi & ~lo);
    c3 += __popc(lo & hi);
  }
}

// fill the missing bytes of piece p (3 -> 4 + v) and write the piece back if it held one
__device__ __forceinline__ void imp_fill(const ImpCol& col, int64_t p, uint4 r, int method, int v, uint64_t key, uint64_t thr) {
  uint32_t w[4] = {r.x, r.y, r.z, r.w};
  uint32_t any = 0;
  const int64_t at = col.a0 + 16 * p;
#pragma unroll
  for (int d = 0; d < 4; d++) {
    uint32_t miss = w[d] & (w[d] >> 1) & 0x01010101u;
    any |= miss;
    if (method != TPG_IMPUTE_RANDOM) {
      w[d] ^= miss * (uint32_t)(3 ^ (4 + v));
    } else {
      while (miss) {
        const int bt = (__ffs(miss) - 1) >> 3;
        miss &= miss - 1;
        const int vv = tpg_impute_draw(key, (uint64_t)(at + 4 * d + bt - col.b0), thr);
        w[d] ^= (uint32_t)(3 ^ (4 + vv)) << (8 * bt);
      }
    }
  }
  if (!any) return;
  if (col.full(p)) {
    *(uint4*)(col.bytes + at) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {  // a piece shared with a neighbouring column: only this column's own bytes are stored
    const uint32_t o[4] = {r.x, r.y, r.z, r.w};
    for (int t = 0; t < 16; t++) {
      const uint8_t nb = (uint8_t)(w[t >> 2] >> (8 * (t & 3))), ob = (uint8_t)(o[t >> 2] >> (8 * (t & 3)));
      if (nb != ob && at + t >= col.b0 && at + t < col.b1) col.bytes[at + t] = nb;
    }
  }
}

// WPL waves per locus (1: four loci per 256-thread workgroup); RES: the column stays in registers between count and fill
template <int WPL, bool RES>
__global__ __launch_bounds__(WPL >= 4 ? 64 * WPL : 256) void tpg_impute_store_kernel(uint8_t* __restrict__ bytes, int64_t nrow,
                                                                                       int64_t ncol, int method, uint64_t seed,
                                                                                       int64_t col0, int32_t* __restrict__ stat) {
  constexpr int TPL = 64 * WPL;                     // threads per locus
  constexpr int LPB = (WPL >= 4 ? 64 * WPL : 256) / TPL;  // loci per workgroup
  const int tl = threadIdx.x % TPL;
  const int64_t j = (int64_t)blockIdx.x * LPB + threadIdx.x / TPL;
  if (j >= ncol) return;  // (a whole wave, and with WPL > 1 the whole workgroup)
  ImpCol col;
  col.bytes = bytes;
  col.b0 = j * nrow;
  col.b1 = col.b0 + nrow;
  col.a0 = col.b0 & ~(int64_t)15;
  const int64_t npieces = (col.b1 - col.a0 + 15) >> 4;
  uint4 reg[IMP_PMAX];
  int c1 = 0, c2 = 0, c3 = 0;
  uint32_t bad = 0;
  if (RES) {
#pragma unroll
    for (int k = 0; k < IMP_PMAX; k++) {
      const int64_t p = tl + (int64_t)k * TPL;
      reg[k] = p < npieces ? col.load(p) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < IMP_PMAX; k++) imp_count(reg[k], c1, c2, c3, bad);
  } else {
    for (int64_t p = tl; p < npieces; p += TPL) imp_count(col.load(p), c1, c2, c3, bad);
  }
  c1 = tpg_wave_sum(c1);
  c2 = tpg_wave_sum(c2);
  c3 = tpg_wave_sum(c3);
  int nbad = tpg_wave_sum(bad ? 1 : 0);
  if (WPL > 1) {
    __shared__ int red[WPL > 1 ? WPL : 1][4];
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wv][0] = c1; red[wv][1] = c2; red[wv][2] = c3; red[wv][3] = nbad; }
    __syncthreads();
    c1 = c2 = c3 = nbad = 0;
    for (int w = 0; w < WPL; w++) { c1 += red[w][0]; c2 += red[w][1]; c3 += red[w][2]; nbad += red[w][3]; }
  }
  if (nbad) {  // already imputed, or not a CODE_012 store: the column is left alone and the call will be refused
    if (tl == 0) stat[j] = IMP_REFUSED;
    return;
  }
  if (c3 == 0) {
    if (tl == 0) stat[j] = 0;
    return;
  }
  const int64_t c0 = nrow - c1 - c2 - c3, t = nrow - c3, s = (int64_t)c1 + 2 * (int64_t)c2;
  if (t == 0) {  // nobody typed: stays missing
    if (tl == 0) stat[j] = IMP_ALL_MISSING;
    return;
  }
  const int v = method == TPG_IMPUTE_RANDOM ? 0 : tpg_impute_fill(method, c0, c1, c2);
  const uint64_t key = tpg_impute_locus_key(seed, (uint64_t)(col0 + j)), thr = ((uint64_t)s << 31) / (uint64_t)t;
  if (RES) {
#pragma unroll
    for (int k = 0; k < IMP_PMAX; k++) {
      const int64_t p = tl + (int64_t)k * TPL;
      if (p < npieces) imp_fill(col, p, reg[k], method, v, key, thr);
    }
  } else {
    for (int64_t p = tl; p < npieces; p += TPL) imp_fill(col, p, col.load(p), method, v, key, thr);
  }
  if (tl == 0) stat[j] = c3;
}

// stat[ncol] -> d_rep {imputed, loci_all_missing, columns refused}: one atomic per wave (an atomic per locus on one word
// is a million same-address atomics at the bench size: 10 ms of a 12 ms kernel when it was tried)
__global__ __launch_bounds__(256) void tpg_impute_report_kernel(const int32_t* __restrict__ stat, int64_t ncol,
                                                                unsigned long long* __restrict__ d_rep) {
  int64_t imp = 0;
  int miss = 0, bad = 0;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < ncol; j += (int64_t)gridDim.x * blockDim.x) {
    const int32_t v = stat[j];
    if (v > 0) imp += v;
    miss += v == IMP_ALL_MISSING;
    bad += v == IMP_REFUSED;
  }
  int lo = (int)(imp & 0xFFFFF), hi = (int)(imp >> 20);  // a thread sums far less than 2^51; a wave's sums fit two ints
  lo = tpg_wave_sum(lo);
  hi = tpg_wave_sum(hi);
  miss = tpg_wave_sum(miss);
  bad = tpg_wave_sum(bad);
  if ((threadIdx.x & 63) == 0) {
    const unsigned long long tot = ((unsigned long long)hi << 20) + (unsigned long long)lo;
    if (tot) atomicAdd(d_rep, tot);
    if (miss) atomicAdd(d_rep + 1, (unsigned long long)miss);
    if (bad) atomicAdd(d_rep + 2, (unsigned long long)bad);
  }
}

// the refusal's way back: in the columns that were not refused a byte 4..6 is a fill of the call being undone
__global__ __launch_bounds__(256) void tpg_impute_undo_kernel(uint8_t* __restrict__ bytes, int64_t nrow, int64_t ncol,
                                                              const int32_t* __restrict__ stat) {
  const int64_t total = nrow * ncol;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const uint8_t b = bytes[idx];
    if (b >= 4 && b <= 6 && stat[idx / nrow] != IMP_REFUSED) bytes[idx] = 3;
  }
}

template <int WPL>
static void launch_store(tpg_ctx* ctx, bool res, tpg_fbm* f, int method, uint64_t seed, int64_t col0, int32_t* d_stat) {
  constexpr int NT = WPL >= 4 ? 64 * WPL : 256;
  constexpr int LPB = NT / (64 * WPL);
  const dim3 grid((unsigned)ceil_div(f->ncol, LPB));
  if (res)
    TPG_LAUNCH(ctx, "impute_store", (tpg_impute_store_kernel<WPL, true>), grid, dim3(NT), 0, f->d_bytes, f->nrow, f->ncol, method, seed,
               col0, d_stat);
  else
    TPG_LAUNCH(ctx, "impute_store", (tpg_impute_store_kernel<WPL, false>), grid, dim3(NT), 0, f->d_bytes, f->nrow, f->ncol, method, seed,
               col0, d_stat);
}

static int check_method(int method) {
  TPG_REQUIRE(method == TPG_IMPUTE_MODE || method == TPG_IMPUTE_MEAN0 || method == TPG_IMPUTE_RANDOM, TPG_EINVAL,
              "impute method %d is not TPG_IMPUTE_MODE, _MEAN0 or _RANDOM", method);
  return TPG_OK;
}

extern "C" int tpg_fbm_impute_simple(tpg_ctx* ctx, tpg_fbm* fbm, int method, uint64_t seed, tpg_impute_report* rep) {
  return tpg_fbm_impute_simple_at(ctx, fbm, 0, method, seed, rep);
}

extern "C" int tpg_fbm_impute_simple_at(tpg_ctx* ctx, tpg_fbm* fbm, int64_t col0, int method, uint64_t seed, tpg_impute_report* rep) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && fbm && col0 >= 0, TPG_EINVAL, "null argument or negative col0");
  TPG_TRY(check_method(method));
  TPG_REQUIRE(fbm->bed_bpl == 0, TPG_EUNSUPPORTED,
              "a .bed-form store has no byte to hold an imputed genotype: impute a view of it with tpg_view_impute");
  TPG_REQUIRE(fbm->nrow > 0 && fbm->ncol > 0, TPG_EINVAL, "empty store");
  TPG_REQUIRE(fbm->nrow < (1ll << 30) && fbm->ncol < (1ll << 31), TPG_EINVAL, "store too large (%lld x %lld)", (long long)fbm->nrow,
              (long long)fbm->ncol);
  // 16-byte pieces a column can overlap; one wave keeps 8 per lane (8 190 rows), a workgroup of 4 / 16 waves beyond that.
  // TPG_IMPUTE_WPL = 1 | 4 | 16 forces the shape (tools/impute_only.py measures the crossover)
  const int64_t pieces = (fbm->nrow + 30) / 16;
  int wpl = pieces <= IMP_PMAX * 64 ? 1 : pieces <= IMP_PMAX * 256 ? 4 : 16;
  const int w = tpg_env_int("TPG_IMPUTE_WPL", 0);
  if (w == 1 || w == 4 || w == 16) wpl = w;
  const bool res = pieces <= (int64_t)IMP_PMAX * 64 * wpl;
  DevBuf stat;  // per locus: entries filled, or IMP_ALL_MISSING / IMP_REFUSED; then the report's three sums
  const size_t stat_bytes = (4 * (size_t)fbm->ncol + 31) & ~(size_t)31;
  TPG_TRY(stat.alloc(stat_bytes + 32));
  int32_t* const d_stat = stat.as<int32_t>();
  unsigned long long* d_rep = (unsigned long long*)(stat.as<uint8_t>() + stat_bytes);
  TPG_HIP(hipMemsetAsync(d_rep, 0, 32, ctx->stream));
  unsigned long long h[3] = {0, 0, 0};
  if (wpl == 1) launch_store<1>(ctx, res, fbm, method, seed, col0, d_stat);
  else if (wpl == 4) launch_store<4>(ctx, res, fbm, method, seed, col0, d_stat);
  else launch_store<16>(ctx, res, fbm, method, seed, col0, d_stat);
  TPG_CHECK_LAUNCH();
  const unsigned blocks = (unsigned)std::min<int64_t>(1024, ceil_div(fbm->ncol, 256));
  TPG_LAUNCH(ctx, "impute_report", tpg_impute_report_kernel, dim3(blocks), dim3(256), 0, (const int32_t*)d_stat, fbm->ncol, d_rep);
  TPG_CHECK_LAUNCH();
  TPG_HIP(tpg_fetch_small(ctx, h, d_rep, sizeof(h)));
  if (h[2]) {
    TPG_LAUNCH(ctx, "impute_undo", tpg_impute_undo_kernel, dim3(4096), dim3(256), 0, fbm->d_bytes, fbm->nrow, fbm->ncol,
               (const int32_t*)d_stat);
    TPG_CHECK_LAUNCH();
    TPG_HIP(hipStreamSynchronize(ctx->stream));
  }
  stat.free();
  TPG_REQUIRE(h[2] == 0, TPG_EUNSUPPORTED, "object x is already imputed (%llu loci hold a store byte above 3; the store is unchanged)",
              h[2]);
  if (rep) {
    rep->imputed = (int64_t)h[0];
    rep->loci_all_missing = (int64_t)h[1];
  }
  return TPG_OK;
}

// ---------------------------------------------------------------------------
// L -> L.  Grid: one wave per 32-locus tile, four tiles per workgroup.  col0: position of the view's first locus in the
// object being imputed (a streamed block's offset in the job's selection)
__global__ __launch_bounds__(256) void tpg_impute_view_kernel(const uint4* __restrict__ L, uint4* __restrict__ out, int64_t n_lt, int64_t Q,
                                                              int64_t n, int64_t m, int method, uint64_t seed, int64_t col0,
                                                              unsigned long long* __restrict__ d_rep) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int64_t lt = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (lt >= n_lt) return;
  const uint4* p = L + (lt * Q) * 64 + lane;
  uint4* o = out + (lt * Q) * 64 + lane;
  int c1 = 0, c2 = 0, c3 = 0;
  for (int64_t q = 0; q < Q; q++) {
    const uint4 a = p[q * 64];
    const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const uint32_t lo = w[d] & 0x55555555u, hi = (w[d] >> 1) & 0x55555555u;
      c1 += __popc(lo & ~hi);
      c2 += __popc(hi & ~lo);
      c3 += __popc(lo & hi);
    }
  }
  c1 += __shfl_xor(c1, 32);
  c2 += __shfl_xor(c2, 32);
  c3 += __shfl_xor(c3, 32);
  const int64_t j = lt * 32 + r;
  c3 -= (int)(Q * 128 - n);  // the padding individuals are code 3 too
  const int64_t c0 = n - c1 - c2 - c3, t = n - c3, s = (int64_t)c1 + 2 * (int64_t)c2;
  const bool fill = j < m && t > 0 && c3 > 0;
  const int v = fill && method != TPG_IMPUTE_RANDOM ? tpg_impute_fill(method, c0, c1, c2) : 0;
  const uint64_t key = tpg_impute_locus_key(seed, (uint64_t)(col0 + j)), thr = fill ? ((uint64_t)s << 31) / (uint64_t)t : 0;
  for (int64_t q = 0; q < Q; q++) {
    const uint4 a = p[q * 64];
    uint32_t w[4] = {a.x, a.y, a.z, a.w};
    if (fill) {
#pragma unroll
      for (int d = 0; d < 4; d++) {
        const int64_t base = 128 * q + 32 * d + 16 * h;  // individual of element 0 of this dword
        uint32_t miss = w[d] & (w[d] >> 1) & 0x55555555u;
        if (base + 16 > n) {  // the padding stays missing
          uint32_t real = 0;
          for (int e = 0; e < 16; e++)
            if (base + e < n) real |= 1u << tpg_elem_shift(e);
          miss &= real;
        }
        if (method != TPG_IMPUTE_RANDOM) {
          w[d] = (w[d] & ~(miss * 3u)) | (miss * (uint32_t)v);
        } else {
          while (miss) {
            const int pos = __ffs(miss) - 1;  // 8 b + 2 k: element 4 k + b
            miss &= miss - 1;
            const int e = 4 * ((pos & 7) >> 1) + (pos >> 3);
            const int vv = tpg_impute_draw(key, (uint64_t)(base + e), thr);
            w[d] = (w[d] & ~(3u << pos)) | ((uint32_t)vv << pos);
          }
        }
      }
    }
    o[q * 64] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  // report: one atomic per wave
  int imp = lane < 32 && fill ? c3 : 0, allmiss = lane < 32 && j < m && t == 0 ? 1 : 0;
  imp = tpg_wave_sum(imp);
  allmiss = tpg_wave_sum(allmiss);
  if (lane == 0) {
    if (imp) atomicAdd(d_rep, (unsigned long long)imp);
    if (allmiss) atomicAdd(d_rep + 1, (unsigned long long)allmiss);
  }
}

int tpg_view_impute_at(tpg_ctx* ctx, const tpg_view* raw, int method, uint64_t seed, int64_t col0, tpg_view** out,
                       tpg_impute_report* rep) {
  TPG_REQUIRE(ctx && raw && out, TPG_EINVAL, "null argument");
  TPG_TRY(check_method(method));
  TPG_TRY(tpg_view_need_L(ctx, raw));
  ViewPtr v(new tpg_view(ctx, raw->n, raw->m));
  DevBuf d_rep;
  TPG_HIP(tpg_pmalloc((void**)&v->L, v->bytes_each));
  TPG_TRY(d_rep.alloc(16));
  TPG_HIP(hipMemsetAsync(d_rep.p, 0, 16, ctx->stream));
  const int64_t n_lt = 4 * raw->KG;
  TPG_LAUNCH(ctx, "impute_view", tpg_impute_view_kernel, dim3((unsigned)ceil_div(n_lt, 4)), dim3(256), 0, (const uint4*)raw->L, v->L, n_lt,
             raw->Q, raw->n, raw->m, method, seed, col0, d_rep.as<unsigned long long>());
  TPG_CHECK_LAUNCH();
  unsigned long long h[2] = {0, 0};
  if (rep) TPG_HIP(tpg_fetch_small(ctx, h, d_rep.p, sizeof(h)));
  if (rep) {
    rep->imputed = (int64_t)h[0];
    rep->loci_all_missing = (int64_t)h[1];
  }
  *out = v.release();
  return TPG_OK;
}

extern "C" int tpg_view_impute(tpg_ctx* ctx, const tpg_view* raw, int method, uint64_t seed, tpg_view** out, tpg_impute_report* rep) {
  TpgEnter _enter(ctx);
  return tpg_view_impute_at(ctx, raw, method, seed, 0, out, rep);
}
