// ld.hip -- LD clumping (loci_ld_clump) on the device: the link relation of neighbouring loci as a bit band, the
// priority order and the greedy resolution.  The definition is in include/tpg.h ("LD clumping"); DESIGN.md 3.6 has the
// mapping and what bounds the kernels.
//
//  * tpg_ld_band_kernel: r^2 of two loci without missing genotypes follows from integer sums; the only quadratic one,
//    Sxy = sum_i x_j x_k, is the banded product of the locus-tiled layout L with itself on the FP4 matrix cores that
//    ldband.h holds (tpg_band_contract, shared with knnimp.hip; its operand helpers are devfrag.h's): exact in FP32 for
//    every n < 2^22.
//    A workgroup owns the 32 loci of row tile jt and walks the column tiles jt .. (last neighbour of the tile) / 32 in
//    super-chunks of 16; wave w of 4 holds the accumulators of tiles w, w + 4, w + 8, w + 12 of the chunk and contracts
//    them over Q.  In the epilogue every lane forms num and the comparison for its 16 elements; a ballot turns a register
//    into the 32 column bits of two rows, the strips of a super-chunk meet in LDS, are shifted to the row's own origin
//    (bit b of row j = locus j + 1 + b) and leave as whole words.  The transposed relation (for locus k: which loci of
//    row tile jt are linked to it) is one OR over a lane's registers and leaves as whole words as well, so that the
//    resolution reads two contiguous rows per locus instead of one bit from each of `window` rows.
//  * priority: a 64-bit key per locus (minor allele count, or the caller's S made order-preserving), stable radix sort,
//    rank[locus] stays in HBM.
//  * tpg_ld_round_kernel: one Jacobi round of the resolution (16 lanes per undecided locus); tpg_ld_finish_kernel: one
//    wave walks what is still undecided after TPG_LD_MAX_ROUNDS in rank order.
#include "common.h"
#include "devfrag.h"
#include "ldband.h"
#include <hipcub/hipcub.hpp>

#include <cmath>

#define TPG_LD_MAX_ROUNDS 32
#define LD_UNDECIDED 0
#define LD_KEPT 1
#define LD_FALLEN 2

// counts (m x 4 {n0, n1, n2, nNA}) -> Sx, d = n Sxx - Sx^2 (below 2^46: exact as a double), the default priority
// (minor allele count) and whether anything is missing
__global__ __launch_bounds__(256) void tpg_ld_prep_kernel(const int4* __restrict__ counts, int64_t n, int64_t m,
                                                          int32_t* __restrict__ sx, double* __restrict__ dd,
                                                          int32_t* __restrict__ flags) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const int4 c = counts[j];
  if (c.w != 0) atomicOr(flags, 1);
  const int64_t s = (int64_t)c.y + 2 * (int64_t)c.z, sxx = (int64_t)c.y + 4 * (int64_t)c.z;
  sx[j] = (int32_t)s;
  dd[j] = (double)(n * sxx - s * s);
}

__global__ __launch_bounds__(256) void tpg_ld_band_kernel(const uint4* __restrict__ L, int64_t Q, int64_t n, int64_t m,
                                                          const int64_t* __restrict__ hi, const int32_t* __restrict__ sx,
                                                          const double* __restrict__ dd, double thr,
                                                          uint32_t* __restrict__ bits, int64_t stride,
                                                          uint32_t* __restrict__ back, int64_t bstride,
                                                          unsigned long long* __restrict__ links) {
  __shared__ uint32_t strip[32][TPG_BAND_SC + 1];  // [row][0: last tile of the super-chunk before | 1 + tile of this one]
  __shared__ int32_t r_sx[32];
  __shared__ double r_dd[32];
  __shared__ int64_t r_hi[32];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t jt = blockIdx.x, j0 = jt * 32;
  if (tid < 32) {
    const int64_t j = j0 + tid;
    r_sx[tid] = j < m ? sx[j] : 0;
    r_dd[tid] = j < m ? dd[j] : 0.0;
    r_hi[tid] = j < m ? hi[j] : -1;  // a padding row has no neighbour
    strip[tid][0] = 0;
  }
  const int NT = tpg_band_tiles(hi, jt, m);
  const int nsc = NT / TPG_BAND_SC + 1;  // the last word of a row needs the tile behind it: one more chunk at a multiple
  __syncthreads();
  unsigned cnt = 0;
  for (int sc = 0; sc < nsc; sc++) {
    const int t0 = sc * TPG_BAND_SC + wv;  // tiles of this wave: offsets t0 + 4 i from jt; the first `nt` of them lie inside the band
    v16f acc[TPG_BAND_TK];
#pragma unroll
    for (int i = 0; i < TPG_BAND_TK; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][r] = 0.f;  // (all four: zeroing only the tiles inside the band costs 130 more registers)
    const int nt = tpg_band_contract<TPG_BAND_TK>(L, Q, jt, NT, sc, wv, lane, acc);
    // epilogue: link bits of this wave's tiles -> row strips in LDS, column strips to `back`
#pragma unroll
    for (int i = 0; i < TPG_BAND_TK; i++) {
      const int slot = 1 + wv + 4 * i;
      if (i < nt) {
        const int t = t0 + 4 * i;
        const int64_t k = (jt + t) * 32 + (lane & 31);
        const int64_t sxk = k < m ? sx[k] : 0;
        const double ddk = k < m ? dd[k] : 0.0;
        uint32_t colmask = 0;
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int row = tpg_cd_row(r, lane);
          const int64_t sxy = (int64_t)acc[i][r];
          const int64_t num = n * sxy - (int64_t)r_sx[row] * sxk;
          const double dn = (double)num;
          const double lhs = dn * dn;
          const double den = r_dd[row] * ddk;
          const double rhs = thr * den;
          const bool link = lhs > rhs && k > j0 + row && k <= r_hi[row];
          const unsigned long long bal = __ballot(link);
          if ((lane & 31) == 0) strip[row][slot] = lane < 32 ? (uint32_t)bal : (uint32_t)(bal >> 32);
          colmask |= link ? 1u << row : 0u;
        }
        colmask |= (uint32_t)__shfl_xor((int)colmask, 32);
        if (back && lane < 32 && k < m && t < bstride) back[k * bstride + t] = colmask;
      } else if (lane < 32) {
        strip[lane][slot] = 0;
      }
    }
    __syncthreads();
    // word w of row j holds the loci j + 1 + 32 w .. j + 32 + 32 w: tiles w and w + 1 from jt, shifted by row + 1
    for (int idx = tid; idx < 32 * TPG_BAND_SC; idx += 256) {
      const int row = idx / TPG_BAND_SC, wl = idx % TPG_BAND_SC;
      const int64_t w = (int64_t)sc * TPG_BAND_SC - 1 + wl;
      const unsigned long long both = ((unsigned long long)strip[row][wl + 1] << 32) | strip[row][wl];
      const uint32_t word = (uint32_t)(both >> (row + 1));
      if (w >= 0 && w < stride && j0 + row < m) {
        bits[(j0 + row) * stride + w] = word;
        cnt += __popc(word);
      }
    }
    uint32_t carry = 0;
    if (tid < 32) carry = strip[tid][TPG_BAND_SC];
    __syncthreads();
    if (tid < 32) strip[tid][0] = carry;
  }
  cnt = (unsigned)tpg_wave_sum((int)cnt);
  if (lane == 0 && cnt) atomicAdd(links, (unsigned long long)cnt);
}

// ---- priority ---------------------------------------------------------------------------------------------------
// ascending radix key of "more important first": n - minor allele count (below 2^23), or the caller's S through the
// order-preserving map of IEEE doubles, complemented (-0 counts as 0: R's order() compares values)
__global__ __launch_bounds__(256) void tpg_ld_key_kernel(const int32_t* __restrict__ sx, const double* __restrict__ S,
                                                         int64_t n, int64_t m, unsigned long long* __restrict__ key,
                                                         uint32_t* __restrict__ idx, int32_t* __restrict__ flags) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  idx[j] = (uint32_t)j;
  if (!S) {
    const int64_t s = sx[j], mac = s < 2 * n - s ? s : 2 * n - s;
    key[j] = (unsigned long long)(n - mac);
    return;
  }
  const double v = S[j];
  if (v != v) {
    atomicOr(flags, 2);
    key[j] = 0;
    return;
  }
  const uint64_t u = v == 0.0 ? 0ull : (uint64_t)__double_as_longlong(v);
  key[j] = ~TPG_DKEY(u);
}

__global__ __launch_bounds__(256) void tpg_ld_rank_kernel(const uint32_t* __restrict__ order, int64_t m,
                                                          uint32_t* __restrict__ rank, const uint8_t* __restrict__ exclude,
                                                          uint8_t* __restrict__ state) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  rank[order[i]] = (uint32_t)i;
  state[i] = exclude && exclude[i] ? LD_FALLEN : LD_UNDECIDED;  // an excluded locus is never kept and removes nobody
}

// ---- resolution -------------------------------------------------------------------------------------------------
// One Jacobi round: an undecided locus falls if a linked locus of higher priority is kept, is kept if all of them have
// fallen.  16 lanes share a locus: its forward row (bits) and its backward row (back, one word per row tile).
__global__ __launch_bounds__(256) void tpg_ld_round_kernel(const uint32_t* __restrict__ bits, int64_t stride,
                                                           const uint32_t* __restrict__ back, int64_t bstride,
                                                           const uint32_t* __restrict__ rank, const uint8_t* __restrict__ s_in,
                                                           uint8_t* __restrict__ s_out, int64_t m,
                                                           unsigned long long* __restrict__ undecided) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t j = g >> 4;
  const int sub = (int)(g & 15);
  const int st = j < m ? s_in[j] : LD_FALLEN;
  int any_kept = 0, all_fallen = 1;
  if (st == LD_UNDECIDED) {
    const uint32_t rj = rank[j];
    auto see = [&](int64_t k) {
      if (rank[k] < rj) {
        const int s = s_in[k];
        any_kept |= s == LD_KEPT;
        all_fallen &= s == LD_FALLEN;
      }
    };
    for (int64_t w = sub; w < stride; w += 16) {
      uint32_t word = bits[j * stride + w];
      const int64_t base = j + 1 + 32 * w;
      while (word) {
        const int b = __ffs((int)word) - 1;
        word &= word - 1;
        see(base + b);
      }
    }
    for (int64_t t = sub; t < bstride; t += 16) {
      uint32_t word = back[j * bstride + t];
      const int64_t base = ((j >> 5) - t) * 32;
      while (word) {
        const int b = __ffs((int)word) - 1;
        word &= word - 1;
        see(base + b);
      }
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    any_kept |= __shfl_xor(any_kept, o);
    all_fallen &= __shfl_xor(all_fallen, o);
  }
  int left = 0;
  if (sub == 0 && j < m) {
    const int ns = st != LD_UNDECIDED ? st : any_kept ? LD_FALLEN : all_fallen ? LD_KEPT : LD_UNDECIDED;
    s_out[j] = (uint8_t)ns;
    left = ns == LD_UNDECIDED;
  }
  const unsigned long long bal = __ballot(left);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(undecided, (unsigned long long)__popcll(bal));
}

// What the bounded rounds left: one wave walks the loci in rank order.  Everything of higher priority is decided when a
// locus is reached, and a kept neighbour is of higher priority (it could not have been kept before this one fell), so
// the locus falls iff a linked locus is kept.  The wave reads back its own stores: device-scope atomics.
__global__ __launch_bounds__(64) void tpg_ld_finish_kernel(const uint32_t* __restrict__ bits, int64_t stride,
                                                           const uint32_t* __restrict__ back, int64_t bstride,
                                                           const uint32_t* __restrict__ order, uint8_t* state, int64_t m) {
  const int lane = threadIdx.x;
  for (int64_t i0 = 0; i0 < m; i0 += 64) {
    const int64_t i = i0 + lane;
    const int64_t j = i < m ? (int64_t)order[i] : 0;
    const int st = i < m ? __hip_atomic_load(&state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : LD_FALLEN;
    unsigned long long todo = __ballot(st == LD_UNDECIDED);
    while (todo) {
      const int b = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int64_t ju = (int64_t)(uint32_t)__shfl((int)j, b);
      int any = 0;
      for (int64_t w = lane; w < stride + bstride; w += 64) {
        uint32_t word;
        int64_t base;
        if (w < stride) {
          word = bits[ju * stride + w];
          base = ju + 1 + 32 * w;
        } else {
          word = back[ju * bstride + (w - stride)];
          base = ((ju >> 5) - (w - stride)) * 32;
        }
        while (word) {
          const int bb = __ffs((int)word) - 1;
          word &= word - 1;
          any |= __hip_atomic_load(&state[base + bb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == LD_KEPT;
        }
      }
      const bool falls = __ballot(any) != 0;
      if (lane == 0)
        __hip_atomic_store(&state[ju], (uint8_t)(falls ? LD_FALLEN : LD_KEPT), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    }
  }
}

__global__ __launch_bounds__(256) void tpg_ld_keep_kernel(const uint8_t* __restrict__ state, int64_t m, uint8_t* __restrict__ keep,
                                                          unsigned long long* __restrict__ kept) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int k = j < m && state[j] == LD_KEPT;
  if (j < m) keep[j] = (uint8_t)k;
  const unsigned long long bal = __ballot(k);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(kept, (unsigned long long)__popcll(bal));
}

// ---- host side --------------------------------------------------------------------------------------------------
namespace {

struct LdBand {
  int64_t words = 0;  // ceil(max(hi[j] - j) / 32)
  int32_t* d_sx = nullptr;
  double* d_dd = nullptr;
  int64_t* d_hi = nullptr;
  int32_t* d_flags = nullptr;              // bit 0: a missing genotype, bit 1: a NaN in S
  unsigned long long* d_counters = nullptr;  // [0] links, [1] kept, [2 + r] undecided after round r
};

// the window: hi[j] in [j, m), non-decreasing.  `hi` may be device memory.
int ld_window(tpg_ctx* ctx, const int64_t* hi, int64_t m, HostIn<int64_t>& h, int64_t* words) {
  TPG_TRY(h.init(ctx, hi, m));
  int64_t W = 0;
  for (int64_t j = 0; j < m; j++) {
    TPG_REQUIRE(h[(size_t)j] >= j && h[(size_t)j] < m, TPG_EINVAL, "hi[%lld] = %lld outside [%lld, %lld)", (long long)j,
                (long long)h[(size_t)j], (long long)j, (long long)m);
    TPG_REQUIRE(j == 0 || h[(size_t)j] >= h[(size_t)j - 1], TPG_EINVAL, "hi decreases at locus %lld", (long long)j);
    if (h[(size_t)j] - j > W) W = h[(size_t)j] - j;
  }
  *words = ceil_div(W, 32);
  return TPG_OK;
}

int ld_check_args(tpg_ctx* ctx, const tpg_view* v, const int64_t* hi, double thr_r2) {
  TPG_REQUIRE(ctx && v && hi, TPG_EINVAL, "null argument");
  TPG_REQUIRE(thr_r2 >= 0.0 && thr_r2 <= 1.0, TPG_EINVAL, "thr_r2 must lie in [0, 1]");  // (a NaN fails both)
  TPG_REQUIRE(v->m >= 1 && v->n >= 1, TPG_EINVAL, "empty view");
  TPG_REQUIRE(v->n < TPG_BAND_MAX_N, TPG_EUNSUPPORTED, "LD of 2^22 individuals or more");  // FP32 sums of dosage products
  TPG_REQUIRE(v->m < (1ll << 31) - 64, TPG_EUNSUPPORTED, "LD of 2^31 loci or more");
  return TPG_OK;
}

// counts -> Sx, d and the missing-value check; the window goes up.  Nothing of the caller's is written.
int ld_prepare(tpg_ctx* ctx, const tpg_view* v, const HostIn<int64_t>& h, DevArena& sc, LdBand* B) {
  const int64_t m = v->m;
  int32_t* d_counts = nullptr;
  TPG_TRY(sc.get(&d_counts, 4 * (size_t)m));
  TPG_TRY(sc.get(&B->d_sx, (size_t)m));
  TPG_TRY(sc.get(&B->d_dd, (size_t)m));
  TPG_TRY(sc.get(&B->d_hi, (size_t)m));
  TPG_TRY(sc.get(&B->d_flags, 1));
  TPG_TRY(sc.get(&B->d_counters, 2 + TPG_LD_MAX_ROUNDS));
  TPG_HIP(hipMemsetAsync(B->d_flags, 0, sizeof(int32_t), ctx->stream));
  TPG_HIP(hipMemsetAsync(B->d_counters, 0, sizeof(unsigned long long) * (2 + TPG_LD_MAX_ROUNDS), ctx->stream));
  TPG_TRY(tpg_launch_loci_counts(ctx, v, d_counts));
  TPG_LAUNCH(ctx, "ld_prep", tpg_ld_prep_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, (const int4*)d_counts, v->n, m,
             B->d_sx, B->d_dd, B->d_flags);
  TPG_CHECK_LAUNCH();
  TPG_HIP(tpg_upload(ctx, B->d_hi, h.p, sizeof(int64_t) * (size_t)m));
  return TPG_OK;
}

int ld_launch_band(tpg_ctx* ctx, const tpg_view* v, double thr_r2, const LdBand& B, uint32_t* d_bits, int64_t stride,
                   uint32_t* d_back, int64_t bstride) {
  const int64_t m = v->m;
  TPG_TRY(tpg_view_need_L(ctx, v));
  if (stride > 0) TPG_HIP(hipMemsetAsync(d_bits, 0, sizeof(uint32_t) * (size_t)m * (size_t)stride, ctx->stream));
  if (d_back) TPG_HIP(hipMemsetAsync(d_back, 0, sizeof(uint32_t) * (size_t)m * (size_t)bstride, ctx->stream));
  TPG_LAUNCH(ctx, "ld_band", tpg_ld_band_kernel, dim3((unsigned)ceil_div(m, 32)), dim3(256), 0, (const uint4*)v->L, v->Q, v->n,
             m, (const int64_t*)B.d_hi, (const int32_t*)B.d_sx, (const double*)B.d_dd, thr_r2, d_bits, stride, d_back,
             bstride, B.d_counters);
  TPG_CHECK_LAUNCH();
  return TPG_OK;
}

}  // namespace

extern "C" int tpg_ld_band_links(tpg_ctx* ctx, const tpg_view* v, const int64_t* hi, double thr_r2, uint32_t* bits,
                                 int64_t stride_words, int64_t* n_links) {
  TpgEnter _enter(ctx);
  TPG_TRY(ld_check_args(ctx, v, hi, thr_r2));
  TPG_REQUIRE(stride_words >= 0 && (bits || stride_words == 0), TPG_EINVAL, "null argument");
  HostIn<int64_t> h;
  LdBand B;
  TPG_TRY(ld_window(ctx, hi, v->m, h, &B.words));
  TPG_REQUIRE(stride_words >= B.words, TPG_EINVAL, "stride_words = %lld, the window needs %lld", (long long)stride_words,
              (long long)B.words);
  DevArena sc;
  TPG_TRY(ld_prepare(ctx, v, h, sc, &B));
  int32_t flags = 0;
  TPG_HIP(tpg_fetch_small(ctx, &flags, B.d_flags, sizeof(flags)));
  TPG_REQUIRE(!(flags & 1), TPG_ENUMERIC, "LD of a view with missing genotypes (impute it first)");
  unsigned long long links = 0;
  if (stride_words > 0) {
    OutBuf o;
    TPG_TRY(o.init(bits, sizeof(uint32_t) * (size_t)v->m * (size_t)stride_words));
    TPG_TRY(ld_launch_band(ctx, v, thr_r2, B, o.dev<uint32_t>(), stride_words, nullptr, 0));
    TPG_HIP(tpg_fetch_small(ctx, &links, B.d_counters, sizeof(links)));  // waits for the kernel
    TPG_TRY(o.commit(ctx));
  }
  if (n_links) *n_links = (int64_t)links;
  return TPG_OK;
}

extern "C" int tpg_ld_clump(tpg_ctx* ctx, const tpg_view* v, const int64_t* hi, double thr_r2, const double* S,
                            const uint8_t* exclude, uint8_t* keep, tpg_ld_report* report) {
  TpgEnter _enter(ctx);
  TPG_TRY(ld_check_args(ctx, v, hi, thr_r2));
  TPG_REQUIRE(keep, TPG_EINVAL, "null argument");
  const int64_t m = v->m;
  HostIn<int64_t> h;
  LdBand B;
  TPG_TRY(ld_window(ctx, hi, m, h, &B.words));
  const int64_t stride = B.words > 0 ? B.words : 1, bstride = B.words + 1;
  DevArena sc;
  TPG_TRY(ld_prepare(ctx, v, h, sc, &B));
  InBuf inS, inX;
  if (S) TPG_TRY(inS.init(ctx, S, sizeof(double) * (size_t)m));
  if (exclude) TPG_TRY(inX.init(ctx, exclude, (size_t)m));
  // priority: key, stable sort, rank
  unsigned long long *d_key = nullptr, *d_key2 = nullptr;
  uint32_t *d_idx = nullptr, *d_order = nullptr, *d_rank = nullptr;
  uint8_t *d_s0 = nullptr, *d_s1 = nullptr;
  TPG_TRY(sc.get(&d_key, (size_t)m));
  TPG_TRY(sc.get(&d_key2, (size_t)m));
  TPG_TRY(sc.get(&d_idx, (size_t)m));
  TPG_TRY(sc.get(&d_order, (size_t)m));
  TPG_TRY(sc.get(&d_rank, (size_t)m));
  TPG_TRY(sc.get(&d_s0, (size_t)m));
  TPG_TRY(sc.get(&d_s1, (size_t)m));
  const unsigned g256 = (unsigned)ceil_div(m, 256);
  TPG_LAUNCH(ctx, "ld_key", tpg_ld_key_kernel, dim3(g256), dim3(256), 0, (const int32_t*)B.d_sx, S ? inS.dev<double>() : nullptr,
             v->n, m, d_key, d_idx, B.d_flags);
  TPG_CHECK_LAUNCH();
  int32_t flags = 0;
  TPG_HIP(tpg_fetch_small(ctx, &flags, B.d_flags, sizeof(flags)));
  TPG_REQUIRE(!(flags & 1), TPG_ENUMERIC, "LD clumping of a view with missing genotypes (impute it first)");
  TPG_REQUIRE(!(flags & 2), TPG_EINVAL, "NaN in S");
  {
    const int end_bit = S ? 64 : 24;
    size_t t_sort = 0;
    TPG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, t_sort, d_key, d_key2, d_idx, d_order, (int)m, 0, end_bit, ctx->stream));
    uint8_t* d_tmp = nullptr;
    TPG_TRY(sc.get(&d_tmp, t_sort));
    ProfScope ps(ctx, "ld_sort");
    TPG_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp, t_sort, d_key, d_key2, d_idx, d_order, (int)m, 0, end_bit, ctx->stream));
  }
  TPG_LAUNCH(ctx, "ld_rank", tpg_ld_rank_kernel, dim3(g256), dim3(256), 0, (const uint32_t*)d_order, m, d_rank,
             exclude ? inX.dev<uint8_t>() : nullptr, d_s0);
  TPG_CHECK_LAUNCH();
  // the band, both halves
  uint32_t *d_bits = nullptr, *d_back = nullptr;
  TPG_TRY(sc.get(&d_bits, (size_t)m * (size_t)stride));
  TPG_TRY(sc.get(&d_back, (size_t)m * (size_t)bstride));
  TPG_TRY(ld_launch_band(ctx, v, thr_r2, B, d_bits, stride, d_back, bstride));
  // bounded Jacobi rounds, then the walk in rank order
  int64_t rounds = 0;
  unsigned long long left = (unsigned long long)m;
  uint8_t *s_in = d_s0, *s_out = d_s1;
  const unsigned g16 = (unsigned)ceil_div(m * 16, 256);
  while (left > 0 && rounds < TPG_LD_MAX_ROUNDS) {
    TPG_LAUNCH(ctx, "ld_round", tpg_ld_round_kernel, dim3(g16), dim3(256), 0, (const uint32_t*)d_bits, stride,
               (const uint32_t*)d_back, bstride, (const uint32_t*)d_rank, (const uint8_t*)s_in, s_out, m,
               B.d_counters + 2 + rounds);
    TPG_CHECK_LAUNCH();
    TPG_HIP(tpg_fetch_small(ctx, &left, B.d_counters + 2 + rounds, sizeof(left)));
    rounds++;
    std::swap(s_in, s_out);
  }
  if (left > 0) {
    TPG_LAUNCH(ctx, "ld_finish", tpg_ld_finish_kernel, dim3(1), dim3(64), 0, (const uint32_t*)d_bits, stride,
               (const uint32_t*)d_back, bstride, (const uint32_t*)d_order, s_in, m);
    TPG_CHECK_LAUNCH();
  }
  OutBuf o;
  TPG_TRY(o.init(keep, (size_t)m));
  TPG_LAUNCH(ctx, "ld_keep", tpg_ld_keep_kernel, dim3(g256), dim3(256), 0, (const uint8_t*)s_in, m, o.dev<uint8_t>(),
             B.d_counters + 1);
  TPG_CHECK_LAUNCH();
  unsigned long long lk[2] = {0, 0};
  TPG_HIP(tpg_fetch_small(ctx, lk, B.d_counters, sizeof(lk)));  // waits for everything above
  TPG_TRY(o.commit(ctx));
  if (report) {
    report->links = (int64_t)lk[0];
    report->kept = (int64_t)lk[1];
    report->rounds = rounds;
    report->finish_loci = (int64_t)left;
    report->band_bytes = (int64_t)(sizeof(uint32_t) * (size_t)m * (size_t)(stride + bstride));
  }
  return TPG_OK;
}
