// knnimp.hip -- LD-kNN imputation (gt_impute_knn) on the device.  The definition is in include/tpg.h ("LD-kNN imputation");
// DESIGN.md 3.19 has the mapping and what bounds the kernels.
//
//  * tpg_knn_band_kernel: the banded contraction of ldband.h (tpg_band_contract, shared with tpg_ld_band_kernel of ld.hip) --
//    Sxy = sum_i x_j x_k of neighbouring loci as an FP4 MFMA product of the locus-tiled layout L with itself, exact in FP32 for
//    n < 2^22; the operand helpers and the wave sum are devfrag.h's -- with an epilogue that writes the int32
//    sums of the FORWARD band: band[(j - row0) * W + (k - j - 1)] for j < k <= hi[j].  The loci are walked in chunks so that the
//    band stays under a cap (KNN_BAND_CAP); a chunk's band starts W rows before its first locus, for the backward entries.
//  * tpg_knn_select_kernel: a wave per locus.  Its forward row is contiguous, its backward entries are strided reads of at most
//    W rows.  (r2 desc, |k - j| asc, k asc) is a strict total order of the candidates, so round t takes the largest candidate
//    BEHIND the one round t - 1 took: l rounds of a wave-wide argmax and no state but the last pick.
//  * tpg_knn_vote_kernel, the hot path: one workgroup per locus with a missing entry (a compacted list).  Every individual's
//    profile over the l_j neighbour loci (host/host_knnimp.h: a 64-bit thermometer word, a 32-bit missing mask) and its code at
//    the locus itself go to LDS, or beyond KNN_LDS_MAX_NPAD individuals to a global scratch of the workgroup's own; then a wave
//    per missing individual: the lanes stride over the individuals and add to the wave's own histogram in LDS, one lane walks it
//    (host_knn_vote) and leaves 4 + fill in the code array, which nobody reads as a vote.  Integers only; no launch shape changes
//    a bit of the result.
//  * fill-the-store, check-the-store and compare (the error counts) are byte / 2-bit sweeps.
#include <algorithm>

#include "common.h"
#include "devfrag.h"
#include "ldband.h"
#include "host/host_knnimp.h"

#define KNN_BAND_CAP (256ull << 20)        // bytes of band per chunk of loci
#define KNN_BAND_CAP_SMALL (8ull << 10)   // TPG_KNN_SMALL_CHUNKS: the tests' way into the chunk walk
#define KNN_HIST_STRIDE 196                // 65 x 3 int32, rounded up to a multiple of 4
// copies of a wave's histogram, lane & 3 picks one: the votes of a wave fall on a handful of (distance, genotype) bins, and
// LDS atomics of one instruction on one address run one after the other
#define KNN_HIST_COPIES 4
#define KNN_LDS_HEAD ((4 * KNN_HIST_COPIES * KNN_HIST_STRIDE + 32) * 4)  // the histograms of four waves and the neighbour list
#define KNN_PROFILE_BYTES 13               // thermometer 8 + missing mask 4 + code at the locus 1, as three arrays
// individuals (padded to 128) whose profiles one workgroup keeps in LDS: 12 672 + 13 * 11 520 = 162 432 <= 163 840
#define KNN_LDS_MAX_NPAD 11520

// counts (m x 4 {n0, n1, n2, nNA}) of the mode-filled view -> Sx and d = n Sxx - Sx^2, as tpg_ld_prep_kernel forms them.  A
// locus typed nowhere has d = 0 and is nobody's candidate; a locus typed in part is the caller's mistake (flags bit 0).
__global__ __launch_bounds__(256) void tpg_knn_prep_kernel(const int4* __restrict__ counts, int64_t n, int64_t m,
                                                           int32_t* __restrict__ sx, double* __restrict__ dd,
                                                           int32_t* __restrict__ flags) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const int4 c = counts[j];
  if (c.w != 0 && c.w < n) atomicOr(flags, 1);
  const int64_t s = (int64_t)c.y + 2 * (int64_t)c.z, sxx = (int64_t)c.y + 4 * (int64_t)c.z;
  sx[j] = (int32_t)s;
  dd[j] = c.w != 0 ? 0.0 : (double)(n * sxx - s * s);
}

// Row tile jt = tile0 + blockIdx.x; band rows count from row0 = 32 tile0.
__global__ __launch_bounds__(256) void tpg_knn_band_kernel(const uint4* __restrict__ L, int64_t Q, int64_t m,
                                                           const int64_t* __restrict__ hi, int64_t tile0, int64_t W,
                                                           int32_t* __restrict__ band) {
  __shared__ int64_t r_hi[32];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t jt = tile0 + blockIdx.x, j0 = jt * 32, row0 = tile0 * 32;
  if (tid < 32) r_hi[tid] = j0 + tid < m ? hi[j0 + tid] : -1;  // a padding row has no neighbour
  const int NT = tpg_band_tiles(hi, jt, m);
  const int nsc = (NT + TPG_BAND_SC - 1) / TPG_BAND_SC;
  __syncthreads();
  for (int sc = 0; sc < nsc; sc++) {
    const int t0 = sc * TPG_BAND_SC + wv;
    v16f acc[TPG_BAND_TK];
#pragma unroll
    for (int i = 0; i < TPG_BAND_TK; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][r] = 0.f;  // (all four: zeroing only the tiles inside the band costs 130 more registers)
    const int nt = tpg_band_contract<TPG_BAND_TK>(L, Q, jt, NT, sc, wv, lane, acc);
    // epilogue: the sums of the forward band, 32 consecutive k of one row per half wave
#pragma unroll
    for (int i = 0; i < TPG_BAND_TK; i++) {
      if (i < nt) {
        const int64_t k = (jt + t0 + 4 * i) * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int row = tpg_cd_row(r, lane);
          const int64_t j = j0 + row;
          if (k > j && k <= r_hi[row]) band[(j - row0) * W + (k - j - 1)] = (int32_t)acc[i][r];
        }
      }
    }
  }
}

// (r2, k) of candidate a comes before candidate b of locus j; kb < 0: b is nobody
__device__ __forceinline__ bool knn_before(double ra, int ka, double rb, int kb, int j) {
  if (kb < 0) return true;
  if (ra != rb) return ra > rb;
  const int da = ka > j ? ka - j : j - ka, db = kb > j ? kb - j : j - kb;
  if (da != db) return da < db;
  return ka < kb;
}

// a wave per locus of [ja, jb)
__global__ __launch_bounds__(256) void tpg_knn_select_kernel(const int32_t* __restrict__ band, int64_t row0, int64_t W,
                                                             const int64_t* __restrict__ hi, const int32_t* __restrict__ sx,
                                                             const double* __restrict__ dd, int64_t n, int64_t ja, int64_t jb,
                                                             int l, double min_r2, int32_t* __restrict__ nbr,
                                                             double* __restrict__ r2out) {
  const int lane = threadIdx.x & 63;
  const int64_t j = ja + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= jb) return;
  const double dj = dd[j];
  const int64_t sxj = sx[j], hij = hi[j];
  double last_r = 0.0;
  int last_k = -1;
  int t = 0;
  if (dj > 0.0) {
    for (; t < l; t++) {
      double best_r = 0.0;
      int best_k = -1;
      for (int64_t c = lane; c < 2 * W; c += 64) {
        int64_t k, sxy;
        if (c < W) {
          k = j + 1 + c;
          if (k > hij) continue;
          sxy = band[(j - row0) * W + c];
        } else {
          k = j - 1 - (c - W);
          if (k < 0 || hi[k] < j) continue;
          sxy = band[(k - row0) * W + (j - k - 1)];
        }
        const double dk = dd[k];
        if (!(dk > 0.0)) continue;
        const int64_t num = n * sxy - sxj * (int64_t)sx[k];
        const double dn = (double)num;
        const double sq = dn * dn;
        const double den = dj * dk;
        const double r = sq / den;
        if (!(r > min_r2)) continue;
        if (last_k >= 0 && !knn_before(last_r, last_k, r, (int)k, (int)j)) continue;  // taken by an earlier round
        if (knn_before(r, (int)k, best_r, best_k, (int)j)) {
          best_r = r;
          best_k = (int)k;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double orr = __shfl_xor(best_r, o);
        const int ok = __shfl_xor(best_k, o);
        if (ok >= 0 && knn_before(orr, ok, best_r, best_k, (int)j)) {
          best_r = orr;
          best_k = ok;
        }
      }
      if (best_k < 0) break;  // (the same on every lane)
      if (lane == 0) {
        nbr[j * l + t] = best_k;
        r2out[j * l + t] = best_r;
      }
      last_r = best_r;
      last_k = best_k;
    }
  }
  for (int u = t + lane; u < l; u += 64) {
    nbr[j * l + u] = -1;
    r2out[j * l + u] = 0.0;
  }
}

// the loci with a missing entry, in no particular order (nothing depends on it)
__global__ __launch_bounds__(256) void tpg_knn_list_kernel(const int4* __restrict__ counts, int64_t m, int32_t* __restrict__ list,
                                                           unsigned int* __restrict__ nlist) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool has = j < m && counts[j].w > 0;
  const unsigned long long bal = __ballot(has);
  if (!bal) return;
  unsigned int base = 0;
  if (lane == 0) base = atomicAdd(nlist, (unsigned int)__popcll(bal));
  base = (unsigned int)__shfl((int)base, 0);
  if (has) list[base + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)j;
}

// rep: {imputed, loci_all_missing, entries_left, loci_without_neighbours}
template <bool GLB>
__global__ __launch_bounds__(256) void tpg_knn_vote_kernel(const uint32_t* __restrict__ Lw, uint32_t* __restrict__ Ow, int64_t Q,
                                                           int64_t n, const int4* __restrict__ counts,
                                                           const int32_t* __restrict__ list, int64_t nlist,
                                                           const int32_t* __restrict__ nbr, int l, int k, uint64_t* g_th,
                                                           uint32_t* g_ms, uint8_t* g_cj, unsigned long long* __restrict__ rep) {
  extern __shared__ __attribute__((aligned(16))) uint8_t knn_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t npad = Q * 128;
  int32_t* const hist = (int32_t*)knn_lds + wv * KNN_HIST_COPIES * KNN_HIST_STRIDE;  // copy 0 takes the sums before the walk
  int32_t* const s_nbr = (int32_t*)knn_lds + 4 * KNN_HIST_COPIES * KNN_HIST_STRIDE;
  uint64_t* th;
  uint32_t* ms;
  uint8_t* cj;
  if (GLB) {
    th = g_th + (int64_t)blockIdx.x * npad;
    ms = g_ms + (int64_t)blockIdx.x * npad;
    cj = g_cj + (int64_t)blockIdx.x * npad;
  } else {
    th = (uint64_t*)(knn_lds + KNN_LDS_HEAD);
    ms = (uint32_t*)(th + npad);
    cj = (uint8_t*)(ms + npad);
  }
  for (int64_t it = blockIdx.x; it < nlist; it += gridDim.x) {
    const int64_t j = list[it];
    const int64_t nna = counts[j].w;
    if (nna >= n) {  // nobody is typed: T = 0 for every entry (the same decision in every thread)
      if (tid == 0) {
        atomicAdd(rep + 1, 1ull);
        atomicAdd(rep + 2, (unsigned long long)n);
        atomicAdd(rep + 3, 1ull);  // (d = 0: no candidate)
      }
      continue;
    }
    if (tid < 32) s_nbr[tid] = tid < l ? nbr[j * l + tid] : -1;
    __syncthreads();
    int lj = 0;
    for (int t = 0; t < l; t++) lj += s_nbr[t] >= 0;  // the used slots come first
    // 1. profiles: a thread takes the 16 individuals of one dword of L
    for (int64_t grp = tid; grp < npad / 16; grp += 256) {
      const int64_t i0 = grp * 16, qq = i0 >> 7;
      const int s = (int)(i0 >> 5) & 3, h = (int)(i0 >> 4) & 1;
      auto word = [&](int64_t x) { return Lw[((((x >> 5) * Q + qq) * 64 + (x & 31) + 32 * h) << 2) + s]; };
      uint64_t pth[16];
      uint32_t pms[16];
#pragma unroll
      for (int e = 0; e < 16; e++) {
        pth[e] = 0;
        pms[e] = 0;
      }
      for (int t = 0; t < lj; t++) {
        const uint32_t w = word(s_nbr[t]);
#pragma unroll
        for (int e = 0; e < 16; e++) host_knn_profile_add(&pth[e], &pms[e], t, (int)((w >> tpg_elem_shift(e)) & 3u));
      }
      const uint32_t wj = word(j);
      uint32_t cw[4] = {0, 0, 0, 0};
#pragma unroll
      for (int e = 0; e < 16; e++) {
        th[i0 + e] = pth[e];
        ms[i0 + e] = pms[e];
        cw[e >> 2] |= ((wj >> tpg_elem_shift(e)) & 3u) << (8 * (e & 3));  // (a padding individual is code 3 in L)
      }
      *(uint4*)(cj + i0) = make_uint4(cw[0], cw[1], cw[2], cw[3]);
    }
    __syncthreads();
    // 2. a wave per missing individual; the chunks of 64 individuals are dealt to the waves
    const int64_t T = n - nna;
    const int nb = 3 * (2 * lj + 1);  // bins a distance can reach
    for (int64_t c0 = (int64_t)wv * 64; c0 < n; c0 += 256) {
      const int64_t i = c0 + lane;
      unsigned long long todo = __ballot(i < n && cj[i] == 3);
      while (todo) {
        const int64_t a = c0 + (__ffsll((long long)todo) - 1);
        todo &= todo - 1;
        const uint64_t th_a = th[a];
        const uint32_t ms_a = ms[a];
#pragma unroll
        for (int r = 0; r < KNN_HIST_COPIES; r++)
          for (int x = lane; x < nb; x += 64) hist[r * KNN_HIST_STRIDE + x] = 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        // four individuals per lane and step: their LDS reads are in flight together
        int32_t* const mine = hist + (lane & (KNN_HIST_COPIES - 1)) * KNN_HIST_STRIDE;
        for (int64_t b0 = lane; b0 < n; b0 += 256) {
          int g[4];
          uint64_t th_b[4];
          uint32_t ms_b[4];
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int64_t b = b0 + 64 * u;
            const int64_t at = b < n ? b : 0;
            g[u] = b < n ? cj[at] : 3;
            th_b[u] = th[at];
            ms_b[u] = ms[at];
          }
#pragma unroll
          for (int u = 0; u < 4; u++)
            if (g[u] < 3) atomicAdd(&mine[3 * host_knn_dist(th_a, ms_a, th_b[u], ms_b[u]) + g[u]], 1);  // (a filled entry is 4 + fill: no voter)
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (int x = lane; x < nb; x += 64) {
          int s = hist[x];
#pragma unroll
          for (int r = 1; r < KNN_HIST_COPIES; r++) s += hist[r * KNN_HIST_STRIDE + x];
          hist[x] = s;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
          const int f = host_knn_vote(hist, 2 * lj + 1, k, T);
          if (f < 3) cj[a] = (uint8_t)(4 + f);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
      }
    }
    __syncthreads();
    // 3. the fills go into the new view's L, whole dwords
    int filled = 0, left = 0;
    for (int64_t grp = tid; grp < npad / 16; grp += 256) {
      const int64_t i0 = grp * 16, qq = i0 >> 7;
      const int s = (int)(i0 >> 5) & 3, h = (int)(i0 >> 4) & 1;
      const int64_t at = ((((j >> 5) * Q + qq) * 64 + (j & 31) + 32 * h) << 2) + s;
      const uint32_t w = Lw[at];
      uint32_t nw = w;
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int c = cj[i0 + e];
        if (c >= 4) {
          nw = (nw & ~(3u << tpg_elem_shift(e))) | ((uint32_t)(c - 4) << tpg_elem_shift(e));
          filled++;
        } else if (c == 3 && i0 + e < n) {
          left++;
        }
      }
      if (nw != w) Ow[at] = nw;
    }
    filled = tpg_wave_sum(filled);
    left = tpg_wave_sum(left);
    if (lane == 0) {
      if (filled) atomicAdd(rep, (unsigned long long)filled);
      if (left) atomicAdd(rep + 2, (unsigned long long)left);
    }
    if (tid == 0 && lj == 0) atomicAdd(rep + 3, 1ull);
    __syncthreads();  // the profiles and the neighbour list are rewritten for the next locus
  }
}

// a byte above 3 anywhere in the store
__global__ __launch_bounds__(256) void tpg_knn_store_check_kernel(const uint8_t* __restrict__ bytes, int64_t total, int32_t* __restrict__ flag) {
  uint32_t bad = 0;
  const int64_t n16 = total / 16, stride = (int64_t)gridDim.x * 256;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n16; p += stride) {
    const uint4 r = ((const uint4*)bytes)[p];
    bad |= (r.x | r.y | r.z | r.w) & 0xFCFCFCFCu;
  }
  for (int64_t p = n16 * 16 + (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += stride) bad |= bytes[p] & 0xFCu;
  if (__ballot(bad != 0) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// store byte 3 -> 4 + the code the filled view holds for it (a code 3 there: left as it is)
__global__ __launch_bounds__(256) void tpg_knn_store_fill_kernel(uint8_t* __restrict__ bytes, int64_t nrow, int64_t ncol,
                                                                 const uint32_t* __restrict__ Lw, int64_t Q) {
  const int64_t total = nrow * ncol;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    if (bytes[idx] != 3) continue;
    const int64_t j = idx / nrow, i = idx - j * nrow;
    const uint32_t w = Lw[((((j >> 5) * Q + (i >> 7)) * 64 + (j & 31) + 32 * ((i >> 4) & 1)) << 2) + ((i >> 5) & 3)];
    const uint32_t c = (w >> tpg_elem_shift((int)(i & 15))) & 3u;
    if (c != 3) bytes[idx] = (uint8_t)(4 + c);
  }
}

// per locus: entries typed in `full` and missing in `train`, and how many of them `filled` has wrong (an entry left at 3 is
// wrong).  One wave per 32-locus tile, lane (r, h) as in tpg_impute_view_kernel.
__global__ __launch_bounds__(256) void tpg_knn_errors_kernel(const uint4* __restrict__ F, const uint4* __restrict__ Tr,
                                                             const uint4* __restrict__ Fi, int64_t n_lt, int64_t Q, int64_t m,
                                                             long long* __restrict__ per_locus, unsigned long long* __restrict__ tot) {
  const int lane = threadIdx.x & 63, r = lane & 31;
  const int64_t lt = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (lt >= n_lt) return;
  const int64_t base = (lt * Q) * 64 + lane;
  int held = 0, wrong = 0;
  for (int64_t q = 0; q < Q; q++) {
    const uint4 a4 = F[base + q * 64], t4 = Tr[base + q * 64], f4 = Fi[base + q * 64];
    const uint32_t a[4] = {a4.x, a4.y, a4.z, a4.w}, t[4] = {t4.x, t4.y, t4.z, t4.w}, f[4] = {f4.x, f4.y, f4.z, f4.w};
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const uint32_t typed = ~(a[d] & (a[d] >> 1)) & 0x55555555u;  // (a padding individual is code 3: not typed)
      const uint32_t hm = typed & t[d] & (t[d] >> 1);
      const uint32_t x = f[d] ^ a[d];
      held += __popc(hm);
      wrong += __popc(hm & (x | (x >> 1)));
    }
  }
  held += __shfl_xor(held, 32);
  wrong += __shfl_xor(wrong, 32);
  const int64_t j = lt * 32 + r;
  const bool mine = lane < 32 && j < m;
  if (mine) {
    per_locus[2 * j] = held;
    per_locus[2 * j + 1] = wrong;
  }
  const int th = tpg_wave_sum(mine ? held : 0), tw = tpg_wave_sum(mine ? wrong : 0);
  if (lane == 0) {
    if (th) atomicAdd(tot, (unsigned long long)th);
    if (tw) atomicAdd(tot + 1, (unsigned long long)tw);
  }
}

// ---- host side --------------------------------------------------------------------------------------------------
namespace {

// the window of "LD clumping": hi[j] in [j, m), non-decreasing; *W = max(hi[j] - j)
int knn_window(tpg_ctx* ctx, const int64_t* hi, int64_t m, HostIn<int64_t>& h, int64_t* W) {
  TPG_TRY(h.init(ctx, hi, m));
  int64_t w = 0;
  for (int64_t j = 0; j < m; j++) {
    TPG_REQUIRE(h[j] >= j && h[j] < m, TPG_EINVAL, "hi[%lld] = %lld outside [%lld, %lld)", (long long)j, (long long)h[j],
                (long long)j, (long long)m);
    TPG_REQUIRE(j == 0 || h[j] >= h[j - 1], TPG_EINVAL, "hi decreases at locus %lld", (long long)j);
    w = std::max(w, h[j] - j);
  }
  *W = w;
  return TPG_OK;
}

int knn_check_args(tpg_ctx* ctx, const tpg_view* v, const int64_t* hi, int l, int k, double min_r2, int flags) {
  TPG_REQUIRE(ctx && v && hi, TPG_EINVAL, "null argument");
  TPG_REQUIRE(l >= 1 && l <= HOST_KNN_MAX_L, TPG_EINVAL, "l = %d outside [1, %d]", l, HOST_KNN_MAX_L);
  TPG_REQUIRE(k >= 1, TPG_EINVAL, "k = %d is not positive", k);
  TPG_REQUIRE(min_r2 >= 0.0 && min_r2 <= 1.7976931348623157e308, TPG_EINVAL, "min_r2 must be a finite number >= 0");  // (a NaN fails)
  TPG_REQUIRE((flags & ~(TPG_KNN_PROFILES_GLOBAL | TPG_KNN_SMALL_CHUNKS)) == 0, TPG_EINVAL, "unknown flags %d", flags);
  TPG_REQUIRE(v->m >= 1 && v->n >= 1, TPG_EINVAL, "empty view");
  TPG_REQUIRE(v->n < TPG_BAND_MAX_N, TPG_EINVAL, "LD-kNN imputation of 2^22 individuals or more");  // FP32 sums of dosage products
  TPG_REQUIRE(v->m < (1ll << 31) - 64, TPG_EINVAL, "LD-kNN imputation of 2^31 loci or more");
  TPG_REQUIRE(v->L || v->LM, TPG_EINVAL, "the view has no locus-tiled layout");
  return TPG_OK;
}

// loci whose neighbours one chunk selects, so that the band of the chunk (W rows in front of it, a tile of slack at either
// end) stays under `cap` -- or the 32 loci a chunk cannot go below
int64_t knn_chunk_loci(int64_t m, int64_t W, size_t cap) {
  if (W == 0) return std::max<int64_t>(32, (m + 31) / 32 * 32);
  const int64_t rows = (int64_t)(cap / (4 * (size_t)W));
  const int64_t sel = (rows - W - 64) / 32 * 32;
  return std::min<int64_t>(std::max<int64_t>(sel, 32), (m + 31) / 32 * 32);
}
int64_t knn_band_rows(int64_t m, int64_t W, size_t cap) { return knn_chunk_loci(m, W, cap) + W + 64; }

// nbr (m x l) and r2 (m x l) of a view whose loci are typed everywhere or nowhere; d_hi: the window in device memory
int knn_neighbours(tpg_ctx* ctx, const tpg_view* w, int64_t W, const int64_t* d_hi, int l, double min_r2, int flags, DevArena& sc,
                   int32_t* d_nbr, double* d_r2) {
  const int64_t m = w->m;
  int32_t *d_counts = nullptr, *d_sx = nullptr, *d_flags = nullptr, *d_band = nullptr;
  double* d_dd = nullptr;
  TPG_TRY(sc.get(&d_counts, 4 * (size_t)m));
  TPG_TRY(sc.get(&d_sx, (size_t)m));
  TPG_TRY(sc.get(&d_dd, (size_t)m));
  TPG_TRY(sc.get(&d_flags, 1));
  TPG_HIP(hipMemsetAsync(d_flags, 0, sizeof(int32_t), ctx->stream));
  TPG_TRY(tpg_view_need_L(ctx, w));
  TPG_TRY(tpg_launch_loci_counts(ctx, w, d_counts));
  TPG_LAUNCH(ctx, "knn_prep", tpg_knn_prep_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, (const int4*)d_counts, w->n, m, d_sx,
             d_dd, d_flags);
  TPG_CHECK_LAUNCH();
  int32_t flg = 0;
  TPG_HIP(tpg_fetch_small(ctx, &flg, d_flags, sizeof(flg)));
  TPG_REQUIRE(!(flg & 1), TPG_ENUMERIC, "LD neighbours of a view with missing genotypes (impute it first)");
  const size_t cap = (flags & TPG_KNN_SMALL_CHUNKS) ? KNN_BAND_CAP_SMALL : KNN_BAND_CAP;
  const int64_t sel = knn_chunk_loci(m, W, cap);
  TPG_TRY(sc.get(&d_band, (size_t)knn_band_rows(m, W, cap) * (size_t)std::max<int64_t>(W, 1)));
  for (int64_t a = 0; a < m; a += sel) {
    const int64_t b = std::min(m, a + sel);
    const int64_t tile0 = std::max<int64_t>(0, a - W) / 32, tiles = ceil_div(b, 32) - tile0;  // (tiles * 32 <= sel + W + 63 rows)
    if (W > 0) {
      TPG_LAUNCH(ctx, "knn_band", tpg_knn_band_kernel, dim3((unsigned)tiles), dim3(256), 0, (const uint4*)w->L, w->Q, m, d_hi, tile0, W,
                 d_band);
      TPG_CHECK_LAUNCH();
    }
    TPG_LAUNCH(ctx, "knn_select", tpg_knn_select_kernel, dim3((unsigned)ceil_div(b - a, 4)), dim3(256), 0, (const int32_t*)d_band,
               tile0 * 32, W, d_hi, (const int32_t*)d_sx, (const double*)d_dd, w->n, a, b, l, min_r2, d_nbr, d_r2);
    TPG_CHECK_LAUNCH();
  }
  return TPG_OK;
}

// the whole method on a raw view; *out is a new view, rep4 = {imputed, loci_all_missing, entries_left, loci_without_neighbours}
int knn_impute_view(tpg_ctx* ctx, const tpg_view* raw, const int64_t* hi, int l, int k, double min_r2, int flags, tpg_view** out,
                    unsigned long long* rep4) {
  const int64_t n = raw->n, m = raw->m;
  HostIn<int64_t> h;
  int64_t W = 0;
  TPG_TRY(knn_window(ctx, hi, m, h, &W));
  TPG_TRY(tpg_view_need_L(ctx, raw));
  DevArena sc;
  int64_t* d_hi = nullptr;
  int32_t *d_nbr = nullptr, *d_counts = nullptr, *d_list = nullptr;
  double* d_r2 = nullptr;
  unsigned long long* d_rep = nullptr;  // [0..3] the report, [4] the length of the list (as an unsigned int)
  TPG_TRY(sc.get(&d_hi, (size_t)m));
  TPG_TRY(sc.get(&d_nbr, (size_t)m * l));
  TPG_TRY(sc.get(&d_r2, (size_t)m * l));
  TPG_TRY(sc.get(&d_counts, 4 * (size_t)m));
  TPG_TRY(sc.get(&d_list, (size_t)m));
  TPG_TRY(sc.get(&d_rep, 5));
  TPG_HIP(hipMemsetAsync(d_rep, 0, 5 * sizeof(unsigned long long), ctx->stream));
  TPG_HIP(tpg_upload(ctx, d_hi, h.p, sizeof(int64_t) * (size_t)m));
  {  // step 1 on the mode-filled view, which goes back to the pool before the vote
    tpg_view* wp = nullptr;
    TPG_TRY(tpg_view_impute_at(ctx, raw, TPG_IMPUTE_MODE, 0, 0, &wp, nullptr));
    ViewPtr w(wp);
    DevArena sc1;
    TPG_TRY(knn_neighbours(ctx, w.get(), W, d_hi, l, min_r2, flags, sc1, d_nbr, d_r2));
    TPG_HIP(hipStreamSynchronize(ctx->stream));
  }
  ViewPtr v(new tpg_view(ctx, n, m));
  TPG_HIP(tpg_pmalloc((void**)&v->L, v->bytes_each));
  TPG_HIP(tpg_copy_dev(ctx, v->L, raw->L, v->bytes_each));
  TPG_TRY(tpg_launch_loci_counts(ctx, raw, d_counts));
  TPG_LAUNCH(ctx, "knn_list", tpg_knn_list_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, (const int4*)d_counts, m, d_list,
             (unsigned int*)(d_rep + 4));
  TPG_CHECK_LAUNCH();
  unsigned long long hrep[5] = {0, 0, 0, 0, 0};
  TPG_HIP(tpg_fetch_small(ctx, &hrep[4], d_rep + 4, sizeof(unsigned long long)));
  const int64_t nlist = (int64_t)(hrep[4] & 0xFFFFFFFFull);
  if (nlist > 0) {
    const int64_t npad = raw->Q * 128;
    const bool glb = (flags & TPG_KNN_PROFILES_GLOBAL) || npad > KNN_LDS_MAX_NPAD;
    if (glb) {
      const int64_t grid = std::min<int64_t>(nlist, (int64_t)ctx->num_cu * 2);
      uint64_t* g_th = nullptr;
      uint32_t* g_ms = nullptr;
      uint8_t* g_cj = nullptr;
      TPG_TRY(sc.get(&g_th, (size_t)(grid * npad)));
      TPG_TRY(sc.get(&g_ms, (size_t)(grid * npad)));
      TPG_TRY(sc.get(&g_cj, (size_t)(grid * npad)));
      TPG_LAUNCH(ctx, "knn_vote", tpg_knn_vote_kernel<true>, dim3((unsigned)grid), dim3(256), KNN_LDS_HEAD, (const uint32_t*)raw->L,
                 (uint32_t*)v->L, raw->Q, n, (const int4*)d_counts, (const int32_t*)d_list, nlist, (const int32_t*)d_nbr, l, k, g_th,
                 g_ms, g_cj, d_rep);
    } else {
      const size_t lds = KNN_LDS_HEAD + (size_t)KNN_PROFILE_BYTES * (size_t)npad;
      const int64_t grid = std::min<int64_t>(nlist, (int64_t)ctx->num_cu * 4);
      (void)hipFuncSetAttribute((const void*)tpg_knn_vote_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      TPG_LAUNCH(ctx, "knn_vote", tpg_knn_vote_kernel<false>, dim3((unsigned)grid), dim3(256), lds, (const uint32_t*)raw->L,
                 (uint32_t*)v->L, raw->Q, n, (const int4*)d_counts, (const int32_t*)d_list, nlist, (const int32_t*)d_nbr, l, k,
                 (uint64_t*)nullptr, (uint32_t*)nullptr, (uint8_t*)nullptr, d_rep);
    }
    TPG_CHECK_LAUNCH();
  }
  TPG_HIP(tpg_fetch_small(ctx, hrep, d_rep, 4 * sizeof(unsigned long long)));  // waits for the vote
  for (int i = 0; i < 4; i++) rep4[i] = hrep[i];
  *out = v.release();
  return TPG_OK;
}

void knn_report(const unsigned long long* r, tpg_impute_report* rep, int64_t* rep_knn) {
  if (rep) {
    rep->imputed = (int64_t)r[0];
    rep->loci_all_missing = (int64_t)r[1];
  }
  if (rep_knn) {
    rep_knn[0] = (int64_t)r[2];
    rep_knn[1] = (int64_t)r[3];
  }
}

}  // namespace

extern "C" size_t tpg_knn_impute_scratch_bytes(int64_t n, int64_t m, int64_t width, int l) {
  if (n < 1 || m < 1 || width < 0 || l < 1) return 0;
  const size_t Q = (size_t)ceil_div(n, 128), KG = (size_t)ceil_div(m, 128);
  size_t b = 2 * Q * KG * 4096;                                                          // the mode-filled view and the result
  b += (size_t)knn_band_rows(m, width, KNN_BAND_CAP) * (size_t)std::max<int64_t>(width, 1) * 4;  // the band of one chunk
  b += (size_t)m * (size_t)l * 12;                                                       // nbr and r2
  b += (size_t)m * (8 + 16 + 16 + 4 + 8 + 4);                                            // hi, two count tables, Sx, d, the list
  if ((int64_t)Q * 128 > KNN_LDS_MAX_NPAD) b += (size_t)512 * Q * 128 * KNN_PROFILE_BYTES;  // profiles of 2 workgroups per CU
  return b;
}

extern "C" int tpg_ld_top_neighbours(tpg_ctx* ctx, const tpg_view* v, const int64_t* hi, int l, double min_r2, int flags, int32_t* nbr,
                                     double* r2) {
  TpgEnter _enter(ctx);
  TPG_TRY(knn_check_args(ctx, v, hi, l, 1, min_r2, flags));
  TPG_REQUIRE(nbr && r2, TPG_EINVAL, "null argument");
  HostIn<int64_t> h;
  int64_t W = 0;
  TPG_TRY(knn_window(ctx, hi, v->m, h, &W));
  DevArena sc;
  int64_t* d_hi = nullptr;
  TPG_TRY(sc.get(&d_hi, (size_t)v->m));
  TPG_HIP(tpg_upload(ctx, d_hi, h.p, sizeof(int64_t) * (size_t)v->m));
  OutBuf on, orr;
  TPG_TRY(on.init(nbr, sizeof(int32_t) * (size_t)v->m * l));
  TPG_TRY(orr.init(r2, sizeof(double) * (size_t)v->m * l));
  TPG_TRY(knn_neighbours(ctx, v, W, d_hi, l, min_r2, flags, sc, on.dev<int32_t>(), orr.dev<double>()));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  TPG_TRY(on.commit(ctx));
  TPG_TRY(orr.commit(ctx));
  return TPG_OK;
}

extern "C" int tpg_view_impute_knn(tpg_ctx* ctx, const tpg_view* raw, const int64_t* hi, int l, int k, double min_r2, int flags,
                                   tpg_view** out, tpg_impute_report* rep, int64_t* rep_knn) {
  TpgEnter _enter(ctx);
  TPG_TRY(knn_check_args(ctx, raw, hi, l, k, min_r2, flags));
  TPG_REQUIRE(out, TPG_EINVAL, "null argument");
  unsigned long long r[4] = {0, 0, 0, 0};
  TPG_TRY(knn_impute_view(ctx, raw, hi, l, k, min_r2, flags, out, r));
  knn_report(r, rep, rep_knn);
  return TPG_OK;
}

extern "C" int tpg_fbm_impute_knn(tpg_ctx* ctx, tpg_fbm* fbm, const int64_t* hi, int l, int k, double min_r2, int flags,
                                  tpg_impute_report* rep, int64_t* rep_knn) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && fbm && hi, TPG_EINVAL, "null argument");
  TPG_REQUIRE(fbm->bed_bpl == 0, TPG_EUNSUPPORTED,
              "a .bed-form store has no byte to hold an imputed genotype: impute a view of it with tpg_view_impute_knn");
  TPG_REQUIRE(fbm->nrow > 0 && fbm->ncol > 0, TPG_EINVAL, "empty store");
  const int64_t total = fbm->nrow * fbm->ncol;
  DevBuf flag;
  TPG_TRY(flag.alloc(sizeof(int32_t)));
  TPG_HIP(hipMemsetAsync(flag.p, 0, sizeof(int32_t), ctx->stream));
  const unsigned blocks = (unsigned)std::min<int64_t>((int64_t)ctx->num_cu * 8, ceil_div(total, 4096));
  TPG_LAUNCH(ctx, "knn_store_check", tpg_knn_store_check_kernel, dim3(blocks), dim3(256), 0, (const uint8_t*)fbm->d_bytes, total,
             flag.as<int32_t>());
  TPG_CHECK_LAUNCH();
  int32_t bad = 0;
  TPG_HIP(tpg_fetch_small(ctx, &bad, flag.p, sizeof(bad)));
  TPG_REQUIRE(!bad, TPG_EUNSUPPORTED, "object x is already imputed (the store holds a byte above 3; it is unchanged)");
  tpg_view* rp = nullptr;
  TPG_TRY(tpg_view_create(ctx, fbm, nullptr, 0, nullptr, 0, nullptr, &rp));
  ViewPtr raw(rp);
  TPG_TRY(knn_check_args(ctx, raw.get(), hi, l, k, min_r2, flags));
  unsigned long long r[4] = {0, 0, 0, 0};
  tpg_view* fp = nullptr;
  TPG_TRY(knn_impute_view(ctx, raw.get(), hi, l, k, min_r2, flags, &fp, r));
  ViewPtr filled(fp);
  TPG_LAUNCH(ctx, "knn_store_fill", tpg_knn_store_fill_kernel, dim3(blocks), dim3(256), 0, fbm->d_bytes, fbm->nrow, fbm->ncol,
             (const uint32_t*)filled->L, filled->Q);
  TPG_CHECK_LAUNCH();
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  knn_report(r, rep, rep_knn);
  return TPG_OK;
}

extern "C" int tpg_view_impute_errors(tpg_ctx* ctx, const tpg_view* full, const tpg_view* train, const tpg_view* filled,
                                      int64_t* per_locus, int64_t* totals) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && full && train && filled && per_locus && totals, TPG_EINVAL, "null argument");
  TPG_REQUIRE(full->n == train->n && full->m == train->m && full->n == filled->n && full->m == filled->m, TPG_EINVAL,
              "the three views differ in geometry");
  TPG_TRY(tpg_view_need_L(ctx, full));
  TPG_TRY(tpg_view_need_L(ctx, train));
  TPG_TRY(tpg_view_need_L(ctx, filled));
  const int64_t m = full->m, n_lt = 4 * full->KG;
  DevBuf d_tot;
  TPG_TRY(d_tot.alloc(16));
  TPG_HIP(hipMemsetAsync(d_tot.p, 0, 16, ctx->stream));
  OutBuf o;
  TPG_TRY(o.init(per_locus, sizeof(int64_t) * 2 * (size_t)m));
  TPG_LAUNCH(ctx, "knn_errors", tpg_knn_errors_kernel, dim3((unsigned)ceil_div(n_lt, 4)), dim3(256), 0, (const uint4*)full->L,
             (const uint4*)train->L, (const uint4*)filled->L, n_lt, full->Q, m, o.dev<long long>(), d_tot.as<unsigned long long>());
  TPG_CHECK_LAUNCH();
  unsigned long long t[2] = {0, 0};
  TPG_HIP(tpg_fetch_small(ctx, t, d_tot.p, sizeof(t)));
  TPG_TRY(o.commit(ctx));
  totals[0] = (int64_t)t[0];
  totals[1] = (int64_t)t[1];
  return TPG_OK;
}
