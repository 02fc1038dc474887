// ldstat.hip -- LD statistics (loci_ld_score, ld_decay, ld_region_r2) on the device: how much LD there is inside the window that
// LD clumping and LD-kNN imputation only search.  The definition is in include/tpg.h ("LD statistics"); DESIGN.md 3.21 has the
// mapping and what was measured.
//
//  * tpg_ldstat_kernel<false>: the frame of tpg_knn_band_kernel -- a workgroup per row tile, super-chunks of TPG_BAND_SC column
//    tiles, Sxy from tpg_band_contract (ldband.h) -- with an epilogue that never writes the band.  For every accumulator inside
//    j < k <= hi[j] a lane forms r2 and its fixed-point value q (host/host_ldstat.h, the routines the host program runs) and adds
//    q three ways: to the sum of its COLUMN k, kept in a register over the 16 accumulator registers of a tile and sent off as one
//    64-bit atomic per column and tile; to the sum of its ROW, by a transposing butterfly over the 32 lanes that share a row
//    (ldstat_row_reduce: 16 exchanges for 16 registers) into the workgroup's row sums in LDS, sent off once per workgroup; and to
//    its distance bin in a workgroup-local histogram in LDS, flushed once per workgroup.  Every sum is an integer sum: no order
//    changes a bit, and a NULL output group only removes instructions.
//  * tpg_ldstat_kernel<true>: the same frame for the row tiles that meet [j0, j1); the epilogue stores r2 itself.
#include <algorithm>

#include "common.h"
#include "devfrag.h"
#include "ldband.h"
#include "host/host_ldstat.h"

#define LDSTAT_MAX_PAIRS (1ll << 33)   // sum_j (hi[j] - j) below this: no sum of q <= 2^30 passes 2^63
#define LDSTAT_MAX_VALUES (1ll << 26)  // doubles a tpg_ld_band_r2 call returns
#define LDSTAT_MAX_POS (1ll << 61)     // |pos| below this: no distance overflows
// bins the workgroup-local histogram holds; a pair in a bin beyond goes to the global sums directly
#define LDSTAT_HIST_BINS 512
// copies of the histogram, lane & 3 picks one: with a coarse bin_size the pairs of one instruction fall in one or two bins, and
// LDS atomics of one instruction on one address run one after the other (KNN_HIST_COPIES of knnimp.hip)
#define LDSTAT_HIST_COPIES 4
// count and sum of q of the at most 32 pairs a row or a column has inside one 32 x 32 tile, in one word: q <= 2^30
#define LDSTAT_PACK_SHIFT 40
#define LDSTAT_PACK_MASK ((1ull << LDSTAT_PACK_SHIFT) - 1ull)

// counts (m x 4 {n0, n1, n2, nNA}) -> Sx and d = n Sxx - Sx^2, as tpg_ld_prep_kernel forms them; any missing genotype: flags bit 0
__global__ __launch_bounds__(256) void tpg_ldstat_prep_kernel(const int4* __restrict__ counts, int64_t n, int64_t m,
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

__global__ __launch_bounds__(256) void tpg_ldstat_nan_kernel(double* __restrict__ x, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) x[i] = TPG_QNAN;
}

// v[r] of a lane belongs to row tpg_cd_row(r, lane), and the 32 lanes of a half wave share their 16 rows.  Four exchange steps
// halve the registers a lane still sums while doubling the lanes summed, a fifth joins the two halves of 16 lanes: 16 exchanges
// where a butterfly per register takes 80.  Returns, on every lane, the sum over the half wave of register
// ldstat_row_reduced_reg(lane).
__device__ __forceinline__ unsigned long long ldstat_row_reduce(unsigned long long (&v)[16], int lane) {
  tpg_static_for<4>([&](auto B) {
    constexpr int b = decltype(B)::value, H = 8 >> b;
    const bool up = (lane >> b) & 1;
    tpg_static_for<H>([&](auto I) {
      constexpr int i = decltype(I)::value;
      const unsigned long long send = up ? v[i] : v[i + H], keep = up ? v[i + H] : v[i];
      v[i] = keep + __shfl_xor(send, 1 << b);
    });
  });
  return v[0] + __shfl_xor(v[0], 16);
}
__device__ __forceinline__ int ldstat_row_reduced_reg(int lane) {
  return ((lane & 1) << 3) | ((lane & 2) << 1) | ((lane & 4) >> 1) | ((lane & 8) >> 3);
}

// Row tile jt = tile0 + blockIdx.x.
//   VALUES = false: score_q / n_partners (NULL together); sums = {valid pairs, valid pairs beyond the last bin} and behind them
//     {pairs, sum_q, sum_dist} x nbins (nbins = 0: no decay curve); pos == NULL: the distance of two loci is k - j.
//   VALUES = true: r2out[(j - j_lo) * stride + (k - j - 1)] for j_lo <= j < j_hi, NaN for an invalid pair.
template <bool VALUES>
__global__ __launch_bounds__(256) void tpg_ldstat_kernel(const uint4* __restrict__ L, int64_t Q, int n, int64_t m,
                                                         const int64_t* __restrict__ hi, const int32_t* __restrict__ sx,
                                                         const double* __restrict__ dd, int64_t tile0,
                                                         const int64_t* __restrict__ pos, int64_t bin_size, int nbins,
                                                         unsigned long long* __restrict__ score_q, int32_t* __restrict__ n_partners,
                                                         unsigned long long* __restrict__ sums, int64_t j_lo, int64_t j_hi,
                                                         double* __restrict__ r2out, int64_t stride) {
  __shared__ unsigned long long hist[VALUES ? 1 : LDSTAT_HIST_COPIES * 3 * LDSTAT_HIST_BINS];  // [copy][pairs, sum_q, sum_dist][bin]
  __shared__ unsigned long long s_rowq[32];
  __shared__ unsigned int s_rowc[32];
  __shared__ int64_t r_hi[32], r_pos[32];
  __shared__ int32_t r_sx[32];
  __shared__ double r_dd[32];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t jt = tile0 + blockIdx.x, j0 = jt * 32;
  if (tid < 32) {
    const int64_t j = j0 + tid;
    r_sx[tid] = j < m ? sx[j] : 0;
    r_dd[tid] = j < m ? dd[j] : 0.0;
    r_hi[tid] = j < m ? hi[j] : -1;  // a padding row has no neighbour
    r_pos[tid] = pos && j < m ? pos[j] : j;
    s_rowq[tid] = 0;
    s_rowc[tid] = 0;
  }
  const bool decay = !VALUES && nbins > 0, scores = !VALUES && score_q != nullptr;
  unsigned long long* const bins = sums + 2;
  if (decay)
    for (int x = tid; x < LDSTAT_HIST_COPIES * 3 * LDSTAT_HIST_BINS; x += 256) hist[x] = 0;
  const int NT = tpg_band_tiles(hi, jt, m);
  const int nsc = (NT + TPG_BAND_SC - 1) / TPG_BAND_SC;
  __syncthreads();
  unsigned long long* const myhist = hist + (VALUES ? 0 : (lane & (LDSTAT_HIST_COPIES - 1)) * 3 * LDSTAT_HIST_BINS);
  unsigned int nvalid = 0, nbeyond = 0;  // (at most 16 NT per lane, and NT < 2^13: LDSTAT_MAX_PAIRS bounds the window)
  for (int sc = 0; sc < nsc; sc++) {
    const int t0 = sc * TPG_BAND_SC + wv;
    v16f acc[TPG_BAND_TK];
#pragma unroll
    for (int i = 0; i < TPG_BAND_TK; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][r] = 0.f;  // (all four, as tpg_knn_band_kernel does)
    const int nt = tpg_band_contract<TPG_BAND_TK>(L, Q, jt, NT, sc, wv, lane, acc);
#pragma unroll
    for (int i = 0; i < TPG_BAND_TK; i++) {
      if (i < nt) {
        const int64_t k = (jt + t0 + 4 * i) * 32 + (lane & 31);
        const int32_t sxk = k < m ? sx[k] : 0;
        const double ddk = k < m ? dd[k] : 0.0;
        const int64_t pk = pos && k < m ? pos[k] : k;
        unsigned long long rowp[16], colp = 0;
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int row = tpg_cd_row(r, lane);
          const int64_t j = j0 + row;
          const bool inside = k > j && k <= r_hi[row];  // (k < m and j < m with it)
          const bool valid = inside && r_dd[row] > 0.0 && ddk > 0.0;
          unsigned long long p = 0;
          if (VALUES) {
            if (inside && j >= j_lo && j < j_hi)
              r2out[(j - j_lo) * stride + (k - j - 1)] =
                  valid ? host_ldstat_r2(n, (int32_t)acc[i][r], r_sx[row], sxk, r_dd[row], ddk) : TPG_QNAN;
          } else if (valid) {
            const uint64_t q = host_ldstat_q(host_ldstat_r2(n, (int32_t)acc[i][r], r_sx[row], sxk, r_dd[row], ddk));
            p = q | (1ull << LDSTAT_PACK_SHIFT);
            nvalid++;
            if (decay) {
              const int64_t dist = pk - r_pos[row];
              const int b = host_ldstat_bin(dist, bin_size, nbins);
              if (b >= nbins) {
                nbeyond++;
              } else if (b < LDSTAT_HIST_BINS) {
                atomicAdd(&myhist[b], 1ull);
                atomicAdd(&myhist[LDSTAT_HIST_BINS + b], (unsigned long long)q);
                atomicAdd(&myhist[2 * LDSTAT_HIST_BINS + b], (unsigned long long)dist);
              } else {
                atomicAdd(&bins[b], 1ull);
                atomicAdd(&bins[nbins + b], (unsigned long long)q);
                atomicAdd(&bins[2 * (int64_t)nbins + b], (unsigned long long)dist);
              }
            }
          }
          rowp[r] = p;
          colp += p;
        }
        if (scores) {
          colp += __shfl_xor(colp, 32);
          if (lane < 32 && colp) {  // (a pair inside the window: k < m)
            atomicAdd(&score_q[k], colp & LDSTAT_PACK_MASK);
            atomicAdd(&n_partners[k], (int32_t)(colp >> LDSTAT_PACK_SHIFT));
          }
          const unsigned long long rs = ldstat_row_reduce(rowp, lane);
          if (!(lane & 16) && rs) {
            const int row = tpg_cd_row(ldstat_row_reduced_reg(lane), lane);
            atomicAdd(&s_rowq[row], rs & LDSTAT_PACK_MASK);
            atomicAdd(&s_rowc[row], (unsigned int)(rs >> LDSTAT_PACK_SHIFT));
          }
        }
      }
    }
  }
  if (VALUES) return;
  __syncthreads();
  if (scores && tid < 32 && s_rowc[tid]) {  // (a row with a pair: j0 + tid < m)
    atomicAdd(&score_q[j0 + tid], s_rowq[tid]);
    atomicAdd(&n_partners[j0 + tid], (int32_t)s_rowc[tid]);
  }
  if (decay) {
    for (int x = tid; x < 3 * LDSTAT_HIST_BINS; x += 256) {
      const int which = x / LDSTAT_HIST_BINS, b = x % LDSTAT_HIST_BINS;
      unsigned long long s = 0;
#pragma unroll
      for (int c = 0; c < LDSTAT_HIST_COPIES; c++) s += hist[c * 3 * LDSTAT_HIST_BINS + x];
      if (s) atomicAdd(&bins[(int64_t)which * nbins + b], s);  // (s != 0: b < nbins)
    }
  }
  unsigned long long cv = nvalid, cb = nbeyond;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cv += __shfl_xor(cv, o);
    cb += __shfl_xor(cb, o);
  }
  if (lane == 0) {
    if (cv) atomicAdd(sums, cv);
    if (cb) atomicAdd(sums + 1, cb);
  }
}

// ---- host side --------------------------------------------------------------------------------------------------
namespace {

struct LdstatWindow {
  int64_t width = 0;  // max(hi[j] - j)
  int64_t pairs = 0;  // sum(hi[j] - j)
  int64_t tiles = 0;  // 32 x 32 tiles the band kernel contracts
};

// the window of "LD clumping": hi[j] in [j, m), non-decreasing -- and what the band of it amounts to
int ldstat_window(tpg_ctx* ctx, const int64_t* hi, int64_t m, HostIn<int64_t>& h, LdstatWindow* w) {
  TPG_TRY(h.init(ctx, hi, m));
  for (int64_t j = 0; j < m; j++) {
    TPG_REQUIRE(h[j] >= j && h[j] < m, TPG_EINVAL, "hi[%lld] = %lld outside [%lld, %lld)", (long long)j, (long long)h[j],
                (long long)j, (long long)m);
    TPG_REQUIRE(j == 0 || h[j] >= h[j - 1], TPG_EINVAL, "hi decreases at locus %lld", (long long)j);
    w->width = std::max(w->width, h[j] - j);
    w->pairs += h[j] - j;
    if ((j & 31) == 31 || j == m - 1) w->tiles += (h[j] >> 5) - (j >> 5) + 1;
  }
  return TPG_OK;
}

int ldstat_check_args(tpg_ctx* ctx, const tpg_view* v, const int64_t* hi) {
  TPG_REQUIRE(ctx && v && hi, TPG_EINVAL, "null argument");
  TPG_REQUIRE(v->m >= 1 && v->n >= 1, TPG_EINVAL, "empty view");
  TPG_REQUIRE(v->n < TPG_BAND_MAX_N, TPG_EUNSUPPORTED, "LD of 2^22 individuals or more");  // FP32 sums of dosage products
  TPG_REQUIRE(v->m < (1ll << 31) - 64, TPG_EUNSUPPORTED, "LD of 2^31 loci or more");
  return TPG_OK;
}

struct LdstatPrep {
  int32_t* d_sx = nullptr;
  double* d_dd = nullptr;
  int64_t* d_hi = nullptr;
};

// counts -> Sx, d; the window goes up; a missing genotype: TPG_ENUMERIC.  Nothing of the caller's is written.
int ldstat_prepare(tpg_ctx* ctx, const tpg_view* v, const HostIn<int64_t>& h, DevArena& sc, LdstatPrep* P) {
  const int64_t m = v->m;
  int32_t *d_counts = nullptr, *d_flags = nullptr;
  TPG_TRY(sc.get(&d_counts, 4 * (size_t)m));
  TPG_TRY(sc.get(&P->d_sx, (size_t)m));
  TPG_TRY(sc.get(&P->d_dd, (size_t)m));
  TPG_TRY(sc.get(&P->d_hi, (size_t)m));
  TPG_TRY(sc.get(&d_flags, 1));
  TPG_HIP(hipMemsetAsync(d_flags, 0, sizeof(int32_t), ctx->stream));
  TPG_TRY(tpg_view_need_L(ctx, v));
  TPG_TRY(tpg_launch_loci_counts(ctx, v, d_counts));
  TPG_LAUNCH(ctx, "ldstat_prep", tpg_ldstat_prep_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, (const int4*)d_counts, v->n, m,
             P->d_sx, P->d_dd, d_flags);
  TPG_CHECK_LAUNCH();
  TPG_HIP(tpg_upload(ctx, P->d_hi, h.p, sizeof(int64_t) * (size_t)m));
  int32_t flags = 0;
  TPG_HIP(tpg_fetch_small(ctx, &flags, d_flags, sizeof(flags)));
  TPG_REQUIRE(!(flags & 1), TPG_ENUMERIC, "LD statistics of a view with missing genotypes (impute it first)");
  return TPG_OK;
}

}  // namespace

extern "C" int tpg_ld_stats(tpg_ctx* ctx, const tpg_view* v, const int64_t* hi, const int64_t* pos, int64_t bin_size, int nbins,
                            int64_t* score_q, int32_t* n_partners, int64_t* bin_pairs, int64_t* bin_sum_q, int64_t* bin_sum_dist,
                            int64_t* report) {
  TpgEnter _enter(ctx);
  TPG_TRY(ldstat_check_args(ctx, v, hi));
  const bool scores = score_q || n_partners, decay = bin_pairs || bin_sum_q || bin_sum_dist;
  TPG_REQUIRE(!scores || (score_q && n_partners), TPG_EINVAL, "score_q and n_partners are NULL together or not at all");
  TPG_REQUIRE(!decay || (bin_pairs && bin_sum_q && bin_sum_dist), TPG_EINVAL,
              "bin_pairs, bin_sum_q and bin_sum_dist are NULL together or not at all");
  if (decay) {
    TPG_REQUIRE(bin_size >= 1, TPG_EINVAL, "bin_size = %lld is not positive", (long long)bin_size);
    TPG_REQUIRE(nbins >= 1 && nbins <= HOST_LDSTAT_MAX_BINS, TPG_EINVAL, "nbins = %d outside [1, %d]", nbins, HOST_LDSTAT_MAX_BINS);
  }
  const int64_t m = v->m;
  HostIn<int64_t> h, hp;
  LdstatWindow w;
  TPG_TRY(ldstat_window(ctx, hi, m, h, &w));
  TPG_REQUIRE(w.pairs < LDSTAT_MAX_PAIRS, TPG_EUNSUPPORTED, "LD statistics of %lld pairs of loci (2^33 or more)", (long long)w.pairs);
  if (decay && pos) {
    TPG_TRY(hp.init(ctx, pos, m));
    int64_t far = 0;  // the largest distance inside a window
    for (int64_t j = 0; j < m; j++) {
      TPG_REQUIRE(hp[j] > -LDSTAT_MAX_POS && hp[j] < LDSTAT_MAX_POS, TPG_EINVAL, "pos[%lld] = %lld is not a position", (long long)j,
                  (long long)hp[j]);
      // neighbours j and j + 1 in ascending order is ascending order inside every window: hi does not decrease
      TPG_REQUIRE(h[j] == j || hp[j + 1] >= hp[j], TPG_EINVAL, "pos decreases at locus %lld, inside a window", (long long)j + 1);
      far = std::max(far, hp[h[j]] - hp[j]);
    }
    // sum_dist of a bin: fewer than 2^33 pairs, each closer than `far` and than the end of the last bin
    const __int128 reach = std::min<__int128>((__int128)far, (__int128)bin_size * nbins);
    TPG_REQUIRE(reach * (__int128)std::max<int64_t>(w.pairs, 1) < ((__int128)1 << 63), TPG_EUNSUPPORTED,
                "the distances of the pairs in a bin may add up to 2^63 or more");
  }
  DevArena sc;
  LdstatPrep P;
  TPG_TRY(ldstat_prepare(ctx, v, h, sc, &P));
  int64_t* d_pos = nullptr;
  if (decay && pos) {
    TPG_TRY(sc.get(&d_pos, (size_t)m));
    TPG_HIP(tpg_upload(ctx, d_pos, hp.p, sizeof(int64_t) * (size_t)m));
  }
  const int nb = decay ? nbins : 0;
  unsigned long long* d_sums = nullptr;  // {valid, beyond}, then {pairs, sum_q, sum_dist} x nb
  TPG_TRY(sc.get(&d_sums, 2 + 3 * (size_t)nb));
  TPG_HIP(hipMemsetAsync(d_sums, 0, sizeof(unsigned long long) * (2 + 3 * (size_t)nb), ctx->stream));
  const unsigned long long* d_bins = d_sums + 2;
  OutBuf oq, op;
  if (scores) {
    TPG_TRY(oq.init(score_q, sizeof(uint64_t) * (size_t)m));
    TPG_TRY(op.init(n_partners, sizeof(int32_t) * (size_t)m));
    TPG_HIP(hipMemsetAsync(oq.d, 0, sizeof(uint64_t) * (size_t)m, ctx->stream));
    TPG_HIP(hipMemsetAsync(op.d, 0, sizeof(int32_t) * (size_t)m, ctx->stream));
  }
  if (w.width > 0) {
    TPG_LAUNCH(ctx, "ldstat_band", tpg_ldstat_kernel<false>, dim3((unsigned)ceil_div(m, 32)), dim3(256), 0, (const uint4*)v->L, v->Q,
               (int)v->n, m, (const int64_t*)P.d_hi, (const int32_t*)P.d_sx, (const double*)P.d_dd, (int64_t)0, (const int64_t*)d_pos,
               decay ? bin_size : (int64_t)1, nb, scores ? oq.dev<unsigned long long>() : nullptr, scores ? op.dev<int32_t>() : nullptr,
               d_sums, (int64_t)0, (int64_t)0, (double*)nullptr, (int64_t)0);
    TPG_CHECK_LAUNCH();
  }
  unsigned long long cnt[2] = {0, 0};
  TPG_HIP(tpg_fetch_small(ctx, cnt, d_sums, sizeof(cnt)));  // waits for the kernel
  if (scores) {
    TPG_TRY(oq.commit(ctx));
    TPG_TRY(op.commit(ctx));
  }
  if (decay) {
    TPG_TRY(tpg_deliver(ctx, bin_pairs, (const int64_t*)d_bins, (size_t)nbins));
    TPG_TRY(tpg_deliver(ctx, bin_sum_q, (const int64_t*)(d_bins + nbins), (size_t)nbins));
    TPG_TRY(tpg_deliver(ctx, bin_sum_dist, (const int64_t*)(d_bins + 2 * (size_t)nbins), (size_t)nbins));
    TPG_HIP(hipStreamSynchronize(ctx->stream));
  }
  if (report) {
    report[0] = w.pairs;
    report[1] = (int64_t)cnt[0];
    report[2] = (int64_t)cnt[1];
    report[3] = w.width > 0 ? w.tiles : 0;
  }
  return TPG_OK;
}

extern "C" int tpg_ld_band_r2(tpg_ctx* ctx, const tpg_view* v, const int64_t* hi, int64_t j0, int64_t j1, double* r2, int64_t stride) {
  TpgEnter _enter(ctx);
  TPG_TRY(ldstat_check_args(ctx, v, hi));
  TPG_REQUIRE(r2, TPG_EINVAL, "null argument");
  const int64_t m = v->m;
  TPG_REQUIRE(j0 >= 0 && j0 < j1 && j1 <= m, TPG_EINVAL, "[j0, j1) = [%lld, %lld) is not a range of the %lld loci", (long long)j0,
              (long long)j1, (long long)m);
  TPG_REQUIRE(stride >= 1 && stride <= LDSTAT_MAX_VALUES && (j1 - j0) * stride <= LDSTAT_MAX_VALUES, TPG_EINVAL,
              "(j1 - j0) * stride = %lld x %lld outside [1, 2^26]", (long long)(j1 - j0), (long long)stride);
  HostIn<int64_t> h;
  LdstatWindow w;
  TPG_TRY(ldstat_window(ctx, hi, m, h, &w));
  int64_t need = 0;
  for (int64_t j = j0; j < j1; j++) need = std::max(need, h[j] - j);
  TPG_REQUIRE(stride >= need, TPG_EINVAL, "stride = %lld, the window of the region needs %lld", (long long)stride, (long long)need);
  DevArena sc;
  LdstatPrep P;
  TPG_TRY(ldstat_prepare(ctx, v, h, sc, &P));
  const int64_t count = (j1 - j0) * stride;
  OutBuf o;
  TPG_TRY(o.init(r2, sizeof(double) * (size_t)count));
  TPG_LAUNCH(ctx, "ldstat_nan", tpg_ldstat_nan_kernel, dim3((unsigned)ceil_div(count, 256)), dim3(256), 0, o.dev<double>(), count);
  TPG_CHECK_LAUNCH();
  if (need > 0) {
    const int64_t tile0 = j0 >> 5, tiles = ((j1 - 1) >> 5) - tile0 + 1;
    TPG_LAUNCH(ctx, "ldstat_r2", tpg_ldstat_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, (const uint4*)v->L, v->Q, (int)v->n, m,
               (const int64_t*)P.d_hi, (const int32_t*)P.d_sx, (const double*)P.d_dd, tile0, (const int64_t*)nullptr, (int64_t)1, 0,
               (unsigned long long*)nullptr, (int32_t*)nullptr, (unsigned long long*)nullptr, j0, j1, o.dev<double>(), stride);
    TPG_CHECK_LAUNCH();
  }
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  TPG_TRY(o.commit(ctx));
  return TPG_OK;
}
