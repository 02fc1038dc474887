// autosvd.hip -- PCA with removal of long-range LD regions (include/tpg.h "autoSVD"): clump, SVD, robust distance of the
// loadings, Gaussian rolling mean per chromosome, Tukey fence with the medcouple, remove the outliers, repeat.
//
// Replaces the arithmetic behind R/gt_pca_autoSVD.R (bigsnpr::snp_autoSVD with bigutilsr::rollmean / tukey_mc_up and
// robustbase::mc -- third-party, not among the reference's sources: the definition is the one include/tpg.h gives).
//
// Clumping, the SVD and the OGK distance are the library's entry points (ld.hip, pca.hip, pcadapt.hip).  New here:
//   * asv_gather_kernel: the view of a subset of another view's loci.  In the L layout a locus is one 16-byte lane piece per
//     half (h) and individual block (q), so a sub-view is a pure uint4 gather; T, T4 and the counts are rebuilt on demand.
//   * asv_rollmean_kernel: one thread per locus, the weight table in LDS, the window clipped to the chromosome segment.
//   * the fence: ONE radix sort of the order-preserving keys gives the quartiles and the median.  The sorted array also IS the
//     two operands of the medcouple: with z = x - med ascending, A = {z > 0} is its suffix and B = {|z| : z <= 0} its prefix
//     read backwards.  The two middle ratios b / a are found by bisection over the 63-bit pattern of a non-negative double:
//     per bit one launch of asv_mc_step_kernel, in which every row a binary-searches B for the prefix with b / a <= t and adds
//     its length to a 64-bit count.  The n+ x n- ratios are never formed.  Every launch replays the earlier counts to know its
//     prefix, so the 63 steps need no host round trip: two small fetches per fence (the sorted statistics, the two ratios).
// Integer atomics only; a result depends on the inputs alone.
#include "common.h"
#include "devfrag.h"
#include "host/host_autosvd.h"

#include <hipcub/hipcub.hpp>
#include <math.h>

#include <algorithm>

namespace {

constexpr int ASV_MAX_RADIUS = 1024;
constexpr int MC_STEPS = 63;


inline unsigned grid_for(int64_t count) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(count, 256), 4096)); }

// ---- the sub-view ------------------------------------------------------------------------------------------------------
__global__ void asv_check_idx_kernel(const int64_t* __restrict__ idx, int64_t count, int64_t m, int* __restrict__ flag) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x)
    if (idx[i] < 0 || idx[i] >= m) flag[0] = 1;
}

// out block (lt', q), lane (r', h) <- L block (lt, q), lane (r, h) with 32 lt + r = idx[32 lt' + r']; padding loci: code 3
__global__ void asv_gather_kernel(const uint4* __restrict__ L, uint4* __restrict__ out, const int64_t* __restrict__ idx, int64_t count,
                                  int64_t Q, int64_t total) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(t & 63), r = lane & 31, h = lane >> 5;
    const int64_t blk = t >> 6, q = blk % Q, lt = blk / Q, jn = lt * 32 + r;
    uint4 val = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    if (jn < count) {
      const int64_t j = idx[jn];
      val = L[((j >> 5) * Q + q) * 64 + (j & 31) + 32 * h];
    }
    out[t] = val;
  }
}

// d_idx: device, every entry already known to lie in [0, v->m)
int select_loci_device(tpg_ctx* ctx, const tpg_view* v, const int64_t* d_idx, int64_t count, tpg_view** out) {
  TPG_TRY(tpg_view_need_L(ctx, v));
  ViewPtr w(new tpg_view(ctx, v->n, count));
  TPG_HIP(tpg_pmalloc((void**)&w->L, w->bytes_each));
  const int64_t total = (int64_t)(w->bytes_each / 16);
  TPG_LAUNCH(ctx, "autosvd_gather", asv_gather_kernel, dim3(grid_for(total)), dim3(256), 0, (const uint4*)v->L, w->L, d_idx, count, v->Q, total);
  TPG_CHECK_LAUNCH();
  *out = w.release();
  return TPG_OK;
}

// ---- rolling mean ------------------------------------------------------------------------------------------------------
// seg: nseg + 1 non-decreasing starts, seg[0] = 0, seg[nseg] = m (an empty segment owns no locus)
__global__ __launch_bounds__(256) void asv_rollmean_kernel(const double* __restrict__ x, int64_t m, const int64_t* __restrict__ seg, int nseg,
                                                           int R, const double* __restrict__ w, double* __restrict__ out) {
  extern __shared__ double w_lds[];
  for (int i = threadIdx.x; i < 2 * R + 1; i += blockDim.x) w_lds[i] = w[i];
  __syncthreads();
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = nseg;  // the last s with seg[s] <= j
    while (hi - lo > 1) {
      const int mid = (lo + hi) / 2;
      if (seg[mid] <= j) lo = mid;
      else hi = mid;
    }
    const int64_t a = seg[lo], b = seg[lo + 1];
    double num = 0.0, den = 0.0;
    for (int i = 0; i <= 2 * R; i++) {
      const int64_t p = j - R + i;
      if (p >= a && p < b) {
        num += w_lds[i] * x[p];
        den += w_lds[i];
      }
    }
    out[j] = num / den;
  }
}

// h_seg: the host copy of the starts, d_seg the device copy; allow_empty: a segment without loci is skipped, not refused
int rollmean_device(tpg_ctx* ctx, const double* d_x, int64_t m, const int64_t* h_seg, const int64_t* d_seg, int64_t nseg, int radius,
                    bool allow_empty, double* d_out) {
  TPG_REQUIRE(radius >= 0 && radius <= ASV_MAX_RADIUS, TPG_EINVAL, "roll_size = %d out of [0, %d]", radius, ASV_MAX_RADIUS);
  TPG_REQUIRE(nseg >= 1 && nseg < 2147483647ll && h_seg[0] == 0 && h_seg[nseg] == m, TPG_EINVAL, "segments must tile [0, m)");
  const int64_t len = 2 * (int64_t)radius + 1;
  for (int64_t s = 0; s < nseg; s++) {
    const int64_t l = h_seg[s + 1] - h_seg[s];
    TPG_REQUIRE(l >= 0 && (l > 0 || allow_empty), TPG_EINVAL, "segment starts must increase");
    TPG_REQUIRE(l == 0 || l >= len, TPG_EINVAL, "roll_size exceeds the number of variants on at least one chromosome");
  }
  if (radius == 0) {
    if (d_out != d_x) TPG_HIP(tpg_copy_dev(ctx, d_out, d_x, sizeof(double) * (size_t)m));
    return TPG_OK;
  }
  std::vector<double> w((size_t)len);
  host_rollmean_weights(radius, w.data());
  DevBuf d_w;
  TPG_TRY(d_w.alloc_n<double>((size_t)len));
  TPG_HIP(tpg_push_small(ctx, d_w.p, w.data(), sizeof(double) * (size_t)len));
  TPG_LAUNCH(ctx, "autosvd_rollmean", asv_rollmean_kernel, dim3(grid_for(m)), dim3(256), sizeof(double) * (size_t)len, d_x, m, d_seg, (int)nseg,
             radius, (const double*)d_w.p, d_out);
  TPG_CHECK_LAUNCH();
  return TPG_OK;
}

// ---- the fence ---------------------------------------------------------------------------------------------------------
// keys[i]: the order-preserving key of x[i] + 0.0; a value that is not finite gets the largest key and is not counted
__global__ void asv_keys_kernel(const double* __restrict__ x, int64_t count, uint64_t* __restrict__ keys, unsigned long long* __restrict__ n_finite) {
  unsigned long long mine = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t u = (uint64_t)__double_as_longlong(x[i] + 0.0);
    const bool ok = (u & TPG_D_EXP_MASK) != TPG_D_EXP_MASK;
    keys[i] = ok ? TPG_DKEY(u) : ~0ull;
    mine += ok ? 1ull : 0ull;
  }
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_finite, mine);
}

struct TukeyStats {
  long long c;       // finite values
  long long pA, p0;  // first sorted index with x - med > 0, with x - med >= 0
  double q1, q3, med;
};

// one thread: the quartiles and the median from the sorted keys, and where z = x - med changes sign
__global__ void asv_stats_kernel(const uint64_t* __restrict__ s, const unsigned long long* __restrict__ n_finite, TukeyStats* __restrict__ out) {
  const long long c = (long long)n_finite[0];
  TukeyStats st;
  st.c = c;
  st.pA = st.p0 = 0;
  st.q1 = st.q3 = st.med = TPG_QNAN;
  if (c > 0) {
    const double ps[2] = {0.25, 0.75};
    double q[2];
    for (int i = 0; i < 2; i++) {
      const double h = (double)(c - 1) * ps[i];
      const long long lo = (long long)floor(h), up = lo + 1 < c ? lo + 1 : c - 1;
      const double a = tpg_dunkey(s[lo]), b = tpg_dunkey(s[up]);
      q[i] = a + (h - (double)lo) * (b - a);
    }
    st.q1 = q[0];
    st.q3 = q[1];
    st.med = (c & 1) ? tpg_dunkey(s[(c - 1) / 2]) : (tpg_dunkey(s[c / 2 - 1]) + tpg_dunkey(s[c / 2])) / 2;
    long long lo = 0, hi = c;  // first index with z > 0
    while (lo < hi) {
      const long long mid = (lo + hi) / 2;
      if (tpg_dunkey(s[mid]) - st.med > 0.0) hi = mid;
      else lo = mid + 1;
    }
    st.pA = lo;
    lo = 0, hi = st.pA;  // first index with z >= 0
    while (lo < hi) {
      const long long mid = (lo + hi) / 2;
      if (tpg_dunkey(s[mid]) - st.med >= 0.0) hi = mid;
      else lo = mid + 1;
    }
    st.p0 = lo;
  }
  out[0] = st;
}

// the prefixes the first `steps` launches have decided, one per rank: bit 62 - s is set iff fewer than rank + 1 ratios are
// <= the candidate with that bit clear and every lower bit set
__device__ __forceinline__ void asv_mc_replay(const unsigned long long* __restrict__ cnt, int steps, uint64_t k, uint64_t nB, uint64_t rank_lo,
                                              uint64_t rank_hi, uint64_t& P0, uint64_t& P1) {
  P0 = P1 = 0;
  for (int s = 0; s < steps; s++) {
    const uint64_t bit = 1ull << (62 - s), low = bit - 1;
    if (cnt[2 * s] + tpg_mc_tie_count(k, nB, P0 | low) < rank_lo + 1) P0 |= bit;
    if (cnt[2 * s + 1] + tpg_mc_tie_count(k, nB, P1 | low) < rank_hi + 1) P1 |= bit;
  }
}

// how many b of B (ascending: B[j] = |s[pA - 1 - j] - med|, j < pA) have b / a <= the ratio with pattern cand: a prefix of B
__device__ __forceinline__ uint64_t asv_mc_prefix(const uint64_t* __restrict__ s, long long pA, double med, double a, uint64_t cand) {
  long long lo = 0, hi = pA;
  while (lo < hi) {
    const long long mid = (lo + hi) / 2;
    const double b = fabs(tpg_dunkey(s[pA - 1 - mid]) - med);
    if ((uint64_t)__double_as_longlong(b / a) <= cand) lo = mid + 1;
    else hi = mid;
  }
  return (uint64_t)lo;
}

// step `step` of the bisection: cnt[2 step + w] += sum over the rows a = s[i] - med, pA <= i < c, of the prefix length at
// the candidate of rank w
__global__ __launch_bounds__(256) void asv_mc_step_kernel(const uint64_t* __restrict__ s, long long pA, long long c, long long k, double med,
                                                          uint64_t rank_lo, uint64_t rank_hi, int step, unsigned long long* __restrict__ cnt) {
  __shared__ uint64_t cand[2];
  if (threadIdx.x == 0) {
    uint64_t P0, P1;
    asv_mc_replay(cnt, step, (uint64_t)k, (uint64_t)pA, rank_lo, rank_hi, P0, P1);
    const uint64_t low = (1ull << (62 - step)) - 1;
    cand[0] = P0 | low;
    cand[1] = P1 | low;
  }
  __syncthreads();
  const uint64_t c0 = cand[0], c1 = cand[1];
  unsigned long long mine0 = 0, mine1 = 0;
  for (long long i = pA + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < c; i += (long long)gridDim.x * blockDim.x) {
    const double a = tpg_dunkey(s[i]) - med;
    const uint64_t n0 = asv_mc_prefix(s, pA, med, a, c0);
    mine0 += n0;
    mine1 += c1 == c0 ? n0 : asv_mc_prefix(s, pA, med, a, c1);
  }
  for (int o = 32; o > 0; o >>= 1) {
    mine0 += __shfl_xor(mine0, o);
    mine1 += __shfl_xor(mine1, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (mine0) atomicAdd(&cnt[2 * step], mine0);
    if (mine1) atomicAdd(&cnt[2 * step + 1], mine1);
  }
}

__global__ void asv_mc_final_kernel(const unsigned long long* __restrict__ cnt, long long k, long long nB, uint64_t rank_lo, uint64_t rank_hi,
                                    uint64_t* __restrict__ out) {
  uint64_t P0, P1;
  asv_mc_replay(cnt, MC_STEPS, (uint64_t)k, (uint64_t)nB, rank_lo, rank_hi, P0, P1);
  out[0] = P0;
  out[1] = P1;
}

// report = {n_finite, q1, q3, med, mc, coef, thr} of d_x[count]; with_fence false: coef and thr stay NaN
int tukey_device(tpg_ctx* ctx, const double* d_x, int64_t count, double alpha, bool with_fence, double* report) {
  TPG_REQUIRE(count >= 0 && count < 2147483647ll, TPG_EUNSUPPORTED, "a fence over %lld values", (long long)count);
  for (int i = 1; i < 7; i++) report[i] = NAN;
  report[0] = 0;
  if (count == 0) return TPG_OK;
  DevArena sc;
  uint64_t *d_keys, *d_sorted, *d_ratio;
  unsigned long long *d_nf, *d_cnt;
  TukeyStats* d_st;
  TPG_TRY(sc.get(&d_keys, (size_t)count));
  TPG_TRY(sc.get(&d_sorted, (size_t)count));
  TPG_TRY(sc.get(&d_ratio, 2));
  TPG_TRY(sc.get(&d_nf, 1));
  TPG_TRY(sc.get(&d_cnt, 2 * (size_t)MC_STEPS));
  TPG_TRY(sc.get(&d_st, 1));
  TPG_HIP(hipMemsetAsync(d_nf, 0, sizeof(unsigned long long), ctx->stream));
  TPG_HIP(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * 2 * MC_STEPS, ctx->stream));
  TPG_LAUNCH(ctx, "autosvd_keys", asv_keys_kernel, dim3(grid_for(count)), dim3(256), 0, d_x, count, d_keys, d_nf);
  {
    size_t t_sort = 0;
    TPG_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, t_sort, d_keys, d_sorted, (int)count, 0, 64, ctx->stream));
    uint8_t* d_tmp = nullptr;
    TPG_TRY(sc.get(&d_tmp, t_sort));
    ProfScope ps(ctx, "autosvd_sort");
    TPG_HIP(hipcub::DeviceRadixSort::SortKeys(d_tmp, t_sort, d_keys, d_sorted, (int)count, 0, 64, ctx->stream));
  }
  TPG_LAUNCH(ctx, "autosvd_stats", asv_stats_kernel, dim3(1), dim3(1), 0, (const uint64_t*)d_sorted, (const unsigned long long*)d_nf, d_st);
  TPG_CHECK_LAUNCH();
  TukeyStats st;
  TPG_HIP(tpg_fetch_small(ctx, &st, d_st, sizeof(st)));
  report[0] = (double)st.c;
  if (st.c == 0) return TPG_OK;
  const long long k = st.pA - st.p0, nB = st.pA, nA = st.c - st.pA;
  const uint64_t N = (uint64_t)(nA + k) * (uint64_t)nB, rank_lo = (N - 1) / 2, rank_hi = N / 2;
  for (int step = 0; step < MC_STEPS; step++)
    TPG_LAUNCH(ctx, "autosvd_mc_step", asv_mc_step_kernel, dim3(grid_for(nA)), dim3(256), 0, (const uint64_t*)d_sorted, st.pA, st.c, k, st.med,
               rank_lo, rank_hi, step, d_cnt);
  TPG_LAUNCH(ctx, "autosvd_mc_final", asv_mc_final_kernel, dim3(1), dim3(1), 0, (const unsigned long long*)d_cnt, k, nB, rank_lo, rank_hi, d_ratio);
  TPG_CHECK_LAUNCH();
  uint64_t ratio[2];
  TPG_HIP(tpg_fetch_small(ctx, ratio, d_ratio, sizeof(ratio)));
  report[1] = st.q1;
  report[2] = st.q3;
  report[3] = st.med;
  report[4] = host_mc_from_ratio_bits(ratio[0], ratio[1]);
  if (with_fence) host_tukey_fence((double)st.c, st.q1, st.q3, report[4], alpha, &report[5], &report[6]);
  return TPG_OK;
}

// ---- the driver's small kernels ----------------------------------------------------------------------------------------
// exclude[j] = minor allele count below min_mac; flag: a missing genotype met
__global__ void asv_mac_kernel(const int4* __restrict__ counts, int64_t m, int64_t n, int64_t min_mac, uint8_t* __restrict__ exclude,
                               int* __restrict__ flag) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const int4 c = counts[j];
    if (c.w != 0) flag[0] = 1;
    const int64_t sx = (int64_t)c.y + 2 * (int64_t)c.z, mac = sx < 2 * n - sx ? sx : 2 * n - sx;
    exclude[j] = mac < min_mac ? 1 : 0;
  }
}
__global__ void asv_start_kernel(const uint8_t* __restrict__ exclude, int64_t m, int64_t* __restrict__ iota, uint8_t* __restrict__ keep) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    iota[j] = j;
    if (exclude) keep[j] = exclude[j] ? 0 : 1;
  }
}
// S = sqrt(dist); flag: a dist that is not finite
__global__ void asv_sqrt_kernel(const double* __restrict__ dist, int64_t count, double* __restrict__ S, int* __restrict__ flag) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < count; j += (int64_t)gridDim.x * blockDim.x) {
    const double d = dist[j];
    if (!(fabs(d) <= 1.79769313486231570815e308)) flag[0] = 1;
    S[j] = sqrt(d);
  }
}
// seg[r] = the first kept position whose locus is >= run_start[r] (idx ascending), seg[nruns] = count
__global__ void asv_seg_kernel(const int64_t* __restrict__ idx, int64_t count, const int64_t* __restrict__ run_start, int nruns,
                               int64_t* __restrict__ seg) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > nruns) return;
  int64_t lo = 0, hi = count;
  if (r == nruns) lo = count;
  while (lo < hi) {
    const int64_t mid = (lo + hi) / 2;
    if (idx[mid] >= run_start[r]) hi = mid;
    else lo = mid + 1;
  }
  seg[r] = lo;
}
__global__ void asv_fence_kernel(const double* __restrict__ S2, int64_t count, double thr, uint8_t* __restrict__ keep, uint8_t* __restrict__ out) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < count; j += (int64_t)gridDim.x * blockDim.x) {
    const bool o = S2[j] > thr;
    out[j] = o ? 1 : 0;
    keep[j] = o ? 0 : 1;
  }
}

// d_out <- the entries of d_in[count] whose flag is set, in order; *h_sel = how many
int select_flagged(tpg_ctx* ctx, const int64_t* d_in, const uint8_t* d_flags, int64_t* d_out, int64_t count, int64_t* d_num, int64_t* h_sel) {
  TPG_REQUIRE(count < 2147483647ll, TPG_EUNSUPPORTED, "a selection over %lld loci", (long long)count);
  size_t t_sel = 0;
  TPG_HIP(hipcub::DeviceSelect::Flagged(nullptr, t_sel, d_in, d_flags, d_out, d_num, (int)count, ctx->stream));
  DevBuf tmp;
  TPG_TRY(tmp.alloc(t_sel));
  {
    ProfScope ps(ctx, "autosvd_compact");
    TPG_HIP(hipcub::DeviceSelect::Flagged(tmp.p, t_sel, d_in, d_flags, d_out, d_num, (int)count, ctx->stream));
  }
  TPG_HIP(tpg_fetch_small(ctx, h_sel, d_num, sizeof(int64_t)));
  return TPG_OK;
}

int fetch_i64(tpg_ctx* ctx, std::vector<int64_t>& host, const int64_t* d_src, size_t count) {
  host.resize(count);
  if (!count) return TPG_OK;
  if (sizeof(int64_t) * count <= tpg_ctx::MAIL_FETCH_BYTES) TPG_HIP(tpg_fetch_small(ctx, host.data(), d_src, sizeof(int64_t) * count));
  else TPG_HIP(tpg_download(ctx, host.data(), d_src, sizeof(int64_t) * count));
  return TPG_OK;
}

}  // namespace

struct AsvIter {
  int64_t n_kept = 0, n_out = 0;
  double report[7] = {0, 0, 0, 0, 0, 0, 0};
  std::vector<int64_t> pos, idx0;  // the outliers: position in this iteration's kept list, locus of the view
};

// the result of one tpg_pca_auto_svd (host memory, owned by the library)
struct tpg_autosvd {
  int64_t n = 0, m = 0, count = 0;
  int k = 0, iters = 0, converged = 0;
  std::vector<double> d, u, v, center, scale;
  double fro = 0;
  std::vector<int64_t> idx0;
  std::vector<int32_t> chrom;
  std::vector<AsvIter> hist;
};

extern "C" int tpg_view_select_loci(tpg_ctx* ctx, const tpg_view* v, const int64_t* idx0, int64_t count, tpg_view** out) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && out, TPG_EINVAL, "null argument");
  TPG_REQUIRE(count >= 1 && idx0, TPG_EINVAL, "a selection of %lld loci", (long long)count);
  InBuf ii;
  TPG_TRY(ii.init(ctx, idx0, sizeof(int64_t) * (size_t)count));
  DevBuf d_flag;
  TPG_TRY(d_flag.alloc(16));
  TPG_HIP(hipMemsetAsync(d_flag.p, 0, 16, ctx->stream));
  TPG_LAUNCH(ctx, "autosvd_check_idx", asv_check_idx_kernel, dim3(grid_for(count)), dim3(256), 0, ii.dev<int64_t>(), count, v->m, d_flag.as<int>());
  TPG_CHECK_LAUNCH();
  int flag = 0;
  TPG_HIP(tpg_fetch_small(ctx, &flag, d_flag.p, sizeof(flag)));
  TPG_REQUIRE(!flag, TPG_EINVAL, "a locus index outside [0, %lld)", (long long)v->m);
  TPG_TRY(select_loci_device(ctx, v, ii.dev<int64_t>(), count, out));
  TPG_HIP(hipStreamSynchronize(ctx->stream));  // the index buffer may be the call's own
  return TPG_OK;
}

extern "C" int tpg_qnorm_upper(double p, double* x) {
  TPG_REQUIRE(x, TPG_EINVAL, "null argument");
  TPG_REQUIRE(p > 0.0 && p < 1.0, TPG_EINVAL, "p = %g outside (0, 1)", p);
  *x = host_qnorm_upper(p);
  return TPG_OK;
}

extern "C" int tpg_rollmean_weights(int radius, double* w) {
  TPG_REQUIRE(w, TPG_EINVAL, "null argument");
  TPG_REQUIRE(radius >= 0 && radius <= ASV_MAX_RADIUS, TPG_EINVAL, "roll_size = %d out of [0, %d]", radius, ASV_MAX_RADIUS);
  host_rollmean_weights(radius, w);
  return TPG_OK;
}

extern "C" int tpg_rollmean_segments(tpg_ctx* ctx, const double* x, int64_t m, const int64_t* seg_start, int64_t nseg, int radius,
                                     double* out) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && x && seg_start && out, TPG_EINVAL, "null argument");
  TPG_REQUIRE(m >= 1 && nseg >= 1 && nseg <= m, TPG_EINVAL, "%lld values in %lld segments", (long long)m, (long long)nseg);
  HostIn<int64_t> hs;
  InBuf is, ix;
  TPG_TRY(hs.init(ctx, seg_start, nseg + 1));
  TPG_TRY(is.init(ctx, seg_start, sizeof(int64_t) * (size_t)(nseg + 1)));
  TPG_TRY(ix.init(ctx, x, sizeof(double) * (size_t)m));
  DevBuf d_out;  // x and out may be the same array
  TPG_TRY(d_out.alloc_n<double>((size_t)m));
  TPG_TRY(rollmean_device(ctx, ix.dev<double>(), m, hs.p, is.dev<int64_t>(), nseg, radius, false, d_out.as<double>()));
  OutBuf oo;
  TPG_TRY(oo.init(out, sizeof(double) * (size_t)m));
  TPG_HIP(tpg_copy_dev(ctx, oo.dev<double>(), d_out.p, sizeof(double) * (size_t)m));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return oo.commit(ctx);
}

extern "C" int tpg_medcouple(tpg_ctx* ctx, const double* x, int64_t count, double* mc) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && mc && (x || count == 0), TPG_EINVAL, "null argument");
  InBuf ix;
  if (count > 0) TPG_TRY(ix.init(ctx, x, sizeof(double) * (size_t)count));
  double report[7];
  TPG_TRY(tukey_device(ctx, ix.dev<double>(), count, 0.0, false, report));
  *mc = report[4];
  return TPG_OK;
}

extern "C" int tpg_tukey_mc_up(tpg_ctx* ctx, const double* x, int64_t count, double alpha, double* report) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && report && (x || count == 0), TPG_EINVAL, "null argument");
  TPG_REQUIRE(alpha > 0.0 && alpha < 1.0, TPG_EINVAL, "alpha = %g outside (0, 1)", alpha);
  InBuf ix;
  if (count > 0) TPG_TRY(ix.init(ctx, x, sizeof(double) * (size_t)count));
  double rep[7];
  TPG_TRY(tukey_device(ctx, ix.dev<double>(), count, alpha, true, rep));
  std::copy(rep, rep + 7, report);
  return TPG_OK;
}

extern "C" int tpg_pca_auto_svd(tpg_ctx* ctx, const tpg_view* v, const int32_t* chrom, const int64_t* hi, int k, double thr_r2,
                                int roll_size, double alpha_tukey, int64_t min_mac, int max_iter, void** out) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && chrom && out, TPG_EINVAL, "null argument");
  const int64_t n = v->n, m = v->m;
  TPG_REQUIRE(m >= 1 && m < 2147483647ll, TPG_EINVAL, "a view of %lld loci", (long long)m);
  TPG_REQUIRE(k >= 1 && k <= TPG_PCADAPT_MAX_K, TPG_EINVAL, "k = %d out of [1, %d]", k, TPG_PCADAPT_MAX_K);
  TPG_REQUIRE(roll_size >= 0 && roll_size <= ASV_MAX_RADIUS, TPG_EINVAL, "roll_size = %d out of [0, %d]", roll_size, ASV_MAX_RADIUS);
  TPG_REQUIRE(alpha_tukey > 0.0 && alpha_tukey < 1.0, TPG_EINVAL, "alpha_tukey = %g outside (0, 1)", alpha_tukey);
  TPG_REQUIRE(min_mac >= 0 && max_iter >= 0, TPG_EINVAL, "min_mac = %lld, max_iter = %d", (long long)min_mac, max_iter);
  std::unique_ptr<tpg_autosvd> res(new tpg_autosvd);
  res->n = n;
  res->m = m;
  res->k = k;
  // chromosomes: every one a contiguous run
  HostIn<int32_t> hc;
  TPG_TRY(hc.init(ctx, chrom, m));
  res->chrom.assign(hc.p, hc.p + m);
  std::vector<int64_t> run_start;
  {
    std::set<int32_t> seen;
    for (int64_t j = 0; j < m; j++)
      if (j == 0 || hc[j] != hc[j - 1]) {
        TPG_REQUIRE(seen.insert(hc[j]).second, TPG_EINVAL, "loci are not ordered: chromosome %d appears in more than one run", (int)hc[j]);
        run_start.push_back(j);
      }
  }
  const int nruns = (int)run_start.size();
  TPG_REQUIRE(sizeof(int64_t) * (size_t)(nruns + 1) <= tpg_ctx::MAIL_PUSH_MAX, TPG_EUNSUPPORTED, "%d chromosomes", nruns);

  DevArena sc;
  int32_t* d_counts;
  uint8_t *d_excl, *d_keep, *d_outf;
  int64_t *d_iota, *d_idx, *d_idx2, *d_opos, *d_oidx, *d_num, *d_runs, *d_seg;
  double *d_dist, *d_S, *d_S2;
  int* d_flag;
  TPG_TRY(sc.get(&d_counts, 4 * (size_t)m));
  TPG_TRY(sc.get(&d_excl, (size_t)m));
  TPG_TRY(sc.get(&d_keep, (size_t)m));
  TPG_TRY(sc.get(&d_outf, (size_t)m));
  TPG_TRY(sc.get(&d_iota, (size_t)m));
  TPG_TRY(sc.get(&d_idx, (size_t)m));
  TPG_TRY(sc.get(&d_idx2, (size_t)m));
  TPG_TRY(sc.get(&d_opos, (size_t)m));
  TPG_TRY(sc.get(&d_oidx, (size_t)m));
  TPG_TRY(sc.get(&d_num, 2));
  TPG_TRY(sc.get(&d_runs, (size_t)nruns + 1));
  TPG_TRY(sc.get(&d_seg, (size_t)nruns + 1));
  TPG_TRY(sc.get(&d_dist, (size_t)m));
  TPG_TRY(sc.get(&d_S, (size_t)m));
  TPG_TRY(sc.get(&d_S2, (size_t)m));
  TPG_TRY(sc.get(&d_flag, 4));
  TPG_HIP(hipMemsetAsync(d_flag, 0, 4 * sizeof(int), ctx->stream));
  TPG_HIP(tpg_push_small(ctx, d_runs, run_start.data(), sizeof(int64_t) * (size_t)nruns));

  // step 0: no missing genotype, the MAC filter
  TPG_TRY(tpg_launch_loci_counts(ctx, v, d_counts));
  TPG_LAUNCH(ctx, "autosvd_mac", asv_mac_kernel, dim3(grid_for(m)), dim3(256), 0, (const int4*)d_counts, m, n, min_mac, d_excl, d_flag);
  TPG_CHECK_LAUNCH();
  int flag = 0;
  TPG_HIP(tpg_fetch_small(ctx, &flag, d_flag, sizeof(flag)));
  TPG_REQUIRE(!flag, TPG_ENUMERIC, "You can't have missing values in 'X'.");
  // step 1: clumping, or the complement of step 0
  if (hi) TPG_TRY(tpg_ld_clump(ctx, v, hi, thr_r2, nullptr, d_excl, d_keep, nullptr));
  TPG_LAUNCH(ctx, "autosvd_start", asv_start_kernel, dim3(grid_for(m)), dim3(256), 0, hi ? (const uint8_t*)nullptr : (const uint8_t*)d_excl, m, d_iota,
             d_keep);
  TPG_CHECK_LAUNCH();
  int64_t mk = 0;
  TPG_TRY(select_flagged(ctx, d_iota, d_keep, d_idx, m, d_num, &mk));
  TPG_REQUIRE(mk >= 1, TPG_ENUMERIC, "no locus is left after the minor-allele-count filter and clumping");

  // step 2: the loop
  int iter = 0;
  std::vector<int64_t> h_seg;
  for (;;) {
    iter++;
    {
      tpg_view* p = nullptr;
      TPG_TRY(select_loci_device(ctx, v, d_idx, mk, &p));
      ViewPtr sub(p);
      res->d.assign((size_t)k, 0.0);
      res->u.assign((size_t)n * k, 0.0);
      res->v.assign((size_t)mk * k, 0.0);
      res->center.assign((size_t)mk, 0.0);
      res->scale.assign((size_t)mk, 0.0);
      TPG_TRY(tpg_pca_partial_svd(ctx, sub.get(), k, res->d.data(), res->u.data(), res->v.data(), res->center.data(), res->scale.data(),
                                  &res->fro));
    }
    if (iter > max_iter) break;
    // step 3: S = sqrt of the robust distance of the loadings
    TPG_TRY(tpg_robust_dist_ogk(ctx, res->v.data(), mk, k, d_dist, nullptr, nullptr, nullptr, nullptr));
    TPG_LAUNCH(ctx, "autosvd_sqrt", asv_sqrt_kernel, dim3(grid_for(mk)), dim3(256), 0, (const double*)d_dist, mk, d_S, d_flag + 1);
    // step 4: rolling mean per chromosome segment of the kept loci
    TPG_LAUNCH(ctx, "autosvd_seg", asv_seg_kernel, dim3((unsigned)ceil_div(nruns + 1, 64)), dim3(64), 0, (const int64_t*)d_idx, mk,
               (const int64_t*)d_runs, nruns, d_seg);
    TPG_CHECK_LAUNCH();
    TPG_TRY(fetch_i64(ctx, h_seg, d_seg, (size_t)nruns + 1));
    TPG_HIP(tpg_fetch_small(ctx, &flag, d_flag + 1, sizeof(flag)));
    TPG_REQUIRE(!flag, TPG_ENUMERIC, "iteration %d: a robust distance that is not finite", iter);
    TPG_TRY(rollmean_device(ctx, d_S, mk, h_seg.data(), d_seg, nruns, roll_size, true, d_S2));
    // step 5: the fence and the outliers
    AsvIter it;
    it.n_kept = mk;
    TPG_TRY(tukey_device(ctx, d_S2, mk, alpha_tukey, true, it.report));
    TPG_LAUNCH(ctx, "autosvd_fence", asv_fence_kernel, dim3(grid_for(mk)), dim3(256), 0, (const double*)d_S2, mk, it.report[6], d_keep, d_outf);
    TPG_CHECK_LAUNCH();
    TPG_TRY(select_flagged(ctx, d_iota, d_outf, d_opos, mk, d_num, &it.n_out));
    if (it.n_out > 0) {
      int64_t again = 0;
      TPG_TRY(select_flagged(ctx, d_idx, d_outf, d_oidx, mk, d_num, &again));
      TPG_TRY(fetch_i64(ctx, it.pos, d_opos, (size_t)it.n_out));
      TPG_TRY(fetch_i64(ctx, it.idx0, d_oidx, (size_t)it.n_out));
    }
    const int64_t n_out = it.n_out;
    res->hist.push_back(std::move(it));
    if (n_out == 0) {
      res->converged = 1;
      break;
    }
    int64_t left = 0;
    TPG_TRY(select_flagged(ctx, d_idx, d_keep, d_idx2, mk, d_num, &left));
    TPG_REQUIRE(left >= 1, TPG_ENUMERIC, "iteration %d: every locus is an outlier", iter);
    std::swap(d_idx, d_idx2);
    mk = left;
  }
  res->iters = iter;
  res->count = mk;
  TPG_TRY(fetch_i64(ctx, res->idx0, d_idx, (size_t)mk));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  *out = res.release();
  return TPG_OK;
}

extern "C" int64_t tpg_autosvd_count(const void* r) { return r ? ((const tpg_autosvd*)r)->count : 0; }
extern "C" int tpg_autosvd_iters(const void* r) { return r ? ((const tpg_autosvd*)r)->iters : 0; }
extern "C" int tpg_autosvd_converged(const void* r) { return r ? ((const tpg_autosvd*)r)->converged : 0; }

extern "C" int tpg_autosvd_fetch(const void* r, double* d, double* u, double* vload, double* center, double* scale, int64_t* idx0,
                                 double* square_frobenius) {
  TPG_REQUIRE(r, TPG_EINVAL, "null argument");
  const tpg_autosvd* a = (const tpg_autosvd*)r;
  if (d) std::copy(a->d.begin(), a->d.end(), d);
  if (u) std::copy(a->u.begin(), a->u.end(), u);
  if (vload) std::copy(a->v.begin(), a->v.end(), vload);
  if (center) std::copy(a->center.begin(), a->center.end(), center);
  if (scale) std::copy(a->scale.begin(), a->scale.end(), scale);
  if (idx0) std::copy(a->idx0.begin(), a->idx0.end(), idx0);
  if (square_frobenius) *square_frobenius = a->fro;
  return TPG_OK;
}

extern "C" int tpg_autosvd_history(const void* r, int iter, int64_t* n_kept, int64_t* n_outliers, double* report) {
  TPG_REQUIRE(r, TPG_EINVAL, "null argument");
  const tpg_autosvd* a = (const tpg_autosvd*)r;
  TPG_REQUIRE(iter >= 0 && (size_t)iter < a->hist.size(), TPG_EINVAL, "iteration %d of %zu", iter, a->hist.size());
  const AsvIter& it = a->hist[(size_t)iter];
  if (n_kept) *n_kept = it.n_kept;
  if (n_outliers) *n_outliers = it.n_out;
  if (report) std::copy(it.report, it.report + 7, report);
  return TPG_OK;
}

extern "C" int tpg_autosvd_outliers(const void* r, int iter, int64_t* pos0, int64_t* idx0) {
  TPG_REQUIRE(r, TPG_EINVAL, "null argument");
  const tpg_autosvd* a = (const tpg_autosvd*)r;
  TPG_REQUIRE(iter >= 0 && (size_t)iter < a->hist.size(), TPG_EINVAL, "iteration %d of %zu", iter, a->hist.size());
  const AsvIter& it = a->hist[(size_t)iter];
  if (pos0) std::copy(it.pos.begin(), it.pos.end(), pos0);
  if (idx0) std::copy(it.idx0.begin(), it.idx0.end(), idx0);
  return TPG_OK;
}

extern "C" int tpg_autosvd_intervals(const void* r, int iter, int64_t min_size, int64_t* first0, int64_t* last0, int64_t* count) {
  TPG_REQUIRE(r && count, TPG_EINVAL, "null argument");
  const tpg_autosvd* a = (const tpg_autosvd*)r;
  TPG_REQUIRE(iter >= 0 && (size_t)iter < a->hist.size(), TPG_EINVAL, "iteration %d of %zu", iter, a->hist.size());
  TPG_REQUIRE(min_size >= 1, TPG_EINVAL, "int_min_size = %lld", (long long)min_size);
  const AsvIter& it = a->hist[(size_t)iter];
  std::vector<int32_t> ch(it.idx0.size());
  for (size_t i = 0; i < ch.size(); i++) ch[i] = a->chrom[(size_t)it.idx0[i]];
  std::vector<int64_t> first, last;
  host_outlier_runs(it.pos.data(), ch.data(), (int64_t)it.pos.size(), min_size, first, last);
  for (size_t i = 0; i < first.size(); i++) {
    if (first0) first0[i] = it.idx0[(size_t)first[i]];
    if (last0) last0[i] = it.idx0[(size_t)last[i]];
  }
  *count = (int64_t)first.size();
  return TPG_OK;
}

extern "C" void tpg_autosvd_free(void* r) { delete (tpg_autosvd*)r; }
