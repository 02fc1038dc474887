// pcadapt.hip -- PCA-based genome scan (include/tpg.h "pcadapt"): per-locus z-scores of the regression on the PCA scores, a
// robust Mahalanobis distance of those z-scores by OGK (Maronna-Zamar, median / MAD), genomic control and log10 p-values.
//
// Replaces the arithmetic behind R/gt_pcadapt.R:44-86 (bigsnpr::snp_pcadapt -- third-party, not among the reference's sources:
// the definition is the one include/tpg.h gives).
//
// The regression sums are the FP64 row-scaled sweep of pca.hip (tpg_sweep_loci_rowscale); what is new here is the batched exact
// selection, pcadapt_select_kernel: one workgroup per VIRTUAL column -- a stored column, its absolute deviations from a centre,
// the sum or difference of two stored columns, or the absolute deviations of those -- formed on the fly, never materialised.
// It is a radix select on the order-preserving 64-bit key of a double (all bits flipped for negatives, the sign bit for the
// rest), 12 bits per level.  Level 0 counts the finite entries into a 4096-bin LDS histogram (sign and exponent), which also
// gives the count c and with it the two ranks (c - 1) / 2 and c / 2 -- two states (prefix, rank) that share a histogram while
// their prefixes agree and get one each from the level at which they part.  As soon as the bucket of a state holds at most
// TPG_SELECT_TILE keys, one more pass over the column collects them into scratch (one pass fills both lists when the two states
// qualify at the same level) and the remaining levels run on that list; until then a level reads the column again with the
// prefix as a filter.  Two states that part can become small at different levels: then each costs a collecting pass of its own.  Reads of the operands: 2 when the level-0 bucket of
// the rank is small (the tests' shapes, spread-out exponents), 3 when it takes a second level to get there (a million z-scores:
// a quarter of them share the exponent of the median absolute deviation), up to 6 for a column of mostly equal values.
// NaN and infinite entries never enter a count or a rank.  Integer LDS atomics only; the result does not depend on their order.
#include "common.h"
#include "devfrag.h"
#include "host/host_pcadapt.h"

#include <math.h>

#include <algorithm>

namespace {

constexpr int SEL_THREADS = 1024;
constexpr int SEL_CAP = TPG_SELECT_TILE;
constexpr int SEL_BINS = 4096;
static_assert(SEL_BINS == 4 * SEL_THREADS, "the pick step gives every thread four bins");

enum { SEL_X = 0, SEL_ABSDEV = 1, SEL_SUM = 2, SEL_DIFF = 3, SEL_SUM_ABSDEV = 4, SEL_DIFF_ABSDEV = 5 };
struct SelDesc {
  int32_t a, b;   // stored columns
  int32_t kind;   // SEL_*
  int32_t cidx;   // the centre of an ABSDEV kind: cvals[cidx]
};


// the value of virtual column `d` at `row` as its sort key; false: not finite.  -0 is read as +0 (x + 0.0), so that equal
// values have equal keys
__device__ __forceinline__ bool sel_key(const double* __restrict__ X, int64_t ld, const SelDesc d, double c, int64_t row, uint64_t& key) {
  double x = X[row + (int64_t)d.a * ld];
  if (d.kind >= SEL_SUM) {
    const double y = X[row + (int64_t)d.b * ld];
    x = (d.kind == SEL_SUM || d.kind == SEL_SUM_ABSDEV) ? x + y : x - y;
  }
  if (d.kind == SEL_ABSDEV || d.kind >= SEL_SUM_ABSDEV) x = fabs(x - c);
  x = x + 0.0;
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  if ((u & TPG_D_EXP_MASK) == TPG_D_EXP_MASK) return false;
  key = TPG_DKEY(u);
  return true;
}

// which bins hold the elements of (0-based) ranks rank0 (in h0) and rank1 (in h1, which may be h0): res[s] = {bin, rank inside
// the bin, count of the bin}.  All threads call it; res is valid after it returns
__device__ __forceinline__ void sel_pick2(const uint32_t* h0, const uint32_t* h1, uint32_t rank0, uint32_t rank1,
                                          uint32_t* __restrict__ wtot, uint32_t (*res)[4]) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int s = 0; s < 2; s++) {
    const uint32_t* h = s ? h1 : h0;
    const uint32_t rank = s ? rank1 : rank0;
    const uint32_t c0 = h[4 * t], c1 = h[4 * t + 1], c2 = h[4 * t + 2], c3 = h[4 * t + 3];
    const uint32_t sum = c0 + c1 + c2 + c3;
    uint32_t inc = sum;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(inc, o);
      if (lane >= o) inc += y;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; w++) base += wtot[w];
    const uint32_t excl = base + inc - sum;
    if (rank >= excl && rank < excl + sum) {  // one thread at most
      uint32_t r = rank - excl, bin = 4 * t, cnt = c0;
      if (r >= c0) {
        r -= c0; bin++; cnt = c1;
        if (r >= c1) {
          r -= c1; bin++; cnt = c2;
          if (r >= c2) { r -= c2; bin++; cnt = c3; }
        }
      }
      res[s][0] = bin; res[s][1] = r; res[s][2] = cnt;
    }
    __syncthreads();
  }
}

// out[col] = median of the finite entries of virtual column desc[col] over `rows` rows (NaN if there is none), cnt[col] = how
// many there are.  cand: 2 * SEL_CAP keys per column.  Needs rows < 2^31 (32-bit counts).
__global__ __launch_bounds__(SEL_THREADS) void pcadapt_select_kernel(const double* __restrict__ X, int64_t rows, int64_t ld,
                                                                     const SelDesc* __restrict__ desc, const double* __restrict__ cvals,
                                                                     uint64_t* __restrict__ cand, double* __restrict__ out,
                                                                     int64_t* __restrict__ cnt_out) {
  __shared__ uint32_t hist[2][SEL_BINS];
  __shared__ uint32_t wtot[SEL_THREADS / 64];
  __shared__ uint32_t res[2][4];
  __shared__ uint32_t listn[2];
  __shared__ uint32_t s_count;
  const int t = threadIdx.x;
  const uint32_t nrow = (uint32_t)rows;  // rows < 2^31: row + SEL_THREADS does not wrap
  const int64_t col = blockIdx.x;
  const SelDesc d = desc[col];
  const double c = (d.kind == SEL_ABSDEV || d.kind >= SEL_SUM_ABSDEV) ? cvals[d.cidx] : 0.0;
  uint64_t* const lists = cand + col * 2 * SEL_CAP;

  // two states (prefix, rank), one per middle rank; state 1 follows state 0 while the count is odd.  All of it is uniform
  uint32_t count = 0;
  int ns = 1;
  uint64_t prefix[2] = {0, 0};
  uint32_t rank[2] = {0, 0}, bcount[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
  bool on_list[2] = {false, false}, same = true;
  int lst[2] = {0, 1};
  if (t < 2) listn[t] = 0;
  if (t == 0) s_count = 0;

  for (int L = 0; L < 6; L++) {
    // prefix[] holds the top `done` bits of the key of each rank; this level decides the next nb
    const int done = 12 * L, nb = L < 5 ? 12 : 4, shift = 64 - done - nb;
    const uint32_t mask = (1u << nb) - 1u;
    // the bucket of a state is small: its keys go to scratch, this level and the remaining ones read them from there.  One pass
    // over the column serves both states; while they share a prefix they share list 0
    const bool col0 = !on_list[0] && bcount[0] <= (uint32_t)SEL_CAP;
    const bool col1 = ns == 2 && !same && !on_list[1] && bcount[1] <= (uint32_t)SEL_CAP;
    if (col0 || col1) {  // (bcount is known: L > 0, done > 0)
      for (uint32_t row = t; row < nrow; row += SEL_THREADS) {
        uint64_t key;
        if (!sel_key(X, ld, d, c, row, key)) continue;
        const uint64_t hi = key >> (64 - done);
        if (col0 && hi == prefix[0]) {
          const uint32_t pos = atomicAdd(&listn[0], 1u);
          if (pos < (uint32_t)SEL_CAP) lists[pos] = key;
        }
        if (col1 && hi == prefix[1]) {
          const uint32_t pos = atomicAdd(&listn[1], 1u);
          if (pos < (uint32_t)SEL_CAP) lists[SEL_CAP + pos] = key;
        }
      }
      if (col0) { on_list[0] = true; lst[0] = 0; }
      if (col1) { on_list[1] = true; lst[1] = 1; }
    }
    if (ns == 2 && same && on_list[0] && !on_list[1]) { on_list[1] = true; lst[1] = lst[0]; }
    const int nh = same ? 1 : 2;  // histograms this level
    for (int i = t; i < nh * SEL_BINS; i += SEL_THREADS) (&hist[0][0])[i] = 0;
    __syncthreads();
    if (!on_list[0] || (nh == 2 && !on_list[1])) {  // some state still reads the column: one pass serves both
      uint32_t mine = 0;
      for (uint32_t row = t; row < nrow; row += SEL_THREADS) {
        uint64_t key;
        if (!sel_key(X, ld, d, c, row, key)) continue;
        mine++;
        const uint64_t hi = done ? key >> (64 - done) : 0;
        const uint32_t dig = (uint32_t)(key >> shift) & mask;
        if (!on_list[0] && hi == prefix[0]) atomicAdd(&hist[0][dig], 1u);
        if (nh == 2 && !on_list[1] && hi == prefix[1]) atomicAdd(&hist[1][dig], 1u);
      }
      if (L == 0) {  // the number of finite entries
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
        if ((t & 63) == 0 && mine) atomicAdd(&s_count, mine);
      }
    }
#pragma unroll
    for (int s = 0; s < 2; s++) {
      if (s >= nh || !on_list[s]) continue;
      const uint32_t ln = listn[lst[s]];
      for (uint32_t i = t; i < ln; i += SEL_THREADS) {
        const uint64_t key = lists[(int64_t)lst[s] * SEL_CAP + i];
        if ((key >> (64 - done)) == prefix[s]) atomicAdd(&hist[s][(uint32_t)(key >> shift) & mask], 1u);
      }
    }
    __syncthreads();
    if (L == 0) {
      count = s_count;
      if (count == 0) {
        if (t == 0) {
          out[col] = TPG_QNAN;
          if (cnt_out) cnt_out[col] = 0;
        }
        return;
      }
      ns = (count & 1u) ? 1 : 2;  // an even count needs the two middle ranks
      rank[0] = (count - 1) / 2;
      rank[1] = count / 2;
    }
    sel_pick2(hist[0], hist[nh - 1], rank[0], rank[1], wtot, res);
    prefix[0] = (prefix[0] << nb) | res[0][0]; rank[0] = res[0][1]; bcount[0] = res[0][2];
    prefix[1] = (prefix[1] << nb) | res[1][0]; rank[1] = res[1][1]; bcount[1] = res[1][2];
    same = same && prefix[0] == prefix[1];
    __syncthreads();  // res is read by all before it is written again
  }
  if (t == 0) {
    const double lo = tpg_dunkey(prefix[0]), hi = tpg_dunkey(prefix[1]);
    out[col] = ns == 1 ? lo : (lo + hi) / 2;
    if (cnt_out) cnt_out[col] = (int64_t)count;
  }
}

// ---- z-scores ----------------------------------------------------------------------------------------------------------
// mean_j = S1 / n, a column of ones for the sweep's inv_scale; flag: a missing genotype met
__global__ void pcadapt_mean_kernel(const int4* __restrict__ counts, int64_t m, int64_t n, double* __restrict__ mean,
                                    double* __restrict__ ones, int* __restrict__ flag) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const int4 c = counts[j];
    if (c.w != 0) flag[0] = 1;
    mean[j] = (double)(c.y + 2 * c.z) / (double)n;
    ones[j] = 1.0;
  }
}

// beta (m x K, in place) -> z; *n_valid counts the valid loci
__global__ void pcadapt_finalize_kernel(const int4* __restrict__ counts, int64_t m, int64_t n, int K, double* __restrict__ z,
                                        unsigned long long* __restrict__ n_valid) {
  unsigned long long mine = 0;
  const double dof = (double)(n - K - 1);
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const int4 c = counts[j];
    const int64_t S1 = (int64_t)c.y + 2 * (int64_t)c.z, S2 = (int64_t)c.y + 4 * (int64_t)c.z;
    const double tot = (double)(n * S2 - S1 * S1) / (double)n;
    double rss = tot;
    for (int k = 0; k < K; k++) {
      const double b = z[j + (int64_t)k * m];
      rss = rss - b * b;
    }
    const bool ok = tot != 0.0 && rss > 0.0;
    const double den = sqrt(rss / dof);
    for (int k = 0; k < K; k++) z[j + (int64_t)k * m] = ok ? z[j + (int64_t)k * m] / den : TPG_QNAN;
    mine += ok ? 1ull : 0ull;
  }
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_valid, mine);
}

// ---- OGK ---------------------------------------------------------------------------------------------------------------
// X (m x K, ld = m) = Z where every entry of the row is finite, NaN otherwise
__global__ void pcadapt_mask_kernel(const double* __restrict__ Z, int64_t m, int64_t ldz, int K, double* __restrict__ X,
                                    unsigned long long* __restrict__ n_valid) {
  unsigned long long mine = 0;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    bool ok = true;
    for (int k = 0; k < K; k++) ok = ok && fabs(Z[j + (int64_t)k * ldz]) <= 1.79769313486231570815e308;
    for (int k = 0; k < K; k++) X[j + (int64_t)k * m] = ok ? Z[j + (int64_t)k * ldz] : TPG_QNAN;
    mine += ok ? 1ull : 0ull;
  }
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_valid, mine);
}

// Y = X / s, s_k = 1.4826 * mad_k (in place)
__global__ void pcadapt_scale_kernel(double* __restrict__ X, int64_t m, int K, const double* __restrict__ mad) {
  const int64_t total = m * K;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const double s = TPG_PCADAPT_MAD_SCALE * mad[idx / m];
    X[idx] = X[idx] / s;
  }
}

// W = Y E: one thread per row, E (K x K column-major) in LDS; W_jk = sum_a Y_ja * E_ak, a ascending
__global__ __launch_bounds__(256) void pcadapt_rotate_kernel(const double* __restrict__ Y, int64_t m, int K, const double* __restrict__ E,
                                                             double* __restrict__ W) {
  extern __shared__ double e_lds[];
  for (int i = threadIdx.x; i < K * K; i += blockDim.x) e_lds[i] = E[i];
  __syncthreads();
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    for (int k = 0; k < K; k++) {
      double acc = 0.0;
      for (int a = 0; a < K; a++) acc += Y[j + (int64_t)a * m] * e_lds[a + k * K];
      W[j + (int64_t)k * m] = acc;
    }
  }
}

// dist_j = sum_k (W_jk - nu_k)^2 / Gamma_k, Gamma_k = (1.4826 mad_k)^2; a NaN row stays NaN
__global__ void pcadapt_dist_kernel(const double* __restrict__ W, int64_t m, int K, const double* __restrict__ med,
                                    const double* __restrict__ mad, double* __restrict__ dist) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    double acc = 0.0;
    for (int k = 0; k < K; k++) {
      const double s = TPG_PCADAPT_MAD_SCALE * mad[k], g = s * s, dlt = W[j + (int64_t)k * m] - med[k];
      acc += (dlt * dlt) / g;
    }
    dist[j] = acc;
  }
}

// ---- chi-square tail ---------------------------------------------------------------------------------------------------
// out = log Q(a, x / 2) / ln 10; with stat: x = in / lambda, which goes to stat as well
__global__ void pcadapt_log10p_kernel(const double* __restrict__ in, int64_t count, double a, double lga, double lambda,
                                      double* __restrict__ stat, double* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    double x = in[i];
    if (stat) {
      x = x / lambda;
      stat[i] = x;
    }
    out[i] = tpg_logq(a, lga, x / 2) / 2.302585092994045684;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
inline unsigned grid_for(int64_t count) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(count, 256), 4096)); }

// the scratch of a run of selection batches: descriptors and candidate lists for up to `max_cols` virtual columns
struct Selector {
  tpg_ctx* ctx = nullptr;
  SelDesc* d_desc = nullptr;
  uint64_t* d_cand = nullptr;
  size_t max_cols = 0;
  int init(tpg_ctx* c, DevArena* sc, size_t cols) {
    ctx = c; max_cols = cols;
    TPG_TRY(sc->get(&d_desc, cols));
    TPG_TRY(sc->get(&d_cand, cols * 2 * (size_t)SEL_CAP));
    return TPG_OK;
  }
  // d_out[i] = median of virtual column descs[i]; d_cnt (may be NULL) its finite count
  int run(const double* X, int64_t rows, int64_t ld, const std::vector<SelDesc>& descs, const double* d_cvals, double* d_out,
          int64_t* d_cnt) {
    if (descs.empty()) return TPG_OK;
    TPG_REQUIRE(descs.size() <= max_cols, TPG_EINVAL, "selection batch of %zu columns, scratch for %zu", descs.size(), max_cols);
    TPG_REQUIRE(rows >= 0 && rows < 2147483647ll, TPG_EUNSUPPORTED, "selection over %lld rows", (long long)rows);
    const size_t bytes = sizeof(SelDesc) * descs.size();
    if (bytes <= tpg_ctx::H2D_SLOT_BYTES) TPG_HIP(tpg_h2d_async(ctx, d_desc, descs.data(), bytes));
    else TPG_HIP(tpg_upload(ctx, d_desc, descs.data(), bytes));
    TPG_LAUNCH(ctx, "pcadapt_select", pcadapt_select_kernel, dim3((unsigned)descs.size()), dim3(SEL_THREADS), 0, X, rows, ld,
               (const SelDesc*)d_desc, d_cvals, d_cand, d_out, d_cnt);
    TPG_CHECK_LAUNCH();
    return TPG_OK;
  }
};

int fetch_doubles(tpg_ctx* ctx, std::vector<double>& host, const double* d_src, size_t count) {
  host.resize(count);
  if (!count) return TPG_OK;
  if (sizeof(double) * count <= tpg_ctx::MAIL_FETCH_BYTES) TPG_HIP(tpg_fetch_small(ctx, host.data(), d_src, sizeof(double) * count));
  else TPG_HIP(tpg_download(ctx, host.data(), d_src, sizeof(double) * count));
  return TPG_OK;
}

bool good_scale(double mad) {
  const double s = TPG_PCADAPT_MAD_SCALE * mad;
  return s > 0.0 && s <= 1.79769313486231570815e308;
}

int check_K(int K) {
  TPG_REQUIRE(K >= 1 && K <= TPG_PCADAPT_MAX_K, TPG_EINVAL, "K = %d out of [1, %d]", K, TPG_PCADAPT_MAX_K);
  return TPG_OK;
}

// z (device, m x K) and the number of valid loci from a view and U (h_U: host copy for the argument check, d_U: device)
int zscores_device(tpg_ctx* ctx, const tpg_view* v, const double* h_U, const double* d_U, int K, double* d_z, int64_t* n_valid) {
  const int64_t n = v->n, m = v->m;
  TPG_TRY(check_K(K));
  TPG_REQUIRE(n - K - 1 >= 1, TPG_EINVAL, "n - K - 1 = %lld: the regression on K = %d scores needs more individuals", (long long)(n - K - 1), K);
  TPG_REQUIRE(m >= 1, TPG_EINVAL, "the view has no locus");
  double worst = 0;
  for (int a = 0; a < K; a++)
    for (int b = a; b < K; b++) {
      double s = 0;
      for (int64_t i = 0; i < n; i++) s += h_U[i + (int64_t)a * n] * h_U[i + (int64_t)b * n];
      const double e = fabs(s - (a == b ? 1.0 : 0.0));
      if (!(e <= worst)) worst = e;  // a NaN sticks
    }
  TPG_REQUIRE(worst <= 1e-8, TPG_EINVAL, "U is not orthonormal: max |U'U - I| = %g", worst);
  DevArena sc;
  int32_t* d_counts;
  double *d_mean, *d_ones;
  int* d_flag;
  unsigned long long* d_nv;
  TPG_TRY(sc.get(&d_counts, 4 * (size_t)m));
  TPG_TRY(sc.get(&d_mean, (size_t)m));
  TPG_TRY(sc.get(&d_ones, (size_t)m));
  TPG_TRY(sc.get(&d_flag, 2));
  TPG_TRY(sc.get(&d_nv, 1));
  TPG_TRY(tpg_launch_loci_counts(ctx, v, d_counts));
  TPG_HIP(hipMemsetAsync(d_flag, 0, 2 * sizeof(int), ctx->stream));
  TPG_HIP(hipMemsetAsync(d_nv, 0, sizeof(unsigned long long), ctx->stream));
  TPG_LAUNCH(ctx, "pcadapt_mean", pcadapt_mean_kernel, dim3(grid_for(m)), dim3(256), 0, (const int4*)d_counts, m, n, d_mean, d_ones, d_flag);
  int flag[2] = {0, 0};
  TPG_HIP(tpg_fetch_small(ctx, flag, d_flag, sizeof(flag)));
  TPG_REQUIRE(!flag[0], TPG_ENUMERIC, "You can't have missing values in 'X'.");
  TPG_TRY(tpg_sweep_loci_rowscale(ctx, v, d_mean, d_ones, d_U, K, d_z));
  TPG_LAUNCH(ctx, "pcadapt_finalize", pcadapt_finalize_kernel, dim3(grid_for(m)), dim3(256), 0, (const int4*)d_counts, m, n, K, d_z, d_nv);
  TPG_CHECK_LAUNCH();
  unsigned long long nv = 0;
  TPG_HIP(tpg_fetch_small(ctx, &nv, d_nv, sizeof(nv)));
  *n_valid = (int64_t)nv;
  return TPG_OK;
}

// medians and MADs of the K stored columns of X: d_med, d_mad (device, K each)
int col_med_mad(Selector& sel, const double* X, int64_t rows, int64_t ld, int ncols, double* d_med, double* d_mad, int64_t* d_cnt) {
  std::vector<SelDesc> a((size_t)ncols), b((size_t)ncols);
  for (int k = 0; k < ncols; k++) {
    a[(size_t)k] = SelDesc{k, k, SEL_X, 0};
    b[(size_t)k] = SelDesc{k, k, SEL_ABSDEV, k};
  }
  TPG_TRY(sel.run(X, rows, ld, a, nullptr, d_med, d_cnt));
  return sel.run(X, rows, ld, b, d_med, d_mad, nullptr);
}

// dist (device, m) of Z (device, m x K, leading dimension ldz); center[K], cov[K x K], basis[2 K K] (host, may each be NULL)
int ogk_device(tpg_ctx* ctx, const double* d_Z, int64_t m, int64_t ldz, int K, double* d_dist, double* center, double* cov, double* basis,
               int64_t* n_valid) {
  TPG_TRY(check_K(K));
  TPG_REQUIRE(m >= 1 && ldz >= m, TPG_EINVAL, "Z of %lld rows with leading dimension %lld", (long long)m, (long long)ldz);
  const int P = K * (K - 1) / 2;
  DevArena sc;
  Selector sel;
  TPG_TRY(sel.init(ctx, &sc, (size_t)std::max(K, 2 * P)));
  double *X, *W, *d_med, *d_mad, *d_pmed, *d_pmad, *d_E;
  unsigned long long* d_nv;
  TPG_TRY(sc.get(&X, (size_t)m * K));
  TPG_TRY(sc.get(&W, (size_t)m * K));
  TPG_TRY(sc.get(&d_med, (size_t)K));
  TPG_TRY(sc.get(&d_mad, (size_t)K));
  TPG_TRY(sc.get(&d_pmed, (size_t)std::max(1, 2 * P)));
  TPG_TRY(sc.get(&d_pmad, (size_t)std::max(1, 2 * P)));
  TPG_TRY(sc.get(&d_E, (size_t)K * K));
  TPG_TRY(sc.get(&d_nv, 1));
  TPG_HIP(hipMemsetAsync(d_nv, 0, sizeof(unsigned long long), ctx->stream));
  TPG_LAUNCH(ctx, "pcadapt_mask", pcadapt_mask_kernel, dim3(grid_for(m)), dim3(256), 0, d_Z, m, ldz, K, X, d_nv);
  unsigned long long nv = 0;
  TPG_HIP(tpg_fetch_small(ctx, &nv, d_nv, sizeof(nv)));
  if (n_valid) *n_valid = (int64_t)nv;
  TPG_REQUIRE((int64_t)nv >= K + 2, TPG_ENUMERIC, "%lld valid rows of z-scores: the robust distance of K = %d columns needs K + 2", (long long)nv, K);

  std::vector<SelDesc> pair_val((size_t)(2 * P)), pair_dev((size_t)(2 * P));
  {
    int p = 0;
    for (int a = 0; a < K; a++)
      for (int b = a + 1; b < K; b++, p++) {
        pair_val[(size_t)p] = SelDesc{a, b, SEL_SUM, 0};
        pair_val[(size_t)(P + p)] = SelDesc{a, b, SEL_DIFF, 0};
        pair_dev[(size_t)p] = SelDesc{a, b, SEL_SUM_ABSDEV, p};
        pair_dev[(size_t)(P + p)] = SelDesc{a, b, SEL_DIFF_ABSDEV, P + p};
      }
  }
  std::vector<double> h_mad, h_pmad, s_it[2], E_it[2], R;
  for (int it = 0; it < 2; it++) {
    TPG_TRY(col_med_mad(sel, X, m, m, K, d_med, d_mad, nullptr));
    TPG_TRY(fetch_doubles(ctx, h_mad, d_mad, (size_t)K));
    s_it[it].resize((size_t)K);
    for (int k = 0; k < K; k++) {
      TPG_REQUIRE(good_scale(h_mad[(size_t)k]), TPG_ENUMERIC, "OGK iteration %d: the MAD of column %d is %g", it + 1, k, h_mad[(size_t)k]);
      s_it[it][(size_t)k] = TPG_PCADAPT_MAD_SCALE * h_mad[(size_t)k];
    }
    TPG_LAUNCH(ctx, "pcadapt_scale", pcadapt_scale_kernel, dim3(grid_for(m * K)), dim3(256), 0, X, m, K, (const double*)d_mad);
    if (K == 1) {
      E_it[it].assign(1, 1.0);
    } else {
      TPG_TRY(sel.run(X, m, m, pair_val, nullptr, d_pmed, nullptr));
      TPG_TRY(sel.run(X, m, m, pair_dev, d_pmed, d_pmad, nullptr));
      TPG_TRY(fetch_doubles(ctx, h_pmad, d_pmad, (size_t)(2 * P)));
      TPG_REQUIRE(host_ogk_corr(K, h_pmad.data(), h_pmad.data() + P, R, E_it[it]), TPG_ENUMERIC,
                  "OGK iteration %d: a pairwise scale is zero or not finite", it + 1);
    }
    TPG_HIP(tpg_push_small(ctx, d_E, E_it[it].data(), sizeof(double) * (size_t)K * K));
    TPG_LAUNCH(ctx, "pcadapt_rotate", pcadapt_rotate_kernel, dim3(grid_for(m)), dim3(256), sizeof(double) * (size_t)K * K, (const double*)X, m, K,
               (const double*)d_E, W);
    std::swap(X, W);
  }
  TPG_TRY(col_med_mad(sel, X, m, m, K, d_med, d_mad, nullptr));
  std::vector<double> nu;
  TPG_TRY(fetch_doubles(ctx, nu, d_med, (size_t)K));
  TPG_TRY(fetch_doubles(ctx, h_mad, d_mad, (size_t)K));
  std::vector<double> gamma((size_t)K);
  for (int k = 0; k < K; k++) {
    TPG_REQUIRE(good_scale(h_mad[(size_t)k]), TPG_ENUMERIC, "OGK: the MAD of the final column %d is %g", k, h_mad[(size_t)k]);
    const double s = TPG_PCADAPT_MAD_SCALE * h_mad[(size_t)k];
    gamma[(size_t)k] = s * s;
  }
  TPG_LAUNCH(ctx, "pcadapt_dist", pcadapt_dist_kernel, dim3(grid_for(m)), dim3(256), 0, (const double*)X, m, K, (const double*)d_med,
             (const double*)d_mad, d_dist);
  TPG_CHECK_LAUNCH();
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  if (center || cov) {
    std::vector<double> c((size_t)K), cv((size_t)K * K);
    host_ogk_backmap(K, s_it[0].data(), E_it[0].data(), s_it[1].data(), E_it[1].data(), nu.data(), gamma.data(), c.data(), cv.data());
    if (center) std::copy(c.begin(), c.end(), center);
    if (cov) std::copy(cv.begin(), cv.end(), cov);
  }
  if (basis)
    for (int it = 0; it < 2; it++) std::copy(E_it[it].begin(), E_it[it].end(), basis + (size_t)it * K * K);
  return TPG_OK;
}

int log10p_launch(tpg_ctx* ctx, const double* d_in, int64_t count, int df, double lambda, double* d_stat, double* d_out) {
  const double a = 0.5 * df;
  TPG_LAUNCH(ctx, "pcadapt_log10p", pcadapt_log10p_kernel, dim3(grid_for(count)), dim3(256), 0, d_in, count, a, lgamma(a), lambda, d_stat, d_out);
  TPG_CHECK_LAUNCH();
  return TPG_OK;
}

}  // namespace

extern "C" int64_t tpg_select_tile(void) { return SEL_CAP; }

extern "C" int tpg_col_median_mad(tpg_ctx* ctx, const double* X, int64_t rows, int ncols, int64_t ld, double* med, double* mad,
                                  int64_t* n_finite) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && X && med && mad, TPG_EINVAL, "null argument");
  TPG_REQUIRE(rows >= 1 && ncols >= 1 && ld >= rows, TPG_EINVAL, "X of %lld x %d with leading dimension %lld", (long long)rows, ncols,
              (long long)ld);
  InBuf ix;
  TPG_TRY(ix.init(ctx, X, sizeof(double) * ((size_t)ld * (size_t)(ncols - 1) + (size_t)rows)));
  OutBuf om, oa;
  TPG_TRY(om.init(med, sizeof(double) * (size_t)ncols));
  TPG_TRY(oa.init(mad, sizeof(double) * (size_t)ncols));
  DevArena sc;
  int64_t* d_cnt;
  TPG_TRY(sc.get(&d_cnt, (size_t)ncols));
  Selector sel;
  TPG_TRY(sel.init(ctx, &sc, (size_t)ncols));
  TPG_TRY(col_med_mad(sel, ix.dev<double>(), rows, ld, ncols, om.dev<double>(), oa.dev<double>(), d_cnt));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  TPG_TRY(om.commit(ctx));
  TPG_TRY(oa.commit(ctx));
  if (n_finite) {
    OutBuf on;
    TPG_TRY(on.init(n_finite, sizeof(int64_t) * (size_t)ncols));
    TPG_HIP(tpg_copy_dev(ctx, on.dev<int64_t>(), d_cnt, sizeof(int64_t) * (size_t)ncols));
    TPG_TRY(on.commit(ctx));
  }
  return TPG_OK;
}

extern "C" int tpg_pcadapt_zscores(tpg_ctx* ctx, const tpg_view* v, const double* U, int K, double* z, int64_t* n_valid) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && U && z, TPG_EINVAL, "null argument");
  TPG_TRY(check_K(K));
  HostIn<double> hu;
  InBuf iu;
  TPG_TRY(hu.init(ctx, U, v->n * K));
  TPG_TRY(iu.init(ctx, U, sizeof(double) * (size_t)v->n * (size_t)K));
  DevBuf d_z;  // the caller's z is written at the very end only
  TPG_TRY(d_z.alloc_n<double>((size_t)v->m * (size_t)K));
  int64_t nv = 0;
  TPG_TRY(zscores_device(ctx, v, hu.p, iu.dev<double>(), K, d_z.as<double>(), &nv));
  OutBuf oz;
  TPG_TRY(oz.init(z, sizeof(double) * (size_t)v->m * (size_t)K));
  TPG_HIP(tpg_copy_dev(ctx, oz.dev<double>(), d_z.p, sizeof(double) * (size_t)v->m * (size_t)K));
  TPG_TRY(oz.commit(ctx));
  if (n_valid) *n_valid = nv;
  return TPG_OK;
}

extern "C" int tpg_robust_dist_ogk(tpg_ctx* ctx, const double* Z, int64_t m, int K, double* dist, double* center, double* cov,
                                   double* basis, int64_t* n_valid) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && Z && dist, TPG_EINVAL, "null argument");
  TPG_TRY(check_K(K));
  TPG_REQUIRE(m >= 1, TPG_EINVAL, "Z has no rows");
  InBuf iz;
  TPG_TRY(iz.init(ctx, Z, sizeof(double) * (size_t)m * (size_t)K));
  DevBuf d_dist;
  TPG_TRY(d_dist.alloc_n<double>((size_t)m));
  TPG_TRY(ogk_device(ctx, iz.dev<double>(), m, m, K, d_dist.as<double>(), center, cov, basis, n_valid));
  OutBuf od;
  TPG_TRY(od.init(dist, sizeof(double) * (size_t)m));
  TPG_HIP(tpg_copy_dev(ctx, od.dev<double>(), d_dist.p, sizeof(double) * (size_t)m));
  return od.commit(ctx);
}

extern "C" int tpg_pchisq_log10_upper(tpg_ctx* ctx, const double* x, int64_t count, int df, double* out) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && x && out, TPG_EINVAL, "null argument");
  TPG_REQUIRE(count >= 0 && df >= 1, TPG_EINVAL, "count = %lld, df = %d", (long long)count, df);
  if (count == 0) return TPG_OK;
  InBuf ix;
  TPG_TRY(ix.init(ctx, x, sizeof(double) * (size_t)count));
  OutBuf oo;
  TPG_TRY(oo.init(out, sizeof(double) * (size_t)count));
  TPG_TRY(log10p_launch(ctx, ix.dev<double>(), count, df, 1.0, nullptr, oo.dev<double>()));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return oo.commit(ctx);
}

extern "C" int tpg_qchisq_median(int df, double* out) {
  TPG_REQUIRE(out, TPG_EINVAL, "null argument");
  TPG_REQUIRE(df >= 1 && df <= 1000000, TPG_EINVAL, "df = %d", df);
  *out = host_qchisq_median(df);
  return TPG_OK;
}

extern "C" int tpg_pcadapt(tpg_ctx* ctx, const tpg_view* v, const double* U, int K, double* z, double* dist, double* stat,
                           double* log10p, double* gc_lambda, int64_t* n_valid) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && U && dist && stat && log10p, TPG_EINVAL, "null argument");
  TPG_TRY(check_K(K));
  const int64_t m = v->m;
  HostIn<double> hu;
  InBuf iu;
  TPG_TRY(hu.init(ctx, U, v->n * K));
  TPG_TRY(iu.init(ctx, U, sizeof(double) * (size_t)v->n * (size_t)K));
  DevArena sc;
  double *d_z, *d_dist, *d_stat, *d_lp, *d_med;
  TPG_TRY(sc.get(&d_z, (size_t)m * K));
  TPG_TRY(sc.get(&d_dist, (size_t)m));
  TPG_TRY(sc.get(&d_stat, (size_t)m));
  TPG_TRY(sc.get(&d_lp, (size_t)m));
  TPG_TRY(sc.get(&d_med, 1));
  int64_t nv = 0, nv2 = 0;
  TPG_TRY(zscores_device(ctx, v, hu.p, iu.dev<double>(), K, d_z, &nv));
  TPG_TRY(ogk_device(ctx, d_z, m, m, K, d_dist, nullptr, nullptr, nullptr, &nv2));
  // genomic control: lambda = median(dist) / median of chi-square(K)
  Selector sel;
  TPG_TRY(sel.init(ctx, &sc, 1));
  TPG_TRY(sel.run(d_dist, m, m, std::vector<SelDesc>{SelDesc{0, 0, SEL_X, 0}}, nullptr, d_med, nullptr));
  double med = 0;
  TPG_HIP(tpg_fetch_small(ctx, &med, d_med, sizeof(med)));
  const double lambda = med / host_qchisq_median(K);
  TPG_REQUIRE(lambda > 0.0 && lambda <= 1.79769313486231570815e308, TPG_ENUMERIC, "genomic control factor %g", lambda);
  TPG_TRY(log10p_launch(ctx, d_dist, m, K, lambda, d_stat, d_lp));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  // nothing of the caller's has been written so far
  struct { double* user; const double* dev; size_t count; } outs[4] = {
      {z, d_z, (size_t)m * K}, {dist, d_dist, (size_t)m}, {stat, d_stat, (size_t)m}, {log10p, d_lp, (size_t)m}};
  for (auto& o : outs) {
    if (!o.user) continue;
    OutBuf ob;
    TPG_TRY(ob.init(o.user, sizeof(double) * o.count));
    TPG_HIP(tpg_copy_dev(ctx, ob.dev<double>(), o.dev, sizeof(double) * o.count));
    TPG_TRY(ob.commit(ctx));
  }
  if (gc_lambda) *gc_lambda = lambda;
  if (n_valid) *n_valid = nv;
  return TPG_OK;
}
