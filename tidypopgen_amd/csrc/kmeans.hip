// kmeans.hip -- include/tpg.h "k-means on PCA scores" and the device part of "DAPC".
//
// Batched Lloyd iterations.  Every run of a batch is independent; the scores (n x d doubles, 800 kB at 5 000 x 20) stay in L2 and
// the centres of a run pass through LDS.  One iteration is four launches over the runs that are still live:
//   km_assign   grid (point tile, live run): a thread owns one point, its d coordinates in registers; the run's centres come
//               through LDS in chunks of floor(TPG_KMEANS_CHUNK_DOUBLES / d), every lane reading the same LDS address (a
//               broadcast, no bank conflict); the distance is the direct form, 2 FP64 VALU operations per coordinate.  Labels
//               that changed and points per centre are counted with integer atomics (LDS first, one global add per block
//               and centre).
//   km_compact  one workgroup: the runs whose assign changed a label stay on the list, the others get n_iter / converged.
//   km_order    one wave per run: the points of the run sorted by centre, stably (ascending point index inside a centre), by
//               a counting sort whose ranks inside a wave come from 64 lane reads.
//   km_means    a thread per (centre, coordinate) adds its points up in that order and divides: the order of addition is a
//               function of the labels alone, so no launch shape, batch or atomic enters a centre.
// The host reads one integer per iteration, the length of the live list.
// tpg_cluster_wss (the WSS of given labellings, for the Ward route of hclust.hip) counts the labels and reuses km_order, km_means and
// the tile sums.
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "host/host_kmeans.h"
#include "host/host_lda.h"

namespace {

constexpr int KM_TILE = TPG_KMEANS_TILE;
constexpr int KM_CHUNK = TPG_KMEANS_CHUNK_DOUBLES;
static_assert(KM_TILE == 256, "the kernels below are written for workgroups of 256 points");
static_assert(KM_CHUNK >= TPG_KMEANS_MAX_D, "a chunk holds at least one centre");

// start centres: the rows idx[] of X
__global__ void km_gather_kernel(const double* __restrict__ X, int64_t n, int d, const int32_t* __restrict__ rk,
                                 const int64_t* __restrict__ roff, const int32_t* __restrict__ idx, double* __restrict__ C) {
  const int run = blockIdx.y, k = rk[run];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= k * d) return;
  const int c = t % k, j = t / k;
  C[roff[run] * d + t] = X[idx[roff[run] + c] + (int64_t)j * n];
}

// the sum of one value per thread over a workgroup of KM_TILE threads by halving (the order of the header); valid on thread 0
__device__ __forceinline__ double km_tile_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = KM_TILE / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

template <int DT, bool WSS>
__global__ __launch_bounds__(KM_TILE) void km_assign_kernel(const double* __restrict__ X, int64_t n, int d,
                                                            const int32_t* __restrict__ live, const int32_t* __restrict__ rk,
                                                            const int64_t* __restrict__ roff, const double* __restrict__ Call,
                                                            int32_t* __restrict__ labels, int32_t* __restrict__ changed,
                                                            int32_t* __restrict__ counts, double* __restrict__ tile_wss) {
  __shared__ double cs[KM_CHUNK];
  __shared__ int hist[TPG_KMEANS_MAX_K];
  __shared__ double red[WSS ? KM_TILE : 1];
  const int run = live[blockIdx.y], k = rk[run], tid = threadIdx.x;
  const double* __restrict__ C = Call + roff[run] * d;
  const int64_t i = (int64_t)blockIdx.x * KM_TILE + tid;
  const bool valid = i < n;
  double x[DT];
#pragma unroll
  for (int j = 0; j < DT; j++) x[j] = (valid && j < d) ? X[i + (int64_t)j * n] : 0.0;
  for (int c = tid; c < k; c += KM_TILE) hist[c] = 0;
  double best = INFINITY;
  int bl = 0;
  const int ch = KM_CHUNK / d;
  for (int c0 = 0; c0 < k; c0 += ch) {
    const int cn = min(ch, k - c0);
    __syncthreads();
    for (int t = tid; t < cn * d; t += KM_TILE) {
      const int cc = t % cn, j = t / cn;
      cs[cc * d + j] = C[c0 + cc + j * k];
    }
    __syncthreads();
    for (int cc = 0; cc < cn; cc++) {
      const double* __restrict__ cp = cs + cc * d;
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < DT; j++) {
        if (j < d) {
          const double t = x[j] - cp[j];
          s = fma(t, t, s);
        }
      }
      if (s < best) {
        best = s;
        bl = c0 + cc;
      }
    }
  }
  int moved = 0;
  if (valid) {
    const int64_t at = i + (int64_t)run * n;
    moved = labels[at] != bl;
    if (moved) labels[at] = bl;
    atomicAdd(&hist[bl], 1);
  }
  const int nmoved = __syncthreads_count(moved);  // (also orders the histogram before it is read)
  if (tid == 0 && nmoved) atomicAdd(&changed[run], nmoved);
  for (int c = tid; c < k; c += KM_TILE)
    if (hist[c]) atomicAdd(&counts[roff[run] + c], hist[c]);
  if (WSS) {
    const double s = km_tile_sum(valid ? best : 0.0, red);
    if (tid == 0) tile_wss[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
  }
}

// e_i under the run's centres and ITS labels, summed per tile
template <int DT>
__global__ __launch_bounds__(KM_TILE) void km_wss_kernel(const double* __restrict__ X, int64_t n, int d, const int32_t* __restrict__ rk,
                                                         const int64_t* __restrict__ roff, const double* __restrict__ Call,
                                                         const int32_t* __restrict__ labels, double* __restrict__ tile_wss) {
  __shared__ double red[KM_TILE];
  const int run = blockIdx.y, k = rk[run];
  const double* __restrict__ C = Call + roff[run] * d;
  const int64_t i = (int64_t)blockIdx.x * KM_TILE + threadIdx.x;
  double s = 0.0;
  if (i < n) {
    const int c = labels[i + (int64_t)run * n];
#pragma unroll
    for (int j = 0; j < DT; j++) {
      if (j < d) {
        const double t = X[i + (int64_t)j * n] - C[c + j * k];
        s = fma(t, t, s);
      }
    }
  }
  s = km_tile_sum(s, red);
  if (threadIdx.x == 0) tile_wss[(int64_t)run * gridDim.x + blockIdx.x] = s;
}

__global__ void km_wss_finish_kernel(const double* __restrict__ tile_wss, int tiles, int R, double* __restrict__ wss) {
  const int run = blockIdx.x * blockDim.x + threadIdx.x;
  if (run >= R) return;
  double s = 0.0;
  for (int t = 0; t < tiles; t++) s += tile_wss[(int64_t)run * tiles + t];
  wss[run] = s;
}

// The runs of live_in whose assign changed a label go to live_out in the same order (they get an update; while it < max_iter
// they are the next iteration's list); the others have converged.  One workgroup of 1024.
__global__ __launch_bounds__(1024) void km_compact_kernel(const int32_t* __restrict__ live_in, int L, int32_t* __restrict__ live_out,
                                                          int32_t* __restrict__ n_out, int32_t* __restrict__ changed,
                                                          int32_t* __restrict__ n_iter, int32_t* __restrict__ converged, int it) {
  __shared__ int sc[1024];
  const int tid = threadIdx.x, seg = (L + 1023) / 1024, lo = min(tid * seg, L), hi = min(lo + seg, L);
  int keep = 0;
  for (int q = lo; q < hi; q++) {
    const int run = live_in[q];
    n_iter[run] = it;
    if (changed[run]) keep++;
    else converged[run] = 1;
  }
  sc[tid] = keep;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = tid >= off ? sc[tid - off] : 0;
    __syncthreads();
    sc[tid] += v;
    __syncthreads();
  }
  int at = sc[tid] - keep;
  for (int q = lo; q < hi; q++) {
    const int run = live_in[q];
    if (changed[run]) {
      live_out[at++] = run;
      changed[run] = 0;
    }
  }
  if (tid == 1023) *n_out = sc[1023];
}

// One wave per run: starts[c] = the first position of centre c in the run's sorted point list (k + 1 entries), the list itself
// (ascending point index inside a centre), the number of centres that own nothing; the counts go back to zero for the next assign.
__global__ __launch_bounds__(64) void km_order_kernel(int64_t n, const int32_t* __restrict__ live, const int32_t* __restrict__ rk,
                                                      const int64_t* __restrict__ roff, const int32_t* __restrict__ labels,
                                                      int32_t* __restrict__ counts, int32_t* __restrict__ starts,
                                                      int32_t* __restrict__ order, int32_t* __restrict__ n_empty) {
  __shared__ int cursor[TPG_KMEANS_MAX_K];
  const int run = live[blockIdx.x], k = rk[run], lane = threadIdx.x;
  int32_t* __restrict__ cnt = counts + roff[run];
  int32_t* __restrict__ st = starts + roff[run] + run;
  const int seg = (k + 63) / 64, lo = min(lane * seg, k), hi = min(lo + seg, k);
  int s = 0, zero = 0;
  for (int c = lo; c < hi; c++) {
    s += cnt[c];
    zero += cnt[c] == 0;
  }
  int incl = s;
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off);
    if (lane >= off) incl += t;
  }
  for (int off = 32; off >= 1; off >>= 1) zero += __shfl_xor(zero, off);
  int at = incl - s;
  for (int c = lo; c < hi; c++) {
    cursor[c] = at;
    st[c] = at;
    at += cnt[c];
    cnt[c] = 0;
  }
  if (lane == 0) {
    st[k] = (int32_t)n;
    n_empty[run] = zero;
  }
  __syncthreads();
  const int32_t* __restrict__ lab_run = labels + (int64_t)run * n;
  int32_t* __restrict__ ord = order + (int64_t)run * n;
  for (int64_t base = 0; base < n; base += 64) {
    const int64_t i = base + lane;
    const int lab = i < n ? lab_run[i] : -1 - lane;  // (a lane past the end matches nobody)
    int rank = 0, total = 0;
    for (int q = 0; q < 64; q++) {
      const int same = __shfl(lab, q) == lab;
      rank += same & (q < lane);
      total += same;
    }
    if (i < n) ord[cursor[lab] + rank] = (int32_t)i;
    __syncthreads();
    if (i < n && rank == total - 1) cursor[lab] += total;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void km_means_kernel(const double* __restrict__ X, int64_t n, int d, const int32_t* __restrict__ live,
                                                       const int32_t* __restrict__ rk, const int64_t* __restrict__ roff,
                                                       const int32_t* __restrict__ starts, const int32_t* __restrict__ order,
                                                       double* __restrict__ Call) {
  const int run = live[blockIdx.y], k = rk[run];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= k * d) return;
  const int c = t % k, j = t / k;
  const int32_t* __restrict__ st = starts + roff[run] + run;
  const int p0 = st[c], p1 = st[c + 1];
  if (p1 == p0) return;  // owns no point: stays where it is
  const int32_t* __restrict__ ord = order + (int64_t)run * n;
  const double* __restrict__ xj = X + (int64_t)j * n;
  double s = 0.0;
  for (int p = p0; p < p1; p++) s += xj[ord[p]];
  Call[roff[run] * d + t] = s / (double)(p1 - p0);
}

__global__ void km_counts_kernel(const int32_t* __restrict__ starts, int k, int32_t* __restrict__ counts) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < k) counts[c] = starts[c + 1] - starts[c];
}

// counts of every run in the layout of the centres, from the sorted lists' starts
__global__ void km_counts_runs_kernel(const int32_t* __restrict__ starts, const int32_t* __restrict__ rk, const int64_t* __restrict__ roff,
                                      int32_t* __restrict__ counts) {
  const int run = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= rk[run]) return;
  const int32_t* __restrict__ st = starts + roff[run] + run;
  counts[roff[run] + c] = st[c + 1] - st[c];
}

// given labels (tpg_cluster_wss): points per centre by integer atomics, as the assign kernel leaves them; a label outside
// [0, k_run) raises the flag and is not counted
__global__ void km_label_count_kernel(int64_t n, const int32_t* __restrict__ rk, const int64_t* __restrict__ roff,
                                      const int32_t* __restrict__ labels, int32_t* __restrict__ counts, int* __restrict__ flag) {
  const int run = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int lab = labels[i + (int64_t)run * n];
  if (lab < 0 || lab >= rk[run]) *flag = 1;
  else atomicAdd(&counts[roff[run] + lab], 1);
}

__global__ void km_iota_kernel(int32_t* __restrict__ p, int count) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < count) p[t] = t;
}

// ---- the state of a batch on the device
struct KmBatch {
  tpg_ctx* ctx;
  const double* X;
  int64_t n;
  int d, R, kmax, tiles;
  int64_t ktot;
  DevArena sc;
  int32_t *rk, *live[2], *labels, *changed, *counts, *starts, *order, *n_iter, *converged, *n_empty, *n_live;
  int64_t* roff;
  double *C, *tile_wss, *wss;

  int init(tpg_ctx* c, const double* dX, int64_t n_, int d_, int R_, const int32_t* hk) {
    ctx = c, X = dX, n = n_, d = d_, R = R_;
    tiles = (int)ceil_div(n, KM_TILE);
    std::vector<int64_t> off((size_t)R);
    ktot = 0, kmax = 0;
    for (int r = 0; r < R; r++) {
      off[(size_t)r] = ktot;
      ktot += hk[r];
      kmax = std::max(kmax, (int)hk[r]);
    }
    TPG_TRY(sc.get(&rk, (size_t)R));
    TPG_TRY(sc.get(&roff, (size_t)R));
    TPG_TRY(sc.get(&live[0], (size_t)R));
    TPG_TRY(sc.get(&live[1], (size_t)R));
    TPG_TRY(sc.get(&labels, (size_t)n * R));
    TPG_TRY(sc.get(&order, (size_t)n * R));
    TPG_TRY(sc.get(&changed, (size_t)R));
    TPG_TRY(sc.get(&counts, (size_t)ktot));
    TPG_TRY(sc.get(&starts, (size_t)ktot + R));
    TPG_TRY(sc.get(&n_iter, (size_t)R));
    TPG_TRY(sc.get(&converged, (size_t)R));
    TPG_TRY(sc.get(&n_empty, (size_t)R));
    TPG_TRY(sc.get(&n_live, 4));
    TPG_TRY(sc.get(&C, (size_t)ktot * d));
    TPG_TRY(sc.get(&tile_wss, (size_t)R * tiles));
    TPG_TRY(sc.get(&wss, (size_t)R));
    TPG_HIP(tpg_upload(ctx, rk, hk, sizeof(int32_t) * (size_t)R));
    TPG_HIP(tpg_upload(ctx, roff, off.data(), sizeof(int64_t) * (size_t)R));
    TPG_HIP(hipMemsetAsync(labels, 0xFF, sizeof(int32_t) * (size_t)n * R, ctx->stream));  // every label -1
    TPG_HIP(hipMemsetAsync(changed, 0, sizeof(int32_t) * (size_t)R, ctx->stream));
    TPG_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)ktot, ctx->stream));
    TPG_HIP(hipMemsetAsync(n_iter, 0, sizeof(int32_t) * (size_t)R, ctx->stream));
    TPG_HIP(hipMemsetAsync(converged, 0, sizeof(int32_t) * (size_t)R, ctx->stream));
    TPG_HIP(hipMemsetAsync(n_empty, 0, sizeof(int32_t) * (size_t)R, ctx->stream));
    TPG_LAUNCH(ctx, "km_iota", km_iota_kernel, dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, live[0], R);
    TPG_CHECK_LAUNCH();
    return TPG_OK;
  }

  template <bool WSS>
  int assign(const int32_t* d_live, int L) {
    const dim3 grid((unsigned)tiles, (unsigned)L), block(KM_TILE);
#define KM_ASSIGN(DT) \
  TPG_LAUNCH(ctx, "km_assign", (km_assign_kernel<DT, WSS>), grid, block, 0, X, n, d, d_live, rk, roff, C, labels, changed, counts, tile_wss)
    if (d <= 8) KM_ASSIGN(8);
    else if (d <= 16) KM_ASSIGN(16);
    else if (d <= 32) KM_ASSIGN(32);
    else KM_ASSIGN(64);
#undef KM_ASSIGN
    TPG_CHECK_LAUNCH();
    return TPG_OK;
  }

  int update(const int32_t* d_live, int L) {
    TPG_LAUNCH(ctx, "km_order", km_order_kernel, dim3((unsigned)L), dim3(64), 0, n, d_live, rk, roff, labels, counts, starts, order, n_empty);
    TPG_CHECK_LAUNCH();
    TPG_LAUNCH(ctx, "km_means", km_means_kernel, dim3((unsigned)ceil_div((int64_t)kmax * d, 256), (unsigned)L), dim3(256), 0, X, n, d,
               d_live, rk, roff, starts, order, C);
    TPG_CHECK_LAUNCH();
    return TPG_OK;
  }

  int sum_tiles() {
    TPG_LAUNCH(ctx, "km_wss_finish", km_wss_finish_kernel, dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, tile_wss, tiles, R, wss);
    TPG_CHECK_LAUNCH();
    return TPG_OK;
  }

  int final_wss() {
    const dim3 grid((unsigned)tiles, (unsigned)R), block(KM_TILE);
#define KM_WSS(DT) TPG_LAUNCH(ctx, "km_wss", km_wss_kernel<DT>, grid, block, 0, X, n, d, rk, roff, C, labels, tile_wss)
    if (d <= 8) KM_WSS(8);
    else if (d <= 16) KM_WSS(16);
    else if (d <= 32) KM_WSS(32);
    else KM_WSS(64);
#undef KM_WSS
    TPG_CHECK_LAUNCH();
    return sum_tiles();
  }
};

int km_check_shape(int64_t n, int d) {
  TPG_REQUIRE(n >= 1 && n <= TPG_KMEANS_MAX_N, TPG_EINVAL, "n = %lld outside [1, %d]", (long long)n, TPG_KMEANS_MAX_N);
  TPG_REQUIRE(d >= 1 && d <= TPG_KMEANS_MAX_D, TPG_EINVAL, "d = %d outside [1, %d]", d, TPG_KMEANS_MAX_D);
  return TPG_OK;
}

int km_check_k(int k, int64_t n) {
  TPG_REQUIRE(k >= 1 && k <= TPG_KMEANS_MAX_K && k <= n, TPG_EINVAL, "k = %d outside [1, min(n = %lld, %d)]", k, (long long)n,
              TPG_KMEANS_MAX_K);
  return TPG_OK;
}

}  // namespace

extern "C" int64_t tpg_kmeans_chunk_doubles(void) { return KM_CHUNK; }

extern "C" int tpg_kmeans_start(uint64_t seed, int64_t n, int k, int32_t* idx) {
  TPG_REQUIRE(idx, TPG_EINVAL, "null argument");
  TPG_REQUIRE(n >= 1 && n <= TPG_KMEANS_MAX_N, TPG_EINVAL, "n = %lld outside [1, %d]", (long long)n, TPG_KMEANS_MAX_N);
  TPG_REQUIRE(k >= 1 && k <= n, TPG_EINVAL, "k = %d outside [1, n = %lld]", k, (long long)n);
  std::vector<std::pair<uint64_t, int32_t>> keys;
  host_kmeans_start(seed, n, k, idx, keys);
  return TPG_OK;
}

extern "C" int tpg_kmeans_step(tpg_ctx* ctx, const double* X, int64_t n, int d, int k, const double* C_in, int32_t* labels,
                               double* C_out, int32_t* counts, double* wss) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && X && C_in && labels, TPG_EINVAL, "null argument");
  TPG_TRY(km_check_shape(n, d));
  TPG_TRY(km_check_k(k, n));
  InBuf ix, ic;
  TPG_TRY(ix.init(ctx, X, sizeof(double) * (size_t)n * d));
  TPG_TRY(ic.init(ctx, C_in, sizeof(double) * (size_t)k * d));
  KmBatch b;
  const int32_t hk = k;
  TPG_TRY(b.init(ctx, ix.dev<double>(), n, d, 1, &hk));
  TPG_TRY(tpg_check_finite(ctx, b.X, n * d, b.sc, "X"));
  TPG_TRY(tpg_check_finite(ctx, ic.dev<double>(), (int64_t)k * d, b.sc, "C_in"));
  TPG_HIP(tpg_copy_dev(ctx, b.C, ic.dev<double>(), sizeof(double) * (size_t)k * d));
  TPG_TRY(b.assign<true>(b.live[0], 1));
  TPG_TRY(b.sum_tiles());
  TPG_TRY(b.update(b.live[0], 1));
  int32_t* d_cnt;
  TPG_TRY(b.sc.get(&d_cnt, (size_t)k));
  TPG_LAUNCH(ctx, "km_counts", km_counts_kernel, dim3((unsigned)ceil_div(k, 256)), dim3(256), 0, b.starts, k, d_cnt);
  TPG_CHECK_LAUNCH();
  TPG_TRY(tpg_deliver(ctx, labels, b.labels, (size_t)n));
  TPG_TRY(tpg_deliver(ctx, C_out, b.C, (size_t)k * d));
  TPG_TRY(tpg_deliver(ctx, counts, d_cnt, (size_t)k));
  TPG_TRY(tpg_deliver(ctx, wss, b.wss, 1));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return TPG_OK;
}

extern "C" int tpg_kmeans_batch(tpg_ctx* ctx, const double* X, int64_t n, int d, int R, const int32_t* k, const int64_t* seed,
                                int max_iter, const double* centers0, int32_t* labels, double* centers, double* wss, int32_t* n_iter,
                                int32_t* converged, int32_t* n_empty) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && X && k && labels && (seed || centers0), TPG_EINVAL, "null argument");
  TPG_TRY(km_check_shape(n, d));
  TPG_REQUIRE(R >= 1 && R <= TPG_KMEANS_MAX_RUNS, TPG_EINVAL, "R = %d outside [1, %d]", R, TPG_KMEANS_MAX_RUNS);
  TPG_REQUIRE(max_iter >= 1, TPG_EINVAL, "max_iter = %d", max_iter);
  HostIn<int32_t> hk;
  TPG_TRY(hk.init(ctx, k, R));
  for (int r = 0; r < R; r++) TPG_TRY(km_check_k(hk[r], n));
  InBuf ix;
  TPG_TRY(ix.init(ctx, X, sizeof(double) * (size_t)n * d));
  KmBatch b;
  TPG_TRY(b.init(ctx, ix.dev<double>(), n, d, R, hk.p));
  TPG_TRY(tpg_check_finite(ctx, b.X, n * d, b.sc, "X"));
  if (centers0) {
    InBuf ic;
    TPG_TRY(ic.init(ctx, centers0, sizeof(double) * (size_t)b.ktot * d));
    TPG_TRY(tpg_check_finite(ctx, ic.dev<double>(), b.ktot * d, b.sc, "centers0"));
    TPG_HIP(tpg_copy_dev(ctx, b.C, ic.dev<double>(), sizeof(double) * (size_t)b.ktot * d));
    TPG_HIP(hipStreamSynchronize(ctx->stream));  // (ic may own the copy it is read from)
  } else {
    HostIn<int64_t> hs;
    TPG_TRY(hs.init(ctx, seed, R));
    std::vector<int32_t> idx((size_t)b.ktot);
    std::vector<std::pair<uint64_t, int32_t>> keys;
    int64_t at = 0;
    for (int r = 0; r < R; r++) {
      host_kmeans_start((uint64_t)hs[r], n, hk[r], idx.data() + at, keys);
      at += hk[r];
    }
    int32_t* d_idx;
    TPG_TRY(b.sc.get(&d_idx, (size_t)b.ktot));
    TPG_HIP(tpg_upload(ctx, d_idx, idx.data(), sizeof(int32_t) * (size_t)b.ktot));
    TPG_LAUNCH(ctx, "km_gather", km_gather_kernel, dim3((unsigned)ceil_div((int64_t)b.kmax * d, 256), (unsigned)R), dim3(256), 0, b.X, n,
               d, b.rk, b.roff, d_idx, b.C);
    TPG_CHECK_LAUNCH();
  }
  int L = R, cur = 0;
  for (int it = 1; it <= max_iter && L > 0; it++) {
    TPG_TRY(b.assign<false>(b.live[cur], L));
    TPG_LAUNCH(ctx, "km_compact", km_compact_kernel, dim3(1), dim3(1024), 0, b.live[cur], L, b.live[cur ^ 1], b.n_live, b.changed,
               b.n_iter, b.converged, it);
    TPG_CHECK_LAUNCH();
    int32_t nl = 0;
    TPG_HIP(tpg_fetch_small(ctx, &nl, b.n_live, sizeof(int32_t)));
    cur ^= 1, L = nl;
    if (L > 0) TPG_TRY(b.update(b.live[cur], L));
  }
  TPG_TRY(b.final_wss());
  TPG_TRY(tpg_deliver(ctx, labels, b.labels, (size_t)n * R));
  TPG_TRY(tpg_deliver(ctx, centers, b.C, (size_t)b.ktot * d));
  TPG_TRY(tpg_deliver(ctx, wss, b.wss, (size_t)R));
  TPG_TRY(tpg_deliver(ctx, n_iter, b.n_iter, (size_t)R));
  TPG_TRY(tpg_deliver(ctx, converged, b.converged, (size_t)R));
  TPG_TRY(tpg_deliver(ctx, n_empty, b.n_empty, (size_t)R));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return TPG_OK;
}

// The WSS of R given labellings: the means of the labels by km_order / km_means and the tile sums of km_wss, the kernels a run
// of tpg_kmeans_batch ends in, so a labelling that such a run returned gets that run's bits back.
extern "C" int tpg_cluster_wss(tpg_ctx* ctx, const double* X, int64_t n, int d, int R, const int32_t* k, const int32_t* labels,
                               double* wss, int32_t* counts) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && X && k && labels && wss, TPG_EINVAL, "null argument");
  TPG_TRY(km_check_shape(n, d));
  TPG_REQUIRE(R >= 1 && R <= TPG_KMEANS_MAX_RUNS, TPG_EINVAL, "R = %d outside [1, %d]", R, TPG_KMEANS_MAX_RUNS);
  HostIn<int32_t> hk;
  TPG_TRY(hk.init(ctx, k, R));
  for (int r = 0; r < R; r++) TPG_TRY(km_check_k(hk[r], n));
  InBuf ix, il;
  TPG_TRY(ix.init(ctx, X, sizeof(double) * (size_t)n * d));
  TPG_TRY(il.init(ctx, labels, sizeof(int32_t) * (size_t)n * R));
  KmBatch b;
  TPG_TRY(b.init(ctx, ix.dev<double>(), n, d, R, hk.p));
  TPG_TRY(tpg_check_finite(ctx, b.X, n * d, b.sc, "X"));
  TPG_HIP(tpg_copy_dev(ctx, b.labels, il.dev<int32_t>(), sizeof(int32_t) * (size_t)n * R));
  TPG_HIP(hipMemsetAsync(b.C, 0, sizeof(double) * (size_t)b.ktot * d, ctx->stream));  // (a centre that owns nothing stays: at +0)
  int* d_flag;
  TPG_TRY(b.sc.get(&d_flag, 4));
  TPG_HIP(hipMemsetAsync(d_flag, 0, sizeof(int), ctx->stream));
  TPG_LAUNCH(ctx, "km_label_count", km_label_count_kernel, dim3((unsigned)b.tiles, (unsigned)R), dim3(KM_TILE), 0, n, b.rk, b.roff,
             b.labels, b.counts, d_flag);
  TPG_CHECK_LAUNCH();
  int flag = 0;
  TPG_HIP(tpg_fetch_small(ctx, &flag, d_flag, sizeof(int)));  // (il may own the copy the labels were read from: it has been read)
  TPG_REQUIRE(!flag, TPG_EINVAL, "a label outside [0, k) of its labelling");
  TPG_TRY(b.update(b.live[0], R));
  TPG_TRY(b.final_wss());
  int32_t* d_cnt = nullptr;
  if (counts) {
    TPG_TRY(b.sc.get(&d_cnt, (size_t)b.ktot));
    TPG_LAUNCH(ctx, "km_counts_runs", km_counts_runs_kernel, dim3((unsigned)ceil_div(b.kmax, 256), (unsigned)R), dim3(256), 0, b.starts,
               b.rk, b.roff, d_cnt);
    TPG_CHECK_LAUNCH();
  }
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  TPG_TRY(tpg_deliver(ctx, wss, b.wss, (size_t)R));
  TPG_TRY(tpg_deliver(ctx, counts, d_cnt, (size_t)b.ktot));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return TPG_OK;
}

// ---- DAPC

extern "C" int tpg_lda(const double* X, int64_t n, int d, const int32_t* grp0, int G, int n_da, double* prior, double* means,
                       double* mu_out, double* scaling, double* svd, int32_t* n_lda, int32_t* n_da_out, double* ind_coord,
                       double* grp_coord, double* posterior, int32_t* assign) {
  TPG_REQUIRE(X && grp0 && prior && means && scaling && svd && n_lda && n_da_out && ind_coord && grp_coord && posterior && assign,
              TPG_EINVAL, "null argument");
  const char* why = "";
  const int rc = host_lda(X, n, d, grp0, G, n_da, prior, means, mu_out, scaling, svd, n_lda, n_da_out, ind_coord, grp_coord, posterior,
                          assign, &why);
  TPG_REQUIRE(rc == HOST_LDA_OK, rc == HOST_LDA_EINVAL ? TPG_EINVAL : TPG_ENUMERIC, "lda: %s", why);
  return TPG_OK;
}

namespace {

// var_load of a tile of rows and the tile's sums of squares per column
__global__ __launch_bounds__(KM_TILE) void dapc_load_kernel(const double* __restrict__ V, int64_t m, int64_t ldv, int n_pca,
                                                            const double* __restrict__ load, int n_da, double* __restrict__ var_load,
                                                            double* __restrict__ tile_ss) {
  __shared__ double red[KM_TILE];
  const int64_t i = (int64_t)blockIdx.x * KM_TILE + threadIdx.x;
  for (int a = 0; a < n_da; a++) {
    double s = 0.0;
    if (i < m) {
      for (int j = 0; j < n_pca; j++) s = fma(V[i + (int64_t)j * ldv], load[j + a * n_pca], s);
      var_load[i + (int64_t)a * m] = s;
    }
    const double ss = km_tile_sum(i < m ? s * s : 0.0, red);
    if (threadIdx.x == 0) tile_ss[(int64_t)a * gridDim.x + blockIdx.x] = ss;
    __syncthreads();
  }
}

__global__ void dapc_colsum_kernel(const double* __restrict__ tile_ss, int tiles, int n_da, double* __restrict__ colss) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n_da) return;
  double s = 0.0;
  for (int t = 0; t < tiles; t++) s += tile_ss[(int64_t)a * tiles + t];
  colss[a] = s;
}

__global__ void dapc_contr_kernel(const double* __restrict__ var_load, int64_t m, int n_da, const double* __restrict__ colss,
                                  double* __restrict__ var_contr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  for (int a = 0; a < n_da; a++) {
    const double c = colss[a], v = var_load[i + (int64_t)a * m];
    var_contr[i + (int64_t)a * m] = c < 1e-12 ? 0.0 : (v * v) / c;
  }
}

}  // namespace

extern "C" int tpg_dapc_var_contr(tpg_ctx* ctx, const double* V, int64_t m, int64_t ldv, int n_pca, const double* loadings, int n_da,
                                  double* var_load, double* var_contr) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && V && loadings && var_load && var_contr, TPG_EINVAL, "null argument");
  TPG_REQUIRE(m >= 1 && ldv >= m && m <= (int64_t)KM_TILE * 2147483647ll / 4, TPG_EINVAL, "V of %lld rows with leading dimension %lld",
              (long long)m, (long long)ldv);
  TPG_REQUIRE(n_pca >= 1 && n_pca <= 64 && n_da >= 1 && n_da <= 64, TPG_EINVAL, "n_pca = %d, n_da = %d outside [1, 64]", n_pca, n_da);
  InBuf iv, il;
  TPG_TRY(iv.init(ctx, V, sizeof(double) * ((size_t)ldv * (size_t)(n_pca - 1) + (size_t)m)));
  TPG_TRY(il.init(ctx, loadings, sizeof(double) * (size_t)n_pca * n_da));
  OutBuf ol, oc;
  TPG_TRY(ol.init(var_load, sizeof(double) * (size_t)m * n_da));
  TPG_TRY(oc.init(var_contr, sizeof(double) * (size_t)m * n_da));
  const int tiles = (int)ceil_div(m, KM_TILE);
  DevArena sc;
  double *tile_ss, *colss;
  TPG_TRY(sc.get(&tile_ss, (size_t)tiles * n_da));
  TPG_TRY(sc.get(&colss, (size_t)n_da));
  TPG_LAUNCH(ctx, "dapc_load", dapc_load_kernel, dim3((unsigned)tiles), dim3(KM_TILE), 0, iv.dev<double>(), m, ldv, n_pca,
             il.dev<double>(), n_da, ol.dev<double>(), tile_ss);
  TPG_CHECK_LAUNCH();
  TPG_LAUNCH(ctx, "dapc_colsum", dapc_colsum_kernel, dim3(1), dim3(64), 0, tile_ss, tiles, n_da, colss);
  TPG_CHECK_LAUNCH();
  TPG_LAUNCH(ctx, "dapc_contr", dapc_contr_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, ol.dev<double>(), m, n_da, colss,
             oc.dev<double>());
  TPG_CHECK_LAUNCH();
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  TPG_TRY(ol.commit(ctx));
  TPG_TRY(oc.commit(ctx));
  return TPG_OK;
}
