// hclust.hip -- include/tpg.h "Ward clustering on PCA scores".
//
// The device holds the full symmetric S (n x n doubles, both halves, so that a row is one contiguous read), the size and a live
// flag of every slot, and the nearest-neighbour list: for a live i with a live j > i, nn[i] is the first minimum of S(i, j) over
// the live j > i and dnn[i] its value; nn[i] = -1 where no live j > i is left.  One merge is three launches on the stream:
//   hc_pick    one workgroup: the lexicographic minimum of (dnn[i], i) over the live rows is the pair (a, b = nn[a]).  It writes
//              the merge record, hands (a, b, S(a,b), n_a, n_b) to the next kernel, adds the sizes, clears b's live flag and
//              empties the recompute list.
//   hc_update  a thread per slot c: the Lance-Williams recurrence into S(a,c) (coalesced in row a) and S(c,a) (column a), then
//              the repair of the list: row a, and every row whose neighbour was a or b, goes onto the recompute list (an integer
//              atomic appends; the order of the list does not matter); a row c < a whose new S(c,a) is below dnn[c], or equal
//              with a < nn[c], takes a as its neighbour.
//   hc_rownn   a workgroup per listed row scans it for the first minimum over the live j > i; a fixed grid strides over the
//              list, whose length it reads from device memory.
// No kernel waits on memory another workgroup writes: the launch boundary is the barrier.  The host queues the 3 (n - 1) launches
// back to back and reads the result arrays once at the end.  hc_pick, hc_rownn and the order they pick in are in hclust_dev.h,
// which tree.hip uses too.
#include "hclust_dev.h"
#include "host/host_hclust.h"

namespace {

// S(i, j) for a tile of i and one j; the diagonal is +inf.  t = x_i - x_j and x_j - x_i differ in sign alone, so both halves
// hold the same bits.
__global__ __launch_bounds__(HC_BLOCK) void hc_init_kernel(const double* __restrict__ X, int n, int d, int power,
                                                          double* __restrict__ S) {
  const int i = blockIdx.x * HC_BLOCK + threadIdx.x, j = blockIdx.y;
  if (i >= n) return;
  double s = 0.0;
  for (int c = 0; c < d; c++) {
    const double t = X[i + (int64_t)c * n] - X[j + (int64_t)c * n];
    s = fma(t, t, s);
  }
  if (power == 2) s = s * s;
  S[(int64_t)j * n + i] = i == j ? INFINITY : s;
}

__global__ __launch_bounds__(HC_BLOCK) void hc_update_kernel(double* __restrict__ S, int n, const int32_t* __restrict__ size,
                                                            const int32_t* __restrict__ live, const HcStep* __restrict__ cur,
                                                            int32_t* __restrict__ nn, double* __restrict__ dnn,
                                                            int32_t* __restrict__ list, int32_t* __restrict__ list_len) {
  const int c = blockIdx.x * HC_BLOCK + threadIdx.x;
  const int a = cur->a, b = cur->b;
  if (c >= n || a < 0 || !live[c]) return;  // (b is dead already)
  if (c == a) {
    list[atomicAdd(list_len, 1)] = a;
    return;
  }
  const double na = (double)cur->na, nb = (double)cur->nb, nc = (double)size[c], sab = cur->sab;
  const double s = hc_ward_lw(na, nb, nc, S[(int64_t)a * n + c], S[(int64_t)b * n + c], sab);
  S[(int64_t)a * n + c] = s;
  S[(int64_t)c * n + a] = s;
  const int nc_nn = nn[c];
  if (nc_nn == a || nc_nn == b) list[atomicAdd(list_len, 1)] = c;
  else if (c < a && (s < dnn[c] || (s == dnn[c] && a < nc_nn))) nn[c] = a, dnn[c] = s;
}

}  // namespace

extern "C" int tpg_hclust_ward_trace(tpg_ctx* ctx, const double* X, int64_t n, int d, int power, int32_t* merge_a, int32_t* merge_b,
                                     double* height, int32_t* list_len) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && X && merge_a && merge_b && height, TPG_EINVAL, "null argument");
  TPG_REQUIRE(n >= 1 && n <= TPG_HCLUST_MAX_N, TPG_EINVAL, "n = %lld outside [1, %d]", (long long)n, TPG_HCLUST_MAX_N);
  TPG_REQUIRE(d >= 1 && d <= TPG_KMEANS_MAX_D, TPG_EINVAL, "d = %d outside [1, %d]", d, TPG_KMEANS_MAX_D);
  TPG_REQUIRE(power == 1 || power == 2, TPG_EINVAL, "power = %d, not 1 or 2", power);
  InBuf ix;
  TPG_TRY(ix.init(ctx, X, sizeof(double) * (size_t)n * d));
  const double* dX = ix.dev<double>();
  DevArena sc;
  TPG_TRY(tpg_check_finite(ctx, dX, n * d, sc, "X"));
  if (n == 1) return TPG_OK;  // no merge: the outputs are empty
  const int ni = (int)n, steps = ni - 1;
  double *S, *dnn, *d_height;
  int32_t *size, *live, *nn, *list, *d_len, *d_failed, *hist, *d_ma, *d_mb;
  HcStep* cur;
  TPG_TRY(sc.get(&S, (size_t)n * (size_t)n));
  TPG_TRY(sc.get(&dnn, (size_t)n));
  TPG_TRY(sc.get(&d_height, (size_t)steps));
  TPG_TRY(sc.get(&size, (size_t)n));
  TPG_TRY(sc.get(&live, (size_t)n));
  TPG_TRY(sc.get(&nn, (size_t)n));
  TPG_TRY(sc.get(&list, (size_t)n));
  TPG_TRY(sc.get(&d_len, 4));
  TPG_TRY(sc.get(&d_failed, 4));
  TPG_TRY(sc.get(&hist, (size_t)n));
  TPG_TRY(sc.get(&d_ma, (size_t)steps));
  TPG_TRY(sc.get(&d_mb, (size_t)steps));
  TPG_TRY(sc.get(&cur, 1));
  const unsigned tiles = (unsigned)ceil_div(n, HC_BLOCK), nn_grid = (unsigned)std::min<int64_t>(n, HC_ROWNN_GRID);
  TPG_LAUNCH(ctx, "hc_init", hc_init_kernel, dim3(tiles, (unsigned)n), dim3(HC_BLOCK), 0, dX, ni, d, power, S);
  TPG_CHECK_LAUNCH();
  TPG_LAUNCH(ctx, "hc_start", hc_start_kernel, dim3(tiles), dim3(HC_BLOCK), 0, ni, size, live, list, d_len, d_failed);
  TPG_CHECK_LAUNCH();
  TPG_LAUNCH(ctx, "hc_rownn", hc_rownn_kernel, dim3(nn_grid), dim3(HC_BLOCK), 0, S, ni, live, list, d_len, nn, dnn);
  TPG_CHECK_LAUNCH();
  for (int s = 0; s < steps; s++) {
    TPG_LAUNCH(ctx, "hc_pick", hc_pick_kernel, dim3(1), dim3(HC_PICK), 0, ni, s, size, live, nn, dnn, d_len, hist, d_failed, cur, d_ma, d_mb,
               d_height);
    TPG_LAUNCH(ctx, "hc_update", hc_update_kernel, dim3(tiles), dim3(HC_BLOCK), 0, S, ni, size, live, cur, nn, dnn, list, d_len);
    TPG_LAUNCH(ctx, "hc_rownn", hc_rownn_kernel, dim3(nn_grid), dim3(HC_BLOCK), 0, S, ni, live, list, d_len, nn, dnn);
    if ((s & 255) == 255) TPG_CHECK_LAUNCH();
  }
  TPG_CHECK_LAUNCH();
  int32_t failed = 0;
  TPG_HIP(tpg_fetch_small(ctx, &failed, d_failed, sizeof(int32_t)));  // (waits for every step: a fault surfaces here, before an output is touched)
  TPG_REQUIRE(!failed, TPG_ENUMERIC, "a merge step found no live pair");
  TPG_TRY(tpg_deliver(ctx, merge_a, d_ma, (size_t)steps));
  TPG_TRY(tpg_deliver(ctx, merge_b, d_mb, (size_t)steps));
  TPG_TRY(tpg_deliver(ctx, height, d_height, (size_t)steps));
  TPG_TRY(tpg_deliver(ctx, list_len, hist, (size_t)steps));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return TPG_OK;
}

extern "C" int tpg_hclust_ward(tpg_ctx* ctx, const double* X, int64_t n, int d, int power, int32_t* merge_a, int32_t* merge_b,
                               double* height) {
  return tpg_hclust_ward_trace(ctx, X, n, d, power, merge_a, merge_b, height, nullptr);
}

extern "C" int tpg_hclust_cut(int64_t n, const int32_t* merge_a, const int32_t* merge_b, int R, const int32_t* k, int32_t* labels) {
  TPG_REQUIRE(k && labels && (n == 1 || (merge_a && merge_b)), TPG_EINVAL, "null argument");
  const char* why = "";
  TPG_REQUIRE(host_hclust_cut(n, merge_a, merge_b, R, k, labels, &why) == HOST_HCLUST_OK, TPG_EINVAL, "hclust_cut: %s", why);
  return TPG_OK;
}

extern "C" int tpg_hclust_r_merge(int64_t n, const int32_t* merge_a, const int32_t* merge_b, int32_t* merge) {
  TPG_REQUIRE(n == 1 || (merge_a && merge_b && merge), TPG_EINVAL, "null argument");
  const char* why = "";
  TPG_REQUIRE(host_hclust_r_merge(n, merge_a, merge_b, merge, &why) == HOST_HCLUST_OK, TPG_EINVAL, "hclust_r_merge: %s", why);
  return TPG_OK;
}
