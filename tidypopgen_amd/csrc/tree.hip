// tree.hip -- include/tpg.h "Trees from a pairwise matrix": tpg_hclust_dist (single, complete, average, McQuitty and Ward linkage
// on a matrix as given) and tpg_nj (neighbour-joining).
//
// Both calls work on a scratch copy S of the strict lower triangle of D, full and symmetric with +inf on the diagonal, so that a
// row is one contiguous read.  D itself is only read, by tr_build, which also raises a flag for an entry of the triangle that is
// not finite; the host reads the flag before anything else is queued.
//
// Linkages.  The step is hclust.hip's (hclust_dev.h): hc_pick takes the pair from the nearest-later-neighbour list, tr_update
// applies the recurrence -- a template parameter, so a compile-time branch -- and repairs the list, hc_rownn scans the listed
// rows again.  The list caches row minima of S and its repair rule asks nothing of the recurrence: rows whose neighbour was a or
// b, and row a, are scanned again; a row c < a takes a where the new S(c,a) is before its cached minimum.  The row stride of S
// is n here.
//
// Neighbour-joining.  Every q(a,b) = ((r - 2) S(a,b) - R_a) - R_b changes at every join, so no list survives: the step is a full
// scan, three launches with the launch boundary as the only barrier:
//   nj_rowmin  a workgroup per live row i, a fixed grid striding the rows (a dead row costs one load of its flag): the first
//              minimum of (q, j) over the live j > i.  The row stride of S is even (n rounded up), so that row i is read as
//              16-byte pairs (j, j + 1), j even, with R and the live flags of the pair as one load each.
//   nj_pick    one workgroup: the minimum of (q, a) over the rows, the join record, both branch lengths, the new R_a; b dies.
//   nj_update  a thread per live c: t = ((S(a,c) + S(b,c)) - d) / 2 into row a and column a, and R_c.
// The scan reads the live rows' part above the diagonal, dead columns included: at most 4 n^2 bytes a join.
#include "hclust_dev.h"
#include "host/host_hclust.h"
#include "host/host_tree.h"

namespace {

constexpr int NJ_GRID = 2048;

// S(i, j) = S(j, i) = D[max + min n] for a tile of i and one j (ld: the row stride of S); the diagonal is +inf.  Only the thread
// below the diagonal looks at whether the value is finite: the upper triangle and the diagonal of D are never read.
__global__ __launch_bounds__(HC_BLOCK) void tr_build_kernel(const double* __restrict__ D, int n, int64_t ld, double* __restrict__ S,
                                                           int32_t* __restrict__ bad) {
  const int i = blockIdx.x * HC_BLOCK + threadIdx.x, j = blockIdx.y;
  if (i >= n) return;
  double v = INFINITY;
  if (i > j) {
    v = D[i + (int64_t)j * n];
    if (!isfinite(v)) *bad = 1;
  } else if (i < j) v = D[j + (int64_t)i * n];
  S[(int64_t)j * ld + i] = v;
}

enum { LINK_SINGLE = 0, LINK_COMPLETE = 1, LINK_AVERAGE = 2, LINK_MCQUITTY = 3, LINK_WARD = 4 };

template <int LINK>
__global__ __launch_bounds__(HC_BLOCK) void tr_update_kernel(double* __restrict__ S, int n, const int32_t* __restrict__ size,
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
  const double x = S[(int64_t)a * n + c], y = S[(int64_t)b * n + c];
  double s;
  if (LINK == LINK_SINGLE) s = y < x ? y : x;
  else if (LINK == LINK_COMPLETE) s = y > x ? y : x;
  else if (LINK == LINK_AVERAGE) {
    const double na = (double)cur->na, nb = (double)cur->nb;
    const double p = na * x;
    const double q = nb * y;
    s = (p + q) / (na + nb);
  } else if (LINK == LINK_MCQUITTY) s = (x + y) * 0.5;
  else s = hc_ward_lw((double)cur->na, (double)cur->nb, (double)size[c], x, y, cur->sab);
  S[(int64_t)a * n + c] = s;
  S[(int64_t)c * n + a] = s;
  const int nc_nn = nn[c];
  if (nc_nn == a || nc_nn == b) list[atomicAdd(list_len, 1)] = c;
  else if (c < a && (s < dnn[c] || (s == dnn[c] && a < nc_nn))) nn[c] = a, dnn[c] = s;
}

// ---- neighbour-joining

struct NjStep {
  int32_t a, b;
  double d;
};

// live flags, and R_i = sum of S(i, j) over j != i, ascending j from +0, one addition per j: a thread per i walks down column i
// (= row i, S is symmetric), so a wave reads consecutive addresses.  Entries n and n + 1 of live and R pad the pair loads.
__global__ __launch_bounds__(HC_BLOCK) void nj_start_kernel(const double* __restrict__ S, int n, int64_t ld, int32_t* __restrict__ live,
                                                           double* __restrict__ R, int32_t* __restrict__ failed) {
  const int i = blockIdx.x * HC_BLOCK + threadIdx.x;
  if (i == 0) *failed = 0;
  if (i >= n + 2) return;
  if (i >= n) {
    live[i] = 0, R[i] = 0.0;
    return;
  }
  double r = 0.0;
  for (int j = 0; j < n; j++)
    if (j != i) r = r + S[(int64_t)j * ld + i];
  live[i] = 1, R[i] = r;
}

// a candidate whose q is NaN names nobody
__device__ __forceinline__ void nj_take(double q, int j, double& v, int& bj) {
  if (q != q) return;
  if (bj < 0 || q < v) v = q, bj = j;
}

__global__ __launch_bounds__(HC_BLOCK) void nj_rowmin_kernel(const double* __restrict__ S, int n, int64_t ld, int r,
                                                            const int32_t* __restrict__ live, const double* __restrict__ R,
                                                            double* __restrict__ rowq, int32_t* __restrict__ rowj) {
  __shared__ double sv[HC_BLOCK / 64];
  __shared__ int sj[HC_BLOCK / 64];
  const double rm2 = (double)(r - 2);
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    if (!live[i]) continue;  // (uniform over the workgroup)
    const double Ri = R[i];
    const double2* __restrict__ row = reinterpret_cast<const double2*>(S + (int64_t)i * ld);
    const double2* __restrict__ R2 = reinterpret_cast<const double2*>(R);
    const int2* __restrict__ live2 = reinterpret_cast<const int2*>(live);
    double v = INFINITY;
    int bj = -1;
    // pairs (j, j + 1) with j even, from the pair that holds i + 1; a thread's j ascend, so replacing on strictly smaller keeps
    // its first minimum.  j + 1 <= n + 1 <= ld + 1: inside the padded row of S only where j + 1 < ld, which j < n, n <= ld, ld
    // even and j even give; live and R hold n + 2 entries
    for (int j = ((i + 1) & ~1) + 2 * (int)threadIdx.x; j < n; j += 2 * HC_BLOCK) {
      const int2 lv = live2[j >> 1];
      if (!(lv.x | lv.y)) continue;
      const double2 s = row[j >> 1];
      const double2 rj = R2[j >> 1];
      if (lv.x && j > i) nj_take((rm2 * s.x - Ri) - rj.x, j, v, bj);
      if (lv.y && j + 1 < n) nj_take((rm2 * s.y - Ri) - rj.y, j + 1, v, bj);
    }
    hc_block_min<HC_BLOCK>(v, bj, sv, sj);
    if (threadIdx.x == 0) rowj[i] = bj, rowq[i] = v;
  }
}

__global__ __launch_bounds__(HC_PICK) void nj_pick_kernel(const double* __restrict__ S, int n, int64_t ld, int r, int step,
                                                         int32_t* __restrict__ live, double* __restrict__ R,
                                                         const double* __restrict__ rowq, const int32_t* __restrict__ rowj,
                                                         int32_t* __restrict__ failed, NjStep* __restrict__ cur, int32_t* __restrict__ join_a,
                                                         int32_t* __restrict__ join_b, double* __restrict__ len_a, double* __restrict__ len_b) {
  __shared__ double sv[HC_PICK / 64];
  __shared__ int sj[HC_PICK / 64];
  double v = INFINITY;
  int bi = -1;
  for (int i = threadIdx.x; i < n; i += HC_PICK) {
    if (!live[i] || rowj[i] < 0) continue;
    const double q = rowq[i];
    if (bi < 0 || q < v) v = q, bi = i;
  }
  hc_block_min<HC_PICK>(v, bi, sv, sj);
  if (threadIdx.x != 0) return;
  // every q NaN (an overflow): nothing is indexed with -1, nj_update does nothing for a < 0, and the host turns the flag into an
  // error before any output is written
  NjStep st = {-1, -1, 0.0};
  double la = 0.0, lb = 0.0;
  if (bi < 0) *failed = 1;
  else {
    st.a = bi, st.b = rowj[bi], st.d = S[(int64_t)st.a * ld + st.b];
    const double Ra = R[st.a], Rb = R[st.b], d = st.d;
    la = 0.5 * d + (Ra - Rb) / (2.0 * (double)(r - 2));
    lb = d - la;
    R[st.a] = ((Ra + Rb) - (double)r * d) * 0.5;
    live[st.b] = 0;
  }
  *cur = st;
  join_a[step] = st.a, join_b[step] = st.b, len_a[step] = la, len_b[step] = lb;
}

__global__ __launch_bounds__(HC_BLOCK) void nj_update_kernel(double* __restrict__ S, int n, int64_t ld, const int32_t* __restrict__ live,
                                                            double* __restrict__ R, const NjStep* __restrict__ cur) {
  const int c = blockIdx.x * HC_BLOCK + threadIdx.x;
  const int a = cur->a, b = cur->b;
  if (c >= n || a < 0 || c == a || !live[c]) return;  // (b is dead already)
  const double x = S[(int64_t)a * ld + c], y = S[(int64_t)b * ld + c], d = cur->d;
  const double t = ((x + y) - d) * 0.5;
  R[c] = ((R[c] - x) - y) + t;
  S[(int64_t)a * ld + c] = t;
  S[(int64_t)c * ld + a] = t;
}

// the two slots left, x < y, and S(x, y)
__global__ __launch_bounds__(HC_PICK) void nj_last_kernel(const double* __restrict__ S, int n, int64_t ld, const int32_t* __restrict__ live,
                                                         double* __restrict__ last) {
  __shared__ int lo, hi;
  if (threadIdx.x == 0) lo = n, hi = -1;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += HC_PICK)
    if (live[i]) atomicMin(&lo, i), atomicMax(&hi, i);
  __syncthreads();
  if (threadIdx.x == 0 && lo < hi) last[0] = (double)lo, last[1] = (double)hi, last[2] = S[(int64_t)lo * ld + hi];
}

// D -> S on the device with row stride ld, or TPG_ENUMERIC for a lower triangle that is not finite
int tr_build(tpg_ctx* ctx, const double* D, int64_t n, int64_t ld, InBuf& in, DevArena& sc, double** S) {
  TPG_TRY(in.init(ctx, D, sizeof(double) * (size_t)n * (size_t)n));
  int32_t* d_bad;
  TPG_TRY(sc.get(S, (size_t)n * (size_t)ld));
  TPG_TRY(sc.get(&d_bad, 4));
  TPG_HIP(hipMemsetAsync(d_bad, 0, sizeof(int32_t), ctx->stream));
  TPG_LAUNCH(ctx, "tr_build", tr_build_kernel, dim3((unsigned)ceil_div(n, HC_BLOCK), (unsigned)n), dim3(HC_BLOCK), 0, in.dev<double>(), (int)n,
             ld, *S, d_bad);
  TPG_CHECK_LAUNCH();
  int32_t bad = 0;
  TPG_HIP(tpg_fetch_small(ctx, &bad, d_bad, sizeof(int32_t)));
  TPG_REQUIRE(!bad, TPG_ENUMERIC, "the strict lower triangle of D holds a value that is not finite");
  return TPG_OK;
}

}  // namespace

extern "C" int tpg_hclust_dist(tpg_ctx* ctx, const double* D, int64_t n, int method, int32_t* merge_a, int32_t* merge_b, double* height) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && D && merge_a && merge_b && height, TPG_EINVAL, "null argument");
  TPG_REQUIRE(n >= 1 && n <= TPG_HCLUST_MAX_N, TPG_EINVAL, "n = %lld outside [1, %d]", (long long)n, TPG_HCLUST_MAX_N);
  TPG_REQUIRE(method >= LINK_SINGLE && method <= LINK_WARD, TPG_EINVAL, "method = %d is none of TPG_LINK_*", method);
  InBuf in;
  DevArena sc;
  double* S;
  TPG_TRY(tr_build(ctx, D, n, n, in, sc, &S));
  if (n == 1) return TPG_OK;  // no merge: the outputs are empty
  const int ni = (int)n, steps = ni - 1;
  double *dnn, *d_height;
  int32_t *size, *live, *nn, *list, *d_len, *d_failed, *hist, *d_ma, *d_mb;
  HcStep* cur;
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
  TPG_LAUNCH(ctx, "hc_start", hc_start_kernel, dim3(tiles), dim3(HC_BLOCK), 0, ni, size, live, list, d_len, d_failed);
  TPG_CHECK_LAUNCH();
  TPG_LAUNCH(ctx, "hc_rownn", hc_rownn_kernel, dim3(nn_grid), dim3(HC_BLOCK), 0, S, ni, live, list, d_len, nn, dnn);
  TPG_CHECK_LAUNCH();
  for (int s = 0; s < steps; s++) {
    TPG_LAUNCH(ctx, "hc_pick", hc_pick_kernel, dim3(1), dim3(HC_PICK), 0, ni, s, size, live, nn, dnn, d_len, hist, d_failed, cur, d_ma, d_mb,
               d_height);
#define TR_UPDATE(L) \
  TPG_LAUNCH(ctx, "tr_update", tr_update_kernel<L>, dim3(tiles), dim3(HC_BLOCK), 0, S, ni, size, live, cur, nn, dnn, list, d_len)
    switch (method) {
      case LINK_SINGLE: TR_UPDATE(LINK_SINGLE); break;
      case LINK_COMPLETE: TR_UPDATE(LINK_COMPLETE); break;
      case LINK_AVERAGE: TR_UPDATE(LINK_AVERAGE); break;
      case LINK_MCQUITTY: TR_UPDATE(LINK_MCQUITTY); break;
      default: TR_UPDATE(LINK_WARD); break;
    }
#undef TR_UPDATE
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
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return TPG_OK;
}

extern "C" int tpg_nj(tpg_ctx* ctx, const double* D, int64_t n, int32_t* join_a, int32_t* join_b, double* len_a, double* len_b, double* last) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && D, TPG_EINVAL, "null argument");
  TPG_REQUIRE(n >= 1 && n <= TPG_HCLUST_MAX_N, TPG_EINVAL, "n = %lld outside [1, %d]", (long long)n, TPG_HCLUST_MAX_N);
  TPG_REQUIRE(n < 2 || last, TPG_EINVAL, "null argument");
  TPG_REQUIRE(n < 3 || (join_a && join_b && len_a && len_b), TPG_EINVAL, "null argument");
  InBuf in;
  DevArena sc;
  double* S;
  const int64_t ld = (n + 1) & ~(int64_t)1;
  TPG_TRY(tr_build(ctx, D, n, ld, in, sc, &S));
  if (n == 1) return TPG_OK;  // no pair: the outputs are empty
  const int ni = (int)n, joins = ni - 2;
  double *R, *rowq, *d_la, *d_lb, *d_last;
  int32_t *live, *rowj, *d_failed, *d_ja, *d_jb;
  NjStep* cur;
  TPG_TRY(sc.get(&R, (size_t)n + 2));
  TPG_TRY(sc.get(&live, (size_t)n + 2));
  TPG_TRY(sc.get(&rowq, (size_t)n));
  TPG_TRY(sc.get(&rowj, (size_t)n));
  TPG_TRY(sc.get(&d_la, (size_t)std::max(joins, 1)));
  TPG_TRY(sc.get(&d_lb, (size_t)std::max(joins, 1)));
  TPG_TRY(sc.get(&d_ja, (size_t)std::max(joins, 1)));
  TPG_TRY(sc.get(&d_jb, (size_t)std::max(joins, 1)));
  TPG_TRY(sc.get(&d_last, 3));
  TPG_TRY(sc.get(&d_failed, 4));
  TPG_TRY(sc.get(&cur, 1));
  const unsigned tiles = (unsigned)ceil_div(n, HC_BLOCK), row_grid = (unsigned)std::min<int64_t>(n, NJ_GRID);
  TPG_LAUNCH(ctx, "nj_start", nj_start_kernel, dim3((unsigned)ceil_div(n + 2, HC_BLOCK)), dim3(HC_BLOCK), 0, S, ni, ld, live, R, d_failed);
  TPG_CHECK_LAUNCH();
  for (int s = 0; s < joins; s++) {
    const int r = ni - s;
    TPG_LAUNCH(ctx, "nj_rowmin", nj_rowmin_kernel, dim3(row_grid), dim3(HC_BLOCK), 0, S, ni, ld, r, live, R, rowq, rowj);
    TPG_LAUNCH(ctx, "nj_pick", nj_pick_kernel, dim3(1), dim3(HC_PICK), 0, S, ni, ld, r, s, live, R, rowq, rowj, d_failed, cur, d_ja, d_jb, d_la,
               d_lb);
    TPG_LAUNCH(ctx, "nj_update", nj_update_kernel, dim3(tiles), dim3(HC_BLOCK), 0, S, ni, ld, live, R, cur);
    if ((s & 255) == 255) TPG_CHECK_LAUNCH();
  }
  TPG_LAUNCH(ctx, "nj_last", nj_last_kernel, dim3(1), dim3(HC_PICK), 0, S, ni, ld, live, d_last);
  TPG_CHECK_LAUNCH();
  int32_t failed = 0;
  TPG_HIP(tpg_fetch_small(ctx, &failed, d_failed, sizeof(int32_t)));  // (waits for every join: a fault surfaces here, before an output is touched)
  TPG_REQUIRE(!failed, TPG_ENUMERIC, "a join found no pair: every criterion value is NaN");
  TPG_TRY(tpg_deliver(ctx, join_a, d_ja, (size_t)joins));
  TPG_TRY(tpg_deliver(ctx, join_b, d_jb, (size_t)joins));
  TPG_TRY(tpg_deliver(ctx, len_a, d_la, (size_t)joins));
  TPG_TRY(tpg_deliver(ctx, len_b, d_lb, (size_t)joins));
  TPG_TRY(tpg_deliver(ctx, last, d_last, (size_t)3));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return TPG_OK;
}

extern "C" int tpg_hclust_order(int64_t n, const int32_t* merge_a, const int32_t* merge_b, int32_t* order) {
  TPG_REQUIRE(order && (n == 1 || (merge_a && merge_b)), TPG_EINVAL, "null argument");
  const char* why = "";
  TPG_REQUIRE(host_hclust_order(n, merge_a, merge_b, order, &why) == HOST_HCLUST_OK, TPG_EINVAL, "hclust_order: %s", why);
  return TPG_OK;
}

extern "C" int tpg_nj_edges(int64_t n, const int32_t* join_a, const int32_t* join_b, const double* len_a, const double* len_b,
                            const double* last, int32_t* edge, double* edge_length) {
  TPG_REQUIRE(join_a && join_b && len_a && len_b && last && edge && edge_length, TPG_EINVAL, "null argument");
  const char* why = "";
  TPG_REQUIRE(host_tree_nj_edges(n, join_a, join_b, len_a, len_b, last, edge, edge_length, &why) == HOST_TREE_OK, TPG_EINVAL,
              "nj_edges: %s", why);
  return TPG_OK;
}
