// amova.hip -- the device side of include/tpg.h "AMOVA": tpg_class_sums, the within-class sums of an n x n matrix of doubles
// under a batch of R labelings (the hot path of a label-permutation test on a distance matrix: AMOVA here, PERMANOVA alike),
// and the C entry points of the host pieces (host/host_amova.h).  tpg_pairwise_sqdist, which leaves the matrix in HBM, is an
// epilogue of pairwise.hip.
//
//  * classsum_partial_kernel: a workgroup owns CS_TR = 256 rows (one row i per lane, so that a wave reads 512 contiguous bytes
//    of column j), one chunk of CS_C = 512 columns and one batch of CS_B = 32 labelings.  A lane keeps its own 32 labels and 32
//    FP64 accumulators in registers -- 32 independent chains: the add latency is covered without a second wave -- and walks the
//    columns of the chunk in ascending order.  The labels of column j are the same for every lane: 128 contiguous bytes of the
//    label table at a wave-uniform address, which the compiler reads through the scalar cache.  Per (i, j, labeling): one
//    compare, a select of the two halves of a_ij against +0.0 and one v_add_f64; an accumulator starts at +0.0 and can never
//    become -0.0, so adding +0.0 is the same as skipping the term, and a NaN outside the class is selected away, not multiplied.
//    The 32 chunk partials of a row leave as plain vector stores, coalesced over the rows.
//  * classsum_rows_kernel: t(r, i) = the chunk partials of (r, i) in ascending chunk order from 0.0; one thread per (r, i).
//  * classsum_reduce_kernel: sums[r][c] = t(r, i) over the rows of class c in ascending i from 0.0; one thread per (r, c), the loads
//    of 16 rows ahead of the additions of the 16 before them (one row per trip to memory took longer than the partial kernel).
// The three run for every call and every size: nothing in the order depends on R, the batch or the grid.  No atomics.
#include <string.h>

#include <algorithm>

#include "common.h"
#include "host/host_amova.h"

#define CS_C TPG_CLASSSUM_CHUNK
#define CS_TR TPG_CLASSSUM_TILE_ROWS
#define CS_B TPG_CLASSSUM_BATCH
#define CS_RU 16  // rows in flight per thread of the reduce kernel
static_assert(CS_C == HOST_CLASSSUM_CHUNK && CS_TR == HOST_CLASSSUM_TILE_ROWS && CS_B == HOST_CLASSSUM_BATCH &&
                  TPG_CLASSSUM_MAX_CLASSES == HOST_CLASSSUM_MAX_CLASSES,
              "one set of constants");
static_assert(CS_B % 4 == 0 && CS_C % 4 == 0, "the label rows are read four at a time, the columns unrolled by four");

// grid (row tiles, chunks, batches).  tab[(b n + i) CS_B + q]: the label of individual i under labeling q of batch b, -1 outside.
// part[(k rows_pad + b CS_B + q) n + i]: the partial of row i, labeling q of batch b, over chunk k.
__global__ __launch_bounds__(CS_TR) void classsum_partial_kernel(const double* __restrict__ A, int64_t n, const int32_t* __restrict__ tab,
                                                                 int64_t rows_pad, double* __restrict__ part) {
  const int64_t i = (int64_t)blockIdx.x * CS_TR + threadIdx.x;
  const int64_t k = blockIdx.y, b = blockIdx.z;
  const bool live = i < n;
  const int64_t ic = live ? i : n - 1;  // a lane past the last row reads the last row and stores nothing
  int32_t my[CS_B];
  double acc[CS_B];
  {
    const int4* p = (const int4*)(tab + (b * n + ic) * CS_B);
#pragma unroll
    for (int q = 0; q < CS_B / 4; q++) {
      const int4 w = p[q];
      my[4 * q] = w.x; my[4 * q + 1] = w.y; my[4 * q + 2] = w.z; my[4 * q + 3] = w.w;
    }
  }
#pragma unroll
  for (int q = 0; q < CS_B; q++) {
    if (my[q] < 0 || !live) my[q] = -2;  // outside the labeling: equal to no column's label (-1 included)
    acc[q] = 0.0;
  }
  const int64_t j0 = k * CS_C, j1 = j0 + CS_C < n ? j0 + CS_C : n;
  const double* a = A + ic;
  const int32_t* ct = tab + b * n * CS_B;
  auto column = [&](int64_t j, double x) {
    const int32_t* cl = ct + j * CS_B;  // wave-uniform
#pragma unroll
    for (int q = 0; q < CS_B; q++) acc[q] += (cl[q] == my[q]) ? x : 0.0;
  };
  int64_t j = j0;
  for (; j + 4 <= j1; j += 4) {
    const double x0 = a[j * n], x1 = a[(j + 1) * n], x2 = a[(j + 2) * n], x3 = a[(j + 3) * n];
    column(j, x0);
    column(j + 1, x1);
    column(j + 2, x2);
    column(j + 3, x3);
  }
  for (; j < j1; j++) column(j, a[j * n]);
  if (live) {
#pragma unroll
    for (int q = 0; q < CS_B; q++) part[(k * rows_pad + b * CS_B + q) * n + i] = acc[q];
  }
}

// t[r n + i] = the chunk partials of (r, i) in ascending chunk order from 0.0
__global__ __launch_bounds__(256) void classsum_rows_kernel(const double* __restrict__ part, int64_t n, int64_t rows, int64_t rows_pad,
                                                            int64_t nchunks, double* __restrict__ t) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * n) return;
  const int64_t r = idx / n, i = idx - r * n;
  double s = 0.0;
  for (int64_t k = 0; k < nchunks; k++) s += part[(k * rows_pad + r) * n + i];
  t[idx] = s;
}

// sums[r nclasses + c] = t(r, i) over the rows i of class c in ascending order from 0.0
__global__ __launch_bounds__(256) void classsum_reduce_kernel(const double* __restrict__ t, const int32_t* __restrict__ tab, int64_t n,
                                                              int64_t rows, int nclasses, double* __restrict__ sums) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * nclasses) return;
  const int64_t r = idx / nclasses;
  const int32_t c = (int32_t)(idx - r * nclasses);
  const int32_t* lab = tab + (r / CS_B) * n * CS_B + (r % CS_B);
  const double* tr = t + r * n;
  // One chain of additions per thread: the loads of the next CS_RU rows are issued before the additions of the current ones, or
  // every row would cost a trip to memory.  A row past the end reads row n - 1 and adds +0.0; t(r, i) and s start at +0.0 and
  // never become -0.0, so adding +0.0 to s is the same as skipping the row.
  int32_t l0[CS_RU], l1[CS_RU];
  double x0[CS_RU], x1[CS_RU];
  auto load = [&](int64_t i0, int32_t* l, double* x) {
#pragma unroll
    for (int u = 0; u < CS_RU; u++) {
      const int64_t i = i0 + u < n ? i0 + u : n - 1;
      l[u] = lab[i * CS_B];
      x[u] = tr[i];
    }
  };
  auto add = [&](int64_t i0, const int32_t* l, const double* x, double s) {
#pragma unroll
    for (int u = 0; u < CS_RU; u++) s += (i0 + u < n && l[u] == c) ? x[u] : 0.0;
    return s;
  };
  double s = 0.0;
  load(0, l0, x0);
  for (int64_t i0 = 0; i0 < n; i0 += 2 * CS_RU) {
    load(i0 + CS_RU, l1, x1);
    s = add(i0, l0, x0, s);
    load(i0 + 2 * CS_RU, l0, x0);
    s = add(i0 + CS_RU, l1, x1, s);
  }
  sums[idx] = s;
}

extern "C" int64_t tpg_classsum_chunk(void) { return CS_C; }
extern "C" int64_t tpg_classsum_tile_rows(void) { return CS_TR; }
extern "C" int64_t tpg_classsum_batch(void) { return CS_B; }
extern "C" int64_t tpg_class_sums_scratch_bytes(int64_t n, int64_t R, int nclasses) { return host_classsum_scratch_bytes(n, R, nclasses); }

extern "C" int tpg_class_sums(tpg_ctx* ctx, const double* A, int64_t n, const int32_t* labels, int64_t R, int nclasses, double* sums) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx, TPG_EINVAL, "null argument");
  char msg[320];
  if (host_classsum_check(n, labels, R, nclasses, msg, sizeof(msg))) {
    tpg_set_error("%s", msg);
    return TPG_EINVAL;
  }
  if (R == 0) return TPG_OK;
  TPG_REQUIRE(A && sums, TPG_EINVAL, "null argument");
  const int64_t nchunks = host_classsum_chunks(n), ntiles = ceil_div(n, CS_TR);
  const int64_t pass = std::min(host_classsum_pass_rows(n), ceil_div(R, CS_B) * CS_B);  // rows of a pass, padded to whole batches
  InBuf ia;
  TPG_TRY(ia.init(ctx, A, sizeof(double) * (size_t)n * (size_t)n));
  DevArena sc;
  int32_t* d_tab = nullptr;
  double *d_part = nullptr, *d_t = nullptr, *d_sums = nullptr;
  TPG_TRY(sc.get(&d_tab, (size_t)pass * (size_t)n));
  TPG_TRY(sc.get(&d_part, (size_t)nchunks * (size_t)pass * (size_t)n));
  TPG_TRY(sc.get(&d_t, (size_t)pass * (size_t)n));
  TPG_TRY(sc.get(&d_sums, (size_t)pass * (size_t)nclasses));
  std::vector<int32_t> tab((size_t)pass * (size_t)n);
  for (int64_t r0 = 0; r0 < R; r0 += pass) {
    const int64_t rows = std::min(pass, R - r0), nb = ceil_div(rows, CS_B), rows_pad = nb * CS_B;
    host_classsum_table(n, labels + r0 * n, rows, tab.data());
    TPG_HIP(tpg_upload(ctx, d_tab, tab.data(), sizeof(int32_t) * (size_t)rows_pad * (size_t)n));
    TPG_LAUNCH(ctx, "classsum_partial", classsum_partial_kernel, dim3((unsigned)ntiles, (unsigned)nchunks, (unsigned)nb), dim3(CS_TR), 0,
               ia.dev<double>(), n, (const int32_t*)d_tab, rows_pad, d_part);
    TPG_LAUNCH(ctx, "classsum_rows", classsum_rows_kernel, dim3((unsigned)ceil_div(rows * n, 256)), dim3(256), 0, (const double*)d_part, n,
               rows, rows_pad, nchunks, d_t);
    TPG_LAUNCH(ctx, "classsum_reduce", classsum_reduce_kernel, dim3((unsigned)ceil_div(rows * nclasses, 256)), dim3(256), 0,
               (const double*)d_t, (const int32_t*)d_tab, n, rows, nclasses, d_sums);
    TPG_CHECK_LAUNCH();
    // (the download waits for the stream: the host table is free for the next pass, the scratch for its kernels)
    TPG_HIP(tpg_download(ctx, sums + r0 * nclasses, d_sums, sizeof(double) * (size_t)rows * (size_t)nclasses));
  }
  TPG_HIP(hipStreamSynchronize(ctx->stream));  // the scratch of this call goes back to the pool at scope exit
  return TPG_OK;
}

extern "C" int tpg_amova_perm_labels(int64_t n, const int32_t* pop0, int npop, const int32_t* region_of_pop0, int nregion, int scheme,
                                     uint64_t seed, int64_t r, int32_t* pop_out, int32_t* region_of_pop_out) {
  char msg[256];
  if (host_amova_labels(n, pop0, npop, region_of_pop0, nregion, scheme, seed, r, pop_out, region_of_pop_out, msg, sizeof(msg))) {
    tpg_set_error("%s", msg);
    return TPG_EINVAL;
  }
  return TPG_OK;
}

extern "C" int tpg_amova_from_sums(int npop, const int64_t* pop_size, const double* pop_sum, int nregion, const int32_t* region_of_pop0,
                                   const double* region_sum, double total_sum, double* out) {
  char msg[256];
  if (host_amova_from_sums(npop, pop_size, pop_sum, nregion, region_of_pop0, region_sum, total_sum, out, msg, sizeof(msg))) {
    tpg_set_error("%s", msg);
    return TPG_EINVAL;
  }
  return TPG_OK;
}
