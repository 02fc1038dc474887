// mantel.hip -- the device side of include/tpg.h "Mantel tests": tpg_mantel_sums, the cross sums of an n x n matrix A, gathered
// through a batch of R permutations, with up to four matrices B_q (the hot path of a Mantel, partial Mantel or stratified Mantel
// test), the streaming kernels tpg_offdiag_moments and tpg_offdiag_center, and the C entry points of the host pieces
// (host/host_mantel.h).
//
//  * mantel_product_kernel<Q>: a workgroup of ML = 256 threads owns ONE column a of A, which it copies into LDS once (8 n bytes,
//    128 KiB at n = 16 384), and one batch of MANTEL_BATCH = 32 permutations.  Under permutation r that column is the column of
//    j = pi_r^-1(a) -- every (r, j) belongs to exactly one column a, so the workgroups of a batch cover every column term once --
//    and c(r, q, j) = sum_i A[pi_r(i), a] B_q[i, j]: thread t walks i = t, t + ML, ... in ascending order, reads pi_r(i) and
//    B_q[i + j n] with coalesced loads (column j of B_q is contiguous, row r of the permutations too), eight strides ahead of
//    their additions at Q = 1 and four otherwise, and gathers A from LDS:
//    the only scattered access of the sum never leaves the CU.  The product is rounded, then added (no FMA: $(FP_STRICT)); on
//    i = j it is selected away against +0.0, which a partial that started at +0.0 cannot tell from a skip, so a NaN on either
//    diagonal reaches nothing.  The ML partials of a term are added as the header says: through LDS for h = 128 and 64 (one
//    barrier per permutation, two buffers in turn), by lane shuffles of wave 0 for h = 32 .. 1.  The term leaves by a plain
//    vector store.  Staging A by the column of A, not of B, is what keeps the LDS image for the whole batch: no store to LDS and
//    no second barrier per permutation.
//  * mantel_reduce_kernel: sums[r][q] = c(r, q, j) in ascending j from +0.0; one thread per (r, q), the loads of 16 terms ahead
//    of the additions of the 16 before them.
//  * offdiag_moments_kernel: the same partials and the same tree with b = 1.0 (the product a * 1.0 is a) and b = a, one
//    workgroup per column; offdiag_center_kernel: one thread per entry.
// Nothing in the order depends on R, Q, the batch, the pass or the grid.  No atomics.
#include <string.h>

#include <algorithm>

#include "common.h"
#include "host/host_mantel.h"

#define ML TPG_MANTEL_LANES
#define MANTEL_RU 16  // terms in flight per thread of the reduce kernel
static_assert(ML == HOST_MANTEL_LANES && TPG_MANTEL_MAX_N == HOST_MANTEL_MAX_N && TPG_MANTEL_MAX_Q == HOST_MANTEL_MAX_Q, "one set of constants");
static_assert(ML == 256, "the tree below: two steps across the four waves, six inside wave 0");

struct MantelMats {
  const double* b[TPG_MANTEL_MAX_Q];
};

// The partials s[q] of thread t -> the column terms in lane 0 of wave 0 (returned to every lane of wave 0; other waves get
// garbage).  buf: Q x ML doubles of LDS that nobody else touches until the NEXT barrier of the workgroup has been passed.
template <int Q>
__device__ __forceinline__ void mantel_tree(const double (&s)[Q], double* buf, int t, double (&c)[Q]) {
#pragma unroll
  for (int q = 0; q < Q; q++) buf[q * ML + t] = s[q];
  __syncthreads();
  if (t < 64) {
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const double* b = buf + q * ML + t;
      // h = 128: s[t] += s[t + 128] for t < 128; h = 64: s[t] += s[t + 64] for t < 64
      double v = (b[0] + b[128]) + (b[64] + b[192]);
#pragma unroll
      for (int h = 32; h >= 1; h >>= 1) v += __shfl_down(v, h, 64);  // lane t < h reads lane t + h < 2 h: as the header's tree
      c[q] = v;
    }
  }
}

// grid (columns a of A, batches of permutations).  perm[r n + i] = pi_r(i), inv[r n + a] = pi_r^-1(a), r = 0 .. rows - 1.
// term[(r Q + q) n + j] = c(r, q, j).  Dynamic LDS: (n + 2 Q ML) doubles.
template <int Q>
__global__ __launch_bounds__(ML) void mantel_product_kernel(const double* __restrict__ A, MantelMats B, int n, const int32_t* __restrict__ perm,
                                                            const int32_t* __restrict__ inv, int rows, double* __restrict__ term) {
  extern __shared__ double mantel_lds[];
  double* col = mantel_lds;
  double* red = mantel_lds + n;
  const int t = threadIdx.x, a = blockIdx.x;
  const int r_begin = blockIdx.y * HOST_MANTEL_BATCH, r_end = min(rows, r_begin + HOST_MANTEL_BATCH);
  {
    const double* src = A + (size_t)a * n;
    for (int i = t; i < n; i += ML) col[i] = src[i];
  }
  __syncthreads();
  for (int r = r_begin; r < r_end; r++) {
    const int32_t* pr = perm + (size_t)r * n;
    const int j = inv[(size_t)r * n + a];  // the same for every thread
    const double* bq[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) bq[q] = B.b[q] + (size_t)j * n;
    double s[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) s[q] = 0.0;
    // U strides' loads ahead of their additions, the additions in ascending i.  A stride past the end reads row t again and
    // adds +0.0, as the diagonal does: a partial that started at +0.0 cannot tell that from a skip.  Eight strides in flight
    // beat four at Q = 1 (26.8 against 28.8 ms at n = 5 000, 66.9 against 83.8 at n = 16 384, where one workgroup has the CU
    // to itself); at Q = 2 two jobs could not tell them apart (56.4 and 56.1 ms), so the registers stay with four there.
    constexpr int MANTEL_U = HOST_MANTEL_STRIDES(Q);
    for (int i = t; i < n; i += MANTEL_U * ML) {
      int32_t p[MANTEL_U];
      double b[MANTEL_U][Q], x[MANTEL_U];
#pragma unroll
      for (int u = 0; u < MANTEL_U; u++) {
        const int iu = i + u * ML < n ? i + u * ML : t;
        p[u] = pr[iu];
#pragma unroll
        for (int q = 0; q < Q; q++) b[u][q] = bq[q][iu];
      }
#pragma unroll
      for (int u = 0; u < MANTEL_U; u++) x[u] = col[p[u]];
#pragma unroll
      for (int u = 0; u < MANTEL_U; u++) {
        const bool skip = i + u * ML >= n || i + u * ML == j;
#pragma unroll
        for (int q = 0; q < Q; q++) {
          const double prod = x[u] * b[u][q];
          s[q] += skip ? 0.0 : prod;
        }
      }
    }
    double c[Q];
    mantel_tree<Q>(s, red + ((r - r_begin) & 1) * Q * ML, t, c);
    if (t == 0) {
#pragma unroll
      for (int q = 0; q < Q; q++) term[((size_t)r * Q + q) * n + j] = c[q];
    }
  }
}

// sums[k] = term[k n + j] in ascending j from +0.0, k = 0 .. count - 1
__global__ __launch_bounds__(64) void mantel_reduce_kernel(const double* __restrict__ term, int n, int count, double* __restrict__ sums) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const double* tr = term + (size_t)k * n;
  // One chain of additions per thread: the loads of the next MANTEL_RU terms are issued before the additions of the current
  // ones.  A term past the end reads term n - 1 and is not added.
  double x0[MANTEL_RU], x1[MANTEL_RU];
  auto load = [&](int j0, double* x) {
#pragma unroll
    for (int u = 0; u < MANTEL_RU; u++) x[u] = tr[j0 + u < n ? j0 + u : n - 1];
  };
  auto add = [&](int j0, const double* x, double s) {
#pragma unroll
    for (int u = 0; u < MANTEL_RU; u++)
      if (j0 + u < n) s += x[u];
    return s;
  };
  double s = 0.0;
  load(0, x0);
  for (int j0 = 0; j0 < n; j0 += 2 * MANTEL_RU) {
    load(j0 + MANTEL_RU, x1);
    s = add(j0, x0, s);
    load(j0 + 2 * MANTEL_RU, x0);
    s = add(j0 + MANTEL_RU, x1, s);
  }
  sums[k] = s;
}

// grid (columns j).  term[j] = the column term of S (b = 1.0), term[n + j] = that of SS (b = a), identity permutation.
__global__ __launch_bounds__(ML) void offdiag_moments_kernel(const double* __restrict__ A, int n, double* __restrict__ term) {
  __shared__ double red[2 * ML];
  const int t = threadIdx.x, j = blockIdx.x;
  const double* src = A + (size_t)j * n;
  double s[2] = {0.0, 0.0};
  for (int i = t; i < n; i += ML) {
    const double x = src[i];
    const double xx = x * x;
    s[0] += i == j ? 0.0 : x;
    s[1] += i == j ? 0.0 : xx;
  }
  double c[2];
  mantel_tree<2>(s, red, t, c);
  if (t == 0) {
    term[j] = c[0];
    term[n + j] = c[1];
  }
}

__global__ __launch_bounds__(256) void offdiag_center_kernel(const double* A, int n, double mean, double* out) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)n * n) return;
  const int j = (int)(idx / n), i = (int)(idx - (size_t)j * n);
  out[idx] = i == j ? 0.0 : A[idx] - mean;
}

template <int Q>
static int mantel_launch_product(tpg_ctx* ctx, const double* d_A, const MantelMats& B, int n, const int32_t* d_perm, const int32_t* d_inv,
                                 int rows, double* d_term) {
  const size_t lds = sizeof(double) * ((size_t)n + 2 * Q * ML);
  // the limit at the largest n: a launch above 64 KiB needs it raised (on the device of this context)
  TPG_HIP(hipFuncSetAttribute((const void*)mantel_product_kernel<Q>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(double) * ((size_t)TPG_MANTEL_MAX_N + 2 * Q * ML))));
  TPG_LAUNCH(ctx, "mantel_product", mantel_product_kernel<Q>, dim3((unsigned)n, (unsigned)ceil_div(rows, HOST_MANTEL_BATCH)), dim3(ML), lds,
             d_A, B, n, d_perm, d_inv, rows, d_term);
  return TPG_OK;
}

extern "C" int64_t tpg_mantel_lanes(void) { return ML; }
extern "C" int64_t tpg_mantel_strides(int Q) { return Q >= 1 && Q <= TPG_MANTEL_MAX_Q ? HOST_MANTEL_STRIDES(Q) : -1; }
extern "C" int64_t tpg_mantel_pass_rows(int64_t n, int Q) { return host_mantel_size_ok(n, 0, Q) ? host_mantel_pass_rows(n, Q) : -1; }
extern "C" int64_t tpg_mantel_scratch_bytes(int64_t n, int64_t R, int Q) { return host_mantel_scratch_bytes(n, R, Q); }

extern "C" int tpg_mantel_sums(tpg_ctx* ctx, const double* A, const double** B, int Q, int64_t n, const int32_t* perms, int64_t R,
                               double* sums) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx, TPG_EINVAL, "null argument");
  char msg[320];
  if (host_mantel_check(n, Q, perms, R, msg, sizeof(msg))) {
    tpg_set_error("%s", msg);
    return TPG_EINVAL;
  }
  TPG_REQUIRE(A && B && (sums || R == 0), TPG_EINVAL, "null argument");
  for (int q = 0; q < Q; q++) TPG_REQUIRE(B[q], TPG_EINVAL, "null argument");
  if (R == 0) return TPG_OK;
  const size_t bytes = sizeof(double) * (size_t)n * (size_t)n;
  InBuf ia, ib[TPG_MANTEL_MAX_Q];
  TPG_TRY(ia.init(ctx, A, bytes));
  MantelMats mats = {};
  for (int q = 0; q < Q; q++) {
    TPG_TRY(ib[q].init(ctx, B[q], bytes));
    mats.b[q] = ib[q].dev<double>();
  }
  const int64_t pass = std::min(host_mantel_pass_rows(n, Q), R);
  DevArena sc;
  int32_t *d_perm = nullptr, *d_inv = nullptr;
  double *d_term = nullptr, *d_sums = nullptr;
  TPG_TRY(sc.get(&d_perm, (size_t)pass * (size_t)n));
  TPG_TRY(sc.get(&d_inv, (size_t)pass * (size_t)n));
  TPG_TRY(sc.get(&d_term, (size_t)pass * (size_t)Q * (size_t)n));
  TPG_TRY(sc.get(&d_sums, (size_t)pass * (size_t)Q));
  std::vector<int32_t> inv((size_t)pass * (size_t)n);
  for (int64_t r0 = 0; r0 < R; r0 += pass) {
    const int64_t rows = std::min(pass, R - r0);
    host_mantel_inverse(n, perms + r0 * n, rows, inv.data());
    TPG_HIP(tpg_upload(ctx, d_perm, perms + r0 * n, sizeof(int32_t) * (size_t)rows * (size_t)n));
    TPG_HIP(tpg_upload(ctx, d_inv, inv.data(), sizeof(int32_t) * (size_t)rows * (size_t)n));
    switch (Q) {
      case 1: TPG_TRY(mantel_launch_product<1>(ctx, ia.dev<double>(), mats, (int)n, d_perm, d_inv, (int)rows, d_term)); break;
      case 2: TPG_TRY(mantel_launch_product<2>(ctx, ia.dev<double>(), mats, (int)n, d_perm, d_inv, (int)rows, d_term)); break;
      case 3: TPG_TRY(mantel_launch_product<3>(ctx, ia.dev<double>(), mats, (int)n, d_perm, d_inv, (int)rows, d_term)); break;
      default: TPG_TRY(mantel_launch_product<4>(ctx, ia.dev<double>(), mats, (int)n, d_perm, d_inv, (int)rows, d_term)); break;
    }
    TPG_LAUNCH(ctx, "mantel_reduce", mantel_reduce_kernel, dim3((unsigned)ceil_div(rows * Q, 64)), dim3(64), 0, (const double*)d_term, (int)n,
               (int)(rows * Q), d_sums);
    TPG_CHECK_LAUNCH();
    // (the download waits for the stream: the host's inverses are free for the next pass, the scratch for its kernels)
    TPG_HIP(tpg_download(ctx, sums + r0 * Q, d_sums, sizeof(double) * (size_t)rows * (size_t)Q));
  }
  TPG_HIP(hipStreamSynchronize(ctx->stream));  // the scratch of this call goes back to the pool at scope exit
  return TPG_OK;
}

extern "C" int tpg_offdiag_moments(tpg_ctx* ctx, const double* A, int64_t n, double* out) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && A && out, TPG_EINVAL, "null argument");
  TPG_REQUIRE(n >= 1 && n <= TPG_MANTEL_MAX_N, TPG_EINVAL, "n = %lld out of [1, TPG_MANTEL_MAX_N = %d]", (long long)n, TPG_MANTEL_MAX_N);
  InBuf ia;
  TPG_TRY(ia.init(ctx, A, sizeof(double) * (size_t)n * (size_t)n));
  DevArena sc;
  double *d_term = nullptr, *d_sums = nullptr;
  TPG_TRY(sc.get(&d_term, 2 * (size_t)n));
  TPG_TRY(sc.get(&d_sums, 2));
  TPG_LAUNCH(ctx, "offdiag_moments", offdiag_moments_kernel, dim3((unsigned)n), dim3(ML), 0, ia.dev<double>(), (int)n, d_term);
  TPG_LAUNCH(ctx, "mantel_reduce", mantel_reduce_kernel, dim3(1), dim3(64), 0, (const double*)d_term, (int)n, 2, d_sums);
  TPG_CHECK_LAUNCH();
  double got[2];
  TPG_HIP(tpg_download(ctx, got, d_sums, sizeof(got)));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  out[0] = got[0];
  out[1] = got[1];
  return TPG_OK;
}

extern "C" int tpg_offdiag_center(tpg_ctx* ctx, const double* A, int64_t n, double mean, double* out) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && A && out, TPG_EINVAL, "null argument");
  TPG_REQUIRE(n >= 1 && n <= TPG_MANTEL_MAX_N, TPG_EINVAL, "n = %lld out of [1, TPG_MANTEL_MAX_N = %d]", (long long)n, TPG_MANTEL_MAX_N);
  const size_t bytes = sizeof(double) * (size_t)n * (size_t)n;
  InBuf ia;
  TPG_TRY(ia.init(ctx, A, bytes));
  OutBuf ob;
  TPG_TRY(ob.init(out, bytes));
  TPG_LAUNCH(ctx, "offdiag_center", offdiag_center_kernel, dim3((unsigned)ceil_div(n * n, 256)), dim3(256), 0, ia.dev<double>(), (int)n, mean,
             ob.dev<double>());
  TPG_CHECK_LAUNCH();
  TPG_TRY(ob.commit(ctx));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return TPG_OK;
}

extern "C" int tpg_mantel_perms(int64_t n, const int32_t* strata0, int nstrata, uint64_t seed, int64_t r0, int64_t R, int32_t* out) {
  char msg[256];
  if (host_mantel_perms(n, strata0, nstrata, seed, r0, R, out, msg, sizeof(msg))) {
    tpg_set_error("%s", msg);
    return TPG_EINVAL;
  }
  return TPG_OK;
}

extern "C" int tpg_mantel_from_sums(int64_t N, double Sa, double Saa, double Sb, double Sbb, double Sab, double* out) {
  TPG_REQUIRE(out, TPG_EINVAL, "null argument");
  *out = host_mantel_from_sums(N, Sa, Saa, Sb, Sbb, Sab);
  return TPG_OK;
}

extern "C" double tpg_mantel_partial(double r_ab, double r_ac, double r_bc) { return host_mantel_partial(r_ab, r_ac, r_bc); }
