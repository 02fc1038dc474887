// snmf.hip -- ancestry proportions by sparse non-negative matrix factorisation (include/tpg.h "sNMF").
//
// LEA is not among the reference's sources (R/gt_snmf.R writes a .geno file and calls LEA::snmf), so the loss, the alternating
// non-negative least squares and the stop rule are the ones include/tpg.h defines.
//
// The state lives on the device as Qd[i * KT + k] and Gd[(3 j + c) * KT + k]: a row per individual / (locus, class), padded from
// K to the dispatch width KT in {1, 2, 3, 4, 8, 16} with zeros.  A padded matrix has the identity in its padded rows and columns,
// so a padded unknown has a zero right-hand side, never enters the passive set and stays +0.
//
// One iteration is two sweeps of the packed panel in the geometry of admix.hip, each followed by a batched NNLS solve:
//   G right-hand sides  a workgroup per tile of 32 loci of L walks all individuals (Q rows staged through LDS, 128 at a time);
//                       a row entity keeps three class sums of KT doubles.
//   Q right-hand sides  a workgroup per (32 individuals of T, chunk of TPG_ADMIX_CHUNK_LOCI loci); the 3 KT doubles of each of
//                       the block's 128 loci are staged in LDS; partials to part[chunk][i][k], added in ascending chunk order.
//   NNLS                one thread per locus (its three systems, normalisation fused) or per individual.  Lawson-Hanson on the
//                       normal equations with a KT-bit passive mask; an inner solve is a fully unrolled KT x KT Cholesky of the
//                       masked matrix (identity rows for the inactive k: every index is a compile-time constant) and one step of
//                       iterative refinement.  The shared matrix sits in LDS; all lanes read the same address: a broadcast.
//   Gram matrices       Q'Q and GG': per tile of TPG_SNMF_GRAM_ROWS rows (thread (g, e) takes entry e = (k, l) over the rows
//                       g, g + GP, ..; the GP groups in order), then the tiles by a one-workgroup kernel of the same shape.
// Every sum has a fixed shape; the only atomics are integer (the validation flag, the counts of entries and of unsolved systems).
#include "admix_common.h"
#include "host/host_nnls.h"

namespace {

constexpr int SNMF_GRAM_ROWS = TPG_SNMF_GRAM_ROWS;

int snmf_kt(int K) { return K <= 4 ? K : K <= 8 ? 8 : 16; }

#define SNMF_DISPATCH(kt, CALL) \
  switch (kt) {                 \
    case 1: CALL(1); break;     \
    case 2: CALL(2); break;     \
    case 3: CALL(3); break;     \
    case 4: CALL(4); break;     \
    case 8: CALL(8); break;     \
    default: CALL(16); break;   \
  }

// ---- the two sweeps ----------------------------------------------------------------------------------------------------
// rhs[(3 j + c) KT + k] = sum over the individuals with g(i, j) = c of Qd[i KT + k]
template <int KT>
__global__ __launch_bounds__(256) void snmf_g_rhs_kernel(const uint32_t* __restrict__ L, int64_t Qb, int64_t n, int64_t m,
                                                         const double* __restrict__ Qd, double* __restrict__ rhs) {
  __shared__ double stage[128 * KT];  // the reduction needs 96 KT of it
  __shared__ int cnts[32];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int64_t lt = blockIdx.x, j = lt * 32 + r;
  double acc[3 * KT];
#pragma unroll
  for (int v = 0; v < 3 * KT; v++) acc[v] = 0.0;
  int cnt = 0;
  for (int64_t q = 0; q < Qb; q++) {
    __syncthreads();
    admix_stage<KT>(stage, Qd, q, n, 0.0);
    __syncthreads();
    const uint32_t wd = L[((lt * Qb + q) * 64 + lane) * 4 + w];
#pragma unroll 2
    for (int e = 0; e < 16; e++) {
      const int g = admix_code(wd, e);
      if (g == 3) continue;
      const double* __restrict__ qs = stage + (32 * w + 16 * h + e) * KT;
      if (g == 0) {
#pragma unroll
        for (int k = 0; k < KT; k++) acc[k] += qs[k];
      } else if (g == 1) {
#pragma unroll
        for (int k = 0; k < KT; k++) acc[KT + k] += qs[k];
      } else {
#pragma unroll
        for (int k = 0; k < KT; k++) acc[2 * KT + k] += qs[k];
      }
    }
  }
#pragma unroll
  for (int v = 0; v < 3 * KT; v++) acc[v] += __shfl_xor(acc[v], 32);
  admix_wave_order_sum<3 * KT>(acc, cnt, stage, cnts, w, r, h);
  if (w != 0 || h != 0 || j >= m) return;
#pragma unroll
  for (int v = 0; v < 3 * KT; v++) rhs[j * 3 * KT + v] = acc[v];
}

// workgroup (rt, c) = 32 individuals x one chunk of loci -> part[(c n + i) KT + k] = sum over the chunk's typed loci of
// Gd[(3 j + g(i, j)) KT + k], cpart[c n + i] = their number
template <int KT>
__global__ __launch_bounds__(256) void snmf_q_rhs_kernel(const uint32_t* __restrict__ T, int64_t KG, int64_t n, int64_t m,
                                                         const double* __restrict__ Gd, double* __restrict__ part,
                                                         int32_t* __restrict__ cpart) {
  __shared__ double stage[128 * 3 * KT];
  __shared__ int cnts[32];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int64_t rt = blockIdx.x, c = blockIdx.y, i = rt * 32 + r;
  double S[KT];
#pragma unroll
  for (int k = 0; k < KT; k++) S[k] = 0.0;
  int cnt = 0;
  const int64_t kg0 = c * (ADM_CHUNK / 128), kg1 = kg0 + ADM_CHUNK / 128 < KG ? kg0 + ADM_CHUNK / 128 : KG;
  for (int64_t kg = kg0; kg < kg1; kg++) {
    __syncthreads();
    const int64_t j0 = kg * 128;
    for (int idx = threadIdx.x; idx < 128 * 3 * KT; idx += 256) stage[idx] = j0 + idx / (3 * KT) < m ? Gd[j0 * 3 * KT + idx] : 0.0;
    __syncthreads();
    const uint32_t wd = T[((rt * KG + kg) * 64 + lane) * 4 + w];
#pragma unroll 2
    for (int e = 0; e < 16; e++) {
      const int g = admix_code(wd, e);
      if (g == 3) continue;
      const double* __restrict__ gs = stage + ((32 * w + 16 * h + e) * 3 + g) * KT;
#pragma unroll
      for (int k = 0; k < KT; k++) S[k] += gs[k];
      cnt++;
    }
  }
#pragma unroll
  for (int k = 0; k < KT; k++) S[k] += __shfl_xor(S[k], 32);
  cnt += __shfl_xor(cnt, 32);
  admix_wave_order_sum<KT>(S, cnt, stage, cnts, w, r, h);
  if (w != 0 || h != 0 || i >= n) return;
  const int64_t o = c * n + i;
#pragma unroll
  for (int k = 0; k < KT; k++) part[o * KT + k] = S[k];
  cpart[o] = cnt;
}

// the chunks' partials in ascending order -> rhs[i KT + k], typed[i]
__global__ void snmf_q_combine_kernel(const double* __restrict__ part, const int32_t* __restrict__ cpart, int64_t nchunks, int64_t n,
                                      int KT, double* __restrict__ rhs, int64_t* __restrict__ typed) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * KT) return;
  const int64_t i = idx / KT;
  const int k = (int)(idx % KT);
  double s = 0.0;
  int64_t t = 0;
  for (int64_t c = 0; c < nchunks; c++) {
    s += part[(c * n + i) * KT + k];
    t += cpart[c * n + i];
  }
  rhs[idx] = s;
  if (k == 0) typed[i] = t;
}

// ---- NNLS: the solver itself is host/host_nnls.h (one thread per system; also built for the host by tests/host/nnls_san.cpp) ----
__device__ __forceinline__ void snmf_count_unsolved(int bad, unsigned long long* __restrict__ unsolved) {
  bad = tpg_wave_sum(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(unsolved, (unsigned long long)bad);
}

template <int KT>
__device__ __forceinline__ void snmf_load_matrix(double* __restrict__ As, const double* __restrict__ Amat) {
  for (int idx = threadIdx.x; idx < KT * KT; idx += 64) As[idx] = Amat[idx];
  __syncthreads();
}

// G step: thread j solves the three systems of locus j and normalises over the classes
template <int KT>
__global__ __launch_bounds__(64) void snmf_nnls_g_kernel(const double* __restrict__ Amat, const double* __restrict__ rhs, int64_t m, int K,
                                                         double* Gd, unsigned long long* __restrict__ unsolved) {
  __shared__ double As[KT * KT];
  snmf_load_matrix<KT>(As, Amat);
  const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
  int bad = 0;
  if (j < m) {
    double* g = Gd + j * 3 * KT;
    for (int c = 0; c < 3; c++) {
      double b[KT], x[KT];
#pragma unroll
      for (int k = 0; k < KT; k++) b[k] = rhs[(j * 3 + c) * KT + k];
      bad += !snmf_nnls<KT>(As, b, x);
#pragma unroll
      for (int k = 0; k < KT; k++) g[c * KT + k] = x[k];
    }
#pragma unroll
    for (int k = 0; k < KT; k++) {
      const double g0 = g[k], g1 = g[KT + k], g2 = g[2 * KT + k];
      const double s = (g0 + g1) + g2;
      const bool live = s > TPG_SNMF_TINY;
      const double third = k < K ? 1.0 / 3.0 : 0.0;
      g[k] = live ? g0 / s : third;
      g[KT + k] = live ? g1 / s : third;
      g[2 * KT + k] = live ? g2 / s : third;
    }
  }
  snmf_count_unsolved(bad, unsolved);
}

// Q step: thread i solves the system of individual i and normalises the row; qb[i] = Q'(i, .) . b_i
template <int KT>
__global__ __launch_bounds__(64) void snmf_nnls_q_kernel(const double* __restrict__ Bmat, const double* __restrict__ rhs, int64_t n, int K,
                                                         double* __restrict__ Qn, double* __restrict__ qb,
                                                         unsigned long long* __restrict__ unsolved) {
  __shared__ double As[KT * KT];
  snmf_load_matrix<KT>(As, Bmat);
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  int bad = 0;
  if (i < n) {
    double b[KT], x[KT];
#pragma unroll
    for (int k = 0; k < KT; k++) b[k] = rhs[i * KT + k];
    bad = !snmf_nnls<KT>(As, b, x);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < KT; k++) s += x[k];
    const bool live = s > TPG_SNMF_TINY;
    double dot = 0.0;
#pragma unroll
    for (int k = 0; k < KT; k++) {
      const double q = live ? x[k] / s : k < K ? 1.0 / (double)K : 0.0;
      Qn[i * KT + k] = q;
      dot = fma(q, b[k], dot);
    }
    qb[i] = dot;
  }
  snmf_count_unsolved(bad, unsolved);
}

// the solver on its own: B and X nrhs x K column-major
template <int KT>
__global__ __launch_bounds__(64) void snmf_nnls_plain_kernel(const double* __restrict__ Amat, const double* __restrict__ B, int64_t nrhs,
                                                             int K, double* __restrict__ X, unsigned long long* __restrict__ unsolved) {
  __shared__ double As[KT * KT];
  snmf_load_matrix<KT>(As, Amat);
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  int bad = 0;
  if (i < nrhs) {
    double b[KT], x[KT];
#pragma unroll
    for (int k = 0; k < KT; k++) b[k] = k < K ? B[i + (int64_t)k * nrhs] : 0.0;
    bad = !snmf_nnls<KT>(As, b, x);
#pragma unroll
    for (int k = 0; k < KT; k++)
      if (k < K) X[i + (int64_t)k * nrhs] = x[k];
  }
  snmf_count_unsolved(bad, unsolved);
}

// ---- the small matrices and the criterion ------------------------------------------------------------------------------
// part[tile KT^2 + e] = sum over the tile's rows of X[row KT + k] X[row KT + l], e = k KT + l: thread (g, e) adds the rows g, g + GP, ..
// in ascending order with one fused multiply-add each, then the GP groups in ascending order
template <int KT>
__global__ __launch_bounds__(256) void snmf_gram_part_kernel(const double* __restrict__ X, int64_t rows, double* __restrict__ part) {
  constexpr int E = KT * KT, GP = 256 / E;
  __shared__ double st[SNMF_GRAM_ROWS * KT];
  __shared__ double red[256];
  const int64_t r0 = (int64_t)blockIdx.x * SNMF_GRAM_ROWS;
  for (int idx = threadIdx.x; idx < SNMF_GRAM_ROWS * KT; idx += 256) st[idx] = r0 + idx / KT < rows ? X[r0 * KT + idx] : 0.0;
  __syncthreads();
  const int t = threadIdx.x, e = t % E, grp = t / E, k = e / KT, l = e % KT;
  double s = 0.0;
  if (grp < GP)
    for (int row = grp; row < SNMF_GRAM_ROWS; row += GP) s = fma(st[row * KT + k], st[row * KT + l], s);
  red[t] = s;
  __syncthreads();
  if (t < E) {
    double a = red[t];
    for (int g = 1; g < GP; g++) a += red[g * E + t];
    part[(int64_t)blockIdx.x * E + t] = a;
  }
}

// the tiles' partials: thread (g, e) adds the tiles g, g + GP, .. in ascending order, then the groups in ascending order
__global__ __launch_bounds__(256) void snmf_gram_sum_kernel(const double* __restrict__ part, int64_t ntiles, int E, double* __restrict__ out) {
  __shared__ double red[256];
  const int GP = 256 / E, t = threadIdx.x, e = t % E, grp = t / E;
  double s = 0.0;
  if (grp < GP)
    for (int64_t tile = grp; tile < ntiles; tile += GP) s += part[tile * E + e];
  red[t] = s;
  __syncthreads();
  if (t < E) {
    double a = red[t];
    for (int g = 1; g < GP; g++) a += red[g * E + t];
    out[t] = a;
  }
}

// out = ridge(gram + alpha 1 1') of include/tpg.h on the K x K corner, the identity in the padding
__global__ void snmf_ridge_kernel(const double* __restrict__ gram, int K, int KT, double alpha, double* __restrict__ out) {
  const int t = threadIdx.x;
  if (t >= KT * KT) return;
  const int k = t / KT, l = t % KT;
  double tr = 0.0;
  for (int d = 0; d < K; d++) tr += gram[d * KT + d] + alpha;
  const double rho = (TPG_SNMF_RIDGE * tr) / (double)K;
  double x = k == l ? 1.0 : 0.0;
  if (k < K && l < K) {
    x = gram[t] + alpha;
    if (k == l) x += rho;
  }
  out[t] = x;
}

// a user's K x K matrix into the padded form, as given
__global__ void snmf_pad_matrix_kernel(const double* __restrict__ A, int K, int KT, double* __restrict__ out) {
  const int t = threadIdx.x;
  if (t >= KT * KT) return;
  const int k = t / KT, l = t % KT;
  out[t] = k < K && l < K ? A[k + l * K] : k == l ? 1.0 : 0.0;
}

// sum_i qb[i] in the shape of admix_ll_sum_kernel, sum_i typed[i], and ls = T - 2 sum_i qb + sum_kl gq(k, l) gg(k, l)
__global__ __launch_bounds__(256) void snmf_ls_kernel(const double* __restrict__ qb, const int64_t* __restrict__ typed, int64_t n,
                                                      const double* __restrict__ gq, const double* __restrict__ gg, int KT,
                                                      double* __restrict__ out) {
  __shared__ double wq[4];
  __shared__ long long wt[4];
  double s = 0.0;
  long long t = 0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    s += qb[i];
    t += typed[i];
  }
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    t += __shfl_xor(t, o);
  }
  if ((threadIdx.x & 63) == 0) {
    wq[threadIdx.x >> 6] = s;
    wt[threadIdx.x >> 6] = t;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double sqb = ((wq[0] + wq[1]) + wq[2]) + wq[3];
  const long long T = wt[0] + wt[1] + wt[2] + wt[3];
  double dot = 0.0;
  for (int e = 0; e < KT * KT; e++) dot = fma(gq[e], gg[e], dot);
  *out = ((double)T - 2.0 * sqb) + dot;
}

// G = 1/3 everywhere (max_iter = 0), 0 in the padding
__global__ void snmf_fill_g_kernel(double* __restrict__ Gd, int64_t rows, int K, int KT) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * KT) return;
  Gd[idx] = idx % KT < K ? 1.0 / 3.0 : 0.0;
}

// P[j + k m] = G(j, 1, k) / 2 + G(j, 2, k)
__global__ void snmf_store_p_kernel(const double* __restrict__ Gd, int64_t m, int K, int KT, double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m * K) return;
  const int64_t j = idx % m, k = idx / m;
  out[idx] = Gd[(j * 3 + 1) * KT + k] / 2.0 + Gd[(j * 3 + 2) * KT + k];
}

// ---- host side ---------------------------------------------------------------------------------------------------------
int snmf_check_k(int K) {
  TPG_REQUIRE(K >= 1 && K <= TPG_SNMF_MAX_K, TPG_EINVAL, "K = %d out of [1, %d]", K, TPG_SNMF_MAX_K);
  return TPG_OK;
}

int snmf_check_view(const tpg_view* v, int K) {
  TPG_TRY(snmf_check_k(K));
  TPG_REQUIRE(v->n > 0 && v->m > 0, TPG_EINVAL, "sNMF needs at least one individual and one locus (view of %lld x %lld)", (long long)v->n,
              (long long)v->m);
  return TPG_OK;
}

struct SnmfRun {
  tpg_ctx* ctx;
  const tpg_view* v;
  int K, KT;
  int64_t n, m, n_lt, n_rt, nchunks, tiles_q, tiles_g;
  DevArena sc;
  double *Q[2] = {}, *G = nullptr, *rhs_g = nullptr, *rhs_q = nullptr, *part = nullptr, *gpart = nullptr, *qb = nullptr;
  double *gram_q = nullptr, *gram_g = nullptr, *A = nullptr, *B = nullptr, *trace = nullptr;
  int64_t* typed = nullptr;
  int32_t *cpart = nullptr, *flag = nullptr;
  unsigned long long* unsolved = nullptr;

  // sweeps = false: the state and the small things only (the start, the cross-entropy sums)
  int init(tpg_ctx* c, const tpg_view* view, int k, bool sweeps, int64_t trace_len) {
    ctx = c; v = view; K = k; KT = snmf_kt(k);
    n = v->n; m = v->m;
    TPG_TRY(tpg_view_need_L(ctx, v));
    n_lt = ceil_div(m, 32); n_rt = ceil_div(n, 32); nchunks = ceil_div(m, ADM_CHUNK);
    tiles_q = ceil_div(n, SNMF_GRAM_ROWS); tiles_g = ceil_div(3 * m, SNMF_GRAM_ROWS);
    TPG_REQUIRE(n_lt <= 0x7FFFFFFF && n_rt <= 0x7FFFFFFF && nchunks <= 65535 && tiles_g <= 0x7FFFFFFF, TPG_EUNSUPPORTED,
                "sNMF on a view of %lld x %lld", (long long)n, (long long)m);
    TPG_TRY(sc.get(&Q[0], (size_t)n * KT));
    TPG_TRY(sc.get(&G, (size_t)3 * m * KT));
    TPG_TRY(sc.get(&trace, (size_t)(trace_len > 0 ? trace_len : 1)));
    TPG_TRY(sc.get(&flag, (size_t)1));
    TPG_TRY(sc.get(&unsolved, (size_t)1));
    TPG_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), ctx->stream));
    TPG_HIP(hipMemsetAsync(unsolved, 0, sizeof(unsigned long long), ctx->stream));
    if (!sweeps) return TPG_OK;
    TPG_TRY(tpg_view_need_T(ctx, v));
    TPG_TRY(sc.get(&Q[1], (size_t)n * KT));
    TPG_TRY(sc.get(&rhs_g, (size_t)3 * m * KT));
    TPG_TRY(sc.get(&rhs_q, (size_t)n * KT));
    TPG_TRY(sc.get(&part, (size_t)nchunks * n * KT));
    TPG_TRY(sc.get(&cpart, (size_t)nchunks * n));
    TPG_TRY(sc.get(&typed, (size_t)n));
    TPG_TRY(sc.get(&qb, (size_t)n));
    TPG_TRY(sc.get(&gpart, (size_t)(tiles_g > tiles_q ? tiles_g : tiles_q) * KT * KT));
    TPG_TRY(sc.get(&gram_q, (size_t)KT * KT));
    TPG_TRY(sc.get(&gram_g, (size_t)KT * KT));
    TPG_TRY(sc.get(&A, (size_t)KT * KT));
    TPG_TRY(sc.get(&B, (size_t)KT * KT));
    return TPG_OK;
  }

  int gram(const double* X, int64_t rows, int64_t tiles, double* out) {
#define SNMF_GRAM(KT_) \
  TPG_LAUNCH(ctx, "snmf_gram", snmf_gram_part_kernel<KT_>, dim3((unsigned)tiles), dim3(256), 0, X, rows, gpart)
    SNMF_DISPATCH(KT, SNMF_GRAM);
#undef SNMF_GRAM
    TPG_LAUNCH(ctx, "snmf_gram_sum", snmf_gram_sum_kernel, dim3(1), dim3(256), 0, (const double*)gpart, tiles, KT * KT, out);
    return TPG_OK;
  }

  // (G, Q[1 - cur]) from Q[cur]; ls of the new pair -> trace[slot]
  int step(int cur, double alpha, int64_t slot) {
    const double *Qc = Q[cur], *Gc = G;
    double* Qn = Q[1 - cur];
    TPG_TRY(gram(Qc, n, tiles_q, gram_q));
    TPG_LAUNCH(ctx, "snmf_ridge", snmf_ridge_kernel, dim3(1), dim3(256), 0, (const double*)gram_q, K, KT, 0.0, A);
#define SNMF_G(KT_)                                                                                                             \
  do {                                                                                                                          \
    TPG_LAUNCH(ctx, "snmf_g_rhs", snmf_g_rhs_kernel<KT_>, dim3((unsigned)n_lt), dim3(256), 0, (const uint32_t*)v->L, v->Q, n, m, \
               Qc, rhs_g);                                                                                                      \
    TPG_LAUNCH(ctx, "snmf_nnls_g", snmf_nnls_g_kernel<KT_>, dim3((unsigned)ceil_div(m, 64)), dim3(64), 0, (const double*)A,      \
               (const double*)rhs_g, m, K, G, unsolved);                                                                        \
  } while (0)
    SNMF_DISPATCH(KT, SNMF_G);
#undef SNMF_G
    TPG_TRY(gram(Gc, 3 * m, tiles_g, gram_g));
    TPG_LAUNCH(ctx, "snmf_ridge", snmf_ridge_kernel, dim3(1), dim3(256), 0, (const double*)gram_g, K, KT, alpha, B);
#define SNMF_Q(KT_)                                                                                                                 \
  do {                                                                                                                              \
    TPG_LAUNCH(ctx, "snmf_q_rhs", snmf_q_rhs_kernel<KT_>, dim3((unsigned)n_rt, (unsigned)nchunks), dim3(256), 0,                     \
               (const uint32_t*)v->T, v->KG, n, m, Gc, part, cpart);                                                                \
    TPG_LAUNCH(ctx, "snmf_q_combine", snmf_q_combine_kernel, dim3((unsigned)ceil_div(n * KT, 256)), dim3(256), 0, (const double*)part, \
               (const int32_t*)cpart, nchunks, n, KT, rhs_q, typed);                                                                \
    TPG_LAUNCH(ctx, "snmf_nnls_q", snmf_nnls_q_kernel<KT_>, dim3((unsigned)ceil_div(n, 64)), dim3(64), 0, (const double*)B,          \
               (const double*)rhs_q, n, K, Qn, qb, unsolved);                                                                       \
  } while (0)
    SNMF_DISPATCH(KT, SNMF_Q);
#undef SNMF_Q
    TPG_TRY(gram(Qn, n, tiles_q, gram_q));
    TPG_LAUNCH(ctx, "snmf_ls", snmf_ls_kernel, dim3(1), dim3(256), 0, (const double*)qb, (const int64_t*)typed, n, (const double*)gram_q,
               (const double*)gram_g, KT, trace + slot);
    TPG_CHECK_LAUNCH();
    return TPG_OK;
  }

  int fetch_unsolved(int64_t* out) {
    unsigned long long u = 0;
    TPG_HIP(tpg_fetch_small(ctx, &u, unsolved, sizeof u));
    *out = (int64_t)u;
    return TPG_OK;
  }
};

// the state's Q, G and P into the caller's buffers (G and P may be NULL); nothing is committed before every kernel is done
int snmf_store(SnmfRun& run, const double* Qd, double* Q, double* G, double* P) {
  tpg_ctx* ctx = run.ctx;
  const int64_t n = run.n, m = run.m;
  const int K = run.K, KT = run.KT;
  OutBuf oq, og, op;
  TPG_TRY(oq.init(Q, sizeof(double) * (size_t)n * K));
  if (G) TPG_TRY(og.init(G, sizeof(double) * (size_t)3 * m * K));
  if (P) TPG_TRY(op.init(P, sizeof(double) * (size_t)m * K));
  TPG_LAUNCH(ctx, "snmf_store", admix_store_kernel, dim3((unsigned)ceil_div(n * K, 256)), dim3(256), 0, Qd, n, K, KT, oq.dev<double>());
  if (G)
    TPG_LAUNCH(ctx, "snmf_store", admix_store_kernel, dim3((unsigned)ceil_div(3 * m * K, 256)), dim3(256), 0, (const double*)run.G, 3 * m,
               K, KT, og.dev<double>());
  if (P)
    TPG_LAUNCH(ctx, "snmf_store", snmf_store_p_kernel, dim3((unsigned)ceil_div(m * K, 256)), dim3(256), 0, (const double*)run.G, m, K, KT,
               op.dev<double>());
  TPG_CHECK_LAUNCH();
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  TPG_TRY(oq.commit(ctx));
  if (G) TPG_TRY(og.commit(ctx));
  if (P) TPG_TRY(op.commit(ctx));
  return TPG_OK;
}

}  // namespace

extern "C" int tpg_snmf(tpg_ctx* ctx, const tpg_view* v, const double* ploidy, int K, int max_iter, double tol, double alpha,
                        uint64_t seed, const double* q0, double* Q, double* G, double* P, double* ls, double* ls_trace, int* n_iter,
                        int* converged, int64_t* n_unsolved) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && Q, TPG_EINVAL, "null argument");
  TPG_TRY(snmf_check_view(v, K));
  TPG_REQUIRE(max_iter >= 0, TPG_EINVAL, "max_iter = %d is negative", max_iter);
  TPG_REQUIRE(tol >= 0.0, TPG_EINVAL, "tol must be a non-negative number");  // false for a NaN too
  TPG_REQUIRE(alpha >= 0.0 && alpha <= 1.79769313486231570815e308, TPG_EINVAL, "alpha must be a finite non-negative number");
  TPG_TRY(tpg_require_diploid(v->n, ploidy, "sNMF"));
  const int64_t n = v->n, m = v->m;
  SnmfRun run;
  TPG_TRY(run.init(ctx, v, K, max_iter > 0, max_iter));
  const int KT = run.KT;
  const unsigned gn = (unsigned)ceil_div(n, 256);
  InBuf iq;
  if (q0) {
    TPG_TRY(iq.init(ctx, q0, sizeof(double) * (size_t)n * K));
    TPG_LAUNCH(ctx, "snmf_start", admix_load_q_kernel, dim3(gn), dim3(256), 0, iq.dev<double>(), run.Q[0], n, K, KT, true, run.flag);
    TPG_CHECK_LAUNCH();
    int32_t bad = 0;
    TPG_HIP(tpg_fetch_small(ctx, &bad, run.flag, sizeof bad));
    TPG_REQUIRE(!(bad & 1), TPG_EINVAL, "q0 has an entry that is not finite or not positive");
  } else {
    TPG_LAUNCH(ctx, "snmf_start", admix_seed_q_kernel, dim3(gn), dim3(256), 0, run.Q[0], n, K, KT, seed);
  }
  if (max_iter == 0)
    TPG_LAUNCH(ctx, "snmf_start", snmf_fill_g_kernel, dim3((unsigned)ceil_div(3 * m * KT, 256)), dim3(256), 0, run.G, 3 * m, K, KT);
  TPG_CHECK_LAUNCH();
  std::vector<double> lsv((size_t)max_iter + 1, nan(""));
  int cq = 0, t = 0, conv = 0;
  while (t < max_iter) {
    TPG_TRY(run.step(cq, alpha, t));
    TPG_HIP(tpg_fetch_small(ctx, &lsv[(size_t)t], run.trace + t, sizeof(double)));
    cq = 1 - cq;
    t++;
    if (t >= 2 && fabs(lsv[(size_t)t - 2] - lsv[(size_t)t - 1]) <= tol * lsv[(size_t)t - 2]) {
      conv = 1;
      break;
    }
  }
  int64_t uns = 0;
  TPG_TRY(run.fetch_unsolved(&uns));
  // nothing of the caller's has been written so far
  TPG_TRY(snmf_store(run, run.Q[cq], Q, G, P));
  if (ls) *ls = t > 0 ? lsv[(size_t)t - 1] : nan("");
  if (ls_trace)
    for (int s = 0; s < t; s++) ls_trace[s] = lsv[(size_t)s];
  if (n_iter) *n_iter = t;
  if (converged) *converged = conv;
  if (n_unsolved) *n_unsolved = uns;
  return TPG_OK;
}

extern "C" int tpg_snmf_step(tpg_ctx* ctx, const tpg_view* v, int K, double alpha, const double* Q_in, double* Q_out, double* G_out,
                             double* ls, int64_t* n_unsolved) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && Q_in && Q_out, TPG_EINVAL, "null argument");
  TPG_TRY(snmf_check_view(v, K));
  TPG_REQUIRE(alpha >= 0.0 && alpha <= 1.79769313486231570815e308, TPG_EINVAL, "alpha must be a finite non-negative number");
  const int64_t n = v->n;
  SnmfRun run;
  TPG_TRY(run.init(ctx, v, K, true, 1));
  InBuf iq;
  TPG_TRY(iq.init(ctx, Q_in, sizeof(double) * (size_t)n * K));
  TPG_LAUNCH(ctx, "snmf_start", admix_load_q_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, iq.dev<double>(), run.Q[0], n, K,
             run.KT, false, run.flag);
  TPG_TRY(run.step(0, alpha, 0));
  double l = 0.0;
  int64_t uns = 0;
  TPG_HIP(tpg_fetch_small(ctx, &l, run.trace, sizeof l));
  TPG_TRY(run.fetch_unsolved(&uns));
  TPG_TRY(snmf_store(run, run.Q[1], Q_out, G_out, nullptr));
  if (ls) *ls = l;
  if (n_unsolved) *n_unsolved = uns;
  return TPG_OK;
}

extern "C" int tpg_nnls_shared(tpg_ctx* ctx, int K, const double* A, const double* B, int64_t nrhs, double* X, int64_t* n_unsolved) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && A && B && X, TPG_EINVAL, "null argument");
  TPG_TRY(snmf_check_k(K));
  TPG_REQUIRE(nrhs >= 0 && ceil_div(nrhs, 64) <= 0x7FFFFFFF, TPG_EINVAL, "nrhs = %lld", (long long)nrhs);
  const int KT = snmf_kt(K);
  DevArena sc;
  double* Ad = nullptr;
  unsigned long long* d_uns = nullptr;
  TPG_TRY(sc.get(&Ad, (size_t)KT * KT));
  TPG_TRY(sc.get(&d_uns, (size_t)1));
  TPG_HIP(hipMemsetAsync(d_uns, 0, sizeof(unsigned long long), ctx->stream));
  InBuf ia, ib;
  OutBuf ox;
  TPG_TRY(ia.init(ctx, A, sizeof(double) * (size_t)K * K));
  TPG_TRY(ib.init(ctx, B, sizeof(double) * (size_t)nrhs * K));
  TPG_TRY(ox.init(X, sizeof(double) * (size_t)nrhs * K));
  TPG_LAUNCH(ctx, "snmf_start", snmf_pad_matrix_kernel, dim3(1), dim3(256), 0, ia.dev<double>(), K, KT, Ad);
  if (nrhs > 0) {
#define SNMF_N(KT_)                                                                                                              \
  TPG_LAUNCH(ctx, "snmf_nnls", snmf_nnls_plain_kernel<KT_>, dim3((unsigned)ceil_div(nrhs, 64)), dim3(64), 0, (const double*)Ad,   \
             ib.dev<double>(), nrhs, K, ox.dev<double>(), d_uns)
    SNMF_DISPATCH(KT, SNMF_N);
#undef SNMF_N
  }
  TPG_CHECK_LAUNCH();
  unsigned long long u = 0;
  TPG_HIP(tpg_fetch_small(ctx, &u, d_uns, sizeof u));
  TPG_TRY(ox.commit(ctx));
  if (n_unsolved) *n_unsolved = (int64_t)u;
  return TPG_OK;
}

// ---- hold-out by fraction and the cross-entropy (include/tpg.h "sNMF") ---------------------------------------------------------
// The view is admix_common.h's hold-out with the high half of the hash against a threshold instead of a fold.  The sweep is a
// sibling of admix_holdout_sweep_kernel (admix.hip): the same geometry, the same sum shapes; it decodes both planes and adds
// -ln max(p, floor) to one of two sums: typed in `train`, or typed in `full` alone.
namespace {

// one workgroup per tile of 32 loci.  part_m[lt] / part_a[lt] = the tile's share of the masked / all sum; d_cnt[0] / d_cnt[1] += the
// number of their entries
template <int KT>
__global__ __launch_bounds__(256) void snmf_ce_sweep_kernel(const uint32_t* __restrict__ Lf, const uint32_t* __restrict__ Lt, int64_t Qb,
                                                            int64_t n, int64_t m, const double* __restrict__ Qd,
                                                            const double* __restrict__ Gd, double* __restrict__ part_m,
                                                            double* __restrict__ part_a, unsigned long long* __restrict__ d_cnt) {
  __shared__ double stage[128 * KT];
  __shared__ double wl[2][4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int64_t lt = blockIdx.x, j = lt * 32 + r;
  double g[3 * KT];
#pragma unroll
  for (int v = 0; v < 3 * KT; v++) g[v] = j < m ? Gd[j * 3 * KT + v] : 0.0;
  double sm = 0.0, sa = 0.0;
  int cm = 0, ca = 0;
  for (int64_t q = 0; q < Qb; q++) {
    __syncthreads();
    admix_stage<KT>(stage, Qd, q, n, 0.0);
    __syncthreads();
    const int64_t at = ((lt * Qb + q) * 64 + lane) * 4 + w;
    const uint32_t wf = Lf[at], wt = Lt[at];
#pragma unroll 2
    for (int e = 0; e < 16; e++) {
      const int gt = admix_code(wt, e), gf = admix_code(wf, e);
      const int gg = gt != 3 ? gt : gf;
      if (gg == 3) continue;
      const double* __restrict__ qs = stage + (32 * w + 16 * h + e) * KT;
      double p = 0.0;
#pragma unroll
      for (int k = 0; k < KT; k++) p = fma(qs[k], gg == 0 ? g[k] : gg == 1 ? g[KT + k] : g[2 * KT + k], p);
      const double term = -log(fmax(p, TPG_SNMF_P_FLOOR));
      if (gt != 3) {
        sa += term;
        ca++;
      } else {
        sm += term;
        cm++;
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    sm += __shfl_xor(sm, o);
    sa += __shfl_xor(sa, o);
    cm += __shfl_xor(cm, o);
    ca += __shfl_xor(ca, o);
  }
  if (lane == 0) {
    wl[0][w] = sm;
    wl[1][w] = sa;
    if (cm) atomicAdd(d_cnt, (unsigned long long)cm);
    if (ca) atomicAdd(d_cnt + 1, (unsigned long long)ca);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part_m[lt] = ((wl[0][0] + wl[0][1]) + wl[0][2]) + wl[0][3];
    part_a[lt] = ((wl[1][0] + wl[1][1]) + wl[1][2]) + wl[1][3];
  }
}

// G (3M x K column-major) -> Gd, as given
__global__ void snmf_load_g_kernel(const double* __restrict__ G, double* __restrict__ Gd, int64_t rows, int K, int KT) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * KT) return;
  const int64_t row = idx / KT;
  const int k = (int)(idx % KT);
  Gd[idx] = k < K ? G[row + (int64_t)k * rows] : 0.0;
}

}  // namespace

extern "C" int tpg_view_holdout_fraction(tpg_ctx* ctx, const tpg_view* full, double fraction, uint64_t seed, tpg_view** out,
                                         int64_t* n_held) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && full && out, TPG_EINVAL, "null argument");
  TPG_REQUIRE(fraction > 0.0 && fraction < 1.0, TPG_EINVAL, "fraction = %g out of (0, 1)", fraction);
  const uint64_t thr = (uint64_t)floor(fraction * 4294967296.0);
  return admix_holdout_view<HoldoutBelow>(ctx, "snmf_holdout_view", full, seed, out, true, n_held, thr);
}

extern "C" int tpg_snmf_cross_entropy_sums(tpg_ctx* ctx, const tpg_view* full, const tpg_view* train, int K, const double* Q,
                                           const double* G, double* sum_masked, int64_t* n_masked, double* sum_all, int64_t* n_all) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && full && train && Q && G, TPG_EINVAL, "null argument");
  TPG_TRY(snmf_check_view(full, K));
  TPG_REQUIRE(full->n == train->n && full->m == train->m, TPG_EINVAL, "the full view is %lld x %lld, the training view %lld x %lld",
              (long long)full->n, (long long)full->m, (long long)train->n, (long long)train->m);
  TPG_TRY(tpg_view_need_L(ctx, full));
  TPG_TRY(tpg_view_need_L(ctx, train));
  const int64_t n = full->n, m = full->m;
  SnmfRun run;
  TPG_TRY(run.init(ctx, full, K, false, 2));
  const int KT = run.KT;
  unsigned long long* d_cnt = nullptr;
  double *part_m = nullptr, *part_a = nullptr;
  TPG_TRY(run.sc.get(&d_cnt, (size_t)2));
  TPG_TRY(run.sc.get(&part_m, (size_t)run.n_lt));
  TPG_TRY(run.sc.get(&part_a, (size_t)run.n_lt));
  TPG_HIP(hipMemsetAsync(d_cnt, 0, 2 * sizeof(unsigned long long), ctx->stream));
  InBuf iq, ig;
  TPG_TRY(iq.init(ctx, Q, sizeof(double) * (size_t)n * K));
  TPG_TRY(ig.init(ctx, G, sizeof(double) * (size_t)3 * m * K));
  TPG_LAUNCH(ctx, "snmf_start", admix_load_q_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, iq.dev<double>(), run.Q[0], n, K, KT,
             false, run.flag);
  TPG_LAUNCH(ctx, "snmf_start", snmf_load_g_kernel, dim3((unsigned)ceil_div(3 * m * KT, 256)), dim3(256), 0, ig.dev<double>(), run.G, 3 * m,
             K, KT);
#define SNMF_CE(KT_)                                                                                                              \
  TPG_LAUNCH(ctx, "snmf_ce_sweep", snmf_ce_sweep_kernel<KT_>, dim3((unsigned)run.n_lt), dim3(256), 0, (const uint32_t*)full->L,    \
             (const uint32_t*)train->L, full->Q, n, m, (const double*)run.Q[0], (const double*)run.G, part_m, part_a, d_cnt)
  SNMF_DISPATCH(KT, SNMF_CE);
#undef SNMF_CE
  TPG_LAUNCH(ctx, "snmf_ce_sum", admix_ll_sum_kernel, dim3(1), dim3(256), 0, (const double*)part_m, run.n_lt, run.trace);
  TPG_LAUNCH(ctx, "snmf_ce_sum", admix_ll_sum_kernel, dim3(1), dim3(256), 0, (const double*)part_a, run.n_lt, run.trace + 1);
  TPG_CHECK_LAUNCH();
  double s[2] = {0.0, 0.0};
  unsigned long long c[2] = {0, 0};
  TPG_HIP(tpg_fetch_small(ctx, s, run.trace, sizeof s));
  TPG_HIP(tpg_fetch_small(ctx, c, d_cnt, sizeof c));
  if (sum_masked) *sum_masked = s[0];
  if (n_masked) *n_masked = (int64_t)c[0];
  if (sum_all) *sum_all = s[1];
  if (n_all) *n_all = (int64_t)c[1];
  return TPG_OK;
}
