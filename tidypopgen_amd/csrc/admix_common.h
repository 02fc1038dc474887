// admix_common.h -- what the ancestry estimators share (admix.hip: the EM of "admixture"; snmf.hip: "sNMF"): the seeded start,
// the loading and storing of a padded state, the staging of state rows through LDS, the sums of fixed shape and the hash
// hold-out of a view (one kernel and one host routine, by fold or by fraction).  Included by those two files only; everything
// sits in their unnamed namespace.  The decoding of an element and the wave primitives are devfrag.h's.
#pragma once
#include "common.h"
#include "devfrag.h"
#include "synth_common.h"

#include <math.h>

namespace {

constexpr int ADM_CHUNK = TPG_ADMIX_CHUNK_LOCI;
static_assert(ADM_CHUNK % 128 == 0, "a chunk is whole blocks of T");
constexpr uint64_t ADM_F_SALT = 0xF0F0F0F0F0F0F0F0ull;

// u(h) of include/tpg.h: the addition rounds to nearest even once h >> 11 reaches 2^52, the same in every IEEE double
__host__ __device__ inline double admix_u(uint64_t h) { return ((double)(h >> 11) + 0.5) * 0x1p-53; }

__device__ __forceinline__ double admix_clamp(double f) {
  return f < TPG_ADMIX_EPS ? TPG_ADMIX_EPS : f > 1.0 - TPG_ADMIX_EPS ? 1.0 - TPG_ADMIX_EPS : f;
}
__device__ __forceinline__ bool admix_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }

// element e of a packed dword
__device__ __forceinline__ int admix_code(uint32_t w, int e) { return (int)((w >> tpg_elem_shift(e)) & 3u); }

// ---- start, validation, output ---------------------------------------------------------------------------------------
__global__ void admix_seed_q_kernel(double* __restrict__ Qd, int64_t n, int K, int KT, uint64_t seed) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = tpg_mix64(seed ^ tpg_mix64((uint64_t)i));
  double s = 0;
  for (int k = 0; k < K; k++) s += admix_u(tpg_mix64(key ^ tpg_mix64((uint64_t)k)));
  for (int k = 0; k < KT; k++) Qd[i * KT + k] = k < K ? admix_u(tpg_mix64(key ^ tpg_mix64((uint64_t)k))) / s : 0.0;
}

// q0 (n x K column-major) -> Qd, each row divided by its sum (ascending k); normalise = false: as given (tpg_admix_loglik).
// bit 0 of *flag: an entry that is not finite or not positive
__global__ void admix_load_q_kernel(const double* __restrict__ q0, double* __restrict__ Qd, int64_t n, int K, int KT, bool normalise,
                                    int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0;
  bool bad = false;
  for (int k = 0; k < K; k++) {
    const double x = q0[i + (int64_t)k * n];
    bad |= !(admix_finite(x) && x > 0.0);
    s += x;
  }
  if (normalise && bad) atomicOr(flag, 1);
  for (int k = 0; k < KT; k++) {
    const double x = k < K ? q0[i + (int64_t)k * n] : 0.0;
    Qd[i * KT + k] = normalise && k < K ? x / s : x;
  }
}

// rows x K column-major out of the padded state
__global__ void admix_store_kernel(const double* __restrict__ Xd, int64_t rows, int K, int KT, double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * K) return;
  const int64_t i = idx % rows, k = idx / rows;
  out[idx] = Xd[i * KT + k];
}

// ---- the two sweeps ----------------------------------------------------------------------------------------------------
// rows 128 b .. 128 b + 127 of a padded state (rows beyond `rows`: `fill`) into LDS, contiguous 8-byte loads
template <int KT>
__device__ __forceinline__ void admix_stage(double* __restrict__ stage, const double* __restrict__ Xd, int64_t b, int64_t rows,
                                            double fill) {
  const int64_t i0 = b * 128;
  for (int idx = threadIdx.x; idx < 128 * KT; idx += 256) stage[idx] = i0 + idx / KT < rows ? Xd[i0 * KT + idx] : fill;
}

// the waves of a workgroup in order: x[] of lanes 0 .. 31 of wave 0 becomes ((w0 + w1) + w2) + w3, cnt likewise.  LDS: red holds
// NV x 32 doubles, value-major (lane r at red[v * 32 + r]: conflict-free)
template <int NV>
__device__ __forceinline__ void admix_wave_order_sum(double (&x)[NV], int& cnt, double* __restrict__ red, int* __restrict__ cnts, int w,
                                                     int r, int h) {
  __syncthreads();  // the staging area is free
  for (int t = 1; t < 4; t++) {
    if (w == t && h == 0) {
#pragma unroll
      for (int v = 0; v < NV; v++) red[v * 32 + r] = x[v];
      cnts[r] = cnt;
    }
    __syncthreads();
    if (w == 0 && h == 0) {
#pragma unroll
      for (int v = 0; v < NV; v++) x[v] += red[v * 32 + r];
      cnt += cnts[r];
    }
    __syncthreads();
  }
}

// the tiles' shares of the likelihood: thread t adds the tiles t, t + 256, ...; butterfly; the four waves in order
__global__ __launch_bounds__(256) void admix_ll_sum_kernel(const double* __restrict__ ll_part, int64_t ntiles, double* __restrict__ out) {
  __shared__ double wll[4];
  double s = 0.0;
  for (int64_t t = threadIdx.x; t < ntiles; t += 256) s += ll_part[t];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) wll[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *out = ((wll[0] + wll[1]) + wll[2]) + wll[3];
}

// ---- the hash hold-out of a view ---------------------------------------------------------------------------------------
// L -> the L of a new view with some typed entries set to code 3; the geometry of tpg_impute_view_kernel (a wave per tile of 32
// loci, four tiles per workgroup, lane (r, h) owns locus r), one read and one write of the layout.  Whether entry (i, j) is held
// out is a predicate of h = tpg_mix64(key(seed, j) ^ M(i)); M(i) of the 128 individuals of a block is the same for the four tiles
// of a workgroup, so it is staged once per block through LDS (a broadcast read) and an entry costs one tpg_mix64.
constexpr uint64_t ADM_CV_SALT = 0xC3C3C3C3C3C3C3C3ull;

struct HoldoutFold {  // the fold of include/tpg.h "admixture cross-validation": the high word of h, scaled to [0, folds)
  int folds, fold;
  __device__ bool operator()(uint64_t h) const { return (int)(((h >> 32) * (uint64_t)folds) >> 32) == fold; }
};
struct HoldoutBelow {  // the fraction of include/tpg.h "sNMF": the high word of h against floor(fraction 2^32)
  uint64_t thr;
  __device__ bool operator()(uint64_t h) const { return (h >> 32) < thr; }
};

// (the predicate travels as its members, A... = their types: as one struct argument the fold kernel came out 3 % slower)
template <class Held, class... A>
__global__ __launch_bounds__(256) void admix_holdout_view_kernel(const uint4* __restrict__ L, uint4* __restrict__ out, int64_t n_lt,
                                                                 int64_t Qb, A... members, uint64_t seed,
                                                                 unsigned long long* __restrict__ d_held) {
  const Held held_out{members...};
  __shared__ uint64_t mi[2][128];  // M(i) of the block's individuals; two buffers: one barrier per block
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int64_t lt = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool live = lt < n_lt;  // a wave beyond the last tile still stages and meets the barriers
  const uint64_t key = tpg_mix64((seed ^ ADM_CV_SALT) ^ tpg_mix64((uint64_t)(lt * 32 + r)));
  int held = 0;
  for (int64_t q = 0; q < Qb; q++) {
    uint64_t* __restrict__ ms = mi[q & 1];
    if (threadIdx.x < 128) ms[threadIdx.x] = tpg_mix64((uint64_t)(128 * q + threadIdx.x));
    __syncthreads();
    if (!live) continue;
    const uint4 a = L[(lt * Qb + q) * 64 + lane];
    uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int d = 0; d < 4; d++) {
      // typed entries only: the padding (individuals >= n, loci >= m) is code 3 and stays so
      uint32_t typed = ~(w[d] & (w[d] >> 1)) & 0x55555555u;
      while (typed) {
        const int pos = __ffs(typed) - 1;  // 8 b + 2 k: element 4 k + b
        typed &= typed - 1;
        const int e = 4 * ((pos & 7) >> 1) + (pos >> 3);
        if (held_out(tpg_mix64(key ^ ms[32 * d + 16 * h + e]))) {
          w[d] |= 3u << pos;
          held++;
        }
      }
    }
    out[(lt * Qb + q) * 64 + lane] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  held = tpg_wave_sum(held);
  if (lane == 0 && held) atomicAdd(d_held, (unsigned long long)held);
}

// the held-out copy of `full` under Held{members...} (the caller holds the context and has checked the members).  fetch: bring
// the number of held-out entries back, for *n_held (may be NULL)
template <class Held, class... A>
int admix_holdout_view(tpg_ctx* ctx, const char* launch_name, const tpg_view* full, uint64_t seed, tpg_view** out, bool fetch,
                       int64_t* n_held, A... members) {
  TPG_TRY(tpg_view_need_L(ctx, full));
  const int64_t n_lt = 4 * full->KG;
  TPG_REQUIRE(ceil_div(n_lt, 4) <= 0x7FFFFFFF, TPG_EUNSUPPORTED, "a hold-out view of %lld loci", (long long)full->m);
  ViewPtr v(new tpg_view(ctx, full->n, full->m));
  DevBuf d_held;
  TPG_HIP(tpg_pmalloc((void**)&v->L, v->bytes_each));
  TPG_TRY(d_held.alloc(8));
  TPG_HIP(hipMemsetAsync(d_held.p, 0, 8, ctx->stream));
  TPG_LAUNCH(ctx, launch_name, (admix_holdout_view_kernel<Held, A...>), dim3((unsigned)ceil_div(n_lt, 4)), dim3(256), 0,
             (const uint4*)full->L, v->L, n_lt, full->Q, members..., seed, d_held.as<unsigned long long>());
  TPG_CHECK_LAUNCH();
  if (fetch) {
    unsigned long long hh = 0;
    TPG_HIP(tpg_fetch_small(ctx, &hh, d_held.p, sizeof hh));
    if (n_held) *n_held = (int64_t)hh;
  }
  *out = v.release();
  return TPG_OK;
}

}  // namespace
