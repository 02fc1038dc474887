// admix_common.h -- what the ancestry estimators share (admix.hip: the EM of "admixture"; snmf.hip: "sNMF"): the seeded start,
// the loading and storing of a padded state, the staging of state rows through LDS, the sums of fixed shape and the hash
// hold-out of a view.  Included by those two files only; everything sits in their unnamed namespace.
#pragma once
#include "common.h"
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

// element e of a packed dword (common.h: e = 4 k + b at bits 8 b + 2 k)
__device__ __forceinline__ int admix_code(uint32_t w, int e) { return (int)((w >> (8 * (e & 3) + 2 * (e >> 2))) & 3u); }

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

constexpr uint64_t ADM_CV_SALT = 0xC3C3C3C3C3C3C3C3ull;

}  // namespace
