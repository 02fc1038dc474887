// hclust_dev.h -- what hclust.hip (Ward on scores) and tree.hip (linkages and neighbour-joining on a matrix) share, as one text:
// the order in which a pair is picked, the workgroup minimum in that order, the start of the slot state, the row scan that fills
// the nearest-later-neighbour list and the pick of a merge from it.  None of it depends on the recurrence: the list caches row
// minima of S, whatever wrote S.
#pragma once
#include <math.h>

#include "common.h"

namespace {

constexpr int HC_BLOCK = 256;
constexpr int HC_PICK = 1024;
constexpr int HC_ROWNN_GRID = 512;

// what hc_pick hands to the update kernel
struct HcStep {
  int32_t a, b, na, nb;
  double sab;
};

// Ward's Lance-Williams recurrence of the header, every operation rounded once: x = S(a,c), y = S(b,c), the sizes as doubles
__device__ __forceinline__ double hc_ward_lw(double na, double nb, double nc, double x, double y, double sab) {
  const double p = (na + nc) * x;
  const double q = (nb + nc) * y;
  const double r = nc * sab;
  return ((p + q) - r) / ((na + nb) + nc);
}

__global__ void hc_start_kernel(int n, int32_t* __restrict__ size, int32_t* __restrict__ live, int32_t* __restrict__ list,
                                int32_t* __restrict__ list_len, int32_t* __restrict__ failed) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) size[t] = 1, live[t] = 1, list[t] = t;
  if (t == 0) *list_len = n, *failed = 0;
}

// (v, j) < (bv, bj) in the order of the header: a candidate that names nobody (j < 0) loses to everyone
__device__ __forceinline__ bool hc_before(double v, int j, double bv, int bj) {
  if (j < 0) return false;
  if (bj < 0) return true;
  return v < bv || (v == bv && j < bj);
}

// the lexicographic minimum over a workgroup of NT threads; valid on every thread
template <int NT>
__device__ __forceinline__ void hc_block_min(double& v, int& j, double* sv, int* sj) {
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(v, off);
    const int oj = __shfl_xor(j, off);
    if (hc_before(ov, oj, v, j)) v = ov, j = oj;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) sv[wave] = v, sj[wave] = j;
  __syncthreads();
  v = sv[0], j = sj[0];
  for (int w = 1; w < NT / 64; w++)
    if (hc_before(sv[w], sj[w], v, j)) v = sv[w], j = sj[w];
  __syncthreads();
}

__global__ __launch_bounds__(HC_BLOCK) void hc_rownn_kernel(const double* __restrict__ S, int n, const int32_t* __restrict__ live,
                                                           const int32_t* __restrict__ list, const int32_t* __restrict__ list_len,
                                                           int32_t* __restrict__ nn, double* __restrict__ dnn) {
  __shared__ double sv[HC_BLOCK / 64];
  __shared__ int sj[HC_BLOCK / 64];
  const int len = min(*list_len, n);
  for (int q = blockIdx.x; q < len; q += gridDim.x) {
    const int i = list[q];
    const double* __restrict__ row = S + (int64_t)i * n;
    double v = INFINITY;
    int bj = -1;
    // a thread's j ascend, so replacing on strictly smaller keeps its first minimum
    for (int j = i + 1 + threadIdx.x; j < n; j += HC_BLOCK) {
      if (!live[j]) continue;
      const double s = row[j];
      if (bj < 0 || s < v) v = s, bj = j;
    }
    hc_block_min<HC_BLOCK>(v, bj, sv, sj);
    if (threadIdx.x == 0) nn[i] = bj, dnn[i] = bj < 0 ? INFINITY : v;
  }
}

__global__ __launch_bounds__(HC_PICK) void hc_pick_kernel(int n, int step, int32_t* __restrict__ size, int32_t* __restrict__ live,
                                                         const int32_t* __restrict__ nn, const double* __restrict__ dnn,
                                                         int32_t* __restrict__ list_len, int32_t* __restrict__ list_hist,
                                                         int32_t* __restrict__ failed, HcStep* __restrict__ cur, int32_t* __restrict__ merge_a,
                                                         int32_t* __restrict__ merge_b, double* __restrict__ height) {
  __shared__ double sv[HC_PICK / 64];
  __shared__ int sj[HC_PICK / 64];
  double v = INFINITY;
  int bi = -1;
  for (int i = threadIdx.x; i < n; i += HC_PICK) {
    if (!live[i] || nn[i] < 0) continue;
    const double s = dnn[i];
    if (bi < 0 || s < v) v = s, bi = i;
  }
  hc_block_min<HC_PICK>(v, bi, sv, sj);
  if (threadIdx.x != 0) return;
  list_hist[step] = *list_len;
  *list_len = 0;
  // n - 1 steps on n points always find a pair.  Should one not, nothing is indexed with -1: the update kernel does nothing for
  // a < 0, and the host turns the flag into an error before any output is written
  HcStep st = {-1, -1, 0, 0, 0.0};
  if (bi < 0) *failed = 1;
  else {
    st.a = bi, st.b = nn[bi], st.sab = v;
    st.na = size[st.a], st.nb = size[st.b];
    size[st.a] = st.na + st.nb;
    live[st.b] = 0;
  }
  *cur = st;
  merge_a[step] = st.a, merge_b[step] = st.b, height[step] = v;
}

}  // namespace
