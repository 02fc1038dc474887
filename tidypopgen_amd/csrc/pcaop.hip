// pcaop.hip -- the scaled genotype matrix as an OPERATOR on int8 MFMA: the two products a Gram-free PCA needs,
//     zt:  W = Z'Q  (m x b)      W[j,c] = ( sum_i g_ij q~_ic  -  c_j sum_i q~_ic ) / s_j
//     z:   Y = Z W  (n x b)      Y[i,c] =   sum_j g_ij w~'_jc  -  sum_j c_j w~'_jc ,     w'_jc = W[j,c] / s_j
// with Z = (G - 1c')S^-1, codes 0 / 1 / 2, no missing value (the callers' counts check that), 1 <= b <= 64.
//
// Fixed point.  q~ (w~') is the operand rounded to FU_c fractional bits, ONE exponent per column c: ex_c from
// amax_c = max_i |x_ic| (amax_c < 2^ex_c), FU_c = 7 TU - 2 - ex_c, so |x| 2^FU_c < 2^40 and the rounding error of an
// entry is at most 2^-41 2^ex_c <= 2^-40 amax_c.  (The loadings of the SVD take one exponent for the whole block,
// pca.hip: their columns are unit vectors.  The columns a Chebyshev filter leaves differ by up to 1e6 in norm and a
// common exponent would leave the weak ones some 20 bits.)  The rounded integer is split into TU = 6 balanced
// base-128 digits; int8 column c TU + t of the B operand holds digit t of column c: b TU <= 384 int8 columns, at most
// 12 MFMA column tiles.  A column of zeros has digits 0 and comes out as exact zeros.
//
// The contraction.  Both layouts of a view share one fragment format (common.h), so ONE kernel serves both halves:
// zt contracts over individuals with the L layout (row tile = 32 loci, Q chunks of 128 individuals), z over loci with
// the T layout (row tile = 32 individuals, KG chunks of 128 loci).  The A operand is the code bytes themselves; padding
// is code 3 and meets digits that are 0 there.  The chunks are cut into S ranges on blockIdx.y (a 5 000-row panel has
// only 157 row tiles) and every range writes its own int32 partial tile: |acc| <= 2 * 64 * length, so a range is
// shorter than 2^24.  The finalize kernels recombine the digit planes and add the S partials in int64 -- exact, so the
// bits of a result do not depend on S -- and round ONCE to FP64.  No floating-point atomics; the scratch is the digit
// fragments and the partial tiles, linear in n and in m.
//
// The finalize steps are FP64 expressions in a stated order (no contraction: the Makefile compiles this file with
// -ffp-contract=off); tests/pcaop_ref.py restates the model and derives the bounds.
#include <math.h>
#include <stdio.h>

#include <algorithm>

#include "common.h"
#include "devfrag.h"

#define MFMA_I8(a, b, c) __builtin_amdgcn_mfma_i32_32x32x32_i8((a), (b), (c), 0, 0, 0)
#define OP_TU 6        // digits per column (LD_TU of pca.hip)
#define OP_BMAX 64     // columns per block

#define OP_NG 64       // workgroups per column in the column statistics: OP_NG * 256 strided partial results

// pmax[c * OP_NG + g] = max |x_ic| over the rows i = g * 256 + t (mod OP_NG * 256) (x = X / rdiv where rdiv is given),
// NaN if one of them is not finite or too large to scale.  grid (b, OP_NG)
__global__ __launch_bounds__(256) void tpg_pcaop_colmax_kernel(const double* __restrict__ X, int64_t len,
                                                               const double* __restrict__ rdiv, double* __restrict__ pmax) {
  __shared__ double sh[256];
  const int c = blockIdx.x;
  double mx = 0;
  bool bad = false;
  for (int64_t i = blockIdx.y * 256 + threadIdx.x; i < len; i += OP_NG * 256) {
    double x = X[i + (int64_t)c * len];
    if (rdiv) x = x / rdiv[i];
    const double a = fabs(x);
    if (!(a < 1e300)) bad = true;  // NaN, infinity, or too large to scale
    mx = a > mx ? a : mx;
  }
  sh[threadIdx.x] = bad ? TPG_QNAN : mx;
  tpg_block_nanmax<256>(sh);
  if (threadIdx.x == 0) pmax[c * OP_NG + blockIdx.y] = sh[0];
}

// amax[c] and FU[c] = 7 TU - 2 - ex_c, amax_c < 2^ex_c (FU 0 for a column of zeros, and for a column that is not finite:
// its output is NaN).  One workgroup of OP_NG threads per column
__global__ __launch_bounds__(OP_NG) void tpg_pcaop_exponent_kernel(const double* __restrict__ pmax, double* __restrict__ amax,
                                                                  int* __restrict__ FU) {
  __shared__ double sh[OP_NG];
  const int c = blockIdx.x;
  sh[threadIdx.x] = pmax[c * OP_NG + threadIdx.x];
  tpg_block_nanmax<OP_NG>(sh);
  if (threadIdx.x == 0) {
    const double a = sh[0];
    int ex = 0;
    if (a == a && a > 0) frexp(a, &ex);  // a < 2^ex
    amax[c] = a;
    FU[c] = (a == a && a > 0) ? 7 * OP_TU - 2 - ex : 0;
  }
}

__device__ __forceinline__ long long tpg_pcaop_fixed(const double* __restrict__ X, int64_t len, const double* __restrict__ rdiv,
                                                     int64_t i, int c, int fu) {
  double x = X[i + (int64_t)c * len];
  if (rdiv) x = x / rdiv[i];
  return llrint(ldexp(x, fu));  // half to even; |.| <= 2^40
}

// The digit fragments: block ((q * 4 + s) * CT + ct), lane (col = lane & 31, h), byte e  <->  contraction index
// 128 q + 32 s + 16 h + e, int8 column 32 ct + col = c TU + t.  Indices >= len and columns >= b TU hold 0.
// One thread takes the sixteen consecutive indices of one (q, s, h) in ONE column c -- 128 contiguous bytes of the operand,
// the next thread the next sixteen --, rounds each value once and writes the six 16-byte pieces of its digits; the thread
// of the last column also clears the pieces of the int8 columns past b TU.
__global__ __launch_bounds__(256) void tpg_pcaop_digits_kernel(const double* __restrict__ X, int64_t len, int b,
                                                               const double* __restrict__ rdiv, const double* __restrict__ amax,
                                                               const int* __restrict__ FU, int64_t nchunks, int CT,
                                                               uint4* __restrict__ UD) {
  const int64_t nb16 = nchunks * 8, total = nb16 * b;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx / nb16);
    const int64_t blk = idx % nb16;  // = (q * 4 + s) * 2 + h
    const int h = (int)(blk & 1);
    const int64_t qs = blk >> 1, i0 = blk * 16;
    uint32_t w[OP_TU][4];
#pragma unroll
    for (int t = 0; t < OP_TU; t++)
#pragma unroll
      for (int k = 0; k < 4; k++) w[t][k] = 0;
    if (amax[c] > 0) {  // (false for NaN too)
      const int fu = FU[c];
#pragma unroll
      for (int e = 0; e < 16; e++) {
        if (i0 + e >= len) continue;
        long long W = tpg_pcaop_fixed(X, len, rdiv, i0 + e, c, fu);
#pragma unroll
        for (int t = 0; t < OP_TU; t++) {
          long long dig = W & 127;
          if (dig >= 64) dig -= 128;
          W = (W - dig) >> 7;
          w[t][e >> 2] |= (uint32_t)((int)dig & 0xFF) << (8 * (e & 3));
        }
      }
    }
    uint4* const row = UD + qs * CT * 64 + h * 32;  // int8 column `col` of this (q, s, h): row[(col >> 5) * 64 + (col & 31)]
#pragma unroll
    for (int t = 0; t < OP_TU; t++) {
      const int col = c * OP_TU + t;
      row[(col >> 5) * 64 + (col & 31)] = make_uint4(w[t][0], w[t][1], w[t][2], w[t][3]);
    }
    if (c == b - 1)
      for (int col = b * OP_TU; col < CT * 32; col++) row[(col >> 5) * 64 + (col & 31)] = make_uint4(0, 0, 0, 0);
  }
}

// hi 2^21 + lo as the nearest double: both parts are exact in FP64 once lo is brought into [0, 2^21), so the one
// addition rounds the exact integer once
__device__ __forceinline__ double tpg_pcaop_to_double(long long hi, long long lo) {
  const long long carry = lo >> 21;  // arithmetic: floor
  hi += carry;
  lo -= carry << 21;
  return ldexp((double)hi, 21) + (double)lo;
}

// The correction sums of the ROUNDED operand in two steps.  Step 1, grid (b, OP_NG): thread t of workgroup g adds the rows
// i = g * 256 + t, + OP_NG * 256, ... in ascending order, then the 256 sums of a workgroup are added pairwise (t with t + 128,
// then t + 64, ...).  Step 2, one workgroup of OP_NG threads per column: the OP_NG sums pairwise (g with g + 32, ...).
//   wcen == NULL (zt): out[c] = (sum_i x~_ic) 2^-FU_c, the integer sum exact (two int64 limbs), rounded once;
//   wcen given  (z):   out[c] = sum_j wcen_j * (x~_jc 2^-FU_c) in FP64, in that order.
__global__ __launch_bounds__(256) void tpg_pcaop_colsum_kernel(const double* __restrict__ X, int64_t len,
                                                               const double* __restrict__ rdiv,
                                                               const double* __restrict__ amax, const int* __restrict__ FU,
                                                               const double* __restrict__ wcen, double* __restrict__ psum,
                                                               long long* __restrict__ phi, long long* __restrict__ plo) {
  __shared__ long long shi[256], slo[256];
  __shared__ double sh[256];
  const int c = blockIdx.x;
  if (!(amax[c] > 0)) return;  // zeros, or not finite (uniform over the workgroup): step 2 knows
  const int fu = FU[c];
  long long hi = 0, lo = 0;
  double acc = 0;
  for (int64_t i = blockIdx.y * 256 + threadIdx.x; i < len; i += OP_NG * 256) {
    const long long W = tpg_pcaop_fixed(X, len, rdiv, i, c, fu);
    if (wcen) {
      acc += wcen[i] * ldexp((double)W, -fu);
    } else {
      hi += W >> 21;
      lo += W & 0x1FFFFF;
    }
  }
  shi[threadIdx.x] = hi;
  slo[threadIdx.x] = lo;
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      shi[threadIdx.x] += shi[threadIdx.x + w];
      slo[threadIdx.x] += slo[threadIdx.x + w];
      sh[threadIdx.x] += sh[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    psum[c * OP_NG + blockIdx.y] = sh[0];
    phi[c * OP_NG + blockIdx.y] = shi[0];
    plo[c * OP_NG + blockIdx.y] = slo[0];
  }
}

__global__ __launch_bounds__(OP_NG) void tpg_pcaop_colsum2_kernel(const double* __restrict__ psum, const long long* __restrict__ phi,
                                                                 const long long* __restrict__ plo, const double* __restrict__ amax,
                                                                 const int* __restrict__ FU, int fp64, double* __restrict__ out) {
  __shared__ long long shi[OP_NG], slo[OP_NG];
  __shared__ double sh[OP_NG];
  const int c = blockIdx.x;
  const double am = amax[c];
  if (!(am > 0)) {
    if (threadIdx.x == 0) out[c] = am == 0 ? 0.0 : TPG_QNAN;
    return;
  }
  sh[threadIdx.x] = psum[c * OP_NG + threadIdx.x];
  shi[threadIdx.x] = phi[c * OP_NG + threadIdx.x];
  slo[threadIdx.x] = plo[c * OP_NG + threadIdx.x];
  __syncthreads();
  for (int w = OP_NG / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      shi[threadIdx.x] += shi[threadIdx.x + w];
      slo[threadIdx.x] += slo[threadIdx.x + w];
      sh[threadIdx.x] += sh[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[c] = fp64 ? sh[0] : ldexp(tpg_pcaop_to_double(shi[0], slo[0]), -FU[c]);
}

// part[split][row][int8 column] = sum over the split's chunks of code(row, .) * digit(., column).  A workgroup is four
// waves = four consecutive 32-row tiles and ONE range of chunks; every wave keeps CTP accumulator tiles (64 registers at
// CTP = 4) and the four share the digit fragments of a chunk (4 K steps x CTP tiles, 1 KiB each) through LDS: each wave
// fetches a quarter of the next chunk's fragments while the MFMAs of this one run, and stores them into the other
// buffer before the barrier that ends the chunk.  A row tile past the end reads tile 0 and writes nothing; a range
// with no chunk (fewer chunks than ceil(chunks / S) * S) writes zeros.
template <int CTP>
__global__ __launch_bounds__(256) void tpg_pcaop_mfma_kernel(const uint4* __restrict__ A, const uint4* __restrict__ UD,
                                                             int64_t n_rt, int64_t nchunks, int64_t cps, int ct0, int CT,
                                                             int32_t* __restrict__ part, int Cpad, int64_t rows_pad) {
  __shared__ __attribute__((aligned(16))) uint4 ubuf[2][4 * CTP][64];  // [buffer][K step * CTP + column tile][lane]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t rt = (int64_t)blockIdx.x * 4 + wv;
  const bool mine = rt < n_rt;
  const uint4* const pa = A + (mine ? rt : 0) * nchunks * 64 + lane;
  const int64_t q0 = (int64_t)blockIdx.y * cps, q1 = q0 + cps < nchunks ? q0 + cps : nchunks;
  v16i acc[CTP];
#pragma unroll
  for (int c = 0; c < CTP; c++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[c][r] = 0;
  // item it = wv + 4 j of a chunk's 4 * CTP fragments: K step it / CTP, column tile it % CTP
  auto ufrag = [&](int64_t q, int j) {
    const int it = wv + 4 * j;
    return UD[((q * 4 + it / CTP) * CT + ct0 + it % CTP) * 64 + lane];
  };
  if (q0 < q1) {  // (the same for every wave of the workgroup: all of them meet every barrier)
    uint4 a = pa[q0 * 64];
#pragma unroll
    for (int j = 0; j < CTP; j++) ubuf[0][wv + 4 * j][lane] = ufrag(q0, j);
    __syncthreads();
    for (int64_t q = q0; q < q1; q++) {
      const int cur = (int)((q - q0) & 1);
      const bool more = q + 1 < q1;
      const int64_t qn = more ? q + 1 : q;
      const uint4 an = pa[qn * 64];
      uint4 un[CTP];
#pragma unroll
      for (int j = 0; j < CTP; j++) un[j] = ufrag(qn, j);
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const uint32_t w = s == 0 ? a.x : s == 1 ? a.y : s == 2 ? a.z : a.w;
        v4i fg;
#pragma unroll
        for (int k = 0; k < 4; k++) fg[k] = (int)tpg_codes(w, k);
#pragma unroll
        for (int c = 0; c < CTP; c++) {
          const uint4 bq = ubuf[cur][s * CTP + c][lane];
          const v4i fb = {(int)bq.x, (int)bq.y, (int)bq.z, (int)bq.w};
          acc[c] = MFMA_I8(fg, fb, acc[c]);
        }
      }
      // the other buffer was last read in chunk q - 1, which every wave left through the barrier below
#pragma unroll
      for (int j = 0; j < CTP; j++) ubuf[cur ^ 1][wv + 4 * j][lane] = un[j];
      __syncthreads();
      a = an;
    }
  }
  if (!mine) return;
  int32_t* const po = part + ((int64_t)blockIdx.y * rows_pad + rt * 32) * Cpad + 32 * ct0 + (lane & 31);
#pragma unroll
  for (int c = 0; c < CTP; c++)
#pragma unroll
    for (int r = 0; r < 16; r++) po[(int64_t)tpg_cd_row(r, lane) * Cpad + 32 * c] = acc[c][r];
}

// sum_t 128^t sum_splits part[split][row][c TU + t], exact, as the nearest double (see tpg_pcaop_to_double)
__device__ __forceinline__ double tpg_pcaop_recombine(const int32_t* __restrict__ part, int S, int64_t rows_pad, int Cpad,
                                                      int64_t row, int c) {
  long long hi = 0, lo = 0;  // digits 3 .. 5 and 0 .. 2: value = hi 2^21 + lo
  for (int s = 0; s < S; s++) {
    const int32_t* p = part + ((int64_t)s * rows_pad + row) * Cpad + c * OP_TU;
    lo += (long long)p[0] + ((long long)p[1] << 7) + ((long long)p[2] << 14);
    hi += (long long)p[3] + ((long long)p[4] << 7) + ((long long)p[5] << 14);
  }
  return tpg_pcaop_to_double(hi, lo);
}

// W[j + c m] = (gu - center[j] * qsum[c]) / scale[j],   gu = (the exact integer, rounded once) 2^-FU_c
__global__ void tpg_pcaop_finalize_zt_kernel(const int32_t* __restrict__ part, int S, int64_t rows_pad, int Cpad, int64_t m,
                                             int b, const double* __restrict__ amax, const int* __restrict__ FU,
                                             const double* __restrict__ center, const double* __restrict__ scale,
                                             const double* __restrict__ qsum, double* __restrict__ W) {
  const int64_t total = m * b;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % b);  // threads of a wave read one row of `part` contiguously
    const int64_t j = idx / b;
    const double am = amax[c];
    double out;
    if (am == 0) out = 0.0;
    else if (!(am > 0)) out = TPG_QNAN;
    else {
      const double gu = ldexp(tpg_pcaop_recombine(part, S, rows_pad, Cpad, j, c), -FU[c]);
      const double p = center[j] * qsum[c];
      out = (gu - p) / scale[j];
    }
    W[j + (int64_t)c * m] = out;
  }
}

// Y[i + c n] = gu - csum[c]
__global__ void tpg_pcaop_finalize_z_kernel(const int32_t* __restrict__ part, int S, int64_t rows_pad, int Cpad, int64_t n,
                                            int b, const double* __restrict__ amax, const int* __restrict__ FU,
                                            const double* __restrict__ csum, double* __restrict__ Y) {
  const int64_t total = n * b;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % b);
    const int64_t i = idx / b;
    const double am = amax[c];
    double out;
    if (am == 0) out = 0.0;
    else if (!(am > 0)) out = TPG_QNAN;
    else out = ldexp(tpg_pcaop_recombine(part, S, rows_pad, Cpad, i, c), -FU[c]) - csum[c];
    Y[i + (int64_t)c * n] = out;
  }
}

// ---------------------------------------------------------------------------
// host side

// the split of `nchunks` chunks for `nrowtiles` row tiles: the rule of run_sweep (pca.hip) -- double S while the grid is
// short of four workgroups per CU and every range keeps a chunk --, then as many more as keep a range below 2^24 columns
static int64_t pcaop_splits(int64_t nrowtiles, int64_t nchunks, int num_cu) {
  int64_t S = 1;
  const int64_t row_blocks = ceil_div(nrowtiles, 4);
  while (row_blocks * S < 4 * (int64_t)num_cu && S * 2 <= nchunks && S < 64) S *= 2;
  while (ceil_div(nchunks, S) * 128 >= ((int64_t)1 << 24)) S *= 2;
  return S;
}

// the small block: amax, sum, FU (ints), then the OP_NG partial results per column of the maxima, the FP64 sums and the two limbs
#define OP_STAT_DOUBLES (3 * OP_BMAX + 4 * OP_BMAX * OP_NG)
struct PcaOpPlan {
  int64_t Q, KG;
  int CT, Cpad;
  int64_t S_zt, S_z;
  size_t ud_bytes, part_bytes, w_bytes, stat_bytes;
  size_t total() const { return ud_bytes + part_bytes + w_bytes + stat_bytes; }
};
static PcaOpPlan pcaop_plan(int64_t n, int64_t m, int bmax, int num_cu) {
  PcaOpPlan p;
  p.Q = ceil_div(n, 128);
  p.KG = ceil_div(m, 128);
  p.CT = (int)ceil_div((int64_t)bmax * OP_TU, 32);
  p.Cpad = p.CT * 32;
  p.S_zt = pcaop_splits(p.KG * 4, p.Q, num_cu);
  p.S_z = pcaop_splits(p.Q * 4, p.KG, num_cu);
  // the two halves run one after the other on the stream: they share the digit fragments and the partial tiles
  p.ud_bytes = (size_t)std::max(p.Q, p.KG) * 4 * (size_t)p.CT * 1024;
  p.part_bytes = (size_t)std::max(p.S_zt * p.KG, p.S_z * p.Q) * 128 * (size_t)p.Cpad * sizeof(int32_t);
  p.w_bytes = sizeof(double) * (size_t)m * (size_t)bmax;
  p.stat_bytes = OP_STAT_DOUBLES * sizeof(double);
  return p;
}

size_t tpg_pcaop_work_bytes(int64_t n, int64_t m, int bmax, int num_cu) { return pcaop_plan(n, m, bmax, num_cu).total(); }

int tpg_pcaop_init(tpg_ctx* ctx, TpgPcaOp* op, const tpg_view* v, const double* d_center, const double* d_scale, int bmax) {
  TPG_REQUIRE(bmax >= 1 && bmax <= OP_BMAX, TPG_EINVAL, "b = %d out of [1, %d]", bmax, OP_BMAX);
  // |acc| <= 2 * 64 * n in the int32 accumulators of zt, whose contraction over the individuals is cut only to fill the chip
  TPG_REQUIRE(v->n < ((int64_t)1 << 24), TPG_EINVAL, "n = %lld: the operator products take fewer than 2^24 individuals",
              (long long)v->n);
  op->v = v;
  op->d_center = d_center;
  op->d_scale = d_scale;
  op->bmax = bmax;
  op->n_apply = 0;
  const PcaOpPlan p = pcaop_plan(v->n, v->m, bmax, ctx->num_cu);
  TPG_TRY(op->mem.get(&op->UD, p.ud_bytes / sizeof(uint4)));
  TPG_TRY(op->mem.get(&op->part, p.part_bytes / sizeof(int32_t)));
  TPG_TRY(op->mem.get(&op->W, (size_t)v->m * (size_t)bmax));
  TPG_TRY(op->mem.get(&op->stat, OP_STAT_DOUBLES));
  TPG_TRY(tpg_view_need_T(ctx, v));
  TPG_TRY(tpg_view_need_L(ctx, v));
  return TPG_OK;
}

// out (rows x b) = one half: A = the layout whose row tiles are the output's rows, X (len x b) the operand
static int pcaop_half(tpg_ctx* ctx, TpgPcaOp* op, bool zt, const double* d_X, int b, double* d_out) {
  TPG_REQUIRE(b >= 1 && b <= op->bmax, TPG_EINVAL, "b = %d out of [1, %d]", b, op->bmax);
  const tpg_view* v = op->v;
  const int64_t len = zt ? v->n : v->m, rows = zt ? v->m : v->n;
  const int64_t nchunks = zt ? v->Q : v->KG, n_rt = (zt ? v->KG : v->Q) * 4, rows_pad = n_rt * 32;
  const uint4* const A = zt ? v->L : v->T;
  const int CT = (int)ceil_div((int64_t)b * OP_TU, 32), Cpad = CT * 32;
  const int64_t S = pcaop_splits(n_rt, nchunks, ctx->num_cu), cps = ceil_div(nchunks, S);
  double *const d_amax = op->stat, *const d_sum = op->stat + OP_BMAX;
  int* const d_FU = (int*)(op->stat + 2 * OP_BMAX);
  const double* const rdiv = zt ? nullptr : op->d_scale;
  const char* const nm_dig = zt ? "pcaop_zt_digits" : "pcaop_z_digits";
  const char* const nm_mfma = zt ? "pcaop_zt_mfma" : "pcaop_z_mfma";
  const char* const nm_fin = zt ? "pcaop_zt_finalize" : "pcaop_z_finalize";
  double* const d_pmax = op->stat + 3 * OP_BMAX;
  double* const d_psum = d_pmax + OP_BMAX * OP_NG;
  long long *const d_phi = (long long*)(d_psum + OP_BMAX * OP_NG), *const d_plo = d_phi + OP_BMAX * OP_NG;
  const double* const wcen = zt ? (const double*)nullptr : op->d_center;
  TPG_LAUNCH(ctx, nm_dig, tpg_pcaop_colmax_kernel, dim3((unsigned)b, OP_NG), dim3(256), 0, d_X, len, rdiv, d_pmax);
  TPG_LAUNCH(ctx, nm_dig, tpg_pcaop_exponent_kernel, dim3((unsigned)b), dim3(OP_NG), 0, (const double*)d_pmax, d_amax, d_FU);
  TPG_LAUNCH(ctx, nm_dig, tpg_pcaop_digits_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(nchunks * 8 * b, 256), 1 << 20)),
             dim3(256), 0, d_X, len, b, rdiv, (const double*)d_amax, (const int*)d_FU, nchunks, CT, op->UD);
  TPG_LAUNCH(ctx, nm_dig, tpg_pcaop_colsum_kernel, dim3((unsigned)b, OP_NG), dim3(256), 0, d_X, len, rdiv, (const double*)d_amax,
             (const int*)d_FU, wcen, d_psum, d_phi, d_plo);
  TPG_LAUNCH(ctx, nm_dig, tpg_pcaop_colsum2_kernel, dim3((unsigned)b), dim3(OP_NG), 0, (const double*)d_psum, (const long long*)d_phi,
             (const long long*)d_plo, (const double*)d_amax, (const int*)d_FU, zt ? 0 : 1, d_sum);
  const dim3 grid((unsigned)ceil_div(n_rt, 4), (unsigned)S);
  for (int ct0 = 0; ct0 < CT;) {
    const int left = CT - ct0;
#define OP_LAUNCH(C)                                                                                                \
  TPG_LAUNCH(ctx, nm_mfma, (tpg_pcaop_mfma_kernel<C>), grid, dim3(256), 0, A, (const uint4*)op->UD, n_rt, nchunks, cps, \
             ct0, CT, op->part, Cpad, rows_pad)
    if (left >= 4) { OP_LAUNCH(4); ct0 += 4; }
    else if (left == 3) { OP_LAUNCH(3); ct0 += 3; }
    else if (left == 2) { OP_LAUNCH(2); ct0 += 2; }
    else { OP_LAUNCH(1); ct0 += 1; }
#undef OP_LAUNCH
  }
  if (zt)
    TPG_LAUNCH(ctx, nm_fin, tpg_pcaop_finalize_zt_kernel, dim3(2048), dim3(256), 0, (const int32_t*)op->part, (int)S, rows_pad,
               Cpad, rows, b, (const double*)d_amax, (const int*)d_FU, op->d_center, op->d_scale, (const double*)d_sum, d_out);
  else
    TPG_LAUNCH(ctx, nm_fin, tpg_pcaop_finalize_z_kernel, dim3(2048), dim3(256), 0, (const int32_t*)op->part, (int)S, rows_pad,
               Cpad, rows, b, (const double*)d_amax, (const int*)d_FU, (const double*)d_sum, d_out);
  TPG_CHECK_LAUNCH();
  return TPG_OK;
}

int tpg_pcaop_zt(tpg_ctx* ctx, TpgPcaOp* op, const double* d_Q, int b, double* d_W) { return pcaop_half(ctx, op, true, d_Q, b, d_W); }
int tpg_pcaop_z(tpg_ctx* ctx, TpgPcaOp* op, const double* d_W, int b, double* d_Y) { return pcaop_half(ctx, op, false, d_W, b, d_Y); }

// Y = Z (Z'Q): one operator application, nothing waited for
int tpg_pcaop_apply(tpg_ctx* ctx, TpgPcaOp* op, const double* d_Q, int b, double* d_Y) {
  TPG_TRY(pcaop_half(ctx, op, true, d_Q, b, op->W));
  TPG_TRY(pcaop_half(ctx, op, false, op->W, b, d_Y));
  op->n_apply++;
  return TPG_OK;
}

// ---------------------------------------------------------------------------
// C ABI: the halves on their own

// a missing genotype / a zero scale among the arguments: what tpg_pca_center_scale refuses
__global__ void tpg_pcaop_check_kernel(const int4* __restrict__ counts, const double* __restrict__ scale, int64_t m,
                                       int* __restrict__ flags) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    if (counts[j].w != 0) flags[0] = 1;
    if (!(fabs(scale[j]) > 0)) flags[1] = 1;
  }
}

static int pcaop_prod(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale, const double* X, int b,
                      double* out, bool zt) {
  TPG_REQUIRE(ctx && v && center && scale && X && out, TPG_EINVAL, "null argument");
  TPG_REQUIRE(b >= 1 && b <= OP_BMAX, TPG_EINVAL, "b = %d out of [1, %d]", b, OP_BMAX);
  const int64_t n = v->n, m = v->m, len = zt ? n : m, rows = zt ? m : n;
  InBuf ic, is, ix;
  TPG_TRY(ic.init(ctx, center, sizeof(double) * (size_t)m));
  TPG_TRY(is.init(ctx, scale, sizeof(double) * (size_t)m));
  TPG_TRY(ix.init(ctx, X, sizeof(double) * (size_t)len * (size_t)b));
  OutBuf oo;
  TPG_TRY(oo.init(out, sizeof(double) * (size_t)rows * (size_t)b));
  DevBuf d_counts, d_flags;
  TPG_TRY(d_counts.alloc_n<int32_t>(4 * (size_t)m));
  TPG_TRY(d_flags.alloc_n<int>(2));
  TPG_TRY(tpg_launch_loci_counts(ctx, v, d_counts.as<int32_t>()));
  TPG_HIP(hipMemsetAsync(d_flags.p, 0, 2 * sizeof(int), ctx->stream));
  TPG_LAUNCH(ctx, "pcaop_check", tpg_pcaop_check_kernel, dim3(1024), dim3(256), 0, (const int4*)d_counts.p, is.dev<double>(), m,
             d_flags.as<int>());
  int flags[2] = {0, 0};
  TPG_HIP(tpg_fetch_small(ctx, flags, d_flags.p, sizeof(flags)));
  TPG_REQUIRE(!flags[0], TPG_ENUMERIC, "You can't have missing values in 'X'.");
  TPG_REQUIRE(!flags[1], TPG_ENUMERIC, "Some variables have a zero scaling; remove them before attempting to scale variables.");
  TpgPcaOp op;
  TPG_TRY(tpg_pcaop_init(ctx, &op, v, ic.dev<double>(), is.dev<double>(), b));
  TPG_TRY(pcaop_half(ctx, &op, zt, ix.dev<double>(), b, oo.dev<double>()));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return oo.commit(ctx);
}

extern "C" int tpg_pca_zt_prod(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale, const double* Q,
                               int b, double* W) {
  TpgEnter _enter(ctx);
  return pcaop_prod(ctx, v, center, scale, Q, b, W, true);
}

extern "C" int tpg_pca_z_prod(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale, const double* W,
                              int b, double* Y) {
  TpgEnter _enter(ctx);
  return pcaop_prod(ctx, v, center, scale, W, b, Y, false);
}
