// pcrelate.hip -- include/tpg.h "PC-Relate": kinship from the residuals of individual-specific allele frequencies, as three
// n x n Gram matrices of real-valued n x m operands that are never stored.
//
// Step 1 (the coefficients) is the FP64 row-scaled sweep of pca.hip (tpg_sweep_loci_rowscale) with center = the locus mean over
// the typed genotypes and a scale of 1: a missing genotype adds 0 there, which is what the definition asks.
//
// Steps 2 - 3 run per LOCUS BLOCK of B loci (B a multiple of 128, pcr_block_loci: at most 1024, less when 16 B bytes per
// padded row would pass PCR_SCRATCH_CAP), two kernels per block:
//   pcr_operands_kernel  forms mu once per (individual, locus) -- 2 L flops each, as many as one Gram -- in the pinned order of
//     csrc/host/host_pcrelate.h and writes R and S of the block into scratch IN THE FRAGMENT ORDER the Gram kernel reads
//     (M is S != 0: a valid cell has mu in [thr, 1 - thr], so S > 0).  A workgroup is one T block: 32 individuals x 128 loci;
//     thread (r, part) owns individual r and the 16 codes of one T dword (lane (r, h), dword s, part = 2 s + h).  The block's
//     coefficients (128 x L), means and the 32 rows of Q sit in LDS; the loop is k-outer with 16 running sums, so an LDS value
//     of Q serves 16 loci and the per-element order (k ascending from the mean) is the pinned one.
//   pcr_gram_kernel      adds the block to the lower-triangle 16 x 16 tiles of Num, Den, Cnt: three chains of
//     v_mfma_f64_16x16x4_f64 over the same two operand streams.
//
// Fragment order.  The MFMA takes A[row = lane & 15][k = lane >> 4] and B[k = lane >> 4][col = lane & 15], one double per lane,
// and a Gram's two operands are the same matrix: for the 16 individuals of row tile I, step t holds the 64 doubles
//     F[(I * SM + t) * 64 + 16 kq + r16] = X[16 I + r16][locus 4 t + kq of the block],   SM = B / 4 steps,
// so either operand of a step is ONE coalesced 512-byte read and no value moves between lanes.  The tile of individuals j is
// the A operand and the tile of individuals i the B operand: C/D (column = lane & 15, row = (lane >> 4) + 4 reg) then has i on
// the lanes, and the accumulators go to the column-major matrices in 128-byte pieces.
//
// Geometry of the Gram kernel.  A workgroup is a 64 x 64 tile of the lower triangle (4 waves, 32 x 32 each: 2 x 2 MFMA tiles x
// 3 chains = 12 accumulators of 4 doubles, 96 VGPRs); the wave above the diagonal of a diagonal workgroup leaves at once.  A
// step is 8 operand reads (R and S of two row tiles and two column tiles) against 12 MFMAs: the FP64 matrix pipe, not the
// operand traffic, is the limit, so the operands come straight from global memory -- the block's fragments (79 MiB at
// n = 5 000, never more than PCR_SCRATCH_CAP while B > 128) fit the 256 MiB last-level cache and workgroups that run together
// share row and column tiles in L2 -- one step ahead of the MFMAs that use them.  The accumulators live in the output matrices
// between blocks: a wave loads its tiles, adds the block, stores them.  Blocks run in ascending order on one stream and there
// is no floating-point atomic: the same call gives the same bits.  Padding rows (>= n) and loci (>= m) carry code 3 in T: they
// are invalid cells, exact zeros in both operands.
#include "common.h"
#include "devfrag.h"
#include "host/host_pcrelate.h"

namespace {

constexpr int PCR_LB = 128;                          // loci of a T block
constexpr int PCR_MAX_BLOCK = 1024;                  // largest locus block
constexpr size_t PCR_SCRATCH_CAP = (size_t)256 << 20;  // bytes of operand scratch that a block may take while B > 128
constexpr int64_t PCR_ISAF_MAX = (int64_t)1 << 26;   // cells of the dense mu of tpg_pcrelate_isaf

int64_t pcr_rows_pad(int64_t n) { return ceil_div(n, 64) * 64; }
int pcr_block_loci(int64_t n) {
  int64_t B = (int64_t)(PCR_SCRATCH_CAP / (16 * (size_t)pcr_rows_pad(n))) / PCR_LB * PCR_LB;
  return (int)(B < PCR_LB ? PCR_LB : B > PCR_MAX_BLOCK ? PCR_MAX_BLOCK : B);
}
unsigned pcr_grid(int64_t count) { return (unsigned)(ceil_div(count, 256) < 4096 ? ceil_div(count, 256) : 4096); }

// mean over the typed genotypes (0 where none is typed) and the scale of 1 the sweep multiplies by
__global__ void pcr_mean_kernel(const int4* __restrict__ counts, int64_t m, double* __restrict__ mean, double* __restrict__ ones) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const int4 c = counts[j];
    const int64_t t = (int64_t)c.x + c.y + c.z, s1 = (int64_t)c.y + 2 * (int64_t)c.z;
    mean[j] = t > 0 ? (double)s1 / (double)t : 0.0;
    ones[j] = 1.0;
  }
}

// LDS: cs[L][128] (coefficients of the T block, locus order), qs[L][32] (the row tile's Q), ms[128] (means).
// DENSE = false: R and S of T block kg0 + blockIdx.y into the fragments (block-local locus 128 blockIdx.y + jl);
// DENSE = true: mu and valid of every cell inside the data (tpg_pcrelate_isaf)
template <bool DENSE>
__global__ __launch_bounds__(256) void pcr_operands_kernel(const uint4* __restrict__ T, int64_t KG, int64_t kg0, int64_t n, int64_t m,
                                                           const double* __restrict__ mean, const double* __restrict__ c,
                                                           const double* __restrict__ Q, int L, double thr, double hi,
                                                           double* __restrict__ Rf, double* __restrict__ Sf, int64_t SM,
                                                           double* __restrict__ mu_out, uint8_t* __restrict__ valid_out) {
  extern __shared__ double pcr_lds[];
  double* cs = pcr_lds;
  double* qs = cs + (size_t)L * PCR_LB;
  double* ms = qs + (size_t)L * 32;
  const int64_t rt = blockIdx.x, kg = kg0 + blockIdx.y;
  const int r = threadIdx.x & 31, part = threadIdx.x >> 5;
  for (int idx = threadIdx.x; idx < L * PCR_LB; idx += 256) {
    const int64_t j = kg * PCR_LB + (idx & 127);
    cs[idx] = j < m ? c[j + (int64_t)(idx >> 7) * m] : 0.0;
  }
  for (int idx = threadIdx.x; idx < L * 32; idx += 256) {
    const int64_t i = rt * 32 + (idx & 31);
    qs[idx] = i < n ? Q[i + (int64_t)(idx >> 5) * n] : 0.0;
  }
  if (threadIdx.x < PCR_LB) {
    const int64_t j = kg * PCR_LB + threadIdx.x;
    ms[threadIdx.x] = j < m ? mean[j] : 0.0;
  }
  __syncthreads();
  // T lane (r, h), dword s: the loci 32 s + 16 h + e = 16 part + e of the block
  const uint32_t* tw = (const uint32_t*)(T + ((rt * KG + kg) * 64 + r + 32 * (part & 1)));
  const uint32_t w = tw[part >> 1];
  const int jl0 = 16 * part;
  double a[16];
#pragma unroll
  for (int e = 0; e < 16; e++) a[e] = ms[jl0 + e];
  for (int k = 0; k < L; k++) {
    const double q = qs[k * 32 + r];
#pragma unroll
    for (int e = 0; e < 16; e++) a[e] = a[e] + q * cs[k * PCR_LB + jl0 + e];
  }
  const int64_t i = rt * 32 + r;
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int code = (w >> tpg_elem_shift(e)) & 3;
    const double mu = 0.5 * a[e];
    const bool valid = host_pcrelate_valid(code, mu, thr, hi);
    if (DENSE) {
      const int64_t j = kg * PCR_LB + jl0 + e;
      if (i < n && j < m) {
        mu_out[i + j * n] = mu;
        valid_out[i + j * n] = valid ? 1 : 0;
      }
    } else {
      const int jb = PCR_LB * blockIdx.y + jl0 + e;
      const int64_t at = (((i >> 4) * SM + (jb >> 2)) << 6) + 16 * (jb & 3) + (i & 15);
      Rf[at] = valid ? host_pcrelate_r(code, mu) : 0.0;
      Sf[at] = valid ? host_pcrelate_s(mu) : 0.0;
    }
  }
}

// Num, Den, Cnt (n x n column-major, lower triangle) += the `steps` MFMA steps of the block in the fragments
__global__ __launch_bounds__(256) void pcr_gram_kernel(const double* __restrict__ Rf, const double* __restrict__ Sf, int64_t SM, int steps,
                                                       int64_t n, double* __restrict__ num, double* __restrict__ den,
                                                       double* __restrict__ cnt) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, kq = lane >> 4;
  // workgroup x -> tile (bi, bj), bj <= bi, of the lower triangle
  const int64_t x = blockIdx.x;
  int64_t bi = (int64_t)((sqrt(8.0 * (double)x + 1.0) - 1.0) * 0.5);
  while (bi * (bi + 1) / 2 > x) bi--;
  while ((bi + 1) * (bi + 2) / 2 <= x) bi++;
  const int64_t bj = x - bi * (bi + 1) / 2;
  const int wi = wv >> 1, wj = wv & 1;
  if (bi == bj && wj > wi) return;
  const int64_t I0 = bi * 4 + wi * 2, J0 = bj * 4 + wj * 2;  // 16-row tiles
  v4d an[2][2], ad[2][2], ac[2][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) {
      const int64_t i = 16 * (I0 + a) + r16;
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int64_t j = 16 * (J0 + b) + kq + 4 * reg;
        const bool in = i < n && j < n;
        an[a][b][reg] = in ? num[i + j * n] : 0.0;
        ad[a][b][reg] = in ? den[i + j * n] : 0.0;
        ac[a][b][reg] = in ? cnt[i + j * n] : 0.0;
      }
    }
  const double* pri = Rf + (I0 * SM << 6) + lane;
  const double* psi = Sf + (I0 * SM << 6) + lane;
  const double* prj = Rf + (J0 * SM << 6) + lane;
  const double* psj = Sf + (J0 * SM << 6) + lane;
  const int64_t tile = SM << 6;
  double ri[2], si[2], rj[2], sj[2];
#pragma unroll
  for (int a = 0; a < 2; a++) {
    ri[a] = pri[a * tile];
    si[a] = psi[a * tile];
    rj[a] = prj[a * tile];
    sj[a] = psj[a * tile];
  }
  for (int t = 0; t < steps; t++) {
    // the next step's operands leave before this step's MFMAs (the last step reads its own again: inside the fragments)
    const int64_t nx = (int64_t)(t + 1 < steps ? t + 1 : t) << 6;
    double ri2[2], si2[2], rj2[2], sj2[2];
#pragma unroll
    for (int a = 0; a < 2; a++) {
      ri2[a] = pri[a * tile + nx];
      si2[a] = psi[a * tile + nx];
      rj2[a] = prj[a * tile + nx];
      sj2[a] = psj[a * tile + nx];
    }
    double mi[2], mj[2];
#pragma unroll
    for (int a = 0; a < 2; a++) {
      mi[a] = si[a] != 0.0 ? 1.0 : 0.0;
      mj[a] = sj[a] != 0.0 ? 1.0 : 0.0;
    }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++) {
        an[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(rj[b], ri[a], an[a][b], 0, 0, 0);
        ad[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(sj[b], si[a], ad[a][b], 0, 0, 0);
        ac[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(mj[b], mi[a], ac[a][b], 0, 0, 0);
      }
#pragma unroll
    for (int a = 0; a < 2; a++) {
      ri[a] = ri2[a];
      si[a] = si2[a];
      rj[a] = rj2[a];
      sj[a] = sj2[a];
    }
  }
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) {
      const int64_t i = 16 * (I0 + a) + r16;
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int64_t j = 16 * (J0 + b) + kq + 4 * reg;
        if (i < n && j < n) {
          num[i + j * n] = an[a][b][reg];
          den[i + j * n] = ad[a][b][reg];
          cnt[i + j * n] = ac[a][b][reg];
        }
      }
    }
}

// the upper triangle from the lower one
__global__ void pcr_mirror_kernel(int64_t n, double* __restrict__ num, double* __restrict__ den, double* __restrict__ cnt) {
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < n * n; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = idx % n, j = idx / n;
    if (i < j) {
      num[idx] = num[j + i * n];
      den[idx] = den[j + i * n];
      cnt[idx] = cnt[j + i * n];
    }
  }
}

// step 4
__global__ void pcr_epilogue_kernel(int64_t n, const double* __restrict__ num, const double* __restrict__ den,
                                    const double* __restrict__ cnt, double* __restrict__ kin, double* __restrict__ f,
                                    int64_t* __restrict__ n_snp) {
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < n * n; idx += (int64_t)gridDim.x * blockDim.x) {
    const double k = host_pcrelate_kin(num[idx], den[idx]);
    kin[idx] = k;
    if (n_snp) n_snp[idx] = (int64_t)cnt[idx];
    if (idx % n == idx / n) f[idx % n] = host_pcrelate_f(k);
  }
}

int pcr_check_L(int L) {
  TPG_REQUIRE(L >= 1 && L <= TPG_PCRELATE_MAX_K + 1, TPG_EINVAL, "L = %d outside [1, %d]", L, TPG_PCRELATE_MAX_K + 1);
  return TPG_OK;
}
int pcr_check_view(const tpg_view* v) {
  TPG_REQUIRE(v->n >= 1 && v->m >= 1, TPG_EINVAL, "the view is empty (%lld x %lld)", (long long)v->n, (long long)v->m);
  return TPG_OK;
}
int pcr_check_thr(double thr) {
  TPG_REQUIRE(thr > 0.0 && thr < 0.5, TPG_EINVAL, "thr = %g outside (0, 0.5)", thr);
  return TPG_OK;
}
size_t pcr_operand_lds(int L) { return sizeof(double) * ((size_t)L * (PCR_LB + 32) + PCR_LB); }

// step 1, device pointers throughout: d_mean[m], d_c m x L
int pcr_coef(tpg_ctx* ctx, const tpg_view* v, const double* d_Q, int L, double* d_mean, double* d_c, DevArena& sc) {
  const int64_t m = v->m;
  int32_t* d_counts = nullptr;
  double* d_ones = nullptr;
  TPG_TRY(sc.get(&d_counts, 4 * (size_t)m));
  TPG_TRY(sc.get(&d_ones, (size_t)m));
  TPG_TRY(tpg_launch_loci_counts(ctx, v, d_counts));
  TPG_LAUNCH(ctx, "pcrelate_mean", pcr_mean_kernel, dim3(pcr_grid(m)), dim3(256), 0, (const int4*)d_counts, m, d_mean, d_ones);
  TPG_CHECK_LAUNCH();
  return tpg_sweep_loci_rowscale(ctx, v, d_mean, d_ones, d_Q, L, d_c);
}

// steps 2 - 3, device pointers throughout: d_num, d_den, d_cnt n x n, both triangles
int pcr_gram(tpg_ctx* ctx, const tpg_view* v, const double* d_mean, const double* d_c, const double* d_Q, int L, double thr,
             double* d_num, double* d_den, double* d_cnt) {
  const int64_t n = v->n, m = v->m, rows_pad = pcr_rows_pad(n);
  TPG_TRY(tpg_view_need_T(ctx, v));
  int64_t B = pcr_block_loci(n);
  if (B > v->KG * PCR_LB) B = v->KG * PCR_LB;
  const int64_t SM = B / 4, nt64 = rows_pad / 64, tiles = nt64 * (nt64 + 1) / 2;
  TPG_REQUIRE(tiles <= 0x7FFFFFFF, TPG_EINVAL, "n = %lld is more than one launch takes", (long long)n);
  DevBuf frag;
  TPG_TRY(frag.alloc_n<double>(2 * (size_t)rows_pad * (size_t)B));
  double *Rf = frag.as<double>(), *Sf = Rf + rows_pad * B;
  TPG_HIP(hipMemsetAsync(d_num, 0, sizeof(double) * (size_t)n * n, ctx->stream));
  TPG_HIP(hipMemsetAsync(d_den, 0, sizeof(double) * (size_t)n * n, ctx->stream));
  TPG_HIP(hipMemsetAsync(d_cnt, 0, sizeof(double) * (size_t)n * n, ctx->stream));
  const double hi = 1.0 - thr;
  for (int64_t kg0 = 0; kg0 < v->KG; kg0 += B / PCR_LB) {
    const int64_t nb = v->KG - kg0 < B / PCR_LB ? v->KG - kg0 : B / PCR_LB;
    TPG_LAUNCH(ctx, "pcrelate_operands", pcr_operands_kernel<false>, dim3((unsigned)(rows_pad / 32), (unsigned)nb), dim3(256),
               pcr_operand_lds(L), v->T, v->KG, kg0, n, m, d_mean, d_c, d_Q, L, thr, hi, Rf, Sf, SM, (double*)nullptr,
               (uint8_t*)nullptr);
    TPG_LAUNCH(ctx, "pcrelate_gram", pcr_gram_kernel, dim3((unsigned)tiles), dim3(256), 0, (const double*)Rf, (const double*)Sf, SM,
               (int)(nb * (PCR_LB / 4)), n, d_num, d_den, d_cnt);
  }
  TPG_LAUNCH(ctx, "pcrelate_mirror", pcr_mirror_kernel, dim3(pcr_grid(n * n)), dim3(256), 0, n, d_num, d_den, d_cnt);
  TPG_CHECK_LAUNCH();
  TPG_HIP(hipStreamSynchronize(ctx->stream));  // the fragments go back to the pool
  return TPG_OK;
}

struct PcrIn {
  InBuf im, ic, iq;
};
// the checks and uploads that the entry points taking (mean, c, Q) share
int pcr_model_args(tpg_ctx* ctx, const tpg_view* v, const double* mean, const double* c, const double* Q, int L, double thr, PcrIn& in,
                   DevArena& sc) {
  TPG_TRY(pcr_check_L(L));
  TPG_TRY(pcr_check_view(v));
  TPG_TRY(pcr_check_thr(thr));
  TPG_TRY(in.im.init(ctx, mean, sizeof(double) * (size_t)v->m));
  TPG_TRY(in.ic.init(ctx, c, sizeof(double) * (size_t)v->m * (size_t)L));
  TPG_TRY(in.iq.init(ctx, Q, sizeof(double) * (size_t)v->n * (size_t)L));
  TPG_TRY(tpg_check_finite(ctx, in.im.dev<double>(), v->m, sc, "mean"));
  TPG_TRY(tpg_check_finite(ctx, in.ic.dev<double>(), v->m * L, sc, "c"));
  TPG_TRY(tpg_check_finite(ctx, in.iq.dev<double>(), v->n * L, sc, "Q"));
  return TPG_OK;
}

}  // namespace

extern "C" int64_t tpg_pcrelate_block_loci(int64_t n) { return n >= 1 ? pcr_block_loci(n) : 0; }

extern "C" size_t tpg_pcrelate_scratch_bytes(int64_t n, int64_t m, int K) {
  (void)K;  // the operands do not depend on the number of components
  if (n < 1 || m < 1) return 0;
  int64_t B = pcr_block_loci(n);
  if (B > ceil_div(m, PCR_LB) * PCR_LB) B = ceil_div(m, PCR_LB) * PCR_LB;
  return 16 * (size_t)pcr_rows_pad(n) * (size_t)B;
}

extern "C" int64_t tpg_pcrelate_isaf_max_cells(void) { return PCR_ISAF_MAX; }

extern "C" int tpg_pcrelate_basis(const double* V, int64_t n, int K, double* Q) {
  TPG_REQUIRE(Q && (V || K == 0), TPG_EINVAL, "null argument");
  TPG_REQUIRE(K >= 0 && K <= TPG_PCRELATE_MAX_K, TPG_EINVAL, "K = %d outside [0, %d]", K, TPG_PCRELATE_MAX_K);
  TPG_REQUIRE(n >= (int64_t)K + 2, TPG_EINVAL, "n = %lld individuals are too few for %d components and the intercept", (long long)n, K);
  std::vector<double> q((size_t)n * (size_t)(K + 1));
  const int rc = host_pcrelate_basis(V, n, K, q.data());
  TPG_REQUIRE(rc == 0, TPG_EINVAL, "the scores are rank deficient next to the intercept (or hold a value that is not finite)");
  for (size_t i = 0; i < q.size(); i++) Q[i] = q[i];
  return TPG_OK;
}

extern "C" int tpg_pcrelate_coef(tpg_ctx* ctx, const tpg_view* v, const double* Q, int L, double* mean, double* c) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && Q && mean && c, TPG_EINVAL, "null argument");
  TPG_TRY(pcr_check_L(L));
  TPG_TRY(pcr_check_view(v));
  InBuf iq;
  DevArena sc;
  TPG_TRY(iq.init(ctx, Q, sizeof(double) * (size_t)v->n * (size_t)L));
  TPG_TRY(tpg_check_finite(ctx, iq.dev<double>(), v->n * L, sc, "Q"));
  double *d_mean = nullptr, *d_c = nullptr;
  TPG_TRY(sc.get(&d_mean, (size_t)v->m));
  TPG_TRY(sc.get(&d_c, (size_t)v->m * (size_t)L));
  TPG_TRY(pcr_coef(ctx, v, iq.dev<double>(), L, d_mean, d_c, sc));
  TPG_TRY(tpg_deliver(ctx, mean, (const double*)d_mean, (size_t)v->m));
  TPG_TRY(tpg_deliver(ctx, c, (const double*)d_c, (size_t)v->m * (size_t)L));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return TPG_OK;
}

extern "C" int tpg_pcrelate_isaf(tpg_ctx* ctx, const tpg_view* v, const double* mean, const double* c, const double* Q, int L, double thr,
                                 double* mu, uint8_t* valid) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && mean && c && Q && mu && valid, TPG_EINVAL, "null argument");
  TPG_REQUIRE(v->n * v->m <= PCR_ISAF_MAX, TPG_EINVAL, "%lld x %lld cells are more than the %lld a dense mu is offered for", (long long)v->n,
              (long long)v->m, (long long)PCR_ISAF_MAX);
  PcrIn in;
  DevArena sc;
  TPG_TRY(pcr_model_args(ctx, v, mean, c, Q, L, thr, in, sc));
  TPG_TRY(tpg_view_need_T(ctx, v));
  const size_t cells = (size_t)v->n * (size_t)v->m;
  double* d_mu = nullptr;
  uint8_t* d_valid = nullptr;
  TPG_TRY(sc.get(&d_mu, cells));
  TPG_TRY(sc.get(&d_valid, cells));
  TPG_LAUNCH(ctx, "pcrelate_isaf", pcr_operands_kernel<true>, dim3((unsigned)ceil_div(v->n, 32), (unsigned)v->KG), dim3(256),
             pcr_operand_lds(L), v->T, v->KG, (int64_t)0, v->n, v->m, in.im.dev<double>(), in.ic.dev<double>(), in.iq.dev<double>(), L, thr,
             1.0 - thr, (double*)nullptr, (double*)nullptr, (int64_t)0, d_mu, d_valid);
  TPG_CHECK_LAUNCH();
  TPG_TRY(tpg_deliver(ctx, mu, (const double*)d_mu, cells));
  TPG_TRY(tpg_deliver(ctx, valid, (const uint8_t*)d_valid, cells));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return TPG_OK;
}

extern "C" int tpg_pcrelate_gram(tpg_ctx* ctx, const tpg_view* v, const double* mean, const double* c, const double* Q, int L, double thr,
                                 double* num, double* den, double* cnt) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && mean && c && Q && num && den && cnt, TPG_EINVAL, "null argument");
  PcrIn in;
  DevArena sc;
  TPG_TRY(pcr_model_args(ctx, v, mean, c, Q, L, thr, in, sc));
  const size_t nn = (size_t)v->n * (size_t)v->n;
  double *d_num = nullptr, *d_den = nullptr, *d_cnt = nullptr;
  TPG_TRY(sc.get(&d_num, nn));
  TPG_TRY(sc.get(&d_den, nn));
  TPG_TRY(sc.get(&d_cnt, nn));
  TPG_TRY(pcr_gram(ctx, v, in.im.dev<double>(), in.ic.dev<double>(), in.iq.dev<double>(), L, thr, d_num, d_den, d_cnt));
  TPG_TRY(tpg_deliver(ctx, num, (const double*)d_num, nn));
  TPG_TRY(tpg_deliver(ctx, den, (const double*)d_den, nn));
  TPG_TRY(tpg_deliver(ctx, cnt, (const double*)d_cnt, nn));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return TPG_OK;
}

extern "C" int tpg_pcrelate(tpg_ctx* ctx, const tpg_view* v, const double* V, int K, double thr, double* kin, double* f, int64_t* n_snp) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && (V || K == 0) && kin && f, TPG_EINVAL, "null argument");
  TPG_REQUIRE(K >= 0 && K <= TPG_PCRELATE_MAX_K, TPG_EINVAL, "K = %d outside [0, %d]", K, TPG_PCRELATE_MAX_K);
  TPG_TRY(pcr_check_view(v));
  TPG_TRY(pcr_check_thr(thr));
  const int64_t n = v->n, m = v->m;
  const int L = K + 1;
  // step 0 on the host
  HostIn<double> hv;
  if (K > 0) TPG_TRY(hv.init(ctx, V, n * K));
  std::vector<double> q((size_t)n * (size_t)L);
  TPG_TRY(tpg_pcrelate_basis(hv.p, n, K, q.data()));
  InBuf iq;
  DevArena sc;
  TPG_TRY(iq.init(ctx, q.data(), sizeof(double) * q.size()));
  const size_t nn = (size_t)n * (size_t)n;
  double *d_mean = nullptr, *d_c = nullptr, *d_num = nullptr, *d_den = nullptr, *d_cnt = nullptr, *d_kin = nullptr, *d_f = nullptr;
  int64_t* d_ns = nullptr;
  TPG_TRY(sc.get(&d_mean, (size_t)m));
  TPG_TRY(sc.get(&d_c, (size_t)m * (size_t)L));
  TPG_TRY(sc.get(&d_num, nn));
  TPG_TRY(sc.get(&d_den, nn));
  TPG_TRY(sc.get(&d_cnt, nn));
  TPG_TRY(sc.get(&d_kin, nn));
  TPG_TRY(sc.get(&d_f, (size_t)n));
  if (n_snp) TPG_TRY(sc.get(&d_ns, nn));
  TPG_TRY(pcr_coef(ctx, v, iq.dev<double>(), L, d_mean, d_c, sc));
  TPG_TRY(tpg_check_finite(ctx, d_c, m * L, sc, "c (a sum that overflowed)"));
  TPG_TRY(pcr_gram(ctx, v, d_mean, d_c, iq.dev<double>(), L, thr, d_num, d_den, d_cnt));
  TPG_LAUNCH(ctx, "pcrelate_epilogue", pcr_epilogue_kernel, dim3(pcr_grid(n * n)), dim3(256), 0, n, (const double*)d_num,
             (const double*)d_den, (const double*)d_cnt, d_kin, d_f, d_ns);
  TPG_CHECK_LAUNCH();
  TPG_TRY(tpg_deliver(ctx, kin, (const double*)d_kin, nn));
  TPG_TRY(tpg_deliver(ctx, f, (const double*)d_f, (size_t)n));
  TPG_TRY(tpg_deliver(ctx, n_snp, (const int64_t*)d_ns, nn));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return TPG_OK;
}
