// f2.hip -- blocked f2 and allele-frequency products per pair of groups (include/tpg.h "f2 blocks"), and the host-side f4 / f3
// block jackknife on top of them.
//
// What the reference does (R/gt_extract_f2.R:141-189): gt_to_aftable pulls the m x 2G table of grouped_alt_freq_dip_pseudo_cpp
// to R, admixtools::discard_from_aftable filters its rows and admixtools::afs_to_f2_blocks forms m x G x G arrays of
// (p1 - p2)^2 - e1 - e2 before averaging them per block.  admixtools is not among the reference's sources: the arithmetic is
// the definition in include/tpg.h, restated in tests/f2_ref.py.
//
// Here, behind the count sweep of tpg_grouped_counts (loci.hip; the count layout FstSrc reads in fst.hip), whose table stays in HBM:
//   f2_flags    one pass over the table: the locus filters (maxmiss, minmaf / maxmaf, minac2, keep) and poly, one byte per
//               locus.  A workgroup owns 64 loci; the table is read with the class on the lanes, the G values of a locus are
//               then walked by one thread in ascending g (the order the definition gives the mean of p).
//   f2_n_kept   kept loci per block (an integer sum).
//   f2_gemm     one workgroup per (block, 64 x 64 tile of group pairs with tR <= tC).  With w the locus weight (kept, and poly
//               where poly_only asks), m_g = w t, a = m (p^2 - e), b = m, c = m p:
//                   sum of f2 terms = (A B')[g1,g2] + (B A')[g1,g2] - 2 (C C')[g1,g2]     cnt = B B'     sum of ap terms = C C'
//               as in tpg_fst_hudson_gemm_kernel (fst.hip), on v_mfma_f64_16x16x4_f64.  B A' is (A B')' and is formed as a
//               product of its own, so that a tile holds everything its cells need: the division by cnt, the NaN and the +0.0
//               diagonal happen in registers and the result goes straight to the output, both triangles from one tile (f2 and
//               ap are symmetric bit for bit).  No partial sums in memory, no second kernel.
//               The block's loci are staged TPG_F2_CHUNK_LOCI at a time in ascending order from lo[b] and every accumulator is
//               carried through the whole block by the same lane: a cell depends on (lo, hi, g1, g2) alone.
//               poly_only = "f2" (the default) weighs f2 and ap differently: the ap products then take a second launch of the
//               same kernel (two products instead of four).  With equal weights ap comes out of the first.
// No atomics anywhere.
#include "common.h"
#include "devfrag.h"
#include "host/host_f4jack.h"

#include <math.h>
#include <string.h>

namespace {

constexpr int F2_T = 64;                    // groups per tile side
constexpr int F2_LB = TPG_F2_CHUNK_LOCI;    // loci per staged chunk
constexpr int F2_RS = 80;                   // row stride of the staged arrays in doubles: 32 dwords modulo the 64 banks, so that the
                                            // loci l and l + 1 a half-wave reads fall on disjoint banks (as FSTG_RS_MFMA)
typedef double f2_v4d __attribute__((ext_vector_type(4)));

struct F2Src {
  const int32_t* cnt;  // [3][Mpad][Cpad]: het, hom-alt, valid (GroupedCounts)
  int64_t Mpad;
  int Cpad;
  int has_hap;  // class = 2 g + (ploidy == 1)
};

// c (valid alleles) and p = alt / c of group g at locus j, as tpg_group_vals / tpg_grouped_finalize_kernel (loci.hip) form
// them for tpg_grouped_alt_freq_dip_pseudo; c = 0 gives p = NaN
__device__ __forceinline__ void f2_cp(const F2Src& s, int64_t j, int g, double& c, double& p) {
  const int64_t plane = s.Mpad * s.Cpad;
  if (!s.has_hap) {
    const int64_t o = j * s.Cpad + g;
    const int n1 = s.cnt[o], n2 = s.cnt[plane + o], nv = s.cnt[2 * plane + o];
    c = (double)(2 * nv);
    p = (double)(n1 + 2 * n2) / c;
  } else {
    const int64_t o = j * s.Cpad + 2 * g;
    const int n1d = s.cnt[o], n2d = s.cnt[plane + o], nvd = s.cnt[2 * plane + o];
    const int n1h = s.cnt[o + 1], n2h = s.cnt[plane + o + 1], nvh = s.cnt[2 * plane + o + 1];
    c = (double)(2 * nvd + nvh);
    p = ((double)(n1d + 2 * n2d) + 0.5 * (double)(n1h + 2 * n2h)) / c;
  }
}

// flags[j]: bit 0 = the locus passes the filters, bit 1 = poly
__global__ __launch_bounds__(256) void f2_flags_kernel(F2Src src, int64_t m, int G, double maxmiss, double minmaf, double maxmaf,
                                                       int minac2, const uint8_t* __restrict__ keep, uint8_t* __restrict__ flags) {
  __shared__ double tp[32][65];
  __shared__ double tc[32][65];
  const int64_t j0 = (int64_t)blockIdx.x * 64;
  // state of locus j0 + threadIdx.x (threads 0 .. 63)
  int ntyped = 0;
  bool lowc = false, poly = false;
  double sum = 0.0, first = 0.0;
  for (int g0 = 0; g0 < G; g0 += 32) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * 32; idx += 256) {
      const int gl = idx & 31, l = idx >> 5;
      if (g0 + gl < G && j0 + l < m) {
        double c, p;
        f2_cp(src, j0 + l, g0 + gl, c, p);
        tc[gl][l] = c; tp[gl][l] = p;
      }
    }
    __syncthreads();
    if (threadIdx.x < 64 && j0 + threadIdx.x < m) {
      const int gend = G - g0 < 32 ? G - g0 : 32;
      for (int gl = 0; gl < gend; gl++) {
        const double c = tc[gl][threadIdx.x], p = tp[gl][threadIdx.x];
        if (c < 2.0) lowc = true;
        if (c > 0.0) {
          if (ntyped == 0) first = p;
          else if (p != first) poly = true;
          sum += p;
          ntyped++;
        }
      }
    }
  }
  if (threadIdx.x >= 64 || j0 + threadIdx.x >= m) return;
  bool kept = ntyped > 0;
  if ((double)(G - ntyped) / (double)G > maxmiss) kept = false;
  if (kept) {
    const double f = sum / (double)ntyped, r = 1.0 - f;
    const double maf = f < r ? f : r;
    if (maf < minmaf || maf > maxmaf) kept = false;
  }
  if (minac2 && lowc) kept = false;
  if (keep && !keep[j0 + threadIdx.x]) kept = false;
  flags[j0 + threadIdx.x] = (uint8_t)((kept ? 1 : 0) | (poly ? 2 : 0));
}

// one workgroup per block: loci with bit 0 set
__global__ __launch_bounds__(256) void f2_n_kept_kernel(const uint8_t* __restrict__ flags, const int64_t* __restrict__ lo,
                                                        const int64_t* __restrict__ hi, long long* __restrict__ n_kept) {
  __shared__ long long part[4];
  const int64_t b = blockIdx.x;
  long long s = 0;
  for (int64_t j = lo[b] + threadIdx.x; j < hi[b]; j += 256) s += flags[j] & 1;
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) n_kept[b] = part[0] + part[1] + part[2] + part[3];
}

// WITH_A: the f2 pass (products A B', B A', C C', B B' -> f2, cnt and, where the pointers are given, ap, ap_cnt of the SAME locus
// weights); otherwise the ap pass (C C', B B' -> ap, ap_cnt).  Grid (block, tile pair tR <= tC in row-major order of the upper
// triangle).  A wave owns 16 row groups x all 64 column groups: 4 column tiles x 4 (or 2) products of 4 FP64 accumulators.
template <bool WITH_A>
__global__ __launch_bounds__(256) void f2_gemm_kernel(F2Src src, int G, int ntile, const int64_t* __restrict__ lo,
                                                      const int64_t* __restrict__ hi, const uint8_t* __restrict__ flags, int need_poly,
                                                      int apply_corr, double* __restrict__ out_f2, int32_t* __restrict__ out_cnt,
                                                      double* __restrict__ out_ap, int32_t* __restrict__ out_apcnt) {
  __shared__ __attribute__((aligned(16))) double sh[6 * F2_LB * F2_RS];
  int tR = 0, u = blockIdx.y;
  while (u >= ntile - tR) { u -= ntile - tR; tR++; }
  const int tC = tR + u;
  const bool diag = tR == tC;
  double* rA = sh;                       // [l][F2_RS]: a of the row groups
  double* rB = sh + F2_LB * F2_RS;       // b
  double* rC = sh + 2 * F2_LB * F2_RS;   // c
  double* cA = diag ? rA : sh + 3 * F2_LB * F2_RS;  // ... of the column groups (a tile on the diagonal stages its groups once)
  double* cB = diag ? rB : sh + 4 * F2_LB * F2_RS;
  double* cC = diag ? rC : sh + 5 * F2_LB * F2_RS;
  double AB[4][4], BA[4][4], CC[4][4], BB[4][4];  // [column tile][C/D register]
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) { AB[r][c] = 0.0; BA[r][c] = 0.0; CC[r][c] = 0.0; BB[r][c] = 0.0; }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, kq = lane >> 4;
  const int64_t b = blockIdx.x, j_lo = lo[b], j_hi = hi[b];
  const int nstage = (diag ? 1 : 2) * F2_LB * F2_T;
  for (int64_t j0 = j_lo; j0 < j_hi; j0 += F2_LB) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < nstage; idx += 256) {
      const int side = idx / (F2_LB * F2_T), rem = idx % (F2_LB * F2_T);
      const int l = rem / F2_T, gl = rem % F2_T;
      const int g = (side ? tC : tR) * F2_T + gl;
      const int64_t j = j0 + l;
      double av = 0.0, bv = 0.0, cv = 0.0;
      if (j < j_hi && g < G) {
        const int fl = flags[j];
        if ((fl & 1) && (!need_poly || (fl & 2))) {
          double c, p;
          f2_cp(src, j, g, c, p);
          if (c > 0.0) {
            double e = 0.0;
            if (apply_corr) {
              const double cm1 = c - 1.0;
              e = (p * (1.0 - p)) / (cm1 > 1.0 ? cm1 : 1.0);
            }
            av = p * p - e; bv = 1.0; cv = p;
          }
        }
      }
      const int o = l * F2_RS + gl;
      if (side) { if (WITH_A) cA[o] = av; cB[o] = bv; cC[o] = cv; }
      else { if (WITH_A) rA[o] = av; rB[o] = bv; rC[o] = cv; }
    }
    __syncthreads();
    // MFMA operands: A[row group 16 wv + r16][locus l + kq], B[locus l + kq][column group 16 ct + r16]
#pragma unroll
    for (int l = 0; l < F2_LB; l += 4) {
      const int ro = (l + kq) * F2_RS + 16 * wv + r16;
      const double ra = WITH_A ? rA[ro] : 0.0, rb = rB[ro], rc = rC[ro];
#pragma unroll
      for (int ct = 0; ct < 4; ct++) {
        const int co = (l + kq) * F2_RS + 16 * ct + r16;
        const double cb = cB[co], cc = cC[co];
        if (WITH_A) {
          const double ca = cA[co];
          *(f2_v4d*)AB[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra, cb, *(f2_v4d*)AB[ct], 0, 0, 0);
          *(f2_v4d*)BA[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(rb, ca, *(f2_v4d*)BA[ct], 0, 0, 0);
        }
        *(f2_v4d*)CC[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(rc, cc, *(f2_v4d*)CC[ct], 0, 0, 0);
        *(f2_v4d*)BB[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(rb, cb, *(f2_v4d*)BB[ct], 0, 0, 0);
      }
    }
  }
  // C/D: column = lane & 15, row = (lane >> 4) + 4 reg.  Cell (g1, g2) and, off the diagonal tiles, its mirror.
  const int64_t base = b * (int64_t)G * G;
#pragma unroll
  for (int ct = 0; ct < 4; ct++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int g1 = tR * F2_T + 16 * wv + kq + 4 * reg, g2 = tC * F2_T + 16 * ct + r16;
      if (g1 >= G || g2 >= G) continue;
      const int64_t o = base + g1 + (int64_t)g2 * G, ot = base + g2 + (int64_t)g1 * G;
      const double n = BB[ct][reg], cc = CC[ct][reg];  // n: a sum of ones below 2^53, exact
      if (WITH_A) {
        double f = TPG_QNAN;
        if (n > 0.0) f = g1 == g2 ? 0.0 : ((AB[ct][reg] + BA[ct][reg]) - 2.0 * cc) / n;
        if (out_f2) { out_f2[o] = f; if (!diag) out_f2[ot] = f; }
        if (out_cnt) { out_cnt[o] = (int32_t)n; if (!diag) out_cnt[ot] = (int32_t)n; }
      }
      if (out_ap) {
        const double a = n > 0.0 ? cc / n : TPG_QNAN;
        out_ap[o] = a;
        if (!diag) out_ap[ot] = a;
      }
      if (out_apcnt) { out_apcnt[o] = (int32_t)n; if (!diag) out_apcnt[ot] = (int32_t)n; }
    }
}

}  // namespace

extern "C" int64_t tpg_f2_chunk_loci(void) { return F2_LB; }

extern "C" int tpg_f2_params_default(tpg_f2_params* p) {
  TPG_REQUIRE(p, TPG_EINVAL, "null argument");
  p->maxmiss = 0.0;
  p->minmaf = 0.0;
  p->maxmaf = 0.5;
  p->minac2 = 0;
  p->poly_only = TPG_F2_POLY_F2;
  p->apply_corr = 1;
  p->keep = nullptr;
  return TPG_OK;
}

extern "C" int tpg_f4_jackknife(const double* f2, int G, int64_t nb, const int64_t* block_len, const int32_t* quads0, int64_t nq,
                                double* est, double* se, int32_t* n_used) {
  TPG_REQUIRE(G >= 1 && nb >= 0 && nq >= 0, TPG_EINVAL, "G = %d, nb = %lld, nq = %lld", G, (long long)nb, (long long)nq);
  TPG_REQUIRE(nq == 0 || quads0, TPG_EINVAL, "null argument");
  TPG_REQUIRE(nb == 0 || (f2 && block_len), TPG_EINVAL, "null argument");
  for (int64_t k = 0; k < 4 * nq; k++)
    TPG_REQUIRE(quads0[k] >= 0 && quads0[k] < G, TPG_EINVAL, "quads[%lld] = %d out of [0,%d)", (long long)k, quads0[k], G);
  for (int64_t q = 0; q < nq; q++) {
    double e, s;
    int32_t g;
    tpg_f4_jackknife_one(f2, G, nb, block_len, quads0[4 * q], quads0[4 * q + 1], quads0[4 * q + 2], quads0[4 * q + 3], &e, &s, &g);
    if (est) est[q] = e;
    if (se) se[q] = s;
    if (n_used) n_used[q] = g;
  }
  return TPG_OK;
}

extern "C" int tpg_f2_blocks(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups, const double* ploidy,
                             const tpg_f2_params* params, const int64_t* lo, const int64_t* hi, int64_t nb, double* f2, int32_t* cnt,
                             double* ap, int32_t* ap_cnt, int64_t* n_kept) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v, TPG_EINVAL, "null argument");
  TPG_REQUIRE(nb >= 0 && nb <= TPG_F2_MAX_BLOCKS, TPG_EINVAL, "nb = %lld out of [0, %lld]", (long long)nb, (long long)TPG_F2_MAX_BLOCKS);
  TPG_REQUIRE(nb == 0 || (lo && hi), TPG_EINVAL, "null argument");
  TPG_REQUIRE(ngroups >= 1 && ngroups <= TPG_F2_MAX_GROUPS, TPG_EINVAL, "ngroups = %d out of [1, %d]", ngroups, TPG_F2_MAX_GROUPS);
  tpg_f2_params pr;
  tpg_f2_params_default(&pr);
  if (params) pr = *params;
  TPG_REQUIRE(pr.minac2 == 0 || pr.minac2 == 1, TPG_EINVAL, "minac2 = %d: only 0 and 1 are supported", pr.minac2);
  TPG_REQUIRE(pr.poly_only >= 0 && pr.poly_only <= (TPG_F2_POLY_F2 | TPG_F2_POLY_AP), TPG_EINVAL, "poly_only = %d", pr.poly_only);
  TPG_REQUIRE(pr.maxmiss == pr.maxmiss && pr.minmaf == pr.minmaf && pr.maxmaf == pr.maxmaf, TPG_EINVAL, "a filter bound is NaN");
  const int G = ngroups;
  const int64_t m = v->m;
  ClassPlan cp;
  TPG_TRY(make_class_plan(v->n, groupIds0, G, ploidy, &cp));
  if (nb == 0) return TPG_OK;
  TPG_TRY(tpg_check_ranges(ctx, lo, hi, nb, m, "block"));
  GroupedCounts gc;
  TPG_TRY(tpg_grouped_counts(ctx, v, cp.cls.data(), cp.nclass, &gc));
  const F2Src src{gc.cnt, gc.Mpad, gc.Cpad, cp.has_hap};
  InBuf il, ih, ik;
  TPG_TRY(il.init(ctx, lo, sizeof(int64_t) * (size_t)nb));
  TPG_TRY(ih.init(ctx, hi, sizeof(int64_t) * (size_t)nb));
  if (pr.keep) TPG_TRY(ik.init(ctx, pr.keep, (size_t)m));
  const size_t cells = (size_t)G * (size_t)G * (size_t)nb;
  OutBuf of, oc, oa, oac, on;
  if (f2) TPG_TRY(of.init(f2, sizeof(double) * cells));
  if (cnt) TPG_TRY(oc.init(cnt, sizeof(int32_t) * cells));
  if (ap) TPG_TRY(oa.init(ap, sizeof(double) * cells));
  if (ap_cnt) TPG_TRY(oac.init(ap_cnt, sizeof(int32_t) * cells));
  if (n_kept) TPG_TRY(on.init(n_kept, sizeof(int64_t) * (size_t)nb));
  DevArena sc;
  uint8_t* d_flags = nullptr;
  TPG_TRY(sc.get(&d_flags, (size_t)m));
  if (m > 0)
    TPG_LAUNCH(ctx, "f2_flags", f2_flags_kernel, dim3((unsigned)ceil_div(m, 64)), dim3(256), 0, src, m, G, pr.maxmiss, pr.minmaf,
               pr.maxmaf, (int)pr.minac2, pr.keep ? ik.dev<uint8_t>() : (const uint8_t*)nullptr, d_flags);
  if (n_kept)
    TPG_LAUNCH(ctx, "f2_n_kept", f2_n_kept_kernel, dim3((unsigned)nb), dim3(256), 0, (const uint8_t*)d_flags, il.dev<int64_t>(),
               ih.dev<int64_t>(), (long long*)on.dev<int64_t>());
  const int ntile = (int)ceil_div(G, F2_T);
  const dim3 grid((unsigned)nb, (unsigned)(ntile * (ntile + 1) / 2));
  const int poly_f2 = (pr.poly_only & TPG_F2_POLY_F2) ? 1 : 0, poly_ap = (pr.poly_only & TPG_F2_POLY_AP) ? 1 : 0;
  const bool want_f2 = f2 || cnt, want_ap = ap || ap_cnt;
  const bool ap_rides = want_f2 && want_ap && poly_f2 == poly_ap;  // the same locus weights: ap out of the f2 pass
  if (want_f2)
    TPG_LAUNCH(ctx, "f2_gemm", f2_gemm_kernel<true>, grid, dim3(256), 0, src, G, ntile, il.dev<int64_t>(), ih.dev<int64_t>(),
               (const uint8_t*)d_flags, poly_f2, (int)(pr.apply_corr != 0), of.dev<double>(), oc.dev<int32_t>(),
               ap_rides ? oa.dev<double>() : (double*)nullptr, ap_rides ? oac.dev<int32_t>() : (int32_t*)nullptr);
  if (want_ap && !ap_rides)
    TPG_LAUNCH(ctx, "f2_gemm_ap", f2_gemm_kernel<false>, grid, dim3(256), 0, src, G, ntile, il.dev<int64_t>(), ih.dev<int64_t>(),
               (const uint8_t*)d_flags, poly_ap, 0, (double*)nullptr, (int32_t*)nullptr, oa.dev<double>(), oac.dev<int32_t>());
  TPG_CHECK_LAUNCH();
  TPG_HIP(hipStreamSynchronize(ctx->stream));  // the scratch of this call goes back to the pool at scope exit
  if (f2) TPG_TRY(of.commit(ctx));
  if (cnt) TPG_TRY(oc.commit(ctx));
  if (ap) TPG_TRY(oa.commit(ctx));
  if (ap_cnt) TPG_TRY(oac.commit(ctx));
  if (n_kept) TPG_TRY(on.commit(ctx));
  return TPG_OK;
}
