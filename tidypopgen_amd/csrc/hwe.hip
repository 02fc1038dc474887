// hwe.hip -- Hardy-Weinberg exact tests (loci_hwe, gt_grouped_hwe, hwe_on_matrix) on the device, right behind the count
// sweeps of loci.hip: the genotype tables never leave HBM, only the p-values do.
//
// The test itself is tpg_hwe_exact of host/host_hwe.h (the definition, the recurrence from the observed count and its
// error bound are stated there); compiled without FMA contraction like the other FP64 statistics.  One lane runs one
// test.  The loop is data dependent (its trip count is bounded by min(hom1, hom2) + het / 2), so lanes of a wave should
// hold tests of similar size: in the grouped kernel a wave holds 64 consecutive loci of ONE group (same sample size, the
// bound varies with the allele frequency only), and the p-values of a wave are 512 contiguous bytes of the column-major
// result.  The class-count planes have the class index fastest, so a workgroup first moves the tables of its 64 loci x 32
// groups through LDS (contiguous reads along the classes), as tpg_grouped_finalize_kernel does.
#include "common.h"
#include "host/host_hwe.h"

// what a kernel found wrong with its tables (tpg_hwe_exact_counts: the caller's own numbers)
#define HWE_BAD_NEGATIVE 1
#define HWE_BAD_TOO_LARGE 2

// counts = 3 x count, column-major {hom1, het, hom2}
__global__ __launch_bounds__(256) void tpg_hwe_table_kernel(const int32_t* __restrict__ counts3, int64_t count, int midp,
                                                            double* __restrict__ p, int32_t* __restrict__ bad) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = counts3[3 * i], h = counts3[3 * i + 1], b = counts3[3 * i + 2];
    if (a < 0 || h < 0 || b < 0) {
      atomicOr(bad, HWE_BAD_NEGATIVE);
      continue;
    }
    if (a + h + b >= TPG_HWE_MAX_N) {
      atomicOr(bad, HWE_BAD_TOO_LARGE);
      continue;
    }
    p[i] = tpg_hwe_exact(a, h, b, midp);
  }
}

// counts = m x 4 row-major {n0, n1, n2, nNA}, what tpg_launch_loci_counts leaves
__global__ __launch_bounds__(256) void tpg_hwe_loci_kernel(const int4* __restrict__ counts, int64_t m, int midp,
                                                           double* __restrict__ p) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const int4 c = counts[j];
    p[j] = tpg_hwe_exact(c.x, c.y, c.z, midp);
  }
}

// cnt[plane][locus][class] as tpg_grouped_counts leaves it (planes het, hom-alt, valid; Cpad classes per locus);
// p is m x G column-major.  A workgroup owns 64 consecutive loci.
__global__ __launch_bounds__(256) void tpg_hwe_grouped_kernel(const int32_t* __restrict__ cnt, int64_t Mpad, int Cpad,
                                                              int64_t m, int G, int midp, double* __restrict__ p) {
  __shared__ int32_t tab[3][32][65];  // [hom-ref, het, hom-alt][group of the chunk][locus]
  const int64_t j0 = (int64_t)blockIdx.x * 64, plane = Mpad * Cpad;
  for (int g0 = 0; g0 < G; g0 += 32) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * 32; idx += 256) {
      const int gl = idx & 31, l = idx >> 5;
      const int g = g0 + gl;
      const int64_t j = j0 + l;
      if (g < G && j < m) {
        const int64_t o = j * Cpad + g;
        const int n1 = cnt[o], n2 = cnt[plane + o], nv = cnt[2 * plane + o];
        tab[0][gl][l] = nv - n1 - n2;
        tab[1][gl][l] = n1;
        tab[2][gl][l] = n2;
      }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * 32; idx += 256) {
      const int l = idx & 63, gl = idx >> 6;
      const int g = g0 + gl;
      const int64_t j = j0 + l;
      if (g >= G || j >= m) continue;
      p[j + (int64_t)g * m] = tpg_hwe_exact(tab[0][gl][l], tab[1][gl][l], tab[2][gl][l], midp);
    }
  }
}

extern "C" int tpg_hwe_exact_counts(tpg_ctx* ctx, const int32_t* counts3, int64_t count, int midp, double* p) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && (count == 0 || (counts3 && p)), TPG_EINVAL, "null argument");
  TPG_REQUIRE(count >= 0, TPG_EINVAL, "negative number of tables");
  TPG_REQUIRE(midp == 0 || midp == 1, TPG_EINVAL, "midp must be 0 or 1");
  if (count == 0) return TPG_OK;
  InBuf in;
  TPG_TRY(in.init(ctx, counts3, sizeof(int32_t) * 3 * (size_t)count));
  OutBuf o;
  TPG_TRY(o.init(p, sizeof(double) * (size_t)count));
  DevBuf d_bad;
  TPG_TRY(d_bad.alloc_n<int32_t>(1));
  int32_t bad = 0;
  TPG_HIP(tpg_push_small(ctx, d_bad.p, &bad, sizeof(bad)));
  const unsigned grid = (unsigned)(ceil_div(count, 256) < 8192 ? ceil_div(count, 256) : 8192);
  TPG_LAUNCH(ctx, "hwe_table", tpg_hwe_table_kernel, dim3(grid), dim3(256), 0, in.dev<int32_t>(), count, midp,
             o.dev<double>(), d_bad.as<int32_t>());
  TPG_CHECK_LAUNCH();
  TPG_HIP(tpg_fetch_small(ctx, &bad, d_bad.p, sizeof(bad)));  // waits for the kernel
  TPG_REQUIRE(!(bad & HWE_BAD_NEGATIVE), TPG_EINVAL, "negative genotype count");
  TPG_REQUIRE(!(bad & HWE_BAD_TOO_LARGE), TPG_EUNSUPPORTED, "a table of 2^26 individuals or more");
  return o.commit(ctx);
}

extern "C" int tpg_loci_hwe(tpg_ctx* ctx, const tpg_view* v, int midp, double* p) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && p, TPG_EINVAL, "null argument");
  TPG_REQUIRE(midp == 0 || midp == 1, TPG_EINVAL, "midp must be 0 or 1");
  TPG_REQUIRE(v->n < TPG_HWE_MAX_N, TPG_EUNSUPPORTED, "exact test of 2^26 individuals or more");
  DevBuf d_counts;
  TPG_TRY(d_counts.alloc_n<int32_t>(4 * (size_t)v->m));
  TPG_TRY(tpg_launch_loci_counts(ctx, v, d_counts.as<int32_t>()));
  OutBuf o;
  TPG_TRY(o.init(p, sizeof(double) * (size_t)v->m));
  const unsigned grid = (unsigned)(ceil_div(v->m, 256) < 8192 ? ceil_div(v->m, 256) : 8192);
  TPG_LAUNCH(ctx, "hwe_loci", tpg_hwe_loci_kernel, dim3(grid), dim3(256), 0, (const int4*)d_counts.p, v->m, midp,
             o.dev<double>());
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  TPG_CHECK_LAUNCH();
  d_counts.free();
  return o.commit(ctx);
}

extern "C" int tpg_gt_grouped_hwe(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups, int midp,
                                  double* p) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && groupIds0 && p, TPG_EINVAL, "null argument");
  TPG_REQUIRE(midp == 0 || midp == 1, TPG_EINVAL, "midp must be 0 or 1");
  ClassPlan cp;
  TPG_TRY(make_class_plan(v->n, groupIds0, ngroups, nullptr, &cp));
  GroupedCounts gc;
  TPG_TRY(tpg_grouped_counts(ctx, v, cp.cls.data(), cp.nclass, &gc));  // (n < 2^24 there)
  OutBuf o;
  TPG_TRY(o.init(p, sizeof(double) * (size_t)v->m * (size_t)ngroups));
  TPG_LAUNCH(ctx, "hwe_grouped", tpg_hwe_grouped_kernel, dim3((unsigned)ceil_div(v->m, 64)), dim3(256), 0,
             (const int32_t*)gc.cnt, gc.Mpad, gc.Cpad, v->m, ngroups, midp, o.dev<double>());
  TPG_CHECK_LAUNCH();
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return o.commit(ctx);
}
