// tajima.hip -- Tajima's D per group, over the whole view and over windows of loci (include/tpg.h "Tajima's D").
//
// A restatement of the reference's R and C++, not a copy:
//   R/pop_tajimas_d.R:151-166           tajimas_d_from_pi_vec: seg, k_hat, a1, a2, e1, e2, D
//   src/gt_pi_diploid.cpp:22-35         pi of one locus, everybody in one group
//   src/gt_grouped_pi_diploid.cpp:24-38 pi of one locus and one group, no NA guard
//   R/windows_stats_generic.R:113-176   the window loop, n_loci and the min_loci rule
//   R/windows_pop_tajimas_d.R:69-102    one windows_stats_generic(operator = "custom") per group, n = 2 N_g
//
// seg and k_hat add over loci, so both entry points are segmented reductions behind the count sweep of
// tpg_grouped_counts (loci.hip), whose table stays in HBM:
//   whole view  tajima_chunk_sums reads the table with the class index on the fast lanes (a locus's classes are contiguous)
//               and leaves one (seg, k_hat, NaN count) per chunk of TPG_TAJIMA_CHUNK_LOCI loci and group; tajima_combine adds
//               the chunks of a group in a fixed order.  2 G words come down and D is formed on the host.
//   windows     tajima_pi stages pi once as an m x G column-major scratch (through an LDS transpose: table reads and pi
//               writes are both contiguous); tajima_windows reduces lo[w] .. hi[w]-1 of one column per workgroup, contiguous
//               8-byte loads, and forms D from the group's (a1, e1, e2).  Overlapping windows re-read 8 bytes per locus and
//               group instead of three strided count rows.
// Every sum has a fixed shape that depends on (lo, hi) or on m alone: per-thread strided partials, a butterfly over the wave,
// the waves of a workgroup in order.  No atomics.
#include "common.h"
#include "devfrag.h"

#include <math.h>
#include <string.h>

namespace {

constexpr int TAJ_CHUNK = TPG_TAJIMA_CHUNK_LOCI;

// a1, e1, e2 of n sampled alleles (R/pop_tajimas_d.R:158-163), in double, a1 and a2 summed in ascending order of i
void tajima_consts(int64_t n, double* a1, double* e1, double* e2) {
  double s1 = 0, s2 = 0;
  for (int64_t i = 1; i < n; i++) {
    s1 += 1.0 / (double)i;
    s2 += 1.0 / ((double)i * (double)i);
  }
  const double nd = (double)n;
  *a1 = s1;
  *e1 = ((nd + 1) / (3 * (nd - 1)) - 1 / s1) / s1;
  const double e2_num = 2 * (nd * nd + nd + 3) / (9 * nd * (nd - 1)) - (nd + 2) / (nd * s1) + s2 / (s1 * s1);
  *e2 = e2_num / (s1 * s1 + s2);
}

// D from the additive pieces (:164-165): plain IEEE arithmetic, S = 0 gives NaN or +Inf
__host__ __device__ inline double tajima_d(double k_hat, int64_t seg, double a1, double e1, double e2) {
  const double s = (double)seg;
  const double vd = e1 * s + e2 * s * (s - 1);
  return (k_hat - s / a1) / sqrt(vd);
}

// src/gt_grouped_pi_diploid.cpp:24-38, the expression of tpg_grouped_pi_kernel (loci.hip): NaN where nobody is typed
__device__ __forceinline__ double tajima_pi_of(const int32_t* __restrict__ cnt, int64_t plane, int64_t o) {
  const int n1 = cnt[o], n2 = cnt[plane + o], nv = cnt[2 * plane + o];
  const double x = (double)(n1 + 2 * n2), v = (double)(2 * nv);
  return x * (v - x) / (v * (v - 1) / 2);
}

struct TajAcc {
  double k = 0;        // sum of the non-NaN pi
  long long seg = 0;   // 0 < pi < 1
  long long cnt = 0;   // non-NaN pi
  __device__ __forceinline__ void add(double pi) {
    if (pi == pi) { k += pi; cnt++; }
    if (pi > 0.0 && pi < 1.0) seg++;
  }
};

// m x G column-major pi from the count table.  A workgroup owns 64 loci: reads with the class on the lanes, writes with the
// locus on the lanes (as tpg_grouped_finalize_kernel does).
__global__ __launch_bounds__(256) void tajima_pi_kernel(const int32_t* __restrict__ cnt, int64_t Mpad, int Cpad, int64_t m, int G,
                                                        double* __restrict__ pi) {
  __shared__ double tile[32][65];
  const int64_t j0 = (int64_t)blockIdx.x * 64, plane = Mpad * Cpad;
  for (int g0 = 0; g0 < G; g0 += 32) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * 32; idx += 256) {
      const int gl = idx & 31, l = idx >> 5;
      if (g0 + gl < G && j0 + l < m) tile[gl][l] = tajima_pi_of(cnt, plane, (j0 + l) * Cpad + g0 + gl);
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * 32; idx += 256) {
      const int l = idx & 63, gl = idx >> 6;
      if (g0 + gl < G && j0 + l < m) pi[j0 + l + (int64_t)(g0 + gl) * m] = tile[gl][l];
    }
  }
}

// whole view, stage 1: block (chunk c, group tile t) -> part[(c * G + g)] for the groups 32 t .. 32 t + 31.  Thread (gl, s)
// walks the loci j0 + s, j0 + s + 8, ... of group 32 t + gl; the eight partials of a group are added in the order of s.
__global__ __launch_bounds__(256) void tajima_chunk_sums_kernel(const int32_t* __restrict__ cnt, int64_t Mpad, int Cpad, int64_t m,
                                                                int G, double* __restrict__ part_k, long long* __restrict__ part_seg,
                                                                long long* __restrict__ part_cnt) {
  __shared__ double sk[8][32];
  __shared__ long long sseg[8][32], scnt[8][32];
  const int gl = threadIdx.x & 31, s = threadIdx.x >> 5;
  const int g = blockIdx.y * 32 + gl;
  const int64_t j0 = (int64_t)blockIdx.x * TAJ_CHUNK, plane = Mpad * Cpad;
  const int64_t j1 = j0 + TAJ_CHUNK < m ? j0 + TAJ_CHUNK : m;
  TajAcc a;
  if (g < G)
    for (int64_t j = j0 + s; j < j1; j += 8) a.add(tajima_pi_of(cnt, plane, j * Cpad + g));
  sk[s][gl] = a.k; sseg[s][gl] = a.seg; scnt[s][gl] = a.cnt;
  __syncthreads();
  if (s == 0 && g < G) {
    for (int t = 1; t < 8; t++) { a.k += sk[t][gl]; a.seg += sseg[t][gl]; a.cnt += scnt[t][gl]; }
    const int64_t o = (int64_t)blockIdx.x * G + g;
    part_k[o] = a.k; part_seg[o] = a.seg; part_cnt[o] = a.cnt;
  }
}

__device__ __forceinline__ void tajima_wave_sum(TajAcc& a) {
  for (int o = 32; o > 0; o >>= 1) {
    a.k += __shfl_xor(a.k, o);
    a.seg += __shfl_xor(a.seg, o);
    a.cnt += __shfl_xor(a.cnt, o);
  }
}

// whole view, stage 2: one wave per group adds its chunks (lane l: chunks l, l + 64, ...; then the butterfly).
// out_k[g] = k_hat (NaN as soon as one locus of the group has no typed individual), out_seg[g] = seg
__global__ __launch_bounds__(64) void tajima_combine_kernel(const double* __restrict__ part_k, const long long* __restrict__ part_seg,
                                                            const long long* __restrict__ part_cnt, int64_t nchunks, int G, int64_t m,
                                                            double* __restrict__ out_k, long long* __restrict__ out_seg) {
  const int g = blockIdx.x;
  TajAcc a;
  for (int64_t c = threadIdx.x; c < nchunks; c += 64) {
    a.k += part_k[c * G + g]; a.seg += part_seg[c * G + g]; a.cnt += part_cnt[c * G + g];
  }
  tajima_wave_sum(a);
  if (threadIdx.x == 0) {
    out_k[g] = a.cnt == m ? a.k : TPG_QNAN;
    out_seg[g] = a.seg;
  }
}

// one workgroup per (window, group): thread t takes the loci lo + t, lo + t + 256, ... of column g of pi; butterfly over each
// wave, the four waves in order.  consts = (a1, e1, e2) per group.
__global__ __launch_bounds__(256) void tajima_windows_kernel(const double* __restrict__ pi, int64_t m, const int64_t* __restrict__ lo,
                                                             const int64_t* __restrict__ hi, const uint8_t* __restrict__ pad_na,
                                                             int64_t nw, int min_loci, const double* __restrict__ consts,
                                                             double* __restrict__ d, long long* __restrict__ seg,
                                                             double* __restrict__ k_hat, int32_t* __restrict__ n_loci) {
  __shared__ double sk[4];
  __shared__ long long sseg[4], scnt[4];
  const int64_t w = blockIdx.x;
  const int g = blockIdx.y;
  const bool pad = pad_na && pad_na[w];
  const int64_t j0 = lo[w], j1 = pad ? j0 : hi[w];
  const double* __restrict__ col = pi + (int64_t)g * m;
  TajAcc a;
  for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) a.add(col[j]);
  tajima_wave_sum(a);
  if ((threadIdx.x & 63) == 0) { sk[threadIdx.x >> 6] = a.k; sseg[threadIdx.x >> 6] = a.seg; scnt[threadIdx.x >> 6] = a.cnt; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int t = 1; t < 4; t++) { a.k += sk[t]; a.seg += sseg[t]; a.cnt += scnt[t]; }
  const int64_t o = w + (int64_t)g * nw;
  const double a1 = consts[3 * g];  // NaN for a group nobody belongs to: k_hat is NaN there even over an empty window
  const double k = (pad || a.cnt != j1 - j0 || a1 != a1) ? TPG_QNAN : a.k;
  double r = TPG_QNAN;
  if (!pad && a.cnt >= min_loci) r = tajima_d(k, a.seg, a1, consts[3 * g + 1], consts[3 * g + 2]);
  d[o] = r;
  if (seg) seg[o] = a.seg;
  if (k_hat) k_hat[o] = k;
  if (n_loci) n_loci[o] = pad ? -1 : (int32_t)a.cnt;
}

// the class plan (group of every individual, group sizes) and (a1, e1, e2) per group; stopifnot_diploid (R/pop_tajimas_d.R:62, :108)
struct TajPlan : ClassPlan {
  std::vector<double> consts;  // 3 G
};

int tajima_plan(const tpg_view* v, const int32_t* groupIds0, int ngroups, const double* ploidy, TajPlan* p) {
  TPG_REQUIRE(ngroups >= 1 && ngroups <= 65535, TPG_EINVAL, "ngroups = %d out of [1, 65535]", ngroups);
  TPG_TRY(tpg_require_diploid(v->n, ploidy, "Tajima's D"));
  TPG_TRY(make_class_plan(v->n, groupIds0, ngroups, nullptr, p));
  p->consts.assign((size_t)3 * ngroups, NAN);  // a group nobody belongs to: NaN throughout
  for (int g = 0; g < ngroups; g++)
    if (p->group_size[(size_t)g] > 0)
      tajima_consts(2 * (int64_t)p->group_size[(size_t)g], &p->consts[3 * g], &p->consts[3 * g + 1], &p->consts[3 * g + 2]);
  return TPG_OK;
}

}  // namespace

extern "C" int64_t tpg_tajima_chunk_loci(void) { return TAJ_CHUNK; }

extern "C" int tpg_tajimas_d_from_sums(int64_t n_alleles, int64_t seg, double k_hat, double* d) {
  TPG_REQUIRE(d, TPG_EINVAL, "null argument");
  TPG_REQUIRE(n_alleles >= 2 && n_alleles <= 2147483647ll, TPG_EINVAL, "n_alleles = %lld: at least 2 sampled alleles",
              (long long)n_alleles);
  TPG_REQUIRE(seg >= 0, TPG_EINVAL, "seg = %lld is negative", (long long)seg);
  double a1, e1, e2;
  tajima_consts(n_alleles, &a1, &e1, &e2);
  *d = tajima_d(k_hat, seg, a1, e1, e2);
  return TPG_OK;
}

extern "C" int tpg_pop_tajimas_d(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups, const double* ploidy,
                                 double* d, int64_t* seg, double* k_hat) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && d, TPG_EINVAL, "null argument");
  TajPlan pl;
  TPG_TRY(tajima_plan(v, groupIds0, ngroups, ploidy, &pl));
  GroupedCounts gc;
  TPG_TRY(tpg_grouped_counts(ctx, v, pl.cls.data(), ngroups, &gc));
  const int G = ngroups;
  const int64_t m = v->m, nchunks = ceil_div(m, TAJ_CHUNK);
  DevArena sc;
  double *d_pk = nullptr, *d_out = nullptr;
  long long *d_pseg = nullptr, *d_pcnt = nullptr;
  TPG_TRY(sc.get(&d_pk, (size_t)nchunks * G));
  TPG_TRY(sc.get(&d_pseg, (size_t)nchunks * G));
  TPG_TRY(sc.get(&d_pcnt, (size_t)nchunks * G));
  TPG_TRY(sc.get(&d_out, (size_t)2 * G));  // k_hat[G], then seg[G] as 8-byte integers
  if (nchunks > 0)
    TPG_LAUNCH(ctx, "tajima_chunk_sums", tajima_chunk_sums_kernel, dim3((unsigned)nchunks, (unsigned)ceil_div(G, 32)), dim3(256), 0,
               (const int32_t*)gc.cnt, gc.Mpad, gc.Cpad, m, G, d_pk, d_pseg, d_pcnt);
  TPG_LAUNCH(ctx, "tajima_combine", tajima_combine_kernel, dim3((unsigned)G), dim3(64), 0, (const double*)d_pk,
             (const long long*)d_pseg, (const long long*)d_pcnt, nchunks, G, m, d_out, (long long*)(d_out + G));
  TPG_CHECK_LAUNCH();
  std::vector<double> out((size_t)2 * G);
  TPG_HIP(tpg_download(ctx, out.data(), d_out, sizeof(double) * out.size()));  // waits for the stream
  for (int g = 0; g < G; g++) {
    int64_t s;
    memcpy(&s, &out[(size_t)G + g], sizeof s);
    const double k = pl.group_size[(size_t)g] > 0 ? out[(size_t)g] : NAN;
    d[g] = tajima_d(k, s, pl.consts[3 * g], pl.consts[3 * g + 1], pl.consts[3 * g + 2]);
    if (seg) seg[g] = s;
    if (k_hat) k_hat[g] = k;
  }
  return TPG_OK;
}

extern "C" int tpg_windows_pop_tajimas_d(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups,
                                         const double* ploidy, const int64_t* lo, const int64_t* hi, const uint8_t* pad_na,
                                         int64_t nw, int min_loci, double* d, int64_t* seg, double* k_hat, int32_t* n_loci) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && lo && hi && d, TPG_EINVAL, "null argument");
  // one workgroup of 256 threads per window in grid.x: the launch takes fewer than 2^32 threads in that dimension
  TPG_REQUIRE(nw >= 0 && nw <= TPG_TAJIMA_MAX_WINDOWS, TPG_EINVAL, "nw = %lld out of [0, %lld]", (long long)nw,
              (long long)TPG_TAJIMA_MAX_WINDOWS);
  TPG_REQUIRE(min_loci >= 1, TPG_EINVAL, "min_loci must be positive");
  TajPlan pl;
  TPG_TRY(tajima_plan(v, groupIds0, ngroups, ploidy, &pl));
  if (nw == 0) return TPG_OK;
  const int G = ngroups;
  const int64_t m = v->m;
  TPG_TRY(tpg_check_ranges(ctx, lo, hi, nw, m, "window"));
  GroupedCounts gc;
  TPG_TRY(tpg_grouped_counts(ctx, v, pl.cls.data(), G, &gc));
  InBuf il, ih, ip, ic;
  TPG_TRY(il.init(ctx, lo, sizeof(int64_t) * (size_t)nw));
  TPG_TRY(ih.init(ctx, hi, sizeof(int64_t) * (size_t)nw));
  if (pad_na) TPG_TRY(ip.init(ctx, pad_na, (size_t)nw));
  TPG_TRY(ic.init(ctx, pl.consts.data(), sizeof(double) * pl.consts.size()));
  const size_t cells = (size_t)nw * (size_t)G;
  OutBuf od, os, ok, on;
  TPG_TRY(od.init(d, sizeof(double) * cells));
  if (seg) TPG_TRY(os.init(seg, sizeof(int64_t) * cells));
  if (k_hat) TPG_TRY(ok.init(k_hat, sizeof(double) * cells));
  if (n_loci) TPG_TRY(on.init(n_loci, sizeof(int32_t) * cells));
  DevArena sc;
  double* d_pi = nullptr;
  TPG_TRY(sc.get(&d_pi, (size_t)m * (size_t)G));
  TPG_LAUNCH(ctx, "tajima_pi", tajima_pi_kernel, dim3((unsigned)ceil_div(m, 64)), dim3(256), 0, (const int32_t*)gc.cnt, gc.Mpad,
             gc.Cpad, m, G, d_pi);
  TPG_LAUNCH(ctx, "tajima_windows", tajima_windows_kernel, dim3((unsigned)nw, (unsigned)G), dim3(256), 0, (const double*)d_pi, m,
             il.dev<int64_t>(), ih.dev<int64_t>(), pad_na ? ip.dev<uint8_t>() : (const uint8_t*)nullptr, nw, min_loci,
             ic.dev<double>(), od.dev<double>(), (long long*)os.dev<int64_t>(), ok.dev<double>(), on.dev<int32_t>());
  TPG_CHECK_LAUNCH();
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  TPG_TRY(od.commit(ctx));
  if (seg) TPG_TRY(os.commit(ctx));
  if (k_hat) TPG_TRY(ok.commit(ctx));
  if (n_loci) TPG_TRY(on.commit(ctx));
  return TPG_OK;
}
