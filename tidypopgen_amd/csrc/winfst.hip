// winfst.hip -- windowed pairwise Fst (include/tpg.h "windowed pairwise Fst"): from the view's cached count table straight to
// nw x P window means of the per-locus numerators and denominators and their ratio.  The m x P by-locus matrices that
// tpg_pairwise_pop_fst(return_num_dem = 1) + tpg_window_stats go through are never formed.
//
// A restatement of the reference's R, not a copy:
//   R/windows_pairwise_pop_fst.R:62-107   by-locus Hudson num / den, one windows_stats_generic(operator = "mean") each, ratio
//   R/windows_stats_generic.R:113-179     the window loop, n_loci and the min_loci rule
// The per-locus terms are fst.hip's own (fst_terms.h: fst_stage and fst_terms<METHOD, false>, statement order, no FMA
// contraction), so every term is the double the by-locus path writes.
//
// Shape of the work, with C = TPG_WINFST_CHUNK_LOCI loci per chunk, chunks aligned to locus 0:
//   winfst_chunks   walks every WHOLE chunk once: (n, p, h) or (p, e) of LB loci x G populations staged in LDS as
//                   tpg_fst_kernel stages them ([locus][population]: the pairs of a wave read one population broadcast and
//                   consecutive populations, conflict-free), a thread owns 1 or 8 pairs and adds the chunk's terms in
//                   ascending locus order.  Leaves (sum num, sum den) and (n_num, n_den) per (chunk, pair): 24 bytes.
//   winfst_windows  one workgroup per (window, tile of pairs): the head loci up to the next chunk border evaluated from the
//                   table, the whole chunks' sums in ascending order, the tail loci evaluated from the table -- one fixed order
//                   that depends on (lo, hi) alone.  A window with no whole chunk inside is evaluated locus by locus.  Applies
//                   min_loci and pad_na and writes the outputs.
// Pair-locus evaluations: at most m P + 2 C nw P.  No atomics.
#include <algorithm>

#include "common.h"
#include "fst_terms.h"

namespace {

constexpr int WF_CHUNK = TPG_WINFST_CHUNK_LOCI;
static_assert(WF_CHUNK >= 32 && (WF_CHUNK & (WF_CHUNK - 1)) == 0, "TPG_WINFST_CHUNK_LOCI: a power of two, at least 32");
constexpr size_t WF_LDS_MAX = 64 * 1024;  // staged doubles of one workgroup: three to four workgroups share a CU's 160 KiB

// doubles staged per (locus, population): Hudson reads p and e = p q / (n - 1), WC84 and Nei87 read n, p and het_obs
__host__ __device__ constexpr int wf_arrays(int method) { return method == TPG_FST_HUDSON ? 2 : 3; }

// the count table alone: what fst_stage reads of an FstSrc on the fused path (the kernels below never see the m x G matrices of
// the loop mirror, so their pointers need no registers)
struct WfSrc {
  const int32_t* cnt;
  int64_t Mpad;
  int Cpad;
  int has_hap;
  __device__ __forceinline__ FstSrc fst_src() const {
    __builtin_assume(cnt != nullptr);
    return FstSrc{cnt, Mpad, Cpad, has_hap, nullptr, nullptr, nullptr, nullptr};
  }
};

template <int PPT>
struct WfAcc {
  double sn[PPT], sd[PPT];  // sums of the non-NaN numerators / denominators
  int cn[PPT], cd[PPT];     // how many of each
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int k = 0; k < PPT; k++) { sn[k] = 0.0; sd[k] = 0.0; cn[k] = 0; cd[k] = 0; }
  }
};

// this thread's pairs: pair p0 + 256 k with p0 = blockIdx.y * PPT * 256 + threadIdx.x, those below P
template <int PPT>
struct WfPairs {
  int p0, P, g1[PPT], g2[PPT];
  __device__ __forceinline__ int pidx(int k) const { return p0 + 256 * k; }
  __device__ __forceinline__ bool has(int k) const { return p0 + 256 * k < P; }
  __device__ __forceinline__ void load(const int32_t* __restrict__ pairs0, int P_) {
    p0 = blockIdx.y * PPT * 256 + threadIdx.x;
    P = P_;
#pragma unroll
    for (int k = 0; k < PPT; k++) {
      g1[k] = 0; g2[k] = 0;
      if (has(k)) { g1[k] = pairs0[2 * pidx(k)]; g2[k] = pairs0[2 * pidx(k) + 1]; }
    }
  }
};

// adds the terms of the loci ja .. jb-1 (inside [0, m)) to `a`, one by one in ascending locus order; the whole workgroup calls
// it with the same (ja, jb).  LB loci are staged at a time.
template <int METHOD, int PPT>
__device__ __forceinline__ void wf_walk(const FstSrc& src, int64_t m, int G, int LB, int64_t ja, int64_t jb, double* sh,
                                        const WfPairs<PPT>& pr, WfAcc<PPT>& a) {
  double* sh_a = sh;
  double* sh_b = sh + (size_t)LB * G;
  double* sh_c = sh + 2 * (size_t)LB * G;
  for (int64_t j0 = ja; j0 < jb; j0 += LB) {
    const int lmax = (int)((jb - j0) < LB ? (jb - j0) : LB);
    __syncthreads();
    for (int idx = threadIdx.x; idx < lmax * G; idx += 256) {
      const int l = idx / G, g = idx % G;
      double vn, vp, vh;
      fst_stage(src, m, j0 + l, g, vn, vp, vh);
      if (METHOD == TPG_FST_HUDSON) {
        sh_a[idx] = vp;
        sh_b[idx] = (vp * (1 - vp)) / (vn - 1);  // (p q) / (n - 1), once per population: tpg_fst_kernel's expression
      } else {
        sh_a[idx] = vn; sh_b[idx] = vp; sh_c[idx] = vh;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PPT; k++) {
      if (!pr.has(k)) continue;
      double sn = a.sn[k], sd = a.sd[k];
      int cn = a.cn[k], cd = a.cd[k];
#pragma unroll 1
      for (int l = 0; l < lmax; l++) {
        const int o1 = l * G + pr.g1[k], o2 = l * G + pr.g2[k];
        double num, den;
        if (METHOD == TPG_FST_HUDSON)
          fst_terms<METHOD, false>(0.0, sh_a[o1], 0.0, sh_b[o1], 0.0, sh_a[o2], 0.0, sh_b[o2], num, den);
        else
          fst_terms<METHOD, false>(sh_a[o1], sh_b[o1], sh_c[o1], 0.0, sh_a[o2], sh_b[o2], sh_c[o2], 0.0, num, den);
        if (num == num) { sn += num; cn++; }  // counted separately: the reference's two windows_stats_generic calls
        if (den == den) { sd += den; cd++; }
      }
      a.sn[k] = sn; a.sd[k] = sd; a.cn[k] = cn; a.cd[k] = cd;
    }
  }
}

// chunk c = loci C c .. C c + C - 1, whole chunks only (nfull = m / C): psum[c * P + pair] = (sum num, sum den),
// pcnt[c * P + pair] = (n_num, n_den)
template <int METHOD, int PPT>
__global__ __launch_bounds__(256) void winfst_chunk_kernel(WfSrc wsrc, int64_t m, int G, int LB, const int32_t* __restrict__ pairs0,
                                                           int P, int64_t nfull, double2* __restrict__ psum, int2* __restrict__ pcnt) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  const FstSrc src = wsrc.fst_src();
  WfPairs<PPT> pr;
  pr.load(pairs0, P);
  for (int64_t c = blockIdx.x; c < nfull; c += gridDim.x) {
    WfAcc<PPT> a;
    a.zero();
    wf_walk<METHOD, PPT>(src, m, G, LB, c * WF_CHUNK, c * WF_CHUNK + WF_CHUNK, sh, pr, a);
#pragma unroll
    for (int k = 0; k < PPT; k++)
      if (pr.has(k)) {
        psum[c * P + pr.pidx(k)] = make_double2(a.sn[k], a.sd[k]);
        pcnt[c * P + pr.pidx(k)] = make_int2(a.cn[k], a.cd[k]);
      }
  }
}

// workgroup (window w, pair tile): head loci, whole chunks, tail loci, in that order; outputs nw x P column-major
template <int METHOD, int PPT>
__global__ __launch_bounds__(256) void winfst_window_kernel(WfSrc wsrc, int64_t m, int G, int LB, const int32_t* __restrict__ pairs0,
                                                            int P, const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                                                            const uint8_t* __restrict__ pad_na, int64_t nw, int min_loci,
                                                            const double2* __restrict__ psum, const int2* __restrict__ pcnt,
                                                            double* __restrict__ fst, double* __restrict__ mean_num,
                                                            double* __restrict__ mean_den, int32_t* __restrict__ n_num,
                                                            int32_t* __restrict__ n_den) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  const FstSrc src = wsrc.fst_src();
  WfPairs<PPT> pr;
  pr.load(pairs0, P);
  const int64_t w = blockIdx.x;
  const bool pad = pad_na && pad_na[w];
  const int64_t j0 = lo[w], j1 = pad ? j0 : hi[w];
  const int64_t b0 = (j0 + WF_CHUNK - 1) / WF_CHUNK * WF_CHUNK, b1 = j1 / WF_CHUNK * WF_CHUNK;
  WfAcc<PPT> a;
  a.zero();
  // no whole chunk inside (b0 >= b1): the head is the whole window, no chunks, an empty tail
  const bool whole = b0 < b1;
  const int64_t c0 = whole ? b0 / WF_CHUNK : 0, c1 = whole ? b1 / WF_CHUNK : 0;
#pragma unroll 1
  for (int part = 0; part < 2; part++) {  // (one copy of the walk in the code: head and tail differ by their bounds)
    const int64_t ja = part == 0 ? j0 : (whole ? b1 : j1), jb = part == 0 ? (whole ? b0 : j1) : j1;
    wf_walk<METHOD, PPT>(src, m, G, LB, ja, jb, sh, pr, a);
    if (part == 1) break;
    for (int64_t c = c0; c < c1; c++) {  // a chunk's pairs are contiguous: the eight loads of a thread are in flight together
      const double2* __restrict__ ps = psum + c * P + pr.p0;
      const int2* __restrict__ pc = pcnt + c * P + pr.p0;
#pragma unroll
      for (int k = 0; k < PPT; k++) {
        if (!pr.has(k)) continue;
        const double2 s = ps[256 * k];
        const int2 n = pc[256 * k];
        a.sn[k] += s.x; a.sd[k] += s.y; a.cn[k] += n.x; a.cd[k] += n.y;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < PPT; k++) {
    if (!pr.has(k)) continue;
    const int64_t o = w + (int64_t)pr.pidx(k) * nw;
    const double mn = (pad || a.cn[k] == 0 || a.cn[k] < min_loci) ? TPG_QNAN : a.sn[k] / (double)a.cn[k];
    const double md = (pad || a.cd[k] == 0 || a.cd[k] < min_loci) ? TPG_QNAN : a.sd[k] / (double)a.cd[k];
    fst[o] = mn / md;
    if (mean_num) mean_num[o] = mn;
    if (mean_den) mean_den[o] = md;
    if (n_num) n_num[o] = pad ? -1 : a.cn[k];
    if (n_den) n_den[o] = pad ? -1 : a.cd[k];
  }
}

// the scratch block of one call: [psum: nfull P double2][pcnt: nfull P int2][pairs0: 2 P int32]
struct WfScratch {
  int64_t nfull, psum_bytes, pcnt_bytes, pairs_bytes;
  int64_t total() const { return psum_bytes + pcnt_bytes + pairs_bytes; }
};
WfScratch wf_scratch(int64_t m, int P) {
  WfScratch s;
  s.nfull = m / WF_CHUNK;
  s.psum_bytes = s.nfull * P * (int64_t)sizeof(double2);
  s.pcnt_bytes = s.nfull * P * (int64_t)sizeof(int2);
  s.pairs_bytes = 2 * (int64_t)P * (int64_t)sizeof(int32_t);
  return s;
}

}  // namespace

extern "C" int64_t tpg_winfst_chunk_loci(void) { return WF_CHUNK; }

extern "C" int64_t tpg_windows_fst_scratch_bytes(int64_t m, int ngroups, int P, int64_t nw) {
  if (m < 0 || ngroups < 1 || P < 1 || nw < 0) return -1;
  return wf_scratch(m, P).total();
}

extern "C" int tpg_windows_pairwise_pop_fst(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups,
                                            const double* ploidy, int method, const int32_t* pairs1, int P, const int64_t* lo,
                                            const int64_t* hi, const uint8_t* pad_na, int64_t nw, int min_loci, double* fst,
                                            double* mean_num, double* mean_den, int32_t* n_num, int32_t* n_den) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && groupIds0, TPG_EINVAL, "null argument");
  TPG_REQUIRE(method == TPG_FST_HUDSON || method == TPG_FST_NEI87 || method == TPG_FST_WC84, TPG_EINVAL,
              "unknown Fst method %d", method);
  TPG_REQUIRE(P >= 1 && pairs1, TPG_EINVAL, "no population pairs");
  // one workgroup row per window in grid.x
  TPG_REQUIRE(nw >= 0 && nw <= TPG_WINFST_MAX_WINDOWS, TPG_EINVAL, "nw = %lld out of [0, %lld]", (long long)nw,
              (long long)TPG_WINFST_MAX_WINDOWS);
  TPG_REQUIRE(min_loci >= 1, TPG_EINVAL, "min_loci must be positive");
  ClassPlan cp;
  TPG_TRY(make_class_plan(v->n, groupIds0, ngroups, ploidy, &cp));
  // R/pairwise_pop_fst.R:110-115: pseudohaploids only with Hudson
  TPG_REQUIRE(!cp.has_hap || method == TPG_FST_HUDSON, TPG_EINVAL,
              "only method = Hudson is valid when the data include pseudohaploids");
  const int G = ngroups;
  std::vector<int32_t> p0((size_t)2 * P);
  for (int k = 0; k < 2 * P; k++) {
    TPG_REQUIRE(pairs1[k] >= 1 && pairs1[k] <= G, TPG_EINVAL, "pairwise_combn[%d] = %d out of [1,%d]", k, pairs1[k], G);
    p0[(size_t)k] = pairs1[k] - 1;
  }
  if (nw == 0) return TPG_OK;
  TPG_REQUIRE(lo && hi && fst, TPG_EINVAL, "null argument");
  const int64_t m = v->m;
  TPG_TRY(tpg_check_ranges(ctx, lo, hi, nw, m, "window"));
  const int NA = wf_arrays(method);
  int LB = WF_CHUNK;
  while (LB > 1 && (size_t)LB * G * NA * sizeof(double) > WF_LDS_MAX) LB /= 2;
  const size_t shmem = (size_t)LB * G * NA * sizeof(double);
  TPG_REQUIRE(shmem <= WF_LDS_MAX, TPG_EUNSUPPORTED, "too many populations (%d)", G);
  GroupedCounts gc;
  TPG_TRY(tpg_grouped_counts(ctx, v, cp.cls.data(), cp.nclass, &gc));
  const WfSrc src{gc.cnt, gc.Mpad, gc.Cpad, cp.has_hap};
  InBuf il, ih, ip;
  TPG_TRY(il.init(ctx, lo, sizeof(int64_t) * (size_t)nw));
  TPG_TRY(ih.init(ctx, hi, sizeof(int64_t) * (size_t)nw));
  if (pad_na) TPG_TRY(ip.init(ctx, pad_na, (size_t)nw));
  const size_t cells = (size_t)nw * (size_t)P;
  OutBuf of, omn, omd, onn, ond;
  TPG_TRY(of.init(fst, sizeof(double) * cells));
  if (mean_num) TPG_TRY(omn.init(mean_num, sizeof(double) * cells));
  if (mean_den) TPG_TRY(omd.init(mean_den, sizeof(double) * cells));
  if (n_num) TPG_TRY(onn.init(n_num, sizeof(int32_t) * cells));
  if (n_den) TPG_TRY(ond.init(n_den, sizeof(int32_t) * cells));
  // the call's scratch: exactly tpg_windows_fst_scratch_bytes(m, G, P, nw)
  const WfScratch ws = wf_scratch(m, P);
  DevBuf sc;
  TPG_TRY(sc.alloc((size_t)ws.total()));
  double2* const d_psum = (double2*)sc.p;
  int2* const d_pcnt = (int2*)((char*)sc.p + ws.psum_bytes);
  int32_t* const d_pairs = (int32_t*)((char*)sc.p + ws.psum_bytes + ws.pcnt_bytes);
  TPG_HIP(tpg_h2d_async(ctx, d_pairs, p0.data(), (size_t)ws.pairs_bytes));
  const int ppt = P > 256 ? 8 : 1;
  const unsigned ypass = (unsigned)ceil_div(P, 256 * ppt);
  const unsigned cgrid = (unsigned)std::min<int64_t>(ws.nfull, (int64_t)1 << 20);
  const uint8_t* d_pad = pad_na ? ip.dev<uint8_t>() : (const uint8_t*)nullptr;
#define WF_LAUNCH1(M, PP)                                                                                                          \
  do {                                                                                                                             \
    (void)hipFuncSetAttribute((const void*)winfst_chunk_kernel<M, PP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);     \
    (void)hipFuncSetAttribute((const void*)winfst_window_kernel<M, PP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);    \
    if (ws.nfull > 0)                                                                                                              \
      TPG_LAUNCH(ctx, "winfst_chunks", (winfst_chunk_kernel<M, PP>), dim3(cgrid, ypass), dim3(256), shmem, src, m, G, LB,           \
                 (const int32_t*)d_pairs, P, ws.nfull, d_psum, d_pcnt);                                                            \
    TPG_LAUNCH(ctx, "winfst_windows", (winfst_window_kernel<M, PP>), dim3((unsigned)nw, ypass), dim3(256), shmem, src, m, G, LB,    \
               (const int32_t*)d_pairs, P, il.dev<int64_t>(), ih.dev<int64_t>(), d_pad, nw, min_loci, (const double2*)d_psum,      \
               (const int2*)d_pcnt, of.dev<double>(), omn.dev<double>(), omd.dev<double>(), onn.dev<int32_t>(),                    \
               ond.dev<int32_t>());                                                                                                \
  } while (0)
#define WF_LAUNCH(M) do { if (ppt == 8) WF_LAUNCH1(M, 8); else WF_LAUNCH1(M, 1); } while (0)
  if (method == TPG_FST_HUDSON) WF_LAUNCH(TPG_FST_HUDSON);
  else if (method == TPG_FST_WC84) WF_LAUNCH(TPG_FST_WC84);
  else WF_LAUNCH(TPG_FST_NEI87);
#undef WF_LAUNCH
#undef WF_LAUNCH1
  TPG_CHECK_LAUNCH();
  sc.free();  // stream-ordered: commit() waits for host outputs
  TPG_TRY(of.commit(ctx));
  if (mean_num) TPG_TRY(omn.commit(ctx));
  if (mean_den) TPG_TRY(omd.commit(ctx));
  if (n_num) TPG_TRY(onn.commit(ctx));
  if (n_den) TPG_TRY(ond.commit(ctx));
  return TPG_OK;
}
