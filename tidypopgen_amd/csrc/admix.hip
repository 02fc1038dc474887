// admix.hip -- maximum-likelihood ancestry proportions by EM (include/tpg.h "admixture").
//
// ADMIXTURE is not among the reference's sources (R/gt_admixture.R:86-100 exports the panel, runs an outside binary and reads
// its .Q / .P files back), so the model, the EM step and the stop rule are the ones include/tpg.h defines.
//
// The state lives on the device as Qd[i * KT + k] and Fd[j * KT + k]: a row per individual / locus, padded from K to the
// dispatch width KT in {1, 2, 3, 4, 8, 16, 32} with q = 0 and f = 0.5.  A padded term adds q f = +0 to p and to p-bar, so the
// sums over KT equal the sums over K bit for bit and the hot loops carry no bound check on k.
//
// One iteration is two sweeps of the packed panel, both of the same shape: a workgroup of four waves owns 32 "row" entities
// (lane r and r + 32 share one) and walks the other axis in blocks of 128, whose state rows are staged through LDS (128 KT
// doubles; every lane of a half-wave reads the same row: a broadcast).  Wave w takes dword w of each 16-byte lane fragment
// (common.h: 16 codes), so a thread sees the entities 128 b + 32 w + 16 h + e, e = 0 .. 15, of every block b in ascending
// order.  p and p-bar are recomputed from Q and F for every typed entry: K fused multiply-adds each.
//   F sweep  rows = the 32 loci of tile lt of L, walked axis = all individuals; registers f, 1 - f, A, B (4 KT doubles);
//            the same pass adds ln(p^g pbar^(2 - g)) per entry: the likelihood of the OLD state (UPD = false: that alone).
//   Q sweep  rows = the 32 individuals of row tile rt of T, walked axis = one chunk of TPG_ADMIX_CHUNK_LOCI loci; registers q, S
//            (2 KT doubles); partials to part[chunk][i][k], added in ascending chunk order by admix_q_combine.
// Every sum has a fixed shape: a thread's entries in ascending order, lane r + lane r + 32, then the four waves in order (and
// for the likelihood a butterfly over the wave, the waves in order, the tiles by a one-workgroup kernel).  No atomics on
// floating point; the only atomic is the integer OR of the Q0 / F0 validation flag.
#include "admix_common.h"
#include "host/host_squarem.h"

namespace {

// ---- start, validation (the frequencies; admix_common.h has Q's) ------------------------------------------------------
__global__ void admix_seed_f_kernel(double* __restrict__ Fd, int64_t m, int K, int KT, uint64_t seed) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const uint64_t key = tpg_mix64((seed ^ ADM_F_SALT) ^ tpg_mix64((uint64_t)j));
  for (int k = 0; k < KT; k++) Fd[j * KT + k] = k < K ? 0.1 + 0.8 * admix_u(tpg_mix64(key ^ tpg_mix64((uint64_t)k))) : 0.5;
}

// f0 (m x K column-major) -> Fd, clamped; clamp = false: as given.  bit 1 of *flag: an entry that is not finite
__global__ void admix_load_f_kernel(const double* __restrict__ f0, double* __restrict__ Fd, int64_t m, int K, int KT, bool clamp,
                                    int32_t* __restrict__ flag) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  bool bad = false;
  for (int k = 0; k < KT; k++) {
    double x = 0.5;
    if (k < K) {
      x = f0[j + (int64_t)k * m];
      bad |= !admix_finite(x);
      if (clamp) x = admix_clamp(x);
    }
    Fd[j * KT + k] = x;
  }
  if (clamp && bad) atomicOr(flag, 2);
}

// F sweep: one workgroup per tile of 32 loci.  UPD: Fn receives f' (Fn != Fd); ll_part[lt] = the tile's share of l(Qd, Fd)
template <int KT, bool UPD>
__global__ __launch_bounds__(256) void admix_f_sweep_kernel(const uint32_t* __restrict__ L, int64_t Qb, int64_t n, int64_t m, int K,
                                                            const double* __restrict__ Qd, const double* __restrict__ Fd,
                                                            double* __restrict__ Fn, double* __restrict__ ll_part) {
  constexpr int NA = UPD ? KT : 1;
  __shared__ double stage[128 * KT];
  __shared__ double wll[4];
  __shared__ int cnts[32];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int64_t lt = blockIdx.x, j = lt * 32 + r;
  double f[KT], fb[KT], AB[2 * NA];
#pragma unroll
  for (int k = 0; k < KT; k++) {
    f[k] = j < m ? Fd[j * KT + k] : 0.5;
    fb[k] = 1.0 - f[k];
  }
#pragma unroll
  for (int v = 0; v < 2 * NA; v++) AB[v] = 0.0;
  double ll = 0.0;
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
      double p = 0.0, pb = 0.0;
#pragma unroll
      for (int k = 0; k < KT; k++) {
        p = fma(qs[k], f[k], p);
        pb = fma(qs[k], fb[k], pb);
      }
      cnt++;
      ll += log(g == 0 ? pb * pb : g == 1 ? p * pb : p * p);
      if constexpr (UPD) {
        const double w1 = (double)g / p, w0 = (double)(2 - g) / pb;
#pragma unroll
        for (int k = 0; k < KT; k++) {
          AB[k] = fma(qs[k], w1, AB[k]);
          AB[NA + k] = fma(qs[k], w0, AB[NA + k]);
        }
      }
    }
  }
  // the likelihood: butterfly over the wave, the waves in order
  for (int o = 32; o > 0; o >>= 1) ll += __shfl_xor(ll, o);
  if (lane == 0) wll[w] = ll;
  if constexpr (UPD) {
#pragma unroll
    for (int v = 0; v < 2 * NA; v++) AB[v] += __shfl_xor(AB[v], 32);
    cnt += __shfl_xor(cnt, 32);
    admix_wave_order_sum<2 * NA>(AB, cnt, stage, cnts, w, r, h);
  } else {
    __syncthreads();
  }
  if (threadIdx.x == 0) ll_part[lt] = ((wll[0] + wll[1]) + wll[2]) + wll[3];
  if constexpr (UPD) {
    if (w != 0 || h != 0 || j >= m) return;
#pragma unroll
    for (int k = 0; k < KT; k++) {
      double fn = k < K ? f[k] : 0.5;
      if (k < K && cnt > 0) {
        const double a = f[k] * AB[k], b = fb[k] * AB[NA + k], s = a + b;
        if (s > 0.0) fn = admix_clamp(a / s);  // s = 0: every typed individual has q(i, k) = 0; the locus keeps f(k, j)
      }
      Fn[j * KT + k] = fn;
    }
  }
}

// Q sweep: workgroup (rt, c) = 32 individuals x one chunk of loci -> part[(c n + i) KT + k], cpart[c n + i] (typed loci)
template <int KT>
__global__ __launch_bounds__(256) void admix_q_sweep_kernel(const uint32_t* __restrict__ T, int64_t KG, int64_t n, int64_t m,
                                                            const double* __restrict__ Qd, const double* __restrict__ Fd,
                                                            double* __restrict__ part, int32_t* __restrict__ cpart) {
  __shared__ double stage[128 * KT];
  __shared__ int cnts[32];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int64_t rt = blockIdx.x, c = blockIdx.y, i = rt * 32 + r;
  double qv[KT], S[KT];
#pragma unroll
  for (int k = 0; k < KT; k++) {
    qv[k] = i < n ? Qd[i * KT + k] : 0.0;
    S[k] = 0.0;
  }
  int cnt = 0;
  const int64_t kg0 = c * (ADM_CHUNK / 128), kg1 = kg0 + ADM_CHUNK / 128 < KG ? kg0 + ADM_CHUNK / 128 : KG;
  for (int64_t kg = kg0; kg < kg1; kg++) {
    __syncthreads();
    admix_stage<KT>(stage, Fd, kg, m, 0.5);
    __syncthreads();
    const uint32_t wd = T[((rt * KG + kg) * 64 + lane) * 4 + w];
#pragma unroll 2
    for (int e = 0; e < 16; e++) {
      const int g = admix_code(wd, e);
      if (g == 3) continue;
      const double* __restrict__ fs = stage + (32 * w + 16 * h + e) * KT;
      double p = 0.0, pb = 0.0;
#pragma unroll
      for (int k = 0; k < KT; k++) {
        p = fma(qv[k], fs[k], p);
        pb = fma(qv[k], 1.0 - fs[k], pb);
      }
      cnt++;
      const double w1 = (double)g / p, w0 = (double)(2 - g) / pb;
#pragma unroll
      for (int k = 0; k < KT; k++) S[k] = fma(1.0 - fs[k], w0, fma(fs[k], w1, S[k]));
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

// q'(i, k) = (q / (2 T_i)) * (the chunks' partials added in ascending order); T_i = 0 keeps the row
__global__ void admix_q_combine_kernel(const double* __restrict__ part, const int32_t* __restrict__ cpart, int64_t nchunks, int64_t n,
                                       int K, int KT, const double* __restrict__ Qd, double* __restrict__ Qn) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * KT) return;
  const int64_t i = idx / KT;
  const int k = (int)(idx % KT);
  double q = 0.0;
  if (k < K) {
    double s = 0.0;
    int64_t t = 0;
    for (int64_t c = 0; c < nchunks; c++) {
      s += part[(c * n + i) * KT + k];
      t += cpart[c * n + i];
    }
    q = Qd[idx];
    if (t > 0) q = (q / (2.0 * (double)t)) * s;
  }
  Qn[idx] = q;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
int admix_kt(int K) { return K <= 4 ? K : K <= 8 ? 8 : K <= 16 ? 16 : 32; }

#define ADM_DISPATCH(kt, CALL) \
  switch (kt) {                \
    case 1: CALL(1); break;    \
    case 2: CALL(2); break;    \
    case 3: CALL(3); break;    \
    case 4: CALL(4); break;    \
    case 8: CALL(8); break;    \
    case 16: CALL(16); break;  \
    default: CALL(32); break;  \
  }

struct AdmixRun {
  tpg_ctx* ctx;
  const tpg_view* v;
  int K, KT;
  int64_t n, m, n_lt, n_rt, nchunks;
  DevArena sc;
  double *Q[2] = {}, *F[2] = {}, *part = nullptr, *ll_part = nullptr, *trace = nullptr;
  int32_t *cpart = nullptr, *flag = nullptr;

  int init(tpg_ctx* c, const tpg_view* view, int k, bool need_q_sweep, bool need_f_next, int64_t trace_len) {
    ctx = c; v = view; K = k; KT = admix_kt(k);
    n = v->n; m = v->m;
    TPG_TRY(tpg_view_need_L(ctx, v));  // every sweep over the loci reads it
    n_lt = ceil_div(m, 32); n_rt = ceil_div(n, 32); nchunks = ceil_div(m, ADM_CHUNK);
    TPG_REQUIRE(n_lt <= 0x7FFFFFFF && n_rt <= 0x7FFFFFFF && nchunks <= 65535, TPG_EUNSUPPORTED, "admixture on a view of %lld x %lld",
                (long long)n, (long long)m);
    TPG_TRY(sc.get(&Q[0], (size_t)n * KT));
    TPG_TRY(sc.get(&F[0], (size_t)m * KT));
    TPG_TRY(sc.get(&ll_part, (size_t)n_lt));
    TPG_TRY(sc.get(&trace, (size_t)trace_len));
    TPG_TRY(sc.get(&flag, (size_t)1));
    if (need_f_next) TPG_TRY(sc.get(&F[1], (size_t)m * KT));
    if (need_q_sweep) {
      TPG_TRY(tpg_view_need_T(ctx, v));
      TPG_TRY(sc.get(&Q[1], (size_t)n * KT));
      TPG_TRY(sc.get(&part, (size_t)nchunks * n * KT));
      TPG_TRY(sc.get(&cpart, (size_t)nchunks * n));
    }
    return TPG_OK;
  }

  // the start into Q[0], F[0]: the caller's, checked and normalised on the device, or the hash of (seed, position)
  int start(const double* q0, const double* f0, uint64_t seed) {
    const unsigned gn = (unsigned)ceil_div(n, 256), gm = (unsigned)ceil_div(m, 256);
    InBuf iq, ifr;
    TPG_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), ctx->stream));
    if (q0) {
      TPG_TRY(iq.init(ctx, q0, sizeof(double) * (size_t)n * K));
      TPG_LAUNCH(ctx, "admix_start", admix_load_q_kernel, dim3(gn), dim3(256), 0, iq.dev<double>(), Q[0], n, K, KT, true, flag);
    } else {
      TPG_LAUNCH(ctx, "admix_start", admix_seed_q_kernel, dim3(gn), dim3(256), 0, Q[0], n, K, KT, seed);
    }
    if (f0) {
      TPG_TRY(ifr.init(ctx, f0, sizeof(double) * (size_t)m * K));
      TPG_LAUNCH(ctx, "admix_start", admix_load_f_kernel, dim3(gm), dim3(256), 0, ifr.dev<double>(), F[0], m, K, KT, true, flag);
    } else {
      TPG_LAUNCH(ctx, "admix_start", admix_seed_f_kernel, dim3(gm), dim3(256), 0, F[0], m, K, KT, seed);
    }
    TPG_CHECK_LAUNCH();
    if (q0 || f0) {  // (the fetch also waits for the two kernels that read the staged inputs)
      int32_t bad = 0;
      TPG_HIP(tpg_fetch_small(ctx, &bad, flag, sizeof bad));
      TPG_REQUIRE(!(bad & 1), TPG_EINVAL, "q0 has an entry that is not finite or not positive");
      TPG_REQUIRE(!(bad & 2), TPG_EINVAL, "f0 has an entry that is not finite");
    }
    return TPG_OK;
  }

  // the padded state (Qs, Fs) -> the caller's Q (n x K) and P (m x K), host or device memory
  int store(const double* Qs, const double* Fs, double* Qout, double* Pout) {
    OutBuf oq, op;
    TPG_TRY(oq.init(Qout, sizeof(double) * (size_t)n * K));
    TPG_TRY(op.init(Pout, sizeof(double) * (size_t)m * K));
    TPG_LAUNCH(ctx, "admix_store", admix_store_kernel, dim3((unsigned)ceil_div(n * K, 256)), dim3(256), 0, Qs, n, K, KT, oq.dev<double>());
    TPG_LAUNCH(ctx, "admix_store", admix_store_kernel, dim3((unsigned)ceil_div(m * K, 256)), dim3(256), 0, Fs, m, K, KT, op.dev<double>());
    TPG_CHECK_LAUNCH();
    TPG_HIP(hipStreamSynchronize(ctx->stream));
    TPG_TRY(oq.commit(ctx));
    TPG_TRY(op.commit(ctx));
    return TPG_OK;
  }

  // l(Q[cur], F[cur]) -> trace[slot]; update: F[1 - cur] receives f' as well
  int f_sweep(int cur_q, int cur_f, bool update, int64_t slot) { return f_sweep_at(Q[cur_q], F[cur_f], F[1 - cur_f], update, slot); }

  // the same between any buffers: l(Qs, Fs) -> trace[slot]; update: Fn (not Fs) receives f'
  int f_sweep_at(const double* Qs, const double* Fs, double* Fn, bool update, int64_t slot) {
#define ADM_F(KT_)                                                                                                                  \
  do {                                                                                                                              \
    auto k_upd = admix_f_sweep_kernel<KT_, true>;                                                                                   \
    auto k_ll = admix_f_sweep_kernel<KT_, false>;                                                                                   \
    if (update)                                                                                                                     \
      TPG_LAUNCH(ctx, "admix_f_sweep", k_upd, dim3((unsigned)n_lt), dim3(256), 0, (const uint32_t*)v->L, \
                 v->Q, n, m, K, Qs, Fs, Fn, ll_part);                                                                               \
    else                                                                                                                            \
      TPG_LAUNCH(ctx, "admix_loglik", k_ll, dim3((unsigned)n_lt), dim3(256), 0, (const uint32_t*)v->L, \
                 v->Q, n, m, K, Qs, Fs, (double*)nullptr, ll_part);                                                                 \
  } while (0)
    ADM_DISPATCH(KT, ADM_F);
#undef ADM_F
    TPG_LAUNCH(ctx, "admix_ll_sum", admix_ll_sum_kernel, dim3(1), dim3(256), 0, (const double*)ll_part, n_lt, trace + slot);
    TPG_CHECK_LAUNCH();
    return TPG_OK;
  }

  int q_sweep(int cur_q, int cur_f) { return q_sweep_at(Q[cur_q], F[cur_f], Q[1 - cur_q]); }

  // Qn (not Qs) receives q' of (Qs, Fs)
  int q_sweep_at(const double* Qs, const double* Fs, double* Qn) {
#define ADM_Q(KT_)                                                                                                               \
  TPG_LAUNCH(ctx, "admix_q_sweep", admix_q_sweep_kernel<KT_>, dim3((unsigned)n_rt, (unsigned)nchunks), dim3(256), 0,              \
             (const uint32_t*)v->T, v->KG, n, m, Qs, Fs, part, cpart)
    ADM_DISPATCH(KT, ADM_Q);
#undef ADM_Q
    TPG_LAUNCH(ctx, "admix_q_combine", admix_q_combine_kernel, dim3((unsigned)ceil_div(n * KT, 256)), dim3(256), 0, (const double*)part,
               (const int32_t*)cpart, nchunks, n, K, KT, Qs, Qn);
    TPG_CHECK_LAUNCH();
    return TPG_OK;
  }
};

int admix_check_view(const tpg_view* v, int K) {
  TPG_REQUIRE(K >= 1 && K <= TPG_ADMIX_MAX_K, TPG_EINVAL, "K = %d out of [1, %d]", K, TPG_ADMIX_MAX_K);
  TPG_REQUIRE(v->n > 0 && v->m > 0, TPG_EINVAL, "admixture needs at least one individual and one locus (view of %lld x %lld)",
              (long long)v->n, (long long)v->m);
  return TPG_OK;
}

}  // namespace

extern "C" int64_t tpg_admix_chunk_loci(void) { return ADM_CHUNK; }

extern "C" int tpg_admix_params_default(tpg_admix_params* p) {
  TPG_REQUIRE(p, TPG_EINVAL, "null argument");
  p->max_iter = 1000;
  p->tol = 1e-4;
  p->update_q = 1;
  p->update_f = 1;
  p->seed = 0;
  return TPG_OK;
}

extern "C" int tpg_admix_em(tpg_ctx* ctx, const tpg_view* v, const double* ploidy, int K, const tpg_admix_params* params,
                            const double* q0, const double* f0, double* Q, double* P, double* loglik, double* loglik_trace,
                            int32_t* n_iter, int32_t* converged) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && Q && P, TPG_EINVAL, "null argument");
  tpg_admix_params pr;
  tpg_admix_params_default(&pr);
  if (params) pr = *params;
  TPG_TRY(admix_check_view(v, K));
  TPG_REQUIRE(pr.max_iter >= 0, TPG_EINVAL, "max_iter = %d is negative", (int)pr.max_iter);
  TPG_REQUIRE(pr.tol >= 0.0, TPG_EINVAL, "tol must be a non-negative number");  // false for a NaN too
  TPG_TRY(tpg_require_diploid(v->n, ploidy, "admixture"));
  const bool upd_q = pr.update_q != 0, upd_f = pr.update_f != 0;
  AdmixRun run;
  TPG_TRY(run.init(ctx, v, K, upd_q && pr.max_iter > 0, upd_f && pr.max_iter > 0, (int64_t)pr.max_iter + 1));
  TPG_TRY(run.start(q0, f0, (uint64_t)pr.seed));
  // state t - 1 -> state t; the F sweep of that pass leaves l(t - 1) in trace[t - 1]
  std::vector<double> ll((size_t)pr.max_iter + 1);
  int cq = 0, cf = 0, t = 0, conv = 0;
  while (t < pr.max_iter) {
    TPG_TRY(run.f_sweep(cq, cf, upd_f, t));
    if (upd_q) TPG_TRY(run.q_sweep(cq, cf));
    TPG_HIP(tpg_fetch_small(ctx, &ll[(size_t)t], run.trace + t, sizeof(double)));
    if (upd_q) cq = 1 - cq;
    if (upd_f) cf = 1 - cf;
    t++;
    if (t >= 2 && ll[(size_t)t - 1] - ll[(size_t)t - 2] < pr.tol) {
      conv = 1;
      break;
    }
  }
  TPG_TRY(run.f_sweep(cq, cf, false, t));
  TPG_HIP(tpg_fetch_small(ctx, &ll[(size_t)t], run.trace + t, sizeof(double)));
  // nothing of the caller's has been written so far
  TPG_TRY(run.store(run.Q[cq], run.F[cf], Q, P));
  if (loglik) *loglik = ll[(size_t)t];
  if (loglik_trace)
    for (int s = 0; s <= t; s++) loglik_trace[s] = ll[(size_t)s];
  if (n_iter) *n_iter = t;
  if (converged) *converged = conv;
  return TPG_OK;
}

extern "C" int tpg_admix_loglik(tpg_ctx* ctx, const tpg_view* v, int K, const double* Q, const double* P, double* loglik) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && Q && P && loglik, TPG_EINVAL, "null argument");
  TPG_TRY(admix_check_view(v, K));
  const int64_t n = v->n, m = v->m;
  AdmixRun run;
  TPG_TRY(run.init(ctx, v, K, false, false, 1));
  InBuf iq, ip;
  TPG_TRY(iq.init(ctx, Q, sizeof(double) * (size_t)n * K));
  TPG_TRY(ip.init(ctx, P, sizeof(double) * (size_t)m * K));
  TPG_LAUNCH(ctx, "admix_start", admix_load_q_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, iq.dev<double>(), run.Q[0], n, K,
             run.KT, false, run.flag);
  TPG_LAUNCH(ctx, "admix_start", admix_load_f_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, ip.dev<double>(), run.F[0], m, K,
             run.KT, false, run.flag);
  TPG_TRY(run.f_sweep(0, 0, false, 0));
  TPG_HIP(tpg_fetch_small(ctx, loglik, run.trace, sizeof(double)));
  return TPG_OK;
}

// ---- squared extrapolation (include/tpg.h "admixture, accelerated") ----------------------------------------------------------
// Two streaming kernels beside the sweeps, both over the padded states theta0, theta1, theta2 of the halves being updated.
// admix_sq_norms: a workgroup of four waves owns a tile of SQ_TILE consecutive doubles of a padded state; thread t takes the entries
// 256 e + t, e = 0 .. 7, in ascending e (coalesced 8-byte loads), and adds r^2 and v^2 of the live columns by one fused multiply-add
// each; then a butterfly over the wave and the four waves in order -> part[2 tile], part[2 tile + 1].  Q's tiles come first, F's
// after them; admix_sq_combine (one workgroup) has thread t add the tiles t, t + 256, ... in ascending order, then the same
// butterfly and wave order.  No atomics.
// admix_sq_extrap: theta' raw, entry by entry, then the projection of its row.  KT >= 8: KT lanes per row, one entry each
// (coalesced), the "anything moved" flag of the row by a ballot and Q's row sum by K shuffles in ascending k; KT <= 4: one lane
// per row with its KT entries in registers (a row is at most 32 bytes).  No LDS.
namespace {

constexpr int SQ_TILE = 2048;

// the workgroup's two sums -> out[0], out[1]: a butterfly over each wave, then the four waves in order
__device__ __forceinline__ void admix_sq_block_sums(double sr, double sv, double* __restrict__ out) {
  __shared__ double wsum[2][4];
  for (int o = 32; o > 0; o >>= 1) {
    sr += __shfl_xor(sr, o);
    sv += __shfl_xor(sv, o);
  }
  if ((threadIdx.x & 63) == 0) {
    wsum[0][threadIdx.x >> 6] = sr;
    wsum[1][threadIdx.x >> 6] = sv;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const double* w = wsum[threadIdx.x];
    out[threadIdx.x] = ((w[0] + w[1]) + w[2]) + w[3];
  }
}

__global__ __launch_bounds__(256) void admix_sq_norms_kernel(const double* __restrict__ t0, const double* __restrict__ t1,
                                                             const double* __restrict__ t2, int64_t len, int K, int KT,
                                                             double* __restrict__ part) {
  const int64_t base = (int64_t)blockIdx.x * SQ_TILE;
  double sr = 0.0, sv = 0.0;
#pragma unroll
  for (int e = 0; e < SQ_TILE / 256; e++) {
    const int64_t idx = base + e * 256 + threadIdx.x;
    // KT > K only where KT is a power of two (admix_kt): the padding columns are k = idx mod KT >= K
    if (idx < len && (KT == K || (int)(idx & (KT - 1)) < K)) {
      const double a = t0[idx], b = t1[idx], c = t2[idx];
      const double r = b - a, v = (c - b) - r;
      sr = fma(r, r, sr);
      sv = fma(v, v, sv);
    }
  }
  admix_sq_block_sums(sr, sv, part + 2 * (int64_t)blockIdx.x);
}

// out[0] = sr, out[1] = sv: thread t adds the tiles t, t + 256, ...; butterfly; the four waves in order
__global__ __launch_bounds__(256) void admix_sq_combine_kernel(const double* __restrict__ part, int64_t ntiles, double* __restrict__ out) {
  double sr = 0.0, sv = 0.0;
  for (int64_t t = threadIdx.x; t < ntiles; t += 256) {
    sr += part[2 * t];
    sv += part[2 * t + 1];
  }
  admix_sq_block_sums(sr, sv, out);
}

// out = the projected theta' of one half (ISQ: Q, rows = individuals; else F, rows = loci); raw (may be null) = theta' before the
// projection.  a2 = alpha * alpha rounded once, m2a = -2 alpha (exact).  A row in which nothing moved (r = v = 0 in every
// entry: a locus or an individual typed nowhere is one) keeps theta0 bit for bit; the padding comes out as q = 0, f = 0.5.
template <int KT, bool ISQ>
__global__ __launch_bounds__(256) void admix_sq_extrap_kernel(const double* __restrict__ t0, const double* __restrict__ t1,
                                                              const double* __restrict__ t2, double* __restrict__ out,
                                                              double* __restrict__ raw, int64_t rows, int K, double a2, double m2a) {
  constexpr int LG = KT >= 8 ? KT : 1, E = KT / LG;  // lanes per row, entries per lane
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, row = gid / LG;
  const int kl = (int)(gid % LG);
  const bool live = row < rows;  // a lane beyond the last row still meets the ballot and the shuffles
  double a[E], x[E];
  bool moved = false;
#pragma unroll
  for (int e = 0; e < E; e++) {
    a[e] = x[e] = 0.0;
    if (live) {
      const int64_t idx = row * KT + kl * E + e;
      a[e] = t0[idx];
      const double b = t1[idx], c = t2[idx];
      const double r = b - a[e], v = (c - b) - r;
      x[e] = fma(a2, v, fma(m2a, r, a[e]));
      moved |= r != 0.0 || v != 0.0;
      if (raw) raw[idx] = x[e];
    }
  }
  if constexpr (LG > 1) {
    const int lane = threadIdx.x & 63, first = lane & ~(LG - 1);
    moved = ((__ballot(moved) >> first) & ((1ull << LG) - 1)) != 0;
    double y = ISQ ? (x[0] < TPG_ADMIX_EPS ? TPG_ADMIX_EPS : x[0]) : admix_clamp(x[0]);
    if constexpr (ISQ) {
      double s = 0.0;
      for (int k = 0; k < K; k++) s += __shfl(y, first + k);
      y = y / s;
    }
    if (live) out[row * KT + kl] = kl >= K ? (ISQ ? 0.0 : 0.5) : moved ? y : a[0];
  } else {
    if (!live) return;
    double y[E], s = 0.0;
#pragma unroll
    for (int e = 0; e < E; e++) {
      y[e] = ISQ ? (x[e] < TPG_ADMIX_EPS ? TPG_ADMIX_EPS : x[e]) : admix_clamp(x[e]);
      s += y[e];
    }
#pragma unroll
    for (int e = 0; e < E; e++) out[row * KT + e] = !moved ? a[e] : ISQ ? y[e] / s : y[e];
  }
}

// the device side of one extrapolation: the two sums and theta'.  part holds two doubles per tile, sums two doubles.
struct AdmixSqDev {
  tpg_ctx* ctx;
  int64_t n, m;
  int K, KT;
  bool upd_q, upd_f;
  double *part = nullptr, *sums = nullptr;
  int64_t tq = 0, tf = 0;

  int init(tpg_ctx* c, DevArena& sc, int64_t n_, int64_t m_, int k, bool uq, bool uf) {
    ctx = c; n = n_; m = m_; K = k; KT = admix_kt(k); upd_q = uq; upd_f = uf;
    tq = upd_q ? ceil_div(n * KT, SQ_TILE) : 0;
    tf = upd_f ? ceil_div(m * KT, SQ_TILE) : 0;
    TPG_REQUIRE(tq + tf <= 0x7FFFFFFF && ceil_div(m * KT, 256) <= 0x7FFFFFFF && ceil_div(n * KT, 256) <= 0x7FFFFFFF, TPG_EUNSUPPORTED,
                "accelerated admixture on a state of %lld x %lld x %d", (long long)n, (long long)m, KT);
    TPG_TRY(sc.get(&part, (size_t)(2 * (tq + tf))));
    TPG_TRY(sc.get(&sums, (size_t)2));
    return TPG_OK;
  }

  int norms(const double* q0, const double* q1, const double* q2, const double* f0, const double* f1, const double* f2, double* sr,
            double* sv) {
    if (tq)
      TPG_LAUNCH(ctx, "admix_sq_norms", admix_sq_norms_kernel, dim3((unsigned)tq), dim3(256), 0, q0, q1, q2, n * KT, K, KT, part);
    if (tf)
      TPG_LAUNCH(ctx, "admix_sq_norms", admix_sq_norms_kernel, dim3((unsigned)tf), dim3(256), 0, f0, f1, f2, m * KT, K, KT, part + 2 * tq);
    TPG_LAUNCH(ctx, "admix_sq_combine", admix_sq_combine_kernel, dim3(1), dim3(256), 0, (const double*)part, tq + tf, sums);
    TPG_CHECK_LAUNCH();
    double s[2] = {0.0, 0.0};
    TPG_HIP(tpg_fetch_small(ctx, s, sums, sizeof s));
    *sr = s[0];
    *sv = s[1];
    return TPG_OK;
  }

  // qp / fp = the projected theta' of the halves being updated (the other half is not touched); qraw / fraw may be null
  int extrapolate(const double* q0, const double* q1, const double* q2, const double* f0, const double* f1, const double* f2,
                  double alpha, double* qp, double* fp, double* qraw, double* fraw) {
    const double a2 = alpha * alpha, m2a = -2.0 * alpha;
#define ADM_X(KT_)                                                                                                                  \
  do {                                                                                                                              \
    constexpr int LG_ = KT_ >= 8 ? KT_ : 1;                                                                                         \
    if (upd_q)                                                                                                                      \
      TPG_LAUNCH(ctx, "admix_sq_extrap", (admix_sq_extrap_kernel<KT_, true>), dim3((unsigned)ceil_div(n * LG_, 256)), dim3(256), 0, \
                 q0, q1, q2, qp, qraw, n, K, a2, m2a);                                                                              \
    if (upd_f)                                                                                                                      \
      TPG_LAUNCH(ctx, "admix_sq_extrap", (admix_sq_extrap_kernel<KT_, false>), dim3((unsigned)ceil_div(m * LG_, 256)), dim3(256),   \
                 0, f0, f1, f2, fp, fraw, m, K, a2, m2a);                                                                           \
  } while (0)
    ADM_DISPATCH(KT, ADM_X);
#undef ADM_X
    TPG_CHECK_LAUNCH();
    return TPG_OK;
  }
};

// what squarem_drive (host/host_squarem.h) asks of the device: five state slots over the buffers of an AdmixRun
struct AdmixSqOps {
  AdmixRun& run;
  AdmixSqDev& dev;
  double *Qs[5], *Fs[5];

  int step(int src, int dst, int t, double* l) {
    TPG_TRY(run.f_sweep_at(Qs[src], Fs[src], Fs[dst], dev.upd_f, t));
    if (dev.upd_q) TPG_TRY(run.q_sweep_at(Qs[src], Fs[src], Qs[dst]));
    TPG_HIP(tpg_fetch_small(run.ctx, l, run.trace + t, sizeof(double)));
    return TPG_OK;
  }
  int norms(int s0, int s1, int s2, double* sr, double* sv) {
    return dev.norms(Qs[s0], Qs[s1], Qs[s2], Fs[s0], Fs[s1], Fs[s2], sr, sv);
  }
  int extrapolate(int s0, int s1, int s2, int dst, double alpha) {
    return dev.extrapolate(Qs[s0], Qs[s1], Qs[s2], Fs[s0], Fs[s1], Fs[s2], alpha, Qs[dst], Fs[dst], nullptr, nullptr);
  }
};

}  // namespace

extern "C" int tpg_admix_em_squarem(tpg_ctx* ctx, const tpg_view* v, const double* ploidy, int K, const tpg_admix_params* params,
                                    const double* q0, const double* f0, double* Q, double* P, double* loglik, double* loglik_trace,
                                    int32_t* n_iter, int32_t* converged, double* alpha, int32_t* accepted, int32_t* n_cycles,
                                    int32_t* n_rejected) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && Q && P, TPG_EINVAL, "null argument");
  tpg_admix_params pr;
  tpg_admix_params_default(&pr);
  if (params) pr = *params;
  TPG_TRY(admix_check_view(v, K));
  TPG_REQUIRE(pr.max_iter >= 0, TPG_EINVAL, "max_iter = %d is negative", (int)pr.max_iter);
  TPG_REQUIRE(pr.tol >= 0.0, TPG_EINVAL, "tol must be a non-negative number");  // false for a NaN too
  TPG_TRY(tpg_require_diploid(v->n, ploidy, "admixture"));
  const bool upd_q = pr.update_q != 0 && pr.max_iter > 0, upd_f = pr.update_f != 0 && pr.max_iter > 0;
  AdmixRun run;
  TPG_TRY(run.init(ctx, v, K, upd_q, upd_f, (int64_t)pr.max_iter + 1));
  AdmixSqDev dev;
  TPG_TRY(dev.init(ctx, run.sc, v->n, v->m, K, upd_q, upd_f));
  // five slots; a half that is not updated is one buffer under all of them
  AdmixSqOps ops{run, dev, {}, {}};
  for (int s = 0; s < 5; s++) {
    ops.Qs[s] = s < 2 || !upd_q ? run.Q[upd_q ? s : 0] : nullptr;
    ops.Fs[s] = s < 2 || !upd_f ? run.F[upd_f ? s : 0] : nullptr;
    if (!ops.Qs[s]) TPG_TRY(run.sc.get(&ops.Qs[s], (size_t)v->n * run.KT));
    if (!ops.Fs[s]) TPG_TRY(run.sc.get(&ops.Fs[s], (size_t)v->m * run.KT));
  }
  TPG_TRY(run.start(q0, f0, (uint64_t)pr.seed));
  std::vector<double> ll((size_t)pr.max_iter + 1), al((size_t)pr.max_iter / 3 + 1);
  std::vector<int32_t> acc((size_t)pr.max_iter / 3 + 1);
  squarem_result res;
  TPG_TRY(squarem_drive(ops, (int)pr.max_iter, pr.tol, 4.0, ll.data(), al.data(), acc.data(), &res));
  const int t = res.n_iter;
  TPG_TRY(run.f_sweep_at(ops.Qs[res.last], ops.Fs[res.last], nullptr, false, t));
  TPG_HIP(tpg_fetch_small(ctx, &ll[(size_t)t], run.trace + t, sizeof(double)));
  // nothing of the caller's has been written so far
  TPG_TRY(run.store(ops.Qs[res.last], ops.Fs[res.last], Q, P));
  if (loglik) *loglik = ll[(size_t)t];
  if (loglik_trace)
    for (int s = 0; s <= t; s++) loglik_trace[s] = ll[(size_t)s];
  if (n_iter) *n_iter = t;
  if (converged) *converged = res.converged;
  for (int c = 0; c < res.n_cycles; c++) {
    if (alpha) alpha[c] = al[(size_t)c];
    if (accepted) accepted[c] = acc[(size_t)c];
  }
  if (n_cycles) *n_cycles = res.n_cycles;
  if (n_rejected) *n_rejected = res.n_rejected;
  return TPG_OK;
}

extern "C" int tpg_admix_squarem_point(tpg_ctx* ctx, int64_t n, int64_t m, int K, int update_q, int update_f, const double* q0,
                                       const double* f0, const double* q1, const double* f1, const double* q2, const double* f2,
                                       double a_max, double* sr, double* sv, double* alpha, double* Qp, double* Pp, double* Qraw,
                                       double* Praw) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && q0 && f0 && q1 && f1 && q2 && f2, TPG_EINVAL, "null argument");
  TPG_REQUIRE(K >= 1 && K <= TPG_ADMIX_MAX_K, TPG_EINVAL, "K = %d out of [1, %d]", K, TPG_ADMIX_MAX_K);
  TPG_REQUIRE(n > 0 && m > 0, TPG_EINVAL, "a state of %lld individuals and %lld loci", (long long)n, (long long)m);
  TPG_REQUIRE(a_max >= 1.0, TPG_EINVAL, "a_max must be a number >= 1");  // false for a NaN too
  const bool upd_q = update_q != 0, upd_f = update_f != 0;
  const int KT = admix_kt(K);
  DevArena sc;
  AdmixSqDev dev;
  TPG_TRY(dev.init(ctx, sc, n, m, K, upd_q, upd_f));
  // the six matrices as given (no normalisation, no clamp) into padded states; 0 .. 2: Q, 3 .. 5: F; 6, 7: theta'; 8, 9: raw
  const double* in[6] = {q0, q1, q2, f0, f1, f2};
  double* st[10];
  int32_t* flag = nullptr;
  TPG_TRY(sc.get(&flag, (size_t)1));
  InBuf ib[6];
  for (int a = 0; a < 10; a++) TPG_TRY(sc.get(&st[a], (size_t)((a < 3 || a == 6 || a == 8) ? n : m) * KT));
  for (int a = 0; a < 6; a++) {
    const int64_t rows = a < 3 ? n : m;
    TPG_TRY(ib[a].init(ctx, in[a], sizeof(double) * (size_t)rows * K));
    if (a < 3)
      TPG_LAUNCH(ctx, "admix_start", admix_load_q_kernel, dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, ib[a].dev<double>(), st[a],
                 rows, K, KT, false, flag);
    else
      TPG_LAUNCH(ctx, "admix_start", admix_load_f_kernel, dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, ib[a].dev<double>(), st[a],
                 rows, K, KT, false, flag);
  }
  // a half that is not updated comes back as theta0, raw and projected alike
  TPG_HIP(tpg_copy_dev(ctx, st[6], st[0], sizeof(double) * (size_t)n * KT));
  TPG_HIP(tpg_copy_dev(ctx, st[8], st[0], sizeof(double) * (size_t)n * KT));
  TPG_HIP(tpg_copy_dev(ctx, st[7], st[3], sizeof(double) * (size_t)m * KT));
  TPG_HIP(tpg_copy_dev(ctx, st[9], st[3], sizeof(double) * (size_t)m * KT));
  double s_r = 0.0, s_v = 0.0;
  TPG_TRY(dev.norms(st[0], st[1], st[2], st[3], st[4], st[5], &s_r, &s_v));
  bool at_limit = false;
  const double al = squarem_alpha(s_r, s_v, a_max, &at_limit);
  TPG_TRY(dev.extrapolate(st[0], st[1], st[2], st[3], st[4], st[5], al, st[6], st[7], st[8], st[9]));
  // nothing of the caller's has been written so far
  double* outs[4] = {Qp, Pp, Qraw, Praw};
  OutBuf ob[4];
  for (int a = 0; a < 4; a++) {
    if (!outs[a]) continue;
    const int64_t rows = a % 2 == 0 ? n : m;
    TPG_TRY(ob[a].init(outs[a], sizeof(double) * (size_t)rows * K));
    TPG_LAUNCH(ctx, "admix_store", admix_store_kernel, dim3((unsigned)ceil_div(rows * K, 256)), dim3(256), 0, (const double*)st[6 + a], rows,
               K, KT, ob[a].dev<double>());
  }
  TPG_CHECK_LAUNCH();
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  for (int a = 0; a < 4; a++)
    if (outs[a]) TPG_TRY(ob[a].commit(ctx));
  if (sr) *sr = s_r;
  if (sv) *sv = s_v;
  if (alpha) *alpha = al;
  return TPG_OK;
}

// ---- cross-validation (include/tpg.h "admixture cross-validation") -----------------------------------------------------------
// admix_holdout_view is admix_common.h's hold-out with the fold predicate.
// admix_holdout_sweep: the likelihood-only pass over the entries typed in `full` and missing in `train`: wave w decodes dword w of
// BOTH planes at the same offset; the sum shape is that of admix_f_sweep_kernel<KT, false>; the two counts are integers (wave sum,
// one integer atomic per wave).
namespace {

// one workgroup per tile of 32 loci; Lf / Lt: the L planes of the full and the training view (the same geometry).
// ll_part[lt] = the tile's share of sum ln(p^g pbar^(2 - g)) over the held-out entries; d_cnt[0] += their number, d_cnt[1] += g = 1
template <int KT>
__global__ __launch_bounds__(256) void admix_holdout_sweep_kernel(const uint32_t* __restrict__ Lf, const uint32_t* __restrict__ Lt,
                                                                  int64_t Qb, int64_t n, int64_t m, const double* __restrict__ Qd,
                                                                  const double* __restrict__ Fd, double* __restrict__ ll_part,
                                                                  unsigned long long* __restrict__ d_cnt) {
  __shared__ double stage[128 * KT];
  __shared__ double wll[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int64_t lt = blockIdx.x, j = lt * 32 + r;
  double f[KT], fb[KT];
#pragma unroll
  for (int k = 0; k < KT; k++) {
    f[k] = j < m ? Fd[j * KT + k] : 0.5;
    fb[k] = 1.0 - f[k];
  }
  double ll = 0.0;
  int cnt = 0, het = 0;
  for (int64_t q = 0; q < Qb; q++) {
    __syncthreads();
    admix_stage<KT>(stage, Qd, q, n, 0.0);
    __syncthreads();
    const int64_t at = ((lt * Qb + q) * 64 + lane) * 4 + w;
    const uint32_t wf = Lf[at], wt = Lt[at];
    // held out: typed in full (not both bits set) and missing in train (both bits set)
    uint32_t ho = ~(wf & (wf >> 1)) & (wt & (wt >> 1)) & 0x55555555u;
    if (ho == 0) continue;
    // the lane's own held-out entries, bit e = entry e: walked in ascending order, as the likelihood pass adds them; a wave makes
    // as many trips as its fullest lane holds entries, not 16 with a share 1 / folds of its lanes active
    uint32_t mine = 0;
#pragma unroll
    for (int e = 0; e < 16; e++) mine |= ((ho >> tpg_elem_shift(e)) & 1u) << e;
    while (mine) {
      const int e = __ffs(mine) - 1;
      mine &= mine - 1;
      const int g = admix_code(wf, e);
      const double* __restrict__ qs = stage + (32 * w + 16 * h + e) * KT;
      double p = 0.0, pb = 0.0;
#pragma unroll
      for (int k = 0; k < KT; k++) {
        p = fma(qs[k], f[k], p);
        pb = fma(qs[k], fb[k], pb);
      }
      cnt++;
      het += g == 1;
      ll += log(g == 0 ? pb * pb : g == 1 ? p * pb : p * p);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    ll += __shfl_xor(ll, o);
    cnt += __shfl_xor(cnt, o);
    het += __shfl_xor(het, o);
  }
  if (lane == 0) {
    wll[w] = ll;
    if (cnt) atomicAdd(d_cnt, (unsigned long long)cnt);
    if (het) atomicAdd(d_cnt + 1, (unsigned long long)het);
  }
  __syncthreads();
  if (threadIdx.x == 0) ll_part[lt] = ((wll[0] + wll[1]) + wll[2]) + wll[3];
}

int admix_check_folds(int folds) {
  TPG_REQUIRE(folds >= 2 && folds <= TPG_ADMIX_MAX_FOLDS, TPG_EINVAL, "folds = %d out of [2, %d]", folds, TPG_ADMIX_MAX_FOLDS);
  return TPG_OK;
}

// train_f of `full` (the caller holds the context)
int admix_view_holdout(tpg_ctx* ctx, const tpg_view* full, int folds, int fold, uint64_t cv_seed, tpg_view** out, int64_t* n_held) {
  TPG_TRY(admix_check_folds(folds));
  TPG_REQUIRE(fold >= 0 && fold < folds, TPG_EINVAL, "fold = %d out of [0, %d)", fold, folds);
  return admix_holdout_view<HoldoutFold>(ctx, "admix_holdout_view", full, cv_seed, out, n_held != nullptr, n_held, folds, fold);
}

}  // namespace

extern "C" int tpg_view_holdout(tpg_ctx* ctx, const tpg_view* full, int folds, int fold, uint64_t cv_seed, tpg_view** out,
                                int64_t* n_held) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && full && out, TPG_EINVAL, "null argument");
  return admix_view_holdout(ctx, full, folds, fold, cv_seed, out, n_held);
}

extern "C" int tpg_admix_holdout_sums(tpg_ctx* ctx, const tpg_view* full, const tpg_view* train, int K, const double* Q,
                                      const double* P, double* ll, int64_t* n_held, int64_t* n_het) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && full && train && Q && P, TPG_EINVAL, "null argument");
  TPG_TRY(admix_check_view(full, K));
  TPG_REQUIRE(full->n == train->n && full->m == train->m, TPG_EINVAL, "the full view is %lld x %lld, the training view %lld x %lld",
              (long long)full->n, (long long)full->m, (long long)train->n, (long long)train->m);
  TPG_TRY(tpg_view_need_L(ctx, full));
  TPG_TRY(tpg_view_need_L(ctx, train));
  const int64_t n = full->n, m = full->m;
  AdmixRun run;
  TPG_TRY(run.init(ctx, full, K, false, false, 1));
  unsigned long long* d_cnt = nullptr;
  TPG_TRY(run.sc.get(&d_cnt, (size_t)2));
  TPG_HIP(hipMemsetAsync(d_cnt, 0, 2 * sizeof(unsigned long long), ctx->stream));
  InBuf iq, ip;
  TPG_TRY(iq.init(ctx, Q, sizeof(double) * (size_t)n * K));
  TPG_TRY(ip.init(ctx, P, sizeof(double) * (size_t)m * K));
  TPG_LAUNCH(ctx, "admix_start", admix_load_q_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, iq.dev<double>(), run.Q[0], n, K,
             run.KT, false, run.flag);
  TPG_LAUNCH(ctx, "admix_start", admix_load_f_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, ip.dev<double>(), run.F[0], m, K,
             run.KT, false, run.flag);
#define ADM_H(KT_)                                                                                                                 \
  TPG_LAUNCH(ctx, "admix_holdout_sweep", admix_holdout_sweep_kernel<KT_>, dim3((unsigned)run.n_lt), dim3(256), 0,                  \
             (const uint32_t*)full->L, (const uint32_t*)train->L, full->Q, n, m, (const double*)run.Q[0], (const double*)run.F[0], \
             run.ll_part, d_cnt)
  ADM_DISPATCH(run.KT, ADM_H);
#undef ADM_H
  TPG_LAUNCH(ctx, "admix_ll_sum", admix_ll_sum_kernel, dim3(1), dim3(256), 0, (const double*)run.ll_part, run.n_lt, run.trace);
  TPG_CHECK_LAUNCH();
  double l = 0.0;
  unsigned long long c[2] = {0, 0};
  TPG_HIP(tpg_fetch_small(ctx, &l, run.trace, sizeof l));
  TPG_HIP(tpg_fetch_small(ctx, c, d_cnt, sizeof c));
  if (ll) *ll = l;
  if (n_held) *n_held = (int64_t)c[0];
  if (n_het) *n_het = (int64_t)c[1];
  return TPG_OK;
}

extern "C" int tpg_admix_cv_error(int folds, const double* fold_ll, const int64_t* fold_count, const int64_t* fold_het, double* fold_dev,
                                  double* cv_error) {
  TPG_REQUIRE(fold_ll && fold_count && fold_het && cv_error, TPG_EINVAL, "null argument");
  TPG_TRY(admix_check_folds(folds));
  double dev[TPG_ADMIX_MAX_FOLDS], sum = 0.0;
  int64_t total = 0;
  for (int f = 0; f < folds; f++) {
    TPG_REQUIRE(fold_count[f] >= 0 && fold_het[f] >= 0 && fold_het[f] <= fold_count[f], TPG_EINVAL,
                "fold %d: %lld held-out entries, %lld of them heterozygous", f, (long long)fold_count[f], (long long)fold_het[f]);
    // -2 ln(p^g pbar^(2 - g)) - [g = 1] 4 ln 2: two products, then one subtraction (this file is compiled without contraction)
    const double a = -2.0 * fold_ll[f], b = 2.772588722239781 * (double)fold_het[f];
    dev[f] = a - b;
    sum = f == 0 ? dev[0] : sum + dev[f];
    total += fold_count[f];
  }
  TPG_REQUIRE(total > 0, TPG_EINVAL, "no held-out entry in any fold");
  if (fold_dev)
    for (int f = 0; f < folds; f++) fold_dev[f] = dev[f];
  *cv_error = sum / (double)total;
  return TPG_OK;
}

namespace {
// the folds' refits by plain EM or, squarem = true, by the accelerated driver; everything else is shared
int admix_cv(bool squarem, tpg_ctx* ctx, const tpg_view* v, const double* ploidy, int K, const tpg_admix_params* params, int folds,
             uint64_t cv_seed, const double* q0, const double* f0, double* cv_error, double* fold_ll, int64_t* fold_count,
             int64_t* fold_het, int32_t* fold_iter, int32_t* fold_converged) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && cv_error, TPG_EINVAL, "null argument");
  TPG_TRY(admix_check_folds(folds));
  TPG_TRY(admix_check_view(v, K));
  const int64_t n = v->n, m = v->m;
  // the start goes to the device once; every fold's EM reads it there, and its Q and P stay there for the hold-out sums
  InBuf iq, ifr;
  if (q0) TPG_TRY(iq.init(ctx, q0, sizeof(double) * (size_t)n * K));
  if (f0) TPG_TRY(ifr.init(ctx, f0, sizeof(double) * (size_t)m * K));
  DevBuf Qd, Pd;
  TPG_TRY(Qd.alloc_n<double>((size_t)n * K));
  TPG_TRY(Pd.alloc_n<double>((size_t)m * K));
  double ll[TPG_ADMIX_MAX_FOLDS], cv = 0.0;
  int64_t cnt[TPG_ADMIX_MAX_FOLDS], het[TPG_ADMIX_MAX_FOLDS];
  int32_t it[TPG_ADMIX_MAX_FOLDS], conv[TPG_ADMIX_MAX_FOLDS];
  for (int f = 0; f < folds; f++) {
    tpg_view* t = nullptr;
    TPG_TRY(admix_view_holdout(ctx, v, folds, f, cv_seed, &t, nullptr));
    ViewPtr train(t);  // back to the pool before the next fold's is made: one extra view (L and T) at a time
    if (squarem)
      TPG_TRY(tpg_admix_em_squarem(ctx, t, ploidy, K, params, q0 ? iq.dev<double>() : nullptr, f0 ? ifr.dev<double>() : nullptr,
                                   Qd.as<double>(), Pd.as<double>(), nullptr, nullptr, &it[f], &conv[f], nullptr, nullptr, nullptr,
                                   nullptr));
    else
      TPG_TRY(tpg_admix_em(ctx, t, ploidy, K, params, q0 ? iq.dev<double>() : nullptr, f0 ? ifr.dev<double>() : nullptr, Qd.as<double>(),
                           Pd.as<double>(), nullptr, nullptr, &it[f], &conv[f]));
    TPG_TRY(tpg_admix_holdout_sums(ctx, v, t, K, Qd.as<double>(), Pd.as<double>(), &ll[f], &cnt[f], &het[f]));
  }
  TPG_TRY(tpg_admix_cv_error(folds, ll, cnt, het, nullptr, &cv));
  // nothing of the caller's has been written so far
  *cv_error = cv;
  for (int f = 0; f < folds; f++) {
    if (fold_ll) fold_ll[f] = ll[f];
    if (fold_count) fold_count[f] = cnt[f];
    if (fold_het) fold_het[f] = het[f];
    if (fold_iter) fold_iter[f] = it[f];
    if (fold_converged) fold_converged[f] = conv[f];
  }
  return TPG_OK;
}
}  // namespace

extern "C" int tpg_admix_cv(tpg_ctx* ctx, const tpg_view* v, const double* ploidy, int K, const tpg_admix_params* params, int folds,
                            uint64_t cv_seed, const double* q0, const double* f0, double* cv_error, double* fold_ll,
                            int64_t* fold_count, int64_t* fold_het, int32_t* fold_iter, int32_t* fold_converged) {
  return admix_cv(false, ctx, v, ploidy, K, params, folds, cv_seed, q0, f0, cv_error, fold_ll, fold_count, fold_het, fold_iter,
                  fold_converged);
}

extern "C" int tpg_admix_cv_squarem(tpg_ctx* ctx, const tpg_view* v, const double* ploidy, int K, const tpg_admix_params* params,
                                    int folds, uint64_t cv_seed, const double* q0, const double* f0, double* cv_error, double* fold_ll,
                                    int64_t* fold_count, int64_t* fold_het, int32_t* fold_iter, int32_t* fold_converged) {
  return admix_cv(true, ctx, v, ploidy, K, params, folds, cv_seed, q0, f0, cv_error, fold_ll, fold_count, fold_het, fold_iter,
                  fold_converged);
}
