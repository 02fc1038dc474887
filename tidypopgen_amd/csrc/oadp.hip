// oadp.hip -- include/tpg.h "OADP projection" for all new individuals in one launch.  The arithmetic of one individual is
// host_oadp_project (csrc/host/host_oadp.h), the text the host runs too; here its team is a group of G lanes of one wave.
//
// Geometry.  A workgroup is one wave; it holds 64 / G teams, one individual each, and every team has its own workspace in LDS:
// the (K+1) x (K+1) matrix that is first M, then W = A S, then C' and Z, column-major with an odd leading dimension, plus K+1
// doubles (8.9 KB at K = 32, 3.7 KB at K = 20).  G is the smallest of 4, 8, 16 that gives every column pair of a Jacobi round
// its own lane (ceil((K+1)/2) pairs): a lane forms the three dot products of its pair over the rows serially and rotates the
// two columns, so no sum is split over lanes, no value travels between lanes but through LDS, and a row's bits depend on
// nothing but its own inputs.  One thread per individual would need the matrix in scratch; a whole wave per individual would
// leave 47 of 64 lanes without a pair.  The team's sync() is the workgroup barrier -- of a single wave -- and any() the
// barrier's OR: the teams of a wave sweep until the last of them has converged, and a sweep over converged columns rotates
// nothing.  No floating-point atomics; the degenerate rows are counted with one integer atomic per such row.
#include "common.h"
#include "devfrag.h"
#include "host/host_oadp.h"

namespace {

constexpr int OADP_WAVE = 64;

// LDS: 32 doubles of singular values, then 64 / G workspaces
template <int G>
__global__ __launch_bounds__(OADP_WAVE) void oadp_kernel(const double* __restrict__ XV, const double* __restrict__ X_norm, int64_t n, int K,
                                                          const double* __restrict__ sval, double* __restrict__ out,
                                                          unsigned long long* __restrict__ n_degenerate) {
  extern __shared__ double oadp_lds[];
  constexpr int TEAMS = OADP_WAVE / G;
  const int team = (int)(threadIdx.x / G);
  const int64_t i = (int64_t)blockIdx.x * TEAMS + team;
  double* d = oadp_lds;
  double* ws = oadp_lds + HOST_OADP_KMAX + (size_t)team * host_oadp_ws_doubles(K);
  if ((int)threadIdx.x < K) d[threadIdx.x] = sval[threadIdx.x];
  __syncthreads();
  const bool live = i < n;  // (a team beyond the batch works on a row of zeros and stores nothing: it keeps the barriers whole)
  const TpgTeam<G> t;
  const int degenerate = host_oadp_project(t, K, live ? XV + i : nullptr, n, live ? X_norm[i] : 0.0, d, ws, live ? out + i : nullptr, n);
  if (live && degenerate && t.lane() == 0) atomicAdd(n_degenerate, 1ull);
}

int oadp_team_lanes(int K) { return K + 1 <= 8 ? 4 : K + 1 <= 16 ? 8 : 16; }

// device pointers throughout; d_count is zeroed here
int oadp_launch(tpg_ctx* ctx, const double* dXV, const double* dnorm, int64_t n, int K, const double* dsval, double* dout,
                unsigned long long* d_count) {
  TPG_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), ctx->stream));
  if (n == 0) return TPG_OK;
  const int G = oadp_team_lanes(K), teams = OADP_WAVE / G;
  const int64_t blocks = ceil_div(n, teams);
  TPG_REQUIRE(blocks <= 0x7FFFFFFF, TPG_EINVAL, "n = %lld is more than one launch takes", (long long)n);
  const size_t lds = sizeof(double) * ((size_t)HOST_OADP_KMAX + (size_t)teams * (size_t)host_oadp_ws_doubles(K));
#define OADP_GO(G_) \
  TPG_LAUNCH(ctx, "oadp", oadp_kernel<G_>, dim3((unsigned)blocks), dim3(OADP_WAVE), lds, dXV, dnorm, n, K, dsval, dout, d_count)
  if (G == 4) OADP_GO(4);
  else if (G == 8) OADP_GO(8);
  else OADP_GO(16);
#undef OADP_GO
  TPG_CHECK_LAUNCH();
  return TPG_OK;
}

int oadp_check_args(tpg_ctx* ctx, int K, const double* sval, HostIn<double>& hs) {
  TPG_REQUIRE(K >= 1 && K <= HOST_OADP_KMAX, TPG_EINVAL, "K = %d outside [1, %d]", K, HOST_OADP_KMAX);
  TPG_TRY(hs.init(ctx, sval, K));
  const int bad = host_oadp_check_sval(hs.p, K);
  TPG_REQUIRE(bad != 1, TPG_ENUMERIC, "sval holds a value that is not finite");
  TPG_REQUIRE(bad == 0, TPG_EINVAL, "sval must be positive and descending");
  return TPG_OK;
}

}  // namespace

extern "C" int tpg_oadp_proj(tpg_ctx* ctx, const double* XV, const double* X_norm, int64_t n, int K, const double* sval, double* out,
                             int64_t* n_degenerate) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && XV && X_norm && sval && out, TPG_EINVAL, "null argument");
  TPG_REQUIRE(n >= 0, TPG_EINVAL, "n = %lld is negative", (long long)n);
  HostIn<double> hs;
  TPG_TRY(oadp_check_args(ctx, K, sval, hs));
  InBuf ixv, inm, isv;
  OutBuf oo;
  TPG_TRY(ixv.init(ctx, XV, sizeof(double) * (size_t)n * K));
  TPG_TRY(inm.init(ctx, X_norm, sizeof(double) * (size_t)n));
  TPG_TRY(isv.init(ctx, sval, sizeof(double) * (size_t)K));
  TPG_TRY(oo.init(out, sizeof(double) * (size_t)n * K));
  DevArena sc;
  if (n > 0) {
    TPG_TRY(tpg_check_finite(ctx, ixv.dev<double>(), n * K, sc, "XV"));
    TPG_TRY(tpg_check_finite(ctx, inm.dev<double>(), n, sc, "X_norm"));
  }
  unsigned long long* d_count = nullptr;
  TPG_TRY(sc.get(&d_count, (size_t)1));
  TPG_TRY(oadp_launch(ctx, ixv.dev<double>(), inm.dev<double>(), n, K, isv.dev<double>(), oo.dev<double>(), d_count));
  unsigned long long u = 0;
  TPG_HIP(tpg_fetch_small(ctx, &u, d_count, sizeof u));
  TPG_TRY(oo.commit(ctx));
  if (n_degenerate) *n_degenerate = (int64_t)u;
  return TPG_OK;
}

extern "C" int tpg_predict_oadp(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale, const double* V, int K,
                                const double* sval, double* out, double* XV_out, int64_t* n_degenerate) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && center && scale && V && sval && out, TPG_EINVAL, "null argument");
  HostIn<double> hs;
  TPG_TRY(oadp_check_args(ctx, K, sval, hs));
  const int64_t n = v->n;
  InBuf ic, is, iv, isv;
  OutBuf oo;
  TPG_TRY(ic.init(ctx, center, sizeof(double) * (size_t)v->m));
  TPG_TRY(is.init(ctx, scale, sizeof(double) * (size_t)v->m));
  TPG_TRY(iv.init(ctx, V, sizeof(double) * (size_t)v->m * (size_t)K));
  TPG_TRY(isv.init(ctx, sval, sizeof(double) * (size_t)K));
  TPG_TRY(oo.init(out, sizeof(double) * (size_t)n * K));
  DevArena sc;
  double *dXV = nullptr, *dnorm = nullptr;
  unsigned long long* d_count = nullptr;
  TPG_TRY(sc.get(&dXV, (size_t)n * K));
  TPG_TRY(sc.get(&dnorm, (size_t)n));
  TPG_TRY(sc.get(&d_count, (size_t)1));
  // XV and the squared norms stay on the device between the sweep and the projection
  TPG_TRY(tpg_sweep_indiv_colscale(ctx, v, ic.dev<double>(), is.dev<double>(), iv.dev<double>(), K, dXV, dnorm));
  if (n > 0) {
    TPG_TRY(tpg_check_finite(ctx, dXV, n * K, sc, "XV (center, scale or V)"));
    TPG_TRY(tpg_check_finite(ctx, dnorm, n, sc, "X_norm (center or scale)"));
  }
  TPG_TRY(oadp_launch(ctx, dXV, dnorm, n, K, isv.dev<double>(), oo.dev<double>(), d_count));
  unsigned long long u = 0;
  TPG_HIP(tpg_fetch_small(ctx, &u, d_count, sizeof u));
  TPG_TRY(tpg_deliver(ctx, XV_out, (const double*)dXV, (size_t)n * K));
  TPG_TRY(oo.commit(ctx));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  if (n_degenerate) *n_degenerate = (int64_t)u;
  return TPG_OK;
}
