// lsq.hip -- include/tpg.h "least-squares projection": the per-individual normal equations of every individual of a view in one
// pass family over the T layout, on the FP64 matrix cores, and the batched solve (csrc/host/host_lsq.h, the text the host runs
// too).
//
// The sweep.  Per individual i the columns are  P = L (L + 1) / 2 masked pair sums  A_i[a,b] = sum_j mask_ij V[j,a] V[j,b],  the
// count  t_i = sum_j mask_ij  and the L right-hand sides  b_i[a] = sum_j z_ij V[j,a].  They are two chains of
// v_mfma_f64_16x16x4_f64 (rows = 16 individuals, columns = 16 output columns, k = 4 loci): the MASK chain with A operand 0 / 1 and
// P + 1 columns (the pairs, then the count: a column whose B operand is 1), and the Z chain with A operand z and L columns.
// Column tiles of 16: TM = ceil((P + 1) / 16) mask tiles, then TZ = ceil(L / 16) z tiles (L = 32: 34 + 2 = 36 tiles).
//
// Operand mapping.  The MFMA takes A[row = lane & 15][k = lane >> 4] and B[k = lane >> 4][col = lane & 15], one double per lane.
// A T block holds 32 individuals x 128 loci: T lane (r, h), dword s, element e <-> individual 32 rt + r, locus 128 kg + 32 s +
// 16 h + e.  A wave owns the 16 individuals 16 hh .. 16 hh + 15 of one T row tile (hh = 0, 1); its MFMA lane (r16, kq) reads
// the 8 bytes -- dwords 2 (kq >> 1) and 2 (kq >> 1) + 1 -- of T lane (16 hh + r16, h = kq & 1): 32 codes of ITS individual, one
// per MFMA step t = 0 .. 31.  The k order inside an MFMA is free as long as A and B agree, so step t of lane group kq is locus
//     jl(kq, t) = 64 (kq >> 1) + 16 (kq & 1) + 32 (t >> 4) + (t & 15)
// of the block: the four kq groups partition the 128 loci, no code is moved between lanes, and the half-tile of a wave is one
// 512-byte read.  The B side follows: V's L columns, a row of ones, center and 1 / scale of the block are staged in LDS at
// SLOT 4 t + kq, so that the four lanes of a column read four adjacent doubles; rows are LSQ_RS = 132 doubles apart (8 dwords
// modulo the 64 banks: 8 distinct columns of V x 4 kq fill the banks once).  A lane forms its B value when it reads it:
// vs[row1][slot] * vs[row2][slot], where (row1, row2) = (a, b) for a pair column, (ones, ones) for the count, (a, ones) for a
// right-hand side -- one multiply and two LDS reads against a 32-cycle MFMA, and no m x P table anywhere.  Padding columns of
// the last tile point at the ones row and are not stored.
//
// Geometry.  A workgroup is 4 waves = 2 T row tiles x 2 halves = 64 individuals; they share the staged block.  blockIdx.y is the
// locus split (ascending chunks of whole T blocks, at least LSQ_CHUNK_LOCI loci each, at most LSQ_MAX_SPLIT), blockIdx.z the
// column pass: LSQ_CT = 8 column tiles = 128 columns per pass (32 accumulator doubles per lane), every pass re-reading the
// packed panel (n m / 4 bytes).  L = 10: 5 tiles, one pass; L = 20: 16 tiles, two; L = 32: 36 tiles, five.  A workgroup writes
// its partial sums to part[split][column][row]; the reduce kernel adds the splits in ascending order -- no floating-point
// atomics, the same bits on every call.  Padding rows and loci hold code 3: mask 0 and z 0.
//
// The solve.  A workgroup is one wave holding 64 / G teams, one individual each, every team with host_lsq_ws_doubles(L) doubles
// of LDS (528 + 64 at L = 32: 18.5 KB for the 4 teams of G = 16).  G is 4 up to L = 4, 8 up to L = 12, else 16: row k of the
// Cholesky factor has L - 1 - k independent entries, so a team wider than about L / 2 idles through most rows, while one lane
// per individual would put the packed matrix in scratch.  The team's sync() is the barrier of the one-wave workgroup.  The
// singular rows are counted with one integer atomic per such row.
#include "common.h"
#include "devfrag.h"
#include "host/host_lsq.h"

namespace {

constexpr int LSQ_WAVE = 64;
constexpr int LSQ_LB = 128;          // loci per staged block: one T block
constexpr int LSQ_RS = 132;          // doubles between staged rows
constexpr int LSQ_CT = 8;            // column tiles per pass
constexpr int LSQ_CHUNK_LOCI = 512;  // a split chunk is never shorter (tests/test_gpu_lsq.py names it)
constexpr int LSQ_MAX_SPLIT = 64;

__global__ void lsq_inv_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ y) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) y[i] = 1.0 / x[i];
}

// LDS: (L + 1) rows of LSQ_RS doubles (V's columns, then ones), center[128], inv_scale[128], all in slot order
__global__ __launch_bounds__(256) void lsq_sweep_kernel(const uint4* __restrict__ T, int64_t nrowtiles, int64_t KG, int S, int64_t m,
                                                        const double* __restrict__ center, const double* __restrict__ inv_scale,
                                                        const double* __restrict__ V, int L, int P, int TM, int ntiles,
                                                        double* __restrict__ part, int64_t rows_pad) {
  extern __shared__ double lsq_lds[];
  double* vs = lsq_lds;
  double* cs = lsq_lds + (size_t)(L + 1) * LSQ_RS;
  double* is = cs + LSQ_LB;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, kq = lane >> 4;
  const int64_t rt = (int64_t)blockIdx.x * 2 + (wv >> 1);
  const int hh = wv & 1;
  const int split = blockIdx.y;
  const int64_t b0 = KG * split / S, b1 = KG * (split + 1) / S;
  const int t0 = blockIdx.z * LSQ_CT;
  const bool has_z = t0 + LSQ_CT > TM;
  // the two staged rows behind this lane's column of every tile of the pass
  int o1[LSQ_CT], o2[LSQ_CT];
#pragma unroll
  for (int ct = 0; ct < LSQ_CT; ct++) {
    const int tile = t0 + ct;
    int a = L, b = L;
    if (tile < TM) {
      int q = 16 * tile + r16;
      if (q < P) {
        a = 0;
        while (q >= L - a) { q -= L - a; a++; }
        b = a + q;
      }
    } else if (16 * (tile - TM) + r16 < L) {
      a = 16 * (tile - TM) + r16;
    }
    o1[ct] = a * LSQ_RS;
    o2[ct] = b * LSQ_RS;
  }
  double acc[LSQ_CT][4];
#pragma unroll
  for (int ct = 0; ct < LSQ_CT; ct++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) acc[ct][reg] = 0.0;
  const bool live = rt < nrowtiles;
  const uint2* tp = (const uint2*)T + ((live ? rt : 0) * KG * 64 + (16 * hh + r16) + 32 * (kq & 1)) * 2 + (kq >> 1);
  for (int64_t blk = b0; blk < b1; blk++) {
    uint2 w2 = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
    if (live) w2 = tp[blk * 128];
    __syncthreads();
    for (int idx = threadIdx.x; idx < (L + 3) * LSQ_LB; idx += 256) {
      const int row = idx >> 7, jl = idx & 127;
      const int slot = 4 * ((((jl >> 5) & 1) << 4) | (jl & 15)) + (((jl >> 6) << 1) | ((jl >> 4) & 1));
      const int64_t j = blk * LSQ_LB + jl;
      if (row < L) vs[row * LSQ_RS + slot] = j < m ? V[j + (int64_t)row * m] : 0.0;
      else if (row == L) vs[row * LSQ_RS + slot] = 1.0;
      else if (row == L + 1) cs[slot] = j < m ? center[j] : 0.0;
      else is[slot] = j < m ? inv_scale[j] : 0.0;
    }
    __syncthreads();
    const uint32_t w[2] = {w2.x, w2.y};
#pragma unroll
    for (int d = 0; d < 2; d++) {
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int slot = 4 * (16 * d + e) + kq;
        const int code = (w[d] >> tpg_elem_shift(e)) & 3;
        const double am = code == 3 ? 0.0 : 1.0;
        double az = 0.0;
        if (has_z) {
          az = ((double)code - cs[slot]) * is[slot];
          if (code == 3) az = 0.0;
        }
#pragma unroll
        for (int ct = 0; ct < LSQ_CT; ct++) {
          if (t0 + ct < ntiles) {
            const double bv = vs[o1[ct] + slot] * vs[o2[ct] + slot];
            *(v4d*)acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(t0 + ct < TM ? am : az, bv, *(v4d*)acc[ct], 0, 0, 0);
          }
        }
      }
    }
  }
  // C/D: column = lane & 15, row = (lane >> 4) + 4 reg
  if (live) {
    const int64_t ncp = (int64_t)ntiles * 16;
#pragma unroll
    for (int ct = 0; ct < LSQ_CT; ct++) {
      if (t0 + ct < ntiles) {
        const int64_t col = 16 * (int64_t)(t0 + ct) + r16;
#pragma unroll
        for (int reg = 0; reg < 4; reg++)
          part[((int64_t)split * ncp + col) * rows_pad + rt * 32 + 16 * hh + kq + 4 * reg] = acc[ct][reg];
      }
    }
  }
}

// A (n x P), n_typed and b (n x L) = the partial sums of the splits, in split order
__global__ void lsq_reduce_kernel(const double* __restrict__ part, int S, int64_t ncp, int64_t rows_pad, int64_t n, int L, int P, int TM,
                                  double* __restrict__ A, double* __restrict__ b, int64_t* __restrict__ n_typed) {
  const int64_t total = n * (P + 1 + L);
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = idx % n, c = idx / n;
    const int64_t col = c <= P ? c : 16 * (int64_t)TM + (c - P - 1);
    double s = 0.0;
    for (int sp = 0; sp < S; sp++) s += part[((int64_t)sp * ncp + col) * rows_pad + i];
    if (c < P) A[i + c * n] = s;
    else if (c == P) n_typed[i] = (int64_t)s;  // a sum of ones: exact
    else b[i + (c - P - 1) * n] = s;
  }
}

template <int G>
__global__ __launch_bounds__(LSQ_WAVE) void lsq_solve_kernel(const double* __restrict__ A, const double* __restrict__ b,
                                                             const int64_t* __restrict__ n_typed, int64_t n, int L, double* __restrict__ out,
                                                             unsigned long long* __restrict__ n_singular) {
  extern __shared__ double lsq_solve_lds[];
  constexpr int TEAMS = LSQ_WAVE / G;
  const int team = (int)(threadIdx.x / G);
  const int64_t i = (int64_t)blockIdx.x * TEAMS + team;
  double* ws = lsq_solve_lds + (size_t)team * host_lsq_ws_doubles(L);
  const bool live = i < n;  // (a team beyond the batch works on a row of zeros and stores nothing: it keeps the barriers whole)
  const TpgTeam<G> tm;
  const int singular = host_lsq_solve_row(tm, L, live ? A + i : nullptr, n, live ? b + i : nullptr, n, live ? n_typed[i] : 0, ws,
                                          live ? out + i : nullptr, n);
  if (live && singular && tm.lane() == 0) atomicAdd(n_singular, 1ull);
}

int lsq_team_lanes(int L) { return L <= 4 ? 4 : L <= 12 ? 8 : 16; }

// device pointers throughout; d_count is zeroed here
int lsq_solve_launch(tpg_ctx* ctx, const double* dA, const double* db, const int64_t* dnt, int64_t n, int L, double* dout,
                     unsigned long long* d_count) {
  TPG_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), ctx->stream));
  if (n == 0) return TPG_OK;
  const int G = lsq_team_lanes(L), teams = LSQ_WAVE / G;
  const int64_t blocks = ceil_div(n, teams);
  TPG_REQUIRE(blocks <= 0x7FFFFFFF, TPG_EINVAL, "n = %lld is more than one launch takes", (long long)n);
  const size_t lds = sizeof(double) * (size_t)teams * (size_t)host_lsq_ws_doubles(L);
#define LSQ_GO(G_) TPG_LAUNCH(ctx, "lsq_solve", lsq_solve_kernel<G_>, dim3((unsigned)blocks), dim3(LSQ_WAVE), lds, dA, db, dnt, n, L, dout, d_count)
  if (G == 4) LSQ_GO(4);
  else if (G == 8) LSQ_GO(8);
  else LSQ_GO(16);
#undef LSQ_GO
  TPG_CHECK_LAUNCH();
  return TPG_OK;
}

// the split of KG locus blocks for `row_blocks` workgroups of rows: the rule of run_sweep (pca.hip) -- double S while the grid
// is short of four workgroups per CU -- with chunks of at least LSQ_CHUNK_LOCI loci and S <= LSQ_MAX_SPLIT
int lsq_split(tpg_ctx* ctx, int64_t row_blocks, int64_t KG) {
  int64_t S = 1;
  while (row_blocks * S < 4 * (int64_t)ctx->num_cu && S * 2 * (LSQ_CHUNK_LOCI / LSQ_LB) <= KG && S < LSQ_MAX_SPLIT) S *= 2;
  return (int)S;
}

// device pointers throughout: dA n x P, db n x L, dnt[n]; center, scale and V have been checked
int lsq_sweep(tpg_ctx* ctx, const tpg_view* v, const double* d_center, const double* d_scale, const double* d_V, int L, double* dA,
              double* db, int64_t* dnt, DevArena& sc) {
  const int64_t n = v->n, m = v->m;
  const int P = host_lsq_pairs(L), TM = (P + 1 + 15) / 16, TZ = (L + 15) / 16, ntiles = TM + TZ;
  double* d_inv = nullptr;
  TPG_TRY(sc.get(&d_inv, (size_t)m));
  TPG_LAUNCH(ctx, "lsq_inv_scale", lsq_inv_kernel, dim3(1024), dim3(256), 0, d_scale, m, d_inv);
  TPG_TRY(tpg_check_finite(ctx, d_inv, m, sc, "1 / scale (a scale of zero)"));
  TPG_TRY(tpg_view_need_T(ctx, v));
  const int64_t nrowtiles = v->Q * 4, rows_pad = nrowtiles * 32, row_blocks = ceil_div(nrowtiles, 2);
  TPG_REQUIRE(row_blocks <= 0x7FFFFFFF, TPG_EINVAL, "n = %lld is more than one launch takes", (long long)n);
  const int S = lsq_split(ctx, row_blocks, v->KG);
  const int64_t ncp = (int64_t)ntiles * 16;
  DevBuf part;
  TPG_TRY(part.alloc_n<double>((size_t)S * (size_t)ncp * (size_t)rows_pad));
  const int passes = (ntiles + LSQ_CT - 1) / LSQ_CT;
  const size_t lds = sizeof(double) * ((size_t)(L + 1) * LSQ_RS + 2 * LSQ_LB);
  TPG_LAUNCH(ctx, "lsq_sweep", lsq_sweep_kernel, dim3((unsigned)row_blocks, (unsigned)S, (unsigned)passes), dim3(256), lds, v->T,
             nrowtiles, v->KG, S, m, d_center, (const double*)d_inv, d_V, L, P, TM, ntiles, part.as<double>(), rows_pad);
  TPG_LAUNCH(ctx, "lsq_reduce", lsq_reduce_kernel, dim3(1024), dim3(256), 0, (const double*)part.as<double>(), S, ncp, rows_pad, n, L, P,
             TM, dA, db, dnt);
  TPG_CHECK_LAUNCH();
  TPG_HIP(hipStreamSynchronize(ctx->stream));  // part goes back to the pool
  TPG_TRY(tpg_check_finite(ctx, dA, n * P, sc, "A (a sum that overflowed)"));
  TPG_TRY(tpg_check_finite(ctx, db, n * L, sc, "b (a sum that overflowed)"));
  return TPG_OK;
}

struct LsqIn {
  InBuf ic, is, iv;
};

// the argument checks and uploads the two view entry points share
int lsq_view_args(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale, const double* V, int L, LsqIn& in,
                  DevArena& sc) {
  TPG_REQUIRE(L >= 1 && L <= TPG_LSQ_MAX_L, TPG_EINVAL, "L = %d outside [1, %d]", L, TPG_LSQ_MAX_L);
  TPG_REQUIRE(v->m >= 1, TPG_EINVAL, "the view has no loci");
  TPG_TRY(in.ic.init(ctx, center, sizeof(double) * (size_t)v->m));
  TPG_TRY(in.is.init(ctx, scale, sizeof(double) * (size_t)v->m));
  TPG_TRY(in.iv.init(ctx, V, sizeof(double) * (size_t)v->m * (size_t)L));
  TPG_TRY(tpg_check_finite(ctx, in.ic.dev<double>(), v->m, sc, "center"));
  TPG_TRY(tpg_check_finite(ctx, in.is.dev<double>(), v->m, sc, "scale"));
  TPG_TRY(tpg_check_finite(ctx, in.iv.dev<double>(), v->m * L, sc, "V"));
  return TPG_OK;
}

}  // namespace

extern "C" int tpg_lsq_normal(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale, const double* V, int L, double* A,
                              double* b, int64_t* n_typed) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && center && scale && V && A && b && n_typed, TPG_EINVAL, "null argument");
  LsqIn in;
  DevArena sc;
  TPG_TRY(lsq_view_args(ctx, v, center, scale, V, L, in, sc));
  const int64_t n = v->n;
  if (n == 0) return TPG_OK;
  const int P = host_lsq_pairs(L);
  OutBuf oa, ob, ot;
  TPG_TRY(oa.init(A, sizeof(double) * (size_t)n * P));
  TPG_TRY(ob.init(b, sizeof(double) * (size_t)n * L));
  TPG_TRY(ot.init(n_typed, sizeof(int64_t) * (size_t)n));
  TPG_TRY(lsq_sweep(ctx, v, in.ic.dev<double>(), in.is.dev<double>(), in.iv.dev<double>(), L, oa.dev<double>(), ob.dev<double>(),
                    ot.dev<int64_t>(), sc));
  TPG_TRY(oa.commit(ctx));
  TPG_TRY(ob.commit(ctx));
  return ot.commit(ctx);
}

extern "C" int tpg_lsq_solve(tpg_ctx* ctx, const double* A, const double* b, const int64_t* n_typed, int64_t n, int L, double* out,
                             int64_t* n_singular) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && A && b && n_typed && out, TPG_EINVAL, "null argument");
  TPG_REQUIRE(n >= 0, TPG_EINVAL, "n = %lld is negative", (long long)n);
  TPG_REQUIRE(L >= 1 && L <= TPG_LSQ_MAX_L, TPG_EINVAL, "L = %d outside [1, %d]", L, TPG_LSQ_MAX_L);
  const int P = host_lsq_pairs(L);
  InBuf ia, ib, it;
  OutBuf oo;
  TPG_TRY(ia.init(ctx, A, sizeof(double) * (size_t)n * P));
  TPG_TRY(ib.init(ctx, b, sizeof(double) * (size_t)n * L));
  TPG_TRY(it.init(ctx, n_typed, sizeof(int64_t) * (size_t)n));
  TPG_TRY(oo.init(out, sizeof(double) * (size_t)n * L));
  DevArena sc;
  if (n > 0) {
    TPG_TRY(tpg_check_finite(ctx, ia.dev<double>(), n * P, sc, "A"));
    TPG_TRY(tpg_check_finite(ctx, ib.dev<double>(), n * L, sc, "b"));
  }
  unsigned long long* d_count = nullptr;
  TPG_TRY(sc.get(&d_count, (size_t)1));
  TPG_TRY(lsq_solve_launch(ctx, ia.dev<double>(), ib.dev<double>(), it.dev<int64_t>(), n, L, oo.dev<double>(), d_count));
  unsigned long long u = 0;
  TPG_HIP(tpg_fetch_small(ctx, &u, d_count, sizeof u));
  TPG_TRY(oo.commit(ctx));
  if (n_singular) *n_singular = (int64_t)u;
  return TPG_OK;
}

extern "C" int tpg_predict_lsq(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale, const double* V, int L,
                               double* out, int64_t* n_typed_out, int64_t* n_singular) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && center && scale && V && out, TPG_EINVAL, "null argument");
  LsqIn in;
  DevArena sc;
  TPG_TRY(lsq_view_args(ctx, v, center, scale, V, L, in, sc));
  const int64_t n = v->n;
  if (n_singular) *n_singular = 0;
  if (n == 0) return TPG_OK;
  const int P = host_lsq_pairs(L);
  OutBuf oo;
  TPG_TRY(oo.init(out, sizeof(double) * (size_t)n * L));
  double *dA = nullptr, *db = nullptr;
  int64_t* dnt = nullptr;
  unsigned long long* d_count = nullptr;
  TPG_TRY(sc.get(&dA, (size_t)n * P));
  TPG_TRY(sc.get(&db, (size_t)n * L));
  TPG_TRY(sc.get(&dnt, (size_t)n));
  TPG_TRY(sc.get(&d_count, (size_t)1));
  // A, b and the counts stay on the device between the sweep and the solve
  TPG_TRY(lsq_sweep(ctx, v, in.ic.dev<double>(), in.is.dev<double>(), in.iv.dev<double>(), L, dA, db, dnt, sc));
  TPG_TRY(lsq_solve_launch(ctx, dA, db, dnt, n, L, oo.dev<double>(), d_count));
  unsigned long long u = 0;
  TPG_HIP(tpg_fetch_small(ctx, &u, d_count, sizeof u));
  TPG_TRY(tpg_deliver(ctx, n_typed_out, (const int64_t*)dnt, (size_t)n));
  TPG_TRY(oo.commit(ctx));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  if (n_singular) *n_singular = (int64_t)u;
  return TPG_OK;
}
