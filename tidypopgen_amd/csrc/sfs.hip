// sfs.hip -- site frequency spectra with hypergeometric down-projection (include/tpg.h "site frequency spectra"): the 1-D
// spectra of every group and the joint spectra of every pair of groups, per block of loci.
//
// The reference has no SFS code; the arithmetic is the definition in include/tpg.h, restated in tests/sfs_ref.py.
//
// If H is the matrix whose row j holds, for every group g, the n_g + 1 projection weights of locus j (exact zeros where the
// locus is not usable for g), all joint spectra of a block are the blocks of H'H over its loci: a Gram matrix on
// v_mfma_f64_16x16x4_f64.  One more column of H holds 1.0 at every locus: its products with the others are the 1-D spectra,
// so sfs comes out of the same chains (and, when jsfs is not asked for, only the tiles of that column are run).
//
// Behind the count sweep of tpg_grouped_counts (loci.hip), whose table stays in HBM:
//   sfs_nused      n_used1 / n_used2: per 64 loci the t bits of 16 + 16 groups as wave ballots, a popcount per pair and an
//                  INTEGER atomic add per (block, pair) and slice of the block: exact in any order.
//   sfs_operands   one thread per (staged locus, group): x, v from the table, flip, keep, then host/host_sfs.h ONCE, written into
//                  the operand scratch in the fragment order the Gram kernel reads (pcrelate.hip):
//                      F[((c >> 4) * SM + (r >> 2)) * 64 + 16 (r & 3) + (c & 15)] = H[staged row r][column c],  SM = rows / 4,
//                  so an MFMA operand (16 columns x 4 loci) is one coalesced 512-byte read, one double per lane.
//   sfs_gram       a workgroup is (piece, 64 x 64 tile tR <= tC): 4 waves of 32 x 32 (2 x 2 MFMA tiles), 4 operand reads for 4
//                  MFMAs, one step ahead of their use.  A piece is a run of staged loci of one SEGMENT of one block; the
//                  accumulators of a segment live in its partial tile (4096 doubles in register order) between pieces: load,
//                  add the piece, store.
//   sfs_reduce     adds the partial tiles of a block's segments in ascending segment order and writes sfs and both triangles
//                  of jsfs from the one tile (symmetric bit for bit).
// Parallelism.  At W = 603 there are 55 tiles for 256 CUs and the usual call is ONE block of 10^6 loci, so a block of L loci is
// cut into tpg_sfs_segments(L, W) segments (equal multiples of 64 loci): a function of (L, W) alone.  The steps of a chain are
// the loci 4 t .. 4 t + 3 counted from the segment's start, whatever the staging: a cell depends on (lo, hi) and the arguments
// alone.  The host deals the operand scratch (a bound independent of m) to the unfinished segments of a batch of blocks round
// by round; stores and loads of doubles are exact, so the rounds do not enter a result.  No floating-point atomics.
#include "common.h"
#include "devfrag.h"
#include "host/host_sfs.h"

#include <string.h>

#include <algorithm>

namespace {

constexpr int SFS_C = TPG_SFS_CHUNK_LOCI;              // loci per staged chunk (a workgroup of the operand kernel)
constexpr int SFS_T = 64;                              // columns per tile side
constexpr int64_t SFS_SEG_MIN = 1024;                  // loci below which a block is not cut further
constexpr int64_t SFS_SEG_MAX = 64;                    // most segments of a block
constexpr int64_t SFS_WG_TARGET = 1024;                // workgroups the cut aims at: segments x tiles
constexpr size_t SFS_OPER_CAP = (size_t)128 << 20;     // bytes of staged operand
constexpr int64_t SFS_PT_CAP = 2048;                   // partial tiles of a batch of blocks
constexpr int64_t SFS_TILE = SFS_T * SFS_T;            // doubles of a partial tile

struct SfsChunk { int64_t j0; int32_t count; int32_t pad; };                            // staged chunk -> its loci
struct SfsPiece { int64_t slot; int32_t row0; int32_t nloci; int32_t init; int32_t pad; };  // staged rows of one segment
struct SfsRed { int64_t slot; int64_t b; int32_t nseg; int32_t pad; };                   // a block's partial tiles

int sfs_ntile(int64_t W) { return (int)ceil_div(W + 1, SFS_T); }  // + the column of ones
int64_t sfs_segments(int64_t L, int64_t W) {
  const int64_t nt = sfs_ntile(W), tri = nt * (nt + 1) / 2;
  const int64_t cap = std::min<int64_t>(SFS_SEG_MAX, std::max<int64_t>(1, SFS_WG_TARGET / tri));
  return std::min(std::max<int64_t>(1, ceil_div(L, SFS_SEG_MIN)), cap);
}

struct SfsPlan {
  int64_t Wp = 0;      // padded operand width
  int nt = 0;          // tiles a side
  int ntpu = 0;        // tiles a segment runs: the upper triangle, or the column of ones alone
  int64_t rows = 0;    // staged loci (a multiple of SFS_C)
  int64_t PT = 0;      // partial tiles
  size_t b_frag = 0, b_part = 0, b_pieces = 0, b_chunks = 0, b_red = 0, b_groups = 0;
  size_t bytes() const { return b_frag + b_part + b_pieces + b_chunks + b_red + b_groups; }
};
SfsPlan sfs_plan(int64_t m, int G, int64_t W, int64_t nb, bool joint) {
  SfsPlan p;
  p.nt = sfs_ntile(W);
  p.Wp = (int64_t)p.nt * SFS_T;
  p.ntpu = joint ? p.nt * (p.nt + 1) / 2 : p.nt;
  const int64_t cap_rows = std::max<int64_t>(SFS_C, (int64_t)(SFS_OPER_CAP / (sizeof(double) * (size_t)p.Wp)) / SFS_C * SFS_C);
  p.rows = std::min(cap_rows, std::max<int64_t>(1, ceil_div(m, SFS_C)) * SFS_C);
  const int64_t one = sfs_segments(m, W) * p.ntpu;  // the most a block can take
  p.PT = std::max(one, std::min<int64_t>(SFS_PT_CAP, std::max<int64_t>(1, nb) * one));
  p.b_frag = sizeof(double) * (size_t)p.rows * (size_t)p.Wp;
  p.b_part = sizeof(double) * (size_t)p.PT * (size_t)SFS_TILE;
  p.b_pieces = sizeof(SfsPiece) * (size_t)p.PT;
  p.b_chunks = sizeof(SfsChunk) * (size_t)(p.rows / SFS_C);
  p.b_red = sizeof(SfsRed) * (size_t)p.PT;
  p.b_groups = sizeof(int32_t) * 2 * (size_t)G;
  return p;
}

// tile index y of a segment -> (tR, tC): row-major over the upper triangle, or (y, last) for the column of ones alone
__device__ __forceinline__ void sfs_tile_of(int y, int nt, int joint, int& tR, int& tC) {
  if (!joint) { tR = y; tC = nt - 1; return; }
  tR = 0;
  while (y >= nt - tR) { y -= nt - tR; tR++; }
  tC = tR + y;
}

// the t bits of 64 loci at a time.  grid (block, tile of 16 x 16 pairs -- or of 16 groups when only n_used1 is asked for --,
// slice): slice z takes the 64-locus groups z, z + gridDim.z, ... of the block.  gn[g] = n_g >= 1.
__global__ __launch_bounds__(256) void sfs_nused_kernel(const int32_t* __restrict__ valid, int Cpad, int G, const int32_t* __restrict__ gn,
                                                        const uint8_t* __restrict__ keep, const int64_t* __restrict__ lo,
                                                        const int64_t* __restrict__ hi, int full, unsigned long long* __restrict__ n1,
                                                        unsigned long long* __restrict__ n2) {
  __shared__ unsigned long long tm[32];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ntg = (G + 15) / 16;
  const int t1 = full ? (int)blockIdx.y % ntg : (int)blockIdx.y, t2 = full ? (int)blockIdx.y / ntg : (int)blockIdx.y;
  const int g1 = 16 * t1 + (threadIdx.x & 15), g2 = 16 * t2 + (threadIdx.x >> 4);
  const int64_t b = blockIdx.x, j_lo = lo[b], j_hi = hi[b];
  long long acc = 0;
  for (int64_t i = blockIdx.z; j_lo + 64 * i < j_hi; i += gridDim.z) {
    const int64_t j = j_lo + 64 * i + lane;
    const bool kp = j < j_hi && (!keep || keep[j]);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const int idx = wv * 8 + q;
      const int g = idx < 16 ? 16 * t1 + idx : 16 * t2 + idx - 16;
      bool t = false;
      if (kp && g < G) t = 2 * valid[j * Cpad + g] >= gn[g];
      const unsigned long long mask = __ballot(t);
      if (lane == 0) tm[idx] = mask;
    }
    __syncthreads();
    acc += __popcll(tm[threadIdx.x & 15] & tm[16 + (threadIdx.x >> 4)]);
  }
  if (g1 >= G || g2 >= G || acc == 0) return;
  if (n2 && full) atomicAdd(&n2[g1 + (int64_t)G * g2 + (int64_t)G * G * b], (unsigned long long)acc);
  if (n1 && g1 == g2) atomicAdd(&n1[g1 + (int64_t)G * b], (unsigned long long)acc);
}

// the place of H[row][column o + k] in the fragments
struct SfsFragAt {
  double* F;
  int64_t SM, t;  // steps of the scratch, step of the row
  int q16, o;     // 16 (row & 3), first column of the group
  __device__ double& operator()(int64_t k) const {
    const int c = o + (int)k;
    return F[(((int64_t)(c >> 4) * SM + t) << 6) + q16 + (c & 15)];
  }
};

// grid (staged chunk, 4 groups): thread (locus l of the chunk, group).  The thread of group 0 also writes the column of ones.
__global__ __launch_bounds__(256) void sfs_operands_kernel(const int32_t* __restrict__ cnt, int64_t Mpad, int Cpad, int G,
                                                           const int32_t* __restrict__ goff, const int32_t* __restrict__ gn, int W,
                                                           const uint8_t* __restrict__ keep, const uint8_t* __restrict__ flip,
                                                           const SfsChunk* __restrict__ chunks, double* __restrict__ F, int64_t SM) {
  const int l = threadIdx.x & 63, g = blockIdx.y * 4 + (threadIdx.x >> 6);
  const SfsChunk ch = chunks[blockIdx.x];
  const int64_t row = (int64_t)blockIdx.x * SFS_C + l, j = ch.j0 + l;
  const bool has = l < ch.count;
  SfsFragAt at{F, SM, row >> 2, 16 * (int)(row & 3), W};
  if (g == 0) at(0) = has ? 1.0 : 0.0;
  if (g >= G) return;
  const int n = gn[g];
  at.o = goff[g];
  bool usable = false;
  int64_t x = 0, v = 0;
  if (has && (!keep || keep[j])) {
    const int64_t plane = Mpad * Cpad, o = j * Cpad + g;
    const int n1 = cnt[o], n2 = cnt[plane + o], nv = cnt[2 * plane + o];
    v = 2 * (int64_t)nv;
    x = (int64_t)n1 + 2 * (int64_t)n2;
    if (flip && flip[j]) x = v - x;
    usable = v >= n;
  }
  if (usable) {
    host_sfs_row(x, v, (int64_t)n, at);
  } else {
    for (int k = 0; k <= n; k++) at(k) = 0.0;
  }
}

// partial tile of (piece's segment, tile y) += the piece's loci.  C/D: column = lane & 15, row = (lane >> 4) + 4 reg; the
// partial tile keeps the 16 accumulator registers of a wave as 16 runs of 64 lanes.
__global__ __launch_bounds__(256) void sfs_gram_kernel(const double* __restrict__ F, int64_t SM, const SfsPiece* __restrict__ pieces,
                                                       int nt, int joint, double* __restrict__ P) {
  const SfsPiece pc = pieces[blockIdx.x];
  int tR, tC;
  sfs_tile_of((int)blockIdx.y, nt, joint, tR, tC);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wi = wv >> 1, wj = wv & 1;
  const int64_t I0 = tR * 4 + wi * 2, J0 = tC * 4 + wj * 2;  // 16-column tiles
  double* slot = P + (pc.slot + blockIdx.y) * SFS_TILE + wv * 1024 + lane;
  v4d acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++) acc[a][b][reg] = pc.init ? 0.0 : slot[((a * 2 + b) * 4 + reg) * 64];
  const int steps = (pc.nloci + 3) >> 2;
  if (steps > 0) {
    const int64_t t0 = pc.row0 >> 2, tile = SM << 6;
    const double* pr = F + ((I0 * SM + t0) << 6) + lane;
    const double* pq = F + ((J0 * SM + t0) << 6) + lane;
    double ra[2], cb[2];
#pragma unroll
    for (int a = 0; a < 2; a++) {
      ra[a] = pr[a * tile];
      cb[a] = pq[a * tile];
    }
    for (int t = 0; t < steps; t++) {
      // the next step's operands leave before this step's MFMAs (the last step reads its own again: inside the fragments)
      const int64_t nx = (int64_t)(t + 1 < steps ? t + 1 : t) << 6;
      double ra2[2], cb2[2];
#pragma unroll
      for (int a = 0; a < 2; a++) {
        ra2[a] = pr[a * tile + nx];
        cb2[a] = pq[a * tile + nx];
      }
#pragma unroll
      for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[a], cb[b], acc[a][b], 0, 0, 0);
#pragma unroll
      for (int a = 0; a < 2; a++) {
        ra[a] = ra2[a];
        cb[a] = cb2[a];
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++) slot[((a * 2 + b) * 4 + reg) * 64] = acc[a][b][reg];
}

// grid (block of the batch, tile): the segments' partial tiles in ascending order; column W of the operand is the ones
__global__ __launch_bounds__(256) void sfs_reduce_kernel(const double* __restrict__ P, const SfsRed* __restrict__ red, int nt, int joint,
                                                         int ntpu, int64_t W, double* __restrict__ sfs, double* __restrict__ jsfs) {
  const SfsRed r = red[blockIdx.x];
  int tR, tC;
  sfs_tile_of((int)blockIdx.y, nt, joint, tR, tC);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wi = wv >> 1, wj = wv & 1, r16 = lane & 15, kq = lane >> 4;
  const double* slot = P + (r.slot + blockIdx.y) * SFS_TILE + wv * 1024 + lane;
  const int64_t seg = (int64_t)ntpu * SFS_TILE;
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const double* p = slot + ((a * 2 + b) * 4 + reg) * 64;
        double s = p[0];
        for (int k = 1; k < r.nseg; k++) s = s + p[k * seg];
        const int64_t row = 64 * tR + 32 * wi + 16 * a + kq + 4 * reg, col = 64 * tC + 32 * wj + 16 * b + r16;
        if (row >= W || (tR == tC && row > col)) continue;  // a diagonal tile writes its lower cells as mirrors
        if (col == W) {
          if (sfs) sfs[r.b * W + row] = s;
        } else if (col < W && jsfs) {
          double* J = jsfs + r.b * W * W;
          J[row + col * W] = s;
          if (row != col) J[col + row * W] = s;
        }
      }
}

int sfs_check_row(int64_t x, int64_t v, int64_t n) {
  TPG_REQUIRE(v >= 1 && v < 2147483648ll && x >= 0 && x <= v && n >= 1 && n <= v, TPG_EINVAL,
              "(x, v, n) = (%lld, %lld, %lld): 0 <= x <= v, 1 <= n <= v, v < 2^31", (long long)x, (long long)v, (long long)n);
  return TPG_OK;
}

}  // namespace

extern "C" int64_t tpg_sfs_chunk_loci(void) { return SFS_C; }

extern "C" int64_t tpg_sfs_segments(int64_t block_len, int64_t W) {
  if (block_len < 0 || W < 2 || W > TPG_SFS_MAX_WIDTH) return -1;
  return sfs_segments(block_len, W);
}

extern "C" int64_t tpg_sfs_scratch_bytes(int64_t m, int ngroups, int64_t W, int64_t nb, int want_joint) {
  if (m < 0 || ngroups < 1 || W < 2 * (int64_t)ngroups || W > TPG_SFS_MAX_WIDTH || nb < 0 || nb > TPG_SFS_MAX_BLOCKS) return -1;
  return (int64_t)sfs_plan(m, ngroups, W, nb, want_joint != 0).bytes();
}

extern "C" int tpg_sfs_project_row(int64_t x, int64_t v, int64_t n, double* h) {
  TPG_REQUIRE(h, TPG_EINVAL, "null argument");
  TPG_TRY(sfs_check_row(x, v, n));
  host_sfs_row(x, v, n, HostSfsArray{h});
  return TPG_OK;
}

extern "C" int tpg_sfs_blocks(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups, const double* ploidy,
                              const int32_t* proj, const uint8_t* keep, const uint8_t* flip, const int64_t* lo, const int64_t* hi,
                              int64_t nb, double* sfs, int64_t* n_used1, double* jsfs, int64_t* n_used2) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v, TPG_EINVAL, "null argument");
  TPG_REQUIRE(nb >= 0 && nb <= TPG_SFS_MAX_BLOCKS, TPG_EINVAL, "nb = %lld out of [0, %lld]", (long long)nb, (long long)TPG_SFS_MAX_BLOCKS);
  TPG_REQUIRE(nb == 0 || (lo && hi), TPG_EINVAL, "null argument");
  TPG_REQUIRE(ngroups >= 1 && ngroups <= TPG_SFS_MAX_WIDTH / 2, TPG_EINVAL, "ngroups = %d out of [1, %d]", ngroups, TPG_SFS_MAX_WIDTH / 2);
  TPG_TRY(tpg_require_diploid(v->n, ploidy, "The site frequency spectrum"));
  const int G = ngroups;
  const int64_t m = v->m;
  ClassPlan cp;
  TPG_TRY(make_class_plan(v->n, groupIds0, G, nullptr, &cp));
  std::vector<int32_t> groups((size_t)2 * G);  // o_g, then n_g
  int64_t W = 0;
  for (int g = 0; g < G; g++) {
    const int64_t full = 2 * (int64_t)cp.group_size[(size_t)g];
    TPG_REQUIRE(full > 0, TPG_EINVAL, "group %d has no individual", g);
    const int64_t p = proj ? proj[g] : 0;
    TPG_REQUIRE(p >= 0 && p <= full, TPG_EINVAL, "proj[%d] = %lld out of [0, %lld]", g, (long long)p, (long long)full);
    const int64_t n = p ? p : full;
    TPG_REQUIRE(W + n + 1 <= TPG_SFS_MAX_WIDTH, TPG_EINVAL, "the spectra are more than %d entries wide", TPG_SFS_MAX_WIDTH);
    groups[(size_t)g] = (int32_t)W;
    groups[(size_t)G + g] = (int32_t)n;
    W += n + 1;
  }
  if (nb == 0) return TPG_OK;
  TPG_TRY(tpg_check_ranges(ctx, lo, hi, nb, m, "block"));
  HostIn<int64_t> hlo, hhi;
  TPG_TRY(hlo.init(ctx, lo, nb));
  TPG_TRY(hhi.init(ctx, hi, nb));
  GroupedCounts gc;
  TPG_TRY(tpg_grouped_counts(ctx, v, cp.cls.data(), cp.nclass, &gc));
  InBuf ik, ifl;
  if (keep) TPG_TRY(ik.init(ctx, keep, (size_t)m));
  if (flip) TPG_TRY(ifl.init(ctx, flip, (size_t)m));
  const uint8_t* d_keep = keep ? ik.dev<uint8_t>() : nullptr;
  const uint8_t* d_flip = flip ? ifl.dev<uint8_t>() : nullptr;
  OutBuf os, on1, oj, on2;
  if (sfs) TPG_TRY(os.init(sfs, sizeof(double) * (size_t)W * (size_t)nb));
  if (n_used1) TPG_TRY(on1.init(n_used1, sizeof(int64_t) * (size_t)G * (size_t)nb));
  if (jsfs) TPG_TRY(oj.init(jsfs, sizeof(double) * (size_t)W * (size_t)W * (size_t)nb));
  if (n_used2) TPG_TRY(on2.init(n_used2, sizeof(int64_t) * (size_t)G * (size_t)G * (size_t)nb));

  const bool joint = jsfs != nullptr;
  const SfsPlan pl = sfs_plan(m, G, W, nb, joint);
  DevArena sc;
  size_t taken = 0;
  int32_t* d_groups = nullptr;
  TPG_TRY(sc.get(&d_groups, (size_t)2 * G));
  taken += pl.b_groups;
  TPG_HIP(tpg_h2d_async(ctx, d_groups, groups.data(), pl.b_groups));

  if (n_used1 || n_used2) {
    InBuf il, ih;
    TPG_TRY(il.init(ctx, lo, sizeof(int64_t) * (size_t)nb));
    TPG_TRY(ih.init(ctx, hi, sizeof(int64_t) * (size_t)nb));
    int64_t maxL = 0;
    for (int64_t b = 0; b < nb; b++) maxL = std::max(maxL, hhi[b] - hlo[b]);
    if (n_used1) TPG_HIP(hipMemsetAsync(on1.d, 0, on1.bytes, ctx->stream));
    if (n_used2) TPG_HIP(hipMemsetAsync(on2.d, 0, on2.bytes, ctx->stream));
    const int ntg = (G + 15) / 16, full = n_used2 ? 1 : 0;
    const unsigned nz = (unsigned)std::min<int64_t>(64, std::max<int64_t>(1, ceil_div(maxL, 64 * 64)));
    TPG_LAUNCH(ctx, "sfs_nused", sfs_nused_kernel, dim3((unsigned)nb, (unsigned)(full ? ntg * ntg : ntg), nz), dim3(256), 0,
               (const int32_t*)(gc.cnt + 2 * gc.Mpad * gc.Cpad), gc.Cpad, G, (const int32_t*)(d_groups + G), d_keep, il.dev<int64_t>(),
               ih.dev<int64_t>(), full, (unsigned long long*)on1.d, (unsigned long long*)on2.d);
    TPG_CHECK_LAUNCH();
    TPG_HIP(hipStreamSynchronize(ctx->stream));  // il, ih go back to the pool here
  }

  if (sfs || jsfs) {
    double *d_F = nullptr, *d_P = nullptr;
    SfsPiece* d_pieces = nullptr;
    SfsChunk* d_chunks = nullptr;
    SfsRed* d_red = nullptr;
    TPG_TRY(sc.get(&d_F, (size_t)pl.rows * (size_t)pl.Wp));
    TPG_TRY(sc.get(&d_P, (size_t)pl.PT * (size_t)SFS_TILE));
    TPG_TRY(sc.get(&d_pieces, (size_t)pl.PT));
    TPG_TRY(sc.get(&d_chunks, (size_t)(pl.rows / SFS_C)));
    TPG_TRY(sc.get(&d_red, (size_t)pl.PT));
    taken += pl.b_frag + pl.b_part + pl.b_pieces + pl.b_chunks + pl.b_red;
    TPG_REQUIRE((int64_t)taken == tpg_sfs_scratch_bytes(m, G, W, nb, joint ? 1 : 0), TPG_EHIP,
                "the scratch of the call (%zu bytes) is not what tpg_sfs_scratch_bytes reports", taken);
    // the padding columns are never written: zero once
    TPG_HIP(hipMemsetAsync(d_F, 0, pl.b_frag, ctx->stream));
    const int64_t SM = pl.rows / 4, stage_chunks = pl.rows / SFS_C;
    struct Unit { int64_t j, jend, slot; bool started; };
    std::vector<Unit> units;
    std::vector<SfsRed> red;
    std::vector<SfsPiece> pieces;
    std::vector<SfsChunk> chunks;
    int64_t bi = 0;
    while (bi < nb) {
      // a batch: consecutive blocks while their partial tiles fit
      units.clear();
      red.clear();
      int64_t tiles = 0;
      while (bi < nb) {
        const int64_t L = hhi[bi] - hlo[bi], ns = sfs_segments(L, W), need = ns * pl.ntpu;
        if (!units.empty() && tiles + need > pl.PT) break;
        const int64_t SL = std::max<int64_t>(1, ceil_div(ceil_div(L, ns), SFS_C)) * SFS_C;
        red.push_back(SfsRed{tiles, bi, (int32_t)ns, 0});
        for (int64_t s = 0; s < ns; s++) {
          const int64_t ulo = std::min(hlo[bi] + s * SL, hhi[bi]), uhi = std::min(ulo + SL, hhi[bi]);
          units.push_back(Unit{ulo, uhi, tiles + s * pl.ntpu, false});
        }
        tiles += need;
        bi++;
      }
      // rounds: the staged rows go to the unfinished segments in equal shares of whole chunks
      size_t first = 0;
      for (;;) {
        while (first < units.size() && units[first].started && units[first].j >= units[first].jend) first++;
        int64_t nact = 0;
        for (size_t u = first; u < units.size() && nact < stage_chunks; u++) nact += !units[u].started || units[u].j < units[u].jend;
        if (nact == 0) break;
        const int64_t quota = std::max<int64_t>(1, stage_chunks / nact);
        pieces.clear();
        chunks.clear();
        int64_t done = 0;
        for (size_t u = first; u < units.size() && done < nact; u++) {
          Unit& un = units[u];
          if (un.started && un.j >= un.jend) continue;
          const int64_t take = std::min(quota, ceil_div(un.jend - un.j, SFS_C)), nl = std::min(un.jend - un.j, take * SFS_C);
          pieces.push_back(SfsPiece{un.slot, (int32_t)(chunks.size() * SFS_C), (int32_t)nl, un.started ? 0 : 1, 0});
          for (int64_t c = 0; c < take; c++)
            chunks.push_back(SfsChunk{un.j + c * SFS_C, (int32_t)std::min<int64_t>(SFS_C, nl - c * SFS_C), 0});
          un.j += nl;
          un.started = true;
          done++;
        }
        TPG_HIP(tpg_h2d_async(ctx, d_pieces, pieces.data(), sizeof(SfsPiece) * pieces.size()));
        if (!chunks.empty()) {
          TPG_HIP(tpg_h2d_async(ctx, d_chunks, chunks.data(), sizeof(SfsChunk) * chunks.size()));
          TPG_LAUNCH(ctx, "sfs_operands", sfs_operands_kernel, dim3((unsigned)chunks.size(), (unsigned)ceil_div(G, 4)), dim3(256), 0,
                     (const int32_t*)gc.cnt, gc.Mpad, gc.Cpad, G, (const int32_t*)d_groups, (const int32_t*)(d_groups + G), (int)W,
                     d_keep, d_flip, (const SfsChunk*)d_chunks, d_F, SM);
        }
        TPG_LAUNCH(ctx, "sfs_gram", sfs_gram_kernel, dim3((unsigned)pieces.size(), (unsigned)pl.ntpu), dim3(256), 0, (const double*)d_F,
                   SM, (const SfsPiece*)d_pieces, pl.nt, joint ? 1 : 0, d_P);
      }
      TPG_HIP(tpg_h2d_async(ctx, d_red, red.data(), sizeof(SfsRed) * red.size()));
      TPG_LAUNCH(ctx, "sfs_reduce", sfs_reduce_kernel, dim3((unsigned)red.size(), (unsigned)pl.ntpu), dim3(256), 0, (const double*)d_P,
                 (const SfsRed*)d_red, pl.nt, joint ? 1 : 0, pl.ntpu, W, os.dev<double>(), oj.dev<double>());
    }
    TPG_CHECK_LAUNCH();
  }
  TPG_HIP(hipStreamSynchronize(ctx->stream));  // the scratch of this call goes back to the pool at scope exit
  if (sfs) TPG_TRY(os.commit(ctx));
  if (n_used1) TPG_TRY(on1.commit(ctx));
  if (jsfs) TPG_TRY(oj.commit(ctx));
  if (n_used2) TPG_TRY(on2.commit(ctx));
  return TPG_OK;
}
