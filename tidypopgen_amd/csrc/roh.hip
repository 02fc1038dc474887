// roh.hip -- runs of homozygosity per individual (windows_indiv_roh) on the device.  The definition is in include/tpg.h
// ("Runs of homozygosity"); DESIGN.md 3.7 has the mapping and what bounds the kernels.
//
//  * tpg_roh_status_kernel: a workgroup owns the 32 individuals of one row tile of T and a chunk of TPG_ROH_CHUNK_LOCI loci
//    with a halo of HB = ceil((W - 1) / 128) blocks on either side.  Every 1-KiB block is read whole, 16 B per lane; the
//    two-bit codes of a dword are turned into locus-ordered `opp` and `miss` masks by a fixed bit shuffle (locusbits.h: even
//    bits together, then a 4 x 4 bit transpose) and lanes r and r + 32 exchange halves, so that LDS holds 32 loci per word.
//    Word-level prefix popcounts give the sums of the first window of a word, the other 31 follow by sliding (one bit in,
//    one bit out): nothing loops over W.  The same once more over the window-ok bits gives `hits` per locus.  What does
//    not depend on the individual -- which windows exist and cross no break -- comes up once as a bit vector.
//  * tpg_roh_segments_kernel: one workgroup per individual walks its in-run bits, finds segment starts and ends word-parallel,
//    counts them (first launch) and writes them in order (second launch, after a scan over the individuals).  The k-th start
//    of a row belongs to its k-th end, so a segment comes out whole wherever the status stage cut its chunks.
//  * tpg_roh_filter_kernel counts nOpp / nMiss of a segment from T and applies the run filters; a scan over the flags
//    compacts the runs.  Only the two counts (segments, runs) cross to the host.
#include "common.h"
#include "locusbits.h"
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstring>

#define ROH_CB 16                      // blocks of 128 loci per chunk
#define ROH_CHUNK (128 * ROH_CB)       // = TPG_ROH_CHUNK_LOCI
#define ROH_MAX_W 512
static_assert(ROH_CHUNK == TPG_ROH_CHUNK_LOCI, "include/tpg.h states the chunk length");

struct tpg_roh {
  tpg_ctx* ctx = nullptr;
  int64_t n = 0, m = 0, count = 0;
  DevBuf indiv, first, last, nopp, nmiss;  // int32, int64, int64, int32, int32: `count` entries each
  DevBuf pos;                              // int64[m]
};

// bits [sh, sh + 32) of hi:lo
__device__ __forceinline__ uint32_t roh_funnel(uint32_t lo, uint32_t hi, int sh) {
  return sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
}

// exclusive word-level prefix popcounts of row `r` (NWp words): PARTS neighbouring lanes take a piece of the row each, add up
// their piece, learn what lies before it from the lanes below and write their piece's prefixes
template <int PARTS>
__device__ __forceinline__ void roh_word_prefix(const uint32_t* arr, uint16_t* pre, int r, int part, int NWp) {
  const int per = (NWp + PARTS - 1) / PARTS, w0 = part * per, w1 = w0 + per < NWp ? w0 + per : NWp;
  const uint32_t* a = arr + r * NWp;
  uint16_t* p = pre + r * NWp;
  int sum = 0;
  for (int w = w0; w < w1; w++) sum += __popc(a[w]);
  int inc = sum;
#pragma unroll
  for (int o = 1; o < PARTS; o <<= 1) {
    const int u = __shfl_up(inc, o, PARTS);
    if (part >= o) inc += u;
  }
  int run = inc - sum;
  for (int w = w0; w < w1; w++) {
    p[w] = (uint16_t)run;
    run += __popc(a[w]);
  }
}

// LDS rows: NWp = NW + 3 words per individual (odd: the 32 rows of a column fall into 32 banks), the last three zero
__global__ __launch_bounds__(256) void tpg_roh_status_kernel(const uint4* __restrict__ T, int64_t KG, int64_t n, int64_t m, int W,
                                                             int HB, int het, int maxopp, int maxmiss,
                                                             const uint32_t* __restrict__ wok, const int32_t* __restrict__ need,
                                                             uint32_t* __restrict__ bits, int64_t stride, int nchunks) {
  extern __shared__ uint32_t roh_smem[];
  const int NW = (ROH_CB + 2 * HB) * 4, NWp = NW + 3;
  uint32_t* sopp = roh_smem;
  uint32_t* smiss = sopp + 32 * NWp;
  uint32_t* sok = smiss + 32 * NWp;
  uint16_t* pO = (uint16_t*)(sok + 32 * NWp);
  uint16_t* pM = pO + 32 * NWp;
  uint16_t* pQ = pM + 32 * NWp;
  int32_t* sneed = (int32_t*)(pQ + 32 * NWp);  // W + 1 entries
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int chunk = (int)(blockIdx.x % (unsigned)nchunks);
  const int64_t rt = blockIdx.x / (unsigned)nchunks;
  const int64_t kb0 = (int64_t)chunk * ROH_CB, sb = kb0 - HB;  // first block of the chunk, first block in LDS (may be < 0)
  for (int i = tid; i < 3 * 32 * NWp; i += 256) roh_smem[i] = 0;
  for (int i = tid; i <= W; i += 256) sneed[i] = need[i];
  __syncthreads();
  // ---- blocks -> locus-ordered masks in LDS
  {
    const int r = lane & 31, h = lane >> 5;
    for (int b = wv; b < ROH_CB + 2 * HB; b += 4) {
      const int64_t kg = sb + b;
      if (kg < 0 || kg >= KG) continue;  // (the whole wave alike)
      const uint4 f = T[(rt * KG + kg) * 64 + lane];
      uint32_t o01, m01, o23, m23;
      tpg_lb_opp_miss(f.x, f.y, het, o01, m01);
      tpg_lb_opp_miss(f.z, f.w, het, o23, m23);
      const uint32_t po01 = (uint32_t)__shfl_xor((int)o01, 32), pm01 = (uint32_t)__shfl_xor((int)m01, 32);
      const uint32_t po23 = (uint32_t)__shfl_xor((int)o23, 32), pm23 = (uint32_t)__shfl_xor((int)m23, 32);
      // word s = loci 32 s .. 32 s + 31 of the block: low half from lane r, high half from lane r + 32
      // (the exchange of locusbits.h's tpg_lb_words, written out: through that function the kernel compiles to other
      // instructions, and this kernel's code stays as it was measured)
      uint32_t* ro = sopp + r * NWp + 4 * b;
      uint32_t* rm = smiss + r * NWp + 4 * b;
      if (h == 0) {
        ro[0] = (o01 & 0xffffu) | (po01 << 16);
        ro[1] = (o01 >> 16) | (po01 & 0xffff0000u);
        rm[0] = (m01 & 0xffffu) | (pm01 << 16);
        rm[1] = (m01 >> 16) | (pm01 & 0xffff0000u);
      } else {
        ro[2] = (po23 & 0xffffu) | (o23 << 16);
        ro[3] = (po23 >> 16) | (o23 & 0xffff0000u);
        rm[2] = (pm23 & 0xffffu) | (m23 << 16);
        rm[3] = (pm23 >> 16) | (m23 & 0xffff0000u);
      }
    }
  }
  __syncthreads();
  // ---- word-level prefix popcounts of opp and miss: four lanes per (row, mask), a quarter of the row each
  roh_word_prefix<4>(tid < 128 ? sopp : smiss, tid < 128 ? pO : pM, (tid & 127) >> 2, tid & 3, NWp);
  __syncthreads();
  auto cnt = [](const uint32_t* a, const uint16_t* p, int l) {  // set bits below local locus l
    const int w = l >> 5, b = l & 31;
    return (int)p[w] + __popc(a[w] & ((1u << b) - 1u));
  };
  // ---- window-ok bits for the windows that start in [chunk start - (W - 1), chunk end)
  const int wi_lo = (HB * 128 - (W - 1)) >> 5, wi_hi = (HB + ROH_CB) * 4;
  for (int t = tid; t < 32 * (wi_hi - wi_lo); t += 256) {
    const int r = t / (wi_hi - wi_lo), wi = wi_lo + t % (wi_hi - wi_lo);
    const int64_t j0 = sb * 128 + (int64_t)wi * 32;
    uint32_t okw = 0;
    const uint32_t valid = j0 >= 0 && j0 < KG * 128 ? wok[j0 >> 5] : 0u;
    if (valid) {
      const uint32_t *ao = sopp + r * NWp, *am = smiss + r * NWp;
      const uint16_t *po = pO + r * NWp, *pm = pM + r * NWp;
      const int lin = wi * 32 + W, hw = lin >> 5, sh = lin & 31;
      const uint32_t outo = ao[wi], outm = am[wi];
      const uint32_t ino = roh_funnel(ao[hw], ao[hw + 1], sh), inm = roh_funnel(am[hw], am[hw + 1], sh);
      int so = cnt(ao, po, lin) - (int)po[wi], sm = cnt(am, pm, lin) - (int)pm[wi];
#pragma unroll
      for (int b = 0; b < 32; b++) {
        okw |= (uint32_t)((so <= maxopp) & (sm <= maxmiss)) << b;
        so += (int)((ino >> b) & 1u) - (int)((outo >> b) & 1u);
        sm += (int)((inm >> b) & 1u) - (int)((outm >> b) & 1u);
      }
      okw &= valid;
    }
    sok[r * NWp + wi] = okw;
  }
  __syncthreads();
  roh_word_prefix<8>(sok, pQ, tid >> 3, tid & 7, NWp);
  __syncthreads();
  // ---- hits per locus against need[cover]
  const int64_t nwords = (m + 31) >> 5;
  const int64_t mW = m - W;  // the last window
  const int needW = sneed[W];
  for (int t = tid; t < 32 * ROH_CB * 4; t += 256) {
    const int r = t / (ROH_CB * 4), wo = t % (ROH_CB * 4);
    const int64_t ind = rt * 32 + r, gw = kb0 * 4 + wo, j0 = gw * 32;
    if (ind >= n || gw >= nwords) continue;
    const int wi = HB * 4 + wo, l0 = wi * 32;
    const uint32_t* aq = sok + r * NWp;
    const uint16_t* pq = pQ + r * NWp;
    const int lout = l0 - W + 1, ow = lout >> 5;
    const uint32_t inq = roh_funnel(aq[wi], aq[wi + 1], 1), outq = roh_funnel(aq[ow], aq[ow + 1], lout & 31);
    int hits = cnt(aq, pq, l0 + 1) - cnt(aq, pq, lout);
    uint32_t res = 0;
    if (j0 >= W - 1 && j0 + 31 <= mW) {  // every locus of the word lies in W windows
#pragma unroll
      for (int b = 0; b < 32; b++) {
        res |= (uint32_t)(hits >= needW) << b;
        hits += (int)((inq >> b) & 1u) - (int)((outq >> b) & 1u);
      }
    } else {
      for (int b = 0; b < 32; b++) {
        const int64_t j = j0 + b;
        if (j < m) {
          const int64_t hi = j < mW ? j : mW, lo = j - W + 1 > 0 ? j - W + 1 : 0;
          res |= (uint32_t)(hits >= sneed[(int)(hi - lo + 1)]) << b;
        }
        hits += (int)((inq >> b) & 1u) - (int)((outq >> b) & 1u);
      }
    }
    bits[ind * stride + gw] = res;
  }
}

// ---- segments -------------------------------------------------------------------------------------------------------
// brk: bit j = a break between loci j and j + 1; bit m - 1 is set (the last locus ends a segment).  One workgroup per
// individual.  EMIT = false: rowcnt[i] = segments of the row.  EMIT = true: the row's segments from rowoff[i] on.
template <bool EMIT>
__global__ __launch_bounds__(256) void tpg_roh_segments_kernel(const uint32_t* __restrict__ bits, int64_t stride, int64_t nwords,
                                                               const uint32_t* __restrict__ brk, int64_t* __restrict__ rowcnt,
                                                               const int64_t* __restrict__ rowoff, int32_t* __restrict__ indiv,
                                                               int64_t* __restrict__ first, int64_t* __restrict__ last) {
  __shared__ uint32_t wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t i = blockIdx.x;
  const uint32_t* row = bits + i * stride;
  int64_t runS = 0, runE = 0;
  const int64_t off0 = EMIT ? rowoff[i] : 0;
  for (int64_t tb = 0; tb < nwords; tb += 256) {
    const int64_t w = tb + tid;
    uint32_t st = 0, en = 0;
    if (w < nwords) {
      const uint32_t cur = row[w], pw = w > 0 ? row[w - 1] : 0u, nx = w + 1 < nwords ? row[w + 1] : 0u;
      const uint32_t bw = brk[w], bp = w > 0 ? brk[w - 1] : 0u;
      const uint32_t prevbits = (cur << 1) | (pw >> 31), brkprev = (bw << 1) | (bp >> 31);
      const uint32_t nextbits = (cur >> 1) | (nx << 31);
      st = cur & (~prevbits | brkprev);
      en = cur & (~nextbits | bw);
    }
    // exclusive scan of (starts | ends << 16) over the workgroup: at most 8192 of either per tile
    const uint32_t v = (uint32_t)__popc(st) | ((uint32_t)__popc(en) << 16);
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = (uint32_t)__shfl_up((int)inc, o);
      if (lane >= o) inc += u;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t s = wsum[k];
      if (k < wv) before += s;
      total += s;
    }
    __syncthreads();
    if (EMIT) {
      const uint32_t ex = before + inc - v;
      int64_t ks = off0 + runS + (ex & 0xffffu), ke = off0 + runE + (ex >> 16);
      while (st) {
        const int b = __ffs((int)st) - 1;
        st &= st - 1;
        first[ks] = w * 32 + b;
        indiv[ks] = (int32_t)i;
        ks++;
      }
      while (en) {
        const int b = __ffs((int)en) - 1;
        en &= en - 1;
        last[ke++] = w * 32 + b;
      }
    }
    runS += total & 0xffffu;
    runE += total >> 16;
  }
  if (!EMIT && tid == 0) rowcnt[i] = runS;
}

// nOpp / nMiss of every segment from T, and the run filters.  One thread per segment.
__global__ __launch_bounds__(256) void tpg_roh_filter_kernel(const uint32_t* __restrict__ T32, int64_t KG, int het,
                                                             const int64_t* __restrict__ pos, const int32_t* __restrict__ indiv,
                                                             const int64_t* __restrict__ first, const int64_t* __restrict__ last,
                                                             int64_t nseg, int min_snp, int64_t min_len, double min_density,
                                                             int max_opp_run, int max_miss_run, int32_t* __restrict__ nopp,
                                                             int32_t* __restrict__ nmiss, int32_t* __restrict__ keep) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nseg) return;
  const int64_t a = first[k], b = last[k];
  const int64_t ind = indiv[k], rt = ind >> 5;
  const int r = (int)(ind & 31);
  int co = 0, cm = 0;
  for (int64_t g = a >> 4; g <= b >> 4; g++) {  // 16 loci = one dword of one lane
    const int64_t lg = g * 16, kg = lg >> 7;
    const int off = (int)(lg & 127), s = off >> 5, h = (off >> 4) & 1;
    const uint32_t w = T32[(((rt * KG + kg) * 64) + r + 32 * h) * 4 + s];
    uint32_t o, ms;
    tpg_lb_opp_miss(w, 0u, het, o, ms);
    const int lo = a > lg ? (int)(a - lg) : 0, hi = b < lg + 15 ? (int)(b - lg) : 15;
    const uint32_t mask = ((2u << hi) - 1u) & ~((1u << lo) - 1u) & 0xffffu;
    co += __popc(o & mask);
    cm += __popc(ms & mask);
  }
  nopp[k] = co;
  nmiss[k] = cm;
  const int64_t nsnp = b - a + 1, len = pos[b] - pos[a];
  const double lhs = (double)nsnp * 1000.0, rhs = min_density * (double)len;
  const bool run = nsnp >= min_snp && len >= min_len && lhs >= rhs && (max_opp_run < 0 || co <= max_opp_run) &&
                   (max_miss_run < 0 || cm <= max_miss_run);
  keep[k] = run ? 1 : 0;
}

__global__ __launch_bounds__(256) void tpg_roh_compact_kernel(const int32_t* __restrict__ keep, const int32_t* __restrict__ dst,
                                                              int64_t nseg, const int32_t* __restrict__ indiv,
                                                              const int64_t* __restrict__ first, const int64_t* __restrict__ last,
                                                              const int32_t* __restrict__ nopp, const int32_t* __restrict__ nmiss,
                                                              int32_t* __restrict__ o_indiv, int64_t* __restrict__ o_first,
                                                              int64_t* __restrict__ o_last, int32_t* __restrict__ o_nopp,
                                                              int32_t* __restrict__ o_nmiss) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nseg || !keep[k]) return;
  const int32_t d = dst[k];
  o_indiv[d] = indiv[k];
  o_first[d] = first[k];
  o_last[d] = last[k];
  o_nopp[d] = nopp[k];
  o_nmiss[d] = nmiss[k];
}

// per individual: number of runs and sum of pos[last] - pos[first] (integer atomics: the order does not matter)
__global__ __launch_bounds__(256) void tpg_roh_summary_kernel(const int32_t* __restrict__ indiv, const int64_t* __restrict__ first,
                                                              const int64_t* __restrict__ last, const int64_t* __restrict__ pos,
                                                              int64_t count, unsigned long long* __restrict__ n_runs,
                                                              unsigned long long* __restrict__ sum_len) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = k < count;
  const int32_t ind = live ? indiv[k] : -1;
  unsigned long long len = live ? (unsigned long long)(pos[last[k]] - pos[first[k]]) : 0ull;
  // the runs are ordered by individual: a wave whose runs all belong to one adds up first and issues one atomic each
  const int32_t ind0 = __shfl(ind, 0);
  if (ind0 >= 0 && __all(ind == ind0)) {  // (every lane holds a run then)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) len += (unsigned long long)__shfl_xor((long long)len, o);
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&n_runs[ind0], 64ull);
      atomicAdd(&sum_len[ind0], len);
    }
  } else if (live) {
    atomicAdd(&n_runs[ind], 1ull);
    atomicAdd(&sum_len[ind], len);
  }
}

// difference array of the runs: +1 at the first locus, -1 behind the last (diff has m + 1 entries)
__global__ __launch_bounds__(256) void tpg_roh_diff_kernel(const int64_t* __restrict__ first, const int64_t* __restrict__ last,
                                                           int64_t count, int32_t* __restrict__ diff) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= count) return;
  atomicAdd(&diff[first[k]], 1);
  atomicAdd(&diff[last[k] + 1], -1);
}

// ---- host side ------------------------------------------------------------------------------------------------------
namespace {

struct RohPlan {
  int W = 0, HB = 0;
  int64_t nwords = 0;          // ceil(m / 32)
  std::vector<uint32_t> brk;   // KG * 4 + 1 words
  std::vector<uint32_t> wok;   // window w exists and crosses no break
  std::vector<int32_t> need;   // W + 1
  HostIn<int64_t> pos;
};

int roh_plan(tpg_ctx* ctx, const tpg_view* v, const int32_t* chrom, const int64_t* pos, const tpg_roh_params* P, RohPlan* pl) {
  TPG_REQUIRE(ctx && v && chrom && pos && P, TPG_EINVAL, "null argument");
  TPG_REQUIRE(v->m >= 1 && v->n >= 1, TPG_EINVAL, "empty view");
  TPG_REQUIRE(P->window_size >= 1 && P->window_size <= ROH_MAX_W, TPG_EINVAL, "window_size = %d outside [1, %d]",
              (int)P->window_size, ROH_MAX_W);
  TPG_REQUIRE(P->threshold >= 0.0 && P->threshold <= 1.0, TPG_EINVAL, "threshold must lie in [0, 1]");  // (a NaN fails both)
  TPG_REQUIRE(P->max_opp_window >= 0 && P->max_miss_window >= 0, TPG_EINVAL, "max_opp_window / max_miss_window below 0");
  TPG_REQUIRE(P->min_density == P->min_density, TPG_EINVAL, "min_density is NaN");
  const int64_t m = v->m;
  TPG_REQUIRE(m < (1ll << 31) - 64, TPG_EUNSUPPORTED, "runs of homozygosity over 2^31 loci or more");
  const int W = P->window_size;
  pl->W = W;
  pl->HB = (W - 1 + 127) / 128;
  pl->nwords = ceil_div(m, 32);
  HostIn<int32_t> ch;
  TPG_TRY(ch.init(ctx, chrom, m));
  TPG_TRY(pl->pos.init(ctx, pos, m));
  const size_t words = (size_t)v->KG * 4 + 1;
  pl->brk.assign(words, 0u);
  pl->wok.assign(words, 0u);
  // nb = the first break at or behind w (the last locus counts as one); window w is fine iff nb > w + W - 2
  int64_t nb = m - 1;
  pl->brk[(size_t)((m - 1) >> 5)] |= 1u << ((m - 1) & 31);
  for (int64_t j = m - 1; j >= 0; j--) {
    if (j < m - 1) {
      const bool same = ch[(size_t)j] == ch[(size_t)j + 1];
      const int64_t d = pl->pos[(size_t)j + 1] - pl->pos[(size_t)j];
      TPG_REQUIRE(!same || d >= 0, TPG_EINVAL, "loci are not ordered: position decreases at locus %lld", (long long)j + 1);
      if (!same || d > P->max_gap) {
        nb = j;
        pl->brk[(size_t)(j >> 5)] |= 1u << (j & 31);
      }
    }
    if (j + W <= m && (W == 1 || nb > j + W - 2)) pl->wok[(size_t)(j >> 5)] |= 1u << (j & 31);
  }
  pl->need.assign((size_t)W + 1, 1);
  for (int c = 1; c <= W; c++) {
    const double x = P->threshold * (double)c;
    const int k = (int)std::ceil(x);
    pl->need[(size_t)c] = k > 1 ? k : 1;
  }
  return TPG_OK;
}

// in-run bits of every (individual, locus) into d_bits (n rows of `stride` words, zero where nothing is written)
int roh_status(tpg_ctx* ctx, const tpg_view* v, const tpg_roh_params* P, const RohPlan& pl, const uint32_t* d_wok, DevArena& sc,
               uint32_t* d_bits, int64_t stride) {
  const int64_t n = v->n, m = v->m;
  TPG_HIP(hipMemsetAsync(d_bits, 0, sizeof(uint32_t) * (size_t)n * (size_t)stride, ctx->stream));
  if (m < pl.W) return TPG_OK;  // no window, no run
  TPG_TRY(tpg_view_need_T(ctx, v));
  int32_t* d_need = nullptr;
  TPG_TRY(sc.get(&d_need, pl.need.size()));
  TPG_HIP(tpg_upload(ctx, d_need, pl.need.data(), sizeof(int32_t) * pl.need.size()));
  const int64_t nchunks = ceil_div(v->KG, ROH_CB), nrt = ceil_div(n, 32);
  TPG_REQUIRE(nchunks * nrt < (1ll << 31), TPG_EUNSUPPORTED, "runs of homozygosity: too many chunks for one launch");
  const int NWp = (ROH_CB + 2 * pl.HB) * 4 + 3;
  const size_t lds = (size_t)32 * NWp * (3 * 4 + 3 * 2) + sizeof(int32_t) * (size_t)(pl.W + 1);
  TPG_LAUNCH(ctx, "roh_status", tpg_roh_status_kernel, dim3((unsigned)(nchunks * nrt)), dim3(256), lds, (const uint4*)v->T, v->KG, n,
             m, pl.W, pl.HB, P->heterozygosity ? 1 : 0, (int)P->max_opp_window, (int)P->max_miss_window, d_wok,
             (const int32_t*)d_need, d_bits, stride, (int)nchunks);
  TPG_CHECK_LAUNCH();
  return TPG_OK;
}

int roh_upload_words(tpg_ctx* ctx, DevArena& sc, const std::vector<uint32_t>& h, uint32_t** d) {
  TPG_TRY(sc.get(d, h.size()));
  TPG_HIP(tpg_upload(ctx, *d, h.data(), sizeof(uint32_t) * h.size()));
  return TPG_OK;
}

int roh_out(tpg_ctx* ctx, void* user, const void* d_src, size_t bytes) {
  if (!user || bytes == 0) return TPG_OK;
  if (tpg_is_device_ptr(user)) {
    TPG_HIP(tpg_copy_dev(ctx, user, d_src, bytes));
    TPG_HIP(hipStreamSynchronize(ctx->stream));
  } else {
    TPG_HIP(tpg_download(ctx, user, d_src, bytes));
  }
  return TPG_OK;
}

}  // namespace

extern "C" int64_t tpg_roh_chunk_loci(void) { return ROH_CHUNK; }

extern "C" int tpg_roh_snp_status(tpg_ctx* ctx, const tpg_view* v, const int32_t* chrom, const int64_t* pos,
                                  const tpg_roh_params* params, uint32_t* bits, int64_t stride_words) {
  TpgEnter _enter(ctx);
  RohPlan pl;
  TPG_TRY(roh_plan(ctx, v, chrom, pos, params, &pl));
  TPG_REQUIRE(bits, TPG_EINVAL, "null argument");
  TPG_REQUIRE(stride_words >= pl.nwords, TPG_EINVAL, "stride_words = %lld, %lld loci need %lld", (long long)stride_words,
              (long long)v->m, (long long)pl.nwords);
  DevArena sc;
  uint32_t* d_wok = nullptr;
  TPG_TRY(roh_upload_words(ctx, sc, pl.wok, &d_wok));
  OutBuf o;
  TPG_TRY(o.init(bits, sizeof(uint32_t) * (size_t)v->n * (size_t)stride_words));
  TPG_TRY(roh_status(ctx, v, params, pl, d_wok, sc, o.dev<uint32_t>(), stride_words));
  TPG_TRY(o.commit(ctx));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return TPG_OK;
}

extern "C" int tpg_roh_detect(tpg_ctx* ctx, const tpg_view* v, const int32_t* chrom, const int64_t* pos,
                              const tpg_roh_params* params, tpg_roh** out) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(out, TPG_EINVAL, "null argument");
  *out = nullptr;
  RohPlan pl;
  TPG_TRY(roh_plan(ctx, v, chrom, pos, params, &pl));
  const int64_t n = v->n, m = v->m, stride = pl.nwords;
  std::unique_ptr<tpg_roh> R(new tpg_roh);
  R->ctx = ctx;
  R->n = n;
  R->m = m;
  TPG_TRY(R->pos.alloc_n<int64_t>((size_t)m));
  TPG_HIP(tpg_upload(ctx, R->pos.p, pl.pos.p, sizeof(int64_t) * (size_t)m));
  if (m < pl.W) {
    *out = R.release();
    return TPG_OK;
  }
  DevArena sc;
  uint32_t *d_wok = nullptr, *d_brk = nullptr, *d_bits = nullptr;
  TPG_TRY(roh_upload_words(ctx, sc, pl.wok, &d_wok));
  TPG_TRY(roh_upload_words(ctx, sc, pl.brk, &d_brk));
  TPG_TRY(sc.get(&d_bits, (size_t)n * (size_t)stride));
  TPG_TRY(roh_status(ctx, v, params, pl, d_wok, sc, d_bits, stride));
  // segments: count per individual, scan, write in order
  int64_t *d_rowcnt = nullptr, *d_rowoff = nullptr;
  TPG_TRY(sc.get(&d_rowcnt, (size_t)n + 1));
  TPG_TRY(sc.get(&d_rowoff, (size_t)n + 1));
  TPG_HIP(hipMemsetAsync(d_rowcnt, 0, sizeof(int64_t) * ((size_t)n + 1), ctx->stream));
  TPG_LAUNCH(ctx, "roh_seg_count", tpg_roh_segments_kernel<false>, dim3((unsigned)n), dim3(256), 0, (const uint32_t*)d_bits, stride,
             pl.nwords, (const uint32_t*)d_brk, d_rowcnt, (const int64_t*)nullptr, (int32_t*)nullptr, (int64_t*)nullptr,
             (int64_t*)nullptr);
  TPG_CHECK_LAUNCH();
  {
    size_t t_scan = 0;
    TPG_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, t_scan, d_rowcnt, d_rowoff, (int)(n + 1), ctx->stream));
    uint8_t* d_tmp = nullptr;
    TPG_TRY(sc.get(&d_tmp, t_scan));
    ProfScope ps(ctx, "roh_row_scan");
    TPG_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, t_scan, d_rowcnt, d_rowoff, (int)(n + 1), ctx->stream));
  }
  int64_t nseg = 0;
  TPG_HIP(tpg_fetch_small(ctx, &nseg, d_rowoff + n, sizeof(nseg)));
  TPG_REQUIRE(nseg < (1ll << 31) - 1, TPG_EUNSUPPORTED, "runs of homozygosity: 2^31 segments or more in one call");
  if (nseg == 0) {
    *out = R.release();
    return TPG_OK;
  }
  int32_t *d_ind = nullptr, *d_no = nullptr, *d_nm = nullptr, *d_keep = nullptr, *d_dst = nullptr;
  int64_t *d_first = nullptr, *d_last = nullptr;
  TPG_TRY(sc.get(&d_ind, (size_t)nseg));
  TPG_TRY(sc.get(&d_first, (size_t)nseg));
  TPG_TRY(sc.get(&d_last, (size_t)nseg));
  TPG_TRY(sc.get(&d_no, (size_t)nseg));
  TPG_TRY(sc.get(&d_nm, (size_t)nseg));
  TPG_TRY(sc.get(&d_keep, (size_t)nseg + 1));
  TPG_TRY(sc.get(&d_dst, (size_t)nseg + 1));
  TPG_LAUNCH(ctx, "roh_seg_emit", tpg_roh_segments_kernel<true>, dim3((unsigned)n), dim3(256), 0, (const uint32_t*)d_bits, stride,
             pl.nwords, (const uint32_t*)d_brk, (int64_t*)nullptr, (const int64_t*)d_rowoff, d_ind, d_first, d_last);
  TPG_CHECK_LAUNCH();
  TPG_HIP(hipMemsetAsync(d_keep + nseg, 0, sizeof(int32_t), ctx->stream));
  const unsigned gseg = (unsigned)ceil_div(nseg, 256);
  TPG_LAUNCH(ctx, "roh_filter", tpg_roh_filter_kernel, dim3(gseg), dim3(256), 0, (const uint32_t*)v->T, v->KG,
             params->heterozygosity ? 1 : 0, (const int64_t*)R->pos.p, (const int32_t*)d_ind, (const int64_t*)d_first,
             (const int64_t*)d_last, nseg, (int)params->min_snp, (int64_t)params->min_length_bps, params->min_density,
             (int)params->max_opp_run, (int)params->max_miss_run, d_no, d_nm, d_keep);
  TPG_CHECK_LAUNCH();
  {
    size_t t_scan = 0;
    TPG_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, t_scan, d_keep, d_dst, (int)(nseg + 1), ctx->stream));
    uint8_t* d_tmp = nullptr;
    TPG_TRY(sc.get(&d_tmp, t_scan));
    ProfScope ps(ctx, "roh_keep_scan");
    TPG_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, t_scan, d_keep, d_dst, (int)(nseg + 1), ctx->stream));
  }
  int32_t nrun = 0;
  TPG_HIP(tpg_fetch_small(ctx, &nrun, d_dst + nseg, sizeof(nrun)));
  R->count = nrun;
  if (nrun > 0) {
    TPG_TRY(R->indiv.alloc_n<int32_t>((size_t)nrun));
    TPG_TRY(R->first.alloc_n<int64_t>((size_t)nrun));
    TPG_TRY(R->last.alloc_n<int64_t>((size_t)nrun));
    TPG_TRY(R->nopp.alloc_n<int32_t>((size_t)nrun));
    TPG_TRY(R->nmiss.alloc_n<int32_t>((size_t)nrun));
    TPG_LAUNCH(ctx, "roh_compact", tpg_roh_compact_kernel, dim3(gseg), dim3(256), 0, (const int32_t*)d_keep, (const int32_t*)d_dst,
               nseg, (const int32_t*)d_ind, (const int64_t*)d_first, (const int64_t*)d_last, (const int32_t*)d_no,
               (const int32_t*)d_nm, R->indiv.as<int32_t>(), R->first.as<int64_t>(), R->last.as<int64_t>(), R->nopp.as<int32_t>(),
               R->nmiss.as<int32_t>());
    TPG_CHECK_LAUNCH();
  }
  TPG_HIP(hipStreamSynchronize(ctx->stream));  // the scratch goes back to the pool behind finished work
  *out = R.release();
  return TPG_OK;
}

extern "C" int64_t tpg_roh_count(const tpg_roh* r) { return r ? r->count : 0; }

extern "C" int tpg_roh_fetch(tpg_ctx* ctx, const tpg_roh* r, int32_t* indiv0, int64_t* first0, int64_t* last0, int32_t* n_opp,
                             int32_t* n_miss) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && r, TPG_EINVAL, "null argument");
  const size_t c = (size_t)r->count;
  TPG_TRY(roh_out(ctx, indiv0, r->indiv.p, sizeof(int32_t) * c));
  TPG_TRY(roh_out(ctx, first0, r->first.p, sizeof(int64_t) * c));
  TPG_TRY(roh_out(ctx, last0, r->last.p, sizeof(int64_t) * c));
  TPG_TRY(roh_out(ctx, n_opp, r->nopp.p, sizeof(int32_t) * c));
  TPG_TRY(roh_out(ctx, n_miss, r->nmiss.p, sizeof(int32_t) * c));
  return TPG_OK;
}

extern "C" int tpg_roh_indiv_summary(tpg_ctx* ctx, const tpg_roh* r, int64_t* n_runs, int64_t* sum_length_bps) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && r && n_runs && sum_length_bps, TPG_EINVAL, "null argument");
  OutBuf a, b;
  TPG_TRY(a.init(n_runs, sizeof(int64_t) * (size_t)r->n));
  TPG_TRY(b.init(sum_length_bps, sizeof(int64_t) * (size_t)r->n));
  TPG_HIP(hipMemsetAsync(a.d, 0, sizeof(int64_t) * (size_t)r->n, ctx->stream));
  TPG_HIP(hipMemsetAsync(b.d, 0, sizeof(int64_t) * (size_t)r->n, ctx->stream));
  if (r->count > 0) {
    TPG_LAUNCH(ctx, "roh_summary", tpg_roh_summary_kernel, dim3((unsigned)ceil_div(r->count, 256)), dim3(256), 0,
               r->indiv.as<int32_t>(), r->first.as<int64_t>(), r->last.as<int64_t>(), r->pos.as<int64_t>(), r->count,
               a.dev<unsigned long long>(), b.dev<unsigned long long>());
    TPG_CHECK_LAUNCH();
  }
  TPG_TRY(a.commit(ctx));
  TPG_TRY(b.commit(ctx));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return TPG_OK;
}

extern "C" int tpg_roh_locus_counts(tpg_ctx* ctx, const tpg_roh* r, int32_t* counts) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && r && counts, TPG_EINVAL, "null argument");
  const int64_t m = r->m;
  DevArena sc;
  int32_t *d_diff = nullptr, *d_sum = nullptr;
  TPG_TRY(sc.get(&d_diff, (size_t)m + 1));
  TPG_TRY(sc.get(&d_sum, (size_t)m + 1));
  TPG_HIP(hipMemsetAsync(d_diff, 0, sizeof(int32_t) * ((size_t)m + 1), ctx->stream));
  if (r->count > 0) {
    TPG_LAUNCH(ctx, "roh_diff", tpg_roh_diff_kernel, dim3((unsigned)ceil_div(r->count, 256)), dim3(256), 0, r->first.as<int64_t>(),
               r->last.as<int64_t>(), r->count, d_diff);
    TPG_CHECK_LAUNCH();
  }
  {
    size_t t_scan = 0;
    TPG_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, t_scan, d_diff, d_sum, (int)(m + 1), ctx->stream));
    uint8_t* d_tmp = nullptr;
    TPG_TRY(sc.get(&d_tmp, t_scan));
    ProfScope ps(ctx, "roh_locus_scan");
    TPG_HIP(hipcub::DeviceScan::InclusiveSum(d_tmp, t_scan, d_diff, d_sum, (int)(m + 1), ctx->stream));
  }
  TPG_TRY(roh_out(ctx, counts, d_sum, sizeof(int32_t) * (size_t)m));
  TPG_HIP(hipStreamSynchronize(ctx->stream));
  return TPG_OK;
}

extern "C" void tpg_roh_free(tpg_roh* r) { delete r; }
