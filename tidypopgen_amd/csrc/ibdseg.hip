// ibdseg.hip -- IBD segments between pairs of individuals (tpg_ibd_segments) on the device.  The definition is in include/tpg.h
// ("IBD segments"); DESIGN.md 3.22 has the mapping and what bounds the kernel.
//
//  * tpg_ibd_scan_kernel: a workgroup owns a tile of 32 x 32 pairs (row tile ta <= column tile tb; a diagonal tile keeps a < b)
//    and walks the panel in chunks of TPG_IBD_CHUNK_LOCI loci.  Per chunk its four waves read the 1-KiB blocks of T of the 64
//    individuals whole and turn the two-bit codes into locus-ordered masks in LDS by the shuffle of locusbits.h, 32 loci per
//    word: hom0, hom2 and typed for kind 1, the two code planes and typed for kind 2.  A lane carries four pairs (one column,
//    four rows) with the state of host/host_ibdseg.h in registers: a word without bad locus and break costs one popcount,
//    otherwise the lane steps through the set bits -- with thresholds of 33 loci or more only up to the point where nothing
//    is open any more (host_ibd_skip_short).  The brk bits come up once on the host, for all pairs.
//  * EMIT = false counts the reported segments of every pair and adds up their lengths; a scan over the pairs in (a, b) order
//    gives every pair its place; EMIT = true walks again and writes -- only the tiles that hold a segment.  A pair's segments
//    close in ascending order, so the table comes out ordered by (a, b, first) whatever the launch geometry.
#include "common.h"
#include "host/host_ibdseg.h"
#include "locusbits.h"
#include <hipcub/hipcub.hpp>

#define IBD_CB 8                       // blocks of 128 loci per chunk
#define IBD_CHUNK (128 * IBD_CB)       // = TPG_IBD_CHUNK_LOCI
#define IBD_NW (4 * IBD_CB)            // words per individual and chunk
#define IBD_NWP (IBD_NW + 1)           // odd: the 32 rows a wave reads at one word fall into 32 banks
#define IBD_PPL 4                      // pairs per lane: rows (tid >> 5) + 8 k of column tid & 31
static_assert(IBD_CHUNK == TPG_IBD_CHUNK_LOCI, "include/tpg.h states the chunk length");

struct IbdOut {
  int32_t *ind_a, *ind_b, *n_typed, *n_err;
  int64_t *first, *last;
};

// what a lane does with a closed segment of one of its pairs
template <bool EMIT>
struct IbdSink {
  const int64_t* pos;
  int64_t min_snp, min_length, max_err;
  const IbdOut* out;
  int32_t a, b;
  int64_t at;  // EMIT: the place of the pair's next segment; else the number of reported segments so far
  int64_t sum;
  __device__ __forceinline__ void operator()(int32_t first, int32_t last, int32_t n_typed, int32_t n_err) {
    if (n_typed < min_snp) return;  // (before pos is read: nearly every segment ends here)
    const int64_t len = pos[last] - pos[first];
    if (!host_ibd_reported(n_typed, len, n_err, min_snp, min_length, max_err)) return;
    if (EMIT) {
      out->ind_a[at] = a;
      out->ind_b[at] = b;
      out->first[at] = first;
      out->last[at] = last;
      out->n_typed[at] = n_typed;
      out->n_err[at] = n_err;
    }
    at++;
    sum += len;
  }
};

// the place of the pair (a, b), a < b, among the n (n - 1) / 2 pairs in (a, b) order
__host__ __device__ __forceinline__ int64_t ibd_pair_index(int64_t a, int64_t b, int64_t n) { return a * n - a * (a + 1) / 2 + (b - a - 1); }

// grid (tb, ta), 256 threads.  brk: nchunks * IBD_NW words, bit m - 1 set.  cnt / sum / off: one entry per pair (ibd_pair_index).
template <int KIND, bool EMIT>
__global__ __launch_bounds__(256) void tpg_ibd_scan_kernel(const uint4* __restrict__ T, int64_t KG, int64_t n, int nchunks,
                                                           const uint32_t* __restrict__ brk, const int64_t* __restrict__ pos, int32_t B,
                                                           int64_t min_snp, int64_t min_length, int64_t max_err,
                                                           int64_t* __restrict__ cnt, int64_t* __restrict__ sum,
                                                           const int64_t* __restrict__ off, IbdOut out) {
  __shared__ uint32_t sm[3][64 * IBD_NWP];
  const int ta = blockIdx.y, tb = blockIdx.x;
  if (ta > tb) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int col = tid & 31, row0 = tid >> 5;
  const int64_t ib = (int64_t)tb * 32 + col;
  HostIbdState st[IBD_PPL];
  IbdSink<EMIT> sk[IBD_PPL];
  bool live[IBD_PPL];
  const bool skip = host_ibd_skip_short(min_snp, B);
  int any = 0;
#pragma unroll
  for (int k = 0; k < IBD_PPL; k++) {
    const int64_t ia = (int64_t)ta * 32 + row0 + 8 * k;
    live[k] = ia < ib && ib < n;
    sk[k] = IbdSink<EMIT>{pos, min_snp, min_length, max_err, &out, (int32_t)ia, (int32_t)ib, 0, 0};
    if (EMIT && live[k]) {
      sk[k].at = off[ibd_pair_index(ia, ib, n)];
      live[k] = cnt[ibd_pair_index(ia, ib, n)] > 0;  // a pair without a segment has nothing to write
    }
    any |= live[k] ? 1 : 0;
  }
  if (EMIT && !__syncthreads_or(any)) return;
  for (int ch = 0; ch < nchunks; ch++) {
    if (ch) __syncthreads();  // the previous chunk has been read
    // ---- blocks -> locus-ordered masks in LDS: 16 tasks (2 tiles x IBD_CB blocks), a wave each
    {
      const int r = lane & 31, h = lane >> 5;
      for (int task = wv; task < 2 * IBD_CB; task += 4) {
        const int side = task / IBD_CB, blk = task % IBD_CB;
        const int64_t kg = (int64_t)ch * IBD_CB + blk, rt = side ? tb : ta;
        uint4 f = make_uint4(~0u, ~0u, ~0u, ~0u);  // behind the panel: missing
        if (kg < KG) f = T[(rt * KG + kg) * 64 + lane];  // (the whole wave alike)
        uint32_t lo01, hi01, lo23, hi23;
        tpg_lb_planes(f.x, f.y, lo01, hi01);
        tpg_lb_planes(f.z, f.w, lo23, hi23);
        const uint32_t plo01 = (uint32_t)__shfl_xor((int)lo01, 32), phi01 = (uint32_t)__shfl_xor((int)hi01, 32);
        const uint32_t plo23 = (uint32_t)__shfl_xor((int)lo23, 32), phi23 = (uint32_t)__shfl_xor((int)hi23, 32);
        uint32_t lo[2], hi[2];
        tpg_lb_words(h, lo01, plo01, lo23, plo23, lo[0], lo[1]);
        tpg_lb_words(h, hi01, phi01, hi23, phi23, hi[0], hi[1]);
        const int at = (side * 32 + r) * IBD_NWP + 4 * blk + 2 * h;
#pragma unroll
        for (int q = 0; q < 2; q++) {
          sm[0][at + q] = KIND == 1 ? ~(lo[q] | hi[q]) : lo[q];  // hom0 | plane 0
          sm[1][at + q] = KIND == 1 ? hi[q] & ~lo[q] : hi[q];    // hom2 | plane 1
          sm[2][at + q] = ~(lo[q] & hi[q]);                      // typed
        }
      }
    }
    __syncthreads();
    // ---- the pairs
    const uint32_t* bw = brk + (size_t)ch * IBD_NW;
    const uint32_t* cb = &sm[0][(32 + col) * IBD_NWP];
    const int64_t left = KG * 4 - (int64_t)ch * IBD_NW;  // words of the panel from this chunk on
    const int nw = left < IBD_NW ? (int)left : IBD_NW;
    for (int w = 0; w < nw; w++) {
      const uint32_t brkw = bw[w];  // (uniform)
      const uint32_t b0 = cb[w], b1 = cb[64 * IBD_NWP + w], bt = cb[2 * 64 * IBD_NWP + w];
      const int32_t j0 = (ch * IBD_NW + w) * 32;
#pragma unroll
      for (int k = 0; k < IBD_PPL; k++) {
        if (!live[k]) continue;
        const uint32_t* ca = &sm[0][(row0 + 8 * k) * IBD_NWP];
        const uint32_t a0 = ca[w], a1 = ca[64 * IBD_NWP + w], typed = ca[2 * 64 * IBD_NWP + w] & bt;
        const uint32_t bad = KIND == 1 ? (a0 & b1) | (a1 & b0) : ((a0 ^ b0) | (a1 ^ b1)) & typed;
        host_ibd_word(st[k], j0, bad, typed, brkw, B, skip, sk[k]);
      }
    }
  }
  if (!EMIT) {
#pragma unroll
    for (int k = 0; k < IBD_PPL; k++) {
      const int64_t ia = (int64_t)ta * 32 + row0 + 8 * k;
      if (live[k]) {
        cnt[ibd_pair_index(ia, ib, n)] = sk[k].at;
        sum[ibd_pair_index(ia, ib, n)] = sk[k].sum;
      }
    }
  }
}

// the per-pair counts and sums -> the n x n outputs (either may be NULL): symmetric, zero diagonal
__global__ __launch_bounds__(256) void tpg_ibd_mirror_kernel(const int64_t* __restrict__ cnt, const int64_t* __restrict__ sum, int64_t n,
                                                             int32_t* __restrict__ nseg, int64_t* __restrict__ total) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n * n) return;
  const int64_t a = k / n, b = k % n;
  const int64_t p = a == b ? -1 : ibd_pair_index(a < b ? a : b, a < b ? b : a, n);
  if (nseg) nseg[k] = p < 0 ? 0 : (int32_t)cnt[p];
  if (total) total[k] = p < 0 ? 0 : sum[p];
}

extern "C" int64_t tpg_ibd_chunk_loci(void) { return IBD_CHUNK; }

extern "C" int tpg_ibd_genome_length(const int32_t* chrom, const int64_t* pos, int64_t m, int64_t max_gap, int64_t* length) {
  TPG_REQUIRE(chrom && pos && length, TPG_EINVAL, "null argument");
  TPG_REQUIRE(m >= 1, TPG_EINVAL, "no locus");
  TPG_REQUIRE(max_gap >= 0, TPG_EINVAL, "max_gap below 0");
  int64_t len = 0;
  const int64_t at = host_ibd_breaks(chrom, pos, m, max_gap, nullptr, &len);
  TPG_REQUIRE(at < 0, TPG_EINVAL, "loci are not ordered: position decreases at locus %lld", (long long)at);
  *length = len;
  return TPG_OK;
}

extern "C" int tpg_ibd_segments(tpg_ctx* ctx, const tpg_view* v, const int32_t* chrom, const int64_t* pos, int kind, int64_t min_snp,
                                int64_t min_length, int64_t max_gap, int64_t bridge_min_snp, int64_t max_err, int64_t cap,
                                int32_t* ind_a, int32_t* ind_b, int64_t* first0, int64_t* last0, int32_t* n_typed, int32_t* n_err,
                                int64_t* count, int32_t* pair_n_seg, int64_t* pair_sum_length) {
  TpgEnter _enter(ctx);
  TPG_REQUIRE(ctx && v && chrom && pos && count, TPG_EINVAL, "null argument");
  TPG_REQUIRE(v->m >= 1 && v->n >= 1, TPG_EINVAL, "empty view");
  TPG_REQUIRE(kind == 1 || kind == 2, TPG_EINVAL, "kind = %d, not 1 (IBD1) or 2 (IBD2)", kind);
  TPG_REQUIRE(min_snp >= 1, TPG_EINVAL, "min_snp below 1");
  TPG_REQUIRE(min_length >= 0 && max_gap >= 0 && bridge_min_snp >= 0, TPG_EINVAL, "min_length, max_gap or bridge_min_snp below 0");
  TPG_REQUIRE(cap >= 0, TPG_EINVAL, "cap below 0");
  TPG_REQUIRE(cap == 0 || (ind_a && ind_b && first0 && last0 && n_typed && n_err), TPG_EINVAL, "cap > 0 with a NULL segment array");
  const int64_t n = v->n, m = v->m;
  TPG_REQUIRE(m < (1ll << 31) - 64, TPG_EUNSUPPORTED, "IBD segments over 2^31 loci or more");
  TPG_REQUIRE(n <= 65536, TPG_EUNSUPPORTED, "IBD segments of more than 65536 individuals in one call");  // pairs + 1 < 2^31
  const int64_t nchunks = ceil_div(m, IBD_CHUNK), nrt = ceil_div(n, 32), nn = n * n, np = n * (n - 1) / 2;
  std::vector<uint32_t> brk((size_t)nchunks * IBD_NW, 0u);
  InBuf dpos;
  {
    HostIn<int32_t> ch;
    HostIn<int64_t> ps;
    TPG_TRY(ch.init(ctx, chrom, m));
    TPG_TRY(ps.init(ctx, pos, m));
    const int64_t at = host_ibd_breaks(ch.p, ps.p, m, max_gap, brk.data(), nullptr);
    TPG_REQUIRE(at < 0, TPG_EINVAL, "loci are not ordered: position decreases at locus %lld", (long long)at);
    TPG_TRY(dpos.init(ctx, pos, sizeof(int64_t) * (size_t)m));
  }
  TPG_TRY(tpg_view_need_T(ctx, v));
  DevArena sc;
  uint32_t* d_brk = nullptr;
  int64_t *d_cnt = nullptr, *d_off = nullptr, *d_sum = nullptr, *d_total = nullptr;
  int32_t* d_nseg = nullptr;
  TPG_TRY(sc.get(&d_brk, brk.size()));
  TPG_HIP(tpg_upload(ctx, d_brk, brk.data(), sizeof(uint32_t) * brk.size()));
  TPG_TRY(sc.get(&d_cnt, (size_t)np + 1));
  TPG_TRY(sc.get(&d_off, (size_t)np + 1));
  TPG_TRY(sc.get(&d_sum, (size_t)np + 1));
  TPG_HIP(hipMemsetAsync(d_cnt, 0, sizeof(int64_t) * ((size_t)np + 1), ctx->stream));  // (the walks write every pair; entry np is the scan's)
  if (pair_n_seg) TPG_TRY(sc.get(&d_nseg, (size_t)nn));
  if (pair_sum_length) TPG_TRY(sc.get(&d_total, (size_t)nn));
  // a typed count never reaches 2^31: larger thresholds mean "never"
  const int32_t B = (int32_t)(bridge_min_snp < INT32_MAX ? bridge_min_snp : INT32_MAX);
  const dim3 grid((unsigned)nrt, (unsigned)nrt);
  const IbdOut none{};
  if (kind == 1)
    TPG_LAUNCH(ctx, "ibd_count_1", (tpg_ibd_scan_kernel<1, false>), grid, dim3(256), 0, (const uint4*)v->T, v->KG, n, (int)nchunks,
               (const uint32_t*)d_brk, dpos.dev<int64_t>(), B, min_snp, min_length, max_err, d_cnt, d_sum, (const int64_t*)nullptr, none);
  else
    TPG_LAUNCH(ctx, "ibd_count_2", (tpg_ibd_scan_kernel<2, false>), grid, dim3(256), 0, (const uint4*)v->T, v->KG, n, (int)nchunks,
               (const uint32_t*)d_brk, dpos.dev<int64_t>(), B, min_snp, min_length, max_err, d_cnt, d_sum, (const int64_t*)nullptr, none);
  TPG_CHECK_LAUNCH();
  {
    size_t t_scan = 0;
    TPG_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, t_scan, d_cnt, d_off, (int)(np + 1), ctx->stream));
    uint8_t* d_tmp = nullptr;
    TPG_TRY(sc.get(&d_tmp, t_scan));
    ProfScope ps(ctx, "ibd_pair_scan");
    TPG_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, t_scan, d_cnt, d_off, (int)(np + 1), ctx->stream));
  }
  int64_t total = 0;
  TPG_HIP(tpg_fetch_small(ctx, &total, d_off + np, sizeof(total)));
  IbdOut o{};
  if (total > 0 && total <= cap) {
    TPG_TRY(sc.get(&o.ind_a, (size_t)total));
    TPG_TRY(sc.get(&o.ind_b, (size_t)total));
    TPG_TRY(sc.get(&o.first, (size_t)total));
    TPG_TRY(sc.get(&o.last, (size_t)total));
    TPG_TRY(sc.get(&o.n_typed, (size_t)total));
    TPG_TRY(sc.get(&o.n_err, (size_t)total));
    if (kind == 1)
      TPG_LAUNCH(ctx, "ibd_emit_1", (tpg_ibd_scan_kernel<1, true>), grid, dim3(256), 0, (const uint4*)v->T, v->KG, n, (int)nchunks,
                 (const uint32_t*)d_brk, dpos.dev<int64_t>(), B, min_snp, min_length, max_err, d_cnt, d_sum, (const int64_t*)d_off, o);
    else
      TPG_LAUNCH(ctx, "ibd_emit_2", (tpg_ibd_scan_kernel<2, true>), grid, dim3(256), 0, (const uint4*)v->T, v->KG, n, (int)nchunks,
                 (const uint32_t*)d_brk, dpos.dev<int64_t>(), B, min_snp, min_length, max_err, d_cnt, d_sum, (const int64_t*)d_off, o);
    TPG_CHECK_LAUNCH();
  }
  if (pair_n_seg || pair_sum_length) {
    TPG_LAUNCH(ctx, "ibd_mirror", tpg_ibd_mirror_kernel, dim3((unsigned)ceil_div(nn, 256)), dim3(256), 0, (const int64_t*)d_cnt, (const int64_t*)d_sum, n,
               d_nseg, d_total);
    TPG_CHECK_LAUNCH();
  }
  TPG_HIP(hipStreamSynchronize(ctx->stream));  // every kernel has run: from here on the caller's arrays are written
  if (total > 0 && total <= cap) {
    TPG_TRY(tpg_deliver(ctx, ind_a, (const int32_t*)o.ind_a, (size_t)total));
    TPG_TRY(tpg_deliver(ctx, ind_b, (const int32_t*)o.ind_b, (size_t)total));
    TPG_TRY(tpg_deliver(ctx, first0, (const int64_t*)o.first, (size_t)total));
    TPG_TRY(tpg_deliver(ctx, last0, (const int64_t*)o.last, (size_t)total));
    TPG_TRY(tpg_deliver(ctx, n_typed, (const int32_t*)o.n_typed, (size_t)total));
    TPG_TRY(tpg_deliver(ctx, n_err, (const int32_t*)o.n_err, (size_t)total));
  }
  TPG_TRY(tpg_deliver(ctx, pair_n_seg, (const int32_t*)d_nseg, (size_t)nn));
  TPG_TRY(tpg_deliver(ctx, pair_sum_length, (const int64_t*)d_total, (size_t)nn));
  if (tpg_is_device_ptr(count)) {
    TPG_HIP(tpg_push_small(ctx, count, &total, sizeof(total)));
  } else {
    *count = total;
  }
  TPG_HIP(hipStreamSynchronize(ctx->stream));  // the scratch goes back to the pool behind finished work
  return TPG_OK;
}
