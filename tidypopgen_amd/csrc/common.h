// common.h -- internal declarations shared by the HIP translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "../../include/tpg.h"

// ---------------------------------------------------------------------------
// error plumbing (nothing throws across the C ABI)
void tpg_set_error(const char* fmt, ...);

#define TPG_HIP(call)                                                                        \
  do {                                                                                       \
    hipError_t _e = (call);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      tpg_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(_e));     \
      return TPG_EHIP;                                                                       \
    }                                                                                        \
  } while (0)

#define TPG_REQUIRE(cond, code, ...)  \
  do {                                \
    if (!(cond)) {                    \
      tpg_set_error(__VA_ARGS__);     \
      return (code);                  \
    }                                 \
  } while (0)

#define TPG_TRY(call)          \
  do {                         \
    int _rc = (call);          \
    if (_rc != TPG_OK) return _rc; \
  } while (0)

// ---------------------------------------------------------------------------
struct ProfRec {
  std::string name;
  hipEvent_t start, stop;
};

struct tpg_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  bool prof = false;
  std::set<std::string> prof_only;  // empty: every launch is timed
  std::vector<ProfRec> prof_pending;
  std::map<std::string, std::pair<double, int64_t>> prof_acc;  // name -> (ms, launches)
  std::vector<hipEvent_t> event_pool;
  int num_cu = 256;
  int pool_id = 0;  // this context's device-memory pool (runtime.hip): blocks are reused in the order of ITS stream
  void* resident = nullptr;  // pairwise.hip: accumulators kept across increment_* calls
  // pca.hip, digit-split Gram kernel: fractional bits the per-locus weights keep (22: within 2^-23 of the weight, what a
  // whole-panel Gram matrix averages down to 1e-10; a streamed run (stream.hip) adds up many short blocks and asks for 30)
  int pca_digit_fbits = 22;
  // small host -> device copies without a stream synchronisation: a ring of pinned slots (runtime.hip: tpg_h2d_async)
  static constexpr int H2D_SLOTS = 8;
  static constexpr size_t H2D_SLOT_BYTES = 256u << 10;
  uint8_t* h2d_pinned = nullptr;
  hipEvent_t h2d_done[H2D_SLOTS] = {};
  bool h2d_used[H2D_SLOTS] = {};
  int h2d_next = 0;
  // Small results and small inputs WITHOUT the runtime's copy engines or a stream synchronisation (runtime.hip:
  // tpg_fetch_small / tpg_push_small): a one-workgroup kernel copies between device memory and a coherent pinned "mailbox"
  // and raises a sequence number there; the host polls that word.  A hipMemcpyAsync + hipStreamSynchronize round trip
  // costs ~90 us of idle GPU on these boxes (tools/gaps.py), the mailbox ~10.
  static constexpr size_t MAIL_FETCH_BYTES = 64u << 10;   // one result at a time
  static constexpr size_t MAIL_PUSH_BYTES = 512u << 10;   // ring of inputs in flight
  static constexpr size_t MAIL_PUSH_MAX = 64u << 10;      // largest single input
  uint8_t* mail_host = nullptr;  // [flags: 64 B][fetch area][push ring]
  uint8_t* mail_dev = nullptr;   // the same memory as the device sees it
  uint32_t mail_fetch_seq = 0;
  uint32_t mail_push_seq = 0;    // sequence number of the last push
  size_t mail_push_off = 0;      // next free byte of the ring
  uint32_t mail_push_wrap_seq = 0;  // last push of the previous lap: must have been read before the ring is written again
};

struct ProfScope {
  tpg_ctx* ctx;
  ProfRec rec;
  bool on;
  ProfScope(tpg_ctx* c, const char* name);
  ~ProfScope();
};
int tpg_prof_resolve(tpg_ctx* ctx);
// gramcls.hip: S' = sum_j w_j g_i g_k' (n x n, column-major, both triangles) into d_K by weight classes; *done = false
// (nothing written) when the weights take too many distinct values for that to pay.  d_what (may be NULL): the weight
// actually used for every locus (its class representative, within 2^-47 of w_j)
// centred_ok: the caller applies the double centring H K H afterwards, so terms r_i + r_k + const may be left out of S'
// (gramcls.hip: the centred operand layout of the mixed-fold kernel)
// force: take this route whatever the cost model says (the digit route cannot hold these weights in int64); *done is still
// false where the route cannot run at all (TPG_GRAM_DIGITS, m >= 2^31 - 64)
int tpg_gram_classes(tpg_ctx* ctx, const struct tpg_view* v, const double* d_w, double* d_what, double* d_K, bool* done,
                     bool centred_ok, bool force = false);
// The same over the ranks of a communicator, with whole weight classes per rank: `v` holds this rank's loci (counts: its
// m x 4 genotype counts, scale: its binomial scales), the packed columns are exchanged so that rank r ends up with ALL loci
// of the allele-count range it owns, and d_K receives S' of those classes (the sum over the ranks is S' of the panel).
// *done = false (on every rank alike, nothing exchanged) when that would not pay.
int tpg_gram_classes_exchanged(tpg_ctx* ctx, struct tpg_comm* comm, const struct tpg_view* v, const int32_t* d_counts,
                               const double* d_scale, double* d_K, bool* done);

// Launch a kernel on the context's stream, bracketed by HIP events when profiling is on.
#define TPG_LAUNCH(ctx, name, kernel, grid, block, shmem, ...)                          \
  do {                                                                                  \
    ProfScope _ps((ctx), (name));                                                       \
    hipLaunchKernelGGL(kernel, grid, block, shmem, (ctx)->stream, __VA_ARGS__);        \
  } while (0)

#define TPG_CHECK_LAUNCH() TPG_HIP(hipGetLastError())

// ---------------------------------------------------------------------------
// HBM layout of a packed view (see DESIGN.md "Data layout").
//
// A *fragment block* is 1 KiB = 64 lanes x 16 B.  Lane l = (r = l & 31, h = l >> 5)
// holds 4 dwords s = 0..3; dword s packs 16 two-bit codes, element e = 4k + b stored at
// bits [8b + 2k, 8b + 2k + 1], so that (w >> 2k) & 0x03030303 is the 4 code bytes of MFMA
// operand register k.  One dword is exactly the 16-deep K slice that lane (r, h) feeds to
// v_mfma_i32_32x32x32_i8 for row/column r.
//
//   T ("individual-tiled", contraction over loci: pairwise N x N, PCA Gram, Z.V):
//     block (rt, kg): lane (r,h), dword s, element e  <->  individual 32 rt + r,
//     locus 128 kg + 32 s + 16 h + e.          address: ((rt * KG + kg) * 64 + lane) * 16 B
//   L ("locus-tiled", contraction over individuals: per-locus / per-group counts, Z'u):
//     block (lt, q):  lane (r,h), dword s, element e  <->  locus 32 lt + r,
//     individual 128 q + 32 s + 16 h + e.      address: ((lt * Q + q) * 64 + lane) * 16 B
//
// Codes: 0,1,2 = alt-allele dosage, 3 = missing.  Padding (individuals >= n, loci >= m) is 3.
struct tpg_fbm {
  tpg_ctx* ctx;
  uint8_t* d_bytes;
  int64_t nrow, ncol;
  int64_t bed_bpl = 0;  // > 0: d_bytes is a PLINK .bed payload with this many bytes per SNP (4 genotypes per byte)
  bool pooled = false;  // d_bytes came from the context's pool (the per-block uploads of the increment_* mirrors)
};

// class-wise counts via MFMA: cls[n] in [0, nclass); cnt[3][Mpad][Cpad] (het, hom-alt, valid).  A description of the
// buffer the VIEW owns (tpg_view::gc_buf): good until the next tpg_grouped_counts on that view, or its end
struct GroupedCounts {
  int32_t* cnt = nullptr;
  int64_t Mpad = 0;  // 32 * n_lt
  int Cpad = 0;      // 32 * ceil(nclass/32)
  int nclass = 0;
};

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Size-bucketed cache of device allocations (hipMalloc / hipFree cost milliseconds and synchronise
// the device; a step of the hot path needs ~40 scratch buffers).  One pool PER CONTEXT: a context issues
// all its work on one stream, so a block that goes back to its pool and out again is reused in stream
// order; a block never crosses to another context (another device, or another stream of the same device).
// tpg_pmalloc() serves the context the calling thread entered last (TpgEnter, first statement of every C-ABI
// entry point, which also makes that context's device current); tpg_pfree() returns a block to the pool it
// came from, or to hipFree() when that context is gone or the pointer is not the pool's.
hipError_t tpg_pmalloc(void** p, size_t bytes);
void tpg_pfree(void* p);
void tpg_pool_trim(int pool_id);  // release the cached (free) blocks of one pool
struct TpgEnter {
  tpg_ctx* prev;
  explicit TpgEnter(tpg_ctx* ctx);
  ~TpgEnter();
};
tpg_ctx* tpg_current_ctx();

// The owner of ONE pool block: back to its pool at scope exit (the pool is the context's the calling thread entered).
// free() is the explicit early release: the pool is size-bucketed and reuse is stream-ordered, so a block of O(n m) or O(n^2)
// bytes that today goes back before a later allocation of the same call keeps an explicit free() at that spot.
struct DevBuf {
  void* p = nullptr;
  int alloc(size_t bytes) {
    free();
    TPG_HIP(tpg_pmalloc(&p, bytes ? bytes : 16));
    return TPG_OK;
  }
  template <typename T> int alloc_n(size_t count) { return alloc(sizeof(T) * count); }
  void free() { if (p) tpg_pfree(p); p = nullptr; }
  void* release() { void* q = p; p = nullptr; return q; }  // to a longer-lived owner
  template <typename T> T* as() const { return (T*)p; }
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.release()) {}
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { free(); p = o.release(); } return *this; }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { free(); }
};
// All scratch of one call, freed together
struct DevArena {
  std::vector<DevBuf> blocks;
  template <typename T> int get(T** p, size_t count) {
    DevBuf b;
    TPG_TRY(b.alloc_n<T>(count));
    *p = b.as<T>();
    blocks.push_back(std::move(b));
    return TPG_OK;
  }
};

// A view owns its layouts: the destructor returns T, L, LM, T4, lc_part and the cached counts to the pool.
struct tpg_view {
  tpg_ctx* ctx;
  int64_t n, m;    // kept individuals / loci
  int64_t Q, KG;   // ceil(n/128), ceil(m/128)
  mutable uint4* T = nullptr;  // (4Q) row tiles x KG blocks; NULL in the views of tpg_view_create_pair until somebody needs it
                               // (tpg_view_need_T builds it from L)
  mutable uint4* L;  // (4KG) locus tiles x Q blocks; NULL in a view that holds LM instead until somebody needs it
                     // (tpg_view_need_L builds it from LM)
  // L's 16-byte pieces LOCUS-MAJOR (devfrag.h: tpg_lm_piece), bytes_each like L: what the class Gram's gather and the loadings of
  // the PCA read.  The fast pack kernel writes it INSTEAD of L for the second (imputed) view of tpg_view_create_pair; a
  // view without it that goes to the class Gram is copied into a scratch LM per call (gramcls.hip: tpg_gcls_l2lm_kernel)
  mutable uint4* LM = nullptr;
  bool L_borrowed = false;  // L points into somebody else's block (stream.hip: the kept views' layouts end to end): not freed here
  size_t bytes_each;
  // T re-coded as FP4 (E2M1) operand nibbles for the pairwise kernel (pairwise.hip); written by the pack kernel for
  // the first view of tpg_view_create_pair, otherwise made from T on the first tpg_pairwise_accumulate; 2 x bytes_each
  mutable uint4* T4 = nullptr;
  // the last per-class counts computed on this view (grouped_alt_freq, grouped_summaries and the Fst
  // methods of one analysis all use the same grouping): reused while the class vector is unchanged
  mutable DevBuf gc_buf;  // gc_cache.cnt
  mutable GroupedCounts gc_cache;
  mutable std::vector<int32_t> gc_cls;
  // per-locus genotype counts as the fast pack kernel left them (it has every code in registers anyway): for each chunk of
  // 256 individuals and each locus one dword {codes with bit 0 set, with bit 1 set, with both} in fields of 10 bits,
  // lc_part[chunk * lc_row + locus]; tpg_launch_loci_counts adds the chunks up instead of reading the L layout again
  uint32_t* lc_part = nullptr;
  int lc_chunks = 0;
  int64_t lc_row = 0;

  // n x m with no layout yet, or with somebody else's L (borrowed: a piece of a longer locus-tiled buffer)
  tpg_view(tpg_ctx* c, int64_t n_, int64_t m_, uint4* borrowed_L = nullptr)
      : ctx(c), n(n_), m(m_), Q(ceil_div(n_, 128)), KG(ceil_div(m_, 128)), L(borrowed_L), L_borrowed(borrowed_L != nullptr),
        bytes_each((size_t)Q * (size_t)KG * 4096) {}
  tpg_view(const tpg_view&) = delete;
  tpg_view& operator=(const tpg_view&) = delete;
  ~tpg_view();          // runtime.hip
  // release everything that can be rebuilt: T, T4, lc_part, the cached counts, and LM where the view holds L as well
  void drop_derived();
};
typedef std::unique_ptr<tpg_view> ViewPtr;

// tile-packed int32 accumulators of the pairwise kernel: per unit (super-tile I of TPG_PW_TA row tiles, 32-column
// tile jt >= TA I) 5 products x TA sub-tiles x 16 accumulator registers x 64 lanes (MFMA C/D order)
// The slabs hold what the matrix cores summed: MM = mm' (m = missing) where the outputs want V = vv', HM = hm' and MH = mh'
// where they want A = hv' and its transpose; the readers rebuild V and A (pairwise.hip: tpg_pw_tile_counts).
#define TPG_PW_PRODUCTS 5
enum { TPG_PW_SLAB_MM = 0, TPG_PW_SLAB_D = 1 /* D, or D + H (TPG_PW_DH) */, TPG_PW_SLAB_H = 2, TPG_PW_SLAB_HM = 3, TPG_PW_SLAB_MH = 4 };
#define TPG_PW_TA 3        // A row tiles per wave: 96 x 32 pairs, 15 accumulator tiles (240 AGPRs); see pairwise.hip
#define TPG_PW_PLANE_INTS (TPG_PW_TA * 16 * 64)
#define TPG_PW_TILE_INTS (TPG_PW_PRODUCTS * TPG_PW_PLANE_INTS)
struct tpg_pairwise {
  tpg_ctx* ctx;
  int64_t n;
  int64_t nst;  // super-tiles of 32 TPG_PW_TA individuals
  int64_t ntp;  // number of (I, jt) unit slots = TA nst (nst + 1) / 2
  int32_t* acc;
  bool owns;
  void* order;  // device int2[nun]: the units (I, jt) that hold data, in XCD patch order (pairwise.hip)
  int64_t nun;
  int64_t loci;          // loci accumulated since the last zero (all ranks' loci after a reduction): overflow guard
  int64_t as_pad_quirk;  // reference quirk Q1: added to every allele-sharing numerator (tpg_pairwise_set_as_pad_quirk)
  // Sharding over the ranks of a tpg_comm (comm.hip).  The slab of unit (I, jt) sits at tpg_pw_unit_index + rowpad[I]:
  // super-tile rows are dealt to the ranks in contiguous bands of (nearly) equal unit counts, every band padded to
  // `chunk_units` slabs, so that ONE reduce-scatter with equal counts leaves rank r with the sums of band r.  A
  // single rank has one band, rowpad = 0 and chunk_units = ntp (+ tail_units): the unsharded layout.
  // The last `tail_units` slabs of every chunk are not tiles: they take the diagonals MM_ii and D_ii of ALL individuals (two
  // int32 vectors of 32 ceil(n / 32)), which V and A are rebuilt from.  A rank's band does not hold the diagonal tiles of the
  // columns to its right, so before the reduce-scatter every rank copies its partial diagonals into the tail of every chunk:
  // the one it gets back holds their sums.
  int nranks = 1, rank = 0;
  int64_t chunk_units = 0, tail_units = 0;
  std::vector<int32_t> band;   // nranks + 1 super-tile boundaries: band r = rows [band[r], band[r + 1])
  int64_t* rowpad = nullptr;   // device int64[nst]
  bool reduced = false;        // after tpg_pairwise_reduce: only this rank's band holds (complete) sums
  // tpg_pairwise_reduce_begin / _end (the reduce-scatter on a second communicator's stream)
  bool reducing = false;
  hipEvent_t ev_acc = nullptr, ev_red = nullptr;
  int64_t pending_loci = 0;
  int pending_lack = 0;
  // products (TPG_PW_V | D | H | A) every accumulate since the last zero has added: what the epilogues may read
  int have = 31;  // TPG_PW_HAVE_ALL
  // unit tables of the product-subset kernels (pairwise.hip), one per wave-tile shape: key 16 RA + RB -> (device int2[], count)
  std::map<int, std::pair<void*, int64_t>> orders;
};
#define TPG_PW_MAX_LOCI 2147483647ll
#define TPG_PW_HAVE_ALL (TPG_PW_ALL | TPG_PW_DH)  // tpg_pairwise.have after a zero: every product, and with D and H their sum
// the smallest product set that serves the outputs asked for (pairwise.hip kernels: {V, D+H}, {V, D}, {V, D, H}, {V, D, A}, all five)
static inline int tpg_pw_products_for(bool ibs, bool king, bool as_or_grm) {
  if (ibs && !king && !as_or_grm) return TPG_PW_FOR_IBS_ALONE;
  return (ibs ? TPG_PW_FOR_IBS : 0) | (king ? TPG_PW_FOR_KING : 0) | (as_or_grm ? TPG_PW_FOR_AS : 0);
}

// The TPG_* environment switches (INTEGRATION.md "Environment" has the list; tests/test_env_switches.py keeps it true).  Both
// read the environment on every call: a site that wants one read per process keeps the result in a static.
static inline bool tpg_env_set(const char* name) { return getenv(name) != nullptr; }
static inline int tpg_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// host -> device on the context's stream.  Up to a slot's size the source is copied into pinned memory first, so the
// caller's buffer is free at return and nothing waits for the stream; larger copies are waited for.
hipError_t tpg_h2d_async(tpg_ctx* ctx, void* dst, const void* src, size_t bytes);
// device -> host for small results (a multiple of 4 bytes, at most MAIL_FETCH_BYTES; anything else takes the copy engine):
// returns when the bytes are in host_dst, which is when everything enqueued before has run -- without draining the stream
// through the runtime
hipError_t tpg_fetch_small(tpg_ctx* ctx, void* host_dst, const void* d_src, size_t bytes);
// the other direction (the caller's buffer is free at return, nothing is waited for)
hipError_t tpg_push_small(tpg_ctx* ctx, void* d_dst, const void* host_src, size_t bytes);
// device -> device on the stream by a kernel (a hipMemcpyAsync between two kernels costs 15 - 30 us of idle GPU)
hipError_t tpg_copy_dev(tpg_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
// bulk transfers (waited for): large ones are chunked through pinned slots with a team of copying threads
hipError_t tpg_upload(tpg_ctx* ctx, void* dst, const void* src, size_t bytes);
hipError_t tpg_download(tpg_ctx* ctx, void* dst, const void* src, size_t bytes);
// host FBM bytes that will be read through ONE code table: as 2 bits per genotype where table and bytes allow it (runtime.hip)
int tpg_fbm_from_host_for_table(tpg_ctx* ctx, const uint8_t* bytes, int64_t nrow, int64_t ncol, const double* code256, tpg_fbm** out,
                                const double** view_table);
// FBM bytes -> a .bed payload in HBM, packed to 2 bits per genotype on the host through lut16 (runtime.hip); *ok = false: send bytes instead
hipError_t tpg_upload_bedpacked(tpg_ctx* ctx, uint8_t* dst, const uint8_t* src, int64_t nrow, int64_t ncols, const uint8_t* lut16, bool* ok);
// `height` contiguous device pieces of `width` bytes -> host pieces `dpitch` bytes apart (rows of a column-major host matrix)
hipError_t tpg_download_rows(tpg_ctx* ctx, void* dst, size_t dpitch, const void* src, size_t width, size_t height);
// pinned staging buffers (256 MiB each) the process keeps between transfers: at least `buffers` from now on (freeing one
// synchronises the device, so a caller that runs several transfers at once -- tpg_multi's device threads -- raises it first)
void tpg_stage_keep(int buffers);

// device allocation helpers
template <typename T>
static inline int tpg_dmalloc(T** p, size_t count) {
  TPG_HIP(hipMalloc((void**)p, count * sizeof(T) > 0 ? count * sizeof(T) : 16));
  return TPG_OK;
}

// Output buffer that may be host or device memory: kernels write to dev(); commit() copies back
// if the user's pointer is not device memory.
bool tpg_is_device_ptr(const void* p);
struct OutBuf {
  void* user = nullptr;
  void* d = nullptr;
  size_t bytes = 0;
  bool owned = false;
  int init(void* user_ptr, size_t nbytes);
  int commit(tpg_ctx* ctx);  // async copy on ctx stream (+ sync) when user is host memory
  ~OutBuf();
  template <typename T> T* dev() { return (T*)d; }
};
// Input buffer: host or device pointer -> device pointer
struct InBuf {
  const void* d = nullptr;
  void* owned_ptr = nullptr;
  int init(tpg_ctx* ctx, const void* user_ptr, size_t nbytes);
  ~InBuf();
  template <typename T> const T* dev() { return (const T*)d; }
};
// Input array the HOST reads (argument checks, plans): the user's pointer if it is host memory, else `count` elements come down
template <typename T>
struct HostIn {
  const T* p = nullptr;
  std::vector<T> keep;
  int init(tpg_ctx* ctx, const T* user, int64_t count) {
    p = user;
    if (!tpg_is_device_ptr(user)) return TPG_OK;
    keep.resize((size_t)count);
    TPG_HIP(tpg_download(ctx, keep.data(), user, sizeof(T) * (size_t)count));
    p = keep.data();
    return TPG_OK;
  }
  const T& operator[](int64_t i) const { return p[i]; }
};
// device -> the caller's array (host or device memory); a NULL `user` is an output nobody asked for
template <typename T>
static inline int tpg_deliver(tpg_ctx* ctx, T* user, const T* d_src, size_t count) {
  if (!user || !count) return TPG_OK;
  if (tpg_is_device_ptr(user)) TPG_HIP(tpg_copy_dev(ctx, user, d_src, sizeof(T) * count));
  else TPG_HIP(tpg_download(ctx, user, d_src, sizeof(T) * count));
  return TPG_OK;
}
// runtime.hip: every entry of a device array finite, else TPG_ENUMERIC naming `what`; `sc` is the call's scratch (it gives the flag)
int tpg_check_finite(tpg_ctx* ctx, const double* dX, int64_t count, DevArena& sc, const char* what);
// every [lo[i], hi[i]) inside [0, m], lo / hi in host or device memory; what = "window" | "block" (runtime.hip)
int tpg_check_ranges(tpg_ctx* ctx, const int64_t* lo, const int64_t* hi, int64_t count, int64_t m, const char* what);

void tpg_resident_release(tpg_ctx* ctx);

// collectives over the ranks of a communicator (comm.hip).  One rank = one context.  Transport: RCCL (production:
// one process per GPU, or one process driving several GPUs), or a caller-supplied all-reduce through host memory
// (rehearsals of the sharded paths without RCCL: tests with gloo, several ranks sharing one GPU).
struct tpg_comm {
  tpg_ctx* ctx = nullptr;
  int nranks = 1, rank = 0;
  void* nccl = nullptr;  // ncclComm_t
  int (*host_fn)(void* user, void* buf, int64_t count, int dtype) = nullptr;  // in-place sum; dtype 0 int32, 1 float64
  void* host_user = nullptr;
  int32_t* d_status = nullptr;  // device int32[TPG_COMM_STATUS_INTS]: the status word of tpg_comm_agree
  int a2a_state = 0;            // tpg_comm_alltoall_usable: 0 not tried yet, 1 works, -1 does not (on every rank alike)
};
#define TPG_COMM_STATUS_INTS 8
// pca.hip: the k largest eigenpairs of the symmetric K (device memory) at relative residual tol; lambda on the host, U (n x k) in device memory
int tpg_sym_eig_topk_tol(tpg_ctx* ctx, const double* d_K, int64_t n, int k, double tol, double* lambda_host, double* d_U);
int tpg_pca_gram_allreduce(tpg_ctx* ctx, tpg_comm* comm, double* d_K, int64_t n);  // pca.hip: K <- sum over the ranks (its triangle travels)
// pca.hip: the FP64 row-scaled sweep (tpg_sweep_kernel<KC, SW_ROWSCALE>) over the L layout of a view, all in device memory:
// out[j + k m] = sum_i (g_ij - center[j]) * inv_scale[j] * U[i + k n], a missing genotype adding 0; waits for the stream
int tpg_sweep_loci_rowscale(tpg_ctx* ctx, const struct tpg_view* v, const double* d_center, const double* d_inv_scale, const double* d_U,
                            int K, double* d_out);
// pca.hip: the sweep of tpg_fbm256_prod_and_rowSumsSq with every array in device memory (d_scale is the scale, not its inverse):
// d_XV n x K, d_rss[n]; waits for the stream
int tpg_sweep_indiv_colscale(tpg_ctx* ctx, const struct tpg_view* v, const double* d_center, const double* d_scale, const double* d_V,
                             int K, double* d_XV, double* d_rss);
// pcaop.hip: the scaled genotype matrix Z = (G - 1c')S^-1 of a view as an operator on int8 MFMA.  The struct owns the
// scratch of both halves (tpg_pcaop_work_bytes: digit fragments, int32 partial tiles, the m x bmax block between the
// halves), all of it linear in n and in m; center and scale stay the caller's (device memory).  The view must hold no
// missing value and the scale no zero -- the callers' counts check that.  Nothing here waits for the stream.
struct TpgPcaOp {
  const struct tpg_view* v = nullptr;
  const double *d_center = nullptr, *d_scale = nullptr;
  int bmax = 0;
  uint4* UD = nullptr;
  int32_t* part = nullptr;
  double *W = nullptr, *stat = nullptr;
  int n_apply = 0;  // applications of Z Z' so far
  DevArena mem;
};
int tpg_pcaop_init(tpg_ctx* ctx, TpgPcaOp* op, const struct tpg_view* v, const double* d_center, const double* d_scale, int bmax);
size_t tpg_pcaop_work_bytes(int64_t n, int64_t m, int bmax, int num_cu);
int tpg_pcaop_zt(tpg_ctx* ctx, TpgPcaOp* op, const double* d_Q, int b, double* d_W);     // W (m x b) = Z'Q
int tpg_pcaop_z(tpg_ctx* ctx, TpgPcaOp* op, const double* d_W, int b, double* d_Y);      // Y (n x b) = Z W
int tpg_pcaop_apply(tpg_ctx* ctx, TpgPcaOp* op, const double* d_Q, int b, double* d_Y);  // Y = Z (Z'Q), b <= bmax
// stream.hip: a tpg_multi_* analysis of a host FBM with every device streaming its share in blocks under `budget` bytes
int tpg_multi_stream_host(tpg_multi* mg, const uint8_t* fbm_bytes, int64_t nrow, int64_t ncol, size_t budget, const tpg_stream_job* job);
int tpg_comm_agree(tpg_comm* comm, int rc);  // all ranks get the same status (the worst any of them passed in)
int tpg_comm_reduce_scatter_i32(tpg_comm* comm, int32_t* d_buf, int64_t chunk_count);  // in place, chunk r -> rank r
int tpg_comm_allreduce(tpg_comm* comm, void* d_buf, int64_t count, int dtype);          // in place, device memory
// 8-byte words: rank r sends scnt[d] words at soff[d] to rank d, receives rcnt[s] words from rank s at roff[s]
// a tiny all-to-all with known contents, once per communicator: true on every rank or on none.  The class exchange of the
// PCA Gram (gramcls.hip) is only taken when it is.
bool tpg_comm_alltoall_usable(tpg_comm* comm);
int tpg_comm_alltoallv64(tpg_comm* comm, const void* d_send, const size_t* scnt, const size_t* soff, void* d_recv,
                         const size_t* rcnt, const size_t* roff);

// ---- cross-TU entry points (one per .hip file) -----------------------------
int tpg_launch_pack(tpg_ctx* ctx, const tpg_fbm* fbm, const int32_t* d_rows, const int32_t* d_cols,
                    const uint8_t* d_lut, tpg_view* v, tpg_view* v2);
int tpg_launch_unpack(tpg_ctx* ctx, const tpg_view* v, uint8_t* d_codes, int from_L);
// the T layout of a view that was packed without it (from L; a no-op when it is there)
int tpg_view_need_T(tpg_ctx* ctx, const tpg_view* v);
// the L layout of a view that was packed locus-major (from LM; a no-op when it is there): every reader of v->L calls it first
int tpg_view_need_L(tpg_ctx* ctx, const tpg_view* v);
// impute.hip: tpg_view_impute with the view's first locus at position col0 of the object being imputed (a streamed block)
int tpg_view_impute_at(tpg_ctx* ctx, const tpg_view* raw, int method, uint64_t seed, int64_t col0, tpg_view** out,
                       tpg_impute_report* rep);
int tpg_launch_synth(tpg_ctx* ctx, uint8_t* d_bytes, uint64_t seed, int64_t nrow, int64_t ncol, int64_t j0,
                     int npop, uint32_t miss_thresh, int imputed_bytes);

// per-locus
int tpg_launch_loci_counts(tpg_ctx* ctx, const tpg_view* v, int32_t* d_counts /* m x 4 */);
int tpg_grouped_counts(tpg_ctx* ctx, const tpg_view* v, const int32_t* h_cls, int nclass, GroupedCounts* out);
// Class scheme shared by the grouped entry points (loci.hip): with pseudohaploids present class = 2*g + (ploidy==1),
// otherwise class = g.  (ploidy is 1 or 2: the reference's dip_pseudo kernels assume it too.)  groupIds0 == NULL: all in group 0
struct ClassPlan {
  std::vector<int32_t> cls;
  std::vector<int32_t> group_size;
  int nclass = 0;
  int has_hap = 0;
};
int make_class_plan(int64_t n, const int32_t* groupIds0, int ngroups, const double* ploidy, ClassPlan* cp);
// its argument checks alone: ngroups > 0 and every id in [0, ngroups) (TPG_EINVAL); every ploidy 2 (TPG_EINVAL, "<what> only
// works on diploid data": the reference's stopifnot_diploid)
int tpg_check_group_ids(int64_t n, const int32_t* groupIds0, int ngroups);
int tpg_require_diploid(int64_t n, const double* ploidy, const char* what);
// per-individual counts that add up over views (loci.hip): d_acc (n x 4 int32, zero before the first view) += the view's loci,
// read from L; tpg_launch_indiv_finish turns the sums over m loci into {n0, n1, n2, nNA} (d_out may be d_acc)
int tpg_launch_indiv_accumulate(tpg_ctx* ctx, const tpg_view* v, int32_t* d_acc);
int tpg_launch_indiv_finish(tpg_ctx* ctx, const int32_t* d_acc, int64_t n, int64_t m, int32_t* d_out);
