/*
 * tpg.h -- C ABI of the MI355X-native tidypopgen hot path (libtpg_hip.so).
 *
 * This is the drop-in boundary.  The reference crosses from R into native code
 * through `.Call` on Rcpp-generated shims (R/RcppExports.R:4-91, registration
 * table src/RcppExports.cpp:348-377); every entry point below states which of
 * those native functions (and which R driver loop around it) it replaces.  An R
 * shim that binds them is shown in INTEGRATION.md.
 *
 * Conventions (identical to the reference's):
 *   - the genotype store is a bigstatsr FBM.code256: uint8, column-major,
 *     element (i,j) at bytes[i + j*nrow];
 *   - rowInd / colInd are 1-based int32 (as R passes them; src/snp_ibs.cpp:35);
 *   - groupIds are 0-based int32 (R/loci_alt_freq.R:179);
 *   - code256 is double[256], NA = any NaN.  The device path packs genotypes to
 *     2 bits, so every non-NA entry of code256 that occurs must be 0, 1 or 2
 *     (CODE_012 / CODE_IMPUTE_PRED both are); anything else -> TPG_EUNSUPPORTED.
 *     code256 == NULL means "raw bytes": 0/1/2 valid, everything else missing,
 *     which is what increment_{ibs,king,as}_counts do regardless of code256
 *     (src/snp_ibs.cpp:47-54);
 *   - all matrices are column-major doubles, as R stores them;
 *   - output pointers may be host or device memory (hipMemcpyDefault).
 *
 * Every function returns 0 on success, a TPG_E* code otherwise; the message is
 * available from tpg_last_error() (thread-local).  Nothing throws across the
 * boundary.  One host thread per context at a time (R's main thread).
 * There is NO CPU fallback: without a usable HIP device every call fails.
 */
#ifndef TPG_H
#define TPG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPG_OK 0
#define TPG_EINVAL 1       /* bad argument */
#define TPG_EHIP 2         /* HIP runtime error (no device, OOM, launch failure) */
#define TPG_EUNSUPPORTED 3 /* e.g. code256 value outside {0,1,2,NA} */
#define TPG_ENUMERIC 4     /* e.g. missing value / zero scale in PCA (big_SVD stops too) */

typedef struct tpg_ctx tpg_ctx;   /* one GPU, one stream */
typedef struct tpg_fbm tpg_fbm;   /* FBM bytes resident in HBM */
typedef struct tpg_view tpg_view; /* (FBM, rowInd, colInd, code256) packed to 2 bits in HBM */
typedef struct tpg_pairwise tpg_pairwise; /* int32 N x N cross-product accumulators in HBM */
typedef struct tpg_comm tpg_comm;   /* one rank (= one context = one GPU) of a group that shares an analysis sharded by loci */
typedef struct tpg_multi tpg_multi; /* one process driving several GPUs: a context and a communicator per device */

const char* tpg_last_error(void);
const char* tpg_version(void);

/* ---- context ---------------------------------------------------------- */
/* HIP devices visible to this process (0 when there is none or the runtime fails: tpg_ctx_create then says why) */
int tpg_device_count(int* count);
int tpg_ctx_create(int device, tpg_ctx** out);
void tpg_ctx_destroy(tpg_ctx* ctx);
/* One process per GPU on a host with several NUMA nodes: keep the CALLING thread -- and every thread it starts afterwards: the
   upload, pack, download and add teams of this library are started by their caller -- on the CPUs of the node `device` hangs
   off, so that the buffers they touch first land there too.  What a launcher does with `numactl --cpunodebind`; the unmodified
   block loop of an R driver took 0.40 s spread over both sockets of the pool's hosts and 0.31 s on one.
   *node = the node bound to, or -1 when nothing was done: the host has one node, the device's node is unknown, or fewer than
   16 of the CPUs this process may use are on it.  Never an error for those; call it before the process allocates its buffers. */
int tpg_host_bind_near_device(int device, int* node);
/* use an externally owned hipStream_t (e.g. torch's current stream); NULL = own stream */
int tpg_ctx_set_stream(tpg_ctx* ctx, void* hip_stream);
int tpg_ctx_sync(tpg_ctx* ctx);
/* per-kernel HIP-event timing (on the context's stream) */
int tpg_prof_enable(tpg_ctx* ctx, int on);
int tpg_prof_reset(tpg_ctx* ctx);
/* time only the launches whose name is in the comma-separated list (NULL or "": all).  Two event records around a
   launch cost ~5 us of idle GPU on the stream: a timed run brackets the few kernels it prices, not all of them */
int tpg_prof_only(tpg_ctx* ctx, const char* names_csv);
/* total milliseconds and launch count of kernels whose name starts with `prefix` */
int tpg_prof_get(tpg_ctx* ctx, const char* prefix, double* total_ms, int64_t* launches);
/* writes "name\tlaunches\ttotal_ms\n" lines into buf (truncated to cap) */
int tpg_prof_dump(tpg_ctx* ctx, char* buf, size_t cap);

/* plain device buffers for callers without their own allocator (outputs may be device memory) */
int tpg_dev_alloc(tpg_ctx* ctx, size_t bytes, void** out);
void tpg_dev_free(void* p);
/* both copies are complete when the call returns, whatever the size (the context's stream has been waited for) */
int tpg_dev_to_host(tpg_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes);
int tpg_dev_from_host(tpg_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);

/* ---- genotype store (replaces the mmapped FBM) -------- */
int tpg_fbm_from_host(tpg_ctx* ctx, const uint8_t* bytes, int64_t nrow, int64_t ncol, tpg_fbm** out);
/* mmap bigstatsr's <backingfile>.bk and upload it */
int tpg_fbm_open_bk(tpg_ctx* ctx, const char* path, int64_t nrow, int64_t ncol, tpg_fbm** out);
/* An FBM that arrives block of columns by block of columns (the reference's own block loop, R/snp_ibs.R:59-82):
 * tpg_fbm_alloc reserves the HBM, tpg_fbm_upload_cols fills columns [col0, col0 + ncols) (0-based) from host memory.
 * Called from a second host thread with a context of its own, the upload of block b + 1 overlaps the pack /
 * accumulate kernels of block b (views over columns already uploaded).  bench.py's end_to_end leg is the worked example. */
int tpg_fbm_alloc(tpg_ctx* ctx, int64_t nrow, int64_t ncol, tpg_fbm** out);
int tpg_fbm_upload_cols(tpg_ctx* ctx, tpg_fbm* fbm, const uint8_t* host_cols, int64_t col0, int64_t ncols);
/* deterministic synthetic panel generated on the device (csrc/synth_common.h) */
int tpg_fbm_synth(tpg_ctx* ctx, uint64_t seed, int64_t nrow, int64_t ncol, int64_t j0, int npop,
                  uint32_t miss_thresh, int imputed_bytes, tpg_fbm** out);
/* a PLINK .bed file (SNP-major, 2 bits per genotype) as the genotype store, without
 * the 1-byte-per-genotype FBM in between (R/gen_tibble_bed.R:101-125 reads it into an FBM through bigsnpr's
 * readbina; the byte each 2-bit code would have become -- 00,01,10,11 -> 2,3,1,0 -- is what code256 is applied
 * to).  n / m are the line counts of the .fam / .bim files.  `bytes` is the payload after the 3-byte magic. */
int tpg_fbm_open_bed(tpg_ctx* ctx, const char* path, int64_t n, int64_t m, tpg_fbm** out);
int tpg_fbm_from_bed_host(tpg_ctx* ctx, const uint8_t* bytes, int64_t n, int64_t m, tpg_fbm** out);
/* the same store filled block of SNPs by block of SNPs (the .bed form of tpg_fbm_alloc / tpg_fbm_upload_cols: a block of SNPs
 * is one contiguous piece of the payload, ceil(n / 4) bytes per SNP): an uploader thread with a context of its own feeds
 * block b + 1 while views of block b are packed and analysed */
int tpg_fbm_alloc_bed(tpg_ctx* ctx, int64_t n, int64_t m, tpg_fbm** out);
int tpg_fbm_upload_bed_snps(tpg_ctx* ctx, tpg_fbm* fbm, const uint8_t* host_snps, int64_t snp0, int64_t nsnps);
int tpg_fbm_to_host(tpg_ctx* ctx, const tpg_fbm* fbm, uint8_t* bytes);
void tpg_fbm_free(tpg_fbm* fbm);

/* ---- simple imputation (gt_impute_simple, R/gt_impute_simple.R:54-93 around bigsnpr::snp_fastImputeSimple) -----------
 * Per locus j, over the n individuals of the object being imputed: c0, c1, c2 = entries that are 0, 1, 2; t = c0 + c1 + c2,
 * s = c1 + 2 c2; an entry is missing when it is 3 (CODE_012[3] = NA).  Only missing entries change:
 *   TPG_IMPUTE_MODE    the most frequent of 0, 1, 2, on a tie the smaller genotype (which.max);
 *   TPG_IMPUTE_MEAN0   round(s / t), half to even as R's round(): 0 if 2 s <= t, 1 if 2 s < 3 t, else 2 (no floating point);
 *   TPG_IMPUTE_RANDOM  every missing entry on its own Binomial(2, s / (2 t)), a pure function of (seed, i, j), the 0-based
 *                      position of the entry in the object being imputed (store row / column for a store; kept row / kept
 *                      column for a view and for the selection of a streamed job) -- so it does not depend on block plan,
 *                      launch shape or device.  With M = tpg_mix64 of csrc/synth_common.h (the splitmix64 finaliser:
 *                      x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) *
 *                      0x94D049BB133111EB; x ^ x >> 31) and 64-bit unsigned arithmetic throughout:
 *                        key = M(seed ^ M(j));  h = M(key ^ M(i));  u1 = h >> 32;  u2 = h & 0xFFFFFFFF;
 *                        thr = (s << 31) / t;   v = (u1 < thr) + (u2 < thr).
 * A locus nobody is typed at (t = 0) stays missing under every method and is counted in the report; the PCA entry points
 * go on refusing it (TPG_ENUMERIC).
 * A store receives the fill v as byte 4 + v, which CODE_IMPUTE_PRED reads as v and which the raw-byte consumers
 * (increment_*_counts, code256 == NULL) go on treating as missing: the raw / imputed switch of R/gt_has_imputed.R:101-106.
 * A store byte above 3 means "already imputed, or not a CODE_012 store": TPG_EUNSUPPORTED ("object x is already imputed"),
 * store unchanged.  A .bed-form store (tpg_fbm_open_bed) has no byte to hold 4 + v: TPG_EUNSUPPORTED, use tpg_view_impute.
 * A view is imputed into a NEW view of the same geometry that holds v itself (no code 3 left except at t = 0 loci): what the
 * CODE_IMPUTE_PRED view of the imputed store would be.  `raw` is a view through code256 == NULL or CODE_012. */
#define TPG_IMPUTE_NONE 0
#define TPG_IMPUTE_MODE 1
#define TPG_IMPUTE_MEAN0 2
#define TPG_IMPUTE_RANDOM 3
typedef struct tpg_impute_report {
  int64_t imputed;          /* entries filled */
  int64_t loci_all_missing; /* loci left missing because nobody is typed at them */
} tpg_impute_report;
/* in place on a byte store; rep may be NULL */
int tpg_fbm_impute_simple(tpg_ctx* ctx, tpg_fbm* fbm, int method, uint64_t seed, tpg_impute_report* rep);
/* the same for a store that holds columns [col0, col0 + ncol) of a larger one (an FBM that is imputed block of columns by block
 * of columns: the R shim): `random` is keyed by col0 + the column, so the blocks together get the fill of one call */
int tpg_fbm_impute_simple_at(tpg_ctx* ctx, tpg_fbm* fbm, int64_t col0, int method, uint64_t seed, tpg_impute_report* rep);
int tpg_view_impute(tpg_ctx* ctx, const tpg_view* raw, int method, uint64_t seed, tpg_view** out, tpg_impute_report* rep);

/* The (rowInd, colInd) view every reference kernel receives, packed once:
 * rowInd NULL = all rows, colInd NULL = all columns. */
int tpg_view_create(tpg_ctx* ctx, const tpg_fbm* fbm, const int32_t* rowInd1, int64_t n,
                    const int32_t* colInd1, int64_t m, const double* code256, tpg_view** out);
/* two views of the same (rowInd, colInd) through two code tables, packed from ONE read of the FBM bytes: e.g. the raw
 * view (code256_a = NULL) for the pairwise statistics and the imputed view (CODE_IMPUTE_PRED) for the PCA of the same
 * gen_tibble (R/gt_has_imputed.R:101-106 flips the FBM's code256 between exactly these two) */
int tpg_view_create_pair(tpg_ctx* ctx, const tpg_fbm* fbm, const int32_t* rowInd1, int64_t n, const int32_t* colInd1,
                         int64_t m, const double* code256_a, const double* code256_b, tpg_view** out_a,
                         tpg_view** out_b);
/* The view of HOST FBM bytes (e.g. the columns a block of an R driver loop covers) without a store that outlives the call:
 * upload, pack, release.  One code table is known, so the bytes cross PCIe as 2 bits per genotype where table and bytes
 * allow it (every table entry below 16 a code, no byte >= 16: both true for CODE_012 / CODE_IMPUTE_PRED stores), as nibbles
 * or bytes otherwise; the result is the view tpg_fbm_from_host + tpg_view_create give. */
int tpg_view_create_from_host(tpg_ctx* ctx, const uint8_t* fbm_bytes, int64_t nrow, int64_t ncol, const int32_t* rowInd1, int64_t n,
                              const int32_t* colInd1, int64_t m, const double* code256, tpg_view** out);
void tpg_view_free(tpg_view* v);
int64_t tpg_view_n(const tpg_view* v);
int64_t tpg_view_m(const tpg_view* v);
/* unpack to one byte per genotype (0,1,2,3=NA), column-major n x m (tests) */
int tpg_view_unpack(tpg_ctx* ctx, const tpg_view* v, uint8_t* codes);

/* ---- per-locus sweeps --------------------------------------------------- */
/* genotype counts per locus: out is m x 4 int32 row-major {n0,n1,n2,nNA}
 * (the counts behind a4/a6/a11; also bigstatsr::big_counts, R/loci_missingness.R:109-122) */
int tpg_loci_counts(tpg_ctx* ctx, const tpg_view* v, int32_t* out);
/* genotype counts per individual over the view's loci: out is n x 4 int32 row-major {n0,n1,n2,nNA} */
int tpg_indiv_counts(tpg_ctx* ctx, const tpg_view* v, int32_t* out);
/* SURVEY.md §8f(2) "next" rows, same sweeps on the same counts:
 * gt_ind_hetero (src/gt_ind_hetero.cpp:11-42): out is the 2 x n integer matrix {n_het; n_na} (column-major);
 * gt_pi_diploid (src/gt_pi_diploid.cpp:7-38): pi[m];
 * gt_grouped_pi_diploid (src/gt_grouped_pi_diploid.cpp:7-42): pi and n, both m x G */
int tpg_gt_ind_hetero(tpg_ctx* ctx, const tpg_view* v, int32_t* out);
int tpg_gt_pi_diploid(tpg_ctx* ctx, const tpg_view* v, double* pi);
int tpg_gt_grouped_pi_diploid(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups, double* pi,
                              double* n);
/* genotype counts per locus x group, the 3 x ngroups table gt_grouped_hwe fills before each exact test
 * (src/hwe.cpp:238-250; the test on that table, without the download: tpg_gt_grouped_hwe below): out = three m x G int32
 * matrices (column-major), k = 0, 1, 2 alternate alleles */
int tpg_grouped_genotype_counts(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups,
                                int32_t* out);
/* ---- Hardy-Weinberg exact tests (loci_hwe, R/loci_hwe.R; the reference's .Call rows SNPHWE2_R, hwe_on_matrix,
 * gt_grouped_hwe) ----
 * For a table (hom1, het, hom2) of n individuals with r = 2 min(hom1, hom2) + het copies of the rarer allele, the
 * heterozygote count x runs over r mod 2, r mod 2 + 2, ..., r with w(x + 2) / w(x) = (r - x)(2n - r - x) / ((x + 2)(x + 1))
 * (Wigginton, Cutler, Abecasis 2005).  With eps = 2^-44, T = {x : w(x) < w(het)(1 + eps)} and ties = the members of T with
 * w(x) > w(het)(1 - eps): p = sum_T w / sum w; with midp (Graffelman, Moreno 2013) half of ties w(het) is taken off the
 * numerator.  n = 0 gives 1 (mid-p 0.5); a p below 1e-300 may come back as 0.  FP64 recurrence from the observed count,
 * within 8 max(n, 8) 2^-53 of the exact value (relative); tables of n < 2^26.  midp is 0 or 1.  The tests run on the
 * device behind the count sweeps: no count table crosses PCIe. */
/* p[count]; counts3 = 3 x count int32, column-major {hom1, het, hom2} per test (rows 1..3 of bigstatsr::big_counts, what
 * hwe_on_matrix takes); host or device memory both sides */
int tpg_hwe_exact_counts(tpg_ctx* ctx, const int32_t* counts3, int64_t count, int midp, double* p);
/* loci_hwe of an ungrouped object (R/loci_hwe.R:64-95: big_counts + hwe_on_matrix per block): p[m] */
int tpg_loci_hwe(tpg_ctx* ctx, const tpg_view* v, int midp, double* p);
/* gt_grouped_hwe (src/hwe.cpp:220-253): p is m x G column-major; a group nobody belongs to or is typed in gives the
 * n = 0 value */
int tpg_gt_grouped_hwe(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups, int midp, double* p);

/* ---- LD clumping (loci_ld_clump, R/loci_ld_clump.R:84-184 around bigsnpr::snp_clumping) --------------------------------
 * bigsnpr's function is not part of the reference checkout, so the definition below is this project's own.
 * Input: a view of n individuals x m loci in which every code is 0, 1 or 2.  A missing genotype: TPG_ENUMERIC, no output
 *   written (the reference stops on it; impute the view first).  n >= 2^22: TPG_EUNSUPPORTED.
 * Window: hi[m], int64, 0-based inclusive, hi[j] >= j, hi[j] < m, non-decreasing in j (anything else: TPG_EINVAL).  Loci
 *   j < k are NEIGHBOURS iff k <= hi[j]; the host layers derive hi from (chromosome, position, size).
 * Edge: with the int64 sums Sx = sum x, Sxx = sum x^2 over the individuals of a locus, Sxy = sum x_j x_k,
 *   num = n Sxy - Sx_j Sx_k and d_j = n Sxx_j - Sx_j^2, neighbours j and k are LINKED iff
 *       (double)num * (double)num > thr_r2 * ((double)d_j * (double)d_k)
 *   evaluated in exactly this order in IEEE double, no FMA contraction (r^2 > thr_r2 without a division).  A monomorphic
 *   locus (d = 0) is linked to nothing.  thr_r2 in [0, 1].
 * Priority: the larger key is the more important locus: the caller's S (m doubles; a NaN: TPG_EINVAL), or with S == NULL
 *   the minor allele count min(Sx, 2 n - Sx) as an integer (the order of the MAF, without rounding).  Ties go to the
 *   smaller locus index (R's stable order(S, decreasing = TRUE)).
 * Exclusion: exclude (m bytes, may be NULL): an excluded locus is never kept and removes nobody.
 * Result: the sequential greedy set -- walk the loci by priority; a locus still standing is kept and every locus linked
 *   to it falls.  Equivalently the unique set in which a non-excluded locus is kept iff no linked locus of higher priority
 *   is kept.  keep[m] bytes (0 / 1); deterministic, independent of blocking and launch geometry.
 * hi, S and exclude may be host or device memory, bits and keep too; an output must not overlap an input. */
/* the link relation as a bit band: row j = stride_words uint32, bit b of the row (bit b & 31 of word b >> 5) <-> locus
 * j + 1 + b; stride_words >= ceil(max_j(hi[j] - j) / 32); bits outside the window are 0.  *n_links (host, may be NULL) =
 * number of linked pairs. */
int tpg_ld_band_links(tpg_ctx* ctx, const tpg_view* v, const int64_t* hi, double thr_r2, uint32_t* bits,
                      int64_t stride_words, int64_t* n_links);
typedef struct tpg_ld_report {
  int64_t links;       /* linked pairs found */
  int64_t kept;        /* loci kept */
  int64_t rounds;      /* parallel resolution rounds run (at most 32; every round decides at least one locus) */
  int64_t finish_loci; /* loci the bounded rounds left undecided: decided by one wave walking them in priority order */
  int64_t band_bytes;  /* HBM held by the band (both orientations) during the call */
} tpg_ld_report;
/* band, priority order and greedy resolution on the device: only keep comes down (no r^2 value and no part of the band
 * crosses PCIe).  report may be NULL. */
int tpg_ld_clump(tpg_ctx* ctx, const tpg_view* v, const int64_t* hi, double thr_r2, const double* S,
                 const uint8_t* exclude, uint8_t* keep, tpg_ld_report* report);

/* ---- LD-kNN imputation (gt_impute_knn; the method of LinkImpute's LD-kNNi, Money et al. 2015, stated here in integers) ------
 * The reference's second imputation, gt_impute_xgboost, fits boosted trees per locus; this is the published method that does
 * the same job -- a missing genotype is filled from the individuals that look alike at the loci in strongest LD -- and it can
 * be pinned to bits.  The definition is this project's own.
 * Inputs: a raw view v (n individuals, m loci, codes 0 / 1 / 2 / 3 = missing; code256 == NULL or CODE_012); the window hi[m]
 *   exactly as "LD clumping" takes it (for k > j locus k is a neighbour of j iff k <= hi[j]; for k < j iff j <= hi[k]); l, k and
 *   min_r2.  1 <= l <= 32, k >= 1, min_r2 >= 0 and finite, n < 2^22, a view with a locus-tiled layout: anything else is
 *   TPG_EINVAL with nothing written.
 * Step 1, LD neighbours, on w = tpg_view_impute(v, TPG_IMPUTE_MODE), the fill the PCA uses (a locus typed nowhere stays
 *   missing there and is never a candidate).  From w's counts, as LD clumping forms them: Sx, Sxx, d = n Sxx - Sx^2 held as a
 *   double (exact below 2^46).  For a pair of loci num = n Sxy - Sx_j Sx_k in int64, dn = (double)num and
 *       r2 = (dn * dn) / (d_j * d_k)
 *   -- three IEEE double operations in this order, no FMA contraction.  The CANDIDATES of j are its neighbours k with d_j > 0,
 *   d_k > 0 and r2 > min_r2; nbr(j, 0 .. l_j - 1) are the candidates of largest r2, ties to the smaller |k - j|, then to the
 *   smaller k; l_j = min(l, number of candidates).  Unused slots hold nbr = -1 and r2 = 0.
 * Step 2, distances, on v itself: D_j(a, b) = sum_t c(v[a, q_t], v[b, q_t]) over q_t = nbr(j, t), with c(x, y) = |x - y| when
 *   both are typed and 1 otherwise; 0 <= D <= 2 l_j <= 64.
 * Step 3, the vote, for every (i, j) with v[i, j] == 3: hist[dist][g] counts the individuals b with v[b, j] = g in {0, 1, 2}
 *   and D_j(i, b) = dist (i is missing at j and never counts itself); T = sum hist.  T = 0: the entry stays 3.  Otherwise
 *   d* = the smallest dist with sum_{dist' <= dist} sum_g hist[dist'][g] >= min(k, T) -- the whole boundary distance takes
 *   part, no tie is broken by index, so the result depends on no order -- s_g = sum_{dist <= d*} hist[dist][g] *
 *   ((1 << 24) / (1 + dist)) with integer division in int64, and the fill is the g of largest s_g, the smaller g on a tie.
 *   With l_j = 0 every distance is 0 and the fill is the locus's mode over v (tpg_view_impute's TPG_IMPUTE_MODE).
 * Outputs: a NEW view of v's geometry that holds the fills (what tpg_view_impute returns for the simple methods);
 *   rep = {imputed, loci_all_missing}; rep_knn (int64[2], may be NULL) = {entries_left: entries that stayed 3 (T = 0),
 *   loci_without_neighbours: loci with a missing entry and l_j = 0}.
 * Store form: a byte store (the view is the whole store, raw bytes) receives byte 4 + fill wherever it holds 3, as "simple
 *   imputation" specifies; a byte above 3 anywhere: TPG_EUNSUPPORTED ("object x is already imputed") before anything is
 *   written; a .bed-form store: TPG_EUNSUPPORTED, use the view form.
 * Error estimate (the counterpart of xgboost's imputed_errors): train = tpg_view_holdout_fraction(v, fraction, seed) is
 *   imputed with the same hi, l, k, min_r2; tpg_view_impute_errors counts per locus the entries typed in `full` and missing
 *   in `train`, and how many of them `filled` has wrong (an entry left at 3 is wrong): per_locus = m x 2 int64 row-major
 *   {held, wrong}, totals = their two sums (host memory).  Nothing proportional to n m leaves the device.
 * flags: 0, or for the tests TPG_KNN_PROFILES_GLOBAL (the vote reads the profiles from global scratch, as it does above
 *   11 520 individuals where LDS no longer holds them) and TPG_KNN_SMALL_CHUNKS (the band of Sxy values is walked in chunks of a
 *   few KiB instead of 256 MiB); neither changes a bit of any result.
 * hi, nbr, r2 and per_locus may be host or device memory. */
#define TPG_KNN_PROFILES_GLOBAL 1
#define TPG_KNN_SMALL_CHUNKS 2
/* step 1 alone on a view in which every locus is typed everywhere or nowhere (a locus typed in part: TPG_ENUMERIC):
 * nbr = m x l int32 and r2 = m x l doubles, row-major */
int tpg_ld_top_neighbours(tpg_ctx* ctx, const tpg_view* v, const int64_t* hi, int l, double min_r2, int flags, int32_t* nbr,
                          double* r2);
int tpg_view_impute_knn(tpg_ctx* ctx, const tpg_view* raw, const int64_t* hi, int l, int k, double min_r2, int flags,
                        tpg_view** out, tpg_impute_report* rep, int64_t* rep_knn);
int tpg_fbm_impute_knn(tpg_ctx* ctx, tpg_fbm* fbm, const int64_t* hi, int l, int k, double min_r2, int flags,
                       tpg_impute_report* rep, int64_t* rep_knn);
int tpg_view_impute_errors(tpg_ctx* ctx, const tpg_view* full, const tpg_view* train, const tpg_view* filled,
                           int64_t* per_locus, int64_t* totals);
/* the device memory a tpg_view_impute_knn call plans beyond the raw view: the mode-filled view and the result, one chunk of
 * the band (at most 256 MiB, or the 32 loci a chunk cannot go below), nbr and r2, the per-locus tables, and above 11 520
 * individuals the profiles of two workgroups per CU (256 CUs assumed) */
size_t tpg_knn_impute_scratch_bytes(int64_t n, int64_t m, int64_t width, int l);

/* ---- LD statistics (loci_ld_score, ld_decay, ld_region_r2: how much LD there is inside the window; no counterpart in the
 * reference, whose LD functions only search the window) ---------------------------------------------------------------------
 * The definition is this project's own.  Everything below is integers but r2 itself.
 * Input: a view of n individuals x m loci in which every code is 0, 1 or 2.  A missing genotype: TPG_ENUMERIC (impute the view
 *   first).  n >= 2^22: TPG_EUNSUPPORTED.
 * Window: hi[m] exactly as "LD clumping" takes it and checks it.  The PAIRS are all (j, k) with j < k <= hi[j]; the PARTNERS of
 *   locus j are the k > j with k <= hi[j] and the k < j with j <= hi[k], as in "LD-kNN imputation".
 *   sum_j (hi[j] - j) >= 2^33: TPG_EUNSUPPORTED (so that no sum below passes 2^63).
 * r2 of a pair: Sx, Sxx and d = n Sxx - Sx^2 from the counts, d held as a double; num = n Sxy - Sx_j Sx_k in int64,
 *   dn = (double)num and
 *       r2 = (dn * dn) / (d_j * d_k)
 *   -- three IEEE double operations in this order, no FMA contraction: the bits tpg_ld_top_neighbours returns for the pair.
 *   A pair is VALID iff d_j > 0 and d_k > 0: a monomorphic locus has no valid pair.
 * Fixed point: q = (uint64) floor(r2 * 2^30 + 0.5).  Every sum of r2 below is a uint64 sum of q, which depends on no order; the
 *   rounding is at most 2^-31 per pair, far below the sampling error 1 / n of an r2.  No sum reaches 2^63, so the prototypes
 *   spell the arrays int64_t like every other 64-bit output of this header: the bits are those of the uint64 sum.
 * Per locus (score_q and n_partners are NULL together): score_q[m], uint64 = sum of q over the valid pairs of j with its
 *   partners on both sides; n_partners[m], int32 = the number of those pairs.  The self term is not included.
 * Decay (bin_pairs, bin_sum_q and bin_sum_dist are NULL together; bin_size and nbins are read only with them): pos is
 *   int64[m], or NULL.  dist = pos[k] - pos[j], or k - j without pos.  pos[j + 1] < pos[j] for neighbours j, j + 1, or a
 *   |pos| of 2^61 or more: TPG_EINVAL (a decrease across a window border is allowed).  bin_size >= 1 and
 *   1 <= nbins <= 4096, else TPG_EINVAL.  bin = dist / bin_size by integer division; over the valid pairs with bin < nbins:
 *   bin_pairs[nbins] int64 their number, bin_sum_q[nbins] uint64 the sum of q, bin_sum_dist[nbins] int64 the sum of dist
 *   (distances so large that this sum could pass 2^63: TPG_EUNSUPPORTED).  Valid pairs with bin >= nbins are counted in
 *   pairs_beyond.
 * A NULL group does not change a bit of the other group.  hi, pos and all outputs may be host or device memory.  On any error
 *   nothing is written. */
typedef struct tpg_ldstat_report {
  int64_t pairs;        /* sum_j (hi[j] - j) */
  int64_t pairs_valid;  /* pairs of two polymorphic loci */
  int64_t pairs_beyond; /* valid pairs behind the last bin (0 without the decay group) */
  int64_t band_tiles;   /* 32 x 32 tiles of Sxy the call contracted */
} tpg_ldstat_report;
/* one call, one pass over the band.  report (host memory, may be NULL): a tpg_ldstat_report, taken as the four int64_t it
 * consists of */
int tpg_ld_stats(tpg_ctx* ctx, const tpg_view* v, const int64_t* hi, const int64_t* pos, int64_t bin_size, int nbins,
                 int64_t* score_q, int32_t* n_partners, int64_t* bin_pairs, int64_t* bin_sum_q, int64_t* bin_sum_dist,
                 int64_t* report);
/* the values of a region, for heatmaps, tests and small panels: r2[(j - j0) * stride + b] = r2 of the pair (j, j + 1 + b) for
 * j0 <= j < j1 and b < hi[j] - j; NaN outside the window and for a pair that is not valid.  0 <= j0 < j1 <= m,
 * stride >= max(1, hi[j] - j) over the region and (j1 - j0) * stride <= 2^26, else TPG_EINVAL. */
int tpg_ld_band_r2(tpg_ctx* ctx, const tpg_view* v, const int64_t* hi, int64_t j0, int64_t j1, double* r2, int64_t stride);

/* ---- Runs of homozygosity (windows_indiv_roh, R/windows_indiv_roh.R:65-150 around detectRUNS::slidingRuns) ---------------
 * detectRUNS is not part of the reference checkout, so the definition below is this project's own.  It is
 * stated in integers; the two places where a double appears are spelled out.
 * Input: a view of n individuals x m loci (codes 0, 1, 2, and 3 = missing), chrom (int32[m]) and pos (int64[m]) of its loci,
 *   host or device memory, and the parameters below.  window_size W outside [1, 512], threshold outside [0, 1], a negative
 *   max_*_window: TPG_EINVAL.
 * Per individual:
 *   1. opp[j] = (code == 1); with heterozygosity != 0 (runs of heterozygosity) opp[j] = (code is 0 or 2).  miss[j] = (code == 3).
 *   2. brk[j], 0 <= j < m - 1, = chrom[j] != chrom[j + 1] || pos[j + 1] - pos[j] > max_gap.  Only neighbours are compared.  A
 *      position that decreases inside a chromosome: TPG_EINVAL ("not ordered"); equal positions are allowed.
 *   3. Window w covers the loci [w, w + W), 0 <= w <= m - W.  It is OK iff sum opp <= max_opp_window, sum miss <=
 *      max_miss_window and no brk[j] for j in [w, w + W - 2]: a window never spans a chromosome boundary or a gap.  m < W:
 *      no window, no run (TPG_OK).
 *   4. The windows that contain locus j start in [max(0, j - W + 1), min(j, m - W)]: `cover` of them (1 .. W), `hits` of them
 *      OK.  need[c] = max(1, ceil(threshold * (double)c)), c = 1 .. W: one IEEE double multiplication and one ceil, on the
 *      host.  Locus j is IN A RUN iff hits >= need[cover] (the device compares integers).
 *   5. A SEGMENT is a maximal stretch [a, b] of in-run loci with no brk between neighbours inside it; nSNP = b - a + 1,
 *      length = pos[b] - pos[a], nOpp / nMiss = sum of opp / miss over [a, b].  It is a RUN iff nSNP >= min_snp, length >=
 *      min_length_bps, (double)nSNP * 1000.0 >= min_density * (double)length (one multiplication on either side, no
 *      division, no FMA), and nOpp <= max_opp_run, nMiss <= max_miss_run where those are >= 0.
 * Output: all runs, ordered by (individual, first locus); deterministic, independent of chunking and launch geometry. */
typedef struct tpg_roh_params {
  int32_t window_size;     /* W */
  double threshold;        /* share of the windows over a locus that must be OK */
  int32_t min_snp;
  int32_t heterozygosity;  /* 0: runs of homozygosity, otherwise runs of heterozygosity */
  int32_t max_opp_window;
  int32_t max_miss_window;
  int64_t max_gap;         /* bp */
  int64_t min_length_bps;
  double min_density;      /* SNPs per kbp */
  int32_t max_opp_run;     /* < 0: no limit */
  int32_t max_miss_run;    /* < 0: no limit */
} tpg_roh_params;
typedef struct tpg_roh tpg_roh; /* the runs of one call, owned by the library (device memory) */
/* loci per chunk of the status stage (a chunk is cut with a halo of W - 1 loci on either side; results do not depend on it) */
#define TPG_ROH_CHUNK_LOCI 2048
int64_t tpg_roh_chunk_loci(void);
/* step 4 alone: row i = stride_words uint32, bit j & 31 of word j >> 5 <-> locus j of individual i is in a run;
 * stride_words >= ceil(m / 32); unused words and padding bits are 0.  bits may be host or device memory. */
int tpg_roh_snp_status(tpg_ctx* ctx, const tpg_view* v, const int32_t* chrom, const int64_t* pos, const tpg_roh_params* params,
                       uint32_t* bits, int64_t stride_words);
/* steps 1 - 5 on the device: two counts (segments, runs) cross to the host, nothing proportional to n m does */
int tpg_roh_detect(tpg_ctx* ctx, const tpg_view* v, const int32_t* chrom, const int64_t* pos, const tpg_roh_params* params,
                   tpg_roh** out);
int64_t tpg_roh_count(const tpg_roh* r);
/* tpg_roh_count entries each, 0-based, any may be NULL; host or device memory */
int tpg_roh_fetch(tpg_ctx* ctx, const tpg_roh* r, int32_t* indiv0, int64_t* first0, int64_t* last0, int32_t* n_opp,
                  int32_t* n_miss);
/* per individual (n entries each): number of runs, sum of their lengths in bp */
int tpg_roh_indiv_summary(tpg_ctx* ctx, const tpg_roh* r, int64_t* n_runs, int64_t* sum_length_bps);
/* per locus (m entries): individuals with that locus inside a run (a difference array and a scan on the device) */
int tpg_roh_locus_counts(tpg_ctx* ctx, const tpg_roh* r, int32_t* counts);
void tpg_roh_free(tpg_roh* r);

/* ---- IBD segments (where two individuals share DNA: the stretches over which a pair shares at least one haplotype, IBD1, or
 * both, IBD2; the output of `king --ibdseg` / IBIS; no counterpart in the reference) -----------------------------------------
 * The definition is this project's own, recalled from Seidman et al. 2020 (IBIS) and KING, not pinned.
 * Everything is an integer.
 * Input: a view of n individuals x m loci (codes 0, 1, 2, and 3 = missing), chrom (int32[m]) and pos (int64[m]) of its loci,
 *   host or device memory -- pos in any ordered integer unit: bp, or cM scaled to integers -- and the scalars below.
 * Per unordered pair (a, b), a < b, and per locus j: typed[j] = both codes != 3.  bad[j] for kind = 1: typed and the codes are
 *   {0, 2} in either order (opposite homozygotes cannot share a haplotype); for kind = 2: typed and the codes differ (they
 *   cannot share both).  A missing genotype is neither bad nor typed.
 *   1. brk[j], 0 <= j < m - 1, exactly as step 2 of "Runs of homozygosity": a chromosome change, or pos[j + 1] - pos[j] >
 *      max_gap.  A position that decreases inside a chromosome: TPG_EINVAL ("not ordered"); equal positions are allowed.
 *   2. A CLEAN STRETCH is a maximal [s, e] with no bad locus in it and no brk[j] for s <= j < e; its count c = the typed loci
 *      in it.
 *   3. Bridging (bridge_min_snp > 0): two consecutive clean stretches [s1, e1], [s2, e2] are JOINED iff s2 = e1 + 2 (exactly
 *      one bad locus lies between them), brk[e1] and brk[e1 + 1] are both false, c1 >= bridge_min_snp and c2 >=
 *      bridge_min_snp.  A joint depends on its two stretches only, so the order of evaluation does not matter.  A SEGMENT is
 *      a maximal chain of joined stretches [first, last]; n_err = its bridged bad loci, n_typed = the typed loci in
 *      [first, last].  With bridge_min_snp = 0 every clean stretch is its own segment and n_err = 0.
 *   4. A segment is REPORTED iff n_typed >= min_snp, pos[last] - pos[first] >= min_length, and n_err <= max_err where
 *      max_err >= 0 (a negative max_err: no limit).
 * TPG_EINVAL: min_snp < 1 (with min_snp >= 1 a pair with a wholly missing individual reports nothing), min_length < 0,
 *   max_gap < 0, bridge_min_snp < 0, kind not 1 or 2, cap < 0, cap > 0 with a NULL segment array.  m >= 2^31 - 64, or more
 *   than 65536 individuals (2^31 pairs): TPG_EUNSUPPORTED.  n = 1: TPG_OK, no segment.
 * Output: the reported segments of all pairs, ordered by (a, b, first), 0-based; per pair their number and the sum of their
 *   lengths pos[last] - pos[first].  Deterministic, independent of chunking, tile shape and launch geometry. */
/* loci per chunk of the scan (results do not depend on it) */
#define TPG_IBD_CHUNK_LOCI 1024
int64_t tpg_ibd_chunk_loci(void);
/* the sum over the break-free regions of pos[last] - pos[first]: what a pair that shares everything adds up to.  Host only:
 * chrom and pos are host memory.  m < 1, max_gap < 0, not ordered: TPG_EINVAL */
int tpg_ibd_genome_length(const int32_t* chrom, const int64_t* pos, int64_t m, int64_t max_gap, int64_t* length);
/* *count = the number of reported segments, whatever cap is.  count <= cap: the six arrays hold count entries each in the
 * stated order; otherwise they are not written and the caller calls again (cap = 0 with NULL arrays is the counting call).
 * pair_n_seg (int32) and pair_sum_length (int64): n x n, symmetric, zero diagonal; either may be NULL; complete whatever cap
 * is.  Every output may be host or device memory.  On any error the caller's outputs are untouched. */
int tpg_ibd_segments(tpg_ctx* ctx, const tpg_view* v, const int32_t* chrom, const int64_t* pos, int kind, int64_t min_snp,
                     int64_t min_length, int64_t max_gap, int64_t bridge_min_snp, int64_t max_err, int64_t cap, int32_t* ind_a,
                     int32_t* ind_b, int64_t* first0, int64_t* last0, int32_t* n_typed, int32_t* n_err, int64_t* count,
                     int32_t* pair_n_seg, int64_t* pair_sum_length);

/* ---- Tajima's D (pop_tajimas_d, R/pop_tajimas_d.R:151-166; windows_pop_tajimas_d, R/windows_pop_tajimas_d.R:69-102 over
 * R/windows_stats_generic.R:113-176; pi as src/gt_pi_diploid.cpp:22-35 and src/gt_grouped_pi_diploid.cpp:24-38) -----------
 * Group g has N_g individuals in the view and n = 2 N_g sampled alleles: the group's size, not its typed count.  J is a set
 * of loci (the whole view, or a window).
 * pi:    pi(j, g) = x (v - x) / (v (v - 1) / 2), x = alternate alleles over the typed individuals of g at locus j, v = twice
 *        their number; evaluated in exactly this order in IEEE double (no FMA contraction); v = 0 gives NaN.
 * seg:   S = #{j in J : 0 < pi < 1}.  A NaN is not counted; pi = 1 (v = 2, x = 1) is not segregating.
 * k_hat: the sum of pi over J, without a NaN guard: one locus at which the group has no typed individual makes k_hat, and D,
 *        NaN.
 * D:     (k_hat - S / a1) / sqrt(e1 S + e2 S (S - 1)) with a1 = sum_{i<n} 1/i, a2 = sum_{i<n} 1/i^2 (both summed in ascending
 *        order of i), e1 = ((n + 1) / (3 (n - 1)) - 1 / a1) / a1, e2 = (2 (n^2 + n + 3) / (9 n (n - 1)) - (n + 2) / (n a1) +
 *        a2 / a1^2) / (a1^2 + a2), all in double on the host.  Plain IEEE arithmetic, no special case: S = 0 gives NaN (0 / 0)
 *        or +Inf (k_hat / 0), N_g = 1 gives e1 = e2 = 0 exactly.  A group nobody belongs to (the reference cannot have one):
 *        D and k_hat NaN, seg 0.
 * Windows: window w covers the loci lo[w] .. hi[w]-1 with a pad_na flag, the contract of tpg_window_stats.  n_loci = the
 *        number of non-NaN pi in the window, -1 for a pad_na window.  D is NaN where pad_na is set or n_loci < min_loci; seg
 *        and k_hat are reported all the same (0 and NaN for a pad_na window).
 * Determinism: a result depends on (lo, hi, group) alone -- not on nw, on the window's place in the list or on launch
 *        geometry -- and two calls give the same bits.  k_hat is within L 2^-52 k_hat of the exact sum of the L doubles.
 * Diploid only (stopifnot_diploid): ploidy may be NULL; anything other than 2 in it is TPG_EINVAL.
 * groupIds0 == NULL: one group of everybody.  Nothing proportional to m crosses PCIe. */
/* host only, no context, no GPU: D from the additive pieces, so that a caller can add seg and k_hat over shards or blocks.
 * n_alleles < 2 or seg < 0: TPG_EINVAL */
int tpg_tajimas_d_from_sums(int64_t n_alleles, int64_t seg, double k_hat, double* d);
/* loci per partial sum of the whole-view reduction (results do not depend on it) */
#define TPG_TAJIMA_CHUNK_LOCI 1024
int64_t tpg_tajima_chunk_loci(void);
/* whole view: d, seg, k_hat have ngroups entries each, host memory (seg, k_hat may be NULL) */
int tpg_pop_tajimas_d(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups, const double* ploidy, double* d,
                      int64_t* seg, double* k_hat);
/* nw x ngroups column-major each; seg, k_hat, n_loci may be NULL; lo, hi, pad_na (may be NULL) and the outputs host or device
 * memory.  A window outside [0, m], lo > hi, min_loci < 1, nw > TPG_TAJIMA_MAX_WINDOWS (one workgroup per window: split the
 * list): TPG_EINVAL; nw == 0: TPG_OK, nothing written */
#define TPG_TAJIMA_MAX_WINDOWS 16777215
int tpg_windows_pop_tajimas_d(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups, const double* ploidy,
                              const int64_t* lo, const int64_t* hi, const uint8_t* pad_na, int64_t nw, int min_loci, double* d,
                              int64_t* seg, double* k_hat, int32_t* n_loci);

/* ---- f2 blocks (gt_extract_f2, R/gt_extract_f2.R: gt_to_aftable + admixtools::afs_to_f2_blocks; admixtools is not part of
 * the reference's sources, so the arithmetic is defined HERE; "(recalled)" marks what follows admixtools from memory) -------
 * A view of N individuals in G groups; ploidy NULL = all 2, 1 = pseudohaploid as tpg_grouped_alt_freq_dip_pseudo treats it.
 * Per locus j and group g, formed exactly as tpg_grouped_alt_freq_dip_pseudo forms them:
 *   c(j,g) = valid alleles, p(j,g) = alt alleles / c.
 *   t(j,g) = [c > 0] ("typed").
 *   e(j,g) = p (1 - p) / max(1, c - 1) if apply_corr, else 0; evaluated as (p * (1 - p)) / max(1, c - 1) in IEEE double, no FMA
 *            contraction (recalled: pmax(1, counts - 1); NOT the n - 1 of the Hudson numerator of tpg_pairwise_pop_fst).
 * Locus filters, evaluated on the device from the G values of the locus (discard_from_aftable, recalled):
 *   maxmiss: drop the locus if (double)#{g : !t} / (double)G > maxmiss.
 *   minmaf / maxmaf: f = (sum of p over the typed groups, added in ascending g) / #typed; maf = min(f, 1 - f); drop the locus
 *            if maf < minmaf or maf > maxmaf.  A locus with no typed group is dropped.
 *   minac2 in {0, 1}: with 1, drop the locus if any group has c < 2.  (admixtools' experimental minac2 = 2: TPG_EINVAL.)
 *   keep:    uint8[m], host or device memory, may be NULL: the caller's own mask (0 drops the locus).  Transitions,
 *            transversions and outpop are filters on the locus table and stay with the caller.
 *   poly(j) = the p of the typed groups are not all equal (cpp_is_polymorphic, recalled).
 *   poly_only: bit 0 (TPG_F2_POLY_F2, default on) applies poly to f2 and cnt, bit 1 (TPG_F2_POLY_AP) to ap and ap_cnt.
 * Blocks: block b covers the loci lo[b] .. hi[b]-1, the contract of tpg_window_stats: a block may be empty, blocks need not be
 *   disjoint; lo > hi or a block outside [0, m]: TPG_EINVAL; nb == 0: TPG_OK, nothing written.
 * Outputs: G x G x nb each, column-major with g1 fastest; any may be NULL; host or device memory.
 *   cnt    (int32)  #{j in b : kept for f2, t(j,g1), t(j,g2)}
 *   f2     (double) (1 / cnt) sum over those loci of [(p1 - p2)^2 - e1 - e2]; NaN where cnt = 0; for g1 == g2 exactly +0.0
 *                   where cnt > 0 (so that an f4 with a repeated population reduces to f3)
 *   ap_cnt, ap      the same for p1 p2 over the loci kept for ap; the diagonal of ap is the mean of p^2
 *   n_kept (int64[nb]) loci of the block that passed the filters, before poly
 *   A group nobody belongs to has cnt 0 and NaN in its row and column.
 * The sums are formed as masked matrix products over the block's loci, so a value is within
 *   (4 L + 16) 2^-52 (absolute, L = hi - lo) of the exact rational value of the definition; cnt, ap_cnt and n_kept are exact.
 * Determinism: a cell depends on (lo, hi, g1, g2) and the filter arguments alone -- not on nb, on the block's place in the
 *   list or on launch geometry -- and two calls give the same bits; f2 and ap are symmetric bit for bit.  No atomics.
 * Limits: ngroups > TPG_F2_MAX_GROUPS or nb > TPG_F2_MAX_BLOCKS: TPG_EINVAL (split the list). */
#define TPG_F2_POLY_F2 1
#define TPG_F2_POLY_AP 2
#define TPG_F2_MAX_GROUPS 4096
#define TPG_F2_MAX_BLOCKS 16777215
typedef struct tpg_f2_params {
  double maxmiss;       /* 0 */
  double minmaf;        /* 0 */
  double maxmaf;        /* 0.5 */
  int32_t minac2;       /* 0 */
  int32_t poly_only;    /* TPG_F2_POLY_F2 */
  int32_t apply_corr;   /* 1 */
  const uint8_t* keep;  /* NULL */
} tpg_f2_params;
/* the reference's defaults (the comments above) */
int tpg_f2_params_default(tpg_f2_params* p);
/* loci a workgroup stages at a time, in ascending order from lo[b] (results do not depend on it; the tests put block lengths
 * around it) */
#define TPG_F2_CHUNK_LOCI 16
int64_t tpg_f2_chunk_loci(void);
/* groupIds0 == NULL: one group of everybody; params == NULL: the defaults.  Nothing proportional to m leaves the device. */
int tpg_f2_blocks(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups, const double* ploidy,
                  const tpg_f2_params* params, const int64_t* lo, const int64_t* hi, int64_t nb, double* f2, int32_t* cnt,
                  double* ap, int32_t* ap_cnt, int64_t* n_kept);
/* host only, no context, no GPU: f4 (and f3) with the weighted delete-one block jackknife of Busing et al. 1999 (recalled:
 * what admixtools uses) from f2 (G x G x nb as above, host memory) and block_len[nb] (n_kept).  quads0 = 4 nq 0-based group
 * indices (A, B, C, D) per quadruple; f3(C; A, B) is the quadruple (C, A, C, B).  For one quadruple:
 *   theta_b = 0.5 * (f2[A,D,b] + f2[B,C,b] - f2[A,C,b] - f2[B,D,b])      (added in this order)
 *   blocks with theta_b NaN or block_len[b] <= 0 are left out; n_used = g = the blocks used; n_b = (double)block_len[b]
 *   n = sum n_b;  theta = (sum n_b theta_b) / n;  theta_(-b) = (n theta - n_b theta_b) / (n - n_b);  h_b = n / n_b
 *   est = g theta - sum (1 - n_b / n) theta_(-b)
 *   tau_b = h_b theta - (h_b - 1) theta_(-b);  se = sqrt((1 / g) sum ((tau_b - est)^2 / (h_b - 1)))
 * every sum in ascending b, in plain double, in the order written, no FMA contraction.  g < 2: est = theta (NaN if g = 0),
 * se = NaN.  est, se (double[nq]) and n_used (int32[nq]) may each be NULL.  An index outside [0, G): TPG_EINVAL. */
int tpg_f4_jackknife(const double* f2, int G, int64_t nb, const int64_t* block_len, const int32_t* quads0, int64_t nq,
                     double* est, double* se, int32_t* n_used);

/* ---- site frequency spectra (pop_sfs, pairwise_pop_jsfs; the reference has no SFS code and nothing pins it: the arithmetic
 * is defined HERE, recalled, not pinned, from Marth et al. 2004 (the hypergeometric projection of a sample with missing data)
 * and Gutenkunst et al. 2009 (dadi's projection and folding conventions)) -------------------------------------------------
 * A view of N individuals in G groups, diploid only as for Tajima's D: ploidy may be NULL; anything other than 2 in it is
 * TPG_EINVAL.  groupIds0 == NULL: one group of everybody.  A group nobody belongs to: TPG_EINVAL.
 * Per locus j and group g:
 *   v(j,g) = twice the typed individuals of g at j;  x(j,g) = alternate alleles among them.
 *   flip:  uint8[m], host or device memory, may be NULL: where flip[j] != 0, x is replaced by v - x (the counted allele is
 *          then the reference allele: how a caller supplies ancestral states).
 *   keep:  uint8[m], host or device memory, may be NULL: 0 drops the locus everywhere.
 * Projection size: proj (int32[G], host memory, may be NULL = all 0); n_g = proj[g] in [1, 2 N_g], 0 means 2 N_g; anything
 *   else: TPG_EINVAL.  Offsets o_g = sum_{g' < g} (n_g' + 1), W = o_G; W > TPG_SFS_MAX_WIDTH: TPG_EINVAL.
 * Usability: t(j,g) = [keep[j] and v(j,g) >= n_g]: a locus typed at fewer than n_g alleles in g is not usable for g.
 * Weights: h(j,g,k) = C(x,k) C(v - x, n_g - k) / C(v, n_g), k = 0 .. n_g: the hypergeometric probability that a sample of n_g of
 *   the v typed alleles holds k counted ones.  Outside max(0, n_g - (v - x)) <= k <= min(n_g, x) the weight is the exact double
 *   +0.0; where v = n_g the row is exactly the indicator of k = x (1.0 there, no rounding).  The evaluation is pinned in
 *   csrc/host/host_sfs.h (the same text runs on the device and on the host, without FMA contraction): a recurrence outwards
 *   from the mode, normalised by the sum of the support added in ascending k.  With u = 2^-53, an entry whose exact value is at
 *   least 2^-1000 is within (9 n_g + 4) u of it, relatively (the header counts the roundings); a smaller one is a non-negative
 *   double below 2^-999, possibly +0.0, without a relative bound (the recurrence may have passed through subnormal values).
 * Blocks: block b covers the loci lo[b] .. hi[b]-1, the contract of tpg_window_stats and tpg_f2_blocks: a block may be empty,
 *   blocks need not be disjoint; lo > hi or a block outside [0, m]: TPG_EINVAL; nb == 0: TPG_OK, nothing written; nb >
 *   TPG_SFS_MAX_BLOCKS: TPG_EINVAL (split the list).  The whole view is the block (0, m).
 * Outputs, each may be NULL, host or device memory:
 *   sfs     (double, W x nb, column-major)       sfs[o_g + k, b] = sum_{j in b} t(j,g) h(j,g,k)
 *   n_used1 (int64, G x nb)                      sum_{j in b} t(j,g)
 *   jsfs    (double, W x W x nb, column-major)   J[o_g1 + a, o_g2 + c, b] = sum_{j in b} t(j,g1) t(j,g2) h(j,g1,a) h(j,g2,c)
 *           for ALL g1, g2: block (g1, g2) is the joint spectrum of the pair over the loci usable in both; the diagonal blocks
 *           hold the same sum with g1 = g2 (defined, though not a spectrum).  J is symmetric bit for bit.
 *   n_used2 (int64, G x G x nb)                  sum_{j in b} t(j,g1) t(j,g2)
 * Accuracy: the integer outputs are exact.  Every term of sfs and jsfs is non-negative and the sums run on the FP64 matrix
 *   cores as chains over the block's loci, cut into tpg_sfs_segments(hi - lo, W) <= 64 partial sums that are added in ascending
 *   order.  Whatever order the matrix core adds the four products of a step in, a term passes through at most
 *   L = hi - lo additions of its chain and 63 of the partial sums, one rounding for its product and 2 (9 n + 4) for its two
 *   weights, n = max n_g.  So a cell whose exact value is at least 2^-900 is within
 *       TPG_SFS_CELL_ROUNDINGS(n, L) u = (18 n + L + 80) 2^-53, relatively,
 *   of the exact rational value of the definition (8 + 64 + 1 + L roundings, the rest for second-order terms and for terms
 *   below 2^-1000, which add at most L 2^-999 absolutely).  Where every usable locus of a cell has v = n_g -- complete data, or
 *   proj = 0 with any pattern of missingness -- every term is 0 or 1 and the cell is the exact integer count as a double,
 *   whatever the order of the sum.
 * Determinism: a cell depends on (lo, hi, g1, g2, proj, keep, flip) alone -- not on nb, on the block's place in the list or on
 *   launch geometry -- and two calls give the same bits.  No floating-point atomics (n_used adds integers).
 * Scratch: the staged operand (at most 128 MiB, or one chunk of TPG_SFS_CHUNK_LOCI loci x the padded width if that is more:
 *   2.1 MiB at W = 4096) plus the partial tiles (32 KiB each: at most 2048 of them, or one block's if that is more: 2145 at
 *   W = 4096) plus tables of a few hundred KiB: under 200 MiB whatever m and nb are.  On any error the caller's outputs are
 *   untouched. */
#define TPG_SFS_MAX_WIDTH 4096
#define TPG_SFS_MAX_BLOCKS 16777215
#define TPG_SFS_CELL_ROUNDINGS(n, L) (18 * (int64_t)(n) + (int64_t)(L) + 80)
/* loci staged at a time per partial sum, in ascending order from the start of its segment (results do not depend on it; the
 * tests put block lengths around it) */
#define TPG_SFS_CHUNK_LOCI 64
int64_t tpg_sfs_chunk_loci(void);
/* the split rule: how many partial sums a block of that length is cut into at width W (a function of the two alone):
 * min(max(1, ceil(block_len / 1024)), min(64, max(1, 1024 / T))), T = the 64 x 64 tiles of the upper triangle of the
 * (W + 1)-wide operand; segments are equal multiples of TPG_SFS_CHUNK_LOCI loci, the last ones shorter or empty.
 * block_len < 0 or W outside [2, TPG_SFS_MAX_WIDTH]: -1 */
int64_t tpg_sfs_segments(int64_t block_len, int64_t W);
/* host only, no context: the bytes tpg_sfs_blocks takes from the device pool as scratch (beyond the view's count table and
 * the device copies of arguments and outputs the caller keeps in host memory); the call checks its own allocations against
 * it.  want_joint = jsfs is asked for.  A bad size: -1 */
int64_t tpg_sfs_scratch_bytes(int64_t m, int ngroups, int64_t W, int64_t nb, int want_joint);
/* host only, no context: csrc/host/host_sfs.h on one (x, v, n): h[0 .. n].  Not 0 <= x <= v, 1 <= n <= v, v < 2^31: TPG_EINVAL */
int tpg_sfs_project_row(int64_t x, int64_t v, int64_t n, double* h);
int tpg_sfs_blocks(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups, const double* ploidy,
                   const int32_t* proj, const uint8_t* keep, const uint8_t* flip, const int64_t* lo, const int64_t* hi, int64_t nb,
                   double* sfs, int64_t* n_used1, double* jsfs, int64_t* n_used2);

/* ---- admixture (gt_admixture, R/gt_admixture.R:62-100: the reference exports the panel to PLINK, runs an outside `admixture`
 * binary and reads its .Q / .P files back; ADMIXTURE is not part of the reference's sources and nothing pins it, so the model
 * and the algorithm are defined HERE: the plain EM of Tang et al. 2005 (FRAPPE), the fixed-point map that Alexander, Novembre
 * and Lange 2009 accelerate) ------------------------------------------------------------------------------------------------
 * Data and parameters.  A view of N individuals x M loci, diploid; g(i,j) in {0, 1, 2} is the dosage of the counted allele,
 *   code 3 is missing and is skipped everywhere ("typed" = not missing).  K ancestral populations.  Q is N x K with rows that
 *   sum to 1; F is K x M, the frequency of the COUNTED (alt) allele, the one tpg_alt_freq_dip_pseudo counts.  (ADMIXTURE's own
 *   .P file may describe the other allele: compare 1 - P before concluding that two runs disagree.)
 * Per typed entry.  p(i,j) = sum_k q(i,k) f(k,j) and pbar(i,j) = sum_k q(i,k) (1 - f(k,j)), both in ascending k, each term
 *   joined by one fused multiply-add starting from +0.  pbar is a sum of positive terms of its own, never 1 - p: the bounds
 *   below rest on that.
 * Log-likelihood.  l(Q,F) = sum over typed (i,j) of [ g ln p + (2 - g) ln pbar ].  The device forms the term as ONE logarithm,
 *   ln(p^g pbar^(2-g)) with the product p p, p pbar or pbar pbar rounded once; f in [eps, 1 - eps] keeps it >= eps^2.
 * One EM step, both updates from the OLD (Q, F).  With w1 = g / p and w0 = (2 - g) / pbar:
 *   a(k,j) = f(k,j) * sum_i q(i,k) w1(i,j);   b(k,j) = (1 - f(k,j)) * sum_i q(i,k) w0(i,j)      (sums over the typed i)
 *   f'(k,j) = a / (a + b), then clamped into [eps, 1 - eps], eps = TPG_ADMIX_EPS
 *   q'(i,k) = (q(i,k) / (2 T_i)) * sum_j [ f(k,j) w1(i,j) + (1 - f(k,j)) w0(i,j) ]              (sum over the typed j;
 *             T_i = typed loci of i; the two products of a locus enter the sum as two terms)
 *   A locus nobody is typed at keeps its f; so does (k, j) when a + b = 0, which takes q(i,k) = 0 at every typed i and cannot
 *   happen from a start of this header.  An individual typed nowhere keeps its row.  Q has no clamp and is not renormalised:
 *   with f in [eps, 1 - eps] and a row sum of 1, p and pbar are >= eps, and the update keeps the row sum at 1 up to rounding.
 *   The clamp is a box constraint on a separable concave M-step, so the step stays a constrained EM step and l does not
 *   decrease in exact arithmetic.
 * Start.  q0 (N x K, column-major) and / or f0 (M x K, column-major: the shape of a .P file), host or device memory.  Each
 *   q0 row is divided by its sum (added in ascending k); f0 is clamped.  An entry of q0 that is not finite or not positive, or
 *   an entry of f0 that is not finite: TPG_EINVAL, found on the device.  Where q0 / f0 is NULL the start is drawn from `seed`,
 *   a pure function of position (M = tpg_mix64, see "simple imputation" above), so it does not depend on launch shape:
 *     u(h) = ((double)(h >> 11) + 0.5) * 2^-53 in IEEE double (the addition rounds to even once h >> 11 >= 2^52; 0 < u <= 1)
 *     Q: h = M(M(seed ^ M(i)) ^ M(k));  q0(i,k) = u / (sum of the row's u, ascending k)
 *     F: h = M(M((seed ^ 0xF0F0F0F0F0F0F0F0) ^ M(j)) ^ M(k));  f0(k,j) = 0.1 + 0.8 u (a product, then a sum: no fusing)
 * Iteration.  State 0 is the start; iteration t makes state t from state t - 1, and the same pass yields l(t - 1).  Stop after
 *   iteration t when t >= 2 and l(t-1) - l(t-2) < tol (converged = 1), or when t = max_iter (converged = 0 unless the rule
 *   holds there too).  A final likelihood-only pass gives l of the returned state: n_iter = t, loglik = l(t), and
 *   loglik_trace[0 .. t] = l(0) .. l(t); entries beyond t are not written.  max_iter = 0 returns the start and its l.  tol is
 *   absolute (ADMIXTURE's default criterion, 1e-4).  The host reads one double per iteration; nothing proportional to N or M
 *   crosses PCIe before the end.
 * Flags.  update_f = 0: projection onto given frequencies (ADMIXTURE -P); P comes back as it went in after clamping, bit for
 *   bit.  update_q = 0: the same for Q (after normalisation).
 * Determinism.  A result depends on the view, K, the start and the parameters alone, not on launch geometry or device; two
 *   calls give the same bits; no floating-point atomics.  Every sum has a fixed shape (csrc/admix.hip); the Q update adds
 *   partial sums over chunks of TPG_ADMIX_CHUNK_LOCI loci in ascending chunk order.
 * Accuracy, u = 2^-52, FP64 throughout, against the exact rational value of one step from the same (Q, F).  Every sum is a sum
 *   of non-negative terms, so each rounding is a relative error of at most u / 2 <= u of the running value and they add up
 *   (first order; the counts below are roundings along the longest path, whatever the order of a sum):
 *     p: K (one per fused term);  pbar: K + 1 (1 - f);  w1: K + 1;  w0: K + 2
 *     sum_i q w1: fused terms and N additions along any path, N + K + 1;  a: + 1;  b: N + K + 2, + 2 (1 - f, the product)
 *     f' = a / (a + b): (N + K + 2) + (N + K + 5) + 1 = 2 N + 2 K + 8              <= (2 N + 4 K + 40) u f'   (unclamped)
 *     sum_j [..]: terms K + 2 and K + 4, at most 2 T_i additions along any path; q / (2 T_i) and the product: 2
 *     q': 2 T_i + K + 6                                                             <= (2 T_i + 2 K + 16) u q'
 *     l, T typed entries: the argument p^g pbar^(2-g) carries g K + (2 - g)(K + 1) + 1 <= 2 K + 3 roundings, which moves ln by
 *     that many u (absolute); ln itself is good to 1 ulp of the term; T additions:  |dl| <= u [ (2 T + 2) |l| + 2 (K + 4) T ]
 *   An exact value within its bound of eps or 1 - eps may come back clamped or not.
 * Errors.  K < 1, K > TPG_ADMIX_MAX_K, max_iter < 0, tol negative or NaN, an entry of ploidy other than 2 (NULL: all diploid),
 *   a view with N = 0 or M = 0: TPG_EINVAL.  Q and P are written at the very end only: after an error they are untouched. */
#define TPG_ADMIX_EPS 1e-5
#define TPG_ADMIX_MAX_K 32
/* loci per partial sum of the Q update (results do not depend on launch geometry; the tests put m around it) */
#define TPG_ADMIX_CHUNK_LOCI 4096
typedef struct tpg_admix_params {
  int32_t max_iter;  /* 1000 */
  double tol;        /* 1e-4 */
  int32_t update_q;  /* 1 */
  int32_t update_f;  /* 1 */
  uint64_t seed;     /* 0 */
} tpg_admix_params;
int tpg_admix_params_default(tpg_admix_params* p);
int64_t tpg_admix_chunk_loci(void);
/* Q: N x K, P: M x K (P[j + k M] = f(k,j)), column-major doubles, host or device memory; q0 / f0 may be NULL (seeded start);
 * params NULL = the defaults; loglik_trace has room for max_iter + 1 doubles or is NULL; loglik, loglik_trace, n_iter and
 * converged are host memory and may each be NULL */
int tpg_admix_em(tpg_ctx* ctx, const tpg_view* v, const double* ploidy, int K, const tpg_admix_params* params, const double* q0,
                 const double* f0, double* Q, double* P, double* loglik, double* loglik_trace, int32_t* n_iter,
                 int32_t* converged);
/* l(Q, F) alone for a caller's own (Q, P), taken as given (no normalisation, no clamp): one likelihood-only pass */
int tpg_admix_loglik(tpg_ctx* ctx, const tpg_view* v, int K, const double* Q, const double* P, double* loglik);

/* ---- admixture cross-validation (gt_admixture(crossval = TRUE), R/gt_admixture.R:20, 37, 184-196, 287-290: the reference passes
 * --cv to the outside binary and reads "CV error" back from its log; nothing pins that number, so what is computed is defined
 * HERE.  The procedure -- hold-out folds of the typed genotypes, a refit per fold, the binomial deviance of the held-out genotypes
 * under the refit -- is that of Alexander and Lange 2011, RECALLED, NOT PINNED) -------------------------------------------------
 * Folds.  The fold of an entry is a pure function of (cv_seed, i, j), the 0-based position in the VIEW (kept row, kept column),
 *   not in the store, so it does not depend on launch shape, block plan or device.  With M = tpg_mix64 and 64-bit unsigned
 *   arithmetic:
 *     key = M((cv_seed ^ 0xC3C3C3C3C3C3C3C3) ^ M(j));  h = M(key ^ M(i));  fold(i,j) = ((h >> 32) * folds) >> 32.
 *   2 <= folds <= TPG_ADMIX_MAX_FOLDS.  Only typed entries are ever held out; the padding stays code 3.
 * Hold-out view.  train_f is the view with every typed entry of fold f set to code 3 and everything else unchanged: a NEW view of
 *   the same geometry (tpg_view_holdout), which any entry point takes.  A locus or an individual typed nowhere in train_f is
 *   handled by the EM as "admixture" says: it keeps its start, and the held-out entries are still predicted from that state.
 * Hold-out sums of a state (Q, F) for a pair (full, train) of the same geometry, over the entries typed in `full` and missing in
 *   `train`:
 *     ll_h  = sum ln(p^g pbar^(2-g)), p and pbar formed exactly as in "admixture" (ascending k, fused terms, pbar a sum of its
 *             own, the product rounded once, one logarithm);
 *     n_h   = the number of such entries;  het_h = the number of them with g = 1 (both int64, exact).
 *   Q and P are taken as given (no normalisation, no clamp), as tpg_admix_loglik takes them.
 * Deviance and CV error.  Per held-out entry dev = 2 [ g ln(g / 2p) + (2 - g) ln((2 - g) / 2 pbar) ] with 0 ln 0 = 0, which is
 *   -2 ln(p^g pbar^(2-g)) - [g = 1] 4 ln 2.  So for fold f, in IEEE double,
 *     dev_f = -2.0 * ll_f - 2.772588722239781 * (double)het_f          (two products, then one subtraction, no fusing)
 *     cv_error = (dev_0 + dev_1 + ... in ascending f) / (double)(n_0 + n_1 + ...).
 *   A constant factor or offset per entry does not move the K that minimises cv_error; ADMIXTURE's own number may differ by one.
 * Cross-validation (tpg_admix_cv).  For f = 0 .. folds - 1 in order: train_f; tpg_admix_em on it with the caller's parameters and
 *   the SAME start for every fold (q0 / f0, or the seeded one); the hold-out sums of (v, train_f) from the Q and P of that run,
 *   which never leave the device; train_f is freed, so the peak extra memory is one view (its L and T layouts).  Then
 *   tpg_admix_cv_error.  Nothing proportional to N or M crosses PCIe (a host q0 / f0 goes up once).
 * Rounding.  ll_h obeys the bound of "admixture" with T = n_h: |dl| <= u [ (2 T + 2) |l| + 2 (K + 4) T ].  The counts are exact.
 *   Every sum has a fixed shape (a thread's entries ascending, a butterfly over the wave, the four waves in order, the tiles by a
 *   one-workgroup kernel); no floating-point atomics; two calls give the same bits. */
#define TPG_ADMIX_MAX_FOLDS 64
/* train_f of `full` as a new view (free it with tpg_view_free); n_held (host memory, may be NULL) = the entries held out.
 * folds outside [2, TPG_ADMIX_MAX_FOLDS], fold outside [0, folds), a view without its locus-tiled layout: TPG_EINVAL */
int tpg_view_holdout(tpg_ctx* ctx, const tpg_view* full, int folds, int fold, uint64_t cv_seed, tpg_view** out, int64_t* n_held);
/* Q: N x K, P: M x K, column-major doubles, host or device memory; ll, n_held and n_het are host memory and may each be NULL.
 * Views of different n or m, K outside [1, TPG_ADMIX_MAX_K]: TPG_EINVAL, nothing written */
int tpg_admix_holdout_sums(tpg_ctx* ctx, const tpg_view* full, const tpg_view* train, int K, const double* Q, const double* P,
                           double* ll, int64_t* n_held, int64_t* n_het);
/* host only, no context, no GPU: the deviances (fold_dev[folds], may be NULL) and the CV error from the folds' sums.  folds out of
 * range, a negative count, more heterozygotes than entries, a total count of 0: TPG_EINVAL, nothing written */
int tpg_admix_cv_error(int folds, const double* fold_ll, const int64_t* fold_count, const int64_t* fold_het, double* fold_dev,
                       double* cv_error);
/* the per-fold arrays (host memory) have `folds` entries and may each be NULL; q0 / f0 as in tpg_admix_em.  Errors: those of
 * tpg_admix_em, and folds out of range.  Every output is written at the very end: after an error they are untouched. */
int tpg_admix_cv(tpg_ctx* ctx, const tpg_view* v, const double* ploidy, int K, const tpg_admix_params* params, int folds,
                 uint64_t cv_seed, const double* q0, const double* f0, double* cv_error, double* fold_ll, int64_t* fold_count,
                 int64_t* fold_het, int32_t* fold_iter, int32_t* fold_converged);

/* ---- admixture, accelerated (no counterpart in the reference: the outside binary accelerates its own block relaxation; here the
 * EM map of "admixture" is wrapped in squared extrapolation, SQUAREM, scheme S3 of Varadhan and Roland 2008, RECALLED, NOT
 * PINNED.  The same likelihood and the same EM step; fewer of them) --------------------------------------------------------------
 * State.  theta = (Q, F) of "admixture"; E(theta) is one EM step of that section, clamp included; l(theta) its likelihood.  The
 *   pass that applies E to theta also yields l(theta), as there.
 * One cycle from theta0, with a step limit a_max (4 at the start of a run):
 *   1. theta1 = E(theta0), which yields l(theta0); theta2 = E(theta1), which yields l(theta1).
 *   2. Stop rule, the plain one ("a plain EM step gained less than tol"): if l(theta1) - l(theta0) < tol, return theta2 with
 *      converged = 1, as the plain EM returns the state one step past the compared pair.
 *   3. Per entry, in IEEE double, one rounding per operation, no fusing:  r = theta1 - theta0;  v = (theta2 - theta1) - r.
 *   4. sr = sum r^2 and sv = sum v^2 over every entry of the halves being updated (Q only with update_f = 0, F only with
 *      update_q = 0), each term joined to its sum by one fused multiply-add.  The shape of the sums is fixed: the K live columns of
 *      the state stored row by row (row i: q(i, 0 .. K - 1), row j: f(0 .. K - 1, j)) padded to the dispatch width, padding
 *      excluded, cut into tiles of 2048 stored doubles; in a tile, thread t of 256 adds the entries 256 e + t in ascending e, then a
 *      butterfly over each wave of 64 and the four waves in order; Q's tiles come before F's, and a one-workgroup kernel has thread
 *      t add the tiles t, t + 256, ... in ascending order, then the same butterfly and wave order.  No floating-point atomics.
 *   5. The host reads sr and sv (two doubles per cycle) and forms alpha = -sqrt(sr / sv), a correctly rounded quotient, then a
 *      correctly rounded root.  sv = 0, or an alpha that is not finite: alpha = -1.  Then alpha is clipped into [-a_max, -1].
 *   6. theta' raw, per entry: fma(a2, v, fma(-2 alpha, r, theta0)) with a2 = alpha * alpha rounded once.
 *   7. The projection of theta' raw onto the feasible set, row by row (a row = one individual of Q or one locus of F):
 *        F: each entry clamped into [eps, 1 - eps], eps = TPG_ADMIX_EPS;
 *        Q: each entry raised to at least eps, then the row divided by its sum, added in ascending k from 0 (the normalisation of
 *           the start);
 *        a row in which nothing moved (r = v = 0 in every entry) keeps theta0 bit for bit.  A locus or an individual typed
 *        nowhere is such a row, since E keeps it.
 *   8. theta'' = E(theta'), which yields l(theta').  ACCEPT if l(theta') is finite and l(theta') >= l(theta1): the next cycle
 *      starts from theta''; if alpha was clipped at -a_max, a_max becomes 4 a_max.  REJECT otherwise: the next cycle starts from
 *      theta2, and a_max becomes max(1, a_max / 4).  No extra likelihood pass is spent either way.  In exact arithmetic
 *      l(theta'') >= l(theta') >= l(theta1) >= l(theta0) and l(theta2) >= l(theta1): the likelihoods at the starts of the cycles do
 *      not decrease.
 * Counting.  n_iter counts EM steps, so it compares with the plain EM's and with max_iter; a cycle costs three.  max_iter reached
 *   inside a cycle abandons the cycle and returns the last state an EM step produced (theta1 or theta2); reached with the third
 *   step of a cycle it returns the state the next cycle would have started from (theta'', or theta2 after a rejection), and the
 *   cycle counts.  converged = 1 only by the stop rule.  A final likelihood-only pass gives loglik of the returned state.
 *   loglik_trace = l of every state an EM step was applied to, in order, then loglik: n_iter + 1 entries (per whole cycle
 *   l(theta0), l(theta1), l(theta')).  alpha[c] and accepted[c] (1 / 0) of cycle c = 0 .. n_cycles - 1, n_cycles and n_rejected
 *   are additional outputs.  max_iter = 0, both update flags 0 (every cycle then has sr = sv = 0, alpha = -1 and theta' = theta0),
 *   the errors and "outputs untouched after an error" are as in tpg_admix_em.
 * Determinism.  As "admixture": a result is a function of the view, K, the start and the parameters alone; two calls give the
 *   same bits.
 * Rounding, u = 2^-52, first order, nn = the number of entries summed.  Against the exact sum of (theta1 - theta0)^2 of the given
 *   doubles, sr carries the rounding of r (twice in the square), the fused term and at most nn - 1 additions that are not exact
 *   (adding 0 is): |d sr| <= (nn + 3) u sr.  v is a difference of differences, so its error is absolute:
 *     |dv| <= u (|theta2 - theta1| + |r| + |v|);   |d sv| <= 2 sum |v| |dv| + (nn + 3) u sv.
 *   Given sr and sv, alpha is bit-exact; given alpha, r and v, theta' raw is bit-exact. */
/* tpg_admix_em's arguments, then: alpha (double) and accepted (int32) with room for max_iter / 3 entries each (integer division),
 * n_cycles, n_rejected; host memory, each may be NULL */
int tpg_admix_em_squarem(tpg_ctx* ctx, const tpg_view* v, const double* ploidy, int K, const tpg_admix_params* params,
                         const double* q0, const double* f0, double* Q, double* P, double* loglik, double* loglik_trace,
                         int32_t* n_iter, int32_t* converged, double* alpha, int32_t* accepted, int32_t* n_cycles,
                         int32_t* n_rejected);
/* tpg_admix_cv with every fold refitted by tpg_admix_em_squarem: the same folds, hold-out sums and error */
int tpg_admix_cv_squarem(tpg_ctx* ctx, const tpg_view* v, const double* ploidy, int K, const tpg_admix_params* params, int folds,
                         uint64_t cv_seed, const double* q0, const double* f0, double* cv_error, double* fold_ll,
                         int64_t* fold_count, int64_t* fold_het, int32_t* fold_iter, int32_t* fold_converged);
/* steps 3 to 7 for a caller's own theta0, theta1, theta2 (q*: n x K, f*: m x K, column-major doubles, host or device memory, taken
 * as given: no normalisation, no clamp) and a_max >= 1.  sr, sv, alpha: host memory; Qp / Pp = the projected theta', Qraw / Praw =
 * theta' raw (the shapes of q0 / f0, host or device memory); a half that is not updated comes back as theta0 in both.  Every output
 * may be NULL.  K out of [1, TPG_ADMIX_MAX_K], n or m < 1, a_max < 1 or NaN: TPG_EINVAL, nothing written */
int tpg_admix_squarem_point(tpg_ctx* ctx, int64_t n, int64_t m, int K, int update_q, int update_f, const double* q0,
                            const double* f0, const double* q1, const double* f1, const double* q2, const double* f2, double a_max,
                            double* sr, double* sv, double* alpha, double* Qp, double* Pp, double* Qraw, double* Praw);

/* ---- sNMF (gt_snmf, R/gt_snmf.R: the reference writes a .geno file and calls LEA::snmf; LEA is not part of the reference's
 * sources and nothing pins it, so what is computed is defined HERE: sparse non-negative matrix factorisation by alternating
 * non-negative least squares (Frichot et al. 2014; Kim and Park 2007), RECALLED, NOT PINNED) --------------------------------------
 * Data.  A view of N individuals x M loci, diploid.  x(i,j,c) = [g(i,j) = c] for c in {0, 1, 2}: three indicator columns per
 *   locus.  A missing entry (code 3) has all three indicators 0 and STAYS IN THE LOSS (the recalled bit encoding of sNMF does
 *   this; it keeps both normal matrices shared by every system).  A caller who wants otherwise imputes the view first.
 * State.  K in [1, TPG_SNMF_MAX_K].  Q is N x K, non-negative, rows summing to 1.  G(j,c,k) >= 0 with sum_c G(j,c,k) = 1,
 *   returned as a 3M x K column-major matrix with row 3 j + c (the order of LEA's .G file).  P(j,k) = G(j,1,k) / 2 + G(j,2,k)
 *   (a quotient, then a sum), M x K: the frequency of the counted allele.
 * Ridge.  ridge(C) of a K x K matrix C: rho = (TPG_SNMF_RIDGE * tr) / (double)K with tr = C(0,0) + C(1,1) + ... in ascending k;
 *   C + rho I.  With it every matrix below is positive definite and every NNLS optimum is unique.
 * NNLS(C, b) = argmin over x >= 0 of x'Cx / 2 - b'x.
 * One iteration, from Q to (G, Q'):
 *   1. A = ridge(Q'Q).
 *   2. for every (j,c): b(k) = sum over the i with g(i,j) = c of Q(i,k);  gt(j,c,.) = NNLS(A, b).
 *   3. s(j,k) = gt(j,0,k) + gt(j,1,k) + gt(j,2,k) in that order.  s > TPG_SNMF_TINY: G(j,c,k) = gt(j,c,k) / s; else G(j,c,k) = 1/3
 *      (1.0 / 3.0) in the three classes.
 *   4. B = ridge(GG' + alpha 11'): GG'(k,l) = sum over the 3M rows of G(.,k) G(.,l); alpha is added to every entry, then the ridge
 *      from the trace of that sum.
 *   5. for every i: b_i(k) = sum over the typed j of G(j,g(i,j),k);  qt = NNLS(B, b_i);  r = qt(0) + qt(1) + ... in ascending k.
 *      r > TPG_SNMF_TINY: Q'(i,k) = qt(k) / r; else Q'(i,k) = 1 / K (1.0 / (double)K).
 *   Criterion.  ls = T - 2 sum_i Q'(i,.).b_i + sum_kl (Q''Q')(k,l) (GG')(k,l), T = the typed entries of the view, GG' without alpha
 *   and without ridge: ||X - Q'G'||^2 of the returned pair written out, from sums the iteration has anyway (no extra sweep).
 *   The dot products are fused multiply-adds in ascending k (k major, then l) from +0.
 * Start.  q0 (N x K column-major, host or device memory): each row divided by its sum (ascending k); an entry that is not
 *   finite or not positive: TPG_EINVAL, found on the device (as tpg_admix_em does).  q0 = NULL: the seeded Q of "admixture",
 *   bit for bit, from `seed`.
 * Iteration.  State 0 is the start; iteration t makes (G, Q)(t) from Q(t - 1) and ls(t).  Stop after iteration t >= 2 when
 *   |ls(t-1) - ls(t)| <= tol * ls(t-1) (converged = 1), or at t = max_iter.  ls_trace[0 .. t-1] = ls(1) .. ls(t); ls = ls(t).
 *   max_iter = 0 returns the start, G = 1/3 everywhere, n_iter = 0 and ls = NaN.  The host reads one double per iteration.
 * NNLS contract.  With w = b - C x and bmax = max |b(k)|, a returned x has x >= 0, |w(k)| <= tau bmax where x(k) > 0 and
 *   w(k) <= tau bmax where x(k) = 0, tau = TPG_SNMF_KKT_TOL.  A system that misses this when the solver stops is counted in
 *   n_unsolved (int64; its x is still >= 0); 0 is the expected value.  The solver (csrc/snmf.hip) is Lawson and Hanson's
 *   active-set method on the normal equations, each inner solve a Cholesky factorisation of the masked matrix with one step
 *   of iterative refinement.
 * Hold-out by fraction.  With h(i,j) of "admixture cross-validation" (the same salt and order, `seed` in the place of cv_seed),
 *   an entry is held out iff it is typed and (h >> 32) < floor(fraction * 2^32), 0 < fraction < 1: a NEW view, exactly as
 *   tpg_view_holdout makes one.
 * Cross-entropy sums of a state (Q, G) for a pair (full, train) of the same geometry.  Per entry with genotype g:
 *   p = sum_k q(i,k) G(j,g,k), fused terms in ascending k from +0; term = -ln max(p, TPG_SNMF_P_FLOOR).  Summed over (a) the
 *   entries typed in `full` and missing in `train` (masked) and (b) the entries typed in `train` (all); each a double sum and
 *   an int64 count; the cross-entropy is sum / count.  Q and G are taken as given.
 * Determinism.  As "admixture": every sum has a fixed shape (csrc/snmf.hip), no floating-point atomics, no dependence on launch
 *   geometry; the Q step's right-hand sides are partial sums over chunks of TPG_ADMIX_CHUNK_LOCI loci added in ascending chunk
 *   order; Gram matrices are sums over tiles of TPG_SNMF_GRAM_ROWS rows added in ascending tile order.  Two calls: same bits.
 * Out of scope: K > TPG_SNMF_MAX_K, ploidy other than 2, LEA's I initialisation and project files, sNMF inside tpg_stream_* /
 *   tpg_multi_*, a loss that masks missing entries instead of zeroing them.
 * Errors.  K outside [1, TPG_SNMF_MAX_K], max_iter < 0, tol or alpha negative or NaN, ploidy other than 2, N = 0 or M = 0,
 *   fraction outside (0, 1), views of different geometry: TPG_EINVAL.  Q, G and P are written at the very end only: after an
 *   error every output is untouched. */
#define TPG_SNMF_MAX_K 16
#define TPG_SNMF_RIDGE 1e-10
#define TPG_SNMF_TINY 1e-9
#define TPG_SNMF_KKT_TOL 1e-12
#define TPG_SNMF_P_FLOOR 1e-9
#define TPG_SNMF_GRAM_ROWS 256
/* the defaults of gt_snmf: tpg_snmf takes its parameters one by one */
#define TPG_SNMF_MAX_ITER 200
#define TPG_SNMF_TOL 1e-5
#define TPG_SNMF_ALPHA 10.0
/* Q: N x K, G: 3M x K, P: M x K, column-major doubles, host or device memory, G and P may be NULL; q0 may be NULL (seeded start);
 * ls_trace has room for max_iter doubles or is NULL; ls, ls_trace, n_iter, converged and n_unsolved (the total over the run) are
 * host memory and may each be NULL */
int tpg_snmf(tpg_ctx* ctx, const tpg_view* v, const double* ploidy, int K, int max_iter, double tol, double alpha, uint64_t seed,
             const double* q0, double* Q, double* G, double* P, double* ls, double* ls_trace, int* n_iter, int* converged,
             int64_t* n_unsolved);
/* one iteration from Q_in, taken as given (no normalisation): Q_out (N x K), G_out (3M x K, may be NULL), ls and n_unsolved (host
 * memory, may be NULL) */
int tpg_snmf_step(tpg_ctx* ctx, const tpg_view* v, int K, double alpha, const double* Q_in, double* Q_out, double* G_out, double* ls,
                  int64_t* n_unsolved);
/* the batched solver alone: X(r,.) = NNLS(A, B(r,.)), A K x K symmetric positive definite (no ridge is added), B and X
 * nrhs x K column-major, host or device memory */
int tpg_nnls_shared(tpg_ctx* ctx, int K, const double* A, const double* B, int64_t nrhs, double* X, int64_t* n_unsolved);
/* the fraction hold-out of `full` as a new view (free it with tpg_view_free); n_held (host memory, may be NULL) */
int tpg_view_holdout_fraction(tpg_ctx* ctx, const tpg_view* full, double fraction, uint64_t seed, tpg_view** out, int64_t* n_held);
/* Q: N x K, G: 3M x K, column-major doubles, host or device memory; the four outputs are host memory and may each be NULL */
int tpg_snmf_cross_entropy_sums(tpg_ctx* ctx, const tpg_view* full, const tpg_view* train, int K, const double* Q, const double* G,
                                double* sum_masked, int64_t* n_masked, double* sum_all, int64_t* n_all);

/* pop_global_stats (R/pop_global_stats.R:113-212, with compute_np_mn, src/compute_np_mn.cpp:8-34): by_locus =
 * m x 10 column-major {Ho, Hs, Ht, Dst, Htp, Dstp, Fst, Fstp, Fis, Dest} (may be NULL), overall = the 10
 * by_locus = FALSE values (may be NULL).  ploidy (may be NULL) must be all 2: the reference stops otherwise. */
int tpg_pop_global_stats(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups,
                         const double* ploidy, double* by_locus, double* overall);
/* pop_het_obs (which = 0, R/pop_het_obs.R:78-91), pop_het_exp / pop_gene_div (1, R/pop_het_exp.R:85-103) and
 * pop_fis(method = "Nei87") (2, R/pop_fis.R:108-130): by_locus = m x G (may be NULL), colmeans = colMeans(na.rm = TRUE)
 * over the loci, G values (may be NULL).  ploidy as in tpg_pop_global_stats. */
int tpg_pop_basic_stats(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups, const double* ploidy,
                        int which, double* by_locus, double* colmeans);
/* the numeric core of windows_stats_generic (R/windows_stats_generic.R:113-176: runner::mean_run /
 * sum_run with na_rm = TRUE) for every column of the per-locus matrix x (m x ncol, column-major, host or device):
 * window w covers the loci lo[w] .. hi[w]-1 (0-based; the host side derives them from chromosome / position /
 * window_size / step_size); pad_na[w] != 0 marks a window the reference returns as NA under complete = TRUE (may be
 * NULL).  op 0 = mean, 1 = sum.  stat (nw x ncol) is NaN where the window holds no value or fewer than min_loci;
 * n_loci (nw x ncol int32, may be NULL) = values present, -1 for a pad_na window. */
int tpg_window_stats(tpg_ctx* ctx, const double* x, int64_t m, int ncol, const int64_t* lo, const int64_t* hi,
                     const uint8_t* pad_na, int64_t nw, int op, int min_loci, double* stat, int32_t* n_loci);
/* population branch statistic from a by-locus (or by-window) pairwise Fst matrix: pbs_one_triplet of
 * R/nwise_pop_pbs.R:118-156.  fst is m x P (column-major, host or device); triplet t names the columns of
 * (pop1.pop2, pop1.pop3, pop2.pop3) in trip_cols0[3t..3t+2] (0-based); out is m x 6 ntrip, six columns per triplet:
 * pbs_1, pbs_2, pbs_3, pbsn1_1, pbsn1_2, pbsn1_3 */
int tpg_pbs_from_fst(tpg_ctx* ctx, const double* fst, int64_t m, int P, const int32_t* trip_cols0, int ntrip,
                     double* out);
/* replaces alt_freq_dip_pseudo_cpp (src/alt_freq_dip_pseudo_cpp.cpp:8-58) for the whole
 * colInd at once (the big_apply block loop R/loci_alt_freq.R:351-359 collapses):
 * out m x 2 = {n_alt | freq, n_valid} */
int tpg_alt_freq_dip_pseudo(tpg_ctx* ctx, const tpg_view* v, const double* ploidy, int as_counts,
                            double* out);
/* replaces grouped_alt_freq_dip_pseudo_cpp (src/grouped_alt_freq_dip_pseudo_cpp.cpp:8-58):
 * out m x 2G */
int tpg_grouped_alt_freq_dip_pseudo(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0,
                                    int ngroups, const double* ploidy, int as_counts, double* out);
/* replaces grouped_missingness_cpp (src/grouped_missingness_cpp.cpp:8-33): out m x G */
int tpg_grouped_missingness(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups,
                            double* out);
/* replaces grouped_summaries_dip_pseudo_cpp (src/grouped_summaries_dip_pseudo_cpp.cpp:11-63):
 * four m x G outputs (any may be NULL) */
int tpg_grouped_summaries_dip_pseudo(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0,
                                     int ngroups, const double* ploidy, double* freq_alt,
                                     double* freq_ref, double* n, double* het_obs);

/* ---- pairwise population Fst --------------------------------------------- */
#define TPG_FST_HUDSON 0
#define TPG_FST_NEI87 1
#define TPG_FST_WC84 2
/* Fused path: grouped summaries + pair loop without materialising the m x G matrices
 * (replaces R/pairwise_pop_fst.R:123-161).  pairs1 is 2 x P column-major, 1-based.
 * fst_tot[P]; out_a / out_b are m x P (by_locus ratio or numerator / denominator), may be
 * NULL when by_locus == 0. */
int tpg_pairwise_pop_fst(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups,
                         const double* ploidy, int method, const int32_t* pairs1, int P, int by_locus,
                         int return_num_dem, double* fst_tot, double* out_a, double* out_b);
/* Same sweep, but returns the sums over this view's loci of numerator and denominator
 * (sum_num[P], sum_den[P]) instead of their ratio: SNP-block shards on different GPUs add these
 * (one all-reduce of 2P doubles) before dividing. */
int tpg_pairwise_pop_fst_sums(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups,
                              const double* ploidy, int method, const int32_t* pairs1, int P,
                              double* sum_num, double* sum_den);
/* Literal mirrors of the three loop functions (src/pairwise_fst_hudson_loop.cpp:5-63,
 * src/pairwise_fst_wc84_loop.cpp:5-121, src/pairwise_fst_nei87_loop.cpp:5-115): inputs are
 * the m x G double matrices the reference passes; unused ones may be NULL. */
int tpg_pairwise_fst_loop(tpg_ctx* ctx, int method, const int32_t* pairs1, int P, int64_t m, int G,
                          const double* n, const double* freq_alt, const double* freq_ref,
                          const double* het_obs, int by_locus, int return_num_dem, double* fst_tot,
                          double* out_a, double* out_b);

/* ---- windowed pairwise Fst (windows_pairwise_pop_fst, R/windows_pairwise_pop_fst.R:62-107 over
 * R/windows_stats_generic.R:113-179; the Fst behind windows_nwise_pop_pbs, R/windows_nwise_pop_pbs.R:78-114 with
 * pbs_one_triplet of R/nwise_pop_pbs.R:116-157 = tpg_pbs_from_fst) -----------------------------------------------------
 * Per-locus terms: for pair (g1, g2) and locus j, num(j) and den(j) are exactly the doubles tpg_pairwise_pop_fst(...,
 *        return_num_dem = 1) writes for that method: the same statement order, IEEE double, no FMA contraction.
 * Windows: window w covers the loci lo[w] .. hi[w]-1 with a pad_na flag, the contract of tpg_window_stats.  n_num = the
 *        number of non-NaN num in the window, n_den = the number of non-NaN den: counted separately, as the reference's two
 *        windows_stats_generic calls do (they differ at a pseudohaploid group with one typed allele, where p q / (n - 1) is
 *        0 / 0 while den is finite).  mean_num = (sum of the non-NaN num) / n_num, NaN where the window is padded, n_num = 0
 *        or n_num < min_loci; mean_den likewise with n_den.  fst = mean_num / mean_den, one IEEE division of those two
 *        doubles.  n_num and n_den are -1 on a pad_na window.
 * Sums:  with C = TPG_WINFST_CHUNK_LOCI, b0 = C ceil(lo / C) and b1 = C floor(hi / C): if b0 >= b1 the window's terms are
 *        added one by one in ascending locus order; otherwise the terms of lo .. b0-1 one by one, then the sums of the
 *        whole chunks b0 / C .. b1 / C - 1 in ascending order (each the sum of its 64 terms in ascending locus order,
 *        started from 0), then the terms of b1 .. hi-1 one by one.  A window sum is within L 2^-52 sum |x_j| of the exact
 *        sum of its L non-NaN doubles.
 * Determinism: a cell depends on (lo, hi, pair, method, the view and its grouping) alone -- not on nw, on the window's place
 *        in the list, on the other windows or on launch geometry.  No floating-point atomics; two calls give the same bits.
 * Methods: TPG_FST_HUDSON, TPG_FST_NEI87, TPG_FST_WC84; pseudohaploids only with Hudson (TPG_EINVAL otherwise, with the
 *        message of tpg_pairwise_pop_fst).
 * Outputs are nw x P column-major; fst is required, the other four may be NULL.  lo, hi, pad_na (may be NULL) and every output
 * may be host or device memory; pairs1 (2 x P column-major, 1-based) is host memory.  Nothing proportional to m crosses PCIe,
 * and no m x P matrix is formed.
 * A window outside [0, m], lo > hi, min_loci < 1, a pair outside [1, ngroups], P < 1, nw > TPG_WINFST_MAX_WINDOWS (one
 * workgroup row per window: split the list): TPG_EINVAL, nothing written; nw == 0: TPG_OK, nothing written. */
#define TPG_WINFST_CHUNK_LOCI 64
#define TPG_WINFST_MAX_WINDOWS 16777215
/* loci per chunk partial (a power of two; results are defined in terms of it, see "Sums" above) */
int64_t tpg_winfst_chunk_loci(void);
/* host only, no context: the bytes tpg_windows_pairwise_pop_fst takes from the device pool as scratch, beyond the view's
 * count table and the device copies of arguments and outputs the caller keeps in host memory: the chunk partials, 24 bytes
 * per (whole chunk, pair), and the pair list.  At most m P / 2 + 8 P + 32; nw does not enter.  A bad size: -1 */
int64_t tpg_windows_fst_scratch_bytes(int64_t m, int ngroups, int P, int64_t nw);
int tpg_windows_pairwise_pop_fst(tpg_ctx* ctx, const tpg_view* v, const int32_t* groupIds0, int ngroups, const double* ploidy,
                                 int method, const int32_t* pairs1, int P, const int64_t* lo, const int64_t* hi,
                                 const uint8_t* pad_na, int64_t nw, int min_loci, double* fst, double* mean_num,
                                 double* mean_den, int32_t* n_num, int32_t* n_den);

/* ---- Fst under relabelings (pairwise_pop_fst_test: is a pairwise Fst different from zero?  The permutation test of Arlequin,
 * hierfstat and StAMPP: shuffle the individuals between the populations, recompute Fst, see where the observed value falls.  The
 * reference has nothing of the kind, so everything is defined HERE) --------------------------------------------------------------
 * Labels: labels is R x n row-major in host memory; labels[r][i] in {-1, 0 .. ngroups-1} is the group of individual i under
 *        relabeling r, -1 = the individual is outside relabeling r.  A relabeling may leave a group empty.
 * Per-locus terms: for relabeling r, pair (g1, g2) and locus j, num and den are exactly the doubles tpg_pairwise_pop_fst(...,
 *        return_num_dem = 1) writes for that method on the view that keeps only the individuals with label >= 0, grouped by those
 *        labels: integer counts per (locus, group), then the statements of fst_stage and fst_terms<METHOD, false>
 *        (csrc/fst_terms.h) in IEEE double without FMA contraction; for Hudson e = (p (1 - p)) / (n - 1) as tpg_fst_kernel stages
 *        it.  A locus is KEPT for a pair when num and den are both non-NaN; n_kept counts those loci.  (An empty group has
 *        p = 0 / 0: none of its loci is kept, its sums are +0.0, n_kept = 0 and the ratio is NaN.)
 * Sums:  with U = TPG_FSTPERM_UNIT_LOCI (a divisor of 32) and S = TPG_FSTPERM_SPAN_LOCI (a multiple of 128): the kept terms of
 *        unit k, loci k U .. k U + U - 1, are added in ascending locus order from 0.0; the unit sums of span s, loci s S ..
 *        s S + S - 1, are added in ascending order from 0.0 (a unit without kept terms adds its 0.0); the span sums are added in
 *        ascending order from 0.0.  sum_num and sum_den are added separately over the same kept set.  No floating-point atomics.
 *        A sum is within m 2^-52 sum |x_j| of the exact sum of its kept doubles.
 * Determinism: the outputs of a relabeling depend on the view, its label row, ngroups, the pair list and the method alone: not on
 *        R, on its place in the list, on the other rows, on the library's internal batching or on launch geometry.  Two calls
 *        give the same bits.
 * Limits and errors: diploid codes only (there is no ploidy argument).  2 <= ngroups <= TPG_FSTPERM_MAX_GROUPS, because the
 *        classes of a relabeling live in the accumulators of one workgroup; above it TPG_EINVAL with a message that points to the
 *        pairwise scheme (two groups per relabeling).  A label outside [-1, ngroups), a pair outside [1, ngroups] or with
 *        g1 == g2, P < 1, R < 0, an unknown method: TPG_EINVAL, nothing written.  R == 0: TPG_OK, nothing written.
 *        n >= 2^24: TPG_EUNSUPPORTED, as for the grouped counts.  The library walks R in internal batches, so its device scratch is
 *        bounded independently of R: tpg_fst_relabel_scratch_bytes (host only; a bad size: -1).
 * Outputs: sum_num, sum_den (doubles) and n_kept (may be NULL), each R x P row-major, host memory.
 * tpg_fst_perm_labels (host only, no context, no GPU) is the r-th relabeling as a pure function of its arguments.  With
 *        M = tpg_mix64 (see "simple imputation") and 64-bit unsigned arithmetic: the eligible set E is e_0 < e_1 < ... in ascending
 *        index -- scheme 0 "pairwise": the individuals of groups a and b (0-based ids, a != b); scheme 1 "global": everybody.
 *        key(i) = M(seed ^ M((r << 32) + i)); sigma is E sorted by (key, index); individual sigma_t receives the group of e_t.
 *        r = 0 is the identity and is not hashed.  Scheme 0 writes a -> 0, b -> 1 and everybody else -> -1 (use it with
 *        ngroups = 2 and the pair (1, 2)); scheme 1 writes the groups as they are.  0 <= r < 2^31, n < 2^31; a bad argument:
 *        TPG_EINVAL.
 * Not offered: block-bootstrap confidence intervals over loci (the span sums are the hook), pseudohaploids, tpg_stream_* /
 *        tpg_multi_* forms, an R shim entry. */
#define TPG_FSTPERM_UNIT_LOCI 8
#define TPG_FSTPERM_SPAN_LOCI 512
#define TPG_FSTPERM_MAX_GROUPS 64
int tpg_fst_relabel_sums(tpg_ctx* ctx, const tpg_view* v, const int32_t* labels, int64_t R, int ngroups, int method,
                         const int32_t* pairs1, int P, double* sum_num, double* sum_den, int64_t* n_kept);
int64_t tpg_fstperm_unit_loci(void);
int64_t tpg_fstperm_span_loci(void);
int64_t tpg_fst_relabel_scratch_bytes(int64_t n, int64_t m, int ngroups, int P);
int tpg_fst_perm_labels(int64_t n, const int32_t* groupIds0, int ngroups, int scheme, int a, int b, uint64_t seed, int64_t r,
                        int32_t* out);

/* ---- pairwise individual matrices (IBS / KING / allele sharing / GRM) ---- */
/* Accumulators for the four integer cross-products V=vv', D=dd', H=hh', A=hv'
 * (v valid, d = dosage-1, h heterozygous), from which every count matrix of
 * increment_ibs_counts / increment_king_numerator / increment_as_counts follows.
 * If ext_buffer != NULL it must be device memory of tpg_pairwise_buffer_bytes(n)
 * bytes (e.g. a torch tensor).  What the buffer holds is private: the matrix cores multiply the MISSING plane m = 1 - v, so
 * the sums in it are MM = mm' and HM = hm', and the count / epilogue entry points rebuild V = L - m_i - m_j + MM_ij and
 * A = Hc_i - HM_ij from them, the diagonals and the number L of loci the accumulators have seen.  L is not in the buffer: buffers
 * of several ranks are summed by tpg_pairwise_create_sharded + tpg_pairwise_reduce (which sums L with them), not by an
 * all-reduce of the caller's. */
size_t tpg_pairwise_buffer_bytes(int64_t n);
int tpg_pairwise_create(tpg_ctx* ctx, int64_t n, void* ext_buffer, tpg_pairwise** out);
void tpg_pairwise_free(tpg_pairwise* pw);
int tpg_pairwise_zero(tpg_ctx* ctx, tpg_pairwise* pw);
/* add loci [col_begin, col_end) of the view (0-based, end exclusive; -1 = m): all five products */
int tpg_pairwise_accumulate(tpg_ctx* ctx, tpg_pairwise* pw, const tpg_view* v, int64_t col_begin,
                            int64_t col_end);
/* The same for the products one analysis needs (the reference runs 2 / 6 / 4 dense products for allele sharing / IBS /
 * KING: src/snp_as.cpp:64-65, src/snp_ibs.cpp:67-72, src/snp_king.cpp:70-72): `products` = OR of TPG_PW_V (typed x
 * typed), TPG_PW_D (dosage-1 x dosage-1), TPG_PW_H (het x het), TPG_PW_A (het x typed, both orientations).  Each set
 * has a kernel with a wave tile of its own (fewer sums per pair leave registers for more pairs per operand byte).
 * Products that were left out stay unknown until the next tpg_pairwise_zero: the count / epilogue entry points
 * refuse (TPG_EINVAL) an output that needs one of them. */
#define TPG_PW_V 1
#define TPG_PW_D 2
#define TPG_PW_H 4
#define TPG_PW_A 8
/* D and H added up in ONE sum (IBS = V + (D + H), IBS_valid = 2 V: snp_ibs needs nothing else, src/snp_ibs.cpp:67-72).  Two
 * sums per pair instead of three leave registers for a 128 x 64 wave tile: 24 MFMAs per 6 operand fragments where the
 * {V, D, H} kernel has 12 per 4.  Goes with TPG_PW_V only; afterwards D and H are unknown on their own -- the allele-sharing
 * and KING outputs are refused -- and tpg_pairwise_products reports TPG_PW_V | TPG_PW_DH. */
#define TPG_PW_DH 16
#define TPG_PW_FOR_AS (TPG_PW_V | TPG_PW_D)               /* snp_allele_sharing, pairwise_grm */
#define TPG_PW_FOR_IBS (TPG_PW_V | TPG_PW_D | TPG_PW_H)   /* snp_ibs together with allele sharing / GRM */
#define TPG_PW_FOR_IBS_ALONE (TPG_PW_V | TPG_PW_DH)       /* snp_ibs on its own */
#define TPG_PW_FOR_KING (TPG_PW_V | TPG_PW_D | TPG_PW_A)  /* snp_king */
#define TPG_PW_ALL (TPG_PW_V | TPG_PW_D | TPG_PW_H | TPG_PW_A)
int tpg_pairwise_accumulate_products(tpg_ctx* ctx, tpg_pairwise* pw, const tpg_view* v, int64_t col_begin,
                                     int64_t col_end, int products);
/* the products whose sums are complete since the last tpg_pairwise_zero (TPG_PW_ALL when nothing was left out) */
int tpg_pairwise_products(const tpg_pairwise* pw);
/* Reference quirk Q1, opt-in.  increment_as_counts adds +1 to EVERY element of the allele-sharing
 * numerator for every block of the R driver that is one column narrower than the widest (src/snp_as.cpp:57-63 with
 * the scratch matrices of R/snp_allele_sharing.R:55-56).  The default (0 blocks) is the mathematically intended
 * value, which is what the reference's own test asserts; to reproduce a real R run bit for bit pass the number of
 * narrower blocks of that run: as_num, allele sharing and GRM then come out as R's.  tpg_as_pad_quirk_blocks gives
 * that number for m loci cut by CutBySize(m, block_size) (R/local_reimplementations.R:13-15). */
int tpg_pairwise_set_as_pad_quirk(tpg_pairwise* pw, int64_t narrow_blocks);
int64_t tpg_as_pad_quirk_blocks(int64_t m, int64_t block_size);
/* raw count matrices, n x n column-major doubles, any may be NULL:
 * ibs / ibs_valid (snp_ibs raw_counts), king_num / n_Aa_i (snp_king), as_num / as_den */
int tpg_pairwise_counts(tpg_ctx* ctx, const tpg_pairwise* pw, double* ibs, double* ibs_valid,
                        double* king_num, double* n_Aa_i, double* as_num, double* as_den);
/* epilogues of the R drivers */
#define TPG_IBS_PROPORTION 0
#define TPG_IBS_ADJUSTED_COUNTS 1
int tpg_pairwise_ibs(tpg_ctx* ctx, const tpg_pairwise* pw, int type, int64_t m, double* out); /* R/snp_ibs.R:84-103 */
int tpg_pairwise_king(tpg_ctx* ctx, const tpg_pairwise* pw, double* out);           /* R/snp_king.R:79-101 */
int tpg_pairwise_allele_sharing(tpg_ctx* ctx, const tpg_pairwise* pw, double* out); /* R/snp_allele_sharing.R:77-81 */
int tpg_pairwise_grm(tpg_ctx* ctx, const tpg_pairwise* pw, double* out);            /* R/pairwise_grm.R:42-50 */
/* all four epilogues from one pass over the accumulators; any output may be NULL */
int tpg_pairwise_epilogues(tpg_ctx* ctx, const tpg_pairwise* pw, int ibs_type, int64_t m, double* ibs,
                           double* king, double* allele_sharing, double* grm);
/* the reduction pop_fst / pop_fis(method = "WG17") make of the N x N allele-sharing matrix
 * (R/pop_fst.R:40-63, R/pop_fis.R:151-173): mean[g1 + g2 G] = mean(A[rows of g1, columns of g2], na.rm = TRUE),
 * with the diagonal of A left out when skip_diag != 0; count (may be NULL) = number of entries averaged.
 * A is n x n column-major, host or device. */
int tpg_block_means(tpg_ctx* ctx, const double* A, int64_t n, const int32_t* groupIds0, int ngroups, int skip_diag,
                    double* mean, double* count);

/* filter_high_relatedness (R/filter_high_relatedness.R:26-145) on an n x n relatedness matrix (host
 * or device memory, e.g. the KING matrix tpg_pairwise_king left in HBM): keep[i] = 1 for the individuals that pass,
 * in the ORIGINAL order (the reference's third list element); new_order0 (may be NULL) = the order of decreasing mean
 * relatedness the loop walks in (0-based), so that the ids to keep, in the reference's order, are
 * new_order0[k] for the k with keep[new_order0[k]] = 1.  An NA among the compared relatednesses is an error, as in R. */
int tpg_filter_high_relatedness(tpg_ctx* ctx, const double* matrix, int64_t n, double kings_threshold, uint8_t* keep,
                                int32_t* new_order0);

/* Literal per-block mirrors of the three increment_* entry points
 * (src/snp_ibs.cpp:22-74, src/snp_king.cpp:21-74, src/snp_as.cpp:22-67); the scratch matrices of the reference
 * are not needed.  fbm_bytes is the host (mmapped) FBM.  DEFAULT = the reference's semantics: the caller's n x n
 * doubles are incremented when the call returns (an unmodified R driver reads them right after its loop,
 * R/snp_ibs.R:84-95).  Every call uploads the columns of its own block; no copy of the caller's FBM outlives the
 * call, so an FBM that is rewritten in place between analyses (R/gt_impute_simple.R:86) is never read stale.
 * OPT-IN, tpg_increment_defer(ctx, 1): every (K, K2) pair gets device accumulators that live across the calls of the
 * R block loop (R/snp_ibs.R:69-82) and the caller's matrices are incremented by tpg_increment_flush (one line added
 * to the R driver after its loop): one N x N download per analysis instead of per block.  All
 * blocks that accumulate into the same (K, K2) must then pass the same rowInd. */
int tpg_increment_defer(tpg_ctx* ctx, int on);
int tpg_increment_ibs_counts(tpg_ctx* ctx, double* K, double* K2, const uint8_t* fbm_bytes,
                             int64_t nrow, int64_t ncol, const int32_t* rowInd1, int64_t n,
                             const int32_t* colInd1, int64_t m);
int tpg_increment_king_numerator(tpg_ctx* ctx, double* K, double* N_Aa_i, const uint8_t* fbm_bytes,
                                 int64_t nrow, int64_t ncol, const int32_t* rowInd1, int64_t n,
                                 const int32_t* colInd1, int64_t m);
int tpg_increment_as_counts(tpg_ctx* ctx, double* K, double* K2, const uint8_t* fbm_bytes,
                            int64_t nrow, int64_t ncol, const int32_t* rowInd1, int64_t n,
                            const int32_t* colInd1, int64_t m);

/* K += accumulated sums for every pending (K, K2) pair; the device accumulators are released (a no-op unless
 * tpg_increment_defer is on) */
int tpg_increment_flush(tpg_ctx* ctx);
/* release the device scratch the increment_* mirrors keep between calls (an error while increments are pending) */
int tpg_resident_drop(tpg_ctx* ctx);
/* quirk Q1 through the literal mirror (opt-in): the block just passed to tpg_increment_as_counts for the n x n
 * matrix K was one column narrower than the R driver's scratch matrices: +1 on every element, at the flush when K is
 * pending, at once otherwise */
int tpg_increment_as_note_narrow_block(tpg_ctx* ctx, double* K, int64_t n);

/* ---- AMOVA (gt_amova: the analysis of molecular variance of Excoffier, Smouse & Quattro 1992 as Arlequin, pegas, poppr and ade4
 * run it: the squared genotype distances between individuals are partitioned among regions, among populations within regions and
 * within populations, and each Phi is tested by its own permutation scheme.  The reference has nothing of the kind, so everything
 * is defined HERE; the formulas are recalled from Excoffier et al. 1992, not pinned by a run of Arlequin) -------------------------
 * Squared distance, tpg_pairwise_sqdist: with d = dosage - 1, h = heterozygous, v = typed and the accumulators V = vv', D = dd',
 *        A = hv': raw_ij = sum over the loci both i and j are typed at of (d_i - d_j)^2 = 2 V_ij - A_ij - A_ji - 2 D_ij (sum d_i^2 v_j
 *        = V_ij - A_ij), an exact integer, 0 on the diagonal.  type TPG_SQDIST_RAW: raw (m is ignored).  TPG_SQDIST_ADJUSTED:
 *        (raw m) / V_ij -- the product as a 64-bit integer, converted to double, then one IEEE division by (double)V_ij -- NaN
 *        where V_ij = 0; 1 <= m <= 2^30.  Needs TPG_PW_V | TPG_PW_D | TPG_PW_A (TPG_PW_FOR_KING), else TPG_EINVAL.  out: n x n
 *        column-major doubles, host or device memory.
 * Class sums, tpg_class_sums: A is n x n column-major doubles in host or device memory, symmetric or not.  labels is R x n
 *        row-major in host memory, labels[r][i] in {-1, 0 .. nclasses-1}; -1 = individual i is outside labeling r; a class may be
 *        empty.  sums is R x nclasses row-major in host memory: sums[r][c] = sum of A[i + j n] over all ordered pairs (i, j) with
 *        labels[r][i] = labels[r][j] = c, the diagonal included.
 * Order: with C = TPG_CLASSSUM_CHUNK: the partial of row i over chunk k (columns k C .. k C + C - 1) adds the included A[i + j n]
 *        in ascending j from 0.0; t(r, i) adds the chunk partials of row i in ascending k from 0.0 (a chunk without an included
 *        column adds its 0.0); sums[r][c] adds t(r, i) over the rows i of class c in ascending i from 0.0.  IEEE double, no FMA, no
 *        floating-point atomics.  A NaN in A reaches exactly the classes that contain that pair; an empty class gives +0.0.
 *        If A holds integers and every partial sum stays below 2^53, every order gives the exact integer: for raw distances of m
 *        loci that holds when 4 m n^2 < 2^53.  Otherwise a sum is within k 2^-52 sum |x| of the exact sum of its k terms.
 * Determinism: a row of sums depends on A, its own label row and nclasses alone: not on R, on its place in the list, on the
 *        library's internal passes and batches or on launch geometry.  Two calls give the same bits.
 * Limits and errors: 1 <= nclasses <= TPG_CLASSSUM_MAX_CLASSES, 1 <= n <= 2^20, a label outside [-1, nclasses), R < 0:
 *        TPG_EINVAL, nothing written.  R == 0: TPG_OK, nothing written.  The library walks R in internal passes, so its device
 *        scratch (A itself, when it comes from the host, not counted) is bounded independently of R:
 *        tpg_class_sums_scratch_bytes (host only; a bad size: -1).  tpg_classsum_chunk / _tile_rows / _batch: the columns of a
 *        chunk, the rows of a workgroup and the labelings a workgroup carries (TPG_CLASSSUM_*), for tests that place borders.
 * tpg_amova_perm_labels (host only, no context, no GPU): the r-th relabeling as a pure function of its arguments.  pop0[n] in
 *        {-1, 0 .. npop-1} (-1 = outside: stays outside), region_of_pop0[npop] in {0 .. nregion-1}; nregion = 0: no regions, only
 *        scheme 0, region_of_pop0 and region_of_pop_out may be NULL.  With M = tpg_mix64 and 64-bit unsigned arithmetic,
 *        key(u) = M(seed ^ M((r << 32) + u)); a shuffle of a set E = e_0 < e_1 < ... of units: sigma = E sorted by (key, index),
 *        unit sigma_t receives what unit e_t held.  Scheme 0 (tests Phi_ST): E = the individuals with a population, which are
 *        shuffled among the populations -- the rule and, without -1 labels, the bits of tpg_fst_perm_labels scheme 1.  Scheme 1
 *        (Phi_SC): the same inside every region separately, E = that region's individuals: nobody leaves a region.  Scheme 2
 *        (Phi_CT): the populations are the units (u = the population index): population sigma_t receives the region of population
 *        e_t; pop_out = pop0 and region_of_pop_out changes, so region sizes change.  Schemes 0 and 1 copy region_of_pop0.  r = 0
 *        is the identity and is not hashed.  Population sizes are preserved.  An empty population, an empty region, an id out of
 *        range, 0 <= r < 2^31 or n < 2^31 violated: TPG_EINVAL.
 * tpg_amova_from_sums (host only): one relabeling's numbers -> out[21] = df[4], ssd[4], msd[3], ncoef[3], sigma2[4], phi[3], in
 *        IEEE double in the statement order below, without FMA contraction.  n_p = pop_size[p] >= 1, W_p = pop_sum[p] and
 *        R_g = region_sum[g] the class sums, T = total_sum the sum over all ordered included pairs; N = sum n_p, N_g = the
 *        individuals of region g, P = npop, G = nregion; integer sums (N, N_g, sum n_p^2, sum N_g^2) are exact and converted once.
 *        SSD_T = T / (2 N); SSD_WP = W_p / (2 n_p) added over p ascending from 0.0; SSD_WR = R_g / (2 N_g) over g ascending.
 *        x / df is NaN when df = 0.  Rows are (among regions, among populations within regions, within populations, total).
 *        With regions: df = (G - 1, P - G, N - P, N - 1); ssd = (SSD_T - SSD_WR, SSD_WR - SSD_WP, SSD_WP, SSD_T); msd = ssd / df;
 *        S1 = n_p^2 / N_g(p) added over p ascending; ncoef = (n, n', n'') = ((N - S1) / (P - G), (S1 - (sum n_p^2) / N) / (G - 1),
 *        (N - (sum N_g^2) / N) / (G - 1)); s_c = msd_WP; s_b = (msd_AP - s_c) / n; s_a = ((msd_AR - s_c) - n' s_b) / n'';
 *        s_T = (s_a + s_b) + s_c; sigma2 = (s_a, s_b, s_c, s_T); phi = (Phi_CT, Phi_SC, Phi_ST) = (s_a / s_T, s_b / (s_b + s_c),
 *        (s_a + s_b) / s_T).
 *        Without regions (nregion = 0): df = (NaN, P - 1, N - P, N - 1); ssd = (NaN, SSD_T - SSD_WP, SSD_WP, SSD_T);
 *        ncoef = (n_0, NaN, NaN), n_0 = (N - (sum n_p^2) / N) / (P - 1); s_b = (msd_AP - s_c) / n_0; s_T = s_b + s_c;
 *        sigma2 = (NaN, s_b, s_c, s_T); phi = (NaN, NaN, Phi_ST = s_b / s_T).
 *        Negative components and Phi are reported as they come, as Arlequin does.  npop < 1, a population size < 1, a region id
 *        out of range or an empty region: TPG_EINVAL, nothing written.
 * Not offered: PERMANOVA drivers (tpg_class_sums is their kernel), a within-individual level, more than three
 *        levels, tpg_stream_* / tpg_multi_* forms, an R shim entry, distances other than the squared Euclidean one. */
#define TPG_SQDIST_RAW 0
#define TPG_SQDIST_ADJUSTED 1
#define TPG_CLASSSUM_CHUNK 512
#define TPG_CLASSSUM_TILE_ROWS 256
#define TPG_CLASSSUM_BATCH 32
#define TPG_CLASSSUM_MAX_CLASSES 1024
int tpg_pairwise_sqdist(tpg_ctx* ctx, const tpg_pairwise* pw, int type, int64_t m, double* out);
int tpg_class_sums(tpg_ctx* ctx, const double* A, int64_t n, const int32_t* labels, int64_t R, int nclasses, double* sums);
int64_t tpg_class_sums_scratch_bytes(int64_t n, int64_t R, int nclasses);
int64_t tpg_classsum_chunk(void);
int64_t tpg_classsum_tile_rows(void);
int64_t tpg_classsum_batch(void);
int tpg_amova_perm_labels(int64_t n, const int32_t* pop0, int npop, const int32_t* region_of_pop0, int nregion, int scheme,
                          uint64_t seed, int64_t r, int32_t* pop_out, int32_t* region_of_pop_out);
int tpg_amova_from_sums(int npop, const int64_t* pop_size, const double* pop_sum, int nregion, const int32_t* region_of_pop0,
                        const double* region_sum, double total_sum, double* out);

/* ---- Mantel tests (gt_mantel: does genetic distance grow with geographic distance?  The correlation of two distance matrices,
 * tested by permuting the individuals of one of them; the partial test "after controlling for a third matrix"; permutations
 * restricted to strata.  The reference carries coordinates for every individual and has no test that uses them, so everything is
 * defined HERE; it is recalled from Mantel 1967, Smouse, Long & Sokal 1986 and vegan's mantel / mantel.partial, not pinned by a
 * run of vegan) -------------------------------------------------------------------------------------------------------------------
 * The conventions are those of "AMOVA": n x n column-major doubles in host or device memory, IEEE double, no FMA contraction, no
 * floating-point atomics, errors leave the outputs untouched.
 * Cross sums, tpg_mantel_sums: A and the Q matrices B[0 .. Q-1] are n x n, symmetric or not.  perms is R x n row-major in host
 *        memory, every row a permutation pi of 0 .. n-1.  sums is R x Q row-major in host memory: sums[r][q] = the sum over the
 *        ordered pairs i != j of A[pi(i) + pi(j) n] * B_q[i + j n].  The diagonals are never read into a sum: a NaN on a diagonal
 *        changes nothing.  A NaN off the diagonal of A makes every sum NaN, one off the diagonal of B_q makes column q NaN and
 *        no other column.
 * Order: with L = TPG_MANTEL_LANES, the column term c(r, q, j): partial t (0 <= t < L) adds the products for i = t, t + L,
 *        t + 2 L, ... in ascending i from +0.0, each product rounded to double before it is added, i = j skipped; then for
 *        h = L/2, L/4, .., 1: s[t] += s[t + h] for t < h; c = s[0].  sums[r][q] adds c(r, q, j) in ascending j from +0.0.  If A and
 *        B_q hold integers and every partial sum stays below 2^53 every order gives the exact integer; otherwise a sum is
 *        within k 2^-52 sum |x| of the exact sum of its k rounded products.
 * Determinism: sums[r][q] depends on A, B_q and row r of perms alone: not on R, Q, the other matrices, the row's place in the
 *        list, the library's internal passes and batches or launch geometry.  Two calls give the same bits.
 * Limits and errors: 1 <= n <= TPG_MANTEL_MAX_N (a column of A is kept in LDS), 1 <= Q <= TPG_MANTEL_MAX_Q, R >= 0, every
 *        row of perms a bijection (no duplicate, no value out of range; checked on the host before any launch), else TPG_EINVAL
 *        with nothing written.  R == 0: TPG_OK, nothing written.  The library walks R in internal passes, so its device scratch
 *        (the matrices themselves, when they come from the host, not counted) is bounded independently of R:
 *        tpg_mantel_scratch_bytes (host only; a bad size: -1).  tpg_mantel_lanes: L, and tpg_mantel_pass_rows: the permutations
 *        of one internal pass at (n, Q), and tpg_mantel_strides: the strides of L rows a thread of the kernel keeps in flight per
 *        trip of its loop at Q (a bad size: -1 from both), for tests that place borders.  None of them is in the order.  B is declared const double** and not
 *        const double* const*, because the binding's prototype check reads one level of const: nothing is written through
 *        it, and a C caller that holds a const double* const* passes it with a cast.
 * tpg_offdiag_moments: out[0] = S = the sum of a_ij over i != j, out[1] = SS = the sum of a_ij * a_ij, both in the order above
 *        under the identity permutation with b = 1.0 (the product a * 1.0 is a) and b = a.  out is host memory.
 * tpg_offdiag_center: out_ij = a_ij - mean off the diagonal, +0.0 on it; out may be A (in place) or a second matrix, host or
 *        device memory.  A driver centres both matrices by S / N, N = n (n - 1), before it forms the cross sums, so that the
 *        correlation does not cancel on matrices whose entries are all large and positive.
 * tpg_mantel_perms (host only, no context, no GPU): rows r0 .. r0 + R - 1 of the permutation list in ONE call, out R x n; every
 *        row is a pure function of (n, strata, seed, r).  strata0[n] in {0 .. nstrata-1}, or NULL = one stratum.  With M =
 *        tpg_mix64 and 64-bit unsigned arithmetic, key(u) = M(seed ^ M((r << 32) + u)) (the key of tpg_amova_perm_labels); within
 *        a stratum with members e_0 < e_1 < ..., sigma = the members sorted by (key, index) and pi(sigma_t) = e_t: individual
 *        sigma_t takes the row and column that e_t held.  Nobody leaves a stratum.  r = 0 is the identity and is not hashed.
 *        0 <= r < 2^31 violated, a stratum id out of range, R < 0 or n outside the limits: TPG_EINVAL, nothing written.
 * tpg_mantel_from_sums (host only): with N the number of pairs and the moments of both matrices, in IEEE double in this
 *        statement order, without FMA contraction: c = Sab - (Sa * Sb) / N; va = Saa - (Sa * Sa) / N; vb = Sbb - (Sb * Sb) / N;
 *        *out = c / sqrt(va * vb); NaN where va > 0 or vb > 0 does not hold, or N < 1.  Under a permutation of A only Sab changes.
 * tpg_mantel_partial (host only): fa = 1 - r_ac * r_ac; fb = 1 - r_bc * r_bc; (r_ab - r_ac * r_bc) / sqrt(fa * fb); NaN where
 *        fa > 0 or fb > 0 does not hold.  Under a permutation of A r_ab and r_ac change (Q = 2 in one tpg_mantel_sums call) and
 *        r_bc stays.
 * Not offered: n > TPG_MANTEL_MAX_N, Mantel correlograms, PERMANOVA, Kendall's tau, tpg_stream_* / tpg_multi_* forms, an R shim
 *        entry, a rank transform on the device (Spearman's form ranks on the host). */
#define TPG_MANTEL_LANES 256
#define TPG_MANTEL_MAX_N 16384
#define TPG_MANTEL_MAX_Q 4
int tpg_mantel_sums(tpg_ctx* ctx, const double* A, const double** B, int Q, int64_t n, const int32_t* perms, int64_t R, double* sums);
int64_t tpg_mantel_scratch_bytes(int64_t n, int64_t R, int Q);
int64_t tpg_mantel_lanes(void);
int64_t tpg_mantel_pass_rows(int64_t n, int Q);
int64_t tpg_mantel_strides(int Q);
int tpg_offdiag_moments(tpg_ctx* ctx, const double* A, int64_t n, double* out);
int tpg_offdiag_center(tpg_ctx* ctx, const double* A, int64_t n, double mean, double* out);
int tpg_mantel_perms(int64_t n, const int32_t* strata0, int nstrata, uint64_t seed, int64_t r0, int64_t R, int32_t* out);
int tpg_mantel_from_sums(int64_t N, double Sa, double Saa, double Sb, double Sbb, double Sab, double* out);
double tpg_mantel_partial(double r_ab, double r_ac, double r_bc);

/* ---- SNP-block shards over the GPUs of one node -------------------------------------------------
 * The locus axis is the reference's own block axis (R/snp_ibs.R:59-82): a shard is a contiguous range of loci.
 * Per-locus outputs are disjoint slices (no exchange).  What is additive over loci is exchanged by the LIBRARY, over
 * RCCL (xGMI): the int32 pairwise slabs by ONE reduce-scatter -- rank r then finishes band r of the tiles (1 / nranks
 * of the epilogue work and of the output bytes) --, Fst sums, the PCA Gram matrix and the GRM mean by all-reduces of
 * doubles.  With one rank every exchange is the identity: the code path is the same for 1 .. 8 GPUs.
 *
 * One process per GPU (torchrun, mpirun): rank 0 calls tpg_comm_unique_id, the launcher broadcasts the 128 bytes,
 * every rank calls tpg_comm_init_rank with its own context.  One process for all GPUs (an R session): tpg_multi_*. */
int tpg_comm_unique_id(uint8_t* id128);
int tpg_comm_init_rank(tpg_ctx* ctx, int nranks, int rank, const uint8_t* id128, tpg_comm** out);
/* Rehearsal transport (tests): the caller's in-place all-reduce (sum) of `count` elements in HOST memory, dtype 0 =
 * int32, 1 = float64, returning 0 on success -- e.g. torch.distributed over gloo, so that several ranks can share
 * one GPU, which RCCL refuses. */
int tpg_comm_init_host(tpg_ctx* ctx, int nranks, int rank,
                       int (*allreduce)(void* user, void* buf, int64_t count, int dtype), void* user, tpg_comm** out);
void tpg_comm_destroy(tpg_comm* comm);
/* which transport the communicator's collectives run over: "none" (one rank), "host callback" (tpg_comm_init_host), or
 * "rccl: <library name as loaded>" (librccl.so.1 unless TPG_RCCL_LIBRARY names another) */
const char* tpg_comm_transport(const tpg_comm* comm);
int tpg_comm_rank(const tpg_comm* comm);
int tpg_comm_size(const tpg_comm* comm);
/* loci [begin, end) of `rank`: contiguous, boundaries on multiples of 128 loci, sizes differ by at most 128 */
int tpg_shard_loci(int64_t m_total, int nranks, int rank, int64_t* begin, int64_t* end);
/* in-place sum over the ranks of `count` doubles (host or device memory): Fst numerator / denominator sums
 * (tpg_pairwise_pop_fst_sums), the Gram matrix (tpg_pca_gram), the squared Frobenius norm */
int tpg_comm_allreduce_f64(tpg_ctx* ctx, tpg_comm* comm, double* buf, int64_t count);
/* pairwise accumulators laid out for the reduce-scatter; accumulate as usual, then tpg_pairwise_reduce: this rank
 * is left with the complete sums of its band of tiles, and tpg_pairwise_counts / tpg_pairwise_epilogues_sharded write
 * only the part of the N x N outputs the band covers -- rows [row0, row1) x columns [row0, n) and the mirror image
 * rows [row0, n) x columns [row0, row1) (tpg_pairwise_band); the bands of all ranks tile the matrices. */
size_t tpg_pairwise_buffer_bytes_sharded(int64_t n, int nranks);
int tpg_pairwise_create_sharded(tpg_ctx* ctx, const tpg_comm* comm, int64_t n, tpg_pairwise** out);
int tpg_pairwise_reduce(tpg_ctx* ctx, tpg_comm* comm, tpg_pairwise* pw);
/* The same reduction on a SECOND communicator -- one made on another context (= another stream) of the same device, same
 * ranks -- so that the reduce-scatter runs beside what pw's own context enqueues next (in the fused analysis: the PCA's Gram
 * kernels) instead of in front of it.  _begin orders the reduce-scatter behind the accumulate kernels already enqueued on
 * pw's context and returns at once; _end orders pw's context behind the reduce-scatter (nothing may read the accumulators in
 * between).  RCCL orders the operations of ONE communicator, hence the second one; every rank must issue _begin and the
 * collectives of its first communicator in the same order.  Rehearsed over the stream-ordered mock RCCL only:
 * opt-in, nothing in the library calls it by itself. */
int tpg_pairwise_reduce_begin(tpg_ctx* ctx, tpg_comm* side_comm, tpg_pairwise* pw);
int tpg_pairwise_reduce_end(tpg_ctx* ctx, tpg_comm* side_comm, tpg_pairwise* pw);
int tpg_pairwise_band(const tpg_pairwise* pw, int64_t* row0, int64_t* row1);
/* the band rank `rank` of `nranks` gets for n individuals (host arithmetic; no GPU needed) */
int tpg_pairwise_band_of(int64_t n, int nranks, int rank, int64_t* row0, int64_t* row1);
int tpg_pairwise_epilogues_sharded(tpg_ctx* ctx, tpg_comm* comm, const tpg_pairwise* pw, int ibs_type, int64_t m,
                                   double* ibs, double* king, double* allele_sharing, double* grm);
/* gt_pca_partialSVD with the loci sharded over the ranks: `v` holds this rank's loci; center, scale and the rows of
 * the loadings come back for those loci; d and u are the same on every rank (the Gram matrix is summed over the ranks
 * inside, the eigen step is replicated); one rank: identical to tpg_pca_partial_svd */
int tpg_pca_partial_svd_sharded(tpg_ctx* ctx, tpg_comm* comm, const tpg_view* v, int k, double* d, double* u,
                                double* vload, double* center, double* scale, double* square_frobenius);
/* one process, `ndev` GPUs (devices == NULL: 0 .. ndev-1): a context and a communicator (ncclCommInitAll) each */
int tpg_multi_create(int ndev, const int* devices, tpg_multi** out);
void tpg_multi_destroy(tpg_multi* mg);
int tpg_multi_ndev(const tpg_multi* mg);
tpg_ctx* tpg_multi_ctx(tpg_multi* mg, int i);
tpg_comm* tpg_multi_comm(tpg_multi* mg, int i);
/* snp_ibs + snp_king + snp_allele_sharing + pairwise_grm of one HOST FBM on all devices: every device uploads and
 * packs its share of colInd (raw-byte semantics, src/snp_ibs.cpp:47-54), one reduce-scatter, every device writes its
 * band of IBS / KING / allele sharing / GRM straight into the caller's n x n host matrices (any may be NULL).
 * m for TPG_IBS_ADJUSTED_COUNTS is the number of loci kept. */
int tpg_multi_pairwise(tpg_multi* mg, const uint8_t* fbm_bytes, int64_t nrow, int64_t ncol, const int32_t* rowInd1,
                       int64_t n, const int32_t* colInd1, int64_t m, int ibs_type, double* ibs, double* king,
                       double* allele_sharing, double* grm);
/* The other analyses of one HOST FBM on all devices of `mg`, for a caller that is ONE process (an R session): every
 * device uploads and packs its share of colInd (through code256; NULL = raw bytes) and the results land in the
 * caller's arrays (host or device memory).
 *   tpg_multi_grouped_alt_freq: loci_alt_freq of a grouped gen_tibble (R/loci_alt_freq.R:174-197), out m x 2G; with
 *     groupIds0 == NULL the ungrouped form (R/loci_alt_freq.R:328-379), out m x 2.  Per-locus outputs: no exchange.
 *   tpg_multi_pop_fst: pairwise_pop_fst (R/pairwise_pop_fst.R:116-161), arguments as tpg_pairwise_pop_fst; by-locus
 *     rows come from the device that owns the locus, totals from the numerator / denominator sums of all devices.
 *   tpg_multi_pca_partial_svd: gt_pca_partialSVD (R/gt_pca_partialSVD.R:67-108), arguments as tpg_pca_partial_svd;
 *     the Gram matrix is summed over the devices by one all-reduce (RCCL). */
int tpg_multi_grouped_alt_freq(tpg_multi* mg, const uint8_t* fbm_bytes, int64_t nrow, int64_t ncol, const int32_t* rowInd1,
                               int64_t n, const int32_t* colInd1, int64_t m, const double* code256,
                               const int32_t* groupIds0, int ngroups, const double* ploidy, int as_counts, double* out);
int tpg_multi_pop_fst(tpg_multi* mg, const uint8_t* fbm_bytes, int64_t nrow, int64_t ncol, const int32_t* rowInd1, int64_t n,
                      const int32_t* colInd1, int64_t m, const double* code256, const int32_t* groupIds0, int ngroups,
                      const double* ploidy, int method, const int32_t* pairs1, int P, int by_locus, int return_num_dem,
                      double* fst_tot, double* out_a, double* out_b);
int tpg_multi_pca_partial_svd(tpg_multi* mg, const uint8_t* fbm_bytes, int64_t nrow, int64_t ncol, const int32_t* rowInd1,
                              int64_t n, const int32_t* colInd1, int64_t m, const double* code256, int k, double* d,
                              double* u, double* vload, double* center, double* scale, double* square_frobenius);

/* ---- streamed whole analyses: the reference's block loop inside the library ---------------------------------------
 * What defines the reference on this path is that the genotype store is a FILE and is swept in blocks of loci
 * (R/snp_ibs.R:59-82, R/loci_alt_freq.R:351-359, R/gen_tibble_fbm.R:185-194; big_SVD behind
 * R/gt_pca_partialSVD.R:82-89 sweeps it twice).  A tpg_stream is such a store that STAYS ON THE HOST: tpg_stream_run
 * sweeps colInd in blocks of loci, an uploader thread (its own stream) filling one of two block buffers while the kernels
 * of the block before run, and keeps resident only those two blocks of FBM bytes, the packed views of the block at hand
 * and the additive state (pairwise slabs, Gram matrix, Fst sums); per-locus outputs leave block by block (a downloader
 * thread, its own stream) into the caller's arrays.  The PCA's second sweep (the loadings v = Z'u / d) reads the imputed
 * views again if the budget let them stay (n m / 4 bytes), and streams the store a second time otherwise.
 * budget_bytes bounds the HBM taken by FBM bytes + packed views + per-block scratch (0 = no bound: a few large blocks,
 * views kept -- the fastest end-to-end route for a panel that fits); the additive state is not part of it.
 * Results are those of the resident entry points: integer counts bit for bit, FP64 sums in block order. */
typedef struct tpg_stream tpg_stream;
/* the host FBM bytes (e.g. the mmap of bigstatsr's .bk; must stay valid until tpg_stream_close) */
int tpg_stream_open_host(tpg_ctx* ctx, const uint8_t* fbm_bytes, int64_t nrow, int64_t ncol, size_t budget_bytes,
                         tpg_stream** out);
/* <backingfile>.bk, mapped by the library */
int tpg_stream_open_bk(tpg_ctx* ctx, const char* path, int64_t nrow, int64_t ncol, size_t budget_bytes, tpg_stream** out);
/* a PLINK .bed: path (magic checked), or the payload behind its 3-byte magic */
int tpg_stream_open_bed(tpg_ctx* ctx, const char* path, int64_t n, int64_t m, size_t budget_bytes, tpg_stream** out);
int tpg_stream_open_bed_host(tpg_ctx* ctx, const uint8_t* payload, int64_t n, int64_t m, size_t budget_bytes,
                             tpg_stream** out);
/* the synthetic panel of tpg_fbm_synth generated block by block on the device (panels larger than host memory) */
int tpg_stream_open_synth(tpg_ctx* ctx, uint64_t seed, int64_t nrow, int64_t ncol, int npop, uint32_t miss_thresh,
                          int imputed_bytes, size_t budget_bytes, tpg_stream** out);
void tpg_stream_close(tpg_stream* s);

/* What one sweep computes: every output pointer is optional (NULL = not asked for), host or device memory, laid out as
 * the resident entry point of the same name lays it out.  One (rowInd, colInd) selection serves all of them. */
#define TPG_STREAM_MAX_FST 3
typedef struct tpg_stream_job {
  size_t struct_size;     /* sizeof(tpg_stream_job) of the caller's header: this one's, or TPG_STREAM_JOB_SIZE_V1 (a caller
                             built before impute_method existed: the fields behind that size are not read and count as 0) */
  const int32_t* rowInd1; /* NULL = all rows */
  int64_t n;
  const int32_t* colInd1; /* NULL = all columns */
  int64_t m;
  /* snp_ibs / snp_king / snp_allele_sharing / pairwise_grm (raw-byte semantics, src/snp_ibs.cpp:47-54): n x n.  Only
   * the cross-products the requested matrices are made of are accumulated (tpg_pairwise_accumulate_products) */
  int ibs_type;
  double *ibs, *king, *allele_sharing, *grm;
  /* per-locus sweeps through code256 (NULL = raw bytes) */
  const double* code256;
  const double* ploidy;      /* NULL = all diploid */
  const int32_t* groupIds0;  /* needed by the grouped outputs and by Fst */
  int ngroups;
  int as_counts;
  double* alt_freq;            /* m x 2   (tpg_alt_freq_dip_pseudo) */
  double* grouped_alt_freq;    /* m x 2G  (tpg_grouped_alt_freq_dip_pseudo) */
  double* grouped_missingness; /* m x G   (tpg_grouped_missingness) */
  int32_t* loci_counts;        /* m x 4 row-major (tpg_loci_counts) */
  /* pairwise_pop_fst: up to three estimators from one sweep; fst_tot[i] (P, may be NULL) = ratio of the sums over all
   * loci; fst_by_locus[i] (m x P, may be NULL) = the by_locus ratios -- or, with fst_return_num_dem, the numerators, and
   * fst_by_locus_den[i] (m x P) the denominators (R/pairwise_pop_fst.R:103-106) */
  int nfst;
  int fst_method[TPG_STREAM_MAX_FST];
  const int32_t* pairs1; /* 2 x P, 1-based */
  int P;
  int fst_return_num_dem;
  double* fst_tot[TPG_STREAM_MAX_FST];
  double* fst_by_locus[TPG_STREAM_MAX_FST];
  double* fst_by_locus_den[TPG_STREAM_MAX_FST];
  /* gt_pca_partialSVD through code256_pca (e.g. CODE_IMPUTE_PRED); k = 0: no PCA.  pca_tol = 0: the partial SVD's
   * 1e-12, else tpg_pca_random_svd's tolerance */
  const double* code256_pca;
  int k;
  double pca_tol;
  double *d, *u, *v, *center, *scale, *square_frobenius;
  /* TPG_IMPUTE_*: with k > 0 the PCA of every block runs on the imputed raw view (tpg_view_impute; `random` keyed by the
   * position in this job's selection, so every block plan gives the same fill).  code256_pca must then be NULL or CODE_012
   * (TPG_EINVAL otherwise).  The other outputs go on reading the store as it is.  tpg_multi_stream_run: TPG_EUNSUPPORTED. */
  int impute_method;
  uint64_t impute_seed;
} tpg_stream_job;
/* the struct up to and including square_frobenius */
#define TPG_STREAM_JOB_SIZE_V1 (offsetof(tpg_stream_job, square_frobenius) + sizeof(double*))

typedef struct tpg_stream_report {
  int64_t blocks;          /* blocks of the first sweep */
  int64_t block_loci;      /* loci per block (the last one may be narrower) */
  int sweeps;              /* 1, or 2 when the loadings streamed the store again */
  int views_kept;          /* the imputed views stayed in HBM for the loadings */
  size_t bytes_up;         /* host -> device, all sweeps */
  size_t bytes_down;       /* device -> host */
  size_t budget_bytes;     /* as given */
  size_t planned_bytes;    /* what the block plan expects to hold: FBM blocks + views + scratch (<= budget when one was given) */
  size_t state_bytes;      /* additive state (pairwise slabs, Gram matrices, N x N outputs): not part of the budget */
  size_t peak_device_bytes; /* largest growth of the device's used memory over the run (hipMemGetInfo, sampled per block) */
  double seconds;
  double seconds_first_sweep;
} tpg_stream_report;

/* one streamed pass over the store for everything the job asks for; report may be NULL */
int tpg_stream_run(tpg_ctx* ctx, tpg_stream* s, const tpg_stream_job* job, tpg_stream_report* report);
/* The same with the loci sharded over the devices of `mg` ("then stream sub-blocks per GPU"): every device
 * streams its contiguous share of colInd in blocks under the same budget (per device), then one reduce-scatter of the
 * pairwise slabs, all-reduces of the Fst sums and of the Gram matrix, replicated eigen step, each device the loadings of its
 * share.  Outputs must be host memory (device threads write disjoint pieces).  `s` supplies the store and the budget. */
int tpg_multi_stream_run(tpg_multi* mg, tpg_stream* s, const tpg_stream_job* job, tpg_stream_report* report);

/* The QC pass of a store that stays on the host: what qc_report_loci (R/qc_report_loci.R:50-57, 96-107: MAF and missingness
 * from the genotype counts, loci_hwe) and qc_report_indiv (R/qc_report_indiv.R:77-84 over indiv_het_obs,
 * src/gt_ind_hetero.cpp:11-42) need, from ONE sweep with the block plan, the budget accounting, the uploader and downloader
 * threads and the report of tpg_stream_run.  A pass of its own: its result decides the rows and columns of every later
 * pass, and it sets up none of the N x N state.  Every output pointer is optional (NULL = not asked for), host or device
 * memory, laid out as the resident entry point named beside it; integer counts and p-values are those entry points' bit
 * for bit (the exact tests run on the device behind the counts of each block: no count table crosses PCIe on the way).
 * The per-locus outputs leave block by block.  indiv_counts is the one output that is additive over blocks: every block
 * adds its {n1, n2, nNA} per individual to an n x 4 int32 table that stays in HBM (report: state_bytes; sweeps = 1), n0
 * follows from m at the end; m >= 2^31 loci: TPG_EUNSUPPORTED for that output.  A job that asks for nothing, asks for a
 * grouped output without groupIds0 / ngroups >= 1, or has another struct_size: TPG_EINVAL. */
typedef struct tpg_stream_qc_job {
  size_t struct_size;     /* sizeof(tpg_stream_qc_job); any other value: TPG_EINVAL */
  const int32_t* rowInd1; /* NULL = all rows */
  int64_t n;
  const int32_t* colInd1; /* NULL = all columns (a synthetic store: contiguous, as in tpg_stream_run) */
  int64_t m;
  const double* code256;     /* NULL = raw bytes, as in tpg_stream_job */
  const int32_t* groupIds0;  /* needed by the grouped outputs only */
  int ngroups;
  int midp;                /* 0 or 1 */
  int32_t* loci_counts;    /* m x 4 row-major           (tpg_loci_counts) */
  double* hwe_p;           /* m                         (tpg_loci_hwe) */
  int32_t* grouped_counts; /* three m x G, column-major (tpg_grouped_genotype_counts) */
  double* grouped_hwe_p;   /* m x G column-major        (tpg_gt_grouped_hwe) */
  int32_t* indiv_counts;   /* n x 4 row-major {n0,n1,n2,nNA} over the m selected loci (tpg_indiv_counts) */
} tpg_stream_qc_job;
int tpg_stream_qc(tpg_ctx* ctx, tpg_stream* s, const tpg_stream_qc_job* job, tpg_stream_report* report);

/* ---- PCA (gt_pca_partialSVD) ---------------------------------------------- */
/* center / scale of bigsnpr::snp_scaleBinom; TPG_ENUMERIC on a missing value or zero scale */
int tpg_pca_center_scale(tpg_ctx* ctx, const tpg_view* v, double* center, double* scale);
/* Gram matrix K = Z Z' (n x n) accumulated behind bigstatsr::big_SVD
 * (call site R/gt_pca_partialSVD.R:82-89) */
int tpg_pca_gram(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale, double* K);
/* K (device memory, n x n) += Gram matrix of this view's loci: block-by-block accumulation for callers that receive
 * the genotypes in blocks of loci; tpg_sym_eig_topk and tpg_pca_loadings finish the SVD */
int tpg_pca_gram_add(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale, double* K);
/* full partial SVD: d[k], u n x k, v m x k, center[m], scale[m]; square_frobenius may be NULL
 * (R/square_frobenius.R:19-35).  Any k <= n (the eigen solver works on a block of at most 64 vectors: beyond 52
 * components the spectrum is taken in batches of 26 with explicit deflation in between). */
int tpg_pca_partial_svd(tpg_ctx* ctx, const tpg_view* v, int k, double* d, double* u, double* vload,
                        double* center, double* scale, double* square_frobenius);
/* gt_pca_randomSVD (R/gt_pca_randomSVD.R:77-135): the same truncated SVD accepted at the
 * relative residual `tol` of the reference's big_randomSVD / RSpectra path (default there 1e-4):
 * |K u_j - d_j^2 u_j| <= tol * d_1^2 for every returned pair.  This entry forms the n x n Gram matrix K = Z Z' (8 n^2
 * bytes) and iterates on it; tpg_pca_random_svd_op ("PCA by operator products" below) is the same iteration without it. */
int tpg_pca_random_svd(tpg_ctx* ctx, const tpg_view* v, int k, double tol, double* d, double* u, double* vload,
                       double* center, double* scale, double* square_frobenius);
/* The pieces of tpg_pca_partial_svd for SNP-block shards on several GPUs: every rank computes the Gram
 * matrix of its loci (tpg_pca_gram, additive over loci), the N x N partials are summed (one all-reduce),
 * then tpg_sym_eig_topk gives lambda[k] (descending) and U (n x k) of the summed matrix and
 * tpg_pca_loadings the rows of v = Z'u/d that belong to the rank's loci (d = sqrt(lambda)). */
/* K: BOTH triangles filled and bitwise symmetric (K[i + j n] == K[j + i n]; what tpg_pca_gram / tpg_pca_gram_add write): the
 * products K Q read K by rows or by columns, whichever is faster, so a matrix that is symmetric only to rounding, or has one
 * triangle filled, gives the eigenpairs of neither.
 * Contract, for any scale of K from 2^-600 to 2^600 times unit size (residuals are taken relative to lambda_1 before they are
 * squared): |K u_j - lambda_j u_j| <= 1e-12 lambda_1 on acceptance, lambda descending to that tolerance, U orthonormal.
 * k at or above the rank r of K: the k - r trailing values are 0 +- 1e-9 lambda_1 and their vectors an orthonormal basis of a
 * part of the null space, orthogonal to the leading ones; a repeated eigenvalue gets an orthonormal basis of (a part of) its
 * eigenspace.  Beyond 52 components the batches after the first are projected against the vectors already found and accept
 * relative to the first batch's lambda_1 (the residual of a later pair is taken inside the complement of the earlier vectors: in
 * full it can reach sqrt(k) times the tolerance), so the same holds there -- except k = n on a SINGULAR matrix through that route
 * (n > 52), which is not supported: ask for k < n, or for at most the rank. */
int tpg_sym_eig_topk(tpg_ctx* ctx, const double* K, int64_t n, int k, double* lambda, double* U);
int tpg_pca_loadings(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale,
                     const double* U, const double* d, int k, double* vload);
/* replaces fbm256_prod_and_rowSumsSq (src/fbm_prod_and_rowSumSq.cpp:10-47): V m x K,
 * XV n x K, rss[n] */
int tpg_fbm256_prod_and_rowSumsSq(tpg_ctx* ctx, const tpg_view* v, const double* center,
                                  const double* scale, const double* V, int K, double* XV, double* rss);
int tpg_square_frobenius(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale,
                         double* out);
/* out (n x K) [i, k] = sum of Tab[j, k] (m x K) over the loci j at which individual i is typed: the masked sums
 * behind predict(project_method = "least_squares") (R/predict_gt_pca.R:221-228) */
int tpg_fbm256_valid_prod(tpg_ctx* ctx, const tpg_view* v, const double* Tab, int K, double* out);

/* ---- PCA by operator products (gt_pca_randomSVD, R/gt_pca_randomSVD.R:6-7: "linear in time in all dimensions and very
 * memory-efficient"; bigstatsr::big_randomSVD only ever multiplies the scaled matrix by vectors) ------------------------------
 * The scaled matrix Z = (G - 1 center') diag(scale)^-1 of a view (n x m, codes 0 / 1 / 2) as an operator, never as a Gram
 * matrix: the two products on the int8 matrix cores, and the truncated SVD that needs nothing else.  Memory beyond the view
 * is linear in n and in m (tpg_pca_op_scratch_bytes), where tpg_pca_random_svd takes 8 n^2 bytes for the Gram matrix.
 *
 * tpg_pca_zt_prod: W (m x b) = Z'Q, Q n x b.  tpg_pca_z_prod: Y (n x b) = Z W, W m x b.  Column-major, host or device memory,
 *   1 <= b <= 64 (else TPG_EINVAL); a missing genotype in the view or a zero in `scale`: TPG_ENUMERIC, as tpg_pca_center_scale;
 *   n >= 2^24: TPG_EINVAL.
 *   Arithmetic.  The operand -- Q, or W[j, c] / scale[j] -- is rounded to fixed point with ONE binary exponent per column c
 *   (the entry's error is at most 2^-40 times the column's largest magnitude amax_c), the integer products and sums are exact,
 *   the centring term uses the column sums of the ROUNDED operand, and the result is rounded to FP64 once before the centring
 *   term is subtracted (and, for Z'Q, the quotient by scale[j] taken).  So |W - Z'Q|[j, c] <= 2 n 2^-40 amax_c / scale[j] and
 *   |Y - Z W|[i, c] <= 2 m 2^-40 amax_c, plus the few FP64 roundings of the last step (tests/pcaop_ref.py spells them out);
 *   measured, the composition Z (Z'q) is within 2.2e-12 of the FP64 sweeps in norm (1.5e-12 at 5 000 x 1 000 000, 2.1e-12 at
 *   100 000 x 100 000; DESIGN.md 3.17, profiles/pcaop_probe.txt).  A column of zeros gives a
 *   column of exact zeros, a column with a NaN or an infinity a column of NaN.  The bits of a result do not depend on how the
 *   contraction is split over workgroups, and a repeated call returns the same bits.
 *
 * tpg_pca_random_svd_op: the outputs and the acceptance contract of tpg_pca_random_svd -- d[k], u n x k, v m x k, center[m],
 *   scale[m], square_frobenius (may be NULL); |Z Z'u_j - d_j^2 u_j| <= tol d_1^2 for every returned pair, the product taken by
 *   the operator -- without the n x n matrix.  *n_apply (may be NULL): how many times Z Z' was applied to a block.
 *   TPG_EINVAL: k > 52 (more components take the Gram route, whose batches deflate the matrix itself), k > n or m, tol outside
 *   [TPG_PCA_OP_TOL_FLOOR, 1) -- the floor is 100 times the operator's measured relative error (2.1e-10, so 1e-9 as a power of
 *   ten) and not below the 1e-8 the Gram route is tested at: 1e-8 --, n >= 2^24.
 *   Measured (one run): one application to 32 columns 4.5 ms at 5 000 x 1 000 000 where the FP64 sweeps take 27.9;
 *   the whole call at k = 20, tol = 1e-4 75 ms there against the Gram route's 21, and 46 ms against 276 at 40 000 x 100 000.  Not
 *   measured: any spread, the n at which the routes cross at a fixed m, the Gram route at n = 100 000.  TPG_ENUMERIC as tpg_pca_random_svd.  The random start has
 *   a fixed seed: the result is a function of the view alone.
 * tpg_pca_op_scratch_bytes: the device memory a tpg_pca_random_svd_op call plans beyond the view's two layouts (on the 256 CUs
 *   of an MI355X; host only, no context); 0 for arguments the call would refuse.  Doubling n or m at most doubles it, up to the
 *   padding of the tiles. */
#define TPG_PCA_OP_TOL_FLOOR 1e-8
int tpg_pca_zt_prod(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale, const double* Q, int b,
                    double* W);
int tpg_pca_z_prod(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale, const double* W, int b,
                   double* Y);
int tpg_pca_random_svd_op(tpg_ctx* ctx, const tpg_view* v, int k, double tol, double* d, double* u, double* vload,
                          double* center, double* scale, double* square_frobenius, int* n_apply);
size_t tpg_pca_op_scratch_bytes(int64_t n, int64_t m, int k);
/* *fits = 1 when the device memory of the Gram route -- the 8 n^2 bytes of the matrix plus the eigen solver's blocks -- is at most
 * half of the device's free memory at the time of the call, else 0: the rule behind gt_pca_randomSVD(route = "auto"), which takes
 * the operator route only when this says 0.  A rule about what CAN run, not about which route is faster. */
int tpg_pca_gram_route_fits(tpg_ctx* ctx, int64_t n, int k, int* fits);

/* ---- pcadapt (gt_pcadapt, R/gt_pcadapt.R:44-86 around bigsnpr::snp_pcadapt; bigsnpr is not among the reference's sources, so
 * the arithmetic is defined HERE.  Recalled from bigsnpr / pcadapt: the statistic is a robust Mahalanobis distance of the
 * per-locus z-scores of the regression of each locus on the K PCA scores, the robust location / scatter is an OGK estimate,
 * the distance is divided by the genomic-control factor median(dist) / qchisq(0.5, K) and referred to chi-square(K), and U
 * must be orthonormal (bigsnpr checks it with all.equal).  THIS PROJECT'S choices: the degrees of freedom n - K - 1 of the
 * residual variance (a constant factor on z changes nothing downstream), median / MAD as the scale of OGK with two iterations
 * and no reweighting step, the treatment of ties, -0 and non-finite values in a median, every operation order below, and the
 * evaluation of the chi-square tail) ---------------------------------------------------------------------------------------
 * Inputs.  A view of n individuals x m loci, codes 0 / 1 / 2; a missing genotype: TPG_ENUMERIC, as tpg_pca_center_scale
 *   (impute first).  U: n x K column-major, host or device memory.  TPG_EINVAL unless 1 <= K <= TPG_PCADAPT_MAX_K, n - K - 1 >= 1
 *   and max |U'U - I| <= 1e-8 (host, plain double sums in ascending i).
 * 1. z-scores (m x K, column-major).  With the genotype counts n0, n1, n2 of locus j: S1 = n1 + 2 n2, S2 = n1 + 4 n2,
 *   mean_j = S1 / n, tot_j = (n S2 - S1^2) / n (exact integers, one division), beta_jk = sum_i (g_ij - mean_j) U_ik (the FP64
 *   row-scaled sweep of csrc/pca.hip), rss_j = tot_j - sum_k beta_jk^2 (k ascending, each square subtracted in turn),
 *   z_jk = beta_jk / sqrt(rss_j / (n - K - 1)).  tot_j == 0 or rss_j <= 0: the whole row of z is NaN, the locus is INVALID.
 *   Error of the sweep: a sum of n products |d beta_jk| <= n eps ||g_j - mean_j||_2 ||U_k||_2 = n eps sqrt(tot_j) (eps = 2^-53,
 *   first order, whatever the order of the sum or the fusing of its multiply-adds; the rounding of mean_j adds at most
 *   eps mean_j sum_i |U_ik| <= eps 2 sqrt(n)).  Through rss: |d rss_j| <= 2 sum_k |beta_jk| |d beta_jk| + (K + 1) eps tot_j, and
 *   with z = beta sqrt(dof / rss):  |d z_jk| <= |z_jk| (|d beta_jk| / |beta_jk| + |d rss_j| / (2 rss_j)) + 3 eps |z_jk|: the
 *   factor tot_j / rss_j amplifies the relative error of tot_j into that of rss_j.  tests/test_gpu_pcadapt.py evaluates this
 *   bound per cell from the extended-precision route of tests/pcadapt_ref.py.
 * 2. Column statistics, over the FINITE entries of a column only (NaN and +-inf never enter a count or a rank); a value is
 *   read as x + 0.0, i.e. -0 counts as +0.  s = the ascending sort, c = its length:  med = s[(c-1)/2] for odd c,
 *   (s[c/2 - 1] + s[c/2]) / 2 for even c;  mad(x) = med(|x - med(x)|) over the entries whose deviation is finite;
 *   sigma(x) = 1.4826 mad(x).  Exact selections: bit for bit numpy.median of the same values.  c = 0: NaN.
 * 3. Robust distance, OGK (Maronna and Zamar 2002) with median / MAD.  A row of Z with an entry that is not finite is invalid
 *   (its distance is NaN); X(0) = the M' valid rows.  M' < K + 2, or a sigma below that is 0 or not finite: TPG_ENUMERIC.
 *   For t = 1, 2:  s_k = sigma(X_k);  Y_k = X_k / s_k (one division per element);  R_aa = 1,
 *   R_ab = R_ba = (sp sp - sm sm) / 4 with sp = sigma(Y_a + Y_b), sm = sigma(Y_a - Y_b), a < b (each sum or difference rounded
 *   once);  R = E Lambda E' on the host (csrc/host/host_eig.h: host_sym_eig, eigenvalues descending; K = 1: E = 1);
 *   X(t) = W = Y E, W_jk = sum_a Y_ja E_ak, a ascending from +0, no FMA contraction.
 *   Then nu_k = med(W_k), Gamma_k = sigma(W_k)^2 and dist_j = sum_k ((W_jk - nu_k)^2 / Gamma_k), k ascending from +0.
 *   A sign flip of an eigenvector leaves dist unchanged exactly (med(-x) = -med(x)).  K = 1: dist = ((z - med) / sigma)^2 up to
 *   the roundings of the two scalings.  center / cov are nu and diag(Gamma) taken back to the coordinates of Z: a row is
 *   x = B w with B = (D1 E1)(D2 E2), D_t = diag(s of iteration t), so center = B nu, cov = B diag(Gamma) B', in the loop order of
 *   csrc/host/host_pcadapt.h: host_ogk_backmap.
 * 4. Genomic control and p-values.  q50(K) = the root of log Q(K/2, x/2) = log(1/2) by bisection on the host until the ends are
 *   neighbouring doubles (Q by the finite sums for half-integer a, csrc/host/host_pcadapt.h); lambda = med(dist) / q50(K);
 *   stat_j = dist_j / lambda;  log10p_j = log Q(K/2, stat_j / 2) / ln 10 with Q the regularised upper incomplete gamma function:
 *   the series of P and log1p(-P) for x < a + 1, otherwise the modified-Lentz continued fraction and
 *   -x + a ln x - lgamma(a) + ln(cf), so that a stat in the thousands gets a finite log10p.  One function for host and device
 *   (tpg_logq), lgamma(a) from the host.  A NaN in gives a NaN out.
 * Determinism.  Selections are exact; the only atomics are integer counts.  A result depends on the inputs alone. */
#define TPG_PCADAPT_MAX_K 64
/* keys per candidate list of the selection kernel = threads of its workgroup: a bucket of at most this many keys is collected
 * into scratch and finished there (csrc/pcadapt.hip; the tests put their row counts around it) */
#define TPG_SELECT_TILE 1024
int64_t tpg_select_tile(void);
/* The selection primitive on its own.  X: rows x ncols doubles, column-major with leading dimension ld >= rows, host or device
 * memory; med, mad (double[ncols]) and n_finite (int64[ncols], may be NULL; the count of finite entries) host or device.
 * mad = 0 (all finite entries equal) is a result here, not an error.  rows < 2^31. */
int tpg_col_median_mad(tpg_ctx* ctx, const double* X, int64_t rows, int ncols, int64_t ld, double* med, double* mad,
                       int64_t* n_finite);
/* step 1: z (m x K, host or device), n_valid (host, may be NULL) = the number of valid loci; z is written at the end only */
int tpg_pcadapt_zscores(tpg_ctx* ctx, const tpg_view* v, const double* U, int K, double* z, int64_t* n_valid);
/* step 3 on any m x K matrix Z (column-major, host or device): dist[m] (host or device); center[K], cov[K x K] and
 * basis[2 K K] (E of the first, then of the second iteration, column-major) in host memory, each may be NULL; n_valid (host,
 * may be NULL) = M' */
int tpg_robust_dist_ogk(tpg_ctx* ctx, const double* Z, int64_t m, int K, double* dist, double* center, double* cov,
                        double* basis, int64_t* n_valid);
/* out[i] = log10 of the upper tail of chi-square(df) at x[i] (host or device memory, count entries); df >= 1 */
int tpg_pchisq_log10_upper(tpg_ctx* ctx, const double* x, int64_t count, int df, double* out);
/* host only: the median of chi-square(df) */
int tpg_qchisq_median(int df, double* out);
/* The whole scan: steps 1 - 4.  z (m x K, may be NULL), dist, stat, log10p (m each) host or device; gc_lambda and n_valid host,
 * may be NULL.  Bit for bit the three staged calls.  Nothing of the caller's is written before the end. */
int tpg_pcadapt(tpg_ctx* ctx, const tpg_view* v, const double* U, int K, double* z, double* dist, double* stat, double* log10p,
                double* gc_lambda, int64_t* n_valid);

/* ---- autoSVD (gt_pca_autoSVD, R/gt_pca_autoSVD.R around bigsnpr::snp_autoSVD; bigsnpr, bigutilsr and robustbase are not among
 * the reference's sources, so the arithmetic is defined HERE.  Recalled from those packages: clump, compute the SVD, take the
 * square root of a robust Mahalanobis distance of the loadings, smooth it with a Gaussian rolling mean per chromosome, call
 * outliers by a Tukey fence that is corrected for skewness by the medcouple and for multiplicity by Bonferroni, remove them,
 * repeat.  THIS PROJECT'S choices: the OGK distance of "pcadapt" as the robust distance, the medcouple as an exact selection
 * over the ratios b / a (below) instead of the kernel values (a - b) / (a + b), every order, tie rule and evaluation below ----
 * Inputs.  A view of n x m, codes 0 / 1 / 2; a missing genotype: TPG_ENUMERIC, as for the PCA.  chrom[m], int32, every
 *   chromosome one contiguous run (else TPG_EINVAL).  hi[m]: the window of "LD clumping"; NULL skips clumping.  k in
 *   [1, TPG_PCADAPT_MAX_K], thr_r2, roll_size in [0, 1024], alpha_tukey in (0, 1), min_mac >= 0, max_iter >= 0.
 * 0. MAC filter.  mac_j = min(Sx_j, 2 n - Sx_j); loci with mac_j < min_mac are excluded (min_mac = 0: none; a monomorphic
 *   locus then fails in the PCA as it does there).
 * 1. Clumping.  tpg_ld_clump(v, hi, thr_r2, S = NULL, exclude = step 0); without hi the kept set is the complement of step 0.
 * 2. Loop, iter = 0.  iter += 1; the SVD of the kept loci, exactly tpg_pca_partial_svd on a view of those loci.  iter > max_iter:
 *   stop, converged = 0.  Otherwise steps 3 - 5 on V (m_keep x k); no outlier: stop, converged = 1; else remove the outliers and
 *   repeat.  The SVD returned is that of the final kept set; at most max_iter + 1 SVDs are computed.
 * 3. Statistic.  S_j = sqrt(dist_j), dist = tpg_robust_dist_ogk(V).  A dist that is not finite: TPG_ENUMERIC.
 * 4. Rolling mean per chromosome segment of the kept loci.  Radius R = roll_size, len = 2 R + 1; R = 0: S2 = S.  A segment
 *   shorter than len: TPG_EINVAL ("roll_size exceeds the number of variants on at least one chromosome").  Weights (host):
 *   a = 3/8 if len <= 10 else 1/2;  p1 = (1 - a) / (len + 1 - 2 a);  L = qnorm_upper(p1);  t_i = -L + i (2 L / (len - 1)),
 *   i = 0 .. len - 1;  w_i = exp(-(t_i t_i) / 2) / sqrt(2 pi).  S2_j = (sum w_i x_{j-R+i}) / (sum w_i), both sums over the i whose
 *   locus lies inside the segment, i ascending from +0, no FMA contraction, one division.
 *   qnorm_upper(p) = the root x of 0.5 erfc(x / sqrt 2) = p by bisection on [-40, 40] on the host until the ends are
 *   neighbouring doubles; the upper end (csrc/host/host_autosvd.h).
 * 5. Fence (tukey_mc_up) over the c finite values of S2, read as x + 0.0; s = the ascending sort; c < 2^31.
 *   Quartiles (R's type 7): Q(p) = s[lo] + (h - lo)(s[lo + 1] - s[lo]), h = (c - 1) p, lo = floor(h) (lo + 1 capped at c - 1);
 *   Q1 = Q(0.25), Q3 = Q(0.75).  Median: the rule of "pcadapt" step 2.
 *   Medcouple: z_i = x_i - med (one rounding; every z must be finite), A = {z > 0}, B = {|z| : z <= 0} ascending, the k values
 *   with z = 0 first; n+ = |A| + k, n- = |B|, N = n+ n- (int64).  The multiset of N ratios in [0, +inf]: r = b / a (one
 *   correctly rounded division) for every a in A and b in B; +inf for each of the k zero rows against every b > 0; for the k x k
 *   ties at the median k (k - 1) / 2 ratios 0, k ratios 1 and k (k - 1) / 2 ratios +inf (robustbase's sign(k - 1 - i - j)
 *   kernel).  With r_lo, r_hi the ratios of ascending ranks (N - 1) / 2 and N / 2:  mc = (g(r_lo) + g(r_hi)) / 2,
 *   g(r) = (1 - r) / (1 + r), g(+inf) = -1.  c = 0: NaN.  b / a is non-decreasing in b and non-increasing in a after rounding, so
 *   the ratios <= t of a row are a prefix of B: the count of ratios <= t is exact in O(c log c), and the two ranks are found by
 *   bisection over the 63-bit pattern of t on the device.  The n+ x n- values are never formed.
 *   Coefficient: coef = (qnorm_upper(alpha / c) - z75) / (2 z75), z75 = qnorm_upper(0.25) (Tukey's 1.5 for alpha / c = 0.0035).
 *   Fence: thr = Q3 + coef (Q3 - Q1) exp(3 mc) if mc >= 0, else with exp(4 mc); on the host, in that order.
 *   Outliers: S2_j > thr, strictly.
 * Determinism.  Selections and counts are exact integers; the only atomics are integer counts. */
/* the view of loci idx0[count] (int64, 0-based, host or device memory; any order, duplicates allowed) of another view -- also
 * of one that no store can re-pack (tpg_view_impute).  Indistinguishable from a view packed from the store with those columns.
 * An index outside [0, m) or count < 1: TPG_EINVAL. */
int tpg_view_select_loci(tpg_ctx* ctx, const tpg_view* v, const int64_t* idx0, int64_t count, tpg_view** out);
/* host only: qnorm_upper(p), 0 < p < 1 */
int tpg_qnorm_upper(double p, double* x);
/* host only: the 2 radius + 1 weights of step 4 (radius 0: the single weight 1); radius in [0, 1024] */
int tpg_rollmean_weights(int radius, double* w);
/* step 4 on its own.  x / out: m doubles, host or device memory (may be the same array); seg_start: nseg + 1 increasing int64,
 * seg_start[0] = 0, seg_start[nseg] = m: segment s covers [seg_start[s], seg_start[s + 1]) */
int tpg_rollmean_segments(tpg_ctx* ctx, const double* x, int64_t m, const int64_t* seg_start, int64_t nseg, int radius,
                          double* out);
/* the medcouple of the finite values of x[count] (host or device memory); mc on the host */
int tpg_medcouple(tpg_ctx* ctx, const double* x, int64_t count, double* mc);
/* step 5 on its own: report[TPG_TUKEY_REPORT_DOUBLES] (host) = {n_finite, q1, q3, med, mc, coef, thr} */
#define TPG_TUKEY_REPORT_DOUBLES 7
int tpg_tukey_mc_up(tpg_ctx* ctx, const double* x, int64_t count, double alpha, double* report);
/* Steps 0 - 5.  *out: the result, owned by the library until tpg_autosvd_free.  chrom and hi host or device memory.  S, S2, the
 * sort, the fence, the compaction of the kept list and the sub-view stay on the device; V passes through host memory once per
 * iteration (m_keep x k doubles down with the SVD, up again for the distance). */
int tpg_pca_auto_svd(tpg_ctx* ctx, const tpg_view* v, const int32_t* chrom, const int64_t* hi, int k, double thr_r2, int roll_size,
                     double alpha_tukey, int64_t min_mac, int max_iter, void** out);
int64_t tpg_autosvd_count(const void* r); /* kept loci */
int tpg_autosvd_iters(const void* r);     /* SVDs computed */
int tpg_autosvd_converged(const void* r);
/* host memory, any may be NULL: d[k], u n x k, vload count x k, center[count], scale[count], idx0[count] (ascending loci of the
 * view) */
int tpg_autosvd_fetch(const void* r, double* d, double* u, double* vload, double* center, double* scale, int64_t* idx0,
                      double* square_frobenius);
/* detection pass iter (0-based; there are tpg_autosvd_iters of them, one fewer when the loop stopped at max_iter): the size of
 * its kept list, its number of outliers and its fence report */
int tpg_autosvd_history(const void* r, int iter, int64_t* n_kept, int64_t* n_outliers, double* report);
/* its outliers, n_outliers each, any may be NULL: position in that pass's kept list, locus of the view */
int tpg_autosvd_outliers(const void* r, int iter, int64_t* pos0, int64_t* idx0);
/* its runs of at least min_size outliers that are consecutive in that pass's kept list and lie on one chromosome, as loci of
 * the view (first, last); at most n_outliers / min_size of them; first0 / last0 may be NULL (count alone) */
int tpg_autosvd_intervals(const void* r, int iter, int64_t min_size, int64_t* first0, int64_t* last0, int64_t* count);
void tpg_autosvd_free(void* r);

/* ---- k-means on PCA scores (gt_cluster_pca, R/gt_cluster_pca.R:78-170 around stats::kmeans; stats::kmeans is Hartigan-Wong
 * driven by R's random generator, neither part of the reference's sources nor reproducible, so what is computed is defined
 * HERE: Lloyd's algorithm from seeded start rows, NOT PINNED BY THE REFERENCE) ------------------------------------------------
 * Data.  X is n x d doubles, column-major (x_ij at X[i + j n]), host or device memory, every entry finite (else TPG_ENUMERIC).
 * A run is (k, seed), 1 <= k <= n.  Its centres are a k x d column-major block (centre c, coordinate j at c + j k).
 * Start.  With M = tpg_mix64 (see "simple imputation") and 64-bit unsigned arithmetic, h_i = M(seed ^ M(i)), i = 0 .. n - 1.
 *   The start rows are the k rows with the smallest (h_i, i) in that order: centre c is the row with the c-th smallest key.
 *   A pure function of (seed, n, k): tpg_kmeans_start (csrc/host/host_kmeans.h).  With centers0 the given centres are the start.
 * Assign.  D(i,c) = sum_j (x_ij - c_j)^2 in the direct form: from +0, j ascending, t = x_ij - c_j (one rounding), then
 *   D = fma(t, t, D).  Point i goes to the centre with the smallest D(i,c); on equal D the smaller c wins (a scan in ascending c
 *   that replaces the best on strictly smaller only).
 * Update.  A centre becomes the mean of its points: per coordinate the sum over its points in ASCENDING i, one after the other
 *   from +0 (plain additions), then one division by (double)count.  A centre that owns no point keeps its position.
 * Iterate.  Iteration t = 1, 2, ... is an assign, then an update with the new labels.  Before iteration 1 every label is -1, so
 *   the first assign changes every label.  A run has converged when an assign changes no label (its update is then skipped: it
 *   would reproduce the same centres bit for bit); n_iter counts assigns; a run that has not converged after max_iter assigns
 *   stops after the update of iteration max_iter (converged = 0).  Either way the returned centres are the means of the returned
 *   labels, except for centres that own no point; n_empty is the number of those under the returned labels.
 * WSS.  e_i = D(i, label(i)) under the returned centres, formed as in Assign.  The n values are padded with +0 to a multiple of
 *   TPG_KMEANS_TILE; a tile of TPG_KMEANS_TILE consecutive points is summed by halving (for s = TILE/2, TILE/4, .. 1:
 *   e[l] += e[l + s] for l < s); the tile sums are added in ascending tile order from +0.  What compute_wss of
 *   R/gt_cluster_pca.R recomputes, in a stated order.  tpg_kmeans_step returns this sum for its own assign: the smallest D(i,.)
 *   of every point under C_in.
 * Batch.  R runs in one call.  A run's result is a function of (X, n, d, k, seed or centers0, max_iter) alone: it does not depend
 *   on the other runs of the batch, and two calls give the same bits.  There are no floating-point atomics; the integer atomics
 *   count labels that changed and points per centre.  Runs that have stopped leave the list of live runs on the device and cost
 *   nothing further; the host reads one integer (the number of live runs) per iteration.
 * Centres pass through LDS in chunks of floor(TPG_KMEANS_CHUNK_DOUBLES / d) centres (csrc/kmeans.hip); the chunking does not
 *   enter the arithmetic.
 * Rounding bounds (u = 2^-53; eps = 2 u covers the second-order terms for every n, d inside the limits; A = max |x_ij|):
 *   a computed D differs from the exact one of the same operands by at most (d + 2) eps D: d fused terms, all non-negative,
 *     and one subtraction each;
 *   a centre coordinate, a mean of at most n values of magnitude at most A in any order of addition:
 *     bound_centre = n eps A;
 *   wss under exact centres, n non-negative terms in any order: (n + d + 2) eps wss; centres off by delta move each e_i by at most
 *     2 d (2 A) delta + d delta^2, so with delta = bound_centre
 *     bound_wss = (n + d + 2) eps wss + n d (4 A + bound_centre) bound_centre.
 *   Two evaluations (the device's and a restatement's) of the same labels differ by at most twice these.
 * Limits.  1 <= n <= TPG_KMEANS_MAX_N, 1 <= d <= TPG_KMEANS_MAX_D, 1 <= k <= min(n, TPG_KMEANS_MAX_K), 1 <= R <=
 *   TPG_KMEANS_MAX_RUNS, max_iter >= 1; outside them TPG_EINVAL.  After an error every output is untouched.
 * Out of scope: other starts (k-means++), k-means inside tpg_stream_* / tpg_multi_*.  (method = "ward" of the reference: "Ward
 *   clustering on PCA scores" below.) */
#define TPG_KMEANS_MAX_N 16777216
#define TPG_KMEANS_MAX_D 64
#define TPG_KMEANS_MAX_K 1024
#define TPG_KMEANS_MAX_RUNS 65535
#define TPG_KMEANS_TILE 256
#define TPG_KMEANS_CHUNK_DOUBLES 4096
int64_t tpg_kmeans_chunk_doubles(void); /* TPG_KMEANS_CHUNK_DOUBLES of the library as built */
/* host only: idx[k] = the start rows (0-based) */
int tpg_kmeans_start(uint64_t seed, int64_t n, int k, int32_t* idx);
/* one assign and one update from C_in (k x d): labels[n] (0-based), C_out (k x d, may be NULL), counts[k] (may be NULL) and wss
 * (one double, the value under C_in and the new labels, may be NULL); every pointer host or device memory */
int tpg_kmeans_step(tpg_ctx* ctx, const double* X, int64_t n, int d, int k, const double* C_in, int32_t* labels, double* C_out,
                    int32_t* counts, double* wss);
/* R runs.  k[R] and seed[R] (the seeds' 64 bits, read as unsigned); centers0 NULL or the start centres of every run, run r's
 * k_r x d block at offset d (k_0 + .. + k_{r-1}); labels n x R column-major int32 (0-based); centers (may be NULL) laid out as
 * centers0; wss, n_iter, converged, n_empty: R values each, any may be NULL.  Every pointer host or device memory. */
int tpg_kmeans_batch(tpg_ctx* ctx, const double* X, int64_t n, int d, int R, const int32_t* k, const int64_t* seed, int max_iter,
                     const double* centers0, int32_t* labels, double* centers, double* wss, int32_t* n_iter, int32_t* converged,
                     int32_t* n_empty);

/* the WSS of R given labellings in one call: labels n x R column-major int32 (0-based, labelling r in [0, k[r]), else
 * TPG_EINVAL), k[R], wss[R]; counts (may be NULL) the points per label, labelling r's k_r entries at offset k_0 + .. + k_{r-1}.
 * The centres are the means of the labels by the "Update" rule (a label that owns no point has no centre and enters nothing), e_i
 * is formed as in "Assign" and summed as in "WSS": no arithmetic of its own, so the labels a run of tpg_kmeans_batch returned
 * give that run's wss bit for bit, and bound_wss holds as for such a run.  Limits as tpg_kmeans_batch.  Every pointer host or
 * device memory. */
int tpg_cluster_wss(tpg_ctx* ctx, const double* X, int64_t n, int d, int R, const int32_t* k, const int32_t* labels, double* wss,
                    int32_t* counts);

/* ---- Ward clustering on PCA scores (method = "ward" of gt_cluster_pca, R/gt_cluster_pca.R:156-166: for every k,
 * cutree(hclust(dist(x)^2, method = "ward.D2"), k); stats::hclust is not among the reference's sources, so the arithmetic is
 * defined HERE, NOT PINNED BY AN R RUN.  The tree does not depend on k: one tree is built and cut at every k) -----------------
 * ward.D2 squares its input before the Lance-Williams recurrence and takes the root of the heights afterwards, so the reference
 *   runs Ward's recurrence on d^4: power = 2.  The proper criterion (each merge the one of least growth of the within-group sum
 *   of squares) runs it on d^2: power = 1.
 * Data.  X is n x d doubles, column-major, host or device memory, every entry finite (else TPG_ENUMERIC).  1 <= n <=
 *   TPG_HCLUST_MAX_N (the full matrix is 8 n^2 bytes, 8 GiB there), 1 <= d <= TPG_KMEANS_MAX_D, power in {1, 2}; outside these
 *   limits TPG_EINVAL, before anything is allocated.  After an error every output is untouched.
 * Start.  D2(i,j) in the direct form of "Assign" above: from +0, coordinates ascending, t = x_i - x_j (one rounding),
 *   D2 = fma(t, t, D2).  S(i,j) = D2 for power 1, S(i,j) = D2 * D2 (one rounding) for power 2.  S is symmetric by construction.
 * Clusters.  Every point is a cluster of size 1 whose slot is its index; a cluster's slot is always the smallest index among its
 *   members.
 * Step s = 1 .. n - 1.  Among the live pairs a < b the one of smallest S(a,b) merges; on equal S the smallest a wins, then the
 *   smallest b.  merge_a[s-1] = a, merge_b[s-1] = b, height[s-1] = S(a,b).  For every other live c, the sizes converted to double:
 *     p = (n_a + n_c) S(a,c),  q = (n_b + n_c) S(b,c),  r = n_c S(a,b),  S(a,c) = S(c,a) = ((p + q) - r) / ((n_a + n_b) + n_c),
 *   every operation rounded once, nothing fused.  Then n_a += n_b and b is dead.
 * Cut at k.  The first n - k merges are applied; the clusters are labelled 0, 1, .. in the order in which they first appear in
 *   ascending i (cutree's numbering: the rank of the cluster's slot).  The cut goes by step number, not by height: a height may
 *   come out an ulp below its predecessor.
 * WSS of a labelling: tpg_cluster_wss above.
 * Relation to R.  hclust$height = sqrt(height).  hclust$merge (tpg_hclust_r_merge): -(i + 1) for point i on its own, the 1-based
 *   step number for a cluster, a singleton before a cluster, of two singletons the smaller point and of two clusters the earlier
 *   step first.  hclust$order: tpg_hclust_order below.
 * No random generator, no floating-point atomic: the result is a pure function of (X, power), two calls give the same bits.
 * Other linkages, a distance matrix as input and order: "Trees from a pairwise matrix" below.
 * Out of scope: plots, Ward inside tpg_stream_* / tpg_multi_*. */
#define TPG_HCLUST_MAX_N 32768
/* merge_a, merge_b (int32) and height: n - 1 entries each (0-based slots), host or device memory; n = 1 writes nothing */
int tpg_hclust_ward(tpg_ctx* ctx, const double* X, int64_t n, int d, int power, int32_t* merge_a, int32_t* merge_b, double* height);
/* the same, and list_len[n - 1] (may be NULL): list_len[s] = the rows whose nearest neighbour was searched again between
 * step s and step s + 1 of the device's nearest-neighbour list (list_len[0] = n, the first fill): a diagnostic of
 * tools/hclust_probe.py, no part of the definition */
int tpg_hclust_ward_trace(tpg_ctx* ctx, const double* X, int64_t n, int d, int power, int32_t* merge_a, int32_t* merge_b,
                          double* height, int32_t* list_len);
/* host only: labels n x R column-major (0-based), column r the cut at k[r] clusters.  TPG_EINVAL (nothing written) for a k
 * outside [1, n] and for a merge list with a step that does not name two live slots a < b */
int tpg_hclust_cut(int64_t n, const int32_t* merge_a, const int32_t* merge_b, int R, const int32_t* k, int32_t* labels);
/* host only: merge (n - 1) x 2 int32 column-major, R's convention */
int tpg_hclust_r_merge(int64_t n, const int32_t* merge_a, const int32_t* merge_b, int32_t* merge);

/* ---- Trees from a pairwise matrix (the order function of the reference's heatmap_pairwise() and heatmap_add_dendro(),
 * function(x) stats::hclust(stats::as.dist(x)), and the neighbour-joining tree users draw from the same matrices;
 * stats::hclust and ape are not among the reference's sources, so the arithmetic is defined HERE, RECALLED, NOT PINNED BY AN R
 * RUN) ------------------------------------------------------------------------------------------------------------------------
 * Input, common to tpg_hclust_dist and tpg_nj.  D is n x n doubles, column-major, host or device memory.  The value of the pair
 *   {i, j}, i < j, is D[j + i n]: the strict lower triangle, as as.dist reads it.  The diagonal and the upper triangle are never
 *   read (diag(m) <- NA is harmless, an asymmetric matrix is accepted).  Every entry of the strict lower triangle is finite, else
 *   TPG_ENUMERIC and nothing is written; negative values are allowed.  1 <= n <= TPG_HCLUST_MAX_N, else TPG_EINVAL before
 *   anything is allocated.  D is never modified: the working matrix S is a scratch copy, full and symmetric, 8 n^2 bytes.
 * tpg_hclust_dist.  Slots, outputs and tie rule as tpg_hclust_ward: 0-based slots, a < b at every step, slot a survives (a
 *   cluster's slot is its smallest member), n - 1 entries, n = 1 writes nothing.  At each step the merged pair is the
 *   lexicographic minimum of (S(a,b), a, b) over the live pairs a < b; height[s] is that S, no root taken.  Then for every other
 *   live c, with x = S(a,c), y = S(b,c) and the sizes n_a, n_b, n_c from before the merge converted to double, in FP64, every
 *   operation rounded once, nothing fused:
 *     TPG_LINK_SINGLE   0                      S(a,c) = y where y < x, else x
 *     TPG_LINK_COMPLETE 1 (hclust's default)   S(a,c) = y where y > x, else x
 *     TPG_LINK_AVERAGE  2 (UPGMA)              p = n_a x,  q = n_b y,  S(a,c) = (p + q) / (n_a + n_b)
 *     TPG_LINK_MCQUITTY 3 (WPGMA)              S(a,c) = (x + y) 0.5
 *     TPG_LINK_WARD     4 (ward.D on D as given)   the recurrence of "Ward clustering on PCA scores" above, unchanged
 *   and S(c,a) = S(a,c); n_a += n_b and b is dead.  Any other method: TPG_EINVAL.  ward.D2 is the caller's business: square the
 *   input, take the root of the heights.
 * tpg_hclust_order (host only): hclust$order, 0-based, recalled from hcass2, not pinned.  With R's merge matrix as
 *   tpg_hclust_r_merge makes it, leaves(row) = leaves(first column) followed by leaves(second column), a negative entry is that
 *   single point, order = leaves(last row).  n = 1 gives [0].  A merge list that tpg_hclust_cut would refuse: TPG_EINVAL, nothing
 *   written.
 * tpg_nj: neighbour-joining (Saitou & Nei 1987 in Studier & Keppler's form; recalled, not pinned by a run of ape).
 *   State: the live slots, r of them; S; one row sum R_i per live slot.
 *   Start: R_i = sum of S(i,j) over j != i, ascending j, from +0.0, one addition per j.
 *   While r > 2 (join s = 0 .. n - 3), every operator one rounded FP64 operation, left to right:
 *     q(a,b) = ((double)(r - 2) S(a,b) - R_a) - R_b for the live a < b; the join is the lexicographic minimum of (q, a, b); a
 *       NaN q never wins.
 *     d = S(a,b);  len_a[s] = 0.5 d + (R_a - R_b) / (2.0 (double)(r - 2));  len_b[s] = d - len_a[s].
 *     For every other live c, x = S(a,c), y = S(b,c):  t = ((x + y) - d) 0.5;  R_c = ((R_c - x) - y) + t;  S(a,c) = S(c,a) = t.
 *     R_a = ((R_a + R_b) - (double)r d) 0.5 with the R_a, R_b and r of before the join: the exact algebraic identity for the sum
 *       of the t, so that no reduction and no summation order enters.  Slot a holds the new node, slot b is dead, r -= 1.
 *   End: the two slots left are x < y; last = (x, y, S(x,y)), three doubles.  join_a, join_b, len_a, len_b: n - 2 entries; n = 2
 *     writes only last; n = 1 writes nothing.  Branch lengths may come out negative and are returned as they are.
 *   The row sums are UPDATED, not recomputed: in the numpy restatement they drift from recomputed sums by 3e-13 relative at
 *     n = 301.  The definition is the updated sums.
 *   A step that finds no pair (every q NaN after an overflow): TPG_ENUMERIC, nothing written.
 * tpg_nj_edges (host only): the tree in ape's phylo layout, recalled, not pinned; n >= 3, else TPG_EINVAL.  Tips are 1 .. n, the
 *   node of join s is 2n - 2 - s, so the last join is the root n + 1 and Nnode = n - 2.  The root has three children: its a-child,
 *   its b-child and the node of the other slot left (one of the two slots left is always the last join's), at length last[2].
 *   2n - 3 edges; edge is (2n - 3) x 2 int32 column-major (parent, child), in preorder from the root, a-child before b-child
 *   before the third; edge_length alike.  A join list that names a dead slot, a pair outside 0 <= a < b < n, or a last that does
 *   not name the two slots left: TPG_EINVAL, nothing written.
 * No random generator, no floating-point atomic: every result is a pure function of the lower triangle (and method).
 * Out of scope: an R shim entry, the forwarding of gt_cluster_pca(method = "ward"), centroid and median linkage (not monotone),
 *   bootstrap support of a tree over locus blocks, BIONJ / FastME, rooting and plotting, trees inside tpg_stream_* / tpg_multi_*. */
#define TPG_LINK_SINGLE 0
#define TPG_LINK_COMPLETE 1
#define TPG_LINK_AVERAGE 2
#define TPG_LINK_MCQUITTY 3
#define TPG_LINK_WARD 4
int tpg_hclust_dist(tpg_ctx* ctx, const double* D, int64_t n, int method, int32_t* merge_a, int32_t* merge_b, double* height);
int tpg_hclust_order(int64_t n, const int32_t* merge_a, const int32_t* merge_b, int32_t* order);
int tpg_nj(tpg_ctx* ctx, const double* D, int64_t n, int32_t* join_a, int32_t* join_b, double* len_a, double* len_b, double* last);
int tpg_nj_edges(int64_t n, const int32_t* join_a, const int32_t* join_b, const double* len_a, const double* len_b, const double* last,
                 int32_t* edge, double* edge_length);

/* ---- DAPC (gt_dapc, R/gt_dapc.R:137-255 around MASS::lda(XU, pop, tol = 1e-30) and predict(); MASS is not among the
 * reference's sources, so the discriminant analysis is defined HERE, RECALLED FROM MASS, NOT PINNED) ---------------------------
 * X is n x d column-major (the first n_pca PCA scores), grp0[n] the 0-based group in [0, G).
 *   n_g = the group count, pi_g = n_g / n, mu_g = the group mean, mu = sum_g pi_g mu_g (g ascending).
 *   W = (1 / (n - G)) sum_i (x_i - mu_g(i)) (x_i - mu_g(i))',   B = (1 / (G - 1)) sum_g n_g (mu_g - mu) (mu_g - mu)'.
 *   W = R'R (Cholesky, R upper); a pivot R_jj^2 <= 2^-40 T_jj, T_jj = sum_i (x_ij - mu_j)^2 / (n - 1) the total variance of the
 *   variable -- a variable that is constant within the groups up to rounding, or a linear combination of the others there,
 *   where MASS stops -- is TPG_ENUMERIC.  M = R^-T B R^-1 = E diag(lambda) E' (the symmetric
 *   eigen-decomposition of csrc/host/host_eig.h, lambda descending).  scaling S = R^-1 E, so S'WS = I and S'BS = diag(lambda);
 *   svd = sqrt(max(lambda, 0)).  L = #{svd^2 > 1e-10} among the first min(d, G - 1) (R/gt_dapc.R:189); S, svd and eig keep L
 *   columns.
 *   Sign (this project's choice; MASS fixes none): the entry of largest magnitude of each column of S is positive, on equal
 *   magnitudes the smaller row decides.
 *   n_da = min(asked, G - 1, d, L) (at least 1, else TPG_ENUMERIC: no discriminant function separates the groups).
 *   ind.coord = (X - 1 mu') S[:, :n_da];  grp.coord = its group means;  m_g = (mu_g - mu)' S[:, :n_da].
 *   posterior: q_ig = 0.5 ||z_i - m_g||^2 - ln pi_g over the n_da coordinates, p_ig = exp(-(q_ig - min_g q_ig)) / (the sum of
 *   these over g, g ascending);  assign_i = the g of smallest q_ig, on a tie the smaller g.
 *   eig = svd^2 (all L);  loadings = S[:, :n_da].
 * var of gt_dapc is sum d[:n_pca] / sum d over the singular values d of the PCA object -- of d, not of d^2, R/gt_dapc.R:182
 *   verbatim -- and is formed in Python.
 * Errors: G < 2, an empty group, n <= G, d outside [1, 64], a label outside [0, G): TPG_EINVAL.  A non-finite x: TPG_ENUMERIC.
 * Per-locus loadings (R/gt_dapc.R:246-255): var_load = V[:, :n_pca] loadings (m x n_da; each entry a sum of fused terms in
 *   ascending PCA index from +0);  var_contr(j,a) = var_load(j,a)^2 / c_a with c_a = the column's sum of squares, formed as the
 *   WSS above (tiles of TPG_KMEANS_TILE rows by halving, tiles in ascending order);  c_a < 1e-12: the column is all zeros.
 *   Rounding (eps as above): var_load(j,a) lies within E = (n_pca + 1) eps sum_p |V_jp| |l_pa| of the exact product; its square
 *   within q = 2 |var_load| E + E^2; c_a within Ec = sum_j q_j + (m + 2) eps c_a; var_contr within q / c_a + var_contr Ec / c_a +
 *   2 eps var_contr.
 * predict() on new individuals is the same arithmetic on their scores x (the first n_pca columns): z = (x - mu)' S[:, :n_da]
 *   with mu = sum_g pi_g mu_g (g ascending) from the prior and means gt_dapc returns, m_g as above, the posterior and the tie rule
 *   as above; it is formed in Python (predict_gt_dapc) and needs no entry point here.
 * Out of scope: cross-validation of n_pca (xvalDapc), priors other than the group proportions. */
/* host only.  With Lmax = min(d, G - 1): prior[G], means G x d, scaling d x Lmax, svd[Lmax] (columns / entries beyond *n_lda are
 * 0), ind_coord n x Lmax and grp_coord G x Lmax (the first *n_da_out columns are written), posterior n x G, assign[n] (0-based);
 * all column-major host memory; mu_out[d] may be NULL */
int tpg_lda(const double* X, int64_t n, int d, const int32_t* grp0, int G, int n_da, double* prior, double* means, double* mu_out,
            double* scaling, double* svd, int32_t* n_lda, int32_t* n_da_out, double* ind_coord, double* grp_coord,
            double* posterior, int32_t* assign);
/* V: m rows, leading dimension ldv >= m, at least n_pca columns; loadings n_pca x n_da; var_load and var_contr m x n_da; all
 * column-major, host or device memory.  1 <= n_pca <= 64, 1 <= n_da <= 64 */
int tpg_dapc_var_contr(tpg_ctx* ctx, const double* V, int64_t m, int64_t ldv, int n_pca, const double* loadings, int n_da,
                       double* var_load, double* var_contr);

/* ---- OADP projection (predict(pca, new_data, project_method = "OADP"), R/predict_gt_pca.R:177-182 -> bigsnpr::OADP_proj; bigsnpr
 * is not among the reference's sources, so the projection is defined HERE from first principles, RECALLED FROM Zhang, Dey & Lee
 * (2020), NOT PINNED) ---------------------------------------------------------------------------------------------------------
 * Per new individual: l (K) its row of XV, s its X_norm (|z|^2 with missing -> 0), d (K) the singular values of the PCA,
 * positive and descending.
 *   1. rho^2 = max(s - sum_k l_k^2, 0).  M is (K+1) x (K+1): the top-left block diag(d), the last row (l_1 .. l_K, rho), the rest
 *      of the last column 0 -- the reference panel plus the new row in the basis [V, r / rho]; M M' = [[D^2, D l], [l'D, s]].
 *   2. M = A S B'; the K largest singular values S_K; A1 the top K x K block of their columns of A, a the last row.
 *   3. Procrustes of the augmented reference scores U A1 S_K onto U D, rotation and scale, no translation (only XV, X_norm and d
 *      are at hand, as in bigsnpr):  C = S_K A1' D = P Sigma W',  R = P W',  c = tr Sigma / |A1 S_K|_F^2.
 *   4. The row of the result is c (a S_K) R.
 * The signs of singular vectors and rotations within repeated singular values cancel.  l = 0 with s < d_K^2 gives exactly 0: an
 * individual with every genotype missing projects to the origin.  sigma_min(C) <= 2^-40 sigma_max(C): R is not unique, the row
 * is NaN and counted in *n_degenerate (0 is the expected value); l = 0 with s > d_K^2 is such a row, the new sample's own
 * direction displacing PC K.
 * How it is computed (csrc/host/host_oadp.h, one text for host and device): both decompositions are a one-sided Jacobi iteration
 * in a fixed round-robin order -- on the columns of M, whose limit is A S itself, and on C' = D (A1 S_K) with the row a S_K
 * carried along, so that neither C'C nor a matrix of singular vectors is formed; a pair of columns is left alone once
 * |a_i . a_j| <= 2^-52 |a_i| |a_j|, at most 30 sweeps.  A row's bits depend on its own l, s and on d only: not on n, not on
 * its position.
 * XV and out are n x K column-major, X_norm[n], sval[K], host or device memory.  1 <= K <= 32, else TPG_EINVAL; sval not positive
 * or not descending: TPG_EINVAL; a value of XV, X_norm or sval that is not finite: TPG_ENUMERIC. */
int tpg_oadp_proj(tpg_ctx* ctx, const double* XV, const double* X_norm, int64_t n, int K, const double* sval, double* out,
                  int64_t* n_degenerate);
/* the sweep of tpg_fbm256_prod_and_rowSumsSq over the view (V m x K), then the projection, XV and X_norm staying on the device;
 * out n x K, XV_out n x K (the "simple" projection, may be NULL) */
int tpg_predict_oadp(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale, const double* V, int K,
                     const double* sval, double* out, double* XV_out /* may be NULL */, int64_t* n_degenerate);

/* ---- least-squares projection (predict(pca, new_data, project_method = "least_squares"), R/predict_gt_pca.R:187-228: every
 * individual is regressed on the loadings over the loci it is typed at, as SMARTPCA's lsqproject does) -------------------------
 * Inputs: a view (n individuals x m loci), center[m], scale[m], V m x L column-major (the chosen loading columns),
 * 1 <= L <= TPG_LSQ_MAX_L.  For individual i let T_i be the loci where its code is 0, 1 or 2 and t_i = |T_i|:
 *   z_ij     = (g_ij - center_j) * (1 / scale_j)            (the arithmetic of tpg_fbm256_prod_and_rowSumsSq)
 *   A_i[a,b] = sum_{j in T_i} V[j,a] V[j,b]                 b_i[a] = sum_{j in T_i} z_ij V[j,a]
 *   x_i solves A_i x_i = b_i by Cholesky (A_i = R'R).
 * A is kept as its packed upper triangle: pair (a, b), a <= b, a-major, P = L (L + 1) / 2 values per individual.
 * Singular rule, exact and the same on host and device: row i is singular when t_i < L, or a Cholesky pivot p_k fails
 * p_k > L 2^-52 A_i[k,k], or a pivot is not finite.  A singular row is NaN in every component and counted in *n_singular (0 is
 * the expected value); the call succeeds all the same.
 * Rounding, eps = 2^-53.  The sums run on the FP64 matrix cores in an order of the library's choosing, the same on every call
 * (the split of the locus range may depend on n):
 *   |dA_i[a,b]| <= (t_i + 2) eps sum_{j in T_i} |V[j,a] V[j,b]|     (one rounding per product, any order of t_i terms)
 *   |db_i[a]|   <= (t_i + 4) eps sum_{j in T_i} |z_ij V[j,a]|       (z carries three roundings against (g - center) / scale)
 *   n_typed is exact.
 * The solve from given (A, b) is backward stable: |x^ - x|_2 <= k e_c / (1 - k e_c) |x|_2 with k = kappa_2(A) and
 * e_c = 4 L (3 L + 1) eps (the Cholesky backward error of Higham, Accuracy and Stability, Thm 10.4 -- RECALLED, NOT PINNED).
 * How it is computed (csrc/host/host_lsq.h, one text for host and device): a packed Cholesky row by row and two triangular
 * solves; every sum is formed by one member of a team in ascending index order and subtracted once, without contraction, so a
 * row's bits from tpg_lsq_solve depend on its own A, b and t only: not on n, not on its position.
 * Errors: L outside [1, TPG_LSQ_MAX_L], a null argument, a view without loci: TPG_EINVAL; a value of center, scale, V (or of A, b
 * handed to tpg_lsq_solve) that is not finite, a scale of zero, a sum that overflows: TPG_ENUMERIC.
 * All arrays host or device memory, column-major.  Not offered: tpg_stream_* / tpg_multi_* forms, L > 32. */
#define TPG_LSQ_MAX_L 32
/* the sweep: A n x P, b n x L, n_typed[n] */
int tpg_lsq_normal(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale, const double* V, int L, double* A,
                   double* b, int64_t* n_typed);
/* the batched solve: A n x P, b n x L, n_typed[n] -> out n x L; n_singular may be NULL */
int tpg_lsq_solve(tpg_ctx* ctx, const double* A, const double* b, const int64_t* n_typed, int64_t n, int L, double* out,
                  int64_t* n_singular);
/* the sweep, then the solve, A and b staying on the device; out n x L, n_typed_out[n] (may be NULL) */
int tpg_predict_lsq(tpg_ctx* ctx, const tpg_view* v, const double* center, const double* scale, const double* V, int L, double* out,
                    int64_t* n_typed_out /* may be NULL */, int64_t* n_singular);

/* ---- PC-Relate (gt_pcrelate: kinship and inbreeding that stay unbiased under population structure and admixture; Conomos,
 * Reiner, Weir and Thornton 2016, as GENESIS::pcrelate computes it.  The reference has no pcrelate and GENESIS is not among its
 * sources, so the arithmetic is defined HERE -- RECALLED, NOT PINNED to any other implementation: every individual's allele
 * frequency at every locus is modelled from the PCA scores, and kinship is formed from the residuals) ---------------------------
 * Inputs.  A view of n individuals x m loci, codes 0 / 1 / 2 / missing (missing genotypes are allowed).  V: n x K PCA scores,
 *   column-major, host or device memory, 0 <= K <= TPG_PCRELATE_MAX_K.  thr: the frequency bound, 0 < thr < 0.5 (0.01 is the
 *   customary value).  L = K + 1.  eps = 2^-53 below.
 * 0. Basis (host, csrc/host/host_pcrelate.h).  Q (n x L, column-major) is an orthonormal basis of span[1, V]: column 0 is
 *   1 / sqrt(n); column j = 1 .. K is V[, j - 1] after modified Gram-Schmidt against the columns before it, APPLIED TWICE, columns
 *   ascending, every sum ascending in i from +0; nb / na = its norm before / after the projections, Q_ij = w_i / na.  A column with
 *   na <= n 2^-52 nb (or a norm that is not finite) is a rank-deficient design: TPG_EINVAL.  n < L + 1: TPG_EINVAL.
 * 1. Coefficients (device).  For locus s: t_s = the number typed, S1 = n1 + 2 n2 (integers), mean_s = S1 / t_s (one division;
 *   t_s = 0: mean_s = 0), c_sk = sum_{i typed} (g_is - mean_s) Q_ik, k = 0 .. L - 1: the regression of the mean-imputed genotype
 *   column on [1, V]; as 1 lies in the span, the fitted value is mean_s + sum_k Q_ik c_sk.  t_s = 0 gives c_s = 0, and the locus
 *   drops out in step 2.  This is the FP64 row-scaled sweep of csrc/pca.hip with a scale of 1, a missing genotype adding 0; the
 *   order of the sum over i is free.  Outputs mean[m], c (m x L, column-major).  Rounding, as for the beta of "pcadapt":
 *   |d c_sk| <= n eps sqrt(tot_s) with tot_s = sum_{i typed} (g_is - mean_s)^2 (first order, any order of the sum, fused or
 *   not), plus eps mean_s sum_{i typed} |Q_ik| <= eps 2 sqrt(n) from the rounding of mean_s.
 * 2. Frequencies, validity, operands (device, PINNED order, no FMA contraction).  a_is = mean_s + sum_k Q_ik c_sk: starting from
 *   mean_s, for k = 0 .. L - 1 in turn the product Q_ik c_sk is rounded and then added to the running sum; mu_is = 0.5 a_is.
 *   valid_is = typed_is and thr <= mu_is <= hi, hi = 1 - thr rounded once.  For a valid cell R_is = g_is - a_is (2 mu is exact),
 *   S_is = sqrt(mu_is (1 - mu_is)) (1 - mu rounded, the product rounded, the root), M_is = 1; an invalid cell is 0 in all three.
 *   Given the same mean, c and Q, mu and valid are bit for bit those of the numpy model (tests/pcrelate_ref.py).  A monomorphic
 *   locus has c_s = 0 and mu = 0 or 1: invalid for everyone.
 * 3. Grams (device).  Num = R R', Den = S S', Cnt = M M', n x n: the lower triangle is computed on v_mfma_f64_16x16x4_f64 and
 *   mirrored.  Loci are accumulated in ascending blocks (tpg_pcrelate_block_loci) with no floating-point atomic: the same call
 *   gives the same bits.  Cnt is an exact integer while m < 2^53.  |d Num_ij| <= (m + 2) eps sum_s |R_is R_js| (one rounding
 *   per product, any order of the sum) plus the first-order term of the rounding of R itself, 2 eps sum_s |R_is R_js| (R is one
 *   subtraction of the pinned a_is from 0, 1 or 2: within eps of g - a in relative terms); |d Den_ij| <= (m + 2 + 6) eps sum_s S_is S_js
 *   (each S is within 3 eps of its value: two roundings under the root, which halves them, and a root within one ulp = 2 eps).
 *   m here is the number of loci of the view.  tests/test_gpu_pcrelate.py evaluates both per cell
 *   from the extended-precision route of tests/pcrelate_ref.py.
 * 4. Epilogue (plain double).  kin_ij = Num_ij / (4 Den_ij); f_i = 2 kin_ii - 1; n_snp = Cnt.  Den_ij = 0 (no jointly valid
 *   locus) gives NaN (0 / 0): an individual with every genotype missing has a NaN row, a NaN column and a NaN f.
 * mean and c are INPUTS of steps 2 - 3: a caller may compute them from a training subset of unrelated individuals (the role of
 * PC-AiR's partition) and hand them to tpg_pcrelate_gram.
 * No n x m array of doubles exists anywhere: per block of B loci the operands R and S of the block are written once, in the
 * fragment order of the MFMA, into 16 B bytes per padded row (tpg_pcrelate_scratch_bytes; B <= 1024, csrc/pcrelate.hip).
 * Errors: a null argument, K or L out of range, thr outside (0, 0.5), an empty view, n < L + 1, a rank-deficient V: TPG_EINVAL;
 * a value of mean, c or Q that is not finite: TPG_ENUMERIC.  All arrays host or device memory, column-major; the caller's memory
 * is written at the end only.
 * Not offered: the IBD-sharing probabilities k0 / k2 (dominance-coded Grams of the same shape: further chains of the same
 * kernel), GENESIS's `scale` options and its small-sample correction, PC-AiR's choice of an unrelated training set,
 * tpg_stream_* / tpg_multi_* forms, an R shim entry, K > 32. */
#define TPG_PCRELATE_MAX_K 32
/* loci per block for n individuals (a multiple of 128); bytes of operand scratch a call holds: bounded independently of m */
int64_t tpg_pcrelate_block_loci(int64_t n);
size_t tpg_pcrelate_scratch_bytes(int64_t n, int64_t m, int K);
/* the most cells n m that tpg_pcrelate_isaf serves: 2^26 */
int64_t tpg_pcrelate_isaf_max_cells(void);
/* step 0, host memory only: V n x K (may be NULL when K = 0) -> Q n x (K + 1) */
int tpg_pcrelate_basis(const double* V, int64_t n, int K, double* Q);
/* step 1: Q n x L -> mean[m], c m x L */
int tpg_pcrelate_coef(tpg_ctx* ctx, const tpg_view* v, const double* Q, int L, double* mean, double* c);
/* step 2 as a dense result, for tests and small panels (n m <= tpg_pcrelate_isaf_max_cells(), else TPG_EINVAL): mu n x m
 * doubles, valid n x m bytes 0 / 1 */
int tpg_pcrelate_isaf(tpg_ctx* ctx, const tpg_view* v, const double* mean, const double* c, const double* Q, int L, double thr,
                      double* mu, uint8_t* valid);
/* steps 2 - 3: num, den, cnt n x n doubles, both triangles */
int tpg_pcrelate_gram(tpg_ctx* ctx, const tpg_view* v, const double* mean, const double* c, const double* Q, int L, double thr,
                      double* num, double* den, double* cnt);
/* the whole, bit for bit the staged calls: kin n x n, f[n], n_snp n x n (may be NULL) */
int tpg_pcrelate(tpg_ctx* ctx, const tpg_view* v, const double* V, int K, double thr, double* kin, double* f, int64_t* n_snp);

#ifdef __cplusplus
}
#endif
#endif /* TPG_H */
