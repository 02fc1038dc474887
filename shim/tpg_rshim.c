/*
 * tpg_rshim.c -- the R side of the drop-in boundary: `.Call` entry points with the reference's own symbol names and
 * arities (src/RcppExports.cpp:348-371 of the reference; R side R/RcppExports.R:4-91), forwarding to the C ABI of
 * libtpg_hip.so (include/tpg.h).  Plain C against R's C API only: no Rcpp, no bigstatsr headers -- everything the
 * reference's C++ takes from `BM` through bigstatsr's accessors is taken here from the FBM's plain R fields
 * (`backingfile`, `nrow`, `ncol`, `code256`) and the backing file itself.
 *
 * STATUS: written against R's documented C API.  R is not installed in the build image, so what is checked there is:
 * (1) the file compiles with -Wall -Wextra -Werror against tests/rmock/ (declarations of the ~35 R API functions it
 * uses, written from R's documentation -- a syntax and signature guard, NOT R), and (2) linked against the mock runtime
 * of tests/rmock/rmock.c (protect stack counted on every call; GC torture, failing allocation and strict arguments as
 * opt-in modes) every registered symbol runs on the GPU: the increment_* through the block loops of the R drivers
 * (tests/test_gpu_rshim.py), the per-locus, Fst-loop and fbm256 symbols against the oracle under GC torture and strict
 * arguments (tests/test_gpu_rshim_entries.py); the 14 reference symbols also run under ASan/UBSan with every allocation
 * failing in turn (tests/test_host_sanitizers.py).  See INTEGRATION.md.
 *
 * R's rules the shim keeps: every R allocation of an entry point comes before its device view exists (an allocation
 * that fails is a longjmp past tpg_view_free); index vectors are coerced to integer as Rcpp's IntegerVector does; NA_REAL
 * is written where the reference writes it (alt_freq's freq, gt_pi_diploid), a plain NaN where it divides 0 by 0.
 *
 * Where it goes: tidypopgen/src/tpg_rshim.c, replacing the `[[Rcpp::export]]` bodies of the functions listed in
 * tpg_rshim_entries[] (INTEGRATION.md section 2 says how the registration tables are merged), or the package
 * shim/tpgshim beside an unmodified tidypopgen.  R code is UNCHANGED and correct by default: every increment_* call
 * adds its block's sums to k / k2 before it returns, as the reference does.  Opt-in fast path: TPG_RSHIM_DEFERRED=1
 * keeps the sums in HBM across the block loop; the three pairwise drivers then need ONE line after their loop
 * (`tpg_flush()`, see _tidypopgen_tpg_flush below).
 *
 * Threading: R calls these from its main thread only; the shim holds one tpg_ctx per R session.
 */
#define _POSIX_C_SOURCE 200809L /* strdup, mmap */
#include <fcntl.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <R.h>
#include <Rinternals.h>
#include <R_ext/Rdynload.h>

#include "tpg.h"
#include "../tidypopgen_amd/csrc/host/host_hwe.h" /* SNPHWE2_R: one table, on the host */

/* R's missing values come from R_ext/Arith.h, which R.h includes.  A build against stand-in R headers that declare only
 * the API functions (a syntax and signature guard) gets the same values here: NA_real_ is the NaN whose low word is
 * 1954, NA_integer_ is INT_MIN. */
#ifndef NA_INTEGER
#define NA_INTEGER INT_MIN
#endif
#ifndef ISNAN
#define ISNAN(x) (isnan(x))
#endif
#ifndef NA_REAL
static double tpg_na_real(void) {
  const uint64_t bits = 0x7FF00000000007A2ull;
  double d;
  memcpy(&d, &bits, sizeof d);
  return d;
}
#define NA_REAL tpg_na_real()
#endif

/* ---- session state -------------------------------------------------------------------------------------------- */

static tpg_ctx* g_ctx = NULL;

/* TPG_RSHIM_DEFERRED=1: the increment_* functions keep their sums in HBM until tpg_flush() (the R drivers must then
 * call it after their block loop).  Default: off -- an unmodified driver gets the reference's semantics. */
static int deferred(void) {
  const char* e = getenv("TPG_RSHIM_DEFERRED");
  return e && e[0] == '1';
}

static tpg_ctx* ctx(void) {
  if (!g_ctx) {
    const char* dev = getenv("TPG_DEVICE");
    /* TPG_RSHIM_NUMA_BIND=1 (opt-in: it changes the CPU affinity of the R session's thread, as starting R under
       `numactl --cpunodebind` would): stay on the host NUMA node of the GPU -- INTEGRATION.md 3b */
    const char* nb = getenv("TPG_RSHIM_NUMA_BIND");
    if (nb && nb[0] == '1') (void)tpg_host_bind_near_device(dev ? atoi(dev) : 0, NULL);
    if (tpg_ctx_create(dev ? atoi(dev) : 0, &g_ctx) != TPG_OK) Rf_error("tidypopgen (GPU): %s", tpg_last_error());
    if (deferred() && tpg_increment_defer(g_ctx, 1) != TPG_OK) Rf_error("tidypopgen (GPU): %s", tpg_last_error());
  }
  return g_ctx;
}

/* every failure of the library becomes an R error, as BEGIN_RCPP / END_RCPP turn C++ exceptions into R errors */
#define TPG_R(call)                                                         \
  do {                                                                      \
    if ((call) != TPG_OK) Rf_error("tidypopgen (GPU): %s", tpg_last_error()); \
  } while (0)

static SEXP field(SEXP env, const char* name) { /* a field or an active binding of the reference-class object */
  SEXP v = Rf_eval(Rf_install(name), env);
  if (v == R_UnboundValue) Rf_error("FBM object has no field '%s'", name);
  return v;
}

static int64_t field_i64(SEXP env, const char* name) {
  SEXP v = field(env, name);
  return TYPEOF(v) == REALSXP ? (int64_t)REAL(v)[0] : (int64_t)Rf_asInteger(v);
}

static const char* field_path(SEXP env, const char* name) {
  SEXP v = field(env, name);
  if (TYPEOF(v) != STRSXP || XLENGTH(v) < 1) Rf_error("FBM field '%s' is not a file name", name);
  return R_ExpandFileName(CHAR(STRING_ELT(v, 0)));
}

/* A backing file mapped into this process, and (opt-in, for genotype FBMs) its copy in HBM.
 * DEFAULT: no HBM copy outlives a call.  Every per-locus entry point uploads the columns its colInd covers (the R drivers
 * call block by block, so a driver loop moves the file once), exactly as the increment_* mirrors do: an FBM that is
 * rewritten in place between two calls -- bigsnpr::snp_fastImputeSimple (R/gt_impute_simple.R:86), gt_set_imputed-style
 * writes, any store through bigstatsr's own mapping -- can never be served stale.
 * TPG_RSHIM_CACHE=1 (opt-in): the whole genotype FBM is uploaded once and kept in HBM while the file's size, modification
 * time and a fingerprint of 512 pages spread over it are what they were at upload.  That is a HEURISTIC: stores through a
 * mapping do not reliably move the modification time before msync / munmap on tmpfs or NFS, and a sparse edit can miss
 * the sampled pages (0.04 % of a 5 GB file) -- enable it only for read-only data sets, or call tpg_invalidate(BM) /
 * tpg_release() after anything that writes to the FBM. */
typedef struct {
  char* path;
  void* map;
  size_t bytes;
  int writable;
  int64_t nrow, ncol;
  tpg_fbm* dev; /* NULL for the double N x N accumulators, and always unless TPG_RSHIM_CACHE=1 */
  int64_t mtime_ns;
  uint64_t fingerprint;
  uint64_t stamp; /* g_call of the last increment_* call that used this (writable) mapping */
  uint64_t dev_id, ino; /* st_dev / st_ino of the file the mapping was made of */
} mapped_file;

/* an array of POINTERS: a mapped_file* handed out stays valid when the table grows or an entry is forgotten */
static mapped_file** g_files = NULL;
static int g_nfiles = 0;
static uint64_t g_call = 0; /* counts increment_* calls */

static int cache_on(void) {
  const char* e = getenv("TPG_RSHIM_CACHE");
  return e && e[0] == '1';
}

static uint64_t fingerprint_of(const uint8_t* p, size_t bytes) { /* FNV-1a over up to 512 whole 4-KiB pages (2 MB read) */
  const size_t page = 4096, npages = (bytes + page - 1) / page, want = npages < 512 ? npages : 512;
  uint64_t h = 1469598103934665603ull;
  for (size_t k = 0; k < want; k++) {
    const size_t pg = want > 1 ? k * (npages - 1) / (want - 1) : 0, off = pg * page;
    const size_t len = bytes - off < page ? bytes - off : page;
    for (size_t t = 0; t < len; t += 8) {
      uint64_t w = 0;
      memcpy(&w, p + off + t, len - t < 8 ? len - t : 8);
      h = (h ^ w) * 1099511628211ull;
    }
  }
  return h;
}

static int64_t mtime_of(const char* path, size_t* size) {
  struct stat st;
  if (stat(path, &st) != 0) Rf_error("cannot stat backing file '%s'", path);
  *size = (size_t)st.st_size;
  return (int64_t)st.st_mtim.tv_sec * 1000000000ll + (int64_t)st.st_mtim.tv_nsec;
}

static void forget_file(int k) { /* unmap, free the HBM copy, close the gap in g_files */
  mapped_file* f = g_files[k];
  if (f->dev) tpg_fbm_free(f->dev);
  munmap(f->map, f->bytes);
  free(f->path);
  free(f);
  g_files[k] = g_files[g_nfiles - 1];
  g_nfiles--;
}

static mapped_file* map_file(const char* path, size_t bytes, int writable, int64_t nrow, int64_t ncol) {
  /* a mapping is reused only while the PATH still names the file it was made of: a backing file unlinked and created again
     at the same path and size (file.remove() + a new FBM, an explicit backingfile=) is another inode, and adding into the
     old, unlinked one would leave R reading zeros from the new file without any error */
  struct stat st;
  const int have_st = stat(path, &st) == 0;
  for (int k = 0; k < g_nfiles; k++)
    if (strcmp(g_files[k]->path, path) == 0 && g_files[k]->bytes == bytes && g_files[k]->writable == writable) {
      if (have_st && g_files[k]->dev_id == (uint64_t)st.st_dev && g_files[k]->ino == (uint64_t)st.st_ino) return g_files[k];
      /* Under TPG_RSHIM_DEFERRED=1 the library may still hold this mapping's address for sums it has not written yet: they
         belong to the OLD file (the one the block loop was filling), so they are written there before the mapping goes --
         never into unmapped memory, never into the new file. */
      if (writable && deferred() && g_ctx && tpg_increment_flush(g_ctx) != TPG_OK)
        Rf_error("tidypopgen (GPU): %s", tpg_last_error());
      forget_file(k);
      break;
    }
  int fd = open(path, writable ? O_RDWR : O_RDONLY);
  if (fd < 0) Rf_error("cannot open backing file '%s'", path);
  if (fstat(fd, &st) != 0 || (size_t)st.st_size < bytes) {
    close(fd);
    Rf_error("backing file '%s' is smaller than the FBM it should hold", path);
  }
  /* MAP_SHARED: the same pages bigstatsr's own mapping of the file reads and writes */
  void* p = mmap(NULL, bytes, writable ? (PROT_READ | PROT_WRITE) : PROT_READ, MAP_SHARED, fd, 0);
  close(fd);
  if (p == MAP_FAILED) Rf_error("mmap of '%s' failed", path);
#ifdef MADV_POPULATE_WRITE
  /* an accumulator is written in full by the first call that uses it: one batched populate (Linux 5.14) instead of a write
     fault per page of a shared file mapping from the adding threads (49 000 per matrix at n = 5 000) */
  if (writable) (void)madvise(p, bytes, MADV_POPULATE_WRITE);
#endif
  mapped_file** nf = (mapped_file**)realloc(g_files, sizeof(mapped_file*) * (size_t)(g_nfiles + 1));
  mapped_file* f = nf ? (mapped_file*)calloc(1, sizeof(mapped_file)) : NULL;
  char* pc = f ? strdup(path) : NULL;
  if (nf) g_files = nf;
  if (!pc) {
    free(f);
    munmap(p, bytes);
    Rf_error("out of memory");
  }
  g_files[g_nfiles++] = f;
  f->path = pc;
  f->map = p;
  f->bytes = bytes;
  f->writable = writable;
  f->nrow = nrow;
  f->ncol = ncol;
  f->dev_id = (uint64_t)st.st_dev;
  f->ino = (uint64_t)st.st_ino;
  return f;
}

/* the genotype FBM.code256 behind `BM`: its host mapping */
static mapped_file* genotype_fbm(SEXP BM) {
  const int64_t nrow = field_i64(BM, "nrow"), ncol = field_i64(BM, "ncol");
  return map_file(field_path(BM, "backingfile"), (size_t)nrow * (size_t)ncol, 0, nrow, ncol);
}

/* TPG_RSHIM_CACHE=1 only: the HBM copy of the whole FBM, re-uploaded when the heuristic above says the bytes changed */
static tpg_fbm* genotype_fbm_dev(SEXP BM) {
  mapped_file* f = genotype_fbm(BM);
  size_t size = 0;
  const int64_t mt = mtime_of(f->path, &size);
  if (size < f->bytes) Rf_error("backing file '%s' shrank below the FBM it should hold", f->path);
  const uint64_t fp = fingerprint_of((const uint8_t*)f->map, f->bytes);
  if (f->dev && (mt != f->mtime_ns || fp != f->fingerprint)) { /* the bytes changed under us */
    tpg_fbm_free(f->dev);
    f->dev = NULL;
  }
  /* the library maps the file, touches its pages with a team of threads and uploads it with one copy */
  if (!f->dev) {
    TPG_R(tpg_fbm_open_bk(ctx(), f->path, f->nrow, f->ncol, &f->dev));
    f->mtime_ns = mt;
    f->fingerprint = fp;
  }
  return f->dev;
}

static const double* code256_of(SEXP BM) {
  SEXP c = field(BM, "code256");
  if (TYPEOF(c) != REALSXP || XLENGTH(c) != 256) Rf_error("BM$code256 is not a double[256]");
  return REAL(c);
}

/* a double FBM (the N x N accumulators the R drivers allocate with bigstatsr::FBM(n, n, init = 0)).  Its mapping is kept
 * while the block loop that uses it runs -- mapping a 200 MB file afresh for every block costs its 49 000 page faults
 * every time: 65 ms per call against 14 with the mapping kept (two matrices of 5 000 x 5 000, 8 threads adding) -- and is
 * dropped by the first increment_* call that does NOT use it (the next analysis), by tpg_flush / tpg_release and at unload,
 * so that a session holds at most one analysis' pair of R temp files mapped. */
static double* double_fbm(SEXP K, int64_t n) {
  const int64_t nrow = field_i64(K, "nrow"), ncol = field_i64(K, "ncol");
  if (nrow != n || ncol != n) Rf_error("accumulator FBM is %lld x %lld, expected %lld x %lld", (long long)nrow,
                                       (long long)ncol, (long long)n, (long long)n);
  mapped_file* f = map_file(field_path(K, "backingfile"), sizeof(double) * (size_t)n * (size_t)n, 1, n, n);
  f->stamp = g_call;
  return (double*)f->map;
}

static void release_accumulators(int all) {
  for (int k = g_nfiles - 1; k >= 0; k--)
    if (g_files[k]->writable && (all || g_files[k]->stamp != g_call)) forget_file(k);
}

/* after an increment_* call: by default its sums are already in k / k2; the accumulators of EARLIER analyses can go */
static void after_increment(void) {
  if (!deferred()) release_accumulators(0);
}

/* An index vector as Rcpp's `const IntegerVector&` takes it: a double vector (vctrs::vec_data(.x) rows, ind.row = c(1, 3),
 * .group_ids(x) - 1) is coerced, as R's as.integer() does it -- the caller PROTECTs the result. */
static SEXP as_int(SEXP x) { return TYPEOF(x) == INTSXP ? x : Rf_coerceVector(x, INTSXP); }
static SEXP as_real(SEXP x) { return TYPEOF(x) == REALSXP ? x : Rf_coerceVector(x, REALSXP); }

/* every entry of a 1-based index vector (INTSXP) in [1, hi]: NA (or a NaN coerced to it) is an R error too */
static const int* checked_index(SEXP ind, int64_t hi, const char* what) {
  const int* p = INTEGER(ind);
  for (R_xlen_t k = 0; k < XLENGTH(ind); k++)
    if (p[k] == NA_INTEGER || p[k] < 1 || p[k] > hi)
      Rf_error("tidypopgen (GPU): %s[%lld] = %s out of [1,%lld]", what, (long long)k, p[k] == NA_INTEGER ? "NA" : "a value",
               (long long)hi);
  return p;
}

/* the packed (rowInd, colInd, code256) view a per-locus entry point works on.  Default: the columns colInd covers are
 * uploaded for this call alone (the contiguous blocks of the R drivers: their covering range; a scattered colInd: gathered
 * on the host first) and released with it; TPG_RSHIM_CACHE=1: packed from the cached HBM copy of the whole FBM.
 * rowInd / colInd are INTSXP (as_int).  Every R allocation of the entry point comes BEFORE this: an allocation that fails
 * is a longjmp that would jump past tpg_view_free. */
static tpg_view* view_of(SEXP BM, SEXP rowInd, SEXP colInd, int raw_bytes) {
  const int64_t n = (int64_t)XLENGTH(rowInd), m = (int64_t)XLENGTH(colInd);
  const double* code = raw_bytes ? NULL : code256_of(BM);
  if (m < 1) Rf_error("tidypopgen (GPU): empty colInd");
  int* cols = (int*)R_alloc((size_t)m, sizeof(int)); /* R's transient storage: freed when .Call returns or errors */
  tpg_view* v = NULL;
  if (cache_on()) {
    tpg_fbm* d = genotype_fbm_dev(BM);
    mapped_file* f = genotype_fbm(BM);
    checked_index(rowInd, f->nrow, "rowInd");
    checked_index(colInd, f->ncol, "colInd");
    TPG_R(tpg_view_create(ctx(), d, INTEGER(rowInd), n, INTEGER(colInd), m, code, &v));
    return v;
  }
  mapped_file* f = genotype_fbm(BM);
  const uint8_t* bytes = (const uint8_t*)f->map;
  const int64_t nrow = f->nrow;
  checked_index(rowInd, nrow, "rowInd");
  const int* ci = checked_index(colInd, f->ncol, "colInd");
  int lo = ci[0], hi = ci[0];
  for (int64_t j = 0; j < m; j++) {
    if (ci[j] < lo) lo = ci[j];
    if (ci[j] > hi) hi = ci[j];
  }
  const int64_t span = (int64_t)hi - lo + 1;
  /* tpg_view_create_from_host: upload for this ONE code table (2 bits per genotype over PCIe where table and bytes allow it),
     pack, release the uploaded columns -- nothing of the FBM outlives the call */
  if (span <= 2 * m + 64) {
    for (int64_t j = 0; j < m; j++) cols[j] = ci[j] - (lo - 1);
    TPG_R(tpg_view_create_from_host(ctx(), bytes + (size_t)(lo - 1) * (size_t)nrow, nrow, span, INTEGER(rowInd), n, cols, m, code, &v));
  } else {
    uint8_t* stage = (uint8_t*)malloc((size_t)nrow * (size_t)m);
    if (!stage) Rf_error("tidypopgen (GPU): out of memory gathering %lld columns", (long long)m);
    for (int64_t j = 0; j < m; j++) {
      memcpy(stage + (size_t)j * (size_t)nrow, bytes + (size_t)(ci[j] - 1) * (size_t)nrow, (size_t)nrow);
      cols[j] = (int)(j + 1);
    }
    const int rc = tpg_view_create_from_host(ctx(), stage, nrow, m, INTEGER(rowInd), n, cols, m, code, &v); /* waited for: the staging buffer may go */
    free(stage);
    TPG_R(rc);
  }
  return v;
}

static SEXP named_list(int n, const char** names, SEXP* values) {
  SEXP out = PROTECT(Rf_allocVector(VECSXP, n));
  SEXP nm = PROTECT(Rf_allocVector(STRSXP, n));
  for (int k = 0; k < n; k++) {
    SET_VECTOR_ELT(out, k, values[k]);
    SET_STRING_ELT(nm, k, Rf_mkChar(names[k]));
  }
  Rf_setAttrib(out, R_NamesSymbol, nm);
  UNPROTECT(2);
  return out;
}

static void set_colnames2(SEXP mat, const char* a, const char* b) {
  SEXP cn = PROTECT(Rf_allocVector(STRSXP, 2));
  SET_STRING_ELT(cn, 0, Rf_mkChar(a));
  SET_STRING_ELT(cn, 1, Rf_mkChar(b));
  SEXP dn = PROTECT(Rf_allocVector(VECSXP, 2));
  SET_VECTOR_ELT(dn, 0, R_NilValue);
  SET_VECTOR_ELT(dn, 1, cn);
  Rf_setAttrib(mat, R_DimNamesSymbol, dn);
  UNPROTECT(2);
}

/* ngroups as Rcpp's `int` takes it (an integer or a double); NA or < 1 is an R error, not a matrix of -2^31 columns */
static int ngroups_of(SEXP ngroups) {
  const int G = Rf_asInteger(ngroups);
  if (G == NA_INTEGER || G < 1) Rf_error("tidypopgen (GPU): ngroups must be a positive integer");
  return G;
}

/* views are released even when the library call fails (Rf_error does not return) */
#define TPG_R_VIEW(v, call)          \
  do {                               \
    int _rc = (call);                \
    tpg_view_free(v);                \
    if (_rc != TPG_OK) Rf_error("tidypopgen (GPU): %s", tpg_last_error()); \
  } while (0)

/* ---- per-locus sweeps --------------------------------------------------------------------------------------- */

/* alt_freq_dip_pseudo_cpp(BM, rowInd, colInd, ploidy, ncores, as_counts)   src/alt_freq_dip_pseudo_cpp.cpp:8-58 */
SEXP _tidypopgen_alt_freq_dip_pseudo_cpp(SEXP BM, SEXP rowInd, SEXP colInd, SEXP ploidy, SEXP ncores, SEXP as_counts) {
  (void)ncores;
  const int counts = Rf_asLogical(as_counts);
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP pl = PROTECT(Rf_coerceVector(ploidy, REALSXP));
  const int m = (int)XLENGTH(ci);
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, m, 2));
  set_colnames2(out, counts ? "n_alt" : "freq", "n_valid"); /* :44, :56 */
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_alt_freq_dip_pseudo(ctx(), v, REAL(pl), counts, REAL(out)));
  double* f = REAL(out);
  if (!counts)
    for (int j = 0; j < m; j++)
      if (!(f[m + j] > 0)) f[j] = NA_REAL; /* :49-53: NA_real_, not the device's NaN */
  UNPROTECT(4);
  return out;
}

/* grouped_alt_freq_dip_pseudo_cpp(BM, rowInd, colInd, groupIds, ngroups, ploidy, ncores, as_counts)
   src/grouped_alt_freq_dip_pseudo_cpp.cpp:8-58 -> m x 2G */
SEXP _tidypopgen_grouped_alt_freq_dip_pseudo_cpp(SEXP BM, SEXP rowInd, SEXP colInd, SEXP groupIds, SEXP ngroups,
                                                 SEXP ploidy, SEXP ncores, SEXP as_counts) {
  (void)ncores;
  const int G = ngroups_of(ngroups);
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP pl = PROTECT(Rf_coerceVector(ploidy, REALSXP));
  SEXP gid = PROTECT(Rf_coerceVector(groupIds, INTSXP));
  const int counts = Rf_asLogical(as_counts);
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, (int)XLENGTH(ci), 2 * G));
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_grouped_alt_freq_dip_pseudo(ctx(), v, INTEGER(gid), G, REAL(pl), counts, REAL(out)));
  UNPROTECT(5);
  return out;
}

/* grouped_missingness_cpp(BM, rowInd, colInd, groupIds, ngroups, ncores)   src/grouped_missingness_cpp.cpp:8-33 */
SEXP _tidypopgen_grouped_missingness_cpp(SEXP BM, SEXP rowInd, SEXP colInd, SEXP groupIds, SEXP ngroups, SEXP ncores) {
  (void)ncores;
  const int G = ngroups_of(ngroups);
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP gid = PROTECT(Rf_coerceVector(groupIds, INTSXP));
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, (int)XLENGTH(ci), G));
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_grouped_missingness(ctx(), v, INTEGER(gid), G, REAL(out)));
  UNPROTECT(4);
  return out;
}

/* grouped_summaries_dip_pseudo_cpp(BM, rowInd, colInd, groupIds, ngroups, ploidy, ncores)
   src/grouped_summaries_dip_pseudo_cpp.cpp:11-63 -> list(freq_alt, freq_ref, n, het_obs), each m x G */
SEXP _tidypopgen_grouped_summaries_dip_pseudo_cpp(SEXP BM, SEXP rowInd, SEXP colInd, SEXP groupIds, SEXP ngroups,
                                                  SEXP ploidy, SEXP ncores) {
  (void)ncores;
  const int G = ngroups_of(ngroups);
  const int m = (int)XLENGTH(colInd);
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP pl = PROTECT(Rf_coerceVector(ploidy, REALSXP));
  SEXP gid = PROTECT(Rf_coerceVector(groupIds, INTSXP));
  SEXP mats[4];
  for (int k = 0; k < 4; k++) mats[k] = PROTECT(Rf_allocMatrix(REALSXP, m, G));
  static const char* names[4] = {"freq_alt", "freq_ref", "n", "het_obs"}; /* :59-62 */
  SEXP out = PROTECT(named_list(4, names, mats));
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_grouped_summaries_dip_pseudo(ctx(), v, INTEGER(gid), G, REAL(pl), REAL(mats[0]), REAL(mats[1]),
                                                 REAL(mats[2]), REAL(mats[3])));
  UNPROTECT(9);
  return out;
}

/* gt_ind_hetero(BM, rowInd, colInd, ncores)   src/gt_ind_hetero.cpp:11-42 -> integer 2 x n {n_het; n_na} */
SEXP _tidypopgen_gt_ind_hetero(SEXP BM, SEXP rowInd, SEXP colInd, SEXP ncores) {
  (void)ncores;
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP out = PROTECT(Rf_allocMatrix(INTSXP, 2, (int)XLENGTH(ri)));
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_gt_ind_hetero(ctx(), v, INTEGER(out)));
  UNPROTECT(3);
  return out;
}

/* gt_pi_diploid(BM, rowInd, colInd, ncores)   src/gt_pi_diploid.cpp:7-38 */
SEXP _tidypopgen_gt_pi_diploid(SEXP BM, SEXP rowInd, SEXP colInd, SEXP ncores) {
  (void)ncores;
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP out = PROTECT(Rf_allocVector(REALSXP, XLENGTH(ci)));
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_gt_pi_diploid(ctx(), v, REAL(out)));
  /* :35-36: a locus without a valid genotype is NA_real_ (the only NaN pi can be: valid > 0 means valid >= 2) */
  double* pi = REAL(out);
  for (R_xlen_t j = 0; j < XLENGTH(out); j++)
    if (ISNAN(pi[j])) pi[j] = NA_REAL;
  UNPROTECT(3);
  return out;
}

/* gt_grouped_pi_diploid(BM, rowInd, colInd, groupIds, ngroups, ncores)   src/gt_grouped_pi_diploid.cpp:7-42 */
SEXP _tidypopgen_gt_grouped_pi_diploid(SEXP BM, SEXP rowInd, SEXP colInd, SEXP groupIds, SEXP ngroups, SEXP ncores) {
  (void)ncores;
  const int G = ngroups_of(ngroups);
  const int m = (int)XLENGTH(colInd);
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP gid = PROTECT(Rf_coerceVector(groupIds, INTSXP));
  SEXP mats[2];
  for (int k = 0; k < 2; k++) mats[k] = PROTECT(Rf_allocMatrix(REALSXP, m, G));
  static const char* names[2] = {"pi", "n"};
  SEXP out = PROTECT(named_list(2, names, mats));
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_gt_grouped_pi_diploid(ctx(), v, INTEGER(gid), G, REAL(mats[0]), REAL(mats[1])));
  UNPROTECT(6);
  return out;
}

/* ---- pairwise population Fst loops --------------------------------------------------------------------------- */

/* common body of the three loop functions.  pairwise_combn arrives as a 2 x P matrix (NumericMatrix: utils::combn gives an
   integer one, which Rcpp coerces); so do the m x G matrices, and an integer matrix is coerced as Rcpp coerces it. */
static SEXP fst_matrix(SEXP x, int m, int G, const char* what) {
  SEXP dim = Rf_getAttrib(x, R_DimSymbol);
  if ((TYPEOF(x) != REALSXP && TYPEOF(x) != INTSXP && TYPEOF(x) != LGLSXP) || Rf_length(dim) != 2)
    Rf_error("%s must be a numeric matrix", what);
  if (m >= 0 && (INTEGER(dim)[0] != m || INTEGER(dim)[1] != G)) Rf_error("%s is not %d x %d", what, m, G);
  return as_real(x);
}

static SEXP fst_loop(int method, SEXP pairwise_combn, SEXP n, SEXP freq_alt, SEXP freq_ref, SEXP het_obs, SEXP by_locus,
                     SEXP return_num_dem) {
  SEXP nr = PROTECT(fst_matrix(n, -1, 0, "n"));
  SEXP dim = Rf_getAttrib(nr, R_DimSymbol);
  const int m = INTEGER(dim)[0], G = INTEGER(dim)[1];
  SEXP fa = PROTECT(fst_matrix(freq_alt, m, G, "freq_alt"));
  SEXP fr = PROTECT(freq_ref == R_NilValue ? R_NilValue : fst_matrix(freq_ref, m, G, "freq_ref"));
  SEXP ho = PROTECT(het_obs == R_NilValue ? R_NilValue : fst_matrix(het_obs, m, G, "het_obs"));
  SEXP pdim = Rf_getAttrib(pairwise_combn, R_DimSymbol);
  if (Rf_length(pdim) != 2 || INTEGER(pdim)[0] != 2) Rf_error("pairwise_combn must be a 2-row matrix");
  SEXP pc = PROTECT(Rf_coerceVector(pairwise_combn, INTSXP));
  checked_index(pc, G, "pairwise_combn");
  const int P = (int)(XLENGTH(pc) / 2);
  const int byl = Rf_asLogical(by_locus) != 0, rnd = Rf_asLogical(return_num_dem) != 0;
  SEXP tot = PROTECT(Rf_allocVector(REALSXP, P));
  /* :17-21: fst_locus is m x P only under by_locus, fst_locus_dem only under return_num_dem, 0 x 0 otherwise; both are
     filled under by_locus alone (:35-42), so return_num_dem without by_locus gives a 0 x 0 numerator and a zero
     denominator, as Rcpp's zero-initialised NumericMatrix leaves it */
  SEXP a = PROTECT(Rf_allocMatrix(REALSXP, byl ? m : 0, byl ? P : 0));
  SEXP b = PROTECT(Rf_allocMatrix(REALSXP, rnd ? m : 0, rnd ? P : 0));
  if (rnd) memset(REAL(b), 0, sizeof(double) * (size_t)m * (size_t)P);
  SEXP out;
  if (!rnd) { /* :54-60 */
    static const char* names[2] = {"fst_locus", "fst_tot"};
    SEXP vals[2] = {a, tot};
    out = PROTECT(named_list(2, names, vals));
  } else {
    static const char* names[2] = {"Fst_by_locus_num", "Fst_by_locus_den"};
    SEXP vals[2] = {a, b};
    out = PROTECT(named_list(2, names, vals));
  }
  TPG_R(tpg_pairwise_fst_loop(ctx(), method, INTEGER(pc), P, m, G, REAL(nr), REAL(fa), fr == R_NilValue ? NULL : REAL(fr),
                              ho == R_NilValue ? NULL : REAL(ho), byl, byl && rnd, REAL(tot), byl ? REAL(a) : NULL,
                              byl && rnd ? REAL(b) : NULL));
  UNPROTECT(9);
  return out;
}

/* pairwise_fst_hudson_loop(pairwise_combn, n, freq_alt, freq_ref, by_locus, return_num_dem)
   src/pairwise_fst_hudson_loop.cpp:5-63 */
SEXP _tidypopgen_pairwise_fst_hudson_loop(SEXP pairwise_combn, SEXP n, SEXP freq_alt, SEXP freq_ref, SEXP by_locus,
                                          SEXP return_num_dem) {
  return fst_loop(TPG_FST_HUDSON, pairwise_combn, n, freq_alt, freq_ref, R_NilValue, by_locus, return_num_dem);
}

/* pairwise_fst_wc84_loop(pairwise_combn, n, freq_alt, het_obs, by_locus, return_num_dem)
   src/pairwise_fst_wc84_loop.cpp:5-121 */
SEXP _tidypopgen_pairwise_fst_wc84_loop(SEXP pairwise_combn, SEXP n, SEXP freq_alt, SEXP het_obs, SEXP by_locus,
                                        SEXP return_num_dem) {
  return fst_loop(TPG_FST_WC84, pairwise_combn, n, freq_alt, R_NilValue, het_obs, by_locus, return_num_dem);
}

/* pairwise_fst_nei87_loop(pairwise_combn, n, het_obs, freq_alt, freq_ref, by_locus, return_num_dem)
   src/pairwise_fst_nei87_loop.cpp:5-115 */
SEXP _tidypopgen_pairwise_fst_nei87_loop(SEXP pairwise_combn, SEXP n, SEXP het_obs, SEXP freq_alt, SEXP freq_ref,
                                         SEXP by_locus, SEXP return_num_dem) {
  return fst_loop(TPG_FST_NEI87, pairwise_combn, n, freq_alt, freq_ref, het_obs, by_locus, return_num_dem);
}

/* ---- pairwise individual matrices: the per-block increment functions ----------------------------------------------
 * The R drivers (R/snp_ibs.R:59-82, R/snp_king.R:51-77, R/snp_allele_sharing.R:49-70) call these once per locus block
 * with the same FBM and the same two N x N double FBMs.
 * Default: every call uploads the columns of its block, accumulates, and adds the sums to k / k2 before it returns.
 * TPG_RSHIM_DEFERRED=1: the accumulators stay in HBM across the calls and the sums reach k / k2 when
 * _tidypopgen_tpg_flush is called.  The scratch matrices the reference fills are not touched. */

/* increment_ibs_counts(k, k2, genotype0, genotype1, genotype2, BM, rowInd, colInd)   src/snp_ibs.cpp:22-74 */
SEXP _tidypopgen_increment_ibs_counts(SEXP k, SEXP k2, SEXP g0, SEXP g1, SEXP g2, SEXP BM, SEXP rowInd, SEXP colInd) {
  (void)g0; (void)g1; (void)g2;
  g_call++;
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  mapped_file* f = genotype_fbm(BM);
  const int64_t n = (int64_t)XLENGTH(ri);
  const int *r1 = checked_index(ri, f->nrow, "rowInd"), *c1 = checked_index(ci, f->ncol, "colInd");
  TPG_R(tpg_increment_ibs_counts(ctx(), double_fbm(k, n), double_fbm(k2, n), (const uint8_t*)f->map, f->nrow, f->ncol, r1,
                                 n, c1, (int64_t)XLENGTH(ci)));
  after_increment();
  UNPROTECT(2);
  return R_NilValue;
}

/* increment_king_numerator(k, n_Aa_i, genotype0, genotype1, genotype2, genotype_valid, BM, rowInd, colInd)
   src/snp_king.cpp:21-74 */
SEXP _tidypopgen_increment_king_numerator(SEXP k, SEXP n_Aa_i, SEXP g0, SEXP g1, SEXP g2, SEXP gv, SEXP BM, SEXP rowInd,
                                          SEXP colInd) {
  (void)g0; (void)g1; (void)g2; (void)gv;
  g_call++;
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  mapped_file* f = genotype_fbm(BM);
  const int64_t n = (int64_t)XLENGTH(ri);
  const int *r1 = checked_index(ri, f->nrow, "rowInd"), *c1 = checked_index(ci, f->ncol, "colInd");
  TPG_R(tpg_increment_king_numerator(ctx(), double_fbm(k, n), double_fbm(n_Aa_i, n), (const uint8_t*)f->map, f->nrow,
                                     f->ncol, r1, n, c1, (int64_t)XLENGTH(ci)));
  after_increment();
  UNPROTECT(2);
  return R_NilValue;
}

/* increment_as_counts(k, k2, na_mat, dos_mat, BM, rowInd, colInd)   src/snp_as.cpp:22-67
 * Quirk Q1: the reference adds +1 to every numerator for a block one column narrower than the scratch
 * matrices.  Off by default (the intended value, what the reference's own test asserts); TPG_EMULATE_AS_PAD_QUIRK=1
 * reproduces the reference binary bit for bit. */
SEXP _tidypopgen_increment_as_counts(SEXP k, SEXP k2, SEXP na_mat, SEXP dos_mat, SEXP BM, SEXP rowInd, SEXP colInd) {
  (void)na_mat;
  g_call++;
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  mapped_file* f = genotype_fbm(BM);
  const int64_t n = (int64_t)XLENGTH(ri), m = (int64_t)XLENGTH(ci);
  const int *r1 = checked_index(ri, f->nrow, "rowInd"), *c1 = checked_index(ci, f->ncol, "colInd");
  double* K = double_fbm(k, n);
  TPG_R(tpg_increment_as_counts(ctx(), K, double_fbm(k2, n), (const uint8_t*)f->map, f->nrow, f->ncol, r1, n, c1, m));
  const char* q = getenv("TPG_EMULATE_AS_PAD_QUIRK");
  if (q && q[0] == '1') {
    SEXP dim = Rf_getAttrib(dos_mat, R_DimSymbol);
    if (Rf_length(dim) == 2 && (int64_t)INTEGER(dim)[1] == m + 1) TPG_R(tpg_increment_as_note_narrow_block(ctx(), K, n));
  }
  after_increment();
  UNPROTECT(2);
  return R_NilValue;
}

/* tpg_flush(): under TPG_RSHIM_DEFERRED=1 the one line the three pairwise drivers gain after their block loop -- writes
 * the sums held in HBM into the k / k2 FBMs (one download of two N x N matrices per analysis); a no-op otherwise.  Not a
 * reference symbol. */
SEXP _tidypopgen_tpg_flush(void) {
  if (g_ctx) TPG_R(tpg_increment_flush(g_ctx));
  release_accumulators(1);
  return R_NilValue;
}

/* tpg_release(): drop the HBM copies and mappings (e.g. after the FBM was modified, or to free the GPU) */
SEXP _tidypopgen_tpg_release(void) {
  if (g_ctx) {
    TPG_R(tpg_increment_flush(g_ctx));
    TPG_R(tpg_resident_drop(g_ctx));
  }
  while (g_nfiles > 0) forget_file(g_nfiles - 1);
  free(g_files);
  g_files = NULL;
  g_nfiles = 0;
  return R_NilValue;
}

/* tpg_invalidate(BM): forget the HBM copy of this FBM (only TPG_RSHIM_CACHE=1 keeps one).  The caller's job after anything
 * that writes to the FBM (gt_impute_simple, gt_set_imputed ...): the tpgshim package exports it as tpg_invalidate() and does
 * NOT wrap the mutating functions itself; a write that leaves size and mtime alone is otherwise caught by the fingerprint */
SEXP _tidypopgen_tpg_invalidate(SEXP BM) {
  mapped_file* f = genotype_fbm(BM);
  if (f->dev) {
    tpg_fbm_free(f->dev);
    f->dev = NULL;
  }
  return R_NilValue;
}

/* tpg_impute_simple(BM, method, seed): gt_impute_simple's write to the FBM (bigsnpr::snp_fastImputeSimple behind
 * R/gt_impute_simple.R:86), in place on the backing file: column blocks go up, are imputed (tpg_fbm_impute_simple_at: `random`
 * keyed by the FBM's own row / column) and only the columns that changed are written back; then what tpg_invalidate does.
 * method 1 = mode, 2 = mean0, 3 = random (TPG_IMPUTE_*).  A byte above 3 anywhere: the R error "object x is already imputed",
 * file unchanged.  -> c(imputed, loci_all_missing) as doubles.
 * The two library symbols are referenced weakly: the shim still links and loads against a library built before they existed
 * (and against the host-only stand-in of the sanitizer jobs); the call then is an R error. */
#pragma weak tpg_fbm_impute_simple_at
#pragma weak tpg_fbm_to_host
SEXP _tidypopgen_tpg_impute_simple(SEXP BM, SEXP method, SEXP seed) {
  if (!tpg_fbm_impute_simple_at || !tpg_fbm_to_host) Rf_error("tidypopgen (GPU): this libtpg_hip has no tpg_fbm_impute_simple");
  const int meth = Rf_asInteger(method);
  SEXP sdx = PROTECT(as_real(seed));
  const double sd = XLENGTH(sdx) == 1 ? REAL(sdx)[0] : -1.0;
  UNPROTECT(1);
  if (!(sd >= 0 && sd < 18446744073709551616.0)) Rf_error("seed must be a non-negative number below 2^64");
  const uint64_t sd64 = (uint64_t)sd;
  const int64_t nrow = field_i64(BM, "nrow"), ncol = field_i64(BM, "ncol");
  if (nrow <= 0 || ncol <= 0) Rf_error("empty FBM");
  mapped_file* f = map_file(field_path(BM, "backingfile"), (size_t)nrow * (size_t)ncol, 1, nrow, ncol);
  uint8_t* bytes = (uint8_t*)f->map;
  int64_t per = ((int64_t)256 << 20) / nrow;
  if (per < 1) per = 1;
  if (per > ncol) per = ncol;
  uint8_t* back = (uint8_t*)malloc((size_t)per * (size_t)nrow);
  if (!back) Rf_error("tidypopgen (GPU): out of memory");
  double imputed = 0, all_missing = 0;
  int rc = TPG_OK;
  int64_t j0 = 0;
  for (; j0 < ncol && rc == TPG_OK; j0 += per) {
    const int64_t nb = ncol - j0 < per ? ncol - j0 : per;
    uint8_t* at = bytes + (size_t)j0 * (size_t)nrow;
    tpg_fbm* d = NULL;
    tpg_impute_report rep = {0, 0};
    rc = tpg_fbm_from_host(ctx(), at, nrow, nb, &d);
    if (rc == TPG_OK) rc = tpg_fbm_impute_simple_at(ctx(), d, j0, meth, sd64, &rep);
    if (rc == TPG_OK) rc = tpg_fbm_to_host(ctx(), d, back);
    tpg_fbm_free(d);
    if (rc != TPG_OK) break;
    for (int64_t j = 0; j < nb; j++) /* only the columns that changed are written: the others' pages stay clean */
      if (memcmp(at + (size_t)j * (size_t)nrow, back + (size_t)j * (size_t)nrow, (size_t)nrow) != 0)
        memcpy(at + (size_t)j * (size_t)nrow, back + (size_t)j * (size_t)nrow, (size_t)nrow);
    imputed += (double)rep.imputed;
    all_missing += (double)rep.loci_all_missing;
  }
  free(back);
  if (rc != TPG_OK) {
    /* the blocks in front of the failing one were free of bytes above 3 before this call: their 4..6 are its fills */
    const size_t done = (size_t)j0 * (size_t)nrow;
    for (size_t i = 0; i < done; i++)
      if (bytes[i] >= 4 && bytes[i] <= 6) bytes[i] = 3;
  }
  _tidypopgen_tpg_invalidate(BM);
  if (rc != TPG_OK) Rf_error("tidypopgen (GPU): %s", tpg_last_error());
  SEXP out = PROTECT(Rf_allocVector(REALSXP, 2));
  REAL(out)[0] = imputed;
  REAL(out)[1] = all_missing;
  UNPROTECT(1);
  return out;
}

/* ---- PCA projection -------------------------------------------------------------------------------------------- */

/* fbm256_prod_and_rowSumsSq(BM, ind_row, ind_col, center, scale, V)   src/fbm_prod_and_rowSumSq.cpp:10-47
   -> list(XV n x K, rowSumsSq n), unnamed as in the reference (:46) */
SEXP _tidypopgen_fbm256_prod_and_rowSumsSq(SEXP BM, SEXP ind_row, SEXP ind_col, SEXP center, SEXP scale, SEXP V) {
  SEXP dim = Rf_getAttrib(V, R_DimSymbol);
  if ((TYPEOF(V) != REALSXP && TYPEOF(V) != INTSXP) || Rf_length(dim) != 2) Rf_error("V must be a numeric matrix");
  const int K = INTEGER(dim)[1];
  if ((R_xlen_t)INTEGER(dim)[0] != XLENGTH(ind_col)) Rf_error("Incompatibility between dimensions."); /* myassert_size, :23 */
  const R_xlen_t m = XLENGTH(ind_col);
  if (XLENGTH(center) != m || XLENGTH(scale) != m) Rf_error("Incompatibility between dimensions.");
  SEXP ri = PROTECT(as_int(ind_row)), ci = PROTECT(as_int(ind_col));
  SEXP Vr = PROTECT(as_real(V));
  SEXP ce = PROTECT(Rf_coerceVector(center, REALSXP));
  SEXP sc = PROTECT(Rf_coerceVector(scale, REALSXP));
  SEXP XV = PROTECT(Rf_allocMatrix(REALSXP, (int)XLENGTH(ri), K));
  SEXP rss = PROTECT(Rf_allocVector(REALSXP, XLENGTH(ri)));
  SEXP out = PROTECT(Rf_allocVector(VECSXP, 2));
  SET_VECTOR_ELT(out, 0, XV);
  SET_VECTOR_ELT(out, 1, rss);
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_fbm256_prod_and_rowSumsSq(ctx(), v, REAL(ce), REAL(sc), REAL(Vr), K, REAL(XV), REAL(rss)));
  UNPROTECT(8);
  return out;
}

/* ---- whole analyses on all the GPUs of the node (additions; not reference symbols) ---------------------------------
 * The per-block entry points above are literal drop-ins and run on one GPU.  An R session is ONE process, so the way to
 * the other GPUs is one call per analysis: the library gives every device a share of colInd (its own upload, pack and
 * sweep on a host thread per device) and exchanges what is additive over loci itself (RCCL).  These replace the BODY of
 * the R drivers -- snp_ibs / snp_king / snp_allele_sharing / pairwise_grm (R/snp_ibs.R:42-104 ...), pairwise_pop_fst's
 * numeric part (R/pairwise_pop_fst.R:116-161), loci_alt_freq on a grouped tibble (R/loci_alt_freq.R:174-197),
 * gt_pca_partialSVD's big_SVD call (R/gt_pca_partialSVD.R:82-89) -- INTEGRATION.md 2c shows the R side.
 * Devices: TPG_DEVICES (a count; default = all visible). */
static tpg_multi* g_multi = NULL;

static tpg_multi* multi(void) {
  if (!g_multi) {
    int ndev = 0;
    const char* e = getenv("TPG_DEVICES");
    if (e) ndev = atoi(e);
    else TPG_R(tpg_device_count(&ndev));
    if (ndev < 1) Rf_error("tidypopgen (GPU): no HIP device");
    TPG_R(tpg_multi_create(ndev, NULL, &g_multi));
  }
  return g_multi;
}


/* tpg_snp_pairwise(BM, rowInd, colInd, adjusted_counts, which) -> list(ibs, king, allele_sharing, grm), each n x n or NULL.
 * which: integer mask of the matrices wanted (1 ibs, 2 king, 4 allele_sharing, 8 grm; NULL = all four).  Only the
 * cross-products those need are accumulated (tpg_multi_pairwise): 2 of 5 for the GRM alone, 4 for KING + GRM. */
SEXP _tidypopgen_tpg_snp_pairwise(SEXP BM, SEXP rowInd, SEXP colInd, SEXP adjusted_counts, SEXP which) {
  rowInd = PROTECT(as_int(rowInd));
  colInd = PROTECT(as_int(colInd));
  mapped_file* f = genotype_fbm(BM);
  const uint8_t* bytes = (const uint8_t*)f->map;
  const int64_t nrow = f->nrow, ncol = f->ncol;
  const int n = (int)XLENGTH(rowInd);
  const int want = which == R_NilValue ? 15 : Rf_asInteger(which);
  if (want < 1 || want > 15) Rf_error("tidypopgen (HIP): which must be a mask of 1 (ibs), 2 (king), 4 (allele_sharing), 8 (grm)");
  SEXP mats[4];
  for (int k = 0; k < 4; k++) mats[k] = PROTECT((want >> k) & 1 ? Rf_allocMatrix(REALSXP, n, n) : R_NilValue);
  TPG_R(tpg_multi_pairwise(multi(), bytes, nrow, ncol, INTEGER(rowInd), n, INTEGER(colInd), (int64_t)XLENGTH(colInd),
                           Rf_asLogical(adjusted_counts) ? TPG_IBS_ADJUSTED_COUNTS : TPG_IBS_PROPORTION,
                           mats[0] != R_NilValue ? REAL(mats[0]) : NULL, mats[1] != R_NilValue ? REAL(mats[1]) : NULL,
                           mats[2] != R_NilValue ? REAL(mats[2]) : NULL, mats[3] != R_NilValue ? REAL(mats[3]) : NULL));
  static const char* names[4] = {"ibs", "king", "allele_sharing", "grm"};
  SEXP out = named_list(4, names, mats);
  UNPROTECT(6);
  return out;
}

/* tpg_grouped_alt_freq(BM, rowInd, colInd, groupIds, ngroups, ploidy, as_counts) -> m x 2G (groupIds NULL: m x 2) */
SEXP _tidypopgen_tpg_grouped_alt_freq(SEXP BM, SEXP rowInd, SEXP colInd, SEXP groupIds, SEXP ngroups, SEXP ploidy,
                                      SEXP as_counts) {
  rowInd = PROTECT(as_int(rowInd));
  colInd = PROTECT(as_int(colInd));
  mapped_file* f = genotype_fbm(BM);
  const int grouped = groupIds != R_NilValue;
  const int G = grouped ? Rf_asInteger(ngroups) : 0;
  SEXP pl = PROTECT(Rf_coerceVector(ploidy, REALSXP));
  SEXP gid = PROTECT(grouped ? Rf_coerceVector(groupIds, INTSXP) : R_NilValue);
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, (int)XLENGTH(colInd), grouped ? 2 * G : 2));
  TPG_R(tpg_multi_grouped_alt_freq(multi(), (const uint8_t*)f->map, f->nrow, f->ncol, INTEGER(rowInd), (int64_t)XLENGTH(rowInd),
                                   INTEGER(colInd), (int64_t)XLENGTH(colInd), code256_of(BM), grouped ? INTEGER(gid) : NULL, G,
                                   REAL(pl), Rf_asLogical(as_counts), REAL(out)));
  UNPROTECT(5);
  return out;
}

/* tpg_pairwise_pop_fst(BM, rowInd, colInd, groupIds, ngroups, ploidy, method, pairwise_combn, by_locus, return_num_dem)
 * method: 0 Hudson, 1 Nei87, 2 WC84.  Same list as the three loop functions return. */
SEXP _tidypopgen_tpg_pairwise_pop_fst(SEXP BM, SEXP rowInd, SEXP colInd, SEXP groupIds, SEXP ngroups, SEXP ploidy, SEXP method,
                                      SEXP pairwise_combn, SEXP by_locus, SEXP return_num_dem) {
  rowInd = PROTECT(as_int(rowInd));
  colInd = PROTECT(as_int(colInd));
  mapped_file* f = genotype_fbm(BM);
  const int G = Rf_asInteger(ngroups), m = (int)XLENGTH(colInd);
  SEXP pl = PROTECT(Rf_coerceVector(ploidy, REALSXP));
  SEXP gid = PROTECT(Rf_coerceVector(groupIds, INTSXP));
  SEXP pc = PROTECT(Rf_coerceVector(pairwise_combn, INTSXP));
  const int P = (int)(XLENGTH(pc) / 2), rnd = Rf_asLogical(return_num_dem), want_a = Rf_asLogical(by_locus) || rnd;
  SEXP tot = PROTECT(Rf_allocVector(REALSXP, P));
  SEXP a = PROTECT(Rf_allocMatrix(REALSXP, want_a ? m : 0, want_a ? P : 0));
  SEXP b = PROTECT(Rf_allocMatrix(REALSXP, rnd ? m : 0, rnd ? P : 0));
  TPG_R(tpg_multi_pop_fst(multi(), (const uint8_t*)f->map, f->nrow, f->ncol, INTEGER(rowInd), (int64_t)XLENGTH(rowInd),
                          INTEGER(colInd), m, code256_of(BM), INTEGER(gid), G, REAL(pl), Rf_asInteger(method), INTEGER(pc), P,
                          want_a, rnd, REAL(tot), want_a ? REAL(a) : NULL, rnd ? REAL(b) : NULL));
  SEXP out;
  if (!rnd) {
    static const char* names[2] = {"fst_locus", "fst_tot"};
    SEXP vals[2] = {a, tot};
    out = named_list(2, names, vals);
  } else {
    static const char* names[2] = {"Fst_by_locus_num", "Fst_by_locus_den"};
    SEXP vals[2] = {a, b};
    out = named_list(2, names, vals);
  }
  UNPROTECT(8);
  return out;
}

/* tpg_pca_partial_svd(BM, rowInd, colInd, k) -> list(d, u, v, center, scale, square_frobenius): what big_SVD returns to
 * gt_pca_partialSVD (R/gt_pca_partialSVD.R:82-105) plus the squared Frobenius norm of R/square_frobenius.R */
SEXP _tidypopgen_tpg_pca_partial_svd(SEXP BM, SEXP rowInd, SEXP colInd, SEXP k) {
  rowInd = PROTECT(as_int(rowInd));
  colInd = PROTECT(as_int(colInd));
  mapped_file* f = genotype_fbm(BM);
  const int n = (int)XLENGTH(rowInd), m = (int)XLENGTH(colInd), K = Rf_asInteger(k);
  SEXP vals[6];
  vals[0] = PROTECT(Rf_allocVector(REALSXP, K));
  vals[1] = PROTECT(Rf_allocMatrix(REALSXP, n, K));
  vals[2] = PROTECT(Rf_allocMatrix(REALSXP, m, K));
  vals[3] = PROTECT(Rf_allocVector(REALSXP, m));
  vals[4] = PROTECT(Rf_allocVector(REALSXP, m));
  vals[5] = PROTECT(Rf_allocVector(REALSXP, 1));
  TPG_R(tpg_multi_pca_partial_svd(multi(), (const uint8_t*)f->map, f->nrow, f->ncol, INTEGER(rowInd), n, INTEGER(colInd), m,
                                  code256_of(BM), K, REAL(vals[0]), REAL(vals[1]), REAL(vals[2]), REAL(vals[3]), REAL(vals[4]),
                                  REAL(vals[5])));
  static const char* names[6] = {"d", "u", "v", "center", "scale", "square_frobenius"};
  SEXP out = named_list(6, names, vals);
  UNPROTECT(8);
  return out;
}

/* ---- Hardy-Weinberg exact tests ------------------------------------------------------------------------------ */

/* The three library symbols are referenced weakly, as those of tpg_impute_simple are: the shim still links and loads
 * against a library built before they existed (and against the host-only stand-in of the sanitizer jobs); the call then is
 * an R error. */
#pragma weak tpg_hwe_exact_counts
#pragma weak tpg_loci_hwe
#pragma weak tpg_gt_grouped_hwe
#define TPG_NEEDS(sym) \
  do { \
    if (!(sym)) Rf_error("tidypopgen (GPU): this libtpg_hip has no " #sym); \
  } while (0)

static int midp_of(SEXP midp) { /* Rcpp's uint32_t midp: TRUE / FALSE / a number; the test only asks whether it is set */
  const int v = Rf_asLogical(midp);
  if (v == NA_INTEGER) Rf_error("tidypopgen (GPU): midp must be TRUE or FALSE");
  return v != 0;
}

/* SNPHWE2_R(obs_hets, obs_hom1, obs_hom2, midp)   src/hwe.cpp:193-200: one table, heterozygotes first.  No device call. */
SEXP _tidypopgen_SNPHWE2_R(SEXP obs_hets, SEXP obs_hom1, SEXP obs_hom2, SEXP midp) {
  const int het = Rf_asInteger(obs_hets), hom1 = Rf_asInteger(obs_hom1), hom2 = Rf_asInteger(obs_hom2), mid = midp_of(midp);
  if (het == NA_INTEGER || hom1 == NA_INTEGER || hom2 == NA_INTEGER || het < 0 || hom1 < 0 || hom2 < 0)
    Rf_error("tidypopgen (GPU): genotype counts must be non-negative integers");
  SEXP out = PROTECT(Rf_allocVector(REALSXP, 1));
  REAL(out)[0] = tpg_hwe_exact(hom1, het, hom2, mid);
  UNPROTECT(1);
  return out;
}

/* hwe_on_matrix(geno_counts, midp)   src/hwe.cpp:203-213: rows 1..3 of a big_counts matrix (hom1, het, hom2; its fourth
   row, the NA count, is not read) -> one p-value per column */
SEXP _tidypopgen_hwe_on_matrix(SEXP geno_counts, SEXP midp) {
  TPG_NEEDS(tpg_hwe_exact_counts);
  const int mid = midp_of(midp);
  SEXP gc = PROTECT(as_int(geno_counts));
  SEXP dim = Rf_getAttrib(gc, R_DimSymbol);
  if (dim == R_NilValue || XLENGTH(dim) != 2 || INTEGER(dim)[0] < 3) Rf_error("tidypopgen (GPU): geno_counts must be a matrix of at least 3 rows");
  const int nr = INTEGER(dim)[0], m = INTEGER(dim)[1];
  SEXP out = PROTECT(Rf_allocVector(REALSXP, m));
  const int* tab = INTEGER(gc);
  if (nr != 3 && m > 0) {
    int* t3 = (int*)R_alloc((size_t)3 * (size_t)m, sizeof(int));
    for (int j = 0; j < m; j++)
      for (int k = 0; k < 3; k++) t3[3 * (size_t)j + k] = tab[(size_t)nr * (size_t)j + k];
    tab = t3;
  }
  for (R_xlen_t k = 0; k < (R_xlen_t)3 * m; k++)
    if (tab[k] == NA_INTEGER) Rf_error("tidypopgen (GPU): NA in geno_counts");
  TPG_R(tpg_hwe_exact_counts(ctx(), tab, m, mid, REAL(out)));
  UNPROTECT(2);
  return out;
}

/* gt_grouped_hwe(BM, rowInd, colInd, groupIds, ngroups, midp)   src/hwe.cpp:220-253 -> m x G */
SEXP _tidypopgen_gt_grouped_hwe(SEXP BM, SEXP rowInd, SEXP colInd, SEXP groupIds, SEXP ngroups, SEXP midp) {
  TPG_NEEDS(tpg_gt_grouped_hwe);
  const int G = ngroups_of(ngroups), mid = midp_of(midp);
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP gid = PROTECT(Rf_coerceVector(groupIds, INTSXP));
  if (XLENGTH(gid) != XLENGTH(ri)) Rf_error("tidypopgen (GPU): groupIds and rowInd differ in length");
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, (int)XLENGTH(ci), G));
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_gt_grouped_hwe(ctx(), v, INTEGER(gid), G, mid, REAL(out)));
  UNPROTECT(4);
  return out;
}

/* tpg_loci_hwe(BM, rowInd, colInd, midp): the whole of R/loci_hwe.R:74-89 (big_counts + hwe_on_matrix per block) in one
   call -> one p-value per locus */
SEXP _tidypopgen_tpg_loci_hwe(SEXP BM, SEXP rowInd, SEXP colInd, SEXP midp) {
  TPG_NEEDS(tpg_loci_hwe);
  const int mid = midp_of(midp);
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  if (XLENGTH(ri) < 2) Rf_error("Not implemented for a single individual"); /* R/loci_hwe.R:92 */
  SEXP out = PROTECT(Rf_allocVector(REALSXP, XLENGTH(ci)));
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_loci_hwe(ctx(), v, mid, REAL(out)));
  UNPROTECT(3);
  return out;
}

/* ---- LD clumping ---------------------------------------------------------------------------------------------- */

#pragma weak tpg_ld_clump

/* tpg_ld_clump(BM, rowInd, colInd, hi, thr_r2, S, exclude): the bigsnpr::snp_clumping call of R/loci_ld_clump.R:161-174 on
 * the loci of colInd, in one call -> a logical per locus of colInd (include/tpg.h "LD clumping" is the definition).  hi[j] =
 * the 1-based position in colInd of the last neighbour of locus j (>= j, non-decreasing), integer or double; S = NULL or one
 * double per locus; exclude = NULL or one logical per locus.  A missing genotype is an R error, as in the reference. */
SEXP _tidypopgen_tpg_ld_clump(SEXP BM, SEXP rowInd, SEXP colInd, SEXP hi, SEXP thr_r2, SEXP S, SEXP exclude) {
  TPG_NEEDS(tpg_ld_clump);
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP hr = PROTECT(as_real(hi)), tr = PROTECT(as_real(thr_r2));
  if (XLENGTH(tr) != 1) Rf_error("tidypopgen (GPU): thr_r2 must be one number");
  const double thr = REAL(tr)[0];
  SEXP sr = PROTECT(S == R_NilValue ? R_NilValue : as_real(S));
  SEXP ex = PROTECT(exclude == R_NilValue ? R_NilValue : Rf_coerceVector(exclude, LGLSXP));
  const R_xlen_t m = XLENGTH(ci);
  if (XLENGTH(hr) != m) Rf_error("tidypopgen (GPU): hi and colInd differ in length");
  if (sr != R_NilValue && XLENGTH(sr) != m) Rf_error("tidypopgen (GPU): S and colInd differ in length");
  if (ex != R_NilValue && XLENGTH(ex) != m) Rf_error("tidypopgen (GPU): exclude and colInd differ in length");
  SEXP out = PROTECT(Rf_allocVector(LGLSXP, m));
  int64_t* h0 = (int64_t*)R_alloc((size_t)(m > 0 ? m : 1), sizeof(int64_t));
  uint8_t* x8 = (uint8_t*)R_alloc((size_t)(m > 0 ? m : 1), 1); /* exclude */
  uint8_t* k8 = (uint8_t*)R_alloc((size_t)(m > 0 ? m : 1), 1); /* keep */
  for (R_xlen_t j = 0; j < m; j++) {
    const double v = REAL(hr)[j];
    if (!(v >= 1 && v <= (double)m)) Rf_error("tidypopgen (GPU): hi[%lld] is NA or out of [1,%lld]", (long long)j + 1, (long long)m);
    h0[j] = (int64_t)v - 1;
    x8[j] = 0;
    if (ex != R_NilValue) {
      if (LOGICAL(ex)[j] == NA_LOGICAL) Rf_error("tidypopgen (GPU): NA in exclude");
      x8[j] = LOGICAL(ex)[j] != 0;
    }
  }
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_ld_clump(ctx(), v, h0, thr, sr == R_NilValue ? NULL : REAL(sr), ex == R_NilValue ? NULL : x8, k8, NULL));
  for (R_xlen_t j = 0; j < m; j++) LOGICAL(out)[j] = k8[j] != 0;
  UNPROTECT(7);
  return out;
}

/* ---- runs of homozygosity -------------------------------------------------------------------------------------- */

#pragma weak tpg_roh_detect
#pragma weak tpg_roh_count
#pragma weak tpg_roh_fetch
#pragma weak tpg_roh_free

/* tpg_indiv_roh(BM, rowInd, colInd, chrom, pos, params): the per-individual loop of R/windows_indiv_roh.R:129-143 (one row
 * of the FBM and one detectRUNS::slidingRuns call per individual) in one call; include/tpg.h "Runs of homozygosity" is the
 * definition.  chrom = one integer code per locus of colInd (as.integer(factor(chromosome))), pos = its position; params =
 * 11 numbers in the order of tpg_roh_params: window_size, threshold, min_snp, heterozygosity, max_opp_window,
 * max_miss_window, max_gap, min_length_bps, min_density, max_opp_run, max_miss_run (NA in the last two: no limit).
 * -> list(indiv, nSNP, from, to, lengthBps, first, last), one entry per run ordered by (individual, first locus): indiv =
 * position in rowInd, first / last = positions in colInd, all 1-based; from / to / lengthBps in bp. */
static tpg_roh* g_roh_pending = NULL; /* the runs of a call whose R allocations are still to come: an R error there (a longjmp)
                                         leaves them here, and the next call or the unload frees them */

static void roh_drop_pending(void) {
  if (g_roh_pending && tpg_roh_free) tpg_roh_free(g_roh_pending);
  g_roh_pending = NULL;
}

static int32_t roh_int_param(const double* q, int k, double lo, double hi, const char* name) {
  if (ISNAN(q[k]) || q[k] < lo || q[k] > hi || q[k] != floor(q[k]))
    Rf_error("tidypopgen (GPU): params[%d] (%s) must be a whole number in [%.0f, %.0f]", k + 1, name, lo, hi);
  return (int32_t)q[k];
}

SEXP _tidypopgen_tpg_indiv_roh(SEXP BM, SEXP rowInd, SEXP colInd, SEXP chrom, SEXP pos, SEXP params) {
  TPG_NEEDS(tpg_roh_detect);
  roh_drop_pending();
  if ((TYPEOF(chrom) != INTSXP && TYPEOF(chrom) != REALSXP) || (TYPEOF(pos) != INTSXP && TYPEOF(pos) != REALSXP) ||
      (TYPEOF(params) != INTSXP && TYPEOF(params) != REALSXP))
    Rf_error("tidypopgen (GPU): chrom, pos and params must be integer or double vectors");
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP ch = PROTECT(as_int(chrom)), ps = PROTECT(as_real(pos)), pr = PROTECT(as_real(params));
  const R_xlen_t m = XLENGTH(ci);
  if (XLENGTH(ch) != m || XLENGTH(ps) != m) Rf_error("tidypopgen (GPU): chrom / pos and colInd differ in length");
  if (XLENGTH(pr) != 11) Rf_error("tidypopgen (GPU): params must be the 11 numbers of tpg_roh_params");
  const double* q = REAL(pr);
  for (int k = 0; k < 9; k++)
    if (ISNAN(q[k])) Rf_error("tidypopgen (GPU): NA in params[%d]", k + 1);
  const double big = 2147483647.0, big64 = 9007199254740992.0; /* 2^53: the whole numbers a double holds exactly */
  tpg_roh_params P;
  P.window_size = roh_int_param(q, 0, -big, big, "window_size"); /* (the library says which windows it takes) */
  P.threshold = q[1];
  P.min_snp = roh_int_param(q, 2, -big, big, "min_snp");
  P.heterozygosity = q[3] != 0;
  P.max_opp_window = roh_int_param(q, 4, -big, big, "max_opp_window");
  P.max_miss_window = roh_int_param(q, 5, -big, big, "max_miss_window");
  if (fabs(q[6]) > big64 || fabs(q[7]) > big64) Rf_error("tidypopgen (GPU): max_gap / min_length_bps out of range");
  P.max_gap = (int64_t)q[6];
  P.min_length_bps = (int64_t)q[7];
  P.min_density = q[8];
  P.max_opp_run = ISNAN(q[9]) ? -1 : roh_int_param(q, 9, -big, big, "max_opp_run");
  P.max_miss_run = ISNAN(q[10]) ? -1 : roh_int_param(q, 10, -big, big, "max_miss_run");
  int64_t* p64 = (int64_t*)R_alloc((size_t)(m > 0 ? m : 1), sizeof(int64_t));
  for (R_xlen_t j = 0; j < m; j++) {
    if (INTEGER(ch)[j] == NA_INTEGER || !isfinite(REAL(ps)[j]) || fabs(REAL(ps)[j]) > big64)
      Rf_error("tidypopgen (GPU): NA in chrom or pos");
    p64[j] = (int64_t)REAL(ps)[j];
  }
  tpg_view* v = view_of(BM, ri, ci, 0);
  tpg_roh* r = NULL;
  TPG_R_VIEW(v, tpg_roh_detect(ctx(), v, INTEGER(ch), p64, &P, &r));
  g_roh_pending = r; /* from here to roh_drop_pending() every R allocation may raise an error */
  const int64_t c = tpg_roh_count(r);
  if (c > INT32_MAX) Rf_error("tidypopgen (GPU): too many runs for an R vector of integers");
  SEXP vals[7];
  static const char* names[7] = {"indiv", "nSNP", "from", "to", "lengthBps", "first", "last"};
  static const int is_real[7] = {0, 0, 1, 1, 1, 0, 0};
  for (int k = 0; k < 7; k++) vals[k] = PROTECT(Rf_allocVector(is_real[k] ? REALSXP : INTSXP, (R_xlen_t)c));
  int64_t* ab = (int64_t*)R_alloc((size_t)(c > 0 ? 2 * c : 1), sizeof(int64_t));
  const int rc = tpg_roh_fetch(ctx(), r, (int32_t*)INTEGER(vals[0]), ab, ab + c, NULL, NULL);
  roh_drop_pending();
  if (rc != TPG_OK) Rf_error("tidypopgen (GPU): %s", tpg_last_error());
  for (int64_t k = 0; k < c; k++) {
    const int64_t a = ab[k], b = ab[c + k];
    INTEGER(vals[0])[k] += 1;
    INTEGER(vals[1])[k] = (int)(b - a + 1);
    REAL(vals[2])[k] = (double)p64[a];
    REAL(vals[3])[k] = (double)p64[b];
    REAL(vals[4])[k] = (double)(p64[b] - p64[a]);
    INTEGER(vals[5])[k] = (int)a + 1;
    INTEGER(vals[6])[k] = (int)b + 1;
  }
  SEXP out = named_list(7, names, vals);
  UNPROTECT(12);
  return out;
}

/* ---- Tajima's D ------------------------------------------------------------------------------------------------- */

#pragma weak tpg_pop_tajimas_d
#pragma weak tpg_windows_pop_tajimas_d

/* groupIds as the grouped entry points take it, or NULL (one group of everybody: ngroups must then be 1).  The result is
 * returned UNPROTECTED: the caller must PROTECT it before anything else allocates (both callers do so in the same statement). */
static SEXP tajima_groups(SEXP groupIds, SEXP ri, int G) {
  if (groupIds == R_NilValue) {
    if (G != 1) Rf_error("tidypopgen (GPU): groupIds = NULL means one group, ngroups must be 1");
    return R_NilValue;
  }
  SEXP gid = PROTECT(Rf_coerceVector(groupIds, INTSXP));
  if (XLENGTH(gid) != XLENGTH(ri)) Rf_error("tidypopgen (GPU): groupIds and rowInd differ in length");
  UNPROTECT(1);
  return gid;
}

/* tpg_pop_tajimas_d(BM, rowInd, colInd, groupIds, ngroups): the big_apply of gt_grouped_pi_diploid and the loop over groups
 * of R/pop_tajimas_d.R:113-147 in one call (include/tpg.h "Tajima's D") -> one D per group; groupIds = NULL: one group */
SEXP _tidypopgen_tpg_pop_tajimas_d(SEXP BM, SEXP rowInd, SEXP colInd, SEXP groupIds, SEXP ngroups) {
  TPG_NEEDS(tpg_pop_tajimas_d);
  const int G = ngroups_of(ngroups);
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP gid = PROTECT(tajima_groups(groupIds, ri, G));
  SEXP out = PROTECT(Rf_allocVector(REALSXP, G));
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_pop_tajimas_d(ctx(), v, gid == R_NilValue ? NULL : INTEGER(gid), G, NULL, REAL(out), NULL, NULL));
  UNPROTECT(4);
  return out;
}

/* tpg_windows_pop_tajimas_d(BM, rowInd, colInd, groupIds, ngroups, lo, hi, pad_na, min_loci): loci_pi and the
 * windows_stats_generic(operator = "custom") call per group of R/windows_pop_tajimas_d.R:80-103 in one call.  lo / hi =
 * 0-based half-open locus ranges (positions in colInd), integer or double; pad_na = logical, or NULL.
 * -> list(stat, n_loci), nw x ngroups each: stat is NA_real_ where the reference assigns NA (a pad window, n_loci <
 * min_loci) and the arithmetic value elsewhere, a NaN included; n_loci is NA_integer_ on a pad window. */
SEXP _tidypopgen_tpg_windows_pop_tajimas_d(SEXP BM, SEXP rowInd, SEXP colInd, SEXP groupIds, SEXP ngroups, SEXP lo, SEXP hi,
                                           SEXP pad_na, SEXP min_loci) {
  TPG_NEEDS(tpg_windows_pop_tajimas_d);
  const int G = ngroups_of(ngroups);
  if ((TYPEOF(lo) != INTSXP && TYPEOF(lo) != REALSXP) || (TYPEOF(hi) != INTSXP && TYPEOF(hi) != REALSXP))
    Rf_error("tidypopgen (GPU): lo and hi must be integer or double vectors");
  const int ml = Rf_asInteger(min_loci);
  if (ml == NA_INTEGER || ml < 1) Rf_error("min_loci must be positive."); /* R/windows_stats_generic.R:101-103 */
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP gid = PROTECT(tajima_groups(groupIds, ri, G));
  SEXP lr = PROTECT(as_real(lo)), hr = PROTECT(as_real(hi));
  SEXP pr = PROTECT(pad_na == R_NilValue ? R_NilValue : Rf_coerceVector(pad_na, LGLSXP));
  const R_xlen_t nw = XLENGTH(lr);
  if (XLENGTH(hr) != nw || (pr != R_NilValue && XLENGTH(pr) != nw)) Rf_error("tidypopgen (GPU): lo, hi and pad_na differ in length");
  if (nw > INT_MAX) Rf_error("tidypopgen (GPU): too many windows for an R matrix");
  SEXP mats[2];
  mats[0] = PROTECT(Rf_allocMatrix(REALSXP, (int)nw, G));
  mats[1] = PROTECT(Rf_allocMatrix(INTSXP, (int)nw, G));
  static const char* names[2] = {"stat", "n_loci"};
  SEXP out = PROTECT(named_list(2, names, mats));
  int64_t* w64 = (int64_t*)R_alloc((size_t)(nw > 0 ? 2 * nw : 1), sizeof(int64_t));
  uint8_t* p8 = (uint8_t*)R_alloc((size_t)(nw > 0 ? nw : 1), 1);
  const double m = (double)XLENGTH(ci);
  for (R_xlen_t w = 0; w < nw; w++) {
    const double a = REAL(lr)[w], b = REAL(hr)[w];
    if (!(a >= 0 && a <= b && b <= m) || a != floor(a) || b != floor(b))
      Rf_error("tidypopgen (GPU): window %lld is NA, not whole numbers or outside [0, %.0f]", (long long)w + 1, m);
    w64[w] = (int64_t)a;
    w64[nw + w] = (int64_t)b;
    p8[w] = 0;
    if (pr != R_NilValue) {
      if (LOGICAL(pr)[w] == NA_LOGICAL) Rf_error("tidypopgen (GPU): NA in pad_na");
      p8[w] = LOGICAL(pr)[w] != 0;
    }
  }
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_windows_pop_tajimas_d(ctx(), v, gid == R_NilValue ? NULL : INTEGER(gid), G, NULL, w64, w64 + nw, p8,
                                          (int64_t)nw, ml, REAL(mats[0]), NULL, NULL, (int32_t*)INTEGER(mats[1])));
  double* stat = REAL(mats[0]);
  int* nl = INTEGER(mats[1]);
  for (R_xlen_t k = 0; k < nw * (R_xlen_t)G; k++) {
    if (nl[k] < 0 || nl[k] < ml) stat[k] = NA_REAL; /* results$stat[results$n_loci < min_loci] <- NA, and runner's na_pad */
    if (nl[k] < 0) nl[k] = NA_INTEGER;
  }
  UNPROTECT(9);
  return out;
}

/* ---- windowed pairwise Fst and PBS ------------------------------------------------------------------------------- */

#pragma weak tpg_windows_pairwise_pop_fst
/* the PBS row keeps the window Fst in device memory between two library calls: the three symbols it does that with and the PBS
 * kernel's entry point are weak as well, so that the shim still links against the host-only stand-in, which has none of them */
#pragma weak tpg_dev_alloc
#pragma weak tpg_dev_free
#pragma weak tpg_dev_to_host
#pragma weak tpg_pbs_from_fst

/* lo / hi (REALSXP, coerced by the caller) and pad_na (LGLSXP or NULL) as _tidypopgen_tpg_windows_pop_tajimas_d checks them:
 * whole numbers with 0 <= lo <= hi <= m.  w64 = lo[nw] then hi[nw], p8 = the pad flags, both in R's transient storage. */
static R_xlen_t winfst_windows(SEXP lr, SEXP hr, SEXP pr, double m, int64_t** w64_out, uint8_t** p8_out) {
  const R_xlen_t nw = XLENGTH(lr);
  if (XLENGTH(hr) != nw || (pr != R_NilValue && XLENGTH(pr) != nw)) Rf_error("tidypopgen (GPU): lo, hi and pad_na differ in length");
  if (nw > INT_MAX) Rf_error("tidypopgen (GPU): too many windows for an R matrix");
  int64_t* w64 = (int64_t*)R_alloc((size_t)(nw > 0 ? 2 * nw : 1), sizeof(int64_t));
  uint8_t* p8 = (uint8_t*)R_alloc((size_t)(nw > 0 ? nw : 1), 1);
  for (R_xlen_t w = 0; w < nw; w++) {
    const double a = REAL(lr)[w], b = REAL(hr)[w];
    if (!(a >= 0 && a <= b && b <= m) || a != floor(a) || b != floor(b))
      Rf_error("tidypopgen (GPU): window %lld is NA, not whole numbers or outside [0, %.0f]", (long long)w + 1, m);
    w64[w] = (int64_t)a;
    w64[nw + w] = (int64_t)b;
    p8[w] = 0;
    if (pr != R_NilValue) {
      if (LOGICAL(pr)[w] == NA_LOGICAL) Rf_error("tidypopgen (GPU): NA in pad_na");
      p8[w] = LOGICAL(pr)[w] != 0;
    }
  }
  *w64_out = w64;
  *p8_out = p8;
  return nw;
}

/* utils::combn(G, 2), 1-based, 2 x P column-major, in R's transient storage */
static int32_t* winfst_pairs(int G) {
  const int P = G * (G - 1) / 2;
  int32_t* pairs = (int32_t*)R_alloc((size_t)(P > 0 ? 2 * P : 1), sizeof(int32_t));
  int k = 0;
  for (int a = 1; a <= G; a++)
    for (int b = a + 1; b <= G; b++) {
      pairs[2 * k] = a;
      pairs[2 * k + 1] = b;
      k++;
    }
  return pairs;
}

/* the arguments both rows share, checked in the order of _tidypopgen_tpg_windows_pop_tajimas_d; at least 2 (Fst) or 3 (PBS) groups */
static int winfst_checks(SEXP ngroups, SEXP lo, SEXP hi, SEXP min_loci, int min_groups, int* ml_out) {
  const int G = ngroups_of(ngroups);
  if (G < min_groups) {
    if (min_groups == 3) Rf_error("At least 3 populations are required to compute PBS."); /* R/nwise_pop_pbs.R */
    Rf_error("tidypopgen (GPU): pairwise Fst needs at least 2 populations");
  }
  if (G > 2048) Rf_error("tidypopgen (GPU): too many populations for a matrix of pairs");
  if ((TYPEOF(lo) != INTSXP && TYPEOF(lo) != REALSXP) || (TYPEOF(hi) != INTSXP && TYPEOF(hi) != REALSXP))
    Rf_error("tidypopgen (GPU): lo and hi must be integer or double vectors");
  const int ml = Rf_asInteger(min_loci);
  if (ml == NA_INTEGER || ml < 1) Rf_error("min_loci must be positive."); /* R/windows_stats_generic.R:101-103 */
  *ml_out = ml;
  return G;
}

/* tpg_windows_pairwise_pop_fst(BM, rowInd, colInd, groupIds, ngroups, method, lo, hi, pad_na, min_loci): the by-locus
 * numerators and denominators and the two windows_stats_generic(operator = "mean") calls of
 * R/windows_pairwise_pop_fst.R:62-107 in one call that never forms them (include/tpg.h "windowed pairwise Fst").  method: 0
 * Hudson (what the reference always takes here), 1 Nei87, 2 WC84; every pair of utils::combn(ngroups, 2); lo / hi / pad_na as
 * _tidypopgen_tpg_windows_pop_tajimas_d takes them.  -> the nw x P matrix of window Fst: NA_real_ where the reference assigns
 * NA (a pad window, fewer than min_loci numerators or denominators), the arithmetic value elsewhere, a NaN included. */
SEXP _tidypopgen_tpg_windows_pairwise_pop_fst(SEXP BM, SEXP rowInd, SEXP colInd, SEXP groupIds, SEXP ngroups, SEXP method, SEXP lo,
                                              SEXP hi, SEXP pad_na, SEXP min_loci) {
  TPG_NEEDS(tpg_windows_pairwise_pop_fst);
  int ml;
  const int G = winfst_checks(ngroups, lo, hi, min_loci, 2, &ml);
  const int meth = Rf_asInteger(method);
  if (meth == NA_INTEGER || meth < 0 || meth > 2) Rf_error("tidypopgen (GPU): method must be 0 (Hudson), 1 (Nei87) or 2 (WC84)");
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP gid = PROTECT(Rf_coerceVector(groupIds, INTSXP));
  if (XLENGTH(gid) != XLENGTH(ri)) Rf_error("tidypopgen (GPU): groupIds and rowInd differ in length");
  SEXP lr = PROTECT(as_real(lo)), hr = PROTECT(as_real(hi));
  SEXP pr = PROTECT(pad_na == R_NilValue ? R_NilValue : Rf_coerceVector(pad_na, LGLSXP));
  int64_t* w64;
  uint8_t* p8;
  const R_xlen_t nw = winfst_windows(lr, hr, pr, (double)XLENGTH(ci), &w64, &p8);
  const int P = G * (G - 1) / 2;
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, (int)nw, P));
  const int32_t* pairs = winfst_pairs(G);
  const size_t cells = (size_t)nw * (size_t)P;
  int32_t* nn = (int32_t*)R_alloc(cells > 0 ? 2 * cells : 1, sizeof(int32_t));
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_windows_pairwise_pop_fst(ctx(), v, INTEGER(gid), G, NULL, meth, pairs, P, w64, w64 + nw, p8, (int64_t)nw, ml,
                                             REAL(out), NULL, NULL, nn, nn + cells));
  double* f = REAL(out);
  for (size_t k = 0; k < cells; k++)
    if (nn[k] < ml || nn[cells + k] < ml) f[k] = NA_REAL; /* stat[n_loci < min_loci] <- NA of either mean, and runner's na_pad */
  UNPROTECT(7);
  return out;
}

/* tpg_windows_nwise_pop_pbs(BM, rowInd, colInd, groupIds, ngroups, lo, hi, pad_na, min_loci, return_fst):
 * R/windows_nwise_pop_pbs.R:78-114 -- the windowed Hudson Fst above (the reference's windows_pairwise_pop_fst takes Hudson
 * whatever it is told) kept in device memory, and pbs_one_triplet of R/nwise_pop_pbs.R:116-157 on it for every triplet of
 * utils::combn(ngroups, 3).  -> list(pbs, fst): pbs nw x 6 T (per triplet pbs_1, pbs_2, pbs_3, pbsn1_1, pbsn1_2, pbsn1_3),
 * NA_real_ where one of the triplet's three Fst is NA; fst the nw x P matrix of the row above, or NULL unless return_fst. */
SEXP _tidypopgen_tpg_windows_nwise_pop_pbs(SEXP BM, SEXP rowInd, SEXP colInd, SEXP groupIds, SEXP ngroups, SEXP lo, SEXP hi,
                                           SEXP pad_na, SEXP min_loci, SEXP return_fst) {
  TPG_NEEDS(tpg_windows_pairwise_pop_fst);
  TPG_NEEDS(tpg_pbs_from_fst);
  TPG_NEEDS(tpg_dev_alloc);
  TPG_NEEDS(tpg_dev_free);
  TPG_NEEDS(tpg_dev_to_host);
  int ml;
  const int G = winfst_checks(ngroups, lo, hi, min_loci, 3, &ml);
  const int want_fst = Rf_asLogical(return_fst);
  if (want_fst == NA_LOGICAL) Rf_error("return_fst must be a logical value (TRUE or FALSE)");
  const int P = G * (G - 1) / 2;
  const double T_d = (double)G * (G - 1) * (G - 2) / 6.0;
  if (6.0 * T_d > (double)INT_MAX) Rf_error("tidypopgen (GPU): too many triplets for an R matrix");
  const int T = (int)T_d;
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP gid = PROTECT(Rf_coerceVector(groupIds, INTSXP));
  if (XLENGTH(gid) != XLENGTH(ri)) Rf_error("tidypopgen (GPU): groupIds and rowInd differ in length");
  SEXP lr = PROTECT(as_real(lo)), hr = PROTECT(as_real(hi));
  SEXP pr = PROTECT(pad_na == R_NilValue ? R_NilValue : Rf_coerceVector(pad_na, LGLSXP));
  int64_t* w64;
  uint8_t* p8;
  const R_xlen_t nw = winfst_windows(lr, hr, pr, (double)XLENGTH(ci), &w64, &p8);
  if ((double)nw * 6.0 * T_d > 4503599627370496.0) Rf_error("tidypopgen (GPU): the PBS matrix is too large");
  SEXP vals[2];
  vals[0] = PROTECT(Rf_allocMatrix(REALSXP, (int)nw, 6 * T));
  vals[1] = PROTECT(want_fst ? Rf_allocMatrix(REALSXP, (int)nw, P) : R_NilValue);
  static const char* names[2] = {"pbs", "fst"};
  SEXP out = PROTECT(named_list(2, names, vals));
  const int32_t* pairs = winfst_pairs(G);
  /* the Fst columns (p1.p2, p1.p3, p2.p3) of every triplet, 0-based, triplets and pairs in combn order */
  int32_t* trip = (int32_t*)R_alloc((size_t)3 * (size_t)T, sizeof(int32_t));
  {
    int t = 0;
#define WINFST_COL(a, b) (((a) - 1) * G - ((a) - 1) * (a) / 2 + ((b) - (a) - 1)) /* the column of pair (a, b), a < b, 1-based */
    for (int a = 1; a <= G; a++)
      for (int b = a + 1; b <= G; b++)
        for (int c = b + 1; c <= G; c++) {
          trip[3 * t] = WINFST_COL(a, b);
          trip[3 * t + 1] = WINFST_COL(a, c);
          trip[3 * t + 2] = WINFST_COL(b, c);
          t++;
        }
#undef WINFST_COL
  }
  const size_t cells = (size_t)nw * (size_t)P;
  int32_t* nn = (int32_t*)R_alloc(cells > 0 ? 2 * cells : 1, sizeof(int32_t));
  tpg_view* v = view_of(BM, ri, ci, 0);
  /* from here to the release of the view and the device buffer nothing may longjmp: the status is looked at afterwards */
  void* d_fst = NULL;
  const size_t fst_bytes = sizeof(double) * cells;
  int rc = tpg_dev_alloc(ctx(), fst_bytes, &d_fst);
  if (rc == TPG_OK)
    rc = tpg_windows_pairwise_pop_fst(ctx(), v, INTEGER(gid), G, NULL, TPG_FST_HUDSON, pairs, P, w64, w64 + nw, p8, (int64_t)nw, ml,
                                      (double*)d_fst, NULL, NULL, nn, nn + cells);
  if (rc == TPG_OK && nw > 0) rc = tpg_pbs_from_fst(ctx(), (const double*)d_fst, (int64_t)nw, P, trip, T, REAL(vals[0]));
  if (rc == TPG_OK && nw > 0 && want_fst) rc = tpg_dev_to_host(ctx(), REAL(vals[1]), d_fst, fst_bytes);
  if (d_fst) tpg_dev_free(d_fst);
  tpg_view_free(v);
  if (rc != TPG_OK) Rf_error("tidypopgen (GPU): %s", tpg_last_error());
  double* pbs = REAL(vals[0]);
  for (int t = 0; t < T; t++)
    for (R_xlen_t w = 0; w < nw; w++) {
      int na = 0;
      for (int q = 0; q < 3; q++) {
        const size_t k = (size_t)w + (size_t)trip[3 * t + q] * (size_t)nw;
        na |= nn[k] < ml || nn[cells + k] < ml;
      }
      if (na)
        for (int q = 0; q < 6; q++) pbs[(size_t)w + ((size_t)6 * (size_t)t + (size_t)q) * (size_t)nw] = NA_REAL;
    }
  if (want_fst) {
    double* f = REAL(vals[1]);
    for (size_t k = 0; k < cells; k++)
      if (nn[k] < ml || nn[cells + k] < ml) f[k] = NA_REAL;
  }
  UNPROTECT(9);
  return out;
}

/* ---- f2 blocks ---------------------------------------------------------------------------------------------------- */

#pragma weak tpg_f2_blocks
#pragma weak tpg_f2_params_default

static SEXP f2_array(SEXPTYPE type, int G, R_xlen_t nb) { /* G x G x nb, returned UNPROTECTED (the caller protects it at once) */
  SEXP a = PROTECT(Rf_allocVector(type, (R_xlen_t)G * G * nb));
  SEXP d = PROTECT(Rf_allocVector(INTSXP, 3));
  INTEGER(d)[0] = G;
  INTEGER(d)[1] = G;
  INTEGER(d)[2] = (int)nb;
  Rf_setAttrib(a, R_DimSymbol, d);
  UNPROTECT(2);
  return a;
}

/* tpg_f2_blocks(BM, rowInd, colInd, groupIds, ngroups, ploidy, lo, hi, params): gt_to_aftable, discard_from_aftable and
 * afs_to_f2_blocks of R/gt_extract_f2.R:141-189 in one call (include/tpg.h "f2 blocks").  ploidy = NULL: all diploid.  lo / hi =
 * 0-based half-open locus ranges (positions in colInd), integer or double.  params = c(maxmiss, minmaf, maxmaf, minac2,
 * poly_only, apply_corr), optionally followed by the keep mask of the loci (one 0 / 1 per entry of colInd).
 * -> list(f2, counts, ap, ap_counts: G x G x nb arrays; block_lengths: double[nb]).  NaN where a pair has no locus. */
SEXP _tidypopgen_tpg_f2_blocks(SEXP BM, SEXP rowInd, SEXP colInd, SEXP groupIds, SEXP ngroups, SEXP ploidy, SEXP lo, SEXP hi,
                               SEXP params) {
  TPG_NEEDS(tpg_f2_blocks);
  const int G = ngroups_of(ngroups);
  if ((TYPEOF(lo) != INTSXP && TYPEOF(lo) != REALSXP) || (TYPEOF(hi) != INTSXP && TYPEOF(hi) != REALSXP) ||
      (TYPEOF(params) != INTSXP && TYPEOF(params) != REALSXP && TYPEOF(params) != LGLSXP))
    Rf_error("tidypopgen (GPU): lo, hi and params must be integer or double vectors");
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP gid = PROTECT(tajima_groups(groupIds, ri, G));
  SEXP pl = PROTECT(ploidy == R_NilValue ? R_NilValue : Rf_coerceVector(ploidy, REALSXP));
  SEXP lr = PROTECT(as_real(lo)), hr = PROTECT(as_real(hi)), pr = PROTECT(as_real(params));
  const R_xlen_t nb = XLENGTH(lr), m = XLENGTH(ci);
  if (XLENGTH(hr) != nb) Rf_error("tidypopgen (GPU): lo and hi differ in length");
  if (pl != R_NilValue && XLENGTH(pl) != XLENGTH(ri)) Rf_error("tidypopgen (GPU): ploidy and rowInd differ in length");
  if (XLENGTH(pr) != 6 && XLENGTH(pr) != 6 + m)
    Rf_error("tidypopgen (GPU): params must be the 6 numbers of tpg_f2_params, alone or followed by one keep flag per locus");
  if ((double)G * G * (double)nb > 2147483647.0) Rf_error("tidypopgen (GPU): too many blocks for an R integer array");
  const double* q = REAL(pr);
  for (R_xlen_t k = 0; k < XLENGTH(pr); k++)
    if (ISNAN(q[k])) Rf_error("tidypopgen (GPU): NA in params[%lld]", (long long)k + 1);
  tpg_f2_params P;
  tpg_f2_params_default(&P);
  P.maxmiss = q[0];
  P.minmaf = q[1];
  P.maxmaf = q[2];
  P.minac2 = roh_int_param(q, 3, 0, 1, "minac2");
  P.poly_only = roh_int_param(q, 4, 0, 3, "poly_only");
  P.apply_corr = q[5] != 0;
  uint8_t* keep = NULL;
  if (XLENGTH(pr) > 6) {
    keep = (uint8_t*)R_alloc((size_t)(m > 0 ? m : 1), 1);
    for (R_xlen_t j = 0; j < m; j++) keep[j] = q[6 + j] != 0;
  }
  P.keep = keep;
  int64_t* b64 = (int64_t*)R_alloc((size_t)(nb > 0 ? 3 * nb : 1), sizeof(int64_t));
  for (R_xlen_t b = 0; b < nb; b++) {
    const double x = REAL(lr)[b], y = REAL(hr)[b];
    if (!(x >= 0 && x <= y && y <= (double)m) || x != floor(x) || y != floor(y))
      Rf_error("tidypopgen (GPU): block %lld is NA, not whole numbers or outside [0, %.0f]", (long long)b + 1, (double)m);
    b64[b] = (int64_t)x;
    b64[nb + b] = (int64_t)y;
  }
  SEXP vals[5];
  vals[0] = PROTECT(f2_array(REALSXP, G, nb));
  vals[1] = PROTECT(f2_array(INTSXP, G, nb));
  vals[2] = PROTECT(f2_array(REALSXP, G, nb));
  vals[3] = PROTECT(f2_array(INTSXP, G, nb));
  vals[4] = PROTECT(Rf_allocVector(REALSXP, nb));
  static const char* names[5] = {"f2", "counts", "ap", "ap_counts", "block_lengths"};
  SEXP out = PROTECT(named_list(5, names, vals));
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_f2_blocks(ctx(), v, gid == R_NilValue ? NULL : INTEGER(gid), G, pl == R_NilValue ? NULL : REAL(pl), &P, b64,
                              b64 + nb, (int64_t)nb, REAL(vals[0]), (int32_t*)INTEGER(vals[1]), REAL(vals[2]),
                              (int32_t*)INTEGER(vals[3]), b64 + 2 * nb));
  for (R_xlen_t b = 0; b < nb; b++) REAL(vals[4])[b] = (double)b64[2 * nb + b];
  UNPROTECT(13);
  return out;
}

/* ---- admixture ---------------------------------------------------------------------------------------------------- */

#pragma weak tpg_admix_em
#pragma weak tpg_admix_params_default

/* tpg_admixture(BM, rowInd, colInd, k, seed, max_iter, tol, q0, p0): the PLINK export, the outside `admixture` run and the
 * reading back of its .Q / .P files (R/gt_admixture.R:86-236) as one call of the EM of include/tpg.h "admixture", for one k
 * and one run.  seed = a double vector of length 1 holding a whole number in [0, 2^53]; q0 (N x k) / p0 (M x k) = a start, or
 * NULL for the seeded one.  -> list(Q: N x k, P: M x k (frequency of the counted allele), loglik, n_iter, converged) */
static SEXP admixture_call(int squarem, SEXP BM, SEXP rowInd, SEXP colInd, SEXP k, SEXP seed, SEXP max_iter, SEXP tol, SEXP q0,
                           SEXP p0) {
  const int K = Rf_asInteger(k);
  if (K == NA_INTEGER || K < 1) Rf_error("tidypopgen (GPU): k must be a positive integer");
  if (TYPEOF(seed) != REALSXP || XLENGTH(seed) != 1) Rf_error("tidypopgen (GPU): seed must be a double vector of length 1");
  const double sd = REAL(seed)[0];
  if (!(sd >= 0 && sd <= 9007199254740992.0) || sd != floor(sd))
    Rf_error("tidypopgen (GPU): seed must be a whole number in [0, 2^53]");
  const int mi = Rf_asInteger(max_iter);
  if (mi == NA_INTEGER || mi < 0) Rf_error("tidypopgen (GPU): max_iter must be a non-negative integer");
  if ((TYPEOF(tol) != REALSXP && TYPEOF(tol) != INTSXP) || XLENGTH(tol) != 1) Rf_error("tidypopgen (GPU): tol must be one number");
  SEXP ts = PROTECT(as_real(tol));
  const double tl = REAL(ts)[0];
  UNPROTECT(1);
  if (!(tl >= 0)) Rf_error("tidypopgen (GPU): tol must be a non-negative number");
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  const R_xlen_t n = XLENGTH(ri), m = XLENGTH(ci);
  if (n > INT_MAX || m > INT_MAX) Rf_error("tidypopgen (GPU): too many rows or columns for an R matrix");
  SEXP qs = PROTECT(q0 == R_NilValue ? R_NilValue : Rf_coerceVector(q0, REALSXP));
  SEXP ps = PROTECT(p0 == R_NilValue ? R_NilValue : Rf_coerceVector(p0, REALSXP));
  if (qs != R_NilValue && XLENGTH(qs) != n * (R_xlen_t)K) Rf_error("tidypopgen (GPU): q0 must be length(rowInd) x k");
  if (ps != R_NilValue && XLENGTH(ps) != m * (R_xlen_t)K) Rf_error("tidypopgen (GPU): p0 must be length(colInd) x k");
  SEXP vals[7];
  vals[0] = PROTECT(Rf_allocMatrix(REALSXP, (int)n, K));
  vals[1] = PROTECT(Rf_allocMatrix(REALSXP, (int)m, K));
  vals[2] = PROTECT(Rf_allocVector(REALSXP, 1));
  vals[3] = PROTECT(Rf_allocVector(INTSXP, 1));
  vals[4] = PROTECT(Rf_allocVector(LGLSXP, 1));
  vals[5] = PROTECT(Rf_allocVector(INTSXP, 1));
  vals[6] = PROTECT(Rf_allocVector(INTSXP, 1));
  static const char* names[7] = {"Q", "P", "loglik", "n_iter", "converged", "n_cycles", "n_rejected"};
  SEXP out = PROTECT(named_list(squarem ? 7 : 5, names, vals));
  tpg_admix_params P;
  tpg_admix_params_default(&P);
  P.max_iter = mi;
  P.tol = tl;
  P.seed = (uint64_t)sd;
  int32_t nit = 0, conv = 0, ncyc = 0, nrej = 0;
  tpg_view* v = view_of(BM, ri, ci, 0);
  if (squarem)
    TPG_R_VIEW(v, tpg_admix_em_squarem(ctx(), v, NULL, K, &P, qs == R_NilValue ? NULL : REAL(qs), ps == R_NilValue ? NULL : REAL(ps),
                                       REAL(vals[0]), REAL(vals[1]), REAL(vals[2]), NULL, &nit, &conv, NULL, NULL, &ncyc, &nrej));
  else
    TPG_R_VIEW(v, tpg_admix_em(ctx(), v, NULL, K, &P, qs == R_NilValue ? NULL : REAL(qs), ps == R_NilValue ? NULL : REAL(ps),
                               REAL(vals[0]), REAL(vals[1]), REAL(vals[2]), NULL, &nit, &conv));
  INTEGER(vals[3])[0] = nit;
  LOGICAL(vals[4])[0] = conv != 0;
  INTEGER(vals[5])[0] = ncyc;
  INTEGER(vals[6])[0] = nrej;
  UNPROTECT(12);
  return out;
}

SEXP _tidypopgen_tpg_admixture(SEXP BM, SEXP rowInd, SEXP colInd, SEXP k, SEXP seed, SEXP max_iter, SEXP tol, SEXP q0, SEXP p0) {
  TPG_NEEDS(tpg_admix_em);
  return admixture_call(0, BM, rowInd, colInd, k, seed, max_iter, tol, q0, p0);
}

/* ---- admixture cross-validation ----------------------------------------------------------------------------------- */

#pragma weak tpg_admix_cv
#pragma weak tpg_admix_cv_error

/* tpg_admixture_cv(BM, rowInd, colInd, k, seed, max_iter, tol, q0, p0, folds, cv_seed): what crossval = TRUE adds to a run of
 * R/gt_admixture.R:184-196 (the outside binary's --cv and the "CV error" line of its log), as one call of tpg_admix_cv of
 * include/tpg.h "admixture cross-validation" for one k and one run.  The first nine arguments are those of tpg_admixture; folds =
 * an integer in [2, 64]; cv_seed follows the rule of seed.
 * -> list(cv_error, fold_deviance: folds, fold_count: folds (double), fold_n_iter: folds (integer), fold_converged: folds) */
static SEXP admixture_cv_call(int squarem, SEXP BM, SEXP rowInd, SEXP colInd, SEXP k, SEXP seed, SEXP max_iter, SEXP tol, SEXP q0,
                              SEXP p0, SEXP folds, SEXP cv_seed) {
  const int K = Rf_asInteger(k);
  if (K == NA_INTEGER || K < 1) Rf_error("tidypopgen (GPU): k must be a positive integer");
  if (TYPEOF(seed) != REALSXP || XLENGTH(seed) != 1) Rf_error("tidypopgen (GPU): seed must be a double vector of length 1");
  const double sd = REAL(seed)[0];
  if (!(sd >= 0 && sd <= 9007199254740992.0) || sd != floor(sd))
    Rf_error("tidypopgen (GPU): seed must be a whole number in [0, 2^53]");
  const int mi = Rf_asInteger(max_iter);
  if (mi == NA_INTEGER || mi < 0) Rf_error("tidypopgen (GPU): max_iter must be a non-negative integer");
  if ((TYPEOF(tol) != REALSXP && TYPEOF(tol) != INTSXP) || XLENGTH(tol) != 1) Rf_error("tidypopgen (GPU): tol must be one number");
  SEXP ts = PROTECT(as_real(tol));
  const double tl = REAL(ts)[0];
  UNPROTECT(1);
  if (!(tl >= 0)) Rf_error("tidypopgen (GPU): tol must be a non-negative number");
  const int nf = Rf_asInteger(folds);
  if (nf == NA_INTEGER || nf < 2 || nf > TPG_ADMIX_MAX_FOLDS) Rf_error("tidypopgen (GPU): folds must be an integer in [2, 64]");
  if (TYPEOF(cv_seed) != REALSXP || XLENGTH(cv_seed) != 1) Rf_error("tidypopgen (GPU): cv_seed must be a double vector of length 1");
  const double cs = REAL(cv_seed)[0];
  if (!(cs >= 0 && cs <= 9007199254740992.0) || cs != floor(cs))
    Rf_error("tidypopgen (GPU): cv_seed must be a whole number in [0, 2^53]");
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  const R_xlen_t n = XLENGTH(ri), m = XLENGTH(ci);
  SEXP qs = PROTECT(q0 == R_NilValue ? R_NilValue : Rf_coerceVector(q0, REALSXP));
  SEXP ps = PROTECT(p0 == R_NilValue ? R_NilValue : Rf_coerceVector(p0, REALSXP));
  if (qs != R_NilValue && XLENGTH(qs) != n * (R_xlen_t)K) Rf_error("tidypopgen (GPU): q0 must be length(rowInd) x k");
  if (ps != R_NilValue && XLENGTH(ps) != m * (R_xlen_t)K) Rf_error("tidypopgen (GPU): p0 must be length(colInd) x k");
  SEXP vals[5];
  vals[0] = PROTECT(Rf_allocVector(REALSXP, 1));
  vals[1] = PROTECT(Rf_allocVector(REALSXP, nf));
  vals[2] = PROTECT(Rf_allocVector(REALSXP, nf));
  vals[3] = PROTECT(Rf_allocVector(INTSXP, nf));
  vals[4] = PROTECT(Rf_allocVector(LGLSXP, nf));
  static const char* names[5] = {"cv_error", "fold_deviance", "fold_count", "fold_n_iter", "fold_converged"};
  SEXP out = PROTECT(named_list(5, names, vals));
  tpg_admix_params P;
  tpg_admix_params_default(&P);
  P.max_iter = mi;
  P.tol = tl;
  P.seed = (uint64_t)sd;
  double ll[TPG_ADMIX_MAX_FOLDS], cv = 0;
  int64_t cnt[TPG_ADMIX_MAX_FOLDS], het[TPG_ADMIX_MAX_FOLDS];
  int32_t nit[TPG_ADMIX_MAX_FOLDS], conv[TPG_ADMIX_MAX_FOLDS];
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, (squarem ? tpg_admix_cv_squarem : tpg_admix_cv)(ctx(), v, NULL, K, &P, nf, (uint64_t)cs,
                                                                qs == R_NilValue ? NULL : REAL(qs),
                                                                ps == R_NilValue ? NULL : REAL(ps), &cv, ll, cnt, het, nit, conv));
  TPG_R(tpg_admix_cv_error(nf, ll, cnt, het, REAL(vals[1]), &cv));
  REAL(vals[0])[0] = cv;
  for (int f = 0; f < nf; f++) {
    REAL(vals[2])[f] = (double)cnt[f];
    INTEGER(vals[3])[f] = nit[f];
    LOGICAL(vals[4])[f] = conv[f] != 0;
  }
  UNPROTECT(10);
  return out;
}

SEXP _tidypopgen_tpg_admixture_cv(SEXP BM, SEXP rowInd, SEXP colInd, SEXP k, SEXP seed, SEXP max_iter, SEXP tol, SEXP q0, SEXP p0,
                                  SEXP folds, SEXP cv_seed) {
  TPG_NEEDS(tpg_admix_cv);
  TPG_NEEDS(tpg_admix_cv_error);
  return admixture_cv_call(0, BM, rowInd, colInd, k, seed, max_iter, tol, q0, p0, folds, cv_seed);
}

/* ---- admixture, accelerated ---------------------------------------------------------------------------------------- */

#pragma weak tpg_admix_em_squarem
#pragma weak tpg_admix_cv_squarem

/* tpg_admixture_squarem(BM, rowInd, colInd, k, seed, max_iter, tol, q0, p0): tpg_admixture with the EM under squared extrapolation
 * (tpg_admix_em_squarem of include/tpg.h "admixture, accelerated").  The same arguments and checks.
 * -> list(Q, P, loglik, n_iter (EM steps), converged, n_cycles, n_rejected) */
SEXP _tidypopgen_tpg_admixture_squarem(SEXP BM, SEXP rowInd, SEXP colInd, SEXP k, SEXP seed, SEXP max_iter, SEXP tol, SEXP q0,
                                       SEXP p0) {
  TPG_NEEDS(tpg_admix_em_squarem);
  return admixture_call(1, BM, rowInd, colInd, k, seed, max_iter, tol, q0, p0);
}

/* tpg_admixture_cv_squarem(BM, rowInd, colInd, k, seed, max_iter, tol, q0, p0, folds, cv_seed): tpg_admixture_cv with every fold
 * refitted by the accelerated driver (tpg_admix_cv_squarem).  The same arguments, checks and result list. */
SEXP _tidypopgen_tpg_admixture_cv_squarem(SEXP BM, SEXP rowInd, SEXP colInd, SEXP k, SEXP seed, SEXP max_iter, SEXP tol, SEXP q0,
                                          SEXP p0, SEXP folds, SEXP cv_seed) {
  TPG_NEEDS(tpg_admix_cv_squarem);
  TPG_NEEDS(tpg_admix_cv_error);
  return admixture_cv_call(1, BM, rowInd, colInd, k, seed, max_iter, tol, q0, p0, folds, cv_seed);
}

/* ---- pcadapt ------------------------------------------------------------------------------------------------------ */

#pragma weak tpg_pcadapt

/* tpg_pcadapt(BM, rowInd, colInd, U): the genome scan of R/gt_pcadapt.R:44-86 (bigsnpr::snp_pcadapt) as one call of the scan of
 * include/tpg.h "pcadapt".  U = the first K columns of the PCA's u (length(rowInd) x K, numeric; K is read from its length).
 * -> list(score: M (= dist / gc_lambda), dist: M, log10p: M, gc_lambda) */
SEXP _tidypopgen_tpg_pcadapt(SEXP BM, SEXP rowInd, SEXP colInd, SEXP U) {
  TPG_NEEDS(tpg_pcadapt);
  if (TYPEOF(U) != REALSXP && TYPEOF(U) != INTSXP) Rf_error("tidypopgen (GPU): U must be a numeric matrix");
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  const R_xlen_t n = XLENGTH(ri), m = XLENGTH(ci);
  SEXP us = PROTECT(as_real(U));
  if (n < 1 || XLENGTH(us) < n || XLENGTH(us) % n != 0) Rf_error("tidypopgen (GPU): U must have length(rowInd) rows");
  const R_xlen_t K = XLENGTH(us) / n;
  if (K > INT_MAX) Rf_error("tidypopgen (GPU): too many columns in U");
  SEXP vals[4];
  vals[0] = PROTECT(Rf_allocVector(REALSXP, m));
  vals[1] = PROTECT(Rf_allocVector(REALSXP, m));
  vals[2] = PROTECT(Rf_allocVector(REALSXP, m));
  vals[3] = PROTECT(Rf_allocVector(REALSXP, 1));
  static const char* names[4] = {"score", "dist", "log10p", "gc_lambda"};
  SEXP out = PROTECT(named_list(4, names, vals));
  tpg_view* v = view_of(BM, ri, ci, 0);
  TPG_R_VIEW(v, tpg_pcadapt(ctx(), v, REAL(us), (int)K, NULL, REAL(vals[1]), REAL(vals[0]), REAL(vals[2]), REAL(vals[3]), NULL));
  UNPROTECT(8);
  return out;
}

/* ---- sNMF ---------------------------------------------------------------------------------------------------------- */

#pragma weak tpg_snmf
#pragma weak tpg_view_holdout_fraction
#pragma weak tpg_snmf_cross_entropy_sums

/* tpg_snmf(BM, rowInd, colInd, k, alpha, tolerance, iterations, seed, percentage, q0): the .geno export and the LEA::snmf run of
 * R/gt_snmf.R as one call of the sNMF of include/tpg.h "sNMF", for one k and one run.  seed = a double vector of length 1 holding
 * a whole number in [0, 2^53]; percentage = NULL (no cross-entropy) or one number in (0, 1): that share of the typed genotypes is
 * held out (the mask is keyed by seed), the fit runs on the rest, as LEA's does, and cv / cv_all are the masked / all
 * cross-entropies; q0 (N x k) = a start, or NULL for the seeded one.
 * -> list(Q: N x k, P: M x k (frequency of the counted allele), G: 3M x k (row 3 j + c), ls, n_iter, converged, cv, cv_all);
 * cv and cv_all are NA_real_ without percentage */
SEXP _tidypopgen_tpg_snmf(SEXP BM, SEXP rowInd, SEXP colInd, SEXP k, SEXP alpha, SEXP tolerance, SEXP iterations, SEXP seed,
                          SEXP percentage, SEXP q0) {
  TPG_NEEDS(tpg_snmf);
  TPG_NEEDS(tpg_view_holdout_fraction);
  TPG_NEEDS(tpg_snmf_cross_entropy_sums);
  const int K = Rf_asInteger(k);
  if (K == NA_INTEGER || K < 1) Rf_error("tidypopgen (GPU): k must be a positive integer");
  if ((TYPEOF(alpha) != REALSXP && TYPEOF(alpha) != INTSXP) || XLENGTH(alpha) != 1) Rf_error("tidypopgen (GPU): alpha must be one number");
  if ((TYPEOF(tolerance) != REALSXP && TYPEOF(tolerance) != INTSXP) || XLENGTH(tolerance) != 1)
    Rf_error("tidypopgen (GPU): tolerance must be one number");
  SEXP as = PROTECT(as_real(alpha)), ts = PROTECT(as_real(tolerance));
  const double al = REAL(as)[0], tl = REAL(ts)[0];
  UNPROTECT(2);
  if (!(al >= 0 && al <= DBL_MAX)) Rf_error("tidypopgen (GPU): alpha must be a finite non-negative number");
  if (!(tl >= 0)) Rf_error("tidypopgen (GPU): tolerance must be a non-negative number");
  const int mi = Rf_asInteger(iterations);
  if (mi == NA_INTEGER || mi < 0) Rf_error("tidypopgen (GPU): iterations must be a non-negative integer");
  if (TYPEOF(seed) != REALSXP || XLENGTH(seed) != 1) Rf_error("tidypopgen (GPU): seed must be a double vector of length 1");
  const double sd = REAL(seed)[0];
  if (!(sd >= 0 && sd <= 9007199254740992.0) || sd != floor(sd))
    Rf_error("tidypopgen (GPU): seed must be a whole number in [0, 2^53]");
  double pct = 0;
  if (percentage != R_NilValue) {
    if ((TYPEOF(percentage) != REALSXP && TYPEOF(percentage) != INTSXP) || XLENGTH(percentage) != 1)
      Rf_error("tidypopgen (GPU): percentage must be NULL or one number");
    SEXP ps = PROTECT(as_real(percentage));
    pct = REAL(ps)[0];
    UNPROTECT(1);
    if (!(pct > 0 && pct < 1)) Rf_error("tidypopgen (GPU): percentage must lie strictly between 0 and 1");
  }
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  const R_xlen_t n = XLENGTH(ri), m = XLENGTH(ci);
  if (n > INT_MAX || m > INT_MAX / 3) Rf_error("tidypopgen (GPU): too many rows or columns for an R matrix");
  SEXP qs = PROTECT(q0 == R_NilValue ? R_NilValue : Rf_coerceVector(q0, REALSXP));
  if (qs != R_NilValue && XLENGTH(qs) != n * (R_xlen_t)K) Rf_error("tidypopgen (GPU): q0 must be length(rowInd) x k");
  SEXP vals[8];
  vals[0] = PROTECT(Rf_allocMatrix(REALSXP, (int)n, K));
  vals[1] = PROTECT(Rf_allocMatrix(REALSXP, (int)m, K));
  vals[2] = PROTECT(Rf_allocMatrix(REALSXP, (int)(3 * m), K));
  vals[3] = PROTECT(Rf_allocVector(REALSXP, 1));
  vals[4] = PROTECT(Rf_allocVector(INTSXP, 1));
  vals[5] = PROTECT(Rf_allocVector(LGLSXP, 1));
  vals[6] = PROTECT(Rf_allocVector(REALSXP, 1));
  vals[7] = PROTECT(Rf_allocVector(REALSXP, 1));
  static const char* names[8] = {"Q", "P", "G", "ls", "n_iter", "converged", "cv", "cv_all"};
  SEXP out = PROTECT(named_list(8, names, vals));
  int nit = 0, conv = 0;
  double sm = 0, sa = 0;
  int64_t nm = 0, na = 0;
  tpg_view* v = view_of(BM, ri, ci, 0);
  tpg_view* train = NULL;
  int rc = TPG_OK;
  if (pct > 0) rc = tpg_view_holdout_fraction(ctx(), v, pct, (uint64_t)sd, &train, NULL);
  if (rc == TPG_OK)
    rc = tpg_snmf(ctx(), train ? train : v, NULL, K, mi, tl, al, (uint64_t)sd, qs == R_NilValue ? NULL : REAL(qs), REAL(vals[0]),
                  REAL(vals[2]), REAL(vals[1]), REAL(vals[3]), NULL, &nit, &conv, NULL);
  if (rc == TPG_OK && train) rc = tpg_snmf_cross_entropy_sums(ctx(), v, train, K, REAL(vals[0]), REAL(vals[2]), &sm, &nm, &sa, &na);
  if (train) tpg_view_free(train);
  TPG_R_VIEW(v, rc);
  INTEGER(vals[4])[0] = nit;
  LOGICAL(vals[5])[0] = conv != 0;
  REAL(vals[6])[0] = train && nm > 0 ? sm / (double)nm : NA_REAL;
  REAL(vals[7])[0] = train && na > 0 ? sa / (double)na : NA_REAL;
  UNPROTECT(12);
  return out;
}

/* ---- clusters on PCA scores ------------------------------------------------------------------------------------------ */

#pragma weak tpg_kmeans_batch

static uint64_t mix64(uint64_t x) { /* tpg_mix64 of include/tpg.h "simple imputation" */
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

/* tpg_cluster_pca(scores, k, n_start, n_iter, seed): the loop over k of R/gt_cluster_pca.R:137-155 (stats::kmeans with nstart and
 * compute_wss) as ONE call of the batched k-means of include/tpg.h "k-means on PCA scores".  scores = the n x n_pca numeric matrix
 * of PCA scores; k = the numbers of clusters to try (whole numbers in [1, n]); n_start, n_iter positive integers; seed = a double
 * vector of length 1 holding a whole number in [0, 2^53].  Every k > 1 gets n_start runs from the seeds M(seed ^ M((k << 32) + t)),
 * k = 1 one run; per k the run of smallest WSS is returned, on a tie the smaller t.
 * -> list(groups: n x length(k) integer, 1-based, WSS: length(k), n_iter, converged, n_empty: of the run returned) */
SEXP _tidypopgen_tpg_cluster_pca(SEXP scores, SEXP k, SEXP n_start, SEXP n_iter, SEXP seed) {
  TPG_NEEDS(tpg_kmeans_batch);
  SEXP dim = Rf_getAttrib(scores, R_DimSymbol);
  if ((TYPEOF(scores) != REALSXP && TYPEOF(scores) != INTSXP) || Rf_length(dim) != 2)
    Rf_error("tidypopgen (GPU): scores must be a numeric matrix");
  const int n = INTEGER(dim)[0], d = INTEGER(dim)[1];
  if (n < 1 || d < 1) Rf_error("tidypopgen (GPU): scores must have at least one row and one column");
  if ((TYPEOF(k) != REALSXP && TYPEOF(k) != INTSXP) || XLENGTH(k) < 1 || XLENGTH(k) > INT_MAX)
    Rf_error("tidypopgen (GPU): k must be a vector of whole numbers");
  const int ns = Rf_asInteger(n_start), mi = Rf_asInteger(n_iter);
  if (ns == NA_INTEGER || ns < 1) Rf_error("tidypopgen (GPU): n_start must be a positive integer");
  if (mi == NA_INTEGER || mi < 1) Rf_error("tidypopgen (GPU): n_iter must be a positive integer");
  if (TYPEOF(seed) != REALSXP || XLENGTH(seed) != 1) Rf_error("tidypopgen (GPU): seed must be a double vector of length 1");
  const double sd = REAL(seed)[0];
  if (!(sd >= 0 && sd <= 9007199254740992.0) || sd != floor(sd))
    Rf_error("tidypopgen (GPU): seed must be a whole number in [0, 2^53]");
  SEXP xs = PROTECT(as_real(scores)), kr = PROTECT(as_real(k));
  const int nk = (int)XLENGTH(kr);
  int64_t R = 0;
  for (int a = 0; a < nk; a++) {
    const double kk = REAL(kr)[a];
    if (!(kk >= 1 && kk <= n) || kk != floor(kk)) Rf_error("tidypopgen (GPU): every k must be a whole number in [1, nrow(scores)]");
    R += kk == 1 ? 1 : ns;
  }
  if (R > TPG_KMEANS_MAX_RUNS) Rf_error("tidypopgen (GPU): %lld runs in one call, at most %d", (long long)R, TPG_KMEANS_MAX_RUNS);
  SEXP vals[5];
  vals[0] = PROTECT(Rf_allocMatrix(INTSXP, n, nk));
  vals[1] = PROTECT(Rf_allocVector(REALSXP, nk));
  vals[2] = PROTECT(Rf_allocVector(INTSXP, nk));
  vals[3] = PROTECT(Rf_allocVector(LGLSXP, nk));
  vals[4] = PROTECT(Rf_allocVector(INTSXP, nk));
  static const char* names[5] = {"groups", "WSS", "n_iter", "converged", "n_empty"};
  SEXP out = PROTECT(named_list(5, names, vals));
  /* R's transient storage: freed when .Call returns or errors */
  int32_t* rk = (int32_t*)R_alloc((size_t)R, sizeof(int32_t));
  int64_t* rs = (int64_t*)R_alloc((size_t)R, sizeof(int64_t));
  int32_t* lab = (int32_t*)R_alloc((size_t)R * (size_t)n, sizeof(int32_t));
  double* wss = (double*)R_alloc((size_t)R, sizeof(double));
  int32_t* st = (int32_t*)R_alloc((size_t)3 * (size_t)R, sizeof(int32_t));
  int64_t r = 0;
  for (int a = 0; a < nk; a++) {
    const uint64_t kk = (uint64_t)REAL(kr)[a];
    for (int t = 0; t < (kk == 1 ? 1 : ns); t++, r++) {
      rk[r] = (int32_t)kk;
      rs[r] = (int64_t)mix64((uint64_t)sd ^ mix64((kk << 32) + (uint64_t)t));
    }
  }
  TPG_R(tpg_kmeans_batch(ctx(), REAL(xs), n, d, (int)R, rk, rs, mi, NULL, lab, NULL, wss, st, st + R, st + 2 * R));
  r = 0;
  for (int a = 0; a < nk; a++) {
    const int cnt = rk[r] == 1 ? 1 : ns;
    int64_t best = r;
    for (int t = 1; t < cnt; t++)
      if (wss[r + t] < wss[best]) best = r + t;
    for (int i = 0; i < n; i++) INTEGER(vals[0])[(size_t)a * (size_t)n + (size_t)i] = lab[(size_t)best * (size_t)n + (size_t)i] + 1;
    REAL(vals[1])[a] = wss[best];
    INTEGER(vals[2])[a] = st[best];
    LOGICAL(vals[3])[a] = st[R + best] != 0;
    INTEGER(vals[4])[a] = st[2 * R + best];
    r += cnt;
  }
  UNPROTECT(8);
  return out;
}

/* ---- Ward clustering on PCA scores ----------------------------------------------------------------------------------- */

#pragma weak tpg_hclust_ward
#pragma weak tpg_hclust_cut
#pragma weak tpg_hclust_r_merge
#pragma weak tpg_cluster_wss

/* tpg_cluster_pca_ward(scores, k, power): the loop over k of R/gt_cluster_pca.R:156-166 (hclust(dist(x)^2, "ward.D2") and cutree
 * per k, then compute_wss) as ONE tree of include/tpg.h "Ward clustering on PCA scores", cut at every k, and one tpg_cluster_wss
 * call.  scores = the n x n_pca numeric matrix of PCA scores; k = the numbers of clusters (whole numbers in [1, n]); power = 2
 * (the reference: the recurrence on d^4) or 1 (Ward's criterion, on d^2).  Every k is at most TPG_KMEANS_MAX_K = 1024, the
 * limit of tpg_cluster_wss, and is checked before the tree is built.
 * -> list(groups: n x length(k) integer, 1-based, WSS: length(k), merge: (n - 1) x 2 integer as hclust$merge, height: n - 1,
 * the root of S as hclust$height) */
SEXP _tidypopgen_tpg_cluster_pca_ward(SEXP scores, SEXP k, SEXP power) {
  TPG_NEEDS(tpg_hclust_ward);
  TPG_NEEDS(tpg_hclust_cut);
  TPG_NEEDS(tpg_hclust_r_merge);
  TPG_NEEDS(tpg_cluster_wss);
  SEXP dim = Rf_getAttrib(scores, R_DimSymbol);
  if ((TYPEOF(scores) != REALSXP && TYPEOF(scores) != INTSXP) || Rf_length(dim) != 2)
    Rf_error("tidypopgen (GPU): scores must be a numeric matrix");
  const int n = INTEGER(dim)[0], d = INTEGER(dim)[1];
  if (n < 1 || d < 1) Rf_error("tidypopgen (GPU): scores must have at least one row and one column");
  if ((TYPEOF(k) != REALSXP && TYPEOF(k) != INTSXP) || XLENGTH(k) < 1) Rf_error("tidypopgen (GPU): k must be a vector of whole numbers");
  if (XLENGTH(k) > TPG_KMEANS_MAX_RUNS) Rf_error("tidypopgen (GPU): k holds more than %d values", TPG_KMEANS_MAX_RUNS);
  if ((TYPEOF(power) != REALSXP && TYPEOF(power) != INTSXP) || XLENGTH(power) != 1) Rf_error("tidypopgen (GPU): power must be 1 or 2");
  const int pw = Rf_asInteger(power);
  if (pw != 1 && pw != 2) Rf_error("tidypopgen (GPU): power must be 1 or 2");
  SEXP xs = PROTECT(as_real(scores)), kr = PROTECT(as_real(k));
  const int nk = (int)XLENGTH(kr);
  for (int a = 0; a < nk; a++) {
    const double kk = REAL(kr)[a];
    if (!(kk >= 1 && kk <= n) || kk != floor(kk)) Rf_error("tidypopgen (GPU): every k must be a whole number in [1, nrow(scores)]");
    /* tpg_cluster_wss would refuse it: say so before the tree is built */
    if (kk > TPG_KMEANS_MAX_K) Rf_error("tidypopgen (GPU): k = %.0f is above %d, the largest k the WSS is summed for", kk, TPG_KMEANS_MAX_K);
  }
  SEXP vals[4];
  vals[0] = PROTECT(Rf_allocMatrix(INTSXP, n, nk));
  vals[1] = PROTECT(Rf_allocVector(REALSXP, nk));
  vals[2] = PROTECT(Rf_allocMatrix(INTSXP, n - 1, 2));
  vals[3] = PROTECT(Rf_allocVector(REALSXP, n - 1));
  static const char* names[4] = {"groups", "WSS", "merge", "height"};
  SEXP out = PROTECT(named_list(4, names, vals));
  /* R's transient storage: freed when .Call returns or errors */
  int32_t* ki = (int32_t*)R_alloc((size_t)nk, sizeof(int32_t));
  int32_t* mab = (int32_t*)R_alloc((size_t)2 * (size_t)n, sizeof(int32_t));
  int32_t* lab = (int32_t*)R_alloc((size_t)nk * (size_t)n, sizeof(int32_t));
  for (int a = 0; a < nk; a++) ki[a] = (int32_t)REAL(kr)[a];
  TPG_R(tpg_hclust_ward(ctx(), REAL(xs), n, d, pw, mab, mab + n, REAL(vals[3])));
  TPG_R(tpg_hclust_cut(n, mab, mab + n, nk, ki, lab));
  TPG_R(tpg_hclust_r_merge(n, mab, mab + n, INTEGER(vals[2])));
  TPG_R(tpg_cluster_wss(ctx(), REAL(xs), n, d, nk, ki, lab, REAL(vals[1]), NULL));
  for (size_t t = 0; t < (size_t)nk * (size_t)n; t++) INTEGER(vals[0])[t] = lab[t] + 1;
  for (int s = 0; s < n - 1; s++) REAL(vals[3])[s] = sqrt(REAL(vals[3])[s]);
  UNPROTECT(7);
  return out;
}

/* ---- autoSVD ------------------------------------------------------------------------------------------------------ */

#pragma weak tpg_pca_auto_svd
#pragma weak tpg_autosvd_count
#pragma weak tpg_autosvd_iters
#pragma weak tpg_autosvd_converged
#pragma weak tpg_autosvd_fetch
#pragma weak tpg_autosvd_history
#pragma weak tpg_autosvd_intervals
#pragma weak tpg_autosvd_free

/* tpg_pca_auto_svd(BM, rowInd, colInd, chrom, pos, hi, params): R/gt_pca_autoSVD.R (bigsnpr::snp_autoSVD) as one call of
 * include/tpg.h "autoSVD".  chrom = one integer code per locus of colInd; pos = its position, or NULL (no lrldr then); hi = the
 * clumping window (0-based last neighbour of every locus), or NULL to skip clumping; params = 7 numbers: k, thr_r2, roll_size,
 * int_min_size, alpha_tukey, min_mac, max_iter.
 * -> the big_SVD list(d, u, v, center, scale, n_iter, converged) with attr "subset" (positions in colInd of the kept loci,
 * 1-based) and attr "lrldr" = list(Chr, Start, Stop), one entry per run of at least int_min_size consecutive outliers */
static void* g_asv_pending = NULL; /* the result of a call whose R allocations are still to come (as g_roh_pending) */

static void asv_drop_pending(void) {
  if (g_asv_pending && tpg_autosvd_free) tpg_autosvd_free(g_asv_pending);
  g_asv_pending = NULL;
}

SEXP _tidypopgen_tpg_pca_auto_svd(SEXP BM, SEXP rowInd, SEXP colInd, SEXP chrom, SEXP pos, SEXP hi, SEXP params) {
  TPG_NEEDS(tpg_pca_auto_svd);
  asv_drop_pending();
  if ((TYPEOF(chrom) != INTSXP && TYPEOF(chrom) != REALSXP) || (TYPEOF(params) != INTSXP && TYPEOF(params) != REALSXP) ||
      (pos != R_NilValue && TYPEOF(pos) != INTSXP && TYPEOF(pos) != REALSXP) ||
      (hi != R_NilValue && TYPEOF(hi) != INTSXP && TYPEOF(hi) != REALSXP))
    Rf_error("tidypopgen (GPU): chrom, pos, hi and params must be integer or double vectors");
  SEXP ri = PROTECT(as_int(rowInd)), ci = PROTECT(as_int(colInd));
  SEXP ch = PROTECT(as_int(chrom)), pr = PROTECT(as_real(params));
  SEXP ps = PROTECT(pos == R_NilValue ? pos : as_real(pos)), hs = PROTECT(hi == R_NilValue ? hi : as_real(hi));
  const R_xlen_t n = XLENGTH(ri), m = XLENGTH(ci);
  if (XLENGTH(ch) != m || (ps != R_NilValue && XLENGTH(ps) != m) || (hs != R_NilValue && XLENGTH(hs) != m))
    Rf_error("tidypopgen (GPU): chrom / pos / hi and colInd differ in length");
  if (XLENGTH(pr) != 7) Rf_error("tidypopgen (GPU): params must be 7 numbers: k, thr_r2, roll_size, int_min_size, alpha_tukey, min_mac, max_iter");
  const double* q = REAL(pr);
  for (int k = 0; k < 7; k++)
    if (ISNAN(q[k])) Rf_error("tidypopgen (GPU): NA in params[%d]", k + 1);
  const double big = 2147483647.0;
  const int K = roh_int_param(q, 0, 1, big, "k"), roll = roh_int_param(q, 2, 0, big, "roll_size");
  const int min_size = roh_int_param(q, 3, 1, big, "int_min_size"), min_mac = roh_int_param(q, 5, 0, big, "min_mac");
  const int max_iter = roh_int_param(q, 6, 0, big, "max_iter");
  for (R_xlen_t j = 0; j < m; j++)
    if (INTEGER(ch)[j] == NA_INTEGER) Rf_error("tidypopgen (GPU): NA in chrom");
  int64_t* h64 = NULL;
  if (hs != R_NilValue) {
    h64 = (int64_t*)R_alloc((size_t)(m > 0 ? m : 1), sizeof(int64_t));
    for (R_xlen_t j = 0; j < m; j++) {
      if (!isfinite(REAL(hs)[j]) || fabs(REAL(hs)[j]) > big) Rf_error("tidypopgen (GPU): NA in hi");
      h64[j] = (int64_t)REAL(hs)[j];
    }
  }
  tpg_view* v = view_of(BM, ri, ci, 0);
  void* r = NULL;
  TPG_R_VIEW(v, tpg_pca_auto_svd(ctx(), v, INTEGER(ch), h64, K, q[1], roll, q[4], (int64_t)min_mac, max_iter, &r));
  g_asv_pending = r; /* from here to asv_drop_pending() every R allocation may raise an error */
  const int64_t c = tpg_autosvd_count(r);
  const int iters = tpg_autosvd_iters(r), conv = tpg_autosvd_converged(r), passes = conv ? iters : iters - 1;
  SEXP vals[7];
  static const char* names[7] = {"d", "u", "v", "center", "scale", "n_iter", "converged"};
  vals[0] = PROTECT(Rf_allocVector(REALSXP, K));
  vals[1] = PROTECT(Rf_allocMatrix(REALSXP, (int)n, K));
  vals[2] = PROTECT(Rf_allocMatrix(REALSXP, (int)c, K));
  vals[3] = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)c));
  vals[4] = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)c));
  vals[5] = PROTECT(Rf_allocVector(INTSXP, 1));
  vals[6] = PROTECT(Rf_allocVector(LGLSXP, 1));
  SEXP subset = PROTECT(Rf_allocVector(INTSXP, (R_xlen_t)c));
  int64_t* idx = (int64_t*)R_alloc((size_t)(c > 0 ? c : 1), sizeof(int64_t));
  /* the runs of every pass: counted first, so that every R vector exists before the result is let go */
  int64_t nrun = 0;
  for (int it = 0; it < passes; it++) {
    int64_t cnt = 0;
    if (tpg_autosvd_intervals(r, it, min_size, NULL, NULL, &cnt) != TPG_OK) Rf_error("tidypopgen (GPU): %s", tpg_last_error());
    nrun += cnt;
  }
  if (ps == R_NilValue) nrun = 0;
  SEXP lr[3];
  static const char* lr_names[3] = {"Chr", "Start", "Stop"};
  lr[0] = PROTECT(Rf_allocVector(INTSXP, (R_xlen_t)nrun));
  lr[1] = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)nrun));
  lr[2] = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)nrun));
  int64_t* ab = (int64_t*)R_alloc((size_t)(nrun > 0 ? 2 * nrun : 1), sizeof(int64_t));
  int rc = tpg_autosvd_fetch(r, REAL(vals[0]), REAL(vals[1]), REAL(vals[2]), REAL(vals[3]), REAL(vals[4]), idx, NULL);
  int64_t at = 0;
  for (int it = 0; rc == TPG_OK && nrun > 0 && it < passes; it++) {
    int64_t cnt = 0;
    rc = tpg_autosvd_intervals(r, it, min_size, ab + at, ab + nrun + at, &cnt);
    at += cnt;
  }
  asv_drop_pending();
  if (rc != TPG_OK) Rf_error("tidypopgen (GPU): %s", tpg_last_error());
  for (int64_t j = 0; j < c; j++) INTEGER(subset)[j] = (int)idx[j] + 1;
  for (int64_t k = 0; k < nrun; k++) {
    INTEGER(lr[0])[k] = INTEGER(ch)[ab[k]];
    REAL(lr[1])[k] = REAL(ps)[ab[k]];
    REAL(lr[2])[k] = REAL(ps)[ab[nrun + k]];
  }
  INTEGER(vals[5])[0] = iters;
  LOGICAL(vals[6])[0] = conv != 0;
  SEXP out = PROTECT(named_list(7, names, vals));
  SEXP lrl = PROTECT(named_list(3, lr_names, lr));
  Rf_setAttrib(out, Rf_install("subset"), subset);
  Rf_setAttrib(out, Rf_install("lrldr"), lrl);
  UNPROTECT(19);
  return out;
}

/* ---- registration ------------------------------------------------------------------------------------------------
 * Same names and arities as the reference's table (src/RcppExports.cpp:348-371).  These rows replace the rows of the
 * same name there, and so do the three HWE rows of tpg_rshim_entries_hwe[] below; the other rows of that table
 * (compute_np_mn, the VCF / packedancestry readers, write_to_FBM) keep pointing at the reference's own C++. */
const R_CallMethodDef tpg_rshim_entries[] = {
    {"_tidypopgen_alt_freq_dip_pseudo_cpp", (DL_FUNC)&_tidypopgen_alt_freq_dip_pseudo_cpp, 6},
    {"_tidypopgen_fbm256_prod_and_rowSumsSq", (DL_FUNC)&_tidypopgen_fbm256_prod_and_rowSumsSq, 6},
    {"_tidypopgen_grouped_alt_freq_dip_pseudo_cpp", (DL_FUNC)&_tidypopgen_grouped_alt_freq_dip_pseudo_cpp, 8},
    {"_tidypopgen_grouped_missingness_cpp", (DL_FUNC)&_tidypopgen_grouped_missingness_cpp, 6},
    {"_tidypopgen_grouped_summaries_dip_pseudo_cpp", (DL_FUNC)&_tidypopgen_grouped_summaries_dip_pseudo_cpp, 7},
    {"_tidypopgen_gt_grouped_pi_diploid", (DL_FUNC)&_tidypopgen_gt_grouped_pi_diploid, 6},
    {"_tidypopgen_gt_ind_hetero", (DL_FUNC)&_tidypopgen_gt_ind_hetero, 4},
    {"_tidypopgen_gt_pi_diploid", (DL_FUNC)&_tidypopgen_gt_pi_diploid, 4},
    {"_tidypopgen_pairwise_fst_hudson_loop", (DL_FUNC)&_tidypopgen_pairwise_fst_hudson_loop, 6},
    {"_tidypopgen_pairwise_fst_nei87_loop", (DL_FUNC)&_tidypopgen_pairwise_fst_nei87_loop, 7},
    {"_tidypopgen_pairwise_fst_wc84_loop", (DL_FUNC)&_tidypopgen_pairwise_fst_wc84_loop, 6},
    {"_tidypopgen_increment_as_counts", (DL_FUNC)&_tidypopgen_increment_as_counts, 7},
    {"_tidypopgen_increment_ibs_counts", (DL_FUNC)&_tidypopgen_increment_ibs_counts, 8},
    {"_tidypopgen_increment_king_numerator", (DL_FUNC)&_tidypopgen_increment_king_numerator, 9},
    /* additions (not in the reference): */
    {"_tidypopgen_tpg_flush", (DL_FUNC)&_tidypopgen_tpg_flush, 0},
    {"_tidypopgen_tpg_release", (DL_FUNC)&_tidypopgen_tpg_release, 0},
    {"_tidypopgen_tpg_invalidate", (DL_FUNC)&_tidypopgen_tpg_invalidate, 1},
    {"_tidypopgen_tpg_snp_pairwise", (DL_FUNC)&_tidypopgen_tpg_snp_pairwise, 5},
    {"_tidypopgen_tpg_grouped_alt_freq", (DL_FUNC)&_tidypopgen_tpg_grouped_alt_freq, 7},
    {"_tidypopgen_tpg_pairwise_pop_fst", (DL_FUNC)&_tidypopgen_tpg_pairwise_pop_fst, 10},
    {"_tidypopgen_tpg_pca_partial_svd", (DL_FUNC)&_tidypopgen_tpg_pca_partial_svd, 4},
    {NULL, NULL, 0}};

/* The entry points that WRITE to the genotype FBM, in a table of their own.  Everything in tpg_rshim_entries[] leaves the
 * caller's FBM as it found it (tests/test_gpu_rshim_entries.py runs every row of it on one shared backing file); a row here
 * rewrites the backing file.  Both tables are registered (R_init_tpgshim below; INTEGRATION.md section 2 for the in-package
 * route), so `.Call` finds these like the others. */
const R_CallMethodDef tpg_rshim_entries_write[] = {
    {"_tidypopgen_tpg_impute_simple", (DL_FUNC)&_tidypopgen_tpg_impute_simple, 3},
    {NULL, NULL, 0}};

/* The Hardy-Weinberg exact tests, in a table of their own: the three rows of the reference's table (src/RcppExports.cpp:358-360)
 * and the whole of loci_hwe's block loop in one call.  Registered with the other two tables. */
const R_CallMethodDef tpg_rshim_entries_hwe[] = {
    {"_tidypopgen_SNPHWE2_R", (DL_FUNC)&_tidypopgen_SNPHWE2_R, 4},
    {"_tidypopgen_hwe_on_matrix", (DL_FUNC)&_tidypopgen_hwe_on_matrix, 2},
    {"_tidypopgen_gt_grouped_hwe", (DL_FUNC)&_tidypopgen_gt_grouped_hwe, 6},
    {"_tidypopgen_tpg_loci_hwe", (DL_FUNC)&_tidypopgen_tpg_loci_hwe, 4},
    {NULL, NULL, 0}};

/* LD clumping, in a table of its own as well: the reference has no native row for it (its clumping is bigsnpr's). */
const R_CallMethodDef tpg_rshim_entries_ld[] = {
    {"_tidypopgen_tpg_ld_clump", (DL_FUNC)&_tidypopgen_tpg_ld_clump, 7},
    {NULL, NULL, 0}};

/* Runs of homozygosity, in a table of its own too: the reference's routine is R around detectRUNS, without a native row. */
const R_CallMethodDef tpg_rshim_entries_roh[] = {
    {"_tidypopgen_tpg_indiv_roh", (DL_FUNC)&_tidypopgen_tpg_indiv_roh, 6},
    {NULL, NULL, 0}};

/* Tajima's D, in a table of its own: the reference computes it in R on top of gt_grouped_pi_diploid, without a native row. */
const R_CallMethodDef tpg_rshim_entries_tajima[] = {
    {"_tidypopgen_tpg_pop_tajimas_d", (DL_FUNC)&_tidypopgen_tpg_pop_tajimas_d, 5},
    {"_tidypopgen_tpg_windows_pop_tajimas_d", (DL_FUNC)&_tidypopgen_tpg_windows_pop_tajimas_d, 9},
    {NULL, NULL, 0}};

/* Blocked f2, in a table of its own: the reference hands the allele-frequency table to admixtools, without a native row. */
const R_CallMethodDef tpg_rshim_entries_f2[] = {
    {"_tidypopgen_tpg_f2_blocks", (DL_FUNC)&_tidypopgen_tpg_f2_blocks, 9},
    {NULL, NULL, 0}};

/* Admixture, in a table of its own: the reference runs an outside program, without a native row. */
const R_CallMethodDef tpg_rshim_entries_admix[] = {
    {"_tidypopgen_tpg_admixture", (DL_FUNC)&_tidypopgen_tpg_admixture, 9},
    {NULL, NULL, 0}};

/* Admixture cross-validation, in a table of its own (tpg_rshim_entries_admix[] keeps its one row). */
const R_CallMethodDef tpg_rshim_entries_admix_cv[] = {
    {"_tidypopgen_tpg_admixture_cv", (DL_FUNC)&_tidypopgen_tpg_admixture_cv, 11},
    {NULL, NULL, 0}};

/* Accelerated admixture and its cross-validation, each in a table of its own (the two tables above keep their rows). */
const R_CallMethodDef tpg_rshim_entries_admix_squarem[] = {
    {"_tidypopgen_tpg_admixture_squarem", (DL_FUNC)&_tidypopgen_tpg_admixture_squarem, 9},
    {NULL, NULL, 0}};

const R_CallMethodDef tpg_rshim_entries_admix_cv_squarem[] = {
    {"_tidypopgen_tpg_admixture_cv_squarem", (DL_FUNC)&_tidypopgen_tpg_admixture_cv_squarem, 11},
    {NULL, NULL, 0}};

/* The pcadapt scan, in a table of its own: the reference's routine is bigsnpr's, without a native row. */
const R_CallMethodDef tpg_rshim_entries_pcadapt[] = {
    {"_tidypopgen_tpg_pcadapt", (DL_FUNC)&_tidypopgen_tpg_pcadapt, 4},
    {NULL, NULL, 0}};

/* autoSVD, in a table of its own: the reference's routine is bigsnpr's, without a native row. */
const R_CallMethodDef tpg_rshim_entries_autosvd[] = {
    {"_tidypopgen_tpg_pca_auto_svd", (DL_FUNC)&_tidypopgen_tpg_pca_auto_svd, 7},
    {NULL, NULL, 0}};

/* sNMF, in a table of its own: the reference hands a .geno file to LEA, without a native row. */
const R_CallMethodDef tpg_rshim_entries_snmf[] = {
    {"_tidypopgen_tpg_snmf", (DL_FUNC)&_tidypopgen_tpg_snmf, 10},
    {NULL, NULL, 0}};

/* Clusters on PCA scores, in a table of its own: the reference loops over stats::kmeans in R, without a native row. */
const R_CallMethodDef tpg_rshim_entries_cluster[] = {
    {"_tidypopgen_tpg_cluster_pca", (DL_FUNC)&_tidypopgen_tpg_cluster_pca, 5},
    {NULL, NULL, 0}};

/* Ward clustering on PCA scores, in a table of its own (tpg_rshim_entries_cluster[] keeps its one row). */
const R_CallMethodDef tpg_rshim_entries_hclust[] = {
    {"_tidypopgen_tpg_cluster_pca_ward", (DL_FUNC)&_tidypopgen_tpg_cluster_pca_ward, 3},
    {NULL, NULL, 0}};

/* Windowed pairwise Fst and PBS by the fused window scan, in a table of its own: the reference computes both in R on top of
 * pairwise_pop_fst and windows_stats_generic, without a native row. */
const R_CallMethodDef tpg_rshim_entries_winfst[] = {
    {"_tidypopgen_tpg_windows_pairwise_pop_fst", (DL_FUNC)&_tidypopgen_tpg_windows_pairwise_pop_fst, 10},
    {"_tidypopgen_tpg_windows_nwise_pop_pbs", (DL_FUNC)&_tidypopgen_tpg_windows_nwise_pop_pbs, 10},
    {NULL, NULL, 0}};

#ifdef TPG_RSHIM_STANDALONE
/* The shim as a package of its own (useDynLib(tpgshim, .registration = TRUE)): used to try the GPU path beside an
 * unmodified tidypopgen by assigning these functions over tidypopgen's internal wrappers. */
void R_init_tpgshim(DllInfo* dll) {
  /* R_registerRoutines takes ONE .Call table per DLL: the seventeen tables end to end (the array must outlive the call) */
  static R_CallMethodDef all[sizeof(tpg_rshim_entries) / sizeof(tpg_rshim_entries[0]) +
                             sizeof(tpg_rshim_entries_write) / sizeof(tpg_rshim_entries_write[0]) +
                             sizeof(tpg_rshim_entries_hwe) / sizeof(tpg_rshim_entries_hwe[0]) +
                             sizeof(tpg_rshim_entries_ld) / sizeof(tpg_rshim_entries_ld[0]) +
                             sizeof(tpg_rshim_entries_roh) / sizeof(tpg_rshim_entries_roh[0]) +
                             sizeof(tpg_rshim_entries_tajima) / sizeof(tpg_rshim_entries_tajima[0]) +
                             sizeof(tpg_rshim_entries_f2) / sizeof(tpg_rshim_entries_f2[0]) +
                             sizeof(tpg_rshim_entries_admix) / sizeof(tpg_rshim_entries_admix[0]) +
                             sizeof(tpg_rshim_entries_admix_cv) / sizeof(tpg_rshim_entries_admix_cv[0]) +
                             sizeof(tpg_rshim_entries_admix_squarem) / sizeof(tpg_rshim_entries_admix_squarem[0]) +
                             sizeof(tpg_rshim_entries_admix_cv_squarem) / sizeof(tpg_rshim_entries_admix_cv_squarem[0]) +
                             sizeof(tpg_rshim_entries_pcadapt) / sizeof(tpg_rshim_entries_pcadapt[0]) +
                             sizeof(tpg_rshim_entries_autosvd) / sizeof(tpg_rshim_entries_autosvd[0]) +
                             sizeof(tpg_rshim_entries_snmf) / sizeof(tpg_rshim_entries_snmf[0]) +
                             sizeof(tpg_rshim_entries_cluster) / sizeof(tpg_rshim_entries_cluster[0]) +
                             sizeof(tpg_rshim_entries_hclust) / sizeof(tpg_rshim_entries_hclust[0]) +
                             sizeof(tpg_rshim_entries_winfst) / sizeof(tpg_rshim_entries_winfst[0])];
  size_t k = 0;
  for (const R_CallMethodDef* e = tpg_rshim_entries; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_write; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_hwe; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_ld; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_roh; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_tajima; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_f2; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_admix; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_admix_cv; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_admix_squarem; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_admix_cv_squarem; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_pcadapt; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_autosvd; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_snmf; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_cluster; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_hclust; e->name; e++) all[k++] = *e;
  for (const R_CallMethodDef* e = tpg_rshim_entries_winfst; e->name; e++) all[k++] = *e;
  all[k].name = NULL;
  all[k].fun = NULL;
  all[k].numArgs = 0;
  R_registerRoutines(dll, NULL, all, NULL, NULL);
  R_useDynamicSymbols(dll, FALSE);
}
#endif

void R_unload_tpgshim(DllInfo* dll) {
  (void)dll;
  _tidypopgen_tpg_release();
  roh_drop_pending();
  asv_drop_pending();
  if (g_multi) {
    tpg_multi_destroy(g_multi);
    g_multi = NULL;
  }
  if (g_ctx) {
    tpg_ctx_destroy(g_ctx);
    g_ctx = NULL;
  }
}
