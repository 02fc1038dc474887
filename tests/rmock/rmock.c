/*
 * tests/rmock/rmock.c -- NOT R.  A minimal runtime behind tests/rmock/Rinternals.h, enough to DRIVE shim/tpg_rshim.c
 * from a test the way R drives it: vectors with attributes, environments whose bindings Rf_eval(symbol, env) looks up
 * (how the shim reads the fields of a bigstatsr FBM reference-class object), Rf_error as a longjmp back into
 * rmock_call().  No promises, no active bindings.  Nothing is freed before rmock_reset.
 *
 * Where the shim depends on R's rules, the mock is as strict as R:
 *  - a counted protect stack: every call must leave it as deep as it found it ("stack imbalance"), and an R error
 *    unwinds it to its depth at entry, as R's longjmp does (always on; O(1) per PROTECT / UNPROTECT);
 *  - GC torture (opt-in, rmock_gctorture(1), after R's gctorture): at every allocation inside a call, each object that
 *    call allocated and that is neither protected, nor an argument, nor reachable from one of those through elements or
 *    attributes is marked dead and poisoned; any later accessor on it, or returning it, is "use of an unprotected object";
 *  - a failing allocation (opt-in, rmock_fail_alloc_at(k)): the k-th Rf_alloc* / Rf_coerceVector allocation of the next
 *    call raises Rf_error("cannot allocate vector ..."), as R does when memory runs out;
 *  - strict arguments (opt-in, rmock_strict(1)): the arguments' data and attributes are hashed before the call and
 *    compared after it ("modified its argument");
 *  - NA_REAL with R's bit pattern, NA_INTEGER, and R's coercion rules (NaN or out of range -> NA_INTEGER, otherwise
 *    truncation toward zero).
 * Test helpers (rmock_*) are what the tests call through ctypes.
 */
#define _POSIX_C_SOURCE 200809L
#include <limits.h>
#include <math.h>
#include <setjmp.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "R.h"
#include "R_ext/Rdynload.h"

struct rmock_sexprec {
  SEXPTYPE type;
  R_xlen_t len;
  void* data;                 /* double / int / SEXP array, char* for CHARSXP and SYMSXP */
  struct rmock_sexprec* attr_name[8];
  struct rmock_sexprec* attr_val[8];
  int nattr;
  struct rmock_sexprec* next; /* allocation list, newest first */
  uint64_t call;              /* the call that allocated it (0: outside any call -- never collected) */
  uint64_t mark;              /* GC torture: the mark pass that last reached it */
  int dead;                   /* GC torture: collected */
  int keep;                   /* symbols and R_alloc storage: never collected inside their call */
};

static struct rmock_sexprec nil_rec = {NILSXP, 0, NULL, {0}, {0}, 0, NULL, 0, 0, 0, 1},
                            unbound_rec = {SYMSXP, 0, (void*)"<unbound>", {0}, {0}, 0, NULL, 0, 0, 0, 1};
static struct rmock_sexprec names_rec = {SYMSXP, 0, (void*)"names", {0}, {0}, 0, NULL, 0, 0, 0, 1},
                            dim_rec = {SYMSXP, 0, (void*)"dim", {0}, {0}, 0, NULL, 0, 0, 0, 1},
                            dimnames_rec = {SYMSXP, 0, (void*)"dimnames", {0}, {0}, 0, NULL, 0, 0, 0, 1};
SEXP R_NilValue = &nil_rec, R_UnboundValue = &unbound_rec, R_NamesSymbol = &names_rec, R_DimSymbol = &dim_rec,
     R_DimNamesSymbol = &dimnames_rec;

/* R's NA_real_: a NaN whose low word is 1954 (arithmetic.c) */
static double na_real_of(void) {
  const uint64_t bits = 0x7FF00000000007A2ull;
  double d;
  memcpy(&d, &bits, sizeof d);
  return d;
}
double R_NaReal = 0;
__attribute__((constructor)) static void init_na_real(void) { R_NaReal = na_real_of(); }
int R_IsNA(double x) {
  if (!isnan(x)) return 0;
  uint64_t bits;
  memcpy(&bits, &x, sizeof bits);
  return (bits & 0xFFFFFFFFull) == 1954;
}

static SEXP g_all = NULL;
static jmp_buf g_jmp;
static int g_jmp_set = 0;
static char g_err[1024];

/* the protect stack */
#define RMOCK_PPSTACK 50000 /* R's default --max-ppsize */
static SEXP g_pp[RMOCK_PPSTACK];
static int g_ppdepth = 0;

/* the call in progress */
static uint64_t g_callno = 0, g_cur = 0; /* g_cur: number of the call in progress, 0 outside */
static SEXP* g_args = NULL;
static int g_nargs = 0;
static int g_torture = 0, g_strict = 0;
static long g_fail_at = 0, g_alloc_count = 0; /* failing allocation: armed for the next call */
static long g_fail_next = 0;
static uint64_t g_markno = 0;

static void live(SEXP x) {
  if (x && x->dead) Rf_error("use of an unprotected object (type %u, allocated in this call)", x->type);
}

static void gc_mark(SEXP x, int depth) {
  if (!x || x->mark == g_markno || depth > 64) return;
  x->mark = g_markno;
  if (x->type == STRSXP || x->type == VECSXP)
    for (R_xlen_t i = 0; i < x->len; i++) gc_mark(((SEXP*)x->data)[i], depth + 1);
  for (int k = 0; k < x->nattr; k++) gc_mark(x->attr_val[k], depth + 1);
}

static void poison(SEXP x) {
  size_t elt = x->type == REALSXP ? sizeof(double) : (x->type == INTSXP || x->type == LGLSXP) ? sizeof(int) : 0;
  if (elt && x->data) memset(x->data, 0xA5, elt * (size_t)x->len);
}

/* R's gctorture: a full collection before every allocation of the call in progress */
static void gc_torture(void) {
  if (!g_torture || !g_cur) return;
  g_markno++;
  for (int k = 0; k < g_ppdepth; k++) gc_mark(g_pp[k], 0);
  for (int k = 0; k < g_nargs; k++) gc_mark(g_args[k], 0);
  for (SEXP s = g_all; s && s->call == g_cur; s = s->next)
    if (!s->keep && !s->dead && s->mark != g_markno) {
      s->dead = 1;
      poison(s);
    }
}

static SEXP new_rec(SEXPTYPE type, R_xlen_t len, size_t elt) {
  gc_torture();
  SEXP s = (SEXP)calloc(1, sizeof(struct rmock_sexprec));
  if (!s) abort();
  s->type = type;
  s->len = len;
  s->data = len > 0 && elt ? calloc((size_t)len, elt) : NULL;
  s->call = g_cur;
  s->next = g_all;
  g_all = s;
  return s;
}

/* one allocation the shim asked R for: the one that fails under rmock_fail_alloc_at */
static void counted_alloc(SEXPTYPE type, R_xlen_t n) {
  if (g_cur && g_fail_at > 0 && ++g_alloc_count == g_fail_at)
    Rf_error("cannot allocate vector of type %u and length %lld (rmock_fail_alloc_at)", type, (long long)n);
}

void rmock_reset(void) {
  while (g_all) {
    SEXP n = g_all->next;
    free(g_all->data);
    free(g_all);
    g_all = n;
  }
  g_ppdepth = 0;
}

void Rf_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  if (g_jmp_set) longjmp(g_jmp, 1);
  fprintf(stderr, "Rf_error outside rmock_call: %s\n", g_err);
  abort();
}

/* R_alloc: transient storage R reclaims when .Call returns; here it lives until rmock_reset like every object */
char* R_alloc(size_t n, int size) {
  SEXP s = new_rec(CHARSXP, (R_xlen_t)(n ? n : 1), (size_t)size);
  s->keep = 1;
  return (char*)s->data;
}

int TYPEOF(SEXP x) { live(x); return (int)x->type; }
R_xlen_t XLENGTH(SEXP x) { live(x); return x->len; }
R_len_t Rf_length(SEXP x) { live(x); return (R_len_t)x->len; }
double* REAL(SEXP x) { live(x); if (x->type != REALSXP) Rf_error("REAL() on a non-double"); return (double*)x->data; }
int* INTEGER(SEXP x) { live(x); if (x->type != INTSXP && x->type != LGLSXP) Rf_error("INTEGER() on a non-integer"); return (int*)x->data; }
int* LOGICAL(SEXP x) { live(x); if (x->type != LGLSXP) Rf_error("LOGICAL() on a non-logical"); return (int*)x->data; }
SEXP STRING_ELT(SEXP x, R_xlen_t i) { live(x); if (x->type != STRSXP || i >= x->len) Rf_error("STRING_ELT"); return ((SEXP*)x->data)[i]; }
SEXP VECTOR_ELT(SEXP x, R_xlen_t i) { live(x); if (x->type != VECSXP || i >= x->len) Rf_error("VECTOR_ELT"); return ((SEXP*)x->data)[i]; }
void SET_STRING_ELT(SEXP x, R_xlen_t i, SEXP v) {
  live(x); live(v);
  if (x->type != STRSXP || i >= x->len || v->type != CHARSXP) Rf_error("SET_STRING_ELT");
  ((SEXP*)x->data)[i] = v;
}
SEXP SET_VECTOR_ELT(SEXP x, R_xlen_t i, SEXP v) {
  live(x); live(v);
  if (x->type != VECSXP || i >= x->len) Rf_error("SET_VECTOR_ELT");
  ((SEXP*)x->data)[i] = v;
  return v;
}
const char* CHAR(SEXP x) { live(x); return (const char*)x->data; }
const char* R_ExpandFileName(const char* s) { return s; }

static SEXP alloc_vector(SEXPTYPE type, R_xlen_t n) {
  switch (type) {
    case REALSXP: return new_rec(type, n, sizeof(double));
    case INTSXP: case LGLSXP: return new_rec(type, n, sizeof(int));
    case STRSXP: case VECSXP: { SEXP s = new_rec(type, n, sizeof(SEXP)); for (R_xlen_t i = 0; i < n; i++) ((SEXP*)s->data)[i] = R_NilValue; return s; }
    default: Rf_error("rmock: allocVector of type %u", type);
  }
}

SEXP Rf_allocVector(SEXPTYPE type, R_xlen_t n) {
  counted_alloc(type, n);
  return alloc_vector(type, n);
}

SEXP Rf_allocMatrix(SEXPTYPE type, int nrow, int ncol) {
  if (nrow < 0 || ncol < 0) Rf_error("negative extents to matrix");
  counted_alloc(type, (R_xlen_t)nrow * ncol);
  SEXP s = Rf_protect(alloc_vector(type, (R_xlen_t)nrow * ncol)); /* as R's allocMatrix: the dim vector allocates */
  SEXP d = alloc_vector(INTSXP, 2);
  ((int*)d->data)[0] = nrow;
  ((int*)d->data)[1] = ncol;
  Rf_setAttrib(s, R_DimSymbol, d);
  Rf_unprotect(1);
  return s;
}

SEXP Rf_mkChar(const char* str) {
  SEXP s = new_rec(CHARSXP, (R_xlen_t)strlen(str), 0);
  s->data = strdup(str);
  return s;
}

SEXP Rf_install(const char* name) {
  if (!strcmp(name, "names")) return R_NamesSymbol;
  if (!strcmp(name, "dim")) return R_DimSymbol;
  if (!strcmp(name, "dimnames")) return R_DimNamesSymbol;
  SEXP s = new_rec(SYMSXP, 0, 0);
  s->data = strdup(name);
  s->keep = 1; /* R never collects a symbol */
  return s;
}

static int same_sym(SEXP a, SEXP b) { return a == b || !strcmp((const char*)a->data, (const char*)b->data); }

SEXP Rf_setAttrib(SEXP x, SEXP name, SEXP val) {
  live(x); live(val);
  for (int k = 0; k < x->nattr; k++)
    if (same_sym(x->attr_name[k], name)) { x->attr_val[k] = val; return val; }
  if (x->nattr >= 8) Rf_error("rmock: too many attributes");
  x->attr_name[x->nattr] = name;
  x->attr_val[x->nattr++] = val;
  return val;
}

SEXP Rf_getAttrib(SEXP x, SEXP name) {
  live(x);
  for (int k = 0; k < x->nattr; k++)
    if (same_sym(x->attr_name[k], name)) return x->attr_val[k];
  return R_NilValue;
}

/* environments keep their bindings as attributes (name symbol -> value) */
SEXP Rf_eval(SEXP expr, SEXP env) {
  live(expr); live(env);
  if (expr->type != SYMSXP) return expr;
  if (env->type != ENVSXP) Rf_error("rmock: eval in a non-environment");
  for (int k = 0; k < env->nattr; k++)
    if (same_sym(env->attr_name[k], expr)) return env->attr_val[k];
  Rf_error("object '%s' not found", (const char*)expr->data);
}

/* R's coerceVector for the numeric types: NA stays NA; a double that is NaN or out of int range becomes NA_INTEGER
   (R warns "NAs introduced by coercion to integer range"); any other double is truncated toward zero */
static int real_to_int(double v) {
  if (isnan(v) || v >= 2147483648.0 || v <= -2147483649.0) return NA_INTEGER;
  const double t = trunc(v);
  return t == (double)INT_MIN ? NA_INTEGER : (int)t;
}

SEXP Rf_coerceVector(SEXP x, SEXPTYPE type) {
  live(x);
  if (x->type == type) return x;
  if (!((x->type == REALSXP || x->type == INTSXP || x->type == LGLSXP) && (type == REALSXP || type == INTSXP || type == LGLSXP)))
    Rf_error("rmock: coerceVector from type %u to type %u", x->type, type);
  counted_alloc(type, x->len);
  SEXP out = Rf_protect(alloc_vector(type, x->len));
  for (R_xlen_t i = 0; i < x->len; i++) {
    if (x->type == REALSXP) {
      const double v = ((double*)x->data)[i];
      if (type == INTSXP) ((int*)out->data)[i] = real_to_int(v);
      else ((int*)out->data)[i] = isnan(v) ? NA_LOGICAL : v != 0;
    } else {
      const int v = ((int*)x->data)[i];
      if (type == REALSXP) ((double*)out->data)[i] = v == NA_INTEGER ? NA_REAL : (double)v;
      else if (type == LGLSXP) ((int*)out->data)[i] = v == NA_INTEGER ? NA_LOGICAL : v != 0;
      else ((int*)out->data)[i] = v;
    }
  }
  for (int k = 0; k < x->nattr; k++) Rf_setAttrib(out, x->attr_name[k], x->attr_val[k]);
  Rf_unprotect(1);
  return out;
}

int Rf_asInteger(SEXP x) {
  live(x);
  if (x->len < 1) return NA_INTEGER;
  if (x->type == REALSXP) return real_to_int(((double*)x->data)[0]);
  if (x->type == INTSXP || x->type == LGLSXP) return ((int*)x->data)[0];
  return NA_INTEGER;
}

int Rf_asLogical(SEXP x) {
  live(x);
  if (x->len < 1) return NA_LOGICAL;
  if (x->type == LGLSXP) return ((int*)x->data)[0];
  if (x->type == INTSXP) { const int v = ((int*)x->data)[0]; return v == NA_INTEGER ? NA_LOGICAL : v != 0; }
  if (x->type == REALSXP) { const double v = ((double*)x->data)[0]; return isnan(v) ? NA_LOGICAL : v != 0; }
  return NA_LOGICAL;
}

SEXP Rf_protect(SEXP x) {
  if (g_ppdepth >= RMOCK_PPSTACK) Rf_error("protect(): protection stack overflow");
  live(x);
  g_pp[g_ppdepth++] = x;
  return x;
}
void Rf_unprotect(int n) {
  if (n < 0 || n > g_ppdepth) Rf_error("unprotect(): only %d protected items", g_ppdepth);
  g_ppdepth -= n;
}

int R_registerRoutines(DllInfo* info, const R_CMethodDef* const c, const R_CallMethodDef* const call, const R_FortranMethodDef* const f,
                       const R_ExternalMethodDef* const e) {
  (void)info; (void)c; (void)call; (void)f; (void)e;
  return 1;
}
Rboolean R_useDynamicSymbols(DllInfo* info, Rboolean value) { (void)info; return value; }

/* ---- strict arguments: a hash of an object's data and attributes --------------------------------------------------- */
static uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

static uint64_t hash_of(SEXP x, int depth) {
  uint64_t h = 1469598103934665603ull;
  if (!x || depth > 16) return h;
  h = fnv(h, &x->type, sizeof x->type);
  h = fnv(h, &x->len, sizeof x->len);
  switch (x->type) {
    case REALSXP: h = fnv(h, x->data, sizeof(double) * (size_t)x->len); break;
    case INTSXP: case LGLSXP: h = fnv(h, x->data, sizeof(int) * (size_t)x->len); break;
    case CHARSXP: case SYMSXP: if (x->data) h = fnv(h, x->data, strlen((const char*)x->data)); break;
    case STRSXP: case VECSXP:
      for (R_xlen_t i = 0; i < x->len; i++) { const uint64_t e = hash_of(((SEXP*)x->data)[i], depth + 1); h = fnv(h, &e, sizeof e); }
      break;
    default: break;
  }
  for (int k = 0; k < x->nattr; k++) {
    const uint64_t a = hash_of(x->attr_name[k], depth + 1), v = hash_of(x->attr_val[k], depth + 1);
    h = fnv(fnv(h, &a, sizeof a), &v, sizeof v);
  }
  return h;
}

/* ---- helpers for the tests ------------------------------------------------------------------------------------ */
SEXP rmock_new_env(void) { return new_rec(ENVSXP, 0, 0); }
void rmock_env_set(SEXP env, const char* name, SEXP val) { Rf_setAttrib(env, Rf_install(name), val); }
SEXP rmock_real(const double* v, R_xlen_t n) { SEXP s = alloc_vector(REALSXP, n); if (n) memcpy(s->data, v, sizeof(double) * (size_t)n); return s; }
SEXP rmock_int(const int* v, R_xlen_t n) { SEXP s = alloc_vector(INTSXP, n); if (n) memcpy(s->data, v, sizeof(int) * (size_t)n); return s; }
SEXP rmock_lgl(int v) { SEXP s = alloc_vector(LGLSXP, 1); ((int*)s->data)[0] = v; return s; }
SEXP rmock_str(const char* v) { SEXP s = alloc_vector(STRSXP, 1); ((SEXP*)s->data)[0] = Rf_mkChar(v); return s; }
SEXP rmock_real_matrix(const double* v, int nrow, int ncol) { SEXP s = Rf_allocMatrix(REALSXP, nrow, ncol); if (v) memcpy(s->data, v, sizeof(double) * (size_t)nrow * (size_t)ncol); return s; }
SEXP rmock_int_matrix(const int* v, int nrow, int ncol) { SEXP s = Rf_allocMatrix(INTSXP, nrow, ncol); if (v) memcpy(s->data, v, sizeof(int) * (size_t)nrow * (size_t)ncol); return s; }
SEXP rmock_nil(void) { return R_NilValue; }
void* rmock_data(SEXP x) { return x->data; }
const char* rmock_last_error(void) { return g_err; }
double rmock_na_real(void) { return na_real_of(); }
int rmock_protect_depth(void) { return g_ppdepth; }
void rmock_gctorture(int on) { g_torture = on; }
void rmock_strict(int on) { g_strict = on; }
void rmock_fail_alloc_at(long k) { g_fail_next = k; }
/* what the tests assert on the structure of a result */
SEXP rmock_names_symbol(void) { return R_NamesSymbol; }
SEXP rmock_dim_symbol(void) { return R_DimSymbol; }
SEXP rmock_dimnames_symbol(void) { return R_DimNamesSymbol; }
const char* rmock_string_elt(SEXP x, R_xlen_t i) { return (const char*)((SEXP*)x->data)[i]->data; }

/* call a .Call entry point with up to 10 arguments; NULL (and rmock_last_error) when it raised an R error or broke one of
   the rules above */
SEXP rmock_call_named(const char* name, DL_FUNC fn, int nargs, SEXP* a) {
  typedef SEXP (*F0)(void);
  typedef SEXP (*F1)(SEXP);
  typedef SEXP (*F2)(SEXP, SEXP);
  typedef SEXP (*F3)(SEXP, SEXP, SEXP);
  typedef SEXP (*F4)(SEXP, SEXP, SEXP, SEXP);
  typedef SEXP (*F5)(SEXP, SEXP, SEXP, SEXP, SEXP);
  typedef SEXP (*F6)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
  typedef SEXP (*F7)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
  typedef SEXP (*F8)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
  typedef SEXP (*F9)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
  typedef SEXP (*F10)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
  g_err[0] = 0;
  if (nargs < 0 || nargs > 10) {
    snprintf(g_err, sizeof(g_err), "rmock_call: %d arguments not supported", nargs);
    return NULL;
  }
  uint64_t before[10] = {0};
  if (g_strict)
    for (int k = 0; k < nargs; k++) before[k] = hash_of(a[k], 0);
  const int depth0 = g_ppdepth;
  g_cur = ++g_callno;
  g_args = a;
  g_nargs = nargs;
  g_fail_at = g_fail_next;
  g_fail_next = 0;
  g_alloc_count = 0;
  SEXP out = NULL;
  if (setjmp(g_jmp)) {
    g_jmp_set = 0;
    g_ppdepth = depth0; /* R's longjmp resets the protect stack */
    out = NULL;
    goto done;
  }
  g_jmp_set = 1;
  switch (nargs) {
    case 0: out = ((F0)fn)(); break;
    case 1: out = ((F1)fn)(a[0]); break;
    case 2: out = ((F2)fn)(a[0], a[1]); break;
    case 3: out = ((F3)fn)(a[0], a[1], a[2]); break;
    case 4: out = ((F4)fn)(a[0], a[1], a[2], a[3]); break;
    case 5: out = ((F5)fn)(a[0], a[1], a[2], a[3], a[4]); break;
    case 6: out = ((F6)fn)(a[0], a[1], a[2], a[3], a[4], a[5]); break;
    case 7: out = ((F7)fn)(a[0], a[1], a[2], a[3], a[4], a[5], a[6]); break;
    case 8: out = ((F8)fn)(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]); break;
    case 9: out = ((F9)fn)(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]); break;
    default: out = ((F10)fn)(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]); break;
  }
  g_jmp_set = 0;
  if (g_ppdepth != depth0) {
    snprintf(g_err, sizeof(g_err), "stack imbalance in '%s', %d then %d", name, depth0, g_ppdepth);
    g_ppdepth = depth0;
    out = NULL;
  } else if (out && out->dead) {
    snprintf(g_err, sizeof(g_err), "use of an unprotected object: '%s' returned one", name);
    out = NULL;
  }
done:
  if (g_strict)
    for (int k = 0; k < nargs; k++)
      if (hash_of(a[k], 0) != before[k]) {
        snprintf(g_err + strlen(g_err), sizeof(g_err) - strlen(g_err), "%s'%s' modified its argument %d", g_err[0] ? "; " : "",
                 name, k + 1);
        out = NULL;
      }
  g_cur = 0;
  g_args = NULL;
  g_nargs = 0;
  g_fail_at = 0;
  return out;
}

SEXP rmock_call(DL_FUNC fn, int nargs, SEXP* a) { return rmock_call_named(".Call", fn, nargs, a); }
