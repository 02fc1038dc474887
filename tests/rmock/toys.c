/* tests/rmock/toys.c -- test-only .Call functions that break one of R's rules each (and one that keeps them all): the
 * mock runtime must report every one of them, or a mock that accepts anything would leave the shim's tests green.
 * Checked by tests/test_rmock_strict.py. */
#include <R.h>
#include <Rinternals.h>

/* PROTECTs and forgets the UNPROTECT: R warns "stack imbalance" */
SEXP toy_forget_unprotect(SEXP x) {
  (void)x;
  SEXP a = PROTECT(Rf_allocVector(REALSXP, 1));
  REAL(a)[0] = 1;
  return a;
}

/* keeps an unprotected vector across another allocation: a collection in between frees it */
SEXP toy_unprotected_use(SEXP x) {
  (void)x;
  SEXP a = Rf_allocVector(REALSXP, 3);
  SEXP b = PROTECT(Rf_allocVector(REALSXP, 3));
  REAL(a)[0] = 1;
  REAL(b)[0] = 2;
  UNPROTECT(1);
  return b;
}

/* writes into its argument */
SEXP toy_write_arg(SEXP x) {
  REAL(x)[0] = 42;
  return R_NilValue;
}

/* as.integer(x) */
SEXP toy_coerce(SEXP x) { return Rf_coerceVector(x, INTSXP); }

/* list(a = x * 2, b = "b"): every rule kept */
SEXP toy_correct(SEXP x) {
  SEXP a = PROTECT(Rf_allocVector(REALSXP, XLENGTH(x)));
  for (R_xlen_t i = 0; i < XLENGTH(x); i++) REAL(a)[i] = 2 * REAL(x)[i];
  SEXP b = PROTECT(Rf_allocVector(STRSXP, 1));
  SET_STRING_ELT(b, 0, Rf_mkChar("b"));
  SEXP out = PROTECT(Rf_allocVector(VECSXP, 2));
  SET_VECTOR_ELT(out, 0, a);
  SET_VECTOR_ELT(out, 1, b);
  SEXP nm = PROTECT(Rf_allocVector(STRSXP, 2));
  SET_STRING_ELT(nm, 0, Rf_mkChar("a"));
  SET_STRING_ELT(nm, 1, Rf_mkChar("b"));
  Rf_setAttrib(out, R_NamesSymbol, nm);
  UNPROTECT(4);
  return out;
}

/* an R error after two PROTECTs: R's longjmp unwinds the protect stack */
SEXP toy_error_after_protect(SEXP x) {
  (void)x;
  PROTECT(Rf_allocVector(REALSXP, 1));
  PROTECT(Rf_allocVector(REALSXP, 1));
  Rf_error("toy error");
}
