/* tests/rmock/call11.c -- NOT R.  rmock_call_named (rmock.c) drives a .Call entry point of up to 10 arguments.  An entry point of 11
 * goes through this trampoline: the test parks the function and its last argument here and hands rmock_call_named the
 * trampoline with the first ten, so the call runs under the same rules (protect depth, GC torture, strict arguments; the mock
 * only ever collects objects allocated during the call, so the parked argument is as safe as the ten it sees).  The test itself
 * checks that the eleventh argument comes back unmodified. */
#include <Rinternals.h>

typedef SEXP (*rmock_f11)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
static rmock_f11 g_fn11 = 0;
static SEXP g_arg11 = 0;

void rmock_call11_set(void* fn, SEXP last) {
  g_fn11 = (rmock_f11)fn;
  g_arg11 = last;
}

SEXP rmock_call11_trampoline(SEXP a0, SEXP a1, SEXP a2, SEXP a3, SEXP a4, SEXP a5, SEXP a6, SEXP a7, SEXP a8, SEXP a9) {
  return g_fn11(a0, a1, a2, a3, a4, a5, a6, a7, a8, a9, g_arg11);
}
