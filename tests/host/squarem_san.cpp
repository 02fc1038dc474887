// The host side of the accelerated admixture (tidypopgen_amd/csrc/host/host_squarem.h) as a stand-alone program for the host
// sanitizers (tests/test_admix_squarem_host.py).  No input: it drives squarem_alpha, squarem_accept, squarem_next_limit and
// squarem_drive over a toy map on one double per slot, x -> x / 2 with l(x) = -x^2 (for which one squared extrapolation lands
// on the fixed point 0), checks every case itself and prints one line per case, then "ok squarem".  The traces are heap arrays
// of exactly the sizes the header names, so that a write past them is caught.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "host/host_squarem.h"

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      return 1;                                                   \
    }                                                             \
  } while (0)

static const double NaN = std::numeric_limits<double>::quiet_NaN();
static const double Inf = std::numeric_limits<double>::infinity();

// x -> x / 2 on five slots; sr, sv as the device forms them; no projection.  nan_at: the cycle (0-based) whose l(theta') comes
// back NaN; worse_at: the cycle whose l(theta') comes back below l(theta1); fail_at: the step that answers an error code
struct Toy {
  double x[5] = {8.0, 0, 0, 0, 0};
  int nan_at = -1, worse_at = -1, fail_at = -1, zero_v = 0;
  int steps = 0, cycle = 0, norms_calls = 0;
  bool from_prime = false;
  double forced_sr = -1.0, forced_sv = -1.0;
  int step(int src, int dst, int t, double* l) {
    if (t != steps) return 99;  // the driver names the number of steps before this one
    if (t == fail_at) return 7;
    if (src == dst || src < 0 || src > 4 || dst < 0 || dst > 4) return 98;
    *l = -x[src] * x[src];
    if (from_prime) {
      if (cycle == nan_at) *l = NaN;
      if (cycle == worse_at) *l = -1e300;
      from_prime = false;
      cycle++;
    }
    x[dst] = zero_v ? x[src] : 0.5 * x[src];
    steps++;
    return 0;
  }
  int norms(int s0, int s1, int s2, double* sr, double* sv) {
    const double r = x[s1] - x[s0], v = (x[s2] - x[s1]) - r;
    *sr = forced_sr >= 0 ? forced_sr : r * r;
    *sv = forced_sv >= 0 ? forced_sv : v * v;
    norms_calls++;
    return 0;
  }
  int extrapolate(int s0, int s1, int s2, int dst, double alpha) {
    if (dst == s0 || dst == s1 || dst == s2) return 97;
    const double r = x[s1] - x[s0], v = (x[s2] - x[s1]) - r;
    x[dst] = std::fma(alpha * alpha, v, std::fma(-2.0 * alpha, r, x[s0]));
    from_prime = true;
    return 0;
  }
};

struct Run {
  squarem_result res;
  std::vector<double> ll, alpha;
  std::vector<int32_t> acc;
  int rc = 0;
};

static Run drive(Toy& toy, int max_iter, double tol, double a_max = 4.0) {
  Run r;
  // exact sizes, on the heap
  double* ll = new double[(size_t)max_iter];
  double* al = new double[(size_t)(max_iter / 3)];
  int32_t* ac = new int32_t[(size_t)(max_iter / 3)];
  r.rc = squarem_drive(toy, max_iter, tol, a_max, ll, al, ac, &r.res);
  if (r.rc == 0) {
    r.ll.assign(ll, ll + r.res.n_iter);
    r.alpha.assign(al, al + r.res.n_cycles);
    r.acc.assign(ac, ac + r.res.n_cycles);
  }
  delete[] ll;
  delete[] al;
  delete[] ac;
  return r;
}

int main() {
  bool lim = false;
  // alpha: inside, clipped on both sides, sv = 0, values that are not finite
  CHECK(squarem_alpha(9.0, 1.0, 4.0, &lim) == -3.0 && !lim);
  CHECK(squarem_alpha(100.0, 1.0, 4.0, &lim) == -4.0 && lim);
  CHECK(squarem_alpha(16.0, 1.0, 4.0, &lim) == -4.0 && !lim);  // exactly at the limit is not a clip
  CHECK(squarem_alpha(1.0, 4.0, 4.0, &lim) == -1.0 && !lim);
  CHECK(squarem_alpha(1.0, 0.0, 4.0, &lim) == -1.0 && !lim);
  CHECK(squarem_alpha(0.0, 0.0, 4.0, &lim) == -1.0 && !lim);
  CHECK(squarem_alpha(Inf, 1.0, 4.0, &lim) == -1.0 && !lim);
  CHECK(squarem_alpha(NaN, 1.0, 4.0, &lim) == -1.0 && !lim);
  CHECK(squarem_alpha(1.0, NaN, 4.0, &lim) == -1.0 && !lim);
  CHECK(squarem_alpha(-1.0, 1.0, 4.0, &lim) == -1.0 && !lim);
  CHECK(squarem_alpha(2.0, 1.0, 1.0, &lim) == -1.0 && lim);  // a_max = 1: a plain step
  printf("alpha ok\n");
  // accept
  CHECK(squarem_accept(-1.0, -1.0) && squarem_accept(-1.0, -2.0) && !squarem_accept(-2.0, -1.0));
  CHECK(!squarem_accept(NaN, -1.0) && !squarem_accept(-1.0, NaN) && !squarem_accept(Inf, -1.0) && !squarem_accept(-Inf, -1.0));
  printf("accept ok\n");
  // the limit: growth only at the clip, shrink down to 1 and no further
  CHECK(squarem_next_limit(4.0, true, true) == 16.0 && squarem_next_limit(16.0, true, true) == 64.0);
  CHECK(squarem_next_limit(4.0, true, false) == 4.0);
  CHECK(squarem_next_limit(64.0, false, true) == 16.0 && squarem_next_limit(4.0, false, false) == 1.0);
  CHECK(squarem_next_limit(2.0, false, false) == 1.0 && squarem_next_limit(1.0, false, false) == 1.0);
  printf("limit ok\n");

  // max_iter = 0: nothing runs, the start is returned
  {
    Toy t;
    Run r = drive(t, 0, 0.0);
    CHECK(r.rc == 0 && r.res.n_iter == 0 && r.res.last == 0 && !r.res.converged && r.res.n_cycles == 0 && t.steps == 0);
  }
  // max_iter landing on each of the three steps of the first and of the second cycle.  x0 = 8: theta1 = 4, theta2 = 2,
  // alpha = -2, theta' = 0, theta'' = 0, accepted; second cycle from 0: l(theta1) - l(theta0) = 0 < tol only if tol > 0
  {
    const double want_x[7] = {8, 4, 2, 0, 0, 0, 0};
    const int want_cycles[7] = {0, 0, 0, 1, 1, 1, 2};
    for (int mi = 1; mi <= 6; mi++) {
      Toy t;
      Run r = drive(t, mi, 0.0);
      CHECK(r.rc == 0 && r.res.n_iter == mi && t.steps == mi && !r.res.converged);
      CHECK(t.x[r.res.last] == want_x[mi]);
      CHECK(r.res.n_cycles == want_cycles[mi] && r.res.n_rejected == 0 && (int)r.alpha.size() == want_cycles[mi]);
      CHECK(r.ll[0] == -64.0 && (mi < 2 || r.ll[1] == -16.0) && (mi < 3 || (r.ll[2] == 0.0 && r.alpha[0] == -2.0 && r.acc[0] == 1)));
      printf("max_iter %d ok\n", mi);
    }
  }
  // the stop rule: the second cycle starts at the fixed point and gains 0 < tol; the state one step past the pair is returned
  {
    Toy t;
    Run r = drive(t, 100, 1e-4);
    CHECK(r.rc == 0 && r.res.converged == 1 && r.res.n_iter == 5 && r.res.n_cycles == 1 && t.x[r.res.last] == 0.0);
    printf("stop rule ok\n");
  }
  // the stop rule holds at max_iter too
  {
    Toy t;
    t.zero_v = 1;  // a map that does not move: l(theta1) - l(theta0) = 0
    Run r = drive(t, 2, 1e-4);
    CHECK(r.rc == 0 && r.res.converged == 1 && r.res.n_iter == 2 && r.res.n_cycles == 0 && t.norms_calls == 0);
  }
  // sv = 0 with tol = 0: a map that does not move never stops by the rule (0 < 0 is false); alpha = -1 every cycle
  {
    Toy t;
    t.zero_v = 1;
    Run r = drive(t, 9, 0.0);
    CHECK(r.rc == 0 && !r.res.converged && r.res.n_iter == 9 && r.res.n_cycles == 3 && r.res.n_rejected == 0);
    for (double a : r.alpha) CHECK(a == -1.0);
    CHECK(r.res.a_max == 4.0 && t.x[r.res.last] == 8.0);
    printf("sv = 0 ok\n");
  }
  // a NaN l(theta') rejects: the next cycle starts from theta2 and the limit shrinks 4 -> 1; max_iter at the end of that cycle
  // returns theta2, not theta''
  {
    Toy t;
    t.nan_at = 0;
    Run r = drive(t, 3, 0.0);
    CHECK(r.rc == 0 && r.res.n_cycles == 1 && r.res.n_rejected == 1 && r.acc[0] == 0 && r.res.a_max == 1.0);
    CHECK(t.x[r.res.last] == 2.0 && std::isnan(r.ll[2]));
    Toy u;
    u.nan_at = 0;
    r = drive(u, 4, 0.0);  // and the fourth step is applied to theta2
    CHECK(r.rc == 0 && r.res.n_iter == 4 && r.ll[3] == -4.0 && u.x[r.res.last] == 1.0);
    printf("NaN ok\n");
  }
  // growth: sums that clip alpha at the limit in accepted cycles widen it 4 -> 16 -> 64; the recorded alphas are the clipped ones
  {
    Toy t;
    t.forced_sr = 1e6;
    t.forced_sv = 1.0;
    t.x[0] = 0.0;  // the fixed point: every theta' equals it whatever alpha, so every cycle is accepted
    Run r = drive(t, 9, 0.0);
    CHECK(r.rc == 0 && r.res.n_cycles == 3 && r.res.n_rejected == 0 && r.res.a_max == 256.0);
    CHECK(r.alpha[0] == -4.0 && r.alpha[1] == -16.0 && r.alpha[2] == -64.0);
    printf("growth ok\n");
  }
  // shrink: three rejected cycles from a limit of 64: 16, 4, 1, and it stays at 1
  {
    Toy t;
    t.worse_at = 0;
    Run r = drive(t, 3, 0.0, 64.0);
    CHECK(r.rc == 0 && r.res.n_rejected == 1 && r.res.a_max == 16.0);
    double lim4 = 64.0;
    for (int c = 0; c < 5; c++) lim4 = squarem_next_limit(lim4, false, c % 2 == 0);
    CHECK(lim4 == 1.0);
    printf("shrink ok\n");
  }
  // an error from a step ends the drive with that code
  for (int at = 0; at < 3; at++) {
    Toy t;
    t.fail_at = at;
    Run r = drive(t, 6, 0.0);
    CHECK(r.rc == 7 && t.steps == at);
  }
  printf("ok squarem\n");
  return 0;
}
