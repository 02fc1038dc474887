// host_squarem.h -- the host side of include/tpg.h "admixture, accelerated": the step length, the step limit, the accept /
// reject rule and the cycle driver.  Host only, no HIP: admix.hip hands the driver the device work as callbacks, and
// tests/host/squarem_san.cpp hands it a toy map, so the whole state machine runs stand-alone under the host sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <utility>

// alpha = -sqrt(sr / sv) (a correctly rounded quotient, then a correctly rounded root); sv = 0 or a value that is not finite:
// -1; then clipped into [-a_max, -1].  *at_limit = the clip at -a_max took hold (what makes an accepted cycle grow a_max).
inline double squarem_alpha(double sr, double sv, double a_max, bool* at_limit) {
  double a = -std::sqrt(sr / sv);
  if (sv == 0.0 || !std::isfinite(a)) a = -1.0;
  *at_limit = a < -a_max;
  if (*at_limit) a = -a_max;
  if (a > -1.0) a = -1.0;
  return a;
}

// l(theta') is finite and not below l(theta1): false for a NaN on either side
inline bool squarem_accept(double l_prime, double l_one) { return std::isfinite(l_prime) && l_prime >= l_one; }

// the step limit after a cycle: an accepted cycle whose alpha sat at the limit widens it fourfold; a rejected one narrows it
// fourfold, never below 1 (alpha = -1 is theta2 itself: a plain step)
inline double squarem_next_limit(double a_max, bool accepted, bool at_limit) {
  if (accepted) return at_limit ? 4.0 * a_max : a_max;
  const double a = a_max / 4.0;
  return a < 1.0 ? 1.0 : a;
}

struct squarem_result {
  int32_t n_iter = 0, converged = 0, n_cycles = 0, n_rejected = 0;
  int last = 0;        // the slot of the state to return: inside a cycle the last one an EM step produced, after a whole
                       // cycle the state the next one would start from (theta2 after a rejection); the start if no step ran
  double a_max = 4.0;  // the limit the next cycle would have used
};

// The cycle driver over five state slots 0 .. 4; the start is in slot 0.  Ops has
//   int step(int src, int dst, int t, double* l)     slot dst = E(slot src); *l = l(slot src); t = the EM steps before this one
//   int norms(int s0, int s1, int s2, double* sr, double* sv)
//   int extrapolate(int s0, int s1, int s2, int dst, double alpha)     slot dst = the projected theta'
// each returning 0 or an error code, which ends the drive and is returned.  ll has room for max_iter doubles and receives l of
// every state a step was applied to, in order; alpha / accepted have room for max_iter / 3 entries, or are null.
template <class Ops>
int squarem_drive(Ops& ops, int max_iter, double tol, double a_max0, double* ll, double* alpha, int32_t* accepted,
                  squarem_result* out) {
  squarem_result res;
  res.a_max = a_max0;
  int s[5] = {0, 1, 2, 3, 4};  // the slots of theta0, theta1, theta2, theta', theta''
  int t = 0;
  while (t < max_iter) {
    if (int rc = ops.step(s[0], s[1], t, &ll[t])) return rc;
    const double l0 = ll[t++];
    res.last = s[1];
    if (t == max_iter) break;
    if (int rc = ops.step(s[1], s[2], t, &ll[t])) return rc;
    const double l1 = ll[t++];
    res.last = s[2];
    if (l1 - l0 < tol) {  // a plain EM step gained less than tol: the state one step past the compared pair
      res.converged = 1;
      break;
    }
    if (t == max_iter) break;
    double sr = 0.0, sv = 0.0;
    if (int rc = ops.norms(s[0], s[1], s[2], &sr, &sv)) return rc;
    bool at_limit = false;
    const double a = squarem_alpha(sr, sv, res.a_max, &at_limit);
    if (int rc = ops.extrapolate(s[0], s[1], s[2], s[3], a)) return rc;
    if (int rc = ops.step(s[3], s[4], t, &ll[t])) return rc;
    const double lp = ll[t++];
    res.last = s[4];
    const bool ok = squarem_accept(lp, l1);
    if (alpha) alpha[res.n_cycles] = a;
    if (accepted) accepted[res.n_cycles] = ok ? 1 : 0;
    res.n_cycles++;
    if (!ok) res.n_rejected++;
    res.a_max = squarem_next_limit(res.a_max, ok, at_limit);
    std::swap(s[0], ok ? s[4] : s[2]);  // the next cycle starts from theta'' (accepted) or from theta2 (rejected)
    res.last = s[0];                    // and that state is the one to return if max_iter ends the run here
  }
  res.n_iter = t;
  *out = res;
  return 0;
}
