// Step arithmetic of the scaled Newton-Schulz iterations of the matrix square root (nk_sqrtm.hip): host only, no HIP
// include, so that a plain C++17 compiler builds it (tests/sqrt_schedule_main.cpp).
//
// A step  T = s (3 I - s^2 M) / 2  maps every eigenvalue x of M to p(s^2 x), p(x) = x (3 - x)^2 / 4.  The iterations track an
// interval [a, b] that is meant to hold the spectrum of M and choose s^2 from it; s^2 and sqrt(s^2) become kernel
// coefficients, so every expression below keeps its order of operations: one different rounding changes result bits.
#pragma once
#include <cmath>

namespace nk {

// the map a step applies to the eigenvalues of M
inline double ns_p3(double x) { return x * (3.0 - x) * (3.0 - x) * 0.25; }

// Lower end a of the spectrum interval [a, 1] of M_0 = P / c (c = ||P||_inf bounds the largest eigenvalue) from the
// Frobenius norm and the trace of M_0: the mean of the eigenvalues other than the dominant one -- an OVER-estimate of the
// smallest eigenvalue, which is the safe side: the scaled steps stay inside (0, 3) for every eigenvalue <= b, eigenvalues
// below a still grow by the same factor, and the scaling fades to 1 as a -> 1 (plain Newton-Schulz finish).
inline double ns_interval_estimate(double fro, double tr, int m) {
  double a_lo;
  const double lam1 = fro < 1.0 ? fro : 1.0;
  if (m > 1 && tr > lam1) a_lo = (tr - lam1) / (m - 1);
  else a_lo = tr / m * 1e-2;
  if (!(a_lo > 0.0) || !std::isfinite(a_lo)) a_lo = 1e-12;
  if (a_lo > 1.0) a_lo = 1.0;
  return a_lo;
}

// s^2 = 3 / (a + sqrt(a b) + b) equalises p(s^2 a) = p(s^2 b); s -> 1 as a -> b = 1
inline double ns_scale(double a, double b) { return 3.0 / (a + std::sqrt(a * b) + b); }

// one step of the interval recurrence under the scaling s2
inline void ns_advance(double s2, double& a, double& b) {
  const double xa = s2 * a, xb = s2 * b;
  const double lo = ns_p3(xa) < ns_p3(xb) ? ns_p3(xa) : ns_p3(xb);
  b = (xa <= 1.0 && xb >= 1.0) ? 1.0 : (ns_p3(xa) > ns_p3(xb) ? ns_p3(xa) : ns_p3(xb));
  a = lo < b ? lo : b;
}

// Schedule of the iteration that is queued without host round trips: the scale s2[k] of every step, whether step k's
// residual is worth looking at (check[k]: the schedule's interval says M_k may have converged) and the latest step kmax at
// which the iteration can converge.
constexpr int NS_MAX_STEPS = 100;
struct NsSchedule {
  int kmax = 0;
  double s2[128];
  bool check[128];
};
// estimate: ns_interval_estimate's a; true_lower: a rigorous lower bound of the smallest eigenvalue of M_0 (the true
// interval is [true_lower, 1]), taken no larger than the estimate.
inline NsSchedule ns_queued_schedule(double estimate, double true_lower) {
  NsSchedule sch;
  double ta = true_lower, tb = 1.0;
  if (ta > estimate) ta = estimate;
  // Interval the scaling schedule is built for.  Any lower end is safe (the scaled step keeps every eigenvalue <= b
  // inside (0, 3)); it only decides how long the steps stay aggressively scaled.  The mean-of-the-bulk over-estimate
  // stops scaling after ~4 steps and leaves the smallest eigenvalues to the unscaled 2.25x growth, the rigorous
  // bound keeps scaling for steps nobody needs: a weighted geometric mean (0.8 / 0.2) is used.  Steps at C4, m = 2000,
  // lengthscales 5 / 10 / 20 / 40 / 80: 7 / 9 / 10 / 13 / 16 against 6 / 10 / 13 / 15 / 18 with the over-estimate alone
  // and 8 / 12 / 12 / 13 / - with equal weights.
  const double a_sched = std::pow(estimate, 0.8) * std::pow(ta, 0.2);
  double a = a_sched, b = 1.0;
  int kconv = -1;
  for (int k = 0; k < NS_MAX_STEPS; ++k) {
    if (kconv < 0 && ta >= 1.0 - 1e-9 && tb <= 1.0 + 1e-9) kconv = k;  // M_k is within the 1e-7 residual bar
    sch.check[k] = a >= 0.5;
    const double s2 = ns_scale(a, b);
    sch.s2[k] = s2;
    ns_advance(s2, a, b);
    ns_advance(s2, ta, tb);
    if (kconv >= 0 && k >= kconv + 1) { sch.kmax = k + 1; break; }  // one spare step beyond the predicted last one
  }
  if (sch.kmax == 0) sch.kmax = NS_MAX_STEPS;
  return sch;
}

}  // namespace nk
