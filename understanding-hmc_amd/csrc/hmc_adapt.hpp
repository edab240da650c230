// hmc_adapt.hpp — per-chain step-size adaptation during warm-up: the Nesterov dual averaging of
// Hoffman & Gelman 2014, section 3.2, on a multiplier s of the caller's step (the effective step of
// dimension d is s dt_d; the diagonal minv is untouched).  Written once for the ADAPT instances of
// the GLM kernels (hmc_logit.hip, hmc_glm_nuts.hip), which hold one AdaptState per lane (identical in
// a chain's four lanes), and for the host: adapt_host.cpp prints the rule as compiled here and
// tests/test_adapt_host.py compares the printout with a NumPy restatement.
//
// State of a chain, HMC_ADAPT_STRIDE doubles in the caller's array (include/hmc.h: hmc_adapt):
//   0 log_s   1 log_s_bar   2 H_bar   3 m   4 mu   5 sum_alpha_adapt   6 sum_alpha_after   7 n_after
// After an adapting iteration with acceptance statistic alpha:
//   m += 1;  H_bar = (1 - 1/(m + t0)) H_bar + (delta - alpha)/(m + t0)
//   log_s = clamp(mu - sqrt(m)/gamma H_bar, mu -+ 20 ln 2);  eta = m^-kappa
//   log_s_bar = eta log_s + (1 - eta) log_s_bar
// mu = log(s0): the caller's step is the shrinkage point (Stan takes log(10 s0); see DESIGN.md 3.12
// for what that does to exp(z) of the Poisson family).
#pragma once
#include <math.h>

#include "hmc.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define HMC_ADAPT_FN __host__ __device__ __forceinline__
#else
#define HMC_ADAPT_FN inline
#endif

namespace hmc {

struct AdaptParams {
  double delta, gamma, t0, kappa;
};

struct AdaptState {
  double log_s, log_s_bar, H_bar, m, mu, sum_adapt, sum_after, n_after;
};

constexpr double kAdaptClamp = 20.0 * 0.693147180559945309417;   // 20 ln 2: s within 2^-20 .. 2^20 of s0

HMC_ADAPT_FN AdaptState adapt_initial(double s0) {
  const double l = log(s0);
  return AdaptState{l, l, 0.0, 0.0, l, 0.0, 0.0, 0.0};
}

HMC_ADAPT_FN AdaptState adapt_load(const double* row) {
  return AdaptState{row[0], row[1], row[2], row[3], row[4], row[5], row[6], row[7]};
}

HMC_ADAPT_FN void adapt_store(double* row, const AdaptState& a) {
  row[0] = a.log_s;
  row[1] = a.log_s_bar;
  row[2] = a.H_bar;
  row[3] = a.m;
  row[4] = a.mu;
  row[5] = a.sum_adapt;
  row[6] = a.sum_after;
  row[7] = a.n_after;
}

// One point's (NUTS) or one iteration's (Random) acceptance statistic from dE = E_point - E_init:
// min(1, exp(-dE)); 0 for an energy, or a difference, that is not finite.
HMC_ADAPT_FN double adapt_alpha(double dE, double E_point) {
  if (!(fabs(E_point) <= 1.79769313486231570815e308) || dE != dE) return 0.0;
  return dE <= 0.0 ? 1.0 : exp(-dE);
}

// End of iteration `it` with acceptance statistic alpha: the update above for it < adapt_end, the
// two sums of the iterations after it otherwise.
HMC_ADAPT_FN void adapt_iteration(AdaptState& a, const AdaptParams& p, bool adapting, double alpha) {
  if (!adapting) {
    a.sum_after += alpha;
    a.n_after += 1.0;
    return;
  }
  a.sum_adapt += alpha;
  a.m += 1.0;
  a.H_bar = (1.0 - 1.0 / (a.m + p.t0)) * a.H_bar + (p.delta - alpha) / (a.m + p.t0);
  double ls = a.mu - sqrt(a.m) / p.gamma * a.H_bar;
  ls = ls < a.mu - kAdaptClamp ? a.mu - kAdaptClamp : ls;
  ls = ls > a.mu + kAdaptClamp ? a.mu + kAdaptClamp : ls;
  a.log_s = ls;
  const double eta = pow(a.m, -p.kappa);
  a.log_s_bar = eta * ls + (1.0 - eta) * a.log_s_bar;
}

// The multiplier an iteration runs at: exp(log_s) while adapting, the averaged exp(log_s_bar) after
// (exp(log_s) when nothing has adapted: log_s_bar then has no meaning of its own).  exp(0) = 1
// exactly, so a chain at s0 = 1 that never adapts multiplies by exactly 1.
HMC_ADAPT_FN double adapt_scale(const AdaptState& a, bool adapting) {
  return exp((adapting || a.m == 0.0) ? a.log_s : a.log_s_bar);
}

}  // namespace hmc

#undef HMC_ADAPT_FN
